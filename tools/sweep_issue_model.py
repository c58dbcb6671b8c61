"""Static issue model of the structured sweep's layer loop (sweep_h8_kernel<0, true, true, 0, false>,
the headline kernel: the CHECKED = false instantiation a valid mesh runs; --kernel
sweep_h8_kernelILi0ELb1ELb1ELi0ELb1E is the checked one, FCG_SWEEP_CHECKED=1 or a mesh the
create-time geometry pass rejects): the instructions of one layer per wave from the kernel's ISA, classified by
issue resource and attributed to source lines, against the counters' dynamic counts.

The ISA comes from a device-only compile with line tables, e.g.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -I4c_amd/csrc --offload-device-only -S \
      -gline-tables-only -o sweep.s 4c_amd/csrc/fcg_sweep.hip

usage: sweep_issue_model.py kernel.s [pmc_summary.txt [layers_per_wave]] [--source fcg_sweep.hip]
                            [--kernel REGEX] [--lines N]

The layer loop is the outermost loop of the kernel (the two element visits are unrolled inside
it; small depth-2 loops, such as the wave reduction of the error report, are counted once).
Instructions are split into
  executed  what a wave issues every layer on a valid mesh (every exec-masked branch counted as
            taken: stage-A and emit paths that some waves skip are counted in full), and
  cold      code inlined from a call site that valid meshes never reach: the NEG = true
            instantiation of sweep_visit (elements with fac < 0 at a Gauss point) and the error
            report of stage A.  A call site is cold when its source line matches one of
            COLD_PATTERNS; an instruction is cold when its inline chain (the "@[ file:line ]"
            frames of its .loc comment) passes through such a line.  Instructions without a
            source line take the colour of the majority of their basic block.
The cold instructions are static only: they cost instruction-cache space and a branch around
them, not issue slots.

Issue costs per wave instruction on gfx950 (wave64 on a 16-lane SIMD): VALU 4 cycles (FP64 FMA
at the measured 62.7 TF/s: ~5), LDS 4 cycles of LDS-pipe issue (b64) / 8 (b128, one per 2 cycles
of 128 B/cycle), VMEM 4 cycles of TA issue (64 lanes x 8 B stores: 8 cycles at 64 B/cycle), SALU 1.
"""
import argparse
import collections
import os
import re

COLD_PATTERNS = [r"sweep_visit<KIN,\s*true", r"atomicM(ax|in)\(&A\.err"]

ap = argparse.ArgumentParser()
ap.add_argument("isa")
ap.add_argument("pmc", nargs="?")
ap.add_argument("layers", nargs="?", type=float, default=34.67)
ap.add_argument("--source", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                                 "4c_amd", "csrc", "fcg_sweep.hip"))
ap.add_argument("--kernel", default=r"sweep_h8_kernelILi0ELb1ELb1ELi0ELb0E")
ap.add_argument("--lines", type=int, default=24, help="source lines listed")
args = ap.parse_args()

s = open(args.isa).read().split("\n")
src = open(args.source).read().split("\n")
src_name = os.path.basename(args.source)
cold_lines = {i + 1 for i, l in enumerate(src) if any(re.search(p, l) for p in COLD_PATTERNS)}

st = next(i for i, l in enumerate(s) if re.match(r"^_Z\S*" + args.kernel + r"\S*:", l))
en = next(i for i in range(st, len(s)) if s[i].startswith(".Lfunc_end"))
body = s[st:en]

# the layer loop: the depth-1 loop with the longest body
hdrs = [i for i, l in enumerate(body) if re.match(r"^\.LBB\S+:\s*; =>This (Inner )?Loop Header: Depth=1", l)]
if not hdrs:
    raise SystemExit("no depth-1 loop in the kernel: is this the sweep's ISA?")


def loop_end(h):
    name = body[h].split(":")[0]
    backs = [i for i, l in enumerate(body) if i > h and re.search(r"s_c?branch\S*\s+" + re.escape(name) + r"\s*$", l)]
    return max(backs) if backs else h


outer = max(hdrs, key=lambda h: loop_end(h) - h)
back = loop_end(outer)


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if re.match(r"v_(fma|fmac|mul|add|sub|fma_mix|pk_fma|pk_mul|pk_add)_f64", op):
        return "valu_fp64"
    if "_dpp" in op:
        return "valu_dpp"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("ds_"):
        return "lds_b128" if "b128" in op else "lds"
    if op.startswith(("global_load", "buffer_load", "flat_load", "global_atomic")):
        return "vmem_load"
    if op.startswith(("global_store", "buffer_store", "flat_store")):
        return "vmem_store"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_"):
        return "salu"
    return "other"


# walk the loop: (basic block, class, opcode, text, source line or None, cold by chain or None)
insts = []
block = 0
line, chain_cold = None, None
for l in body[outer:back + 1]:
    t = l.strip()
    if re.match(r"^(\.LBB\S+:|; %bb\.)", t):
        block += 1
        continue
    m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", t)
    if m:
        frames = re.findall(r"(\S+):(\d+):\d+", t.split(";", 1)[1] if ";" in t else "")
        mine = [(f, int(n)) for f, n in frames if os.path.basename(f) == src_name]
        inner = frames[0] if frames else None
        if inner and int(inner[1]) > 0:
            # the innermost frame of the sweep's own file names the line the work belongs to
            line = (src_name, mine[0][1]) if mine else (os.path.basename(inner[0]), int(inner[1]))
            chain_cold = any(n in cold_lines for _, n in mine)
        else:
            line, chain_cold = None, None
        continue
    if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
        continue
    op = t.split()[0]
    insts.append([block, classify(op), op, t, line, chain_cold])
# instructions without a source line: the majority colour of their block
by_block = collections.defaultdict(list)
for it in insts:
    by_block[it[0]].append(it)
for blk in by_block.values():
    known = [it[5] for it in blk if it[5] is not None]
    major = bool(known) and sum(known) * 2 > len(known)
    for it in blk:
        if it[5] is None:
            it[5] = major

cost = {"valu_fp64": 4, "valu_other": 4, "valu_dpp": 4, "lds": 4, "lds_b128": 8, "vmem_load": 4,
        "vmem_store": 8, "salu": 1, "waitcnt": 1, "branch": 1, "barrier": 1, "mfma": 16, "other": 1}
stat, cold = collections.Counter(), collections.Counter()
for _, k, _, _, _, c in insts:
    stat[k] += 1
    if c:
        cold[k] += 1
print(f"layer loop: ISA lines {outer}-{back} of the kernel, {block} basic blocks")
print(f"cold call sites ({src_name}): lines {sorted(cold_lines)}")
print("instructions per layer per wave (every exec-masked branch taken):")
print(f"  {'class':12s} {'static':>7s} {'cold':>6s} {'executed':>9s}  ~issue cycles (executed)")
for k in sorted(stat, key=lambda k: -stat[k]):
    ex = stat[k] - cold[k]
    print(f"  {k:12s} {stat[k]:7d} {cold[k]:6d} {ex:9d}  {ex * cost[k]:7d}")
valu = [k for k in stat if k.startswith("valu")]
for name, cnt in (("static", stat), ("executed", stat - cold), ("cold", cold)):
    tot = sum(cnt[k] for k in valu)
    fp = cnt["valu_fp64"]
    if tot:
        print(f"  VALU {name:8s} {tot:5d}: FP64 {fp}, other {tot - fp} ({100 * (tot - fp) / tot:.1f} % non-FP64)")
ex_i = [it for it in insts if not it[5]]
w = collections.Counter()
for it in ex_i:
    if it[1] == "waitcnt":
        for c in ("lgkmcnt", "vmcnt", "expcnt"):
            if c in it[3]:
                w[c] += 1
print(f"  executed s_waitcnt {sum(1 for it in ex_i if it[1] == 'waitcnt')} "
      f"(naming lgkmcnt {w['lgkmcnt']}, vmcnt {w['vmcnt']}), "
      f"s_cbranch_execz {sum(1 for it in ex_i if it[2].startswith('s_cbranch_exec'))}, "
      f"other branches {sum(1 for it in ex_i if it[1] == 'branch' and not it[2].startswith('s_cbranch_exec'))}")


def line_name(ln):
    return "(no source line)" if ln is None else f"{ln[0]}:{ln[1]}"


def text_of(ln):
    if ln is None or ln[0] != src_name or not (0 < ln[1] <= len(src)):
        return ""
    return src[ln[1] - 1].strip()[:70]


per = collections.defaultdict(collections.Counter)
for it in ex_i:
    if it[1].startswith("valu"):
        per[it[4]][it[1]] += 1
        if it[1] != "valu_fp64":
            per[it[4]]["op:" + re.sub(r"_e(32|64)$", "", it[2])] += 1
print(f"executed VALU per source line (top {args.lines} by non-FP64 count):")
print(f"  {'line':28s} {'fp64':>5s} {'dpp':>4s} {'other':>6s}  top opcodes | source")
rank = sorted(per, key=lambda ln: -(per[ln]["valu_other"] + per[ln]["valu_dpp"]))
for ln in rank[:args.lines]:
    c = per[ln]
    ops = sorted(((o[3:], n) for o, n in c.items() if o.startswith("op:")), key=lambda x: -x[1])[:3]
    print(f"  {line_name(ln):28s} {c['valu_fp64']:5d} {c['valu_dpp']:4d} {c['valu_other']:6d}  "
          + ", ".join(f"{o} {n}" for o, n in ops) + " | " + text_of(ln))
lw = collections.Counter(it[4] for it in ex_i if it[1] == "waitcnt" and "lgkmcnt" in it[3])
print("executed s_waitcnt lgkmcnt per source line (top 16):")
for ln, n in lw.most_common(16):
    print(f"  {line_name(ln):28s} {n:4d}  {text_of(ln)}")
ops = collections.Counter(re.sub(r"_e(32|64)$", "", it[2]) for it in ex_i if it[1] in ("valu_other", "valu_dpp"))
print("top executed non-FP64 VALU opcodes:")
for op, n in ops.most_common(16):
    print(f"  {op:28s} {n}")
cops = collections.Counter(re.sub(r"_e(32|64)$", "", it[2]) for it in insts if it[5] and it[1] in ("valu_other", "valu_dpp"))
print("top cold (static only) non-FP64 VALU opcodes:")
for op, n in cops.most_common(6):
    print(f"  {op:28s} {n}")

if args.pmc:
    pmc = {}
    for l in open(args.pmc):
        m = re.match(r"^(\S+)\s+([0-9.e+]+)\s+\(n=", l)
        if m:
            pmc[m.group(1)] = float(m.group(2))
    waves = pmc["SQ_WAVES"]
    # 1M box: 625 tiles in x-y, 101 node planes in 3 z-segments of 34, 34, 33 planes, each with one
    # layer more than planes: 34.67 layers per workgroup on average
    layers = args.layers
    per_w = lambda k: pmc[k] / waves / layers
    print(f"dynamic (counters, per wave per layer, {layers} layers per wave): VALU {per_w('SQ_INSTS_VALU'):.0f}"
          f" (FP64 FMA {per_w('SQ_INSTS_VALU_FMA_F64'):.0f}, MUL {per_w('SQ_INSTS_VALU_MUL_F64'):.0f},"
          f" ADD {per_w('SQ_INSTS_VALU_ADD_F64'):.0f}), LDS {per_w('SQ_INSTS_LDS'):.0f},"
          f" VMEM rd {per_w('SQ_INSTS_VMEM_RD'):.0f} wr {per_w('SQ_INSTS_VMEM_WR'):.0f}, SALU {per_w('SQ_INSTS_SALU'):.0f}")
    fp64 = pmc["SQ_INSTS_VALU_FMA_F64"] + pmc["SQ_INSTS_VALU_MUL_F64"] + pmc["SQ_INSTS_VALU_ADD_F64"]
    print(f"dynamic non-FP64 VALU share {100 * (1 - fp64 / pmc['SQ_INSTS_VALU']):.1f} %")
    print(f"wave cycles per layer {pmc['SQ_WAVE_CYCLES'] / waves / layers:.0f} (counter units); VALU active {pmc['SQ_ACTIVE_INST_VALU'] / pmc['SQ_WAVE_CYCLES']:.3f},"
          f" LDS active {pmc['SQ_ACTIVE_INST_LDS'] / pmc['SQ_WAVE_CYCLES']:.3f}, waiting {pmc['SQ_WAIT_ANY'] / pmc['SQ_WAVE_CYCLES']:.3f},"
          f" issue-waiting {pmc['SQ_WAIT_INST_ANY'] / pmc['SQ_WAVE_CYCLES']:.3f}")
