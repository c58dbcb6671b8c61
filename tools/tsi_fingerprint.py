#!/usr/bin/env python3
"""SHA-256 fingerprints of what the TSI context computes, for comparing two builds bit by bit.

    tools/tsi_fingerprint.py [--root CHECKOUT] > fingerprint.txt          (one MI355X, a few seconds)
    tools/tsi_fingerprint.py --compare PARENT_A.txt PARENT_B.txt NEW.txt   (no GPU)

The first form imports 4c_amd from CHECKOUT (default: this repository) and prints one line per
(case, item): the SHA-256 of the raw bytes of every output, from seeded numpy inputs, of
  evaluate_device with TSI_ALL, OVERWRITE and ACCUMULATE (onto a seeded start), on hex8 (4, 3, 3),
  hex27 (2, 2, 2) and rank 1 of 2 of hex8 (4, 3, 3);
  capacity, uniform and with a per-element table, both modes, on the same three meshes;
  ost_combine: tangent only, residual only, both (hex8 (4, 3, 3));
  block_apply and one gmres_solve (solution, iteration count) on hex8 (4, 3, 3);
  evaluate_fused on the structured hex8 (6, 5, 4), FCG_TSI_SPLIT unset and = 0.
The second form takes two runs of the parent and one of the new build: lines on which the parent's
two runs disagree are listed and left out (none of the evaluate, capacity or ost lines may be among
them: the library documents those as bitwise reproducible), every other line must be the parent's.
Exit 1 otherwise.
"""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

E, NU, ALPHA, T0, COND, DT, CAPA, THETA = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.05, 3.6, 0.66

MESHES = {
    "h8_433": dict(ct="HEX8", iv=(4, 3, 3), jitter=0.1),
    "h27_222": dict(ct="HEX27", iv=(2, 2, 2), jitter=0.02),
    "h8_433 rank 1 of 2": dict(ct="HEX8", iv=(4, 3, 3), jitter=0.1, rank=1, nranks=2),
}
REPRODUCIBLE = ("evaluate", "capacity", "ost")  # documented as bitwise reproducible


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fingerprint(root):
    sys.path.insert(0, root)
    import torch

    fcg = importlib.import_module("4c_amd").fcg
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = []

    def blocks(rng, mesh, g, zero):
        sizes = {"fs": mesh.n_rows, "Kst": g.nnz_st, "fT": g.n_rows_t, "Ktt": g.nnz_tt, "Kts": g.nnz_ts}
        return {k: t(np.zeros(n) if zero else rng.standard_normal(n)) for k, n in sizes.items()}

    def add(tag, item, *tensors):
        torch.cuda.synchronize()
        out.append((tag, item, sha(*[a.cpu().numpy() if hasattr(a, "cpu") else a for a in tensors])))

    for name, spec in MESHES.items():
        ct = getattr(fcg, spec["ct"])
        mesh = fcg.BoxMesh(ct, spec["iv"], jitter=spec["jitter"], seed=4, rank=spec.get("rank", 0),
                           nranks=spec.get("nranks", 1))
        tev = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND)
        g = tev.graph
        rng = np.random.default_rng(31)
        v = t(1e-1 * rng.standard_normal(mesh.n_cols))
        T = t(T0 + 50.0 * rng.standard_normal(g.n_cols_t))
        for mode, mname in ((fcg.OVERWRITE, "overwrite"), (fcg.ACCUMULATE, "accumulate")):
            o = blocks(rng, mesh, g, zero=False)
            tev.evaluate_device(fcg.TSI_ALL, mode, v, T, 1.0, 1.0 / DT, **o)
            for k, a in o.items():
                add(f"evaluate {name} {mname}", k, a)
        ele_capa = CAPA * (1.0 + rng.random(mesh.n_ele))
        for mode, mname in ((fcg.OVERWRITE, "overwrite"), (fcg.ACCUMULATE, "accumulate")):
            for table, cname in ((None, "uniform"), (ele_capa, "ele_capa")):
                C = t(rng.standard_normal(g.nnz_tt))
                tev.capacity(CAPA, table, mode, out=C)
                add(f"capacity {name} {mname}", cname, C)
        if name != "h8_433":
            tev.close()
            continue
        # one-step-theta on the evaluated k_TT / f_T; the block operator and its solve
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
        C = tev.capacity(CAPA)
        Tn = t(T0 + 50.0 * rng.standard_normal(g.n_cols_t))
        h = t(rng.standard_normal(g.n_rows_t))
        o = blocks(rng, mesh, g, zero=True)
        tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, v, T, THETA, 1.0 / DT, **o)
        for item, want_k, want_f in (("tangent only", True, False), ("residual only", False, True), ("both", True, True)):
            K, f = o["Ktt"].clone(), o["fT"].clone()
            tev.ost_combine(THETA, DT, C, T, Tn, h, Ktt=K if want_k else None, fT=f if want_f else None)
            add(f"ost {name}", item, K, f)
        Kss, fs = t(np.zeros(mesh.nnz)), t(np.zeros(mesh.n_rows))
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, t(1e-3 * rng.standard_normal(mesh.n_cols)), fs, Kss)
        X = fcg.BoxMesh(ct, spec["iv"]).node_x
        rows_t = np.sort(np.asarray(mesh.node_dof_row)[np.isclose(X[:, 0], 0.0)] // 3).astype(np.int32)
        rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
        ev.dirichlet_apply(t(rows_s), Kss)
        tev.dirichlet_apply(t(rows_s), t(rows_t), o["Kst"], o["Kts"], o["Ktt"])
        xs, xt = t(rng.standard_normal(mesh.n_rows)), t(rng.standard_normal(g.n_rows_t))
        ys, yt = torch.zeros_like(xs), torch.zeros_like(xt)
        tev.block_apply(ev, Kss, o["Kst"], o["Kts"], o["Ktt"], xs, xt, ys, yt)
        add(f"block_apply {name}", "y_S, y_T", ys, yt)
        bs, bt = rng.standard_normal(mesh.n_rows), rng.standard_normal(g.n_rows_t)
        bs[rows_s] = 0.0
        bt[rows_t] = 0.0
        xs, xt = torch.zeros_like(xs), torch.zeros_like(xt)
        it, _ = tev.gmres_solve(ev, Kss, o["Kst"], o["Kts"], o["Ktt"], t(bs), t(bt), xs, xt, rtol=1e-10,
                                max_iter=3000, restart=50)
        add(f"gmres_solve {name}", "x_S, x_T", xs, xt)
        add(f"gmres_solve {name}", "iterations", np.int64(it))
        tev.close()
        ev.close()

    # the fused evaluate on a structured mesh, as two passes (the default) and as one
    mesh = fcg.BoxMesh(fcg.HEX8, (6, 5, 4), jitter=0.1, seed=4)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
    tev = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND)
    g = tev.graph
    rng = np.random.default_rng(37)
    u, v = t(1e-3 * rng.standard_normal(mesh.n_cols)), t(1e-1 * rng.standard_normal(mesh.n_cols))
    T = t(T0 + 50.0 * rng.standard_normal(g.n_cols_t))
    for split, sname in ((None, "FCG_TSI_SPLIT unset"), ("0", "FCG_TSI_SPLIT=0")):
        os.environ.pop("FCG_TSI_SPLIT", None)
        if split is not None:
            os.environ["FCG_TSI_SPLIT"] = split
        o = blocks(rng, mesh, g, zero=True)
        o["Kss"] = t(np.zeros(mesh.nnz))
        tev.evaluate_fused(ev, fcg.OVERWRITE, u, v, T, 1.0, 1.0 / DT, **o)
        for k, a in o.items():
            add(f"evaluate_fused h8_654 {sname}", k, a)
    os.environ.pop("FCG_TSI_SPLIT", None)

    for tag, item, h in out:
        print(f"{tag}\t{item}\t{h}")


def compare(parent_a, parent_b, new):
    def read(p):
        with open(p) as fh:
            return {tuple(l.rstrip("\n").split("\t")[:2]): l.rstrip("\n").split("\t")[2] for l in fh if l.count("\t") == 2}

    a, b, n = read(parent_a), read(parent_b), read(new)
    keys = list(a) + [k for k in list(b) + list(n) if k not in a]
    bad = 0
    print(f"{'case':44s}{'item':16s}{'parent sha256':>14s}  {'branch sha256':>14s}  vs parent")
    for k in keys:
        pa, pb, nn = a.get(k), b.get(k), n.get(k)
        if pa and pb and pa != pb:
            fatal = k[0].startswith(REPRODUCIBLE)
            verdict = "PARENT NOT REPRODUCIBLE" if fatal else "excluded: the parent's two runs differ"
            bad += fatal
        else:
            verdict = "identical" if pa == pb == nn else "DIFFERENT" if pa and pb and nn else "MISSING"
            bad += verdict != "identical"
        print(f"{k[0]:44s}{k[1]:16s}{(pa or '-')[:12]:>14s}  {(nn or '-')[:12]:>14s}  {verdict}")
    print(f"{len(keys)} lines, {bad} not accepted")
    return 1 if bad or not keys else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=3, metavar=("PARENT_A", "PARENT_B", "NEW"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else fingerprint(os.path.abspath(a.root)))
