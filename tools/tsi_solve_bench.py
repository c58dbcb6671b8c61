"""One monolithic TSI solve on one GPU: an n^3 hex8 box, clamped and temperature-fixed at x = 0,
a heat flux on the face x = L, at a random admissible state (v != 0, so K_TS != 0).  The four
blocks come from the fused evaluate; the Newton system K dx = -(f_int - f_ext) is solved by
fcg_tsi_gmres_solve.  Prints one JSON line: iterations, ms per inner step split by hipEvents into
operator / preconditioner / orthogonalisation, and the bytes one inner step moves by a model
against the HBM rates fcg_measure_hbm measures on this device.

Model, per inner step at the mean basis length j (mean of the steps' j over the cycles):
  operator   the four blocks (16 values + 1 index per neighbour node) + read x, write y
  precond    K_SS diagonal blocks (9 per node) + K_TS ("bgs") + read r, write z
  orth       two Gram-Schmidt passes of: multi_dot (j + 1 vectors + w once per 8 of them),
             multi_axpy_norm (j + 1 vectors + w read and written); then the scaling of w
--orth-compare J: instead of a solve, one orthogonalisation (both Gram-Schmidt passes and the
norm) against J + 1 basis vectors of the box's stacked length, the library's kernels
(fcg_gmres_orthogonalize) and the same step in torch (h = V[:J+1] @ w, w.addmv_, twice, then the
norm), alternated, medians of 30.
--amg-s / --amg-t: amg.NativeAMG on K_SS / amg.ScalarAMG on K_TT in place of the Jacobi blocks
(fcg_tsi_gmres_solve_amg); the line then also holds each AMG's levels, its numeric setup in ms
(median of 3, host time around the blocking call) and the ms of one V-cycle (hipEvents, median
of 20).  The byte model of the preconditioner covers the Jacobi blocks only.
usage: tsi_solve_bench.py [--n N] [--precond bgs|diag] [--restart M] [--rtol R] [--max-iter K]
                          [--amg-s] [--amg-t] [--orth-compare J]"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fcg = importlib.import_module("4c_amd").fcg
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=32)
ap.add_argument("--precond", choices=["bgs", "diag"], default="bgs")
ap.add_argument("--restart", type=int, default=50)
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--max-iter", type=int, default=20000)
ap.add_argument("--orth-compare", type=int, default=-1)
ap.add_argument("--amg-s", action="store_true")
ap.add_argument("--amg-t", action="store_true")
a = ap.parse_args()
if a.orth_compare >= 0:
    dev = torch.device("cuda:0")
    n, nv = 4 * (a.n + 1) ** 3, a.orth_compare + 1
    gen = torch.Generator(device=dev).manual_seed(1)
    V = torch.randn(nv, n, dtype=torch.float64, device=dev, generator=gen) / math.sqrt(n)
    w0 = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    h = torch.empty(nv + 1, dtype=torch.float64, device=dev)
    work = torch.empty(fcg.gmres_orthogonalize_work(n, nv), dtype=torch.float64, device=dev)
    Vt = V.t()

    def ours(w):
        fcg.gmres_orthogonalize(V, w, h, work=work)

    def with_torch(w):
        for _ in range(2):
            w.addmv_(Vt, V @ w, alpha=-1.0)
        return torch.linalg.vector_norm(w)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {"ours": [], "torch": []}
    for rep in range(33):
        for name, f in (("ours", ours), ("torch", with_torch)):
            w = w0.clone()
            torch.cuda.synchronize()
            e0.record()
            f(w)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:
                ms[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    model = 2 * ((nv + math.ceil(nv / 8)) + (nv + 2)) * 8.0 * n
    print(json.dumps({"orth_compare": True, "n": a.n, "unknowns": n, "basis_vectors": nv,
                      "ours_ms": med["ours"], "torch_ms": med["torch"],
                      "model_mb": model / 1e6, "ours_model_gbs": model / 1e6 / med["ours"],
                      "min_ms": {k: float(np.min(v)) for k, v in ms.items()}}))
    sys.exit(0)
E, NU, ALPHA, T0, COND, DT = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.5
dev = torch.device("cuda:0")
f64 = dict(dtype=torch.float64, device=dev)
iv = (a.n, a.n, a.n)
m = fcg.BoxMesh(fcg.HEX8, iv, jitter=0.1)
ev = fcg.Evaluator(m, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
tev = fcg.TsiEvaluator(m, E, NU, ALPHA, T0, COND)
g = tev.graph
ns, nt = m.n_rows, g.n_rows_t
x0 = fcg.BoxMesh(fcg.HEX8, iv).node_x[:, 0]  # faces by the coordinates of the box without jitter
row_t = np.asarray(m.node_dof_row) // 3
rows_t = np.sort(row_t[np.isclose(x0, x0.min())]).astype(np.int32)
rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
far = row_t[np.isclose(x0, x0.max())]
rng = np.random.default_rng(1)
u = torch.from_numpy(1e-3 * rng.standard_normal(m.n_cols)).to(dev)
v = torch.from_numpy(1e-2 * rng.standard_normal(m.n_cols)).to(dev)
T = torch.from_numpy(T0 + 50.0 * rng.standard_normal(g.n_cols_t)).to(dev)
for t in (u, v):
    t[torch.from_numpy(rows_s).to(dev).long()] = 0.0
T[torch.from_numpy(rows_t).to(dev).long()] = T0
fext_t = torch.zeros(nt, **f64)
fext_t[torch.from_numpy(far).to(dev).long()] = 1.0 / len(far)  # unit heat flux over the face x = L
fs, fT = torch.zeros(ns, **f64), torch.zeros(nt, **f64)
K = {k: torch.zeros(n, **f64) for k, n in (("Kss", m.nnz), ("Kst", g.nnz_st), ("Kts", g.nnz_ts),
                                           ("Ktt", g.nnz_tt))}
tev.evaluate_fused(ev, fcg.OVERWRITE, u, v, T, 1.0, 1.0 / DT, fs=fs, fT=fT, **K)
fs.neg_()
fT.sub_(fext_t).neg_()
ds, dt_ = torch.from_numpy(rows_s).to(dev), torch.from_numpy(rows_t).to(dev)
ev.dirichlet_apply(ds, K["Kss"], fs)
tev.dirichlet_apply(ds, dt_, K["Kst"], K["Kts"], K["Ktt"], fT)
xs, xt = torch.zeros(ns, **f64), torch.zeros(nt, **f64)


def cycle_ms(apply, K_, r, z):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(23):
        torch.cuda.synchronize()
        e0.record()
        apply(K_, r, z)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def setup_ms(h, K_):
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        h.setup(K_)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ms))


amg_s = amg_t = None
amg_out = {}
if a.amg_s or a.amg_t:
    amg_mod = importlib.import_module("4c_amd.amg")
if a.amg_s:
    t = time.perf_counter()
    amg_s = amg_mod.NativeAMG(m, ev, rows_s)
    amg_out["amg_s"] = {"create_s": time.perf_counter() - t, "setup_ms": setup_ms(amg_s, K["Kss"]),
                        "levels": [l["dofs"] for l in amg_s.describe()]}
    amg_out["amg_s"]["vcycle_ms"] = cycle_ms(amg_s.apply, K["Kss"], fs, torch.zeros_like(fs))
if a.amg_t:
    t = time.perf_counter()
    amg_t = amg_mod.ScalarAMG(tev, rows_t)
    amg_out["amg_t"] = {"create_s": time.perf_counter() - t, "setup_ms": setup_ms(amg_t, K["Ktt"]),
                        "levels": [l["rows"] for l in amg_t.describe()]}
    amg_out["amg_t"]["vcycle_ms"] = cycle_ms(amg_t.apply, K["Ktt"], fT, torch.zeros_like(fT))
solve = lambda: tev.gmres_solve(ev, K["Kss"], K["Kst"], K["Kts"], K["Ktt"], fs, fT, xs, xt,
                                rtol=a.rtol, max_iter=a.max_iter, restart=a.restart,
                                precond=a.precond, amg=amg_s, amg_t=amg_t)
solve()  # the first solve allocates the work space and verifies the graphs
fcg.gmres_timing(True)
torch.cuda.synchronize()
t0 = time.perf_counter()
it, rel = solve()
torch.cuda.synchronize()
wall = time.perf_counter() - t0
tm = fcg.gmres_timing()
fcg.gmres_timing(False)
steps = max(1, tm["steps"])
# mean basis length: cycles of `restart` steps, the last one shorter
full, rest = divmod(it, a.restart)
j_mean = (full * sum(range(a.restart)) + sum(range(rest))) / max(1, it)
n = ns + nt
vec = 8.0 * n
nnz = g.nnz_tt
b_op = nnz * (16 * 8 + 4) + 2 * vec
b_pre = 9 * 8 * nt + (3 * 8 + 4) * nnz * (a.precond == "bgs") + 2 * vec
jv = j_mean + 1
b_orth = 2 * ((jv + math.ceil(jv / 8)) + (jv + 2)) * vec + 2 * vec
copy_gbs, fill_gbs = fcg.measure_hbm(0)
out = {"n": a.n, "unknowns": n, "precond": a.precond, "restart": a.restart, "rtol": a.rtol,
       "iterations": it, "rel_residual": rel, "converged": bool(rel <= a.rtol),
       "wall_ms": 1e3 * wall, "steps_timed": tm["steps"], "mean_j": j_mean,
       "ms_per_step": {"operator": tm["operator_ms"] / steps, "precond": tm["precond_ms"] / steps,
                       "orth": tm["orth_ms"] / steps, "wall": 1e3 * wall / max(1, it)},
       "model_mb_per_step": {"operator": b_op / 1e6, "precond": b_pre / 1e6, "orth": b_orth / 1e6},
       "model_gbs": {"operator": b_op / 1e6 / max(1e-9, tm["operator_ms"] / steps),
                     "precond": b_pre / 1e6 / max(1e-9, tm["precond_ms"] / steps),
                     "orth": b_orth / 1e6 / max(1e-9, tm["orth_ms"] / steps)},
       "hbm_copy_gbs": copy_gbs, "hbm_fill_gbs": fill_gbs}
out.update(amg_out)
print(json.dumps(out))
