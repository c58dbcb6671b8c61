"""The scalar AMG's level-0 kernels alone on one GPU: an n^3 hex8 conduction box (v = 0), T fixed
at x = 0.  hipEvent medians of the scalar SpMV, the fused Chebyshev step, the restriction
r_c = P^T r and the prolongation x += P x_c (fcg_scsr_spmv / fcg_scsr_chebyshev_step on K_TT and on
the P_0 the hierarchy reports), one V-cycle, and the numeric setup split by level
(fcg_samg_setup_ms); the rate each kernel reaches by a byte model against the copy rate
fcg_measure_hbm measures in the same process.  Prints one JSON line.

Byte model (8-byte values, 4-byte columns, 8-byte row pointers; a gathered vector counted once):
  spmv      12 nnz + 8 (rows + 1) + 8 cols + 8 rows
  cheb      12 nnz + 8 (rows + 1) + 48 rows          (1 / a_ii, b, x, d read; d, x' written)
  restrict  12 nnz(P) + 8 (n_c + 1) + 8 rows + 8 n_c
  prolong   12 nnz(P) + 8 (rows + 1) + 8 n_c + 16 rows
usage: samg_probe.py [--n N] [--reps R]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fcg = importlib.import_module("4c_amd").fcg
amg = importlib.import_module("4c_amd.amg")
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--reps", type=int, default=30)
a = ap.parse_args()
E, NU, ALPHA, T0, COND, DT = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.5
dev = torch.device("cuda:0")
f64 = dict(dtype=torch.float64, device=dev)
iv = (a.n, a.n, a.n)
m = fcg.BoxMesh(fcg.HEX8, iv, jitter=0.1)
tev = fcg.TsiEvaluator(m, E, NU, ALPHA, T0, COND)
g = tev.graph
nt = g.n_rows_t
x0 = fcg.BoxMesh(fcg.HEX8, iv).node_x[:, 0]
rows_t = np.sort((np.asarray(m.node_dof_row) // 3)[np.isclose(x0, x0.min())]).astype(np.int32)
rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
rng = np.random.default_rng(1)
T = torch.from_numpy(T0 + 50.0 * rng.standard_normal(g.n_cols_t)).to(dev)
Kst, Kts, Ktt = (torch.zeros(k, **f64) for k in (g.nnz_st, g.nnz_ts, g.nnz_tt))
fs, fT = torch.zeros(m.n_rows, **f64), torch.zeros(nt, **f64)
tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, torch.zeros(m.n_cols, **f64), T, 1.0, 1.0 / DT, fs=fs,
                    Kst=Kst, fT=fT, Ktt=Ktt, Kts=Kts)
tev.dirichlet_apply(torch.from_numpy(rows_s).to(dev), torch.from_numpy(rows_t).to(dev), Kst, Kts, Ktt)
del Kst, Kts, fs
h = amg.ScalarAMG(tev, rows_t)
setups = []
for _ in range(5):
    h.setup(Ktt)
    setups.append([l["setup_ms"] for l in h.describe()])
info = h.describe()
L = fcg.lib()
s = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())


def median_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for rep in range(a.reps + 3):
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


ptr, col = torch.from_numpy(g.rowptr_tt).to(dev), torch.from_numpy(g.col_tt).to(dev)
w0 = int(np.diff(g.rowptr_tt).max())
x, b, d, y, xo = (torch.from_numpy(rng.standard_normal(nt)).to(dev) for _ in range(5))
dinv = torch.from_numpy(1.0 / (2.0 + rng.random(nt))).to(dev)
nnz = g.nnz_tt
out = {"n": a.n, "rows": nt, "nnz": nnz, "levels": [l["rows"] for l in info],
       "lmax": [l["lmax"] for l in info],
       "setup_ms_per_level": [float(v) for v in np.median(np.array(setups), axis=0)],
       "setup_ms": float(np.median(np.array(setups).sum(axis=1)))}
ms, mb = {}, {}
ms["spmv"] = median_ms(lambda: L.fcg_scsr_spmv(0, nt, w0, p(ptr), p(col), p(Ktt), p(x), None, p(y), 1.0, 0, s()))
mb["spmv"] = 12 * nnz + 8 * (nt + 1) + 16 * nt
ms["residual"] = median_ms(lambda: L.fcg_scsr_spmv(0, nt, w0, p(ptr), p(col), p(Ktt), p(x), p(b), p(y), 1.0, 2, s()))
mb["residual"] = mb["spmv"] + 8 * nt
ms["cheb"] = median_ms(lambda: L.fcg_scsr_chebyshev_step(0, nt, w0, p(ptr), p(col), p(Ktt), p(dinv), p(b), p(x),
                                                         p(d), p(xo), 0.3, 0.7, 1, s()))
mb["cheb"] = 12 * nnz + 8 * (nt + 1) + 48 * nt
if len(info) > 1:
    pp, pc, pv = h.level_matrix(0, 1)
    nc = info[1]["rows"]
    tp, tc, perm = amg.transpose_pattern(pp, pc, nc)
    dpp, dpc, dpv = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (pp, pc, pv))
    dtp, dtc, dtv = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (tp, tc, pv[perm]))
    xc, rc_ = torch.zeros(nc, **f64), torch.zeros(nc, **f64)
    wp, wt = int(np.diff(pp).max()), int(np.diff(tp).max())
    ms["restrict"] = median_ms(lambda: L.fcg_scsr_spmv(0, nc, wt, p(dtp), p(dtc), p(dtv), p(x), None, p(rc_), 1.0, 0, s()))
    mb["restrict"] = 12 * len(pv) + 8 * (nc + 1) + 8 * nt + 8 * nc
    ms["prolong"] = median_ms(lambda: L.fcg_scsr_spmv(0, nt, wp, p(dpp), p(dpc), p(dpv), p(xc), None, p(y), 1.0, 1, s()))
    mb["prolong"] = 12 * len(pv) + 8 * (nt + 1) + 8 * nc + 16 * nt
    out["p0_nnz"], out["p0_widest_row"], out["pt0_widest_row"] = len(pv), wp, wt
z = torch.zeros(nt, **f64)
ms["vcycle"] = median_ms(lambda: h.apply(Ktt, b, z))
copy_gbs, fill_gbs = fcg.measure_hbm(0)
out["ms"] = ms
out["model_mb"] = {k: v / 1e6 for k, v in mb.items()}
out["model_gbs"] = {k: mb[k] / 1e6 / ms[k] for k in mb}
out["hbm_copy_gbs"], out["hbm_fill_gbs"] = copy_gbs, fill_gbs
out["fraction_of_copy"] = {k: mb[k] / 1e6 / ms[k] / copy_gbs for k in mb}
print(json.dumps(out))
