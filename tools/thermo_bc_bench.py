"""The thermal boundary-condition pass on one GPU: an n^3 hex8 box (default 126, BASELINE config 5's
mesh) with a convection condition on all six sides.  Times, alternated in one process:

    convection   one fcg_tsi_convection call, K_TT and f_T together
    evaluate     the FCG_TSI_THERMO_FINTCOND evaluate of the same context (what the pass follows)
    composed     the torch composition the pass replaces:
                     K.index_add_(0, pos, s_c A);  y = A * T[col];  r = 0.index_add_(0, entry_row, y);
                     f.index_add_(0, rows, s_c (r - s_t g))

hipEvents around `inner` back-to-back calls of each (default 20: one call of the pass is shorter than
an event pair resolves), 23 windows, the first 3 discarded, median and minimum per call.  Also the
host time of fcg_tsi_surface_create (plan and upload) and of fcg_tsi_surface_set (the setup kernel),
and the byte model of the pass: entries (8 A + 4 col + 8 pos + 16 K read and written + 8 T gathered)
+ rows (16 ptr + 4 row + 8 g + 16 f read and written).
The composition's index_add_ uses float atomics: its K and f are not reproducible bit by bit, the
pass's are.  Prints one JSON line.
usage: thermo_bc_bench.py [--n N] [--inner I]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fcg = importlib.import_module("4c_amd").fcg
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=126)
ap.add_argument("--inner", type=int, default=20)
a = ap.parse_args()
E, NU, ALPHA, T0, COND = 210.0, 0.3, 1.2e-5, 293.0, 52.0
S_C, S_T = 0.75, 1.25
assert torch.cuda.is_available(), "thermo_bc_bench.py needs cuda:0"
dev = torch.device("cuda:0")
f64 = dict(dtype=torch.float64, device=dev)


def per_call_ms(fns, inner, reps=23, warm=3):
    """hipEvent time per call of the callables, `inner` calls per window, alternated."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in fns}
    for rep in range(reps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            if rep >= warm:
                ms[k].append(e0.elapsed_time(e1) / inner)
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: float(np.min(v)) for k, v in ms.items()}


n = a.n
m = fcg.BoxMesh(fcg.HEX8, (n, n, n), jitter=0.1)
tev = fcg.TsiEvaluator(m, E, NU, ALPHA, T0, COND)
g = tev.graph
nt, nnz = g.n_rows_t, g.nnz_tt
t = time.perf_counter()
faces, _ = fcg.boundary_faces(m)
faces_ms = 1e3 * (time.perf_counter() - t)
assert len(faces) == 6 * n * n
torch.cuda.synchronize()
t = time.perf_counter()
surf = fcg.TsiSurface(tev, faces)
create_ms = 1e3 * (time.perf_counter() - t)
i = np.arange(len(faces))
coeff, surtemp = np.where(i % 3 == 0, 12.5, 90.0), 300.0 + 5.0 * (i % 4)
surf.set(coeff, surtemp, 1.0)
t = time.perf_counter()
surf.set(coeff, surtemp, 1.0)
set_ms = 1e3 * (time.perf_counter() - t)
info = surf.info

rng = np.random.default_rng(1)
T = torch.from_numpy(T0 + 50.0 * rng.standard_normal(g.n_cols_t)).to(dev)
v = torch.zeros(m.n_cols, **f64)
K, f = torch.empty(nnz, **f64), torch.empty(nt, **f64)
tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, v, T, fT=f, Ktt=K)
tab = surf.tables()
rows, col, pos = tab["rows"].long(), tab["col"].long(), tab["pos"]
A, gv = tab["A"], tab["g"]
entry_row = torch.repeat_interleave(torch.arange(info["n_rows"], device=dev), tab["ptr"][1:] - tab["ptr"][:-1])
r = torch.zeros(info["n_rows"], **f64)

# one call of each on copies: the pass and the composition agree to rounding
K1, f1, K2, f2 = K.clone(), f.clone(), K.clone(), f.clone()
surf.convection(T, fT=f1, Ktt=K1, coeff_scale=S_C, surtemp_scale=S_T)
K2.index_add_(0, pos, S_C * A)
f2.index_add_(0, rows, S_C * (torch.zeros_like(r).index_add_(0, entry_row, A * T[col]) - S_T * gv))
dK = float(((K1 - K2).abs().max() / K1.abs().max()).item())
df = float(((f1 - f2).abs().max() / f1.abs().max()).item())
assert dK <= 1e-14 and df <= 1e-12, (dK, df)


def convection():
    surf.convection(T, fT=f, Ktt=K, coeff_scale=S_C, surtemp_scale=S_T)


def evaluate():
    tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, v, T, fT=f, Ktt=K)


def composed():
    K.index_add_(0, pos, S_C * A)
    r.zero_().index_add_(0, entry_row, A * T[col])
    f.index_add_(0, rows, S_C * (r - S_T * gv))


med, mn = per_call_ms({"convection": convection, "evaluate": evaluate, "composed": composed}, a.inner)
model = info["n_entries"] * 44.0 + info["n_rows"] * 44.0
out = {"n": n, "rows_t": nt, "nnz_tt": nnz, "faces": len(faces), "surface_rows": info["n_rows"],
       "surface_entries": info["n_entries"], "surface_device_mb": info["device_bytes"] / 1e6,
       "boundary_faces_ms": faces_ms, "create_ms": create_ms, "set_ms": set_ms, "inner": a.inner,
       "convection_ms": med["convection"], "evaluate_ms": med["evaluate"], "composed_ms": med["composed"],
       "min_ms": mn, "convection_share_of_evaluate": med["convection"] / med["evaluate"],
       "convection_over_composed": med["convection"] / med["composed"], "model_mb": model / 1e6,
       "convection_model_gbs": model / 1e6 / med["convection"], "pass_vs_composed_rel_dK": dK,
       "pass_vs_composed_rel_df": df}
surf.close()
tev.close()
print(json.dumps(out))
