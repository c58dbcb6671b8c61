"""The transient thermal kernels on one GPU: an n^3 hex8 box (default 126, BASELINE config 5's mesh).
fcg_tsi_capacity once (host time around the blocking call, plan included, and a second call without
the plan), fcg_tsi_ost_combine per call (hipEvents, 23 calls, the first 3 discarded, median: the
warm-up and repeats of tools/tsi_solve_bench.py) against its byte model and the copy rate
fcg_measure_hbm measures in the same process, and against the composition available without the
kernel, alternated with it in the same run:

    K.mul_(theta).add_(C, alpha=1/dt)                               torch, 2 passes over K
    dT = T - Tn;  y = C dT  (fcg_scsr_spmv);  f.mul_(theta).add_(y, alpha=1/dt).add_(h)

Byte model of the fused pass: nnz (8 K read + 8 K write + 8 C + 4 col) + 8 (rows + 1) row pointers
+ the two gathered vectors once (16 cols) + f read and written and h (24 rows).

--tsi N: also one time step of tsi.TsiMonolithic on an N^3 box (the problem of
tools/tsi_solve_bench.py: clamped and temperature-fixed at x = 0, a heat flux on x = L; both AMGs),
static and with thermal="ost", wall time of the second step of each, and the share of the
one-step-theta pass in the transient step (its hipEvent time at N^3 times the Newton iterations).
Prints one JSON line.
usage: thermo_ost_bench.py [--n N] [--theta TH] [--dt DT] [--tsi N]"""
import argparse
import ctypes
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
ap.add_argument("--theta", type=float, default=0.5)
ap.add_argument("--dt", type=float, default=0.5)
ap.add_argument("--tsi", type=int, default=0)
a = ap.parse_args()
E, NU, ALPHA, T0, COND, CAPA = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 3.5
dev = torch.device("cuda:0")
f64 = dict(dtype=torch.float64, device=dev)
L = fcg.lib()
p = lambda t: ctypes.c_void_p(t.data_ptr())


def median_ms(fns, reps=23, warm=3):
    """hipEvent medians of the callables, alternated."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in fns}
    for rep in range(reps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if rep >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: float(np.min(v)) for k, v in ms.items()}


def kernels(n):
    m = fcg.BoxMesh(fcg.HEX8, (n, n, n), jitter=0.1)
    tev = fcg.TsiEvaluator(m, E, NU, ALPHA, T0, COND)
    g = tev.graph
    nt, nnz = g.n_rows_t, g.nnz_tt
    torch.cuda.synchronize()
    t = time.perf_counter()
    C = tev.capacity(CAPA)
    first = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    tev.capacity(CAPA, out=C)
    again = 1e3 * (time.perf_counter() - t)
    rng = np.random.default_rng(1)
    T = torch.from_numpy(T0 + 50.0 * rng.standard_normal(g.n_cols_t)).to(dev)
    Tn = T * (1 - 1e-3)
    h = torch.from_numpy(rng.standard_normal(nt)).to(dev)
    v = torch.zeros(m.n_cols, **f64)
    K, f = torch.empty(nnz, **f64), torch.empty(nt, **f64)
    tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, v, T, fT=f, Ktt=K)
    ptr = torch.from_numpy(np.ascontiguousarray(g.rowptr_tt)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(g.col_tt)).to(dev)
    width = int(np.diff(g.rowptr_tt).max())
    dT, y = torch.empty_like(T), torch.empty(nt, **f64)
    th, dt = a.theta, a.dt
    s = lambda: fcg._torch_stream(None, 0)

    def fused():
        tev.ost_combine(th, dt, C, T, Tn, h=h, Ktt=K, fT=f)

    def composed():
        K.mul_(th).add_(C, alpha=1.0 / dt)
        torch.sub(T, Tn, out=dT)
        L.fcg_scsr_spmv(0, nt, width, p(ptr), p(col), p(C), p(dT), None, p(y), 1.0, 0, s())
        f.mul_(th).add_(y, alpha=1.0 / dt).add_(h)

    # the repeated in-place passes keep K finite: theta <= 1 contracts it towards C / (dt (1 - theta))
    med, mn = median_ms({"fused": fused, "composed": composed})
    model = nnz * 28.0 + 8.0 * (nt + 1) + 16.0 * g.n_cols_t + 24.0 * nt
    copy_gbs, fill_gbs = fcg.measure_hbm(0)
    out = {"n": n, "rows": nt, "nnz": nnz, "capacity_first_ms": first, "capacity_ms": again,
           "combine_ms": med["fused"], "composed_ms": med["composed"], "min_ms": mn,
           "model_mb": model / 1e6, "combine_model_gbs": model / 1e6 / med["fused"],
           "hbm_copy_gbs": copy_gbs, "hbm_fill_gbs": fill_gbs,
           "combine_fraction_of_copy": model / 1e6 / med["fused"] / copy_gbs}
    tev.close()
    return out


def tsi_step(n):
    tsi, amg = importlib.import_module("4c_amd.tsi"), importlib.import_module("4c_amd.amg")
    iv = (n, n, n)
    m = fcg.BoxMesh(fcg.HEX8, iv, jitter=0.1)
    x0 = fcg.BoxMesh(fcg.HEX8, iv).node_x[:, 0]
    row_t = np.asarray(m.node_dof_row) // 3
    rows_t = np.sort(row_t[np.isclose(x0, x0.min())]).astype(np.int32)
    rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
    far = row_t[np.isclose(x0, x0.max())]
    out = {"n": n}
    for thermal in ("statics", "ost"):
        ev = fcg.Evaluator(m, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
        tev = fcg.TsiEvaluator(m, E, NU, ALPHA, T0, COND)
        fext_t = np.zeros(tev.graph.n_rows_t)
        fext_t[far] = 1.0 / len(far)
        run = tsi.TsiMonolithic(ev, tev, a.dt, np.zeros(m.n_rows), fext_t, rows_s, rows_t,
                                T_init=np.full(tev.graph.n_rows_t, T0), lin_rtol=1e-8, tol_inc=1e-8,
                                amg=amg.NativeAMG(m, ev, rows_s), amg_t=amg.ScalarAMG(tev, rows_t),
                                thermal=thermal, capa=CAPA, theta=a.theta)
        run.step()
        torch.cuda.synchronize()
        t = time.perf_counter()
        rec = run.step()
        torch.cuda.synchronize()
        out[thermal] = {"step_ms": 1e3 * (time.perf_counter() - t), "newton": rec["iterations"],
                        "gmres": rec["gmres_iterations"]}
        if thermal == "ost":
            T, Tn, h = run.T, run.T_n, run.h
            K, f = run.Ktt.clone(), run.fT.clone()
            med, _ = median_ms({"fused": lambda: tev.ost_combine(a.theta, a.dt, run.C, T, Tn, h=h, Ktt=K, fT=f)})
            out["combine_ms"] = med["fused"]
            out["combine_share_of_step"] = med["fused"] * rec["iterations"] / out["ost"]["step_ms"]
    return out


res = kernels(a.n)
if a.tsi:
    res["tsi"] = tsi_step(a.tsi)
print(json.dumps(res))
