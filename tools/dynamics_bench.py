"""Timings of the dynamics pieces on one GPU (profiles/dynamics/README.md), one JSON line each:
  efft    fcg_effective_tangent with K and y against its two-pass torch equivalent (K.mul_, K.add_
          of a CSR M, fcg_spmv on that M) and fcg_measure_hbm's copy figure; bytes counted per call:
          2 nnz 8 (K read and written) + nnz / 9 8 (m_node)
  mass    fcg_mass_nodal (first call: with the plan; then the plan reused) beside one CALC_NLNSTIFF
          evaluate of the same context
  newton  one generalized-alpha Newton iteration split into evaluate / effective tangent /
          Dirichlet / linear solve (block-Jacobi PCG on K_eff)
hipEvents around `reps` calls after a warm-up, except the first mass call (host clock around a
call that ends in a synchronise).
usage: dynamics_bench.py {efft,mass,newton} [--celltype hex8] [--n 100] [--reps 20]"""
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
dynamics = importlib.import_module("4c_amd.dynamics")

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["efft", "mass", "newton"])
ap.add_argument("--celltype", default="hex8")
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--kinematics", default="totlag")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dynamics_bench.py needs a GPU")
dev = torch.device("cuda:0")
ct = fcg.HEX8 if a.celltype == "hex8" else fcg.HEX27
kin = fcg.TOTLAG if a.kinematics == "totlag" else fcg.LINEAR
RHO, E, NU = 1e-3, 210.0, 0.3
m = fcg.BoxMesh(ct, (a.n, a.n, a.n), jitter=0.02)
ev = fcg.Evaluator(m, kinematics=kin, youngs=E, poisson=NU)
f64 = dict(dtype=torch.float64, device=dev)
s = torch.cuda.current_stream(dev)
base = {"config": f"{a.celltype}-{a.n}^3", "nnz": m.nnz, "path": int(ev.info.path)}


def timed(fn, reps=a.reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def evaluate_into(u, f, K):
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K)


u = torch.from_numpy(m.u_col(1e-3)).to(dev)
f = torch.zeros(m.n_rows, **f64)
K = torch.empty(m.nnz, **f64)

if a.what == "mass":
    m_node, m_lumped = torch.empty(m.nnz // 9, **f64), torch.empty(m.n_rows, **f64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.mass_nodal(RHO, m_node=m_node, m_lumped=m_lumped)  # returns after the stream drained
    first = (time.perf_counter() - t0) * 1e3
    ms_mass = timed(lambda: ev.mass_nodal(RHO, m_node=m_node, m_lumped=m_lumped), reps=5, warm=1)
    ms_eval = timed(lambda: evaluate_into(u, f, K), reps=5, warm=2)
    print(json.dumps(dict(base, what="mass", ms_mass_nodal_first_with_plan=first,
                          ms_mass_nodal=ms_mass, ms_evaluate_nlnstiff=ms_eval,
                          total_mass=float(m_lumped[0::3].sum()))))

if a.what == "efft":
    evaluate_into(u, f, K)
    m_node, _ = ev.mass_nodal(RHO, m_node=torch.empty(m.nnz // 9, **f64))
    M = ev.mass(RHO)
    x = torch.randn(m.n_cols, **f64)
    y, y2 = torch.zeros(m.n_rows, **f64), torch.zeros(m.n_rows, **f64)
    cK, cM = 0.5, 0.5  # a fixed point exists (K -> cM / (1 - cK) M): no growth over the repetitions
    K2 = K.clone()
    ms_fused = timed(lambda: ev.effective_tangent(cK, cM, m_node, K, x, y, stream=s))
    ms_konly = timed(lambda: ev.effective_tangent(cK, cM, m_node, K, stream=s))
    ms_yonly = timed(lambda: ev.effective_tangent(cK, cM, m_node, None, x, y, stream=s))

    def two_pass():
        K2.mul_(cK)
        K2.add_(M, alpha=cM)
        ev.spmv(M, x, y2, stream=s)

    ms_two = timed(two_pass)
    ms_spmv = timed(lambda: ev.spmv(M, x, y2, stream=s))
    copy_gbs, write_gbs = fcg.measure_hbm(0)
    byt = 2 * 8 * m.nnz + 8 * (m.nnz // 9)
    print(json.dumps(dict(base, what="efft", ms_fused=ms_fused, gb_counted=byt / 1e9,
                          gbs_fused=byt / ms_fused / 1e6, ms_K_only=ms_konly, ms_y_only=ms_yonly,
                          ms_torch_two_pass=ms_two, ms_spmv_csr_M=ms_spmv, hbm_copy_gbs=copy_gbs,
                          hbm_write_gbs=write_gbs,
                          y_vs_spmv=float(torch.linalg.norm(y - y2) / torch.linalg.norm(y2)))))

if a.what == "newton":
    X = m.node_x
    clamped = np.nonzero(np.isclose(X[:, 0], 0.0))[0]
    dbc = np.sort((m.node_dof_row[clamped][:, None] + np.arange(3)).ravel()).astype(np.int32)
    fext = np.zeros(m.n_rows)
    fext[2::3] = -1e-6
    dt = 1e-3  # ~45 x the explicit limit h / c of this box: K_eff is mass-dominated but not trivial
    ga = dynamics.GenAlpha(ev, RHO, dt, fext, dbc, lin_rtol=1e-10, lin_max_iter=3000)
    ga.initialize()
    am, af, beta, gamma = ga.alpha_m, ga.alpha_f, ga.beta, ga.gamma
    cM, cK = (1 - am) / (beta * dt * dt), 1 - af
    d = ga.d.clone()
    ms_eval = timed(lambda: evaluate_into(d, ga.fint, ga.K), reps=5, warm=2)
    ms_efft = timed(lambda: ev.effective_tangent(cK, cM, ga.m_node, ga.K, ga.a, ga._y, stream=s), reps=5, warm=1)
    evaluate_into(d, ga.fint, ga.K)
    ev.effective_tangent(cK, cM, ga.m_node, ga.K, ga.a, ga._y, stream=s)
    r = ga._y - ga.fext_at(dt)
    ms_dbc = timed(lambda: ev.dirichlet_apply(ga.dbc, ga.K, r, ga.freact, stream=s), reps=5, warm=1)
    its = []

    def solve():
        its.append(ev.pcg_solve(ga.K, r, ga.du, 1e-10, 3000, stream=s))

    ms_solve = timed(solve, reps=2, warm=1)
    t0 = time.perf_counter()
    ga.step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(base, what="newton", dt=dt, ms_evaluate=ms_eval, ms_effective_tangent=ms_efft,
                          ms_dirichlet=ms_dbc, ms_pcg_solve=ms_solve, pcg_iterations=its[-1][0],
                          pcg_relres=its[-1][1], init_accel_pcg=list(ga.init_lin),
                          ms_whole_step=step_ms, step_newton_iter=ga.history[-1]["newton_iter"],
                          step_lin_iter=ga.history[-1]["lin_iter"])))
