"""CPU tests of tests/krylov_ref.py, the numpy FGMRES the GPU tests of fcg_gmres_solve and
fcg_tsi_gmres_solve are held against: it solves the monolithic systems of the reference's TSI
known-answer inputs and of a jittered TSI box to the accuracy the condition number allows, and it
stays inside every iteration cap the GPU tests use (tests/test_gmres.py, tests/test_tsi_solve.py).

Error bound: x solves A x = b with |b - A x| <= rtol |b|, so |x - x*| <= |A^-1| rtol |b| <=
cond_2(A) rtol |x*|.
"""

import importlib
import json
import os

import numpy as np
import pytest

import krylov_ref as kr
from parity_util import oracle_evaluate
from tsi_driver import TsiProblem

fcg = importlib.import_module("4c_amd").fcg
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E, NU, ALPHA, T0, COND, DT = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.05
RTOL = 1e-10


def _check(A, b, precond, restart, max_iter, rtol=RTOL):
    x, it, rel, _ = kr.fgmres(A, b, restart, rtol, max_iter, precond)
    ref = np.linalg.solve(A, b)
    assert rel <= rtol, rel
    assert abs(rel - np.linalg.norm(b - A @ x) / np.linalg.norm(b)) <= 1e-6 * rtol
    cond = np.linalg.cond(A)
    err = np.linalg.norm(x - ref)
    assert err <= cond * rtol * np.linalg.norm(ref), (err, cond)
    return ref, it


@pytest.mark.parametrize("name,newton_total", [("tsi_heatflux_monolithic.json", 20),
                                               ("tsi_heatflux_flexoutsurf_monolithic.json", 25)])
def test_reference_solves_the_golden_tsi_systems(name, newton_total):
    """Every Newton system of the known-answer runs, with the settings tsi.TsiMonolithic defaults
    to (block Gauss-Seidel, restart 50, rtol 1e-10): inside lin_max_iter = 2000, and to the
    condition-number bound against the dense solve the driver uses."""
    prob = TsiProblem(json.load(open(os.path.join(GOLD, name))))
    ns, nn = prob.ns, prob.nn
    fixed = np.concatenate([prob.dbc_s, ns + prob.dbc_t]).astype(np.int64)
    d, T = np.zeros(ns), prob.T_init.copy()
    worst, total = 0, 0
    for step in range(1, prob.nstep + 1):
        t = step * prob.dt
        fes, fet = prob.fext_s(t), prob.fext_t(t)
        d_n = d.copy()
        for it in range(30):
            Kss, Kst, Kts, Ktt, fs, fT = prob.assemble_oracle(d, T, (d - d_n) / prob.dt)
            A = kr.apply_dirichlet_dense(np.block([[Kss, Kst], [Kts, Ktt]]), fixed)
            b = -np.concatenate([fs - fes, fT - fet])
            b[fixed] = 0.0
            P = kr.tsi_precond(A[:ns, :ns], A[ns:, :ns], A[ns:, ns:], bgs=True)
            dx, n_it = _check(A, b, P, 50, 2000)
            worst = max(worst, n_it)
            x = np.concatenate([d, T]) + dx
            d, T = x[:ns], x[ns:]
            total += 1
            if np.linalg.norm(dx) <= 1e-13 * max(1.0, np.linalg.norm(x)):
                break
        else:
            raise AssertionError("Newton did not converge")
    print(f"{name}: {total} Newton systems, at most {worst} FGMRES(50) steps per solve")
    assert total == newton_total
    assert worst <= 2000


def _tsi_box(iv, seed=5):
    """A jittered hex8 TSI box at a random state with v != 0 (so K_TS != 0), clamped and
    temperature-fixed at x = 0."""
    mesh = fcg.BoxMesh(fcg.HEX8, iv, jitter=0.1, seed=seed)
    rng = np.random.default_rng(seed)
    u = 1e-3 * rng.standard_normal(mesh.n_cols)
    v = 1e-1 * rng.standard_normal(mesh.n_cols)
    T = T0 + 50.0 * rng.standard_normal(mesh.n_cols // 3)
    Kss, Kst, Kts, Ktt, _, _ = kr.oracle_tsi_blocks(mesh, u, v, T, E, NU, ALPHA, T0, COND, DT)
    ns = mesh.n_rows
    nodes = kr.x0_face(fcg.HEX8, iv)
    c0 = np.asarray(mesh.node_dof_col)[nodes]
    fixed = np.concatenate([(c0[:, None] + np.arange(3)).ravel(), ns + c0 // 3])
    A = kr.apply_dirichlet_dense(np.block([[Kss, Kst], [Kts, Ktt]]), fixed)
    b = rng.standard_normal(A.shape[0])
    b[fixed] = 0.0
    return A, b, ns


@pytest.mark.parametrize("bgs", [False, True], ids=["diag", "bgs"])
def test_reference_solves_a_jittered_tsi_box(bgs):
    A, b, ns = _tsi_box((3, 3, 3))
    assert np.abs(A[ns:, :ns]).max() > 0 and not np.allclose(A[:ns, ns:], A[ns:, :ns].T)
    P = kr.tsi_precond(A[:ns, :ns], A[ns:, :ns], A[ns:, ns:], bgs=bgs)
    # 192 free unknowns: the library's largest restart (128), and a short one
    _, full = _check(A, b, P, 128, 2000)
    _, restarted = _check(A, b, P, 30, 2000)
    print(f"3^3 TSI box bgs={bgs}: {full} steps at restart 128, {restarted} at restart 30")
    assert full <= 2000 and restarted <= 2000


def test_reference_on_a_larger_tsi_box():
    """6^3 elements, 1,372 unknowns, restart 30: the iteration count of a mesh the size the
    solver is meant for stays far inside tsi.TsiMonolithic's lin_max_iter = 2000."""
    A, b, ns = _tsi_box((6, 6, 6))
    P = kr.tsi_precond(A[:ns, :ns], A[ns:, :ns], A[ns:, ns:], bgs=True)
    _, it = _check(A, b, P, 30, 2000)
    print(f"6^3 TSI box: {it} steps at restart 30")
    assert it <= 2000


def test_reference_restart_path_stays_inside_the_gpu_cap():
    """tests/test_gmres.py's restart case: hex8 (4,4,4), block Jacobi, restart 5, rtol 1e-8 must
    converge well inside max_iter = 5000."""
    mesh = fcg.BoxMesh(fcg.HEX8, (4, 4, 4), jitter=0.1, seed=1)
    err, _, Kv, _ = oracle_evaluate(mesh, fcg.LINEAR, E, NU, np.zeros(mesh.n_cols))
    assert err == 0
    A = kr.csr_to_dense(mesh.rowptr, mesh.col_lid, Kv)
    nodes = kr.x0_face(fcg.HEX8, (4, 4, 4))
    rows = (np.asarray(mesh.node_dof_row)[nodes][:, None] + np.arange(3)).ravel()
    A = kr.apply_dirichlet_dense(A, rows)
    b = np.random.default_rng(3).standard_normal(mesh.n_rows)
    b[rows] = 0.0
    _, it = _check(A, b, kr.block_jacobi(A), 5, 5000, rtol=1e-8)
    print(f"hex8 4^3 block Jacobi restart 5: {it} steps")
    assert 5 < it < 5000


def test_reference_matches_csr_and_dense_input():
    rng = np.random.default_rng(0)
    A = np.eye(12) * 4 + rng.standard_normal((12, 12))
    rp = np.arange(13) * 12
    col = np.tile(np.arange(12), 12)
    b = rng.standard_normal(12)
    xa, ia, _, _ = kr.fgmres(A, b, 12, 1e-12, 100)
    xb, ib, _, _ = kr.fgmres((rp, col, A.ravel()), b, 12, 1e-12, 100)
    assert ia == ib and np.allclose(xa, xb, rtol=0, atol=1e-13 * np.linalg.norm(xa))
    assert np.linalg.norm(A @ xa - b) <= 1e-12 * np.linalg.norm(b)
