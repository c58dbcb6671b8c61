"""GPU tests of the scalar smoothed-aggregation AMG of K_TT (4c_amd/csrc/fcg_samg_plan.cpp,
fcg_samg.hip; amg.ScalarAMG) and of the monolithic TSI solve with it as the thermal block of the
preconditioner (fcg_tsi_gmres_solve_amg).

Bounds as in tests/test_tsi_solve.py: a row sum against the extended-precision reference within
(terms + 2) 2^-53 |A||x| (the fused Chebyshev step two roundings more); a Galerkin entry within
(terms + 2) 2^-53 (|P|^T |A| |P|); the dense V-cycle operator against its longdouble rebuild within
8 times the float64 rebuild's own distance from it; a solve's residual within rtol |b| + sigma and
its error within cond_2(A) rtol |x*|."""

import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import krylov_ref as kr
import samg_ref
import solver_ref as sr
from solver_ref import LD, U
from tsi_driver import TsiProblem

torch = pytest.importorskip("torch")
fcg = importlib.import_module("4c_amd").fcg
amg = importlib.import_module("4c_amd.amg")
tsi = importlib.import_module("4c_amd.tsi")
gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E, NU, ALPHA, T0, COND, DT = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.05
FCG_ERR_SINGULAR, FCG_ERR_ARG = 2, 3

MESHES = {
    "h8_322": (fcg.HEX8, (3, 2, 2), 0.1),
    "h8_333": (fcg.HEX8, (3, 3, 3), 0.1),      # an interior row of 27 neighbours
    "h27_221": (fcg.HEX27, (2, 2, 1), 0.02),
    "h27_333": (fcg.HEX27, (3, 3, 3), 0.02),   # 343 nodes, one row of 125 neighbours: 64-lane rows
    "h8_433": (fcg.HEX8, (4, 3, 3), 0.1),
    "h8_654": (fcg.HEX8, (6, 5, 4), 0.1),
    "h27_322": (fcg.HEX27, (3, 2, 2), 0.02),
    "h8_12": (fcg.HEX8, (12, 12, 12), 0.1),
    "h8_24": (fcg.HEX8, (24, 24, 24), 0.1),
}
SMALL = ["h8_322", "h8_333", "h27_221", "h27_333"]
_cache, _sys = {}, {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t if dtype is None else t.to(dtype)


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


def _z(n):
    return torch.zeros(int(n), dtype=torch.float64, device=_dev())


def _case(name, struct=False):
    """(mesh, structural Evaluator or None, TsiEvaluator, rows_s, rows_t): the x = 0 face is the
    Dirichlet set of both fields."""
    _dev()
    if name not in _cache:
        ct, iv, jitter = MESHES[name]
        mesh = fcg.BoxMesh(ct, iv, jitter=jitter, seed=4)
        tev = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND)
        face = kr.x0_face(ct, iv)
        rows_t = np.sort(np.asarray(mesh.node_dof_row)[face] // 3).astype(np.int32)
        rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
        _cache[name] = [mesh, None, tev, rows_s, rows_t]
    c = _cache[name]
    if struct and c[1] is None:
        c[1] = fcg.Evaluator(c[0], kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    return c


def _system(name, v_scale, struct=False):
    """The blocks at a random admissible state (velocity v_scale * N(0, 1)) with the Dirichlet rows
    applied, on the device and the host, and a random right-hand side that is zero on them.
    struct: K_SS too (else only the three TSI blocks)."""
    key = (name, v_scale, struct)
    if key in _sys:
        return _sys[key]
    mesh, ev, tev, rows_s, rows_t = _case(name, struct)
    g = tev.graph
    rng = np.random.default_rng(23)
    u = 1e-3 * rng.standard_normal(mesh.n_cols)
    v = v_scale * rng.standard_normal(mesh.n_cols)
    T = T0 + 50.0 * rng.standard_normal(g.n_cols_t)
    fs, fT = _z(mesh.n_rows), _z(g.n_rows_t)
    d = {"Kst": _z(g.nnz_st), "Kts": _z(g.nnz_ts), "Ktt": _z(g.nnz_tt)}
    if struct:
        d["Kss"] = _z(mesh.nnz)
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(u), fs, d["Kss"])
        ev.dirichlet_apply(_t(rows_s), d["Kss"])
    tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, _t(v), _t(T), 1.0, 1.0 / DT, fs=fs, Kst=d["Kst"],
                        fT=fT, Ktt=d["Ktt"], Kts=d["Kts"])
    tev.dirichlet_apply(_t(rows_s), _t(rows_t), d["Kst"], d["Kts"], d["Ktt"])
    bs, bt = rng.standard_normal(mesh.n_rows), rng.standard_normal(g.n_rows_t)
    bs[rows_s] = 0.0
    bt[rows_t] = 0.0
    torch.cuda.synchronize()
    _sys[key] = (d, {k: a.cpu().numpy() for k, a in d.items()}, bs, bt)
    return _sys[key]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dense(M, n_cols):
    return samg_ref.csr_dense(M[0], M[1], M[2], n_cols, LD)


# ------------------------------------------------------------------------------- 1. primitives
def _spmv(n, w, ptr, col, vals, x, b, y, alpha, mode):
    rc = fcg.lib().fcg_scsr_spmv(0, n, w, _p(ptr), _p(col), _p(vals), _p(x), None if b is None else _p(b),
                                 _p(y), float(alpha), mode, _stream())
    assert rc == 0


def _cheb(n, w, ptr, col, vals, dinv, b, x, d, xo, c_d, c_r, mode):
    rc = fcg.lib().fcg_scsr_chebyshev_step(0, n, w, _p(ptr), _p(col), _p(vals), _p(dinv), _p(b), _p(x),
                                           _p(d), _p(xo), float(c_d), float(c_r), mode, _stream())
    assert rc == 0


@gpu
@pytest.mark.parametrize("name", SMALL)
def test_primitives_componentwise(name):
    """Scalar SpMV (y = alpha A x, y += alpha A x, r = b - A x) and the fused Chebyshev step in its
    three modes on the mesh's k_TT graph with random values, against the 80-bit reference row by
    row; two calls give the same bits."""
    g = _case(name)[2].graph
    n, ptr, col = g.n_rows_t, g.rowptr_tt, g.col_tt
    terms = np.diff(ptr)
    w = int(terms.max())
    rng = np.random.default_rng(31)
    vals, x, b, y0, d0 = (rng.standard_normal(k) for k in (g.nnz_tt, n, n, n, n))
    dinv = 1.0 / (2.0 + rng.random(n))
    alpha, c_d, c_r = -0.75, 0.3125, 1.7
    dptr, dcol, dv, dx, db, ddinv = _t(ptr), _t(col), _t(vals), _t(x), _t(b), _t(dinv)
    ax, aax = sr.csr_matvec_ld(ptr, col, vals, x)
    bl, xl, dl, dil = b.astype(LD), x.astype(LD), d0.astype(LD), dinv.astype(LD)
    worst = {}

    def check(tag, got, ref, absum, extra):
        err = np.abs(got.astype(LD) - ref)
        bound = (terms + 2 + extra) * LD(U) * absum
        worst[tag] = float((err / bound).max())
        assert np.all(np.isfinite(got)) and np.all(err <= bound), (tag, worst[tag])

    for mode, ref, absum in ((0, LD(alpha) * ax, abs(alpha) * aax),
                             (1, y0.astype(LD) + LD(alpha) * ax, np.abs(y0) + abs(alpha) * aax),
                             (2, bl - ax, np.abs(b) + aax)):
        out = []
        for _ in range(2):
            y = _t(y0) if mode == 1 else _nan(n)
            _spmv(n, w, dptr, dcol, dv, dx, db if mode == 2 else None, y, alpha, mode)
            out.append(y)
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1])
        check(f"spmv{mode}", out[0].cpu().numpy(), ref, absum, 0)
    z, az = (bl - ax) * dil, (np.abs(b) + aax) * np.abs(dinv)
    for mode, dref, dabs, xref, xabs in (
            (0, LD(c_r) * z, c_r * az, xl + LD(c_r) * z, np.abs(x) + c_r * az),
            (1, LD(c_d) * dl + LD(c_r) * z, c_d * np.abs(d0) + c_r * az,
             xl + LD(c_d) * dl + LD(c_r) * z, np.abs(x) + c_d * np.abs(d0) + c_r * az),
            (2, LD(c_r) * bl * dil, c_r * np.abs(b * dinv), LD(c_r) * bl * dil, c_r * np.abs(b * dinv))):
        out = []
        for _ in range(2):
            d, xo = _t(d0), _nan(n)
            _cheb(n, w, dptr, dcol, dv, ddinv, db, dx, d, xo, c_d, c_r, mode)
            out.append((d, xo))
        torch.cuda.synchronize()
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        check(f"cheb{mode}.d", out[0][0].cpu().numpy(), dref, dabs, 2)
        check(f"cheb{mode}.x", out[0][1].cpu().numpy(), xref, xabs, 2)
    print(f"primitives {name}: longest row {w}, worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------- 2. Galerkin identity
def _hierarchy(name, v_scale, **opts):
    """(ScalarAMG set up on the mesh's K_TT, its level matrices, prolongators, level info)."""
    mesh, _, tev, rows_s, rows_t = _case(name)
    d, h, bs, bt = _system(name, v_scale)
    a = amg.ScalarAMG(tev, rows_t, **opts)
    a.setup(d["Ktt"])
    info = a.describe()
    A = [a.level_matrix(l, 0) for l in range(len(info))]
    P = [a.level_matrix(l, 1) for l in range(len(info) - 1)]
    return a, A, P, info


@gpu
@pytest.mark.parametrize("name,coarse_max", [("h8_654", 4), ("h27_322", 1)])
def test_galerkin_identity_on_fetched_levels(name, coarse_max):
    mesh, _, tev, rows_s, rows_t = _case(name)
    a, A, P, info = _hierarchy(name, 1e-1, coarse_max=coarse_max)
    print(f"galerkin {name}: levels {[(i['rows'], i['nnz']) for i in info]}, "
          f"lambda_max {[round(i['lmax'], 4) for i in info]}")
    assert len(info) >= 3
    g = tev.graph
    assert np.array_equal(A[0][0], g.rowptr_tt) and np.array_equal(A[0][1], g.col_tt)
    for l in range(len(P)):
        nf, nc = info[l]["rows"], info[l + 1]["rows"]
        Al, Pl, Ac = _dense(A[l], nf), _dense(P[l], nc), _dense(A[l + 1], nc)
        if l == 0:
            assert np.all(np.diff(P[0][0])[rows_t] == 0)  # Dirichlet nodes: empty prolongator rows
        ref = Pl.T @ Al @ Pl
        absum = np.abs(Pl).T @ np.abs(Al) @ np.abs(Pl)
        terms = (Pl != 0).astype(np.float64).T @ (Al != 0).astype(np.float64) @ (Pl != 0).astype(np.float64)
        bound = (terms + 2) * LD(U) * absum
        err = np.abs(Ac - ref)
        on = Ac != 0
        print(f"  level {l + 1}: worst Galerkin error / bound {float((err[on] / bound[on]).max()):.3f}, "
              f"asymmetry / bound {float((np.abs(Ac - Ac.T)[on] / (2 * bound[on])).max()):.3f}")
        assert np.all(err <= bound)
        assert np.all(np.abs(Ac - Ac.T) <= 2 * bound)  # symmetric to rounding
    # P_0 = T - (omega / lambda) D^-1 A T from the fetched A_0, the aggregates and the reported lambda
    n = g.n_rows_t
    skip = np.zeros(n, dtype=np.uint8)
    skip[rows_t] = 1
    agg, n_agg = amg.aggregate(g.rowptr_tt, g.col_tt, skip)
    assert n_agg == info[1]["rows"]
    pptr, pcol, _ = P[0]
    for i in range(n):  # P's pattern is that of A T for these aggregates: their sizes read off it
        want = set() if agg[i] < 0 else {agg[k] for k in g.col_tt[g.rowptr_tt[i]:g.rowptr_tt[i + 1]] if agg[k] >= 0}
        assert set(pcol[pptr[i]:pptr[i + 1]]) == want, i
    size = np.bincount(agg[agg >= 0], minlength=n_agg)
    T = np.zeros((n, n_agg), dtype=LD)
    free = np.nonzero(agg >= 0)[0]
    T[free, agg[free]] = 1.0 / np.sqrt(size[agg[free]].astype(np.float64))  # the plan's float64 entries
    A0 = _dense(A[0], n)
    dinv = 1 / np.diag(A0)
    w = LD(a.opt.omega) / LD(info[0]["lmax"])
    ref = T - w * dinv[:, None] * (A0 @ T)
    absum = np.abs(T) + w * np.abs(dinv)[:, None] * (np.abs(A0) @ np.abs(T))
    terms = (A0 != 0).astype(np.float64) @ (T != 0).astype(np.float64)
    P0 = _dense(P[0], n_agg)
    on = P0 != 0
    bound = (terms + 2) * LD(U) * absum
    err = np.abs(P0 - ref)
    print(f"  P_0: worst error / bound {float((err[on] / bound[on]).max()):.3f}")
    assert np.all(ref[~on] == 0) and np.all(err <= bound)


# ------------------------------------------------------------------------ 3. the V-cycle
@gpu
def test_vcycle_is_the_operator_it_claims():
    name = "h8_433"
    mesh, _, tev, rows_s, rows_t = _case(name)
    a, A, P, info = _hierarchy(name, 0.0, coarse_max=4)
    d = _system(name, 0.0)[0]
    n = tev.graph.n_rows_t
    assert len(info) >= 3
    I = torch.eye(n, dtype=torch.float64, device=_dev())
    M = torch.full((n, n), float("nan"), dtype=torch.float64, device=_dev())  # row j = M e_j
    for j in range(n):
        a.apply(d["Ktt"], I[j], M[j])
    torch.cuda.synchronize()
    M = M.cpu().numpy().T
    rows = [i["rows"] for i in info]
    lmax = [i["lmax"] for i in info]
    ref = {}
    for dt in (np.float64, LD):
        Ad = [samg_ref.csr_dense(*A[l], rows[l], dt) for l in range(len(A))]
        Pd = [samg_ref.csr_dense(*P[l], rows[l + 1], dt) for l in range(len(P))]
        ref[dt] = samg_ref.Cycle(Ad, Pd, lmax, a.opt.nu, a.opt.ratio, a.opt.boost, dt).matrix()
    own = float(np.linalg.norm((ref[np.float64].astype(LD) - ref[LD]).astype(np.float64)))
    err = float(np.linalg.norm((M.astype(LD) - ref[LD]).astype(np.float64)))
    free = np.setdiff1d(np.arange(n), rows_t)
    Mff = M[np.ix_(free, free)]
    asym = float(np.linalg.norm(Mff - Mff.T))
    Aff = samg_ref.csr_dense(*A[0], n)[np.ix_(free, free)]
    L = np.linalg.cholesky(0.5 * (Aff + Aff.T))
    ev = np.linalg.eigvalsh(L.T @ (0.5 * (Mff + Mff.T)) @ L)
    print(f"V-cycle {name}: levels {rows}, |M - M_ld| {err:.3e}, |M_f64 - M_ld| {own:.3e}, "
          f"|M_ff - M_ff^T| {asym:.3e}, eig(M A_ff) in [{ev.min():.4f}, {ev.max():.4f}]")
    assert np.all(np.isfinite(M)) and err <= 8 * own
    assert asym <= 8 * own
    assert np.linalg.norm(Aff - Aff.T) <= 1e-13 * np.linalg.norm(Aff)
    assert ev.min() > 0


# --------------------------------------------------------------------- 4. solve against dense
@gpu
@pytest.mark.parametrize("name,opts", [(k, {"coarse_max": 8}) for k in SMALL] + [("h8_322", {})])
def test_solve_against_dense(name, opts):
    """coarse_max 8 gives every small mesh a coarse level; the default options leave h8_322 (36
    rows) with its smoother alone."""
    mesh, _, tev, rows_s, rows_t = _case(name)
    g = tev.graph
    d, h, bs, bt = _system(name, 1e-1)
    a = amg.ScalarAMG(tev, rows_t, **opts)
    rtol = 1e-10
    x1, x2 = _nan(g.n_rows_t), _nan(g.n_rows_t)
    it, rel = a.solve(d["Ktt"], _t(bt), x1, rtol)
    it2, _ = a.solve(d["Ktt"], _t(bt), x2, rtol)
    torch.cuda.synchronize()
    assert it == it2 and torch.equal(x1, x2)
    x = x1.cpu().numpy()
    assert np.all(np.isfinite(x)) and np.all(x[rows_t] == 0.0)
    y, ay = sr.csr_matvec_ld(g.rowptr_tt, g.col_tt, h["Ktt"], x)
    terms = np.diff(g.rowptr_tt)
    r = bt.astype(LD) - y
    res = float(np.sqrt((r * r).sum()))
    sigma = float(np.sqrt(((terms * LD(U) * ay) ** 2).sum()))
    nb = np.linalg.norm(bt)
    Ad = kr.csr_to_dense(g.rowptr_tt, g.col_tt, h["Ktt"])
    xd = np.linalg.solve(Ad, bt)
    cond = np.linalg.cond(Ad)
    err = np.linalg.norm(x - xd)
    print(f"samg solve {name} {opts}: levels {[i['rows'] for i in a.describe()]}, {it} steps, rel {rel:.3e}, "
          f"independent {res / nb:.3e}, err/|x| {err / np.linalg.norm(xd):.2e}, cond {cond:.2e}")
    assert rel <= rtol and res <= rtol * nb + sigma, (rel, res / nb, sigma / nb)
    assert err <= cond * rtol * np.linalg.norm(xd), (err, cond)


# ----------------------------------------------------------------- 5. the count stops growing
def _jacobi_pcg(ptr, col, vals, b, rtol, max_iter):
    """Jacobi-PCG from x = 0 in torch float64 on the device, stopping on the recurrence residual
    |r| <= rtol |b| as fcg_samg_solve's iteration does.  Returns the steps taken."""
    n = len(ptr) - 1
    rows = _t(np.repeat(np.arange(n), np.diff(ptr)))
    cols, v, b = _t(col, torch.int64), _t(vals), _t(b)
    diag = torch.zeros(n, dtype=torch.float64, device=_dev())
    on = rows == cols
    diag[rows[on]] = v[on]
    mv = lambda x: torch.zeros_like(x).index_add_(0, rows, v * x[cols])
    x, r = torch.zeros_like(b), b.clone()
    z = r / diag
    p, rz, bn = z.clone(), torch.dot(r, z), torch.linalg.norm(b)
    for it in range(1, max_iter + 1):
        q = mv(p)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= rtol * float(bn):
            return it
        z = r / diag
        rzn = torch.dot(r, z)
        p = z + (rzn / rz) * p
        rz = rzn
    return max_iter


_counts = {}


def _iteration_counts(name):
    if name not in _counts:
        mesh, _, tev, rows_s, rows_t = _case(name)
        g = tev.graph
        d, h, bs, bt = _system(name, 0.0)
        a = amg.ScalarAMG(tev, rows_t)  # default options
        x = _nan(g.n_rows_t)
        it, rel = a.solve(d["Ktt"], _t(bt), x, 1e-8)
        assert rel <= 1e-8 and bool(torch.isfinite(x).all())
        jac = _jacobi_pcg(g.rowptr_tt, g.col_tt, h["Ktt"], bt, 1e-8, 2000)
        _counts[name] = (it, jac, [i["rows"] for i in a.describe()], a.setup_ms[-1])
        a.close()
    return _counts[name]


@gpu
def test_iteration_count_no_longer_grows():
    """hex8 12^3 and 24^3 conduction (v = 0), rtol 1e-8, default options.  Measured on one MI355X:
    11 AMG-FCG steps at both sizes (levels 2197, 100 and 15625, 648, 27) against 57 and 108
    Jacobi-PCG steps; a CPU model of the algorithm had given 11 against 58 and 107."""
    a12, j12, l12, ms12 = _iteration_counts("h8_12")
    a24, j24, l24, ms24 = _iteration_counts("h8_24")
    print(f"12^3: levels {l12}, AMG-FCG {a12} steps, Jacobi-PCG {j12} steps (setup {ms12:.1f} ms); "
          f"24^3: levels {l24}, AMG-FCG {a24} steps, Jacobi-PCG {j24} steps (setup {ms24:.1f} ms)")
    assert 2 * a12 <= j12 and 2 * a24 <= j24
    assert a24 < j12
    assert len(l24) >= 3


# ------------------------------------------------------------------- 6. the monolithic solve
_amg_s = {}


def _native_amg(name, Kss, **opts):
    mesh, ev, tev, rows_s, rows_t = _case(name, struct=True)
    if name not in _amg_s:
        _amg_s[name] = amg.NativeAMG(mesh, ev, rows_s, **opts)
    _amg_s[name].setup(Kss)
    return _amg_s[name]


@gpu
@pytest.mark.parametrize("with_amg_s", [False, True])
@pytest.mark.parametrize("precond", ["diag", "bgs"])
@pytest.mark.parametrize("name", ["h8_322", "h8_333", "h27_221"])
def test_monolithic_solve_with_both_amgs(name, precond, with_amg_s):
    mesh, ev, tev, rows_s, rows_t = _case(name, struct=True)
    g = tev.graph
    d, h, bs, bt = _system(name, 1e-1, struct=True)
    at = amg.ScalarAMG(tev, rows_t, coarse_max=8)
    at.setup(d["Ktt"])
    as_ = _native_amg(name, d["Kss"], coarse_max=30) if with_amg_s else None  # a coarse level here too
    ns, nt = mesh.n_rows, g.n_rows_t
    xs, xt = _nan(ns), _nan(nt)
    rtol = 1e-10
    it, rel = tev.gmres_solve(ev, d["Kss"], d["Kst"], d["Kts"], d["Ktt"], _t(bs), _t(bt), xs, xt,
                              rtol=rtol, max_iter=3000, restart=128, precond=precond, amg=as_, amg_t=at)
    xs, xt = xs.cpu().numpy(), xt.cpu().numpy()
    x, b = np.concatenate([xs, xt]), np.concatenate([bs, bt])
    assert np.all(np.isfinite(x)) and np.all(xs[rows_s] == 0.0) and np.all(xt[rows_t] == 0.0)
    gr = {"Kss": (mesh.rowptr, mesh.col_lid), "Kst": (g.rowptr_st, g.col_st),
          "Kts": (g.rowptr_ts, g.col_ts), "Ktt": (g.rowptr_tt, g.col_tt)}
    out = {k: sr.csr_matvec_ld(gr[k][0], gr[k][1], h[k], v)
           for k, v in (("Kss", xs), ("Kst", xt), ("Kts", xs), ("Ktt", xt))}
    y = np.concatenate([out["Kss"][0] + out["Kst"][0], out["Kts"][0] + out["Ktt"][0]])
    ay = np.concatenate([out["Kss"][1] + out["Kst"][1], out["Kts"][1] + out["Ktt"][1]])
    terms = np.concatenate([np.diff(gr["Kss"][0]) + np.diff(gr["Kst"][0]),
                            np.diff(gr["Kts"][0]) + np.diff(gr["Ktt"][0])])
    r = b.astype(LD) - y
    res = float(np.sqrt((r * r).sum()))
    sigma = float(np.sqrt(((terms * LD(U) * ay) ** 2).sum()))
    nb = np.linalg.norm(b)
    A = np.block([[kr.csr_to_dense(*gr["Kss"], h["Kss"]), kr.csr_to_dense(*gr["Kst"], h["Kst"], nt)],
                  [kr.csr_to_dense(*gr["Kts"], h["Kts"], ns), kr.csr_to_dense(*gr["Ktt"], h["Ktt"])]])
    xd = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    err = np.linalg.norm(x - xd)
    print(f"tsi gmres + amg_t {name} {precond} amg_s={with_amg_s}: {it} steps, rel {rel:.3e}, "
          f"independent {res / nb:.3e}, err/|x| {err / np.linalg.norm(xd):.2e}, cond {cond:.2e}")
    assert rel <= rtol and res <= rtol * nb + sigma, (rel, res / nb, sigma / nb)
    assert err <= cond * rtol * np.linalg.norm(xd), (err, cond)


@gpu
def test_monolithic_steps_drop_with_the_thermal_amg():
    """hex8 12^3, v = 0, NativeAMG on K_SS, block Gauss-Seidel: fewer FGMRES steps with the
    thermal V-cycle than with the diagonal of K_TT."""
    name = "h8_12"
    mesh, ev, tev, rows_s, rows_t = _case(name, struct=True)
    g = tev.graph
    d, h, bs, bt = _system(name, 0.0, struct=True)
    as_ = _native_amg(name, d["Kss"])
    at = amg.ScalarAMG(tev, rows_t)
    at.setup(d["Ktt"])
    steps = {}
    for tag, t in (("jacobi", None), ("amg_t", at)):
        xs, xt = _nan(mesh.n_rows), _nan(g.n_rows_t)
        it, rel = tev.gmres_solve(ev, d["Kss"], d["Kst"], d["Kts"], d["Ktt"], _t(bs), _t(bt), xs, xt,
                                  rtol=1e-8, max_iter=3000, restart=50, precond="bgs", amg=as_, amg_t=t)
        assert rel <= 1e-8 and bool(torch.isfinite(xs).all()) and bool(torch.isfinite(xt).all())
        steps[tag] = it
    print(f"monolithic 12^3, AMG_S, bgs: {steps['jacobi']} steps with diag K_TT, {steps['amg_t']} with AMG_T")
    assert steps["amg_t"] < steps["jacobi"]


# ------------------------------------------------------------------------- 7. known answers
_dense_ans = {}


def _dense_answer(name):
    if name not in _dense_ans:
        prob = TsiProblem(json.load(open(os.path.join(GOLD, name))))
        d, T = prob.solve()
        _dense_ans[name] = (prob, d, T, sum(h["iterations"] for h in prob.history))
    return _dense_ans[name]


@gpu
@pytest.mark.parametrize("name,newton_total", [("tsi_heatflux_monolithic.json", 20),
                                               ("tsi_heatflux_flexoutsurf_monolithic.json", 25)])
def test_known_answers_with_the_thermal_amg(name, newton_total):
    _dev()
    prob, d_ref, T_ref, n_ref = _dense_answer(name)
    assert n_ref == newton_total
    dis = fcg.Discretization.from_elements(prob.celltype, prob.elements, prob.X, lattice=False)
    ev = fcg.Evaluator(dis, kinematics=fcg.LINEAR, youngs=prob.E, poisson=prob.nu)
    tev = fcg.TsiEvaluator(dis, prob.E, prob.nu, prob.alpha, prob.T0, prob.conduct)
    at = amg.ScalarAMG(tev, prob.dbc_t, coarse_max=8)
    run = tsi.TsiMonolithic(ev, tev, prob.dt, prob.fext_s, prob.fext_t, prob.dbc_s, prob.dbc_t,
                            T_init=prob.T_init, fused=False, amg_t=at)
    d, T = run.run(prob.nstep)
    d, T = d.cpu().numpy(), T.cpu().numpy()
    for r in prob.fx["results"]:
        got = prob.result(d, T, r)
        assert abs(got - r["value"]) <= r["tol"], (r, got)
    ed = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    eT = np.linalg.norm(T - T_ref) / np.linalg.norm(T_ref)
    its = [n for h in run.history for n in h["gmres_iterations"]]
    print(f"{name} amg_t levels {[i['rows'] for i in at.describe()]}: |dd|/|d| {ed:.2e}, |dT|/|T| {eT:.2e}, "
          f"GMRES steps per solve max {max(its)}, Newton {sum(h['iterations'] for h in run.history)}")
    assert ed <= 1e-9 and eT <= 1e-10
    assert sum(h["iterations"] for h in run.history) == newton_total
    assert max(its) <= run.lin_max_iter
    with pytest.raises(ValueError):  # the thermal Dirichlet rows are checked at construction
        tsi.TsiMonolithic(ev, tev, prob.dt, prob.fext_s, prob.fext_t, prob.dbc_s, prob.dbc_t[:-1], amg_t=at)


# ------------------------------------------------------------------------------ 8. refusals
@gpu
def test_refusals():
    name = "h8_322"
    mesh, ev, tev, rows_s, rows_t = _case(name, struct=True)
    g = tev.graph
    d, h, bs, bt = _system(name, 1e-1, struct=True)
    # a rank of a partition
    rank = fcg.BoxMesh(fcg.HEX8, (4, 2, 2), rank=0, nranks=2)
    rtev = fcg.TsiEvaluator(rank, E, NU, ALPHA, T0, COND)
    with pytest.raises(fcg.FcgError) as e:
        amg.ScalarAMG(rtev, np.zeros(0, dtype=np.int32))
    assert e.value.code == FCG_ERR_ARG
    # a Dirichlet row outside the map
    for bad in (g.n_rows_t, -1):
        with pytest.raises(fcg.FcgError) as e:
            amg.ScalarAMG(tev, np.array([0, bad], dtype=np.int32))
        assert e.value.code == FCG_ERR_ARG
    # apply and solve before any setup
    a = amg.ScalarAMG(tev, rows_t, coarse_max=8)
    for call in (lambda: a.apply(d["Ktt"], _t(bt), _nan(g.n_rows_t)),
                 lambda: a.solve(d["Ktt"], _t(bt), _nan(g.n_rows_t), 1e-8, setup=False)):
        with pytest.raises(fcg.FcgError) as e:
            call()
        assert e.value.code != 0 and "fcg_samg_setup" in str(e.value)
        assert b"setup" in fcg.lib().fcg_samg_last_error(a._h)
    with pytest.raises(RuntimeError):
        a.level_matrix(0, 0)
    # an all-zero K_TT
    with pytest.raises(fcg.FcgError) as e:
        a.setup(torch.zeros_like(d["Ktt"]))
    assert e.value.code == FCG_ERR_SINGULAR
    with pytest.raises(fcg.FcgError):  # ... leaves the handle without a setup
        a.apply(d["Ktt"], _t(bt), _nan(g.n_rows_t))
    # a handle made on another thermo context
    tev2 = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND)
    other = amg.ScalarAMG(tev2, rows_t, coarse_max=8)
    other.setup(d["Ktt"])
    args = (ev, d["Kss"], d["Kst"], d["Kts"], d["Ktt"], _t(bs), _t(bt))
    with pytest.raises(fcg.FcgError) as e:
        tev.gmres_solve(*args, _nan(len(bs)), _nan(len(bt)), amg_t=other)
    assert e.value.code == FCG_ERR_ARG
    # without amg_t nothing changes: the old entry and the new one with NULL give the same bits
    xs1, xt1, xs2, xt2 = _nan(len(bs)), _nan(len(bt)), _nan(len(bs)), _nan(len(bt))
    it1, rel1 = tev.gmres_solve(*args, xs1, xt1, rtol=1e-10, max_iter=3000, restart=50, precond="bgs")
    opt = fcg.gmres_options(50, 3000, 1e-10, 1)
    it2, rel2 = ctypes.c_int(0), ctypes.c_double(0.0)
    rc = fcg.lib().fcg_tsi_gmres_solve_amg(ev._h, tev._h, None, None, *[_p(t) for t in args[1:]], _p(xs2),
                                           _p(xt2), ctypes.byref(opt), ctypes.byref(it2),
                                           ctypes.byref(rel2), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and it2.value == it1 and rel2.value == rel1
    assert torch.equal(xs1, xs2) and torch.equal(xt1, xt2)
