"""The solver primitives every Newton step runs around the evaluate (4c_amd/csrc/fcg_solver.hip:
fcg_spmv, fcg_spmv_f32, fcg_dirichlet_apply, fcg_block_jacobi_setup / apply, fcg_chebyshev_step,
fcg_pcg_solve) against the extended-precision references of tests/solver_ref.py, on the smallest
meshes that reach each code shape (solver_ref's mesh builders).

Unless a test says otherwise K is no physical tangent: seeded standard-normal values on the mesh's
graph with + 4 on every node's own diagonal (solver_ref.random_values) -- every entry distinct,
nothing symmetric, so an index or transpose slip cannot cancel -- and output buffers start as NaN.

Bounds (u = 2^-53; derived, not tuned):
  SpMV                |y - y_ref|_i <= (len_i + 2) u (|K||x|)_i: a dot product of len_i terms in any
                      order of summation; fused multiply-adds only tighten it.
  block inverse       per block e = max|dinv - ref| / (kappa_inf u max|ref|); the kernel's largest e
                      at most 4 x the largest e of the float64 replay of its cofactor formula
                      (another order of operations, contraction); every kappa_inf <= 1e3 asserted.
  block-Jacobi apply  4 u (|scale| (|dinv||r|)_i + |z0_i|), against the GPU's own dinv.
  Chebyshev step      8 u (|c_r| (|dinv|(|b| + |y|))_i + |c_d d_i| + |x_i|).
  PCG                 true residual <= rtol + 10 g, g the float64 replay's gap between its true and
                      its recurrence residual; 5 iterations: within 10 x the float64 replay's
                      distance from the longdouble replay.

Measured on one MI355X with the change that added this file (on top of commit b03713a); the tests
print the figures again with -s:
  block inverse, max e per mesh    h8box   h27box  fan     h8renum
    fcg_block_jacobi_setup         1.322   0.992   0.439   0.802
    float64 replay of the formula  1.242   1.284   0.667   1.287
  PCG rtol 1e-8, |true - reported residual|   h8box     h27box    h8renum
    fcg_pcg_solve                             1.2e-16   6.5e-16   3.5e-17
    float64 replay (g)                        1.6e-16   1.1e-15   8.4e-17
  (56 / 80 / 56 iterations, the replay's counts; true residuals 3.4e-10, 6.5e-10, 1.2e-10.)
"""

import ctypes
import importlib

import numpy as np
import pytest

import solver_ref as sr
from parity_util import oracle_evaluate, oracle_evaluate_single, rel_err

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

LD, U = sr.LD, sr.U
E, NU = 210.0, 0.3


# ============================================================ the reference module itself (CPU)
def test_csr_matvec_ld_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    for m in (sr.h8box(), sr.h8rank(), sr.orphan()):
        v = sr.random_values(m, 1)
        x = np.random.default_rng(2).standard_normal(m.n_cols)
        A = sp.csr_matrix((v, m.col_lid, m.rowptr), shape=(m.n_rows, m.n_cols))
        y, absy = sr.csr_matvec_ld(m.rowptr, m.col_lid, v, x)
        assert y.dtype == LD and absy.dtype == LD
        lens = np.diff(m.rowptr)
        assert np.all(np.abs(A @ x - y.astype(np.float64)) <= (lens + 2) * U * absy.astype(np.float64))
        assert np.allclose(absy.astype(np.float64), abs(A) @ np.abs(x), rtol=1e-14, atol=0)
        y32, _ = sr.csr_matvec_ld(m.rowptr, m.col_lid, v.astype(np.float32), x)
        A32 = sp.csr_matrix((v.astype(np.float32).astype(np.float64), m.col_lid, m.rowptr),
                            shape=(m.n_rows, m.n_cols))
        assert np.all(np.abs(A32 @ x - y32.astype(np.float64)) <= (lens + 2) * U * absy.astype(np.float64) * 1.001)


def test_block_inverse_references_agree():
    m = sr.h8box()
    v = sr.apply_dirichlet_host(m, sr.random_values(m, 1), sr.dirichlet_rows(m))
    D, inv, kappa, ok = sr.block_inverse_ld(m, v)
    assert ok.all() and kappa.max() <= 1e3
    eye = np.einsum("kij,kjl->kil", D, inv)
    assert np.abs(eye - np.eye(3)).max() <= 1e-16
    o = sr.cofactor_inverse_f64(D.astype(np.float64)).reshape(-1, 3, 3)
    e = np.abs(o - inv).max(axis=(1, 2)) / (kappa * U * np.abs(inv).max(axis=(1, 2)))
    assert e.max() <= 4.0, e.max()
    # a roller block is unsymmetric through its unit row
    assert np.abs(D - D.transpose(0, 2, 1)).max() > 1.0


def _physical_host(mesh):
    err, _, K, _ = oracle_evaluate(mesh, fcg.LINEAR, E, NU, np.zeros(mesh.n_cols))
    assert err == 0
    return K


def test_pcg_replay_converges():
    spla = pytest.importorskip("scipy.sparse.linalg")
    sp = pytest.importorskip("scipy.sparse")
    m = sr.h8box()
    rows = sr.dirichlet_rows(m)
    K = sr.apply_dirichlet_host(m, _physical_host(m), rows)
    b = np.random.default_rng(4).standard_normal(m.n_rows)
    b[rows] = 0.0
    D, inv, _, ok = sr.block_inverse_ld(m, K)
    assert ok.all()
    d64 = sr.cofactor_inverse_f64(D.astype(np.float64))
    x, it, rec, true = sr.pcg_replay(m, K, b, d64, 1e-8, 1000)
    assert it % 8 == 0 and 0 < it < 1000 and rec <= 1e-8 and true <= 2e-8
    ref = spla.spsolve(sp.csr_matrix((K, m.col_lid, m.rowptr), shape=(m.n_rows, m.n_cols)).tocsc(), b)
    assert rel_err(x, ref) <= 1e-6
    assert np.all(x[rows] == 0.0)
    xl, itl, _, _ = sr.pcg_replay(m, K, b, inv, 1e-8, 5, dtype=LD)
    x5, it5, rec5, _ = sr.pcg_replay(m, K, b, d64, 1e-8, 5)
    assert itl == it5 == 5 and rec5 > 1e-8
    assert 0 < np.abs(x5 - xl.astype(np.float64)).max() <= 1e-12 * np.abs(x5).max()


def test_fan_passes_the_oracle_element_by_element():
    f = sr.fan()
    assert sorted(set(np.diff(f.rowptr).tolist())) == [24, 36, 66]
    u = 1e-3 * np.random.default_rng(1).standard_normal(f.n_cols)
    for kin in (fcg.LINEAR, fcg.TOTLAG):
        assert oracle_evaluate_single(f, kin, E, NU, u)[0] == 0
        for e in range(f.n_ele):
            one = fcg.Discretization.from_elements(fcg.HEX8, f.ele_nodes[e:e + 1] * 0 + np.arange(8),
                                                   f.node_x[f.ele_nodes[e]])
            assert oracle_evaluate_single(one, kin, E, NU, np.zeros(24))[0] == 0
    assert np.diff(sr.fan(2).rowptr).max() == 99
    x = sr.extra()
    assert [int(n) for n in np.diff(x.rowptr)[[3 * a for a, _ in x.added]]] == [25, 25, 25]


# ======================================================================================= GPU
gpu = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


MESHES = {
    "h8box": (sr.h8box, fcg.PATH_AUTO), "h27box": (sr.h27box, fcg.PATH_AUTO),
    "h8rank": (sr.h8rank, fcg.PATH_AUTO), "h8rank_strict": (lambda: sr.h8rank(True), fcg.PATH_AUTO),
    "h8renum_gather": (sr.h8renum, fcg.PATH_GATHER), "h8renum_general": (sr.h8renum, fcg.PATH_GENERAL),
    "fan": (sr.fan, fcg.PATH_AUTO), "extra": (sr.extra, fcg.PATH_GENERAL),
    "orphan": (sr.orphan, fcg.PATH_GENERAL),
}
_cache = {}


def _ctx(name):
    """(mesh, evaluator, random K) of a named mesh, built once per session and left unchanged."""
    _dev()
    if name not in _cache:
        build, path = MESHES[name]
        mesh = build()
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=path)
        if path != fcg.PATH_AUTO:
            assert ev.info.path == path
        _cache[name] = (mesh, ev, sr.random_values(mesh, 1))
    return _cache[name]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t if dtype is None else t.to(dtype)


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


def _h(t):
    return t.cpu().numpy()


def _stream(ev):
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device("cuda", ev.device)).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bj_setup(ev, K, dinv):
    return fcg.lib().fcg_block_jacobi_setup(ev._h, _p(K), _p(dinv), _stream(ev))


def _bj_apply(ev, dinv, r, z, scale, accumulate):
    return fcg.lib().fcg_block_jacobi_apply(ev._h, _p(dinv), _p(r), _p(z), float(scale),
                                            int(accumulate), _stream(ev))


def _cheb(ev, dinv, b, y, d, x, c_d, c_r, mode):
    return fcg.lib().fcg_chebyshev_step(ev._h, _p(dinv), _p(b), _p(y), _p(d), _p(x), float(c_d),
                                        float(c_r), int(mode), _stream(ev))


def _last_error(ev):
    return fcg.lib().fcg_last_error(ev._h).decode()


# ------------------------------------------------------------------------------------- 1. SpMV
def _check_spmv(name, f32, stream=None, twice=False):
    mesh, ev, v = _ctx(name)
    vals = v.astype(np.float32) if f32 else v
    x = np.random.default_rng(2).standard_normal(mesh.n_cols)
    K, xt = _t(vals), _t(x)
    run = ev.spmv_f32 if f32 else ev.spmv
    y = _nan(mesh.n_rows)
    if stream is None:
        run(K, xt, y)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            run(K, xt, y)
        stream.synchronize()
    torch.cuda.synchronize()
    yr, absy = sr.csr_matvec_ld(mesh.rowptr, mesh.col_lid, vals, x)
    err = np.abs(_h(y).astype(LD) - yr)
    bound = (np.diff(mesh.rowptr) + 2) * LD(U) * absy
    worst = float((err / np.where(bound > 0, bound, 1)).max())
    print(f"spmv {name} f32={f32}: worst error / bound = {worst:.3f}")
    assert np.all(np.isfinite(_h(y)))
    assert np.all(err <= bound), (name, f32, int(np.argmax(err - bound)), worst)
    if twice:
        y2 = _nan(mesh.n_rows)
        run(K, xt, y2)
        assert torch.equal(y, y2)


@gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", [n for n in MESHES if n != "extra"])
def test_spmv_componentwise(name, f32):
    """y = K x with ghost columns carrying x, rows 0 .. 375 long, both value types."""
    _check_spmv(name, f32)


@gpu
def test_spmv_stream_and_reproducible():
    _dev()
    _check_spmv("h27box", False, stream=torch.cuda.Stream())
    _check_spmv("h8renum_gather", True, twice=True)
    _check_spmv("h27box", False, twice=True)


# --------------------------------------------------------------------------- 2. Dirichlet rows
DBC_MESHES = ["h8box", "h27box", "fan", "h8rank"]


def _rows_of_entries(mesh):
    return np.repeat(np.arange(mesh.n_rows), np.diff(mesh.rowptr))


@gpu
@pytest.mark.parametrize("name", DBC_MESHES)
def test_dirichlet_rows_exact(name):
    mesh, ev, v = _ctx(name)
    rows = sr.dirichlet_rows(mesh)
    rt = _t(rows)
    rhs0 = np.random.default_rng(6).standard_normal(mesh.n_rows)
    Kref = sr.apply_dirichlet_host(mesh, v, rows)
    rhs_ref = rhs0.copy()
    rhs_ref[rows] = 0.0
    isd = np.isin(_rows_of_entries(mesh), rows)
    own = sr.col_of_row(mesh)[_rows_of_entries(mesh)]
    # the reference's unit rows: 1 on the row's own column, 0 elsewhere, the rest untouched
    assert np.all(Kref[isd & (mesh.col_lid == own)] == 1.0) and np.array_equal(Kref[~isd], v[~isd])

    K, rhs, fr = _t(v), _t(rhs0), _nan(mesh.n_rows)
    ev.dirichlet_apply(rt, K, rhs, fr)
    assert np.array_equal(_h(K), Kref)
    assert np.array_equal(_h(rhs), rhs_ref)
    frh = _h(fr)
    assert np.array_equal(frh[rows], -rhs0[rows])
    assert np.all(np.isnan(np.delete(frh, rows)))  # written on the Dirichlet rows only

    K = _t(v)  # K only
    ev.dirichlet_apply(rt, K, None, None)
    assert np.array_equal(_h(K), Kref)
    rhs, fr = _t(rhs0), _nan(mesh.n_rows)  # rhs and freact, no K
    ev.dirichlet_apply(rt, None, rhs, fr)
    assert np.array_equal(_h(rhs), rhs_ref) and np.array_equal(_h(fr)[rows], -rhs0[rows])
    rhs = _t(rhs0)  # rhs without freact
    ev.dirichlet_apply(rt, None, rhs, None)
    assert np.array_equal(_h(rhs), rhs_ref)

    K, rhs = _t(v), _t(rhs0)  # n_dbc = 0
    ev.dirichlet_apply(rt[:0], K, rhs, None)
    assert np.array_equal(_h(K), v) and np.array_equal(_h(rhs), rhs0)


@gpu
@pytest.mark.parametrize("name", DBC_MESHES)
@pytest.mark.parametrize("bad", ["below", "above"])
def test_dirichlet_row_outside_the_map(name, bad):
    mesh, ev, v = _ctx(name)
    rows = sr.dirichlet_rows(mesh)
    rhs0 = np.random.default_rng(6).standard_normal(mesh.n_rows)
    lst = np.concatenate([rows[:3], [-1 if bad == "below" else mesh.n_rows], rows[3:]]).astype(np.int32)
    K, rhs = _t(v), _t(rhs0)
    with pytest.raises(fcg.FcgError, match="out of range") as ei:
        ev.dirichlet_apply(_t(lst), K, rhs, None)
    assert ei.value.code == fcg.FCG_ERR_ARG
    isd = np.isin(_rows_of_entries(mesh), rows)
    assert np.array_equal(_h(K)[~isd], v[~isd])
    assert np.array_equal(np.delete(_h(rhs), rows), np.delete(rhs0, rows))
    # the valid rows of the list are applied all the same (include/fourc_gpu.h)
    assert np.array_equal(_h(K), sr.apply_dirichlet_host(mesh, v, rows)) and np.all(_h(rhs)[rows] == 0)


@gpu
def test_dirichlet_row_without_diagonal():
    mesh, ev, v = _ctx("orphan")
    K = _t(v)
    with pytest.raises(fcg.FcgError, match="without a diagonal entry") as ei:
        ev.dirichlet_apply(_t(np.array([0, mesh.orphan_row0 + 1], dtype=np.int32)), K, None, None)
    assert ei.value.code == fcg.FCG_ERR_ARG


# ------------------------------------------------------------------------------ 3. block Jacobi
def _dbc_values(name):
    mesh, ev, v = _ctx(name)
    return sr.apply_dirichlet_host(mesh, v, sr.dirichlet_rows(mesh))


def _block_ratios(mesh, vals, dinv_gpu, select=None):
    """(max e of the GPU inverses, max e of the float64 cofactor replay, reference) over the
    non-singular blocks (`select`: a mask of blocks to look at)."""
    D, inv, kappa, ok = sr.block_inverse_ld(mesh, vals)
    sel = ok if select is None else ok & select
    assert kappa[sel].max() <= 1e3, kappa[sel].max()
    scale = (kappa * U)[sel] * np.abs(inv[sel]).max(axis=(1, 2)).astype(np.float64)
    g = dinv_gpu.reshape(-1, 3, 3)[sel].astype(LD)
    f = sr.cofactor_inverse_f64(D.astype(np.float64)).reshape(-1, 3, 3)[sel].astype(LD)
    e_gpu = (np.abs(g - inv[sel]).max(axis=(1, 2)).astype(np.float64) / scale).max()
    e_f64 = (np.abs(f - inv[sel]).max(axis=(1, 2)).astype(np.float64) / scale).max()
    return float(e_gpu), float(e_f64), ok


BJ_MESHES = ["h8box", "h27box", "fan", "h8renum_gather"]


@gpu
@pytest.mark.parametrize("name", BJ_MESHES)
def test_block_jacobi_setup_and_apply(name):
    mesh, ev, _ = _ctx(name)
    vals = _dbc_values(name)
    row0, _ = sr.row_nodes(mesh)
    nn = len(row0)
    dinv = _nan(9 * nn)
    assert _bj_setup(ev, _t(vals), dinv) == fcg.FCG_OK, _last_error(ev)
    dh = _h(dinv)
    e_gpu, e_f64, ok = _block_ratios(mesh, vals, dh)
    print(f"block inverse {name}: max e GPU {e_gpu:.3f}, float64 replay {e_f64:.3f}")
    assert ok.all() and np.all(np.isfinite(dh))
    assert e_gpu <= 4.0 * e_f64, (e_gpu, e_f64)

    r = np.random.default_rng(7).standard_normal(mesh.n_rows)
    z0 = np.random.default_rng(8).standard_normal(mesh.n_rows)
    absz = sr.block_apply(np.abs(dh), row0, np.abs(r))
    for scale, acc in ((0.5, 1), (1.0, 0)):
        z = _t(z0) if acc else _nan(mesh.n_rows)
        assert _bj_apply(ev, dinv, _t(r), z, scale, acc) == fcg.FCG_OK
        base = z0.astype(LD) if acc else np.zeros(mesh.n_rows, dtype=LD)
        ref = LD(scale) * sr.block_apply(dh, row0, r) + base
        bound = 4 * LD(U) * (abs(scale) * absz + np.abs(base))
        err = np.abs(_h(z).astype(LD) - ref)
        assert np.all(err <= bound), (scale, acc, float((err / bound).max()))


@gpu
def test_block_jacobi_singular_blocks():
    mesh, ev, _ = _ctx("h8box")
    vals = _dbc_values("h8box")
    pos = sr.diag_block_positions(mesh)
    good = _nan(9 * len(pos))
    assert _bj_setup(ev, _t(vals), good) == fcg.FCG_OK
    k = 17
    sing = vals.copy()
    sing[pos[k].ravel()] = 0.0
    dinv = _nan(9 * len(pos))
    assert _bj_setup(ev, _t(sing), dinv) == fcg.FCG_ERR_SINGULAR
    assert "singular" in _last_error(ev)
    dh, gh = _h(dinv).reshape(-1, 9), _h(good).reshape(-1, 9)
    assert np.all(dh[k] == 0.0) and np.array_equal(np.delete(dh, k, axis=0), np.delete(gh, k, axis=0))

    # a node no element holds: its rows have no diagonal entry
    mesh, ev, v = _ctx("orphan")
    dinv = _nan(3 * mesh.n_rows)
    assert _bj_setup(ev, _t(v), dinv) == fcg.FCG_ERR_SINGULAR
    dh = _h(dinv)
    e_gpu, e_f64, ok = _block_ratios(mesh, v, dh)
    assert list(np.nonzero(~ok)[0]) == [mesh.n_rows // 3 - 1]
    assert np.all(dh.reshape(-1, 9)[-1] == 0.0) and np.all(np.isfinite(dh))
    assert e_gpu <= 4.0 * e_f64, (e_gpu, e_f64)


# --------------------------------------------------------------------------- 4. Chebyshev step
@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["h8box", "h27box"])
def test_chebyshev_step_against_the_formula(name, mode):
    mesh, ev, _ = _ctx(name)
    row0, _ = sr.row_nodes(mesh)
    dinv = _nan(3 * mesh.n_rows)
    assert _bj_setup(ev, _t(_dbc_values(name)), dinv) == fcg.FCG_OK
    dh = _h(dinv)
    rng = np.random.default_rng(9)
    b, y, d0, x0 = (rng.standard_normal(mesh.n_rows) for _ in range(4))
    c_d, c_r = 0.37, -1.3
    yt = _nan(mesh.n_rows) if mode == 2 else _t(y)  # mode 2 does not read y
    dt, xt = _t(d0), _t(x0)
    assert _cheb(ev, dinv, _t(b), yt, dt, xt, c_d, c_r, mode) == fcg.FCG_OK
    res = b.astype(LD) if mode == 2 else b.astype(LD) - y.astype(LD)
    d_ref = LD(c_r) * sr.block_apply(dh, row0, res)
    if mode == 1:
        d_ref = d_ref + LD(c_d) * d0.astype(LD)
    x_ref = d_ref if mode == 2 else x0.astype(LD) + d_ref
    mag = np.abs(b) if mode == 2 else np.abs(b) + np.abs(y)
    bound = abs(c_r) * sr.block_apply(np.abs(dh), row0, mag)
    if mode == 1:
        bound = bound + abs(c_d) * np.abs(d0)
    if mode != 2:
        bound = bound + np.abs(x0)
    bound = 8 * LD(U) * bound
    for got, ref in ((dt, d_ref), (xt, x_ref)):
        err = np.abs(_h(got).astype(LD) - ref)
        assert np.all(np.isfinite(_h(got))) and np.all(err <= bound), float((err / bound).max())


@gpu
@pytest.mark.parametrize("mode", [-1, 3])
def test_chebyshev_step_refuses_other_modes(mode):
    mesh, ev, _ = _ctx("h8box")
    v = [_t(np.ones(mesh.n_rows)) for _ in range(4)]
    dinv = _t(np.ones(3 * mesh.n_rows))
    assert _cheb(ev, dinv, v[0], v[1], v[2], v[3], 0.5, 0.5, mode) == fcg.FCG_ERR_ARG
    assert np.all(_h(v[2]) == 1.0) and np.all(_h(v[3]) == 1.0)


# --------------------------------------------------------------------------------------- 5. PCG
_pcg_cache = {}


def _pcg_problem(name):
    """Physical linear K of the mesh after its Dirichlet rows (device and host copies), b random
    and zero on those rows, the float64 / longdouble block inverses of the host copy."""
    if name not in _pcg_cache:
        mesh, ev, _ = _ctx(name)
        dev = _dev()
        rows = sr.dirichlet_rows(mesh)
        K = _nan(mesh.nnz)
        f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=dev)
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE,
                           torch.zeros(mesh.n_cols, dtype=torch.float64, device=dev), f, K)
        ev.dirichlet_apply(_t(rows), K, None, None)
        b = np.random.default_rng(4).standard_normal(mesh.n_rows)
        b[rows] = 0.0
        Kh = _h(K)
        D, inv, _, ok = sr.block_inverse_ld(mesh, Kh)
        assert ok.all()
        _pcg_cache[name] = (mesh, ev, K, Kh, b, rows, sr.cofactor_inverse_f64(D.astype(np.float64)), inv)
    return _pcg_cache[name]


PCG_MESHES = ["h8box", "h27box", "h8renum_gather"]


def _check_pcg_rtol(name, rtol=1e-8):
    mesh, ev, K, Kh, b, rows, d64, _ = _pcg_problem(name)
    x = _nan(mesh.n_rows)
    it, rel = ev.pcg_solve(K, _t(b), x, rtol=rtol, max_iter=2000)
    xr, it_r, rec_r, true_r = sr.pcg_replay(mesh, Kh, b, d64, rtol, 2000)
    g = abs(true_r - rec_r)
    true = sr.true_residual(mesh, Kh, b, _h(x))
    print(f"pcg {name}: it {it} (replay {it_r}), reported {rel:.3e}, true {true:.3e}, "
          f"gap GPU {abs(true - rel):.3e}, gap float64 replay {g:.3e}")
    assert rel <= rtol, rel
    assert it % 8 == 0 and abs(it - 8 * -(-it_r // 8)) <= 8, (it, it_r)
    assert true <= rtol + 10 * g, (true, rel, g)
    assert np.all(_h(x)[rows] == 0.0)
    return x


@gpu
@pytest.mark.parametrize("name", PCG_MESHES)
def test_pcg_to_tolerance(name):
    x1 = _check_pcg_rtol(name)
    mesh, ev, K, Kh, b, rows, d64, _ = _pcg_problem(name)
    x2 = _nan(mesh.n_rows)
    ev.pcg_solve(K, _t(b), x2, rtol=1e-8, max_iter=2000)
    assert torch.equal(x1, x2)  # bitwise reproducible


@gpu
@pytest.mark.parametrize("name", PCG_MESHES)
def test_pcg_iteration_caps_and_zero_rhs(name):
    mesh, ev, K, Kh, b, rows, d64, inv = _pcg_problem(name)
    rtol = 1e-8
    x = _nan(mesh.n_rows)
    it, rel = ev.pcg_solve(K, _t(b), x, rtol=rtol, max_iter=5)
    assert it == 5 and rel > rtol
    xl, itl, _, _ = sr.pcg_replay(mesh, Kh, b, inv, rtol, 5, dtype=LD)
    x5, it5, _, _ = sr.pcg_replay(mesh, Kh, b, d64, rtol, 5)
    assert itl == 5 and it5 == 5
    dist_f64 = float(np.abs(x5.astype(LD) - xl).max())
    dist_gpu = float(np.abs(_h(x).astype(LD) - xl).max())
    print(f"pcg {name}, 5 iterations: |x - x_ld|_max GPU {dist_gpu:.3e}, float64 replay {dist_f64:.3e}")
    assert dist_f64 > 0 and dist_gpu <= 10 * dist_f64, (dist_gpu, dist_f64)

    x = _nan(mesh.n_rows)
    it, rel = ev.pcg_solve(K, _t(b), x, rtol=rtol, max_iter=0)
    assert it == 0 and rel == 1.0 and np.all(_h(x) == 0.0)

    x = _nan(mesh.n_rows)
    it, rel = ev.pcg_solve(K, torch.zeros(mesh.n_rows, dtype=torch.float64, device=_dev()), x,
                           rtol=rtol, max_iter=100)
    assert it == 0 and np.all(_h(x) == 0.0)


@gpu
def test_pcg_refuses_a_rank_of_a_partition():
    mesh, ev, v = _ctx("h8rank")
    x = _nan(mesh.n_rows)
    with pytest.raises(fcg.FcgError, match="single-rank") as ei:
        ev.pcg_solve(_t(v), _t(np.ones(mesh.n_rows)), x)
    assert ei.value.code == fcg.FCG_ERR_ARG


# --------------------------------------------------------------------- 6. contexts without rows
@gpu
def test_contexts_without_rows_are_no_ops():
    dev = _dev()
    dsolve = importlib.import_module("4c_amd.dsolve")
    empty = [m for m in (fcg.BoxMesh(fcg.HEX8, (2, 1, 1), rank=r, nranks=5) for r in range(5))
             if m.n_ele == 0]
    assert empty and empty[0].n_rows == 0
    mesh = empty[0]
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    e = lambda dt=torch.float64: torch.empty(0, dtype=dt, device=dev)
    assert e().data_ptr() == 0
    assert _bj_setup(ev, e(), e()) == fcg.FCG_OK, _last_error(ev)
    assert _bj_apply(ev, e(), e(), e(), 1.0, 0) == fcg.FCG_OK
    for mode in (0, 1, 2):
        assert _cheb(ev, e(), e(), e(), e(), e(), 0.5, 0.5, mode) == fcg.FCG_OK
    ev.dirichlet_apply(e(torch.int32), e(), e(), e())
    ev.spmv(e(), e(), e())
    ev.spmv_f32(e(torch.float32), e(), e())
    assert ev.pcg_solve(e(), e(), e(), rtol=1e-8, max_iter=10) == (0, 0.0)
    pcg = dsolve.DistributedPCG(ev, dsolve.Transport(None, staged=True))
    assert pcg.solve(e(), e(), e(), rtol=1e-8, max_iter=10) == (0, 0.0)


# ------------------------------------------------------------------ 7. duplicate Dirichlet rows
@gpu
def test_static_newton_with_duplicate_dirichlet_rows():
    newton = importlib.import_module("4c_amd.newton")
    mesh, ev, _ = _ctx("h8box")
    rows = sr.dirichlet_rows(mesh)
    fext = 1e-3 * np.random.default_rng(12).standard_normal(mesh.n_rows)
    out = []
    for lst in (rows, np.concatenate([rows, rows[:7]])):
        nt = newton.StaticNewton(ev, fext, lst, tol_res=1e-9, tol_inc=1e-9, lin_rtol=1e-12)
        u = nt.solve()
        assert nt.dbc.numel() == len(rows)
        out.append((_h(u).copy(), _h(nt.freact).copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    # reactions at every Dirichlet row: -(f_int - f_ext), not the -0.0 a second pass would store
    assert np.all(out[1][1][rows] != 0.0)


# -------------------------------------------------------------------- 8. fan and the row limit
def _check_oracle(Kg, fg, Kr, fr):
    """test_gpu_parity._check's bounds."""
    assert rel_err(fg, fr) <= 1e-10, rel_err(fg, fr)
    assert np.all(np.isfinite(Kg))
    assert rel_err(Kg, Kr) <= 1e-12, rel_err(Kg, Kr)
    assert np.abs(Kg - Kr).max() <= 1e-12 * np.abs(Kr).max()


def _evaluate(mesh, kinem, path, u):
    dev = _dev()
    ev = fcg.Evaluator(mesh, kinematics=kinem, youngs=E, poisson=NU, path=path)
    f = _nan(mesh.n_rows)
    K = _nan(mesh.nnz)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, torch.from_numpy(u).to(dev), f, K)
    torch.cuda.synchronize()
    return ev, _h(K), _h(f)


@gpu
@pytest.mark.parametrize("kinem", [fcg.LINEAR, fcg.TOTLAG])
def test_fan_matches_oracle(kinem):
    f = sr.fan()
    u = (1e-3 if kinem == fcg.LINEAR else 5e-2) * np.random.default_rng(1).standard_normal(f.n_cols)
    err, _, Kr, fr = oracle_evaluate_single(f, kinem, E, NU, u)
    assert err == 0
    for path, lands in ((fcg.PATH_AUTO, fcg.PATH_GATHER), (fcg.PATH_GENERAL, fcg.PATH_GENERAL)):
        ev, Kg, fg = _evaluate(f, kinem, path, u)
        assert ev.info.path == lands
        _check_oracle(Kg, fg, Kr, fr)


@gpu
def test_two_layer_fan_is_refused_cleanly():
    _dev()
    with pytest.raises(fcg.FcgError, match="equal-length rows of <= 3\\*neighbours") as ei:
        fcg.Evaluator(sr.fan(2), kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    assert ei.value.code == fcg.FCG_ERR_ARG


# ------------------------------------------------ rows that are not made of DOF triples only
@gpu
def test_extra_columns_assemble_and_operate():
    """A graph with foreign columns (solver_ref.extra): the general path assembles it, the operator
    takes the row-by-row kernel, the PCG solves on it, the AMG refuses it."""
    amg = importlib.import_module("4c_amd.amg")
    mesh, ev, _ = _ctx("extra")
    u = 1e-3 * np.random.default_rng(1).standard_normal(mesh.n_cols)
    err, _, Kr, fr = oracle_evaluate_single(mesh, fcg.LINEAR, E, NU, u)
    assert err == 0
    f, K = _nan(mesh.n_rows), _nan(mesh.nnz)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(u), f, K)
    _check_oracle(_h(K), _h(f), Kr, fr)
    for a, b in mesh.added:
        for d in range(3):
            assert _h(K)[sr.entry_pos(mesh, 3 * a + d, 3 * b + 1)] == 0.0
    _check_spmv("extra", False, twice=True)
    _check_spmv("extra", True)
    _check_pcg_rtol("extra")
    with pytest.raises(fcg.FcgError, match="not node DOF triples") as ei:
        amg.NativeAMG(mesh, ev, sr.dirichlet_rows(mesh))
    assert ei.value.code == fcg.FCG_ERR_ARG
