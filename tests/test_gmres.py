"""GPU tests of fcg_gmres_solve (4c_amd/csrc/fcg_krylov.hip): restarted flexible GMRES on the
context's CSR graph, held against dense solves, the extended-precision CSR product of
tests/solver_ref.py and the numpy replay of tests/krylov_ref.py.

Bounds.  residual: |b - A x| <= rtol |b| + sigma, sigma = |(row length) 2^-53 |A||x||_2, the
rounding term of an FP64 product of that row length (test_spmv_componentwise's bound).  error: |x - x*| <=
cond_2(A) rtol |x*| (|x - x*| <= |A^-1| |r|, |b| <= |A| |x*|), cond computed here.  iteration
counts: at most 1.5 x the replay's (the margin of the project's AMG iteration comparisons) plus
one burst of 8, the granularity at which the host looks at the device's scalars."""

import importlib

import numpy as np
import pytest

import krylov_ref as kr
import solver_ref as sr
from solver_ref import LD, U

torch = pytest.importorskip("torch")
fcg = importlib.import_module("4c_amd").fcg
amg_mod = importlib.import_module("4c_amd.amg")
krylov = importlib.import_module("4c_amd.krylov")
gpu = pytest.mark.gpu
E, NU = 210.0, 0.3
BURST = 8
FCG_ERR_SINGULAR, FCG_ERR_ARG = 2, 3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t if dtype is None else t.to(dtype)


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


def _box(celltype, iv, jitter, renumber=False):
    box = fcg.BoxMesh(celltype, iv, jitter=jitter, seed=7)
    face = kr.x0_face(celltype, iv)
    if not renumber:
        return box, face
    dis = fcg.Discretization.renumbered(box, seed=3)
    return dis, np.sort(dis.node_perm[face])


MESHES = {
    "h8_322": lambda: _box(fcg.HEX8, (3, 2, 2), 0.1),
    "h27_221": lambda: _box(fcg.HEX27, (2, 2, 1), 0.0),
    "h8_332_renumbered": lambda: _box(fcg.HEX8, (3, 3, 2), 0.0, renumber=True),
    "h8_444": lambda: _box(fcg.HEX8, (4, 4, 4), 0.1),
    "h8_888": lambda: _box(fcg.HEX8, (8, 8, 8), 0.0),
}
_cache = {}


def _case(name):
    """(mesh, evaluator, Dirichlet rows, K with unit Dirichlet rows on the host), clamped at x = 0."""
    _dev()
    if name not in _cache:
        mesh, face = MESHES[name]()
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
        rows = np.sort((np.asarray(mesh.node_dof_row)[face][:, None] + np.arange(3)).ravel()).astype(np.int32)
        K = torch.zeros(mesh.nnz, dtype=torch.float64, device=_dev())
        f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=_dev())
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(np.zeros(mesh.n_cols)), f, K)
        ev.dirichlet_apply(_t(rows), K)
        torch.cuda.synchronize()
        _cache[name] = (mesh, ev, rows, K.cpu().numpy())
    return _cache[name]


def _rhs(mesh, rows, seed):
    b = np.random.default_rng(seed).standard_normal(mesh.n_rows)
    b[rows] = 0.0
    return b


def _residual(mesh, vals, b, x):
    """(|b - A x|, sigma) with the product in extended precision."""
    y, absy = sr.csr_matvec_ld(mesh.rowptr, mesh.col_lid, vals, x)
    r = np.asarray(b).astype(LD) - y
    sigma = np.diff(mesh.rowptr) * LD(U) * absy
    return float(np.sqrt((r * r).sum())), float(np.sqrt((sigma * sigma).sum()))


def _solve(ev, vals, b, **kw):
    x = _nan(len(b))
    it, rel = ev.gmres_solve(_t(vals), _t(b), x, **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), it, rel


# --------------------------------------------------------------------- 1. non-symmetric values
@gpu
@pytest.mark.parametrize("name", ["h8_322", "h27_221", "h8_332_renumbered"])
def test_nonsymmetric_values_against_dense(name):
    """Every entry of the free rows scaled by 1 + 0.3 U(-1, 1): nothing symmetric is left.
    restart 128 is full GMRES on the hex8 meshes (81 and 108 free unknowns); the hex27 box has
    180 and restarts once."""
    mesh, ev, rows, K = _case(name)
    rng = np.random.default_rng(11)
    free_entry = ~np.isin(np.repeat(np.arange(mesh.n_rows), np.diff(mesh.rowptr)), rows)
    vals = np.where(free_entry, K * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, mesh.nnz)), K)
    b = _rhs(mesh, rows, 12)
    rtol = 1e-10
    x, it, rel = _solve(ev, vals, b, rtol=rtol, max_iter=2000, restart=128)
    assert np.all(np.isfinite(x)) and np.all(x[rows] == 0.0)
    nb = np.linalg.norm(b)
    res, sigma = _residual(mesh, vals, b, x)
    A = kr.csr_to_dense(mesh.rowptr, mesh.col_lid, vals)
    assert not np.allclose(A, A.T)
    xd = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    err = np.linalg.norm(x - xd)
    print(f"gmres {name}: {it} steps, rel {rel:.3e}, independent {res / nb:.3e}, sigma/|b| "
          f"{sigma / nb:.1e}, err/|x| {err / np.linalg.norm(xd):.2e}, cond {cond:.2e}")
    assert res <= rtol * nb + sigma, (res / nb, sigma / nb)
    assert err <= cond * rtol * np.linalg.norm(xd), (err, cond)
    assert abs(rel / (res / nb) - 1.0) <= 1e-6, (rel, res / nb)


# ------------------------------------------------------------------------------ 2. SPD tangent
@gpu
@pytest.mark.parametrize("name", ["h8_322", "h27_221", "h8_332_renumbered"])
def test_spd_tangent_agrees_with_pcg(name):
    mesh, ev, rows, K = _case(name)
    b = _rhs(mesh, rows, 13)
    rg, rp = 1e-10, 1e-12
    xg, it, rel = _solve(ev, K, b, rtol=rg, max_iter=2000, restart=128)
    xp = _nan(mesh.n_rows)
    ev.pcg_solve(_t(K), _t(b), xp, rtol=rp, max_iter=5000)
    xp = xp.cpu().numpy()
    cond = np.linalg.cond(kr.csr_to_dense(mesh.rowptr, mesh.col_lid, K))
    assert rel <= rg
    assert np.linalg.norm(xg - xp) <= cond * (rg + rp) * np.linalg.norm(xp)


# ----------------------------------------------------------------------------- 3. restart path
@gpu
def test_restart_path_follows_the_replay():
    mesh, ev, rows, K = _case("h8_444")
    b = _rhs(mesh, rows, 14)
    A = kr.csr_to_dense(mesh.rowptr, mesh.col_lid, K)
    _, ref_it, ref_rel, _ = kr.fgmres(A, b, 5, 1e-8, 5000, kr.block_jacobi(A))
    assert ref_it < 5000 and ref_rel <= 1e-8
    x, it, rel = _solve(ev, K, b, rtol=1e-8, max_iter=5000, restart=5)
    print(f"restart 5: {it} steps, replay {ref_it}")
    assert rel <= 1e-8 and it > 5
    assert it <= 1.5 * ref_it + BURST
    res, sigma = _residual(mesh, K, b, x)
    assert res <= 1e-8 * np.linalg.norm(b) + sigma


# -------------------------------------------------------------------------- 4. exact breakdown
@gpu
def test_breakdown_when_the_preconditioner_is_the_inverse():
    """K zeroed outside the nodal diagonal blocks: P A = I, w = v_0 and h_10 is rounding or 0."""
    mesh, ev, rows, K = _case("h8_322")
    pos = sr.diag_block_positions(mesh)
    vals = np.zeros_like(K)
    vals[pos.ravel()] = K[pos.ravel()]
    b = _rhs(mesh, rows, 15)
    x, it, rel = _solve(ev, vals, b, rtol=1e-10, max_iter=100, restart=20)
    assert it <= BURST and np.all(np.isfinite(x)) and rel <= 1e-10
    row0, _ = sr.row_nodes(mesh)
    ref = np.zeros(mesh.n_rows)
    for k, r0 in enumerate(row0):
        ref[r0:r0 + 3] = np.linalg.solve(vals[pos[k]], b[r0:r0 + 3])
    assert np.linalg.norm(x - ref) <= 1e-14 * np.linalg.norm(ref)


# ------------------------------------------------------------------------------------ 5. edges
@gpu
def test_edges():
    mesh, ev, rows, K = _case("h8_322")
    b = _rhs(mesh, rows, 16)
    x, it, rel = _solve(ev, K, np.zeros(mesh.n_rows), rtol=1e-10)
    assert it == 0 and rel == 0.0 and np.all(x == 0.0)
    x, it, rel = _solve(ev, K, b, rtol=1e-10, max_iter=0)
    assert it == 0 and rel == 1.0 and np.all(x == 0.0)
    x1, it1, rel1 = _solve(ev, K, b, rtol=1e-10, restart=10)
    x2, it2, rel2 = _solve(ev, K, b, rtol=1e-10, restart=10)
    assert np.array_equal(x1, x2) and (it1, rel1) == (it2, rel2) and rel1 <= 1e-10
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    Kt, bt, xs = _t(K), _t(b), _nan(mesh.n_rows)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        it3, rel3 = ev.gmres_solve(Kt, bt, xs, rtol=1e-10, restart=10, stream=s)
    s.synchronize()
    assert np.array_equal(xs.cpu().numpy(), x1) and (it3, rel3) == (it1, rel1)
    # the linear-solver protocol of amg.NativeAMG
    g = krylov.Gmres(ev, restart=10)
    xg = _nan(mesh.n_rows)
    assert g.solve(Kt, bt, xg, 1e-10, 1000) == (it1, rel1) and np.array_equal(xg.cpu().numpy(), x1)


# -------------------------------------------------------------------------------- 6. refusals
@gpu
def test_refusals():
    mesh, ev, rows, K = _case("h8_322")
    b = _rhs(mesh, rows, 17)
    for restart in (0, 129):
        with pytest.raises(fcg.FcgError) as e:
            _solve(ev, K, b, restart=restart)
        assert e.value.code == FCG_ERR_ARG
    rank = fcg.BoxMesh(fcg.HEX8, (4, 2, 2), rank=0, nranks=2)
    rev = fcg.Evaluator(rank, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    with pytest.raises(fcg.FcgError) as e:
        rev.gmres_solve(_t(np.ones(rank.nnz)), _t(np.ones(rank.n_rows)), _nan(rank.n_rows))
    assert e.value.code == FCG_ERR_ARG
    pos = sr.diag_block_positions(mesh)
    free_node = int(np.nonzero(~np.isin(sr.row_nodes(mesh)[0], rows))[0][0])
    sing = K.copy()
    sing[pos[free_node].ravel()] = 0.0
    with pytest.raises(fcg.FcgError) as e:
        _solve(ev, sing, b)
    assert e.value.code == FCG_ERR_SINGULAR
    # one NaN off the diagonal blocks: the block Jacobi is fine, the first product is not
    off = np.setdiff1d(np.arange(mesh.rowptr[3 * free_node], mesh.rowptr[3 * free_node + 1]),
                       pos[free_node].ravel())
    bad = K.copy()
    bad[off[0]] = np.nan
    with pytest.raises(fcg.FcgError) as e:
        _solve(ev, bad, b, max_iter=50)
    assert e.value.code == FCG_ERR_SINGULAR
    a = amg_mod.NativeAMG(mesh, ev, rows)
    with pytest.raises(fcg.FcgError):
        ev.gmres_solve(_t(K), _t(b), _nan(mesh.n_rows), amg=a)


# ---------------------------------------------------------------------- 7. AMG preconditioner
@gpu
def test_amg_preconditioner():
    mesh, ev, rows, K = _case("h8_888")
    b = _rhs(mesh, rows, 18)
    a = amg_mod.NativeAMG(mesh, ev, rows, coarse_max=300)
    Kt = _t(K)
    a.setup(Kt)
    assert len(a.describe()) >= 2, a.describe()
    x = _nan(mesh.n_rows)
    it, rel = ev.gmres_solve(Kt, _t(b), x, rtol=1e-8, max_iter=500, restart=30, amg=a)
    _, it_bj, rel_bj = _solve(ev, K, b, rtol=1e-8, max_iter=5000, restart=30)
    print(f"hex8 8^3 rtol 1e-8 restart 30: AMG {it} steps, block Jacobi {it_bj} steps")
    x = x.cpu().numpy()
    res, sigma = _residual(mesh, K, b, x)
    assert 0 < it <= 500 and 0 < it_bj <= 5000
    assert rel <= 1e-8 and rel_bj <= 1e-8 and np.all(x[rows] == 0.0)
    assert res <= 1e-8 * np.linalg.norm(b) + sigma


# ------------------------------------------------------------------ 8. more than one grid pass
@gpu
def test_more_than_one_grid_pass():
    """47^3 elements, 48^3 nodes, 331,776 unknowns: more than the 262,144 doubles one pass of the
    Krylov kernels' capped grid covers (512 workgroups x 256 lanes x 16 bytes), so every
    streaming kernel strides.  The check's own FP64 product adds its rounding, sigma, to the bound;
    the solver's residual is compensated."""
    dev = _dev()
    iv = (47, 47, 47)
    mesh = fcg.BoxMesh(fcg.HEX8, iv)
    assert mesh.n_rows == 331776 > 512 * 256 * 2
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    face = kr.x0_face(fcg.HEX8, iv)
    rows = np.sort((np.asarray(mesh.node_dof_row)[face][:, None] + np.arange(3)).ravel()).astype(np.int32)
    K = torch.zeros(mesh.nnz, dtype=torch.float64, device=dev)
    f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=dev)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, torch.zeros(mesh.n_cols, dtype=torch.float64, device=dev), f, K)
    ev.dirichlet_apply(_t(rows), K)
    b = _t(_rhs(mesh, rows, 19))
    rtol = 1e-6
    x1, x2 = _nan(mesh.n_rows), _nan(mesh.n_rows)
    it, rel = ev.gmres_solve(K, b, x1, rtol=rtol, max_iter=20000, restart=30)
    it2, rel2 = ev.gmres_solve(K, b, x2, rtol=rtol, max_iter=20000, restart=30)
    print(f"47^3 block Jacobi restart 30 rtol 1e-6: {it} steps, rel {rel:.3e}")
    assert torch.equal(x1, x2) and (it, rel) == (it2, rel2)
    y, ay = torch.empty_like(b), torch.empty_like(b)
    ev.spmv(K, x1, y)
    ev.spmv(K.abs(), x1.abs(), ay)
    sigma = 81 * U * torch.linalg.norm(ay).item()
    res = torch.linalg.norm(b - y).item()
    nb = torch.linalg.norm(b).item()
    assert rel <= rtol and res <= rtol * nb + sigma, (rel, res / nb)
    assert abs(rel - res / nb) <= sigma / nb
    assert torch.all(x1[_t(rows).long()] == 0.0)


# ------------------------------------------------------------ 9. the orthogonalisation kernels
@gpu
@pytest.mark.parametrize("n,nv", [(1001, 11), (4096, 8), (300001, 17)])
def test_orthogonalisation_kernels(n, nv):
    """multi_dot / multi_axpy_norm on their own (fcg_gmres_orthogonalize) against the same two
    passes in extended precision: odd n (the 8-byte tail), nv below, at and above the tile of 8,
    and n beyond one pass of the capped grid.  V is orthonormal, so every coefficient and every
    intermediate w is bounded by |w|; with dots of n terms (error n u |w| each, u = 2^-53), an
    update of nv + 2 operations per entry on data of size (1 + sqrt(nv)) |w|, and the first pass'
    coefficient errors carried through the second:
      |h - h_ref| <= u |w| ((2 + sqrt(nv)) n + (nv + 2) (1 + sqrt(nv))),
    and the same bound holds for the norm of the error of the new w."""
    dev = _dev()
    rng = np.random.default_rng(n + nv)
    Q, _ = np.linalg.qr(rng.standard_normal((n, nv)))
    ld = (n + 1) & ~1
    V = np.zeros((nv, ld))
    V[:, :n] = Q.T
    w0 = rng.standard_normal(n)
    Vt = _t(V)
    outs = []
    for _ in range(2):
        w, h = _t(w0), _nan(nv + 1)
        fcg.gmres_orthogonalize(Vt, w, h)
        torch.cuda.synchronize()
        outs.append((w.cpu().numpy(), h.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    w, h = outs[0]
    VL, wl = V[:, :n].astype(LD), w0.astype(LD)
    h1 = VL @ wl
    w1 = wl - h1 @ VL
    h2 = VL @ w1
    w2 = w1 - h2 @ VL
    nw = float(np.sqrt((wl * wl).sum()))
    bound = U * nw * ((2 + np.sqrt(nv)) * n + (nv + 2) * (1 + np.sqrt(nv)))
    eh = float(np.abs(h[:nv].astype(LD) - (h1 + h2)).max())
    ew = float(np.sqrt(((w.astype(LD) - w2) ** 2).sum()))
    en = abs(float(h[nv]) - float(np.sqrt((w2 * w2).sum())))
    print(f"orth n={n} nv={nv}: |dh| {eh:.2e}, |dw| {ew:.2e}, d|w| {en:.2e}, bound {bound:.2e}")
    assert np.all(np.isfinite(h)) and eh <= bound and ew <= bound and en <= bound
    assert float(np.abs(VL @ w.astype(LD)).max()) <= bound  # orthogonal to the basis afterwards
    with pytest.raises(fcg.FcgError):
        fcg.gmres_orthogonalize(_t(np.zeros((129, 8))), _t(np.zeros(8)), _nan(130),
                                work=_nan(4096))


# ------------------------------------------------------- 10. as the Newton loop's linear solver
@gpu
def test_static_newton_accepts_gmres():
    """krylov.Gmres behind newton.StaticNewton(linear_solver=...) on a total-Lagrangian box: the
    same Newton history as with the library's PCG.  Both runs stop with an increment below
    tol_inc = 1e-10 of a quadratically converging iteration, so each is within tol_inc of the
    solution and they are within 2 tol_inc of each other."""
    _dev()
    newton = importlib.import_module("4c_amd.newton")
    mesh, face = _box(fcg.HEX8, (3, 2, 2), 0.1)
    rows = np.sort((np.asarray(mesh.node_dof_row)[face][:, None] + np.arange(3)).ravel()).astype(np.int32)
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU)
    fext = 0.5 * np.random.default_rng(20).standard_normal(mesh.n_rows)
    fext[rows] = 0.0
    runs = []
    for solver in (None, krylov.Gmres(ev, restart=128)):
        nw = newton.StaticNewton(ev, fext, rows, lin_rtol=1e-10, linear_solver=solver)
        u = nw.solve().cpu().numpy()
        runs.append((u, len(nw.history), [h.get("lin_iter", 0) for h in nw.history]))
    (up, np_, _), (ug, ng, lin) = runs
    print(f"StaticNewton: {ng} Newton iterations, GMRES steps {lin}, |u| {np.linalg.norm(up):.3e}")
    assert ng == np_ and max(lin) > 0 and np.linalg.norm(up) > 1e-3
    assert np.linalg.norm(ug - up) <= 2e-10
