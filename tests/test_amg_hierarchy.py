"""The native vector AMG (fcg_amg_create / _setup / _apply, 4c_amd/csrc/fcg_amg_solver.hip) pinned
to an extended-precision rebuild: every matrix of the hierarchy, fetched with fcg_amg_level_matrix /
fcg_amg_level_order, against its definition, and the V-cycle of fcg_amg_apply as a matrix against
tests/amg_ref.py's cycle rebuilt from those matrices in float64 and in longdouble.

Bounds (u = 2^-53), as in tests/test_samg.py and tests/test_solver_primitives.py:
  block inverses     e = max|dinv - ref| / (kappa_inf u max|ref|) per block, ref the longdouble
                     inverse; the kernel's largest e at most 4 x the largest e of the float64 replay
                     of its own Gauss-Jordan (every kappa_inf below 1e6)
  prolongator        |P - (T - w Dinv A T)| <= (terms + b + 3) u (|T| + w |Dinv| |A| |T|), w = omega / lmax:
                     one rounded SpGEMM, one b-term block product, the subtraction
  Galerkin           |A_c - P^T A P| <= (terms + 2) u |P|^T |A| |P|; asymmetry within twice that plus
                     |P|^T |A - A^T| |P|, what the asymmetry of the fetched A_l itself hands down
                     (A_l is symmetric only to the rounding of the product that formed it; without
                     the term the third level of h27_322 and of local missed twice the bound)
  lambda_max         a Ritz value: lmax <= lambda_max(D^-1/2 A_ff D^-1/2) (1 + 1e-10)
  coarsest inverse   |cinv - inv_ld|_F <= CINV_MARGIN |numpy inv - inv_ld|_F (the margin measured,
                     see below), asymmetry within 2 d_gpu + 2 d_64 + |inv_ld - inv_ld^T|_F: the
                     exact inverse of that A is itself unsymmetric by |A^-1|^2 |A - A^T| (2e-15 at
                     n = 6, ten times d_gpu, and matched by the kernel's inverse to 2e-17)
  V-cycle            |M - M_ld|_F <= 8 own and |M_ff - M_ff^T|_F <= 8 own, own = |M_f64 - M_ld|_F;
                     eig(M A_ff) in (0, 1 + 8 own |A_ff|_2]: the error propagator is
                     (I - S A)(I - P M_c P^T A)(I - S A) with the same symmetric S before and after
                     the coarse correction, so it is A-positive-semidefinite whenever
                     eig(M_c A_c) is in (0, 1] -- exactly so for the dense coarsest inverse, by
                     induction above -- however good the smoother is; eig > 0 needs the smoother
                     to contract, where a too-small lambda_max shows.

Measured on one MI355X (printed again under -s):
  case           DOFs per level    block inverses, largest e per level   lmax / lambda_max   d_gpu / d_64
                                   kernel | float64 replay               per level           (coarsest n)
  h8_633         336, 48, 6        0.959 0.426 0.300 | 0.959 0.426 0.300  1.0000 0.9825      0.703 (6)
  h8_633_totlag  336, 48, 6        0.998 0.386 0.420 | 0.998 0.386 0.420  1.0000 0.9832      1.473 (6)
  h27_322        525, 12, 6        1.370 0.706 0.351 | 1.370 0.706 0.351  0.9905 1.0000      0.697 (6)
  roller         336, 48, 6        0.394 0.353 0.129 | 0.394 0.353 0.129  1.0000 0.9992      0.787 (6)
  line_12        351, 30           0.287 0.002       | 0.287 0.002        0.9992             0.999 (30)
  line_30        837, 66           0.154 0.000       | 0.154 0.000        0.9865             0.937 (66)
  h8_1244        975, 96           0.434 0.458       | 0.434 0.448        0.9969             2.606 (96)
  h8_1666        2499, 324         0.476 0.599       | 0.476 0.599        0.9709             1.455 (324)
  h8_2066        3087, 378         0.508 0.493       | 0.508 0.493        0.9634             0.456 (378)
  local          144, 24, 6        1.293 0.445 0.013 | 1.401 0.445 0.013  0.9999 1.0000      1.000 (6)
  (every kappa_inf of a block below 2.2e2.)  The largest d_gpu / d_64 is 2.606: CINV_MARGIN = 8.
  Worst prolongator error / bound 0.463, Galerkin error / bound 0.017, asymmetry / its bound 0.799.

  V-cycle as a matrix   |M - M_ld|_F   own        |M_ff - M_ff^T|_F   [min, max] eig(M A_ff)
  h8_633 nu 2           3.495e-15      5.586e-15  2.108e-15           [0.46735, 1.000000000000]
  h8_633 nu 1           1.291e-15      2.040e-15  2.019e-15           [0.16063, 1.000000000000]
  h8_633 nu 3           5.863e-15      6.390e-15  1.911e-15           [0.70425, 1.000000000000]
  h8_633 no reordering  4.597e-15      6.396e-15  1.229e-15           [0.27414, 1.000000000000]
  h8_633_totlag         4.356e-15      5.674e-15  2.323e-15           [0.46713, 1.000000000000]
  h27_322               6.688e-15      1.310e-14  3.946e-15           [0.21482, 1.000000000000]
  roller                3.645e-15      4.743e-15  9.980e-16           [0.46899, 1.000000000000]
  line_12               8.809e-15      9.005e-15  1.741e-17           [0.53864, 1.000000000000]
  local                 1.460e-15      1.522e-15  3.324e-17           [0.52147, 1.000000000000]
  (the upper end allowed is 1 + 4e-12 .. 1 + 1e-10; without reordering the levels are 336, 18, 6.)
  Large cases, four right-hand sides: |z - z_ld|_2 / |z_f64 - z_ld|_2 at most 3.37 (h8_1244),
  1.71 (h8_1666), 0.60 (h8_2066), 1.29 (line_30).
"""

import contextlib
import ctypes
import importlib
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import amg_ref
import samg_ref
import solver_ref as sr
from amg_ref import U
from parity_util import oracle_evaluate
from samg_ref import LD

torch = pytest.importorskip("torch")
fcg = importlib.import_module("4c_amd").fcg
amg = importlib.import_module("4c_amd.amg")
gpu = pytest.mark.gpu
E, NU = 210.0, 0.3
CINV_MARGIN = 8.0  # twice the largest measured d_gpu / d_64 (2.606), rounded up to a power of two

# bc: "xmin" clamps the x-min face; "roller" also fixes z on the z-min face; "lateral" clamps the
# four lateral faces (every free node on the line y = z = 1/2).  seed: of the renumbering.
CASES = {
    "h8_633": dict(ct="HEX8", iv=(6, 3, 3), jitter=0.1, seed=1, bc="xmin", opts={"coarse_max": 12}),
    "h8_633_totlag": dict(ct="HEX8", iv=(6, 3, 3), jitter=0.1, seed=1, bc="xmin", opts={"coarse_max": 12},
                          totlag=True),
    # (two 125-neighbour aggregates already leave 12 DOFs: coarse_max 6 for the third level)
    "h27_322": dict(ct="HEX27", iv=(3, 2, 2), jitter=0.02, seed=2, bc="xmin", opts={"coarse_max": 6}),
    "roller": dict(ct="HEX8", iv=(6, 3, 3), jitter=0.0, seed=3, bc="roller", opts={"coarse_max": 12}),
    "line_12": dict(ct="HEX8", iv=(12, 2, 2), jitter=0.0, seed=4, bc="lateral", opts={}),
    "line_30": dict(ct="HEX8", iv=(30, 2, 2), jitter=0.0, seed=5, bc="lateral", opts={}),
    "h8_1244": dict(ct="HEX8", iv=(12, 4, 4), jitter=0.0, seed=6, bc="xmin", opts={}),
    "h8_1666": dict(ct="HEX8", iv=(16, 6, 6), jitter=0.0, seed=7, bc="xmin", opts={}),
    "h8_2066": dict(ct="HEX8", iv=(20, 6, 6), jitter=0.0, seed=8, bc="xmin", opts={}),
    "local": dict(ct="HEX8", iv=(4, 3, 3), jitter=0.0, seed=None, bc="xmin", opts={"coarse_max": 12}),
}
ALL = list(CASES)
DEEP = ["h8_633", "h8_633_totlag", "h27_322", "roller"]   # at least 3 levels
LINES = ["line_12", "line_30"]
LARGE = ["h8_1244", "h8_1666", "h8_2066", "line_30"]


def _same(a, b):
    """Bitwise equality of two arrays (float64 compared as bit patterns)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return bool(np.array_equal(a, b))


def _fixed(spec, X):
    """[n_node][3] Dirichlet marks from the coordinates X of the box without jitter."""
    lo = lambda d: np.isclose(X[:, d], 0.0)
    hi = lambda d: np.isclose(X[:, d], 1.0)
    fix = np.zeros((len(X), 3), dtype=bool)
    if spec["bc"] in ("xmin", "roller"):
        fix[lo(0)] = True
    if spec["bc"] == "roller":
        fix[lo(2), 2] = True
    if spec["bc"] == "lateral":
        fix[lo(1) | hi(1) | lo(2) | hi(2)] = True
    return fix


def _mesh(name):
    """(mesh, Dirichlet rows int32 ascending) of a case."""
    spec = CASES[name]
    ct = getattr(fcg, spec["ct"])
    if name == "local":
        mesh = fcg.BoxMesh(ct, spec["iv"], rank=0, nranks=2)
        fix = _fixed(spec, mesh.node_x)
    else:
        flat = fcg.BoxMesh(ct, spec["iv"])
        mesh = fcg.Discretization.renumbered(fcg.BoxMesh(ct, spec["iv"], jitter=spec["jitter"]), seed=spec["seed"])
        fix = np.zeros((flat.n_node, 3), dtype=bool)
        fix[mesh.node_perm] = _fixed(spec, flat.node_x)
    ndr = np.asarray(mesh.node_dof_row, dtype=np.int64)
    node, d = np.nonzero(fix & (ndr >= 0)[:, None])
    return mesh, np.sort(ndr[node] + d).astype(np.int32)


# ------------------------------------------------------------------------------------ CPU part
_host = {}


def _host_hierarchy():
    """A hierarchy built on the host alone: the oracle's K of a jittered hex8 box with the x-min
    face clamped, amg.aggregate / amg.tentative through amg_ref.coarsen_step, scipy products in
    float64, lambda_max from a dense eigen-solve, the replayed Gauss-Jordan as block inverses."""
    if _host:
        return _host
    mesh = fcg.BoxMesh(fcg.HEX8, (6, 3, 3), jitter=0.1)
    flat = fcg.BoxMesh(fcg.HEX8, (6, 3, 3))
    err, _, Kv, _ = oracle_evaluate(mesh, fcg.LINEAR, E, NU, np.zeros(mesh.n_cols))
    assert err == 0
    assert np.array_equal(mesh.node_dof_row, 3 * np.arange(mesh.n_node))
    fix = _fixed({"bc": "xmin"}, flat.node_x)
    rows = np.nonzero(fix.ravel())[0].astype(np.int32)
    Kv = sr.apply_dirichlet_host(mesh, Kv, rows)
    ptr, col, vals = amg_ref.node_blocks(mesh.rowptr, mesh.col_lid, Kv, mesh.n_rows)
    ns, skip = amg_ref.near_null_space(mesh.node_x, fix)
    omega, coarse_max = 4.0 / 3.0, 12
    A, P, dinv, lmax = [amg_ref.bsr_sparse(ptr, col, vals, len(ptr) - 1)], [], [], []
    bs = 3
    while A[-1].shape[0] > coarse_max:
        Ab = A[-1].tobsr(blocksize=(bs, bs))
        Ab.sort_indices()
        D = amg_ref.diag_blocks(Ab.indptr, Ab.indices, Ab.data)
        st = amg_ref.coarsen_step(Ab.indptr.astype(np.int64), Ab.indices.astype(np.int32), ns,
                                  skip.astype(np.uint8) if bs == 3 else None)
        Di = amg_ref.gauss_jordan_f64(D)
        Dinv = amg_ref.block_diag_sparse(Di)
        lm = float(np.linalg.eigvals((Dinv @ A[-1]).toarray()).real.max())
        T = amg_ref.bsr_sparse(*st["T"], st["n_agg"])
        Pl = (T - (omega / lm) * (Dinv @ (A[-1] @ T))).tocsr()
        Ac = (Pl.T @ A[-1] @ Pl).tolil()
        for e in np.nonzero(np.asarray(abs(Pl).sum(axis=0)).ravel() == 0)[0]:
            Ac[e, e] = 1.0  # the unit diagonal of a vanished column
        P.append(Pl)
        dinv.append(Di)
        lmax.append(lm)
        A.append(Ac.tocsr())
        ns, bs = st["ns"], 6
    free = np.nonzero(~fix.ravel())[0]
    _host.update(A=A, P=P, dinv=dinv, lmax=lmax, free=free, nu=2, ratio=20.0, boost=1.1)
    return _host


def _cycles(A, P, dinv, lmax, nu, ratio, boost, cinv_ld=None):
    """(M_f64, M_ld): the float64 rebuild with the given block inverses, the longdouble one with the
    refined inverses of the diagonal blocks of the given A."""
    out = []
    for dt in (np.float64, LD):
        di = dinv
        if dt is LD:
            di = []
            for l in range(len(P)):
                b = dinv[l].shape[1]
                Ab = A[l].tobsr(blocksize=(b, b))
                Ab.sort_indices()
                di.append(amg_ref.block_inverse_ld(amg_ref.diag_blocks(Ab.indptr, Ab.indices, Ab.data))[0])
        out.append(amg_ref.Cycle(A, P, di, lmax, nu, ratio, boost, dt, cinv=cinv_ld if dt is LD else None))
    return out


def _spectrum(Mff, Aff):
    """eig(L^T sym(M_ff) L), A_ff = L L^T: the eigenvalues of M A on the free DOFs."""
    L = np.linalg.cholesky(0.5 * (Aff + Aff.T))
    return np.linalg.eigvalsh(L.T @ (0.5 * (Mff + Mff.T)) @ L)


def test_reference_cycle_float64_and_longdouble_agree():
    h = _host_hierarchy()
    assert len(h["A"]) >= 3
    c64, cld = _cycles(h["A"], h["P"], h["dinv"], h["lmax"], h["nu"], h["ratio"], h["boost"])
    M64, Mld = c64.matrix(), cld.matrix()
    own = float(np.linalg.norm((M64.astype(LD) - Mld).astype(np.float64)))
    n = M64.shape[0]
    # a vector through the cycle and column by column give the same operator
    b = np.random.default_rng(3).standard_normal(n)
    assert np.linalg.norm(c64.apply(b) - M64 @ b) <= 64 * n * U * np.linalg.norm(M64, 2) * np.linalg.norm(b)
    # rounding only: every product of the cycle loses n u at most, the coarsest solve cond(A_c) u
    cond = np.linalg.cond(h["A"][-1].toarray())
    print(f"host cycle: levels {[a.shape[0] for a in h['A']]}, |M_f64 - M_ld| {own:.3e}, |M| "
          f"{np.linalg.norm(M64):.3e}, cond(A_c) {cond:.2e}")
    assert 0 < own <= n * U * max(cond, n) * np.linalg.norm(M64)
    f = h["free"]
    Mff = Mld[np.ix_(f, f)].astype(np.float64)
    assert np.linalg.norm(Mff - Mff.T) <= 8 * own
    h["M64"], h["own"] = M64, own


def test_reference_cycle_spectrum_in_unit_interval():
    """eig(M_ff A_ff) in (0, 1] (module docstring) on the host-built hierarchy."""
    h = _host_hierarchy()
    if "M64" not in h:
        test_reference_cycle_float64_and_longdouble_agree()
    f = h["free"]
    Aff = h["A"][0].toarray()[np.ix_(f, f)]
    assert np.linalg.norm(Aff - Aff.T) <= 1e-13 * np.linalg.norm(Aff)
    ev = _spectrum(h["M64"][np.ix_(f, f)], Aff)
    print(f"host cycle: eig(M A_ff) in [{ev.min():.4f}, {ev.max():.6f}]")
    assert ev.min() > 0 and ev.max() <= 1 + 8 * h["own"] * np.linalg.norm(Aff, 2)


def test_reference_pieces():
    """The Gauss-Jordan replay inverts; the refined longdouble inverses are inverses to 2^-63;
    morton_order is a permutation that sorts a lattice along the Z curve; permute_bsr conjugates."""
    rng = np.random.default_rng(5)
    D = rng.standard_normal((7, 6, 6)) + 6 * np.eye(6)
    ref, kappa = amg_ref.block_inverse_ld(D)
    R = np.matmul(D.astype(LD), ref) - np.eye(6, dtype=LD)
    assert np.abs(R).max() <= 64 * float(np.finfo(LD).eps) * kappa.max()
    assert np.abs(amg_ref.gauss_jordan_f64(D) - ref).max() <= 64 * U * kappa.max() * np.abs(ref).max()
    g = np.stack(np.meshgrid(np.arange(2.0), np.arange(2.0), np.arange(2.0), indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(amg_ref.morton_order(g), np.arange(8))  # x is the most significant bit
    o = amg_ref.morton_order(rng.standard_normal((50, 3)))
    assert np.array_equal(np.sort(o), np.arange(50))
    A = sp.random(12, 12, density=0.3, random_state=1, format="csr") + sp.eye(12)
    Ab = A.tobsr(blocksize=(3, 3))
    Ab.sort_indices()
    n2o = rng.permutation(4).astype(np.int32)
    pp, pc, pv = amg_ref.permute_bsr(Ab.indptr, Ab.indices, Ab.data, n2o)
    dof = (3 * n2o[:, None] + np.arange(3)).ravel()
    assert np.array_equal(amg_ref.bsr_dense(pp, pc, pv, 4), A.toarray()[np.ix_(dof, dof)])


# ------------------------------------------------------------------------------------ GPU part
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_sys, _built = {}, {}


def _system(name):
    """(mesh, Evaluator, Dirichlet rows, K on the device, K on the host)."""
    if name not in _sys:
        dev = _dev()
        mesh, rows = _mesh(name)
        spec = CASES[name]
        totlag = spec.get("totlag", False)
        ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG if totlag else fcg.LINEAR, youngs=E, poisson=NU)
        u = 1e-3 * np.random.default_rng(17).standard_normal(mesh.n_cols) if totlag else np.zeros(mesh.n_cols)
        K = torch.zeros(int(ev.info.nnz), dtype=torch.float64, device=dev)
        f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=dev)
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(u), f, K)
        ev.dirichlet_apply(_t(rows), K)
        torch.cuda.synchronize()
        _sys[name] = (mesh, ev, rows, K, K.cpu().numpy())
    return _sys[name]


class _Fetched:
    pass


def _build(name, env=None, **over):
    """The case's NativeAMG set up for its K, with everything the library reports on the host."""
    env = env or {}
    key = (name, tuple(sorted(env.items())), tuple(sorted(over.items())))
    if key in _built:
        return _built[key]
    mesh, ev, rows, K, Kh = _system(name)
    with _env(env):
        a = amg.NativeAMG(mesh, ev, rows, **{**CASES[name]["opts"], **over})
        a.setup(K)
    f = _Fetched()
    f.a, f.info, f.stats = a, a.describe(), a.stats()
    nl = len(f.info)
    f.nl, f.order = nl, a.order()
    f.A = [a.level_matrix(l, 0) for l in range(nl)]
    f.P = [a.level_matrix(l, 1) for l in range(nl - 1)]
    f.T = [a.level_matrix(l, 2) for l in range(nl - 1)]
    f.dinv = [a.level_matrix(l, 3) for l in range(nl)]
    f.cinv = a.level_matrix(nl - 1, 4) if f.stats["coarse_dense"] else None
    f.nb = [len(A[0]) - 1 for A in f.A]
    f.lmax = [i["lmax"] for i in f.info]
    # Dirichlet marks [nodes][3] in level 0's order
    dbc = np.zeros(mesh.n_rows, dtype=bool)
    dbc[rows] = True
    f.dbc0 = dbc.reshape(-1, 3)[f.order]
    f.dof = (3 * f.order.astype(np.int64)[:, None] + np.arange(3)).ravel()  # caller's DOF of level 0's
    f.cache = {}
    _built[key] = f
    return f


def _sparse(f, which, l, dtype):
    key = (which, l, dtype)
    if key not in f.cache:
        if which == "A":
            f.cache[key] = amg_ref.bsr_sparse(*f.A[l], f.nb[l], dtype)
        elif which == "P":
            f.cache[key] = amg_ref.bsr_sparse(*f.P[l], f.nb[l + 1], dtype)
        else:
            f.cache[key] = amg_ref.bsr_sparse(*f.T[l], f.nb[l + 1], dtype)
    return f.cache[key]


def _empty_dofs(f, l):
    """Coarse DOFs of level l >= 1 whose column of P_{l-1} vanished (a rank-deficient aggregate)."""
    P = _sparse(f, "P", l - 1, np.float64)
    return np.nonzero(np.asarray(abs(P).sum(axis=0)).ravel() == 0)[0]


def _cinv_ld(f):
    if "cinv_ld" not in f.cache:
        f.cache["cinv_ld"] = samg_ref.inverse(_sparse(f, "A", f.nl - 1, np.float64).toarray(), LD)
    return f.cache["cinv_ld"]


@gpu
def test_cases_reach_what_they_are_listed_for():
    sizes = {}
    for name in ALL:
        f = _build(name)
        sizes[name] = [i["dofs"] for i in f.info]
        assert f.stats["coarse_dense"], name
    print("levels: " + ", ".join(f"{k} {v}" for k, v in sizes.items()))
    for name in DEEP:
        assert len(sizes[name]) >= 3, (name, sizes[name])
    for name in LINES:
        f = _build(name)
        assert len(_empty_dofs(f, 1)) >= f.nb[1], name  # an empty coarse row per aggregate
    last = [v[-1] for v in sizes.values()]
    assert any(n < 32 for n in last)
    assert any(n % 32 != 0 and -(-n // 32) % 2 == 1 for n in last)
    assert any(-(-n // 32) % 2 == 0 for n in last)
    assert any(n > 256 for n in last)
    assert not np.array_equal(_build("h8_633").order, np.arange(_build("h8_633").nb[0]))


# ------------------------------------------------------------------------ 1. order and level 0
def _check_level0(name, f):
    mesh, ev, rows, K, Kh = _system(name)
    ptr, col, vals = amg_ref.node_blocks(mesh.rowptr, mesh.col_lid, Kh, mesh.n_rows)
    ptr, col, vals = amg_ref.permute_bsr(ptr, col, vals, f.order)
    assert np.array_equal(f.A[0][0], ptr) and np.array_equal(f.A[0][1], col)
    assert _same(f.A[0][2], vals)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_order_and_level0(name):
    f = _build(name)
    n = f.nb[0]
    if name == "local":
        assert f.a.local and np.array_equal(f.order, np.arange(n))
        mesh = _system(name)[0]
        assert mesh.n_cols > mesh.n_rows and int(f.A[0][0][-1]) * 9 < len(_system(name)[4])  # ghosts dropped
    else:
        assert np.array_equal(f.order, amg_ref.morton_order(f.a._x))
    assert np.array_equal(np.sort(f.order), np.arange(n))
    _check_level0(name, f)


@gpu
def test_order_is_the_identity_without_reordering():
    f = _build("h8_633", env={"FCG_AMG_REORDER": "0"})
    assert np.array_equal(f.order, np.arange(f.nb[0]))
    _check_level0("h8_633", f)
    # level 0 then smooths with the context's own block inverses
    mesh, ev, rows, K, Kh = _system("h8_633")
    d = torch.full((9 * f.nb[0],), float("nan"), dtype=torch.float64, device=_dev())
    s = ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    assert fcg.lib().fcg_block_jacobi_setup(ev._h, ctypes.c_void_p(K.data_ptr()), ctypes.c_void_p(d.data_ptr()), s) == 0
    torch.cuda.synchronize()
    assert _same(f.dinv[0], d.cpu().numpy().reshape(-1, 3, 3))


# --------------------------------------------------------- 2. aggregates, T and the patterns
@gpu
@pytest.mark.parametrize("name", ALL)
def test_aggregates_tentative_and_patterns(name):
    f = _build(name)
    x = f.a._x[f.order]
    ns, skip = amg_ref.near_null_space(x, f.dbc0)
    for l in range(f.nl - 1):
        ptr, col, _ = f.A[l]
        st = amg_ref.coarsen_step(ptr, col, ns, skip.astype(np.uint8) if l == 0 else None)
        assert st["n_agg"] == f.nb[l + 1]
        tptr, tcol, tvals = st["T"]
        assert np.array_equal(f.T[l][0], tptr) and np.array_equal(f.T[l][1], tcol) and _same(f.T[l][2], tvals)
        assert np.array_equal(f.P[l][0], st["P"][0]) and np.array_equal(f.P[l][1], st["P"][1])
        assert np.array_equal(f.A[l + 1][0], st["Ac"][0]) and np.array_equal(f.A[l + 1][1], st["Ac"][1])
        if name in LINES:
            assert st["deficient"] >= st["n_agg"]
        ns = st["ns"]
    if name == "roller":  # nodes with one of three DOFs fixed are aggregated, their rows zeroed
        part = f.dbc0.any(axis=1) & ~f.dbc0.all(axis=1)
        assert part.any() and not skip[part].any()


# --------------------------------------------------------------------------- 3. block inverses
@gpu
@pytest.mark.parametrize("name", ALL)
def test_block_inverses(name):
    f = _build(name)
    out = []
    for l in range(f.nl):
        ptr, col, vals = f.A[l]
        D = amg_ref.diag_blocks(ptr, col, vals)
        ref, kappa = amg_ref.block_inverse_ld(D)
        print(f"block inverses {name} level {l}: {len(D)} blocks, kappa_inf max {kappa.max():.3e}")
        assert kappa.max() < 1e6
        if l == 0 and name == "local":  # the context's cofactor formula (no reordering)
            replay = sr.cofactor_inverse_f64(D).reshape(-1, 3, 3)
        else:
            replay = amg_ref.gauss_jordan_f64(D)
        scale = kappa * U * np.abs(ref).max(axis=(1, 2)).astype(np.float64)
        e_gpu = float((np.abs(f.dinv[l].astype(LD) - ref).max(axis=(1, 2)).astype(np.float64) / scale).max())
        e_f64 = float((np.abs(replay.astype(LD) - ref).max(axis=(1, 2)).astype(np.float64) / scale).max())
        out.append((e_gpu, e_f64))
        assert np.all(np.isfinite(f.dinv[l])) and e_gpu <= 4.0 * e_f64, (l, e_gpu, e_f64)
        if l >= 1:  # an empty scalar row: a unit diagonal, zeros elsewhere in its row and column
            A = _sparse(f, "A", l, np.float64)
            for e in _empty_dofs(f, l):
                unit = np.zeros(A.shape[0])
                unit[e] = 1.0
                assert np.array_equal(A[[e]].toarray().ravel(), unit), (l, e)
                assert np.array_equal(A[:, [e]].toarray().ravel(), unit), (l, e)
    print(f"block inverses {name}: e GPU / e float64 replay per level "
          + ", ".join(f"{g:.3f} / {r:.3f}" for g, r in out))


# ---------------------------------------------------------------------- 4. smoothed prolongator
@gpu
@pytest.mark.parametrize("name", ALL)
def test_smoothed_prolongator(name):
    f = _build(name)
    worst = []
    for l in range(f.nl - 1):
        A, T = _sparse(f, "A", l, LD), _sparse(f, "T", l, LD)
        b = f.A[l][2].shape[1]
        dinv = f.dinv[l]
        slack = 0.0
        if l == 0 and name == "local":
            # without reordering the smoother's inverses (which = 3) are the context's; P_0 is
            # smoothed with the Gauss-Jordan inverses of the BSR copy, which are not fetched: the
            # longdouble inverses stand in, and the bound grows by what test_block_inverses allows
            # those to be off, 4 e kappa u max|ref| per block with e the float64 replay's
            D = amg_ref.diag_blocks(*f.A[0])
            ref, kappa = amg_ref.block_inverse_ld(D)
            scale = kappa * U * np.abs(ref).max(axis=(1, 2)).astype(np.float64)
            e = (np.abs(amg_ref.gauss_jordan_f64(D).astype(LD) - ref).max(axis=(1, 2)).astype(np.float64) / scale).max()
            dinv = ref
            slack = amg_ref.block_diag_sparse(np.ones((len(D), b, b)) * (4 * e * scale)[:, None, None], LD)
        Dinv = amg_ref.block_diag_sparse(dinv, LD)
        w = LD(f.a.opt.omega) / LD(f.lmax[l])
        AT, absAT = A @ T, abs(A) @ abs(T)
        ref = (T - w * (Dinv @ AT)).toarray()
        absum = (abs(T) + w * (abs(Dinv) @ absAT)).toarray()
        terms = ((A != 0).astype(np.float64) @ (T != 0).astype(np.float64)).toarray()
        bound = (terms + b + 3) * LD(U) * absum
        if l == 0 and name == "local":
            bound = bound + w * (slack @ absAT).toarray()
        P = _sparse(f, "P", l, LD).toarray()
        on = np.kron(amg_ref.bsr_pattern(f.P[l][0], f.P[l][1], f.nb[l + 1]), np.ones((b, 6), dtype=bool))
        err = np.abs(P - ref)
        nz = bound > 0
        worst.append(float((err[nz] / bound[nz]).max()))
        assert np.all(ref[~on] == 0) and np.all(P[~on] == 0)
        assert np.all(np.isfinite(P.astype(np.float64))) and np.all(err <= bound), (l, worst[-1])
    print(f"prolongator {name}: worst error / bound per level " + ", ".join(f"{v:.3f}" for v in worst))


# ----------------------------------------------------------------------- 5. Galerkin operators
@gpu
@pytest.mark.parametrize("name", ALL)
def test_galerkin_operators(name):
    f = _build(name)
    worst = []
    for l in range(f.nl - 1):
        A, P = _sparse(f, "A", l, LD), _sparse(f, "P", l, LD)
        ref = (P.T @ (A @ P)).toarray()
        absum = (abs(P).T @ (abs(A) @ abs(P))).toarray()
        nzA, nzP = (A != 0).astype(np.float64), (P != 0).astype(np.float64)
        terms = (nzP.T @ (nzA @ nzP)).toarray()
        bound = (terms + 2) * LD(U) * absum
        Ac = _sparse(f, "A", l + 1, LD).toarray()
        e = _empty_dofs(f, l + 1)
        assert np.all(Ac[e, e] == 1.0)
        Ac[e, e] = 0.0  # the unit diagonals of empty rows: checked in test_block_inverses
        # A_c - A_c^T = (A_c - ref) - (A_c - ref)^T + P^T (A - A^T) P: twice the bound, and what A_l's
        # own asymmetry hands down -- the rounding of the assembly or of the product that formed it
        # (the columns K keeps on its Dirichlet rows meet zero rows of P)
        inherited = (abs(P).T @ (abs(A - A.T) @ abs(P))).toarray()
        err, asym = np.abs(Ac - ref), np.abs(Ac - Ac.T)
        sym_bound = 2 * bound + inherited
        nz, ns = bound > 0, sym_bound > 0
        worst.append((float((err[nz] / bound[nz]).max()), float((asym[ns] / sym_bound[ns]).max())))
        assert np.all(err <= bound), (l, worst[-1])
        assert np.all(asym <= sym_bound), (l, worst[-1])
    print(f"galerkin {name}: worst error / bound, asymmetry / its bound per level "
          + ", ".join(f"{a:.3f} {b:.3f}" for a, b in worst))


# ---------------------------------------------------------------------------- 6. setup switches
@gpu
@pytest.mark.parametrize("name", ["h8_633", "line_12", "h8_1244"])
@pytest.mark.parametrize("switch", ["FCG_AMG_PLAN", "FCG_AMG_PLAN_ORDER"])
def test_setup_switches_change_no_bit(name, switch):
    f, g = _build(name), _build(name, env={switch: "0"})
    assert g.nl == f.nl and g.lmax == f.lmax and np.array_equal(f.order, g.order)
    for l in range(f.nl):
        for F, G in ((f.A, g.A), (f.P, g.P), (f.T, g.T)):
            if l < len(F):
                assert np.array_equal(F[l][0], G[l][0]) and np.array_equal(F[l][1], G[l][1])
                assert _same(F[l][2], G[l][2]), (switch, l)
        assert _same(f.dinv[l], g.dinv[l])
    assert _same(f.cinv, g.cinv)


# -------------------------------------------------------------------------------- 7. lambda_max
@gpu
@pytest.mark.parametrize("name", ALL)
def test_lambda_max_is_a_ritz_value(name):
    f = _build(name)
    out = []
    for l in range(f.nl - 1):
        A = _sparse(f, "A", l, np.float64).tolil()
        b = f.A[l][2].shape[1]
        if l == 0:  # the free DOFs: unit rows and columns on the Dirichlet ones (eigenvalue 1 <= lambda_max)
            fixed = np.nonzero(f.dbc0.ravel())[0]
            A[fixed, :] = 0.0
            A[:, fixed] = 0.0
            A[fixed, fixed] = 1.0
        A = A.tocsr()
        Ab = A.tobsr(blocksize=(b, b))
        Ab.sort_indices()
        D = amg_ref.diag_blocks(Ab.indptr, Ab.indices, Ab.data)
        Li = np.linalg.inv(np.linalg.cholesky(0.5 * (D + D.transpose(0, 2, 1))))
        Linv = amg_ref.block_diag_sparse(Li)
        S = (Linv @ A @ Linv.T).toarray()
        n = S.shape[0]
        lam = float(scipy.linalg.eigh(0.5 * (S + S.T), eigvals_only=True, subset_by_index=[n - 1, n - 1])[0])
        out.append(f.lmax[l] / lam)
        assert 0 < f.lmax[l] <= lam * (1 + 1e-10), (l, f.lmax[l], lam)
    print(f"lambda_max {name}: lmax / lambda_max per level " + ", ".join(f"{v:.4f}" for v in out))


# -------------------------------------------------------------------- 8. dense coarsest inverse
@gpu
@pytest.mark.parametrize("name", ALL)
def test_dense_coarsest_inverse(name):
    f = _build(name)
    A = _sparse(f, "A", f.nl - 1, np.float64).toarray()
    n = A.shape[0]
    assert f.cinv is not None and f.cinv.shape == (n, n) and np.all(np.isfinite(f.cinv))
    ref = _cinv_ld(f)
    d_gpu = float(np.linalg.norm((f.cinv.astype(LD) - ref).astype(np.float64)))
    d_64 = float(np.linalg.norm((np.linalg.inv(A).astype(LD) - ref).astype(np.float64)))
    asym = float(np.linalg.norm(f.cinv - f.cinv.T))
    # the fetched A is symmetric to the rounding of the product that formed it only, and its exact
    # inverse is as unsymmetric as |A^-1|^2 |A - A^T|: that part is the reference's, not the kernel's
    asym_ref = float(np.linalg.norm((ref - ref.T).astype(np.float64)))
    print(f"coarsest inverse {name}: n {n}, cond {np.linalg.cond(A):.2e}, d_gpu {d_gpu:.3e}, d_64 {d_64:.3e}, "
          f"d_gpu / d_64 {d_gpu / d_64:.3f}, asymmetry {asym:.3e}, of the exact inverse {asym_ref:.3e}")
    assert d_gpu <= CINV_MARGIN * d_64
    assert asym <= 2 * d_gpu + 2 * d_64 + asym_ref


# ------------------------------------------------------------------------------- 9. the V-cycle
def _references(f, nu):
    A = [_sparse(f, "A", l, np.float64) for l in range(f.nl)]
    P = [_sparse(f, "P", l, np.float64) for l in range(f.nl - 1)]
    return _cycles(A, P, f.dinv, f.lmax, nu, f.a.opt.ratio, f.a.opt.boost, cinv_ld=_cinv_ld(f))


VCYCLE = [("h8_633", 2, "1"), ("h8_633", 1, "1"), ("h8_633", 3, "1"), ("h8_633", 2, "0"), ("h8_633_totlag", 2, "1"),
          ("h27_322", 2, "1"), ("roller", 2, "1"), ("line_12", 2, "1"), ("local", 2, "1")]


@gpu
@pytest.mark.parametrize("name,nu,reorder", VCYCLE)
def test_vcycle_is_the_operator_it_claims(name, nu, reorder):
    f = _build(name, env={} if reorder == "1" else {"FCG_AMG_REORDER": "0"}, **({} if nu == 2 else {"nu": nu}))
    mesh, ev, rows, K, Kh = _system(name)
    n = mesh.n_rows
    assert f.a.opt.nu == nu
    I = torch.eye(n, dtype=torch.float64, device=_dev())
    M = torch.full((n, n), float("nan"), dtype=torch.float64, device=_dev())  # row j = M e_j
    for j in range(n):
        f.a.apply(K, I[j], M[j])
    torch.cuda.synchronize()
    M = M.cpu().numpy().T
    ref = {}
    for dt, c in zip((np.float64, LD), _references(f, nu)):
        R = np.zeros((n, n), dtype=dt)
        R[np.ix_(f.dof, f.dof)] = c.matrix()  # level 0's order back to the caller's
        ref[dt] = R
    own = float(np.linalg.norm((ref[np.float64].astype(LD) - ref[LD]).astype(np.float64)))
    err = float(np.linalg.norm((M.astype(LD) - ref[LD]).astype(np.float64)))
    free = np.setdiff1d(np.arange(n), rows)
    Mff = M[np.ix_(free, free)]
    asym = float(np.linalg.norm(Mff - Mff.T))
    ptr, col, vals = amg_ref.node_blocks(mesh.rowptr, mesh.col_lid, Kh, n)
    Aff = amg_ref.bsr_dense(ptr, col, vals, n // 3)[np.ix_(free, free)]
    evs = _spectrum(Mff, Aff)
    top = 1 + 8 * own * np.linalg.norm(Aff, 2)
    print(f"V-cycle {name} nu {nu} reorder {reorder}: levels {[i['dofs'] for i in f.info]}, |M - M_ld| {err:.3e}, "
          f"own {own:.3e}, |M_ff - M_ff^T| {asym:.3e}, eig(M A_ff) in [{evs.min():.5f}, {evs.max():.12f}], "
          f"upper end allowed 1 + {top - 1:.2e}")
    assert np.all(np.isfinite(M)) and err <= 8 * own
    assert asym <= 8 * own
    assert np.linalg.norm(Aff - Aff.T) <= 1e-13 * np.linalg.norm(Aff)
    assert evs.min() > 0 and evs.max() <= top


# ------------------------------------------------------------------------------ 10. large cases
@gpu
@pytest.mark.parametrize("name", LARGE)
def test_vcycle_on_right_hand_sides(name):
    f = _build(name)
    mesh, ev, rows, K, Kh = _system(name)
    n = mesh.n_rows
    B = np.random.default_rng(29).standard_normal((n, 4))
    B[rows] = 0.0
    Z = np.empty_like(B)
    for j in range(4):
        z = torch.full((n,), float("nan"), dtype=torch.float64, device=_dev())
        f.a.apply(K, _t(B[:, j]), z)
        Z[:, j] = z.cpu().numpy()
    c64, cld = _references(f, f.a.opt.nu)
    Z64, Zld = np.empty((n, 4)), np.empty((n, 4), dtype=LD)
    Z64[f.dof], Zld[f.dof] = c64.apply(B[f.dof]), cld.apply(B[f.dof])
    own = np.linalg.norm((Z64.astype(LD) - Zld).astype(np.float64), axis=0)
    err = np.linalg.norm((Z.astype(LD) - Zld).astype(np.float64), axis=0)
    print(f"V-cycle {name}: levels {[i['dofs'] for i in f.info]}, |z - z_ld| " + " ".join(f"{v:.3e}" for v in err)
          + ", |z_f64 - z_ld| " + " ".join(f"{v:.3e}" for v in own))
    assert np.all(np.isfinite(Z)) and np.all(err <= 8 * own)


# -------------------------------------------------------------------------------- 11. refusals
@gpu
def test_refusals():
    name = "h8_633"
    mesh, ev, rows, K, Kh = _system(name)
    L = fcg.lib()
    a = amg.NativeAMG(mesh, ev, rows, **CASES[name]["opts"])
    info = a.describe()
    nl = len(info)
    for l in range(nl):  # the all-NULL count query agrees with describe()
        b = 3 if l == 0 else 6
        assert L.fcg_amg_level_matrix(a._h, l, 0, None, None, None, 0) == info[l]["blocks"] * b * b
        assert L.fcg_amg_level_matrix(a._h, l, 3, None, None, None, 0) == info[l]["dofs"] * b
        if l + 1 < nl:
            for which in (1, 2):
                assert L.fcg_amg_level_matrix(a._h, l, which, None, None, None, 0) % (b * 6) == 0
    assert L.fcg_amg_level_matrix(a._h, 0, 2, None, None, None, 0) == 18 * int((~_build(name).dbc0.all(axis=1)).sum())
    with pytest.raises(RuntimeError):  # before any numeric setup
        a.level_matrix(0, 0)
    assert L.fcg_amg_level_matrix(a._h, nl - 1, 4, None, None, None, 0) == -1  # no inverse yet
    a.setup(K)
    count = L.fcg_amg_level_matrix(a._h, 0, 0, None, None, None, 0)
    ptr, col = np.zeros(info[0]["dofs"] // 3 + 1, dtype=np.int64), np.zeros(info[0]["blocks"], dtype=np.int32)
    vals = np.full(count, np.nan)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert L.fcg_amg_level_matrix(a._h, 0, 0, vp(ptr), vp(col), vp(vals), count - 1) == -1  # short capacity
    assert np.all(np.isnan(vals))
    assert L.fcg_amg_level_matrix(a._h, 0, 0, vp(ptr), vp(col), vp(vals), count) == count
    assert _same(vals.reshape(-1, 3, 3), _build(name).A[0][2])
    n_last = info[-1]["dofs"]
    assert L.fcg_amg_level_matrix(a._h, nl - 1, 4, None, None, None, 0) == n_last * n_last
    for bad in ((0, 4), (nl - 2, 4), (nl - 1, 1), (nl - 1, 2), (nl, 0), (-1, 0), (0, 5), (0, -1)):
        assert L.fcg_amg_level_matrix(a._h, bad[0], bad[1], None, None, None, 0) == -1, bad
    assert L.fcg_amg_level_matrix(None, 0, 0, None, None, None, 0) == -1
    with _env({"FCG_AMG_DENSE": "0"}):
        a.setup(K)
    assert not a.stats()["coarse_dense"]
    assert L.fcg_amg_level_matrix(a._h, nl - 1, 4, None, None, None, 0) == -1
    with pytest.raises(ValueError):
        a.level_matrix(nl - 1, 4)
    a.close()
