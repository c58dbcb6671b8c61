"""Explicit dynamics: fcg_centrdiff_step, fcg_stable_dt and dynamics.CentralDifference.

The yardstick is ref_centrdiff below, a numpy restatement of the step's definition
(include/fourc_gpu.h).  The CPU tests validate it and the Gershgorin bound on the CPU oracle's K
and test_mass's numpy mass reference; the GPU tests compare the kernels with numpy formulas and
the driver with ref_centrdiff driven by the oracle's internal force.

Measured on an MI355X: see the docstrings of the trajectory tests and profiles/explicit/README.md.
"""

import importlib
import math

import numpy as np
import pytest

import oracle_lib as orc
from parity_util import oracle_evaluate, oracle_evaluate_single
from test_mass import MassRef

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")
dynamics = importlib.import_module("4c_amd.dynamics")

gpu = pytest.mark.gpu
E, NU, RHO = 210.0, 0.3, 0.05
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------ the yardstick
def ref_centrdiff(fext, fint, m, fixed, d0, v0, dt, nsteps, damp_m=0.0):
    """The recurrence of fcg_centrdiff_step, call by call: fext t -> [n], fint d -> [n], fixed a
    bool mask.  Returns D [nsteps + 2] (d_0 .. d_{nsteps+1}), VH [nsteps + 1] (v_{n+1/2}),
    V and A [nsteps + 1] (v_n, a_n)."""
    d, vh = np.array(d0, dtype=np.float64), np.array(v0, dtype=np.float64)
    D, VH, V, A = [d], [], [], []
    for n in range(nsteps + 1):
        a = np.where(fixed, 0.0, (fext(n * dt) - fint(d)) / m - damp_m * vh)
        v = np.where(fixed, 0.0, vh + 0.5 * (dt if n else 0.0) * a)
        vh = np.where(fixed, 0.0, v + 0.5 * dt * a)
        d = np.where(fixed, d, d + dt * vh)
        for H, x in ((D, d), (VH, vh), (V, v), (A, a)):
            H.append(x)
    return np.array(D), np.array(VH), np.array(V), np.array(A)


def row_sum_bound(rowptr, K, m, fixed):
    """max over the free rows of sum_j |K_ij| / m_i from CSR values."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    s = np.zeros(len(rowptr) - 1)
    np.add.at(s, rows, np.abs(K))
    return float(np.max((s / m)[~fixed]))


def lambda_max(mesh, K, m, fixed):
    """The largest eigenvalue of M_l^-1/2 K_ff M_l^-1/2 on the free rows (single rank)."""
    A = np.zeros((mesh.n_rows, mesh.n_cols))
    A[np.repeat(np.arange(mesh.n_rows), np.diff(mesh.rowptr)), mesh.col_lid] = K
    f = np.nonzero(~fixed)[0]
    s = 1.0 / np.sqrt(m[f])
    Kff = A[np.ix_(f, f)]
    return float(np.linalg.eigvalsh(0.5 * (Kff + Kff.T) * np.outer(s, s))[-1])


class Problem:
    """A single-rank mesh clamped at x = 0 with its reference operators: the oracle's K at u = 0
    (linear) as CSR values and dense, the numpy reference's lumped mass, the fixed mask and a
    nodal tip load in -z on the face x = max."""

    def __init__(self, mesh, rho=RHO, load=1e-2):
        self.mesh = mesh
        self.n = mesh.n_rows
        X = mesh.node_x
        clamped = np.nonzero(np.isclose(X[:, 0], X[:, 0].min()))[0]
        self.dbc = np.sort((mesh.node_dof_row[clamped][:, None] + np.arange(3)).ravel()).astype(np.int32)
        self.fixed = np.zeros(self.n, dtype=bool)
        self.fixed[self.dbc] = True
        tip = np.nonzero(np.isclose(X[:, 0], X[:, 0].max()))[0]
        self.fext = np.zeros(self.n)
        self.fext[mesh.node_dof_row[tip] + 2] = -load / len(tip)
        self.rho = rho
        self.m = MassRef(mesh, rho).lumped(self.n)
        err, _, self.K, _ = self.oracle(fcg.LINEAR, np.zeros(mesh.n_cols), True)
        assert err == 0
        self.Kd = np.zeros((self.n, mesh.n_cols))
        self.Kd[np.repeat(np.arange(self.n), np.diff(mesh.rowptr)), mesh.col_lid] = self.K

    def oracle(self, kinem, u, want_k, material=orc.MAT_STVK):
        if isinstance(self.mesh, fcg.BoxMesh):
            return oracle_evaluate(self.mesh, kinem, E, NU, u, want_k=want_k, material=material)
        assert material == orc.MAT_STVK
        return oracle_evaluate_single(self.mesh, kinem, E, NU, u, want_k=want_k)

    def gershgorin_dt(self):
        return 2.0 / math.sqrt(row_sum_bound(self.mesh.rowptr, self.K, self.m, self.fixed))


_problems = {}


def _problem(name):
    """Built once per name and left unchanged."""
    if name not in _problems:
        make = {
            "h8_322": lambda: fcg.BoxMesh(fcg.HEX8, (3, 2, 2), upper=(3.0, 1.0, 1.0)),
            "h8_422": lambda: fcg.BoxMesh(fcg.HEX8, (4, 2, 2), upper=(4.0, 1.0, 1.0)),
            "h8_333_jit": lambda: fcg.BoxMesh(fcg.HEX8, (3, 3, 3), jitter=0.15),
            "h27_221_jit": lambda: fcg.BoxMesh(fcg.HEX27, (2, 2, 1), jitter=0.1),
            "h27_221": lambda: fcg.BoxMesh(fcg.HEX27, (2, 2, 1), upper=(2.0, 1.0, 0.5)),
            "h27_221_renumbered": lambda: fcg.Discretization.renumbered(
                fcg.BoxMesh(fcg.HEX27, (2, 2, 1), upper=(2.0, 1.0, 0.5))),
        }[name]
        _problems[name] = Problem(make())
    return _problems[name]


def invariant(VH, D, m, Kd):
    """H_n = 1/2 vhalf_n^T M vhalf_n + 1/2 d_n^T K d_{n+1} and the scale of its terms."""
    kin = 0.5 * np.einsum("ni,i,ni->n", VH, m, VH)
    pot = 0.5 * np.einsum("ni,ij,nj->n", D[:-1], Kd, D[1:])
    return kin + pot, float(np.max(kin + np.abs(pot)))


# ------------------------------------------------------------------------------ CPU
def test_reference_recurrence_conserves_the_discrete_invariant():
    """The unloaded, undamped recurrence on the oracle's K of the clamped linear hex8 (3,2,2) box
    from a random v_0 conserves H_n = 1/2 v_{n+1/2}^T M v_{n+1/2} + 1/2 d_n^T K d_{n+1} (multiply
    M (d_{n+1} - 2 d_n + d_{n-1}) = -dt^2 K d_n by d_{n+1} - d_{n-1}): N = 200 steps at half the
    Gershgorin step, |H_n - H_0| <= N 1e-12 x the size of its terms."""
    p = _problem("h8_322")
    N, dt = 200, 0.5 * p.gershgorin_dt()
    v0 = np.random.default_rng(11).standard_normal(p.n)
    zero = np.zeros(p.n)
    D, VH, _, _ = ref_centrdiff(lambda t: zero, lambda d: p.Kd @ d, p.m, p.fixed, zero, v0, dt, N)
    H, scale = invariant(VH, D, p.m, p.Kd)
    drift = float(np.abs(H - H[0]).max())
    print("dt", dt, "H_0", H[0], "max |H_n - H_0| / scale", drift / scale)
    assert np.all(D[:, p.fixed] == 0.0)
    assert H[0] > 0.0 and drift <= N * 1e-12 * scale


@pytest.mark.parametrize("name", ["h8_333_jit", "h27_221_jit"])
def test_row_sum_bound_is_above_lambda_max(name):
    """Gershgorin on M_l^-1 K with the clamped face's rows left out: the row-sum bound is not below
    the largest eigenvalue of M_l^-1/2 K_ff M_l^-1/2."""
    p = _problem(name)
    bound = row_sum_bound(p.mesh.rowptr, p.K, p.m, p.fixed)
    lmax = lambda_max(p.mesh, p.K, p.m, p.fixed)
    print(name, "lambda_max / bound", lmax / bound, "dt_bound / dt_exact", math.sqrt(lmax / bound))
    assert bound >= lmax * (1.0 - 1e-12)


# ------------------------------------------------------------------------------ GPU helpers
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(_dev())


def _h(t):
    return t.cpu().numpy()


_contexts = {}


def _context(celltype, iv):
    _dev()
    key = (celltype, iv)
    if key not in _contexts:
        mesh = fcg.BoxMesh(celltype, iv)
        _contexts[key] = (mesh, fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU))
    return _contexts[key]


def _evaluator(p, kinem=fcg.LINEAR, material=fcg.MAT_STVK):
    _dev()
    return fcg.Evaluator(p.mesh, kinematics=kinem, youngs=E, poisson=NU, material=material)


def _step_inputs(n, seed):
    rng = np.random.default_rng(seed)
    x = {k: rng.standard_normal(n) for k in ("fext", "fint", "vhalf", "d")}
    x["m"] = rng.uniform(0.5, 2.0, n)
    fixed = rng.random(n) < 0.3
    fixed[0], fixed[1] = True, False  # at least one of each
    x["fixed"] = rng.permutation(fixed)
    return x


def _offset_view(a):
    """The array on the device in a buffer one double longer, from its second double on: the base
    is 8-byte but not 16-byte aligned."""
    buf = torch.empty(len(a) + 2, dtype=torch.float64, device=_dev())
    k = 1 if buf.data_ptr() % 16 == 0 else 2
    view = buf[k:k + len(a)]
    view.copy_(_t(a))
    assert view.data_ptr() % 16 == 8
    return view


def _call_step(ev, x, dtp, dtn, damp, skip=(), offset=None):
    """One fcg_centrdiff_step from the inputs x; returns the outputs as numpy arrays."""
    dev = _dev()
    t = {k: (_offset_view(x[k]) if k == offset else _t(x[k])) for k in ("fext", "fint", "m", "d", "vhalf")}
    n = len(x["m"])
    out = {k: (None if k in skip else (_offset_view(np.full(n, np.nan)) if k == offset else
                                       torch.full((n,), float("nan"), dtype=torch.float64, device=dev)))
           for k in ("v", "a")}
    ekin = None if "ekin" in skip else torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    fixed = _t(x["fixed"].astype(np.uint8), torch.uint8)
    ev.centrdiff_step(dtp, dtn, damp, t["fext"], t["fint"], t["m"], fixed, t["d"], t["vhalf"],
                      out["v"], out["a"], ekin)
    got = {"d": _h(t["d"]), "vhalf": _h(t["vhalf"])}
    for k in ("v", "a"):
        if out[k] is not None:
            got[k] = _h(out[k])
    if ekin is not None:
        got["ekin"] = float(ekin)
    return got


def _check_step(x, dtp, dtn, damp, got):
    """Every entry against the definition evaluated in extended precision, at 4 eps x the sum of
    the absolute values of the terms of the entry's expanded expression: the kernel takes at most
    eight roundings of half an eps each from the inputs to d' (subtract, divide, multiply, subtract,
    then multiply and add three times), fewer with fused multiply-adds, each relative to a partial
    result no larger than that sum."""
    L = np.longdouble
    assert np.finfo(L).eps < 1e-18
    fe, fi, m, vh, d = (x[k].astype(L) for k in ("fext", "fint", "m", "vhalf", "d"))
    fx = x["fixed"]
    hp, hn, dn, c = L(0.5) * L(dtp), L(0.5) * L(dtn), L(dtn), L(damp)
    a = (fe - fi) / m - c * vh
    ta = np.abs(fe / m) + np.abs(fi / m) + np.abs(c * vh)
    v = vh + hp * a
    tv = np.abs(vh) + hp * ta
    vh1 = v + hn * a
    th = tv + hn * ta
    d1 = d + dn * vh1
    td = np.abs(d) + dn * th
    for name, want, terms in (("a", a, ta), ("v", v, tv), ("vhalf", vh1, th), ("d", d1, td)):
        g = got[name]
        assert np.all(g[fx] == (x["d"][fx] if name == "d" else 0.0)), name
        err = np.abs(g.astype(L) - want)[~fx]
        bound = (4 * EPS * terms)[~fx]
        assert np.all(err <= bound), (name, float(np.max(err / np.maximum(bound, L(1e-300)))))
    if dtn == 0.0:
        assert np.array_equal(got["d"], x["d"])
        assert np.array_equal(got["vhalf"], got["v"])
    terms = 0.5 * x["m"] * got["v"] ** 2
    want = math.fsum(terms)
    assert abs(got["ekin"] - want) <= len(terms) * EPS * math.fsum(np.abs(terms)), (got["ekin"], want)


STEP_CONTEXTS = [(fcg.HEX8, (1, 1, 1), 24), (fcg.HEX27, (1, 1, 1), 81), (fcg.HEX8, (3, 2, 2), 108),
                 (fcg.HEX8, (12, 12, 12), 6591)]
STEP_PARAMS = [(0.013, 0.021, 0.0), (0.013, 0.021, 0.4), (0.0, 0.02, 0.4), (0.02, 0.0, 0.4),
               (0.02, 0.0, 0.0)]


# ------------------------------------------------------------------------------ GPU: the kernels
@gpu
@pytest.mark.parametrize("celltype,iv,rows", STEP_CONTEXTS)
def test_centrdiff_step_against_formula(celltype, iv, rows):
    """Row counts below a wavefront (24), odd (81: the scalar tail of the 16-byte path), no
    multiple of 64 (108) and odd over several workgroups and partials (6591); dt_prev != dt_next,
    either zero, damping on and off; every optional output NULL in turn; an input and an output
    that start 8 bytes off a 16-byte boundary (one row per lane); two calls give the same bits."""
    mesh, ev = _context(celltype, iv)
    assert mesh.n_rows == rows
    for k, (dtp, dtn, damp) in enumerate(STEP_PARAMS):
        x = _step_inputs(rows, 100 + k)
        full = _call_step(ev, x, dtp, dtn, damp)
        _check_step(x, dtp, dtn, damp, full)
        again = _call_step(ev, x, dtp, dtn, damp)
        for name in full:
            assert np.array_equal(np.asarray(full[name]), np.asarray(again[name])), name
        if k > 1:
            continue
        for skip in ("v", "a", "ekin"):
            part = _call_step(ev, x, dtp, dtn, damp, skip=(skip,))
            assert skip not in part
            for name in part:  # the other outputs do not depend on which ones are asked for
                assert np.array_equal(np.asarray(part[name]), np.asarray(full[name])), (skip, name)
        for offset in ("fint", "d", "v"):
            shifted = _call_step(ev, x, dtp, dtn, damp, offset=offset)
            _check_step(x, dtp, dtn, damp, shifted)
            again = _call_step(ev, x, dtp, dtn, damp, offset=offset)
            for name in shifted:
                assert np.array_equal(np.asarray(shifted[name]), np.asarray(again[name])), name


@gpu
def test_refusals_and_the_empty_context():
    mesh, ev = _context(fcg.HEX8, (3, 2, 2))
    x = _step_inputs(mesh.n_rows, 5)
    for dtp, dtn, damp in ((-0.1, 0.1, 0.0), (0.1, -0.1, 0.0), (0.1, 0.1, -1.0), (float("nan"), 0.1, 0.0),
                           (0.1, float("nan"), 0.0), (0.1, float("inf"), 0.0), (0.1, 0.1, float("inf"))):
        with pytest.raises(fcg.FcgError) as ei:
            _call_step(ev, x, dtp, dtn, damp)
        assert ei.value.code == fcg.FCG_ERR_ARG
    t = {k: _t(x[k]) for k in ("fext", "fint", "m", "d", "vhalf")}
    for missing in t:
        args = dict(t)
        args[missing] = None
        with pytest.raises(fcg.FcgError) as ei:
            ev.centrdiff_step(0.1, 0.1, 0.0, args["fext"], args["fint"], args["m"], None, args["d"],
                              args["vhalf"])
        assert ei.value.code == fcg.FCG_ERR_ARG
    with pytest.raises(fcg.FcgError) as ei:
        ev.stable_dt(None, t["m"])
    assert ei.value.code == fcg.FCG_ERR_ARG
    # hex8 (3,2,2) split over 16 ranks leaves rank 2 without rows: no-ops with NULL buffers
    empty = fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1, rank=2, nranks=16)
    assert empty.n_rows == 0
    ev0 = fcg.Evaluator(empty, kinematics=fcg.TOTLAG, youngs=E, poisson=NU)
    L = fcg.lib()
    assert L.fcg_centrdiff_step(ev0._h, 0.1, 0.1, 0.0, *([None] * 10)) == fcg.FCG_OK
    assert ev0.stable_dt(None, None) == (float("inf"), 0.0)


STABLE_CASES = [("h8_333_jit", fcg.LINEAR), ("h27_221_jit", fcg.LINEAR), ("h8_322", fcg.LINEAR),
                ("h8_322", fcg.TOTLAG)]


@gpu
@pytest.mark.parametrize("name,kinem", STABLE_CASES)
def test_stable_dt(name, kinem):
    """lambda_bound equals the numpy row-sum bound of the library's own K and lumped mass (the
    existing evaluate and mass, copied to the host) to 1e-13, lies above lambda_max and gives
    dt_crit = 2 / sqrt(lambda_bound); the refusals name the row and leave evaluate's flags alone."""
    dev = _dev()
    p = _problem(name)
    mesh = p.mesh
    ev = _evaluator(p, kinem)
    u = _t(mesh.u_col(2e-2) if kinem == fcg.TOTLAG else np.zeros(mesh.n_cols))
    K = torch.empty(mesh.nnz, dtype=torch.float64, device=dev)
    f = torch.empty(mesh.n_rows, dtype=torch.float64, device=dev)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K)
    _, m = ev.mass_nodal(RHO)
    fixed = _t(p.fixed.astype(np.uint8), torch.uint8)
    bytes0 = ev.info.device_bytes
    dt, lam = ev.stable_dt(K, m, fixed)
    bytes1 = ev.info.device_bytes
    assert bytes1 > bytes0  # the partial buffer is counted ...
    want = row_sum_bound(mesh.rowptr, _h(K), _h(m), p.fixed)
    lmax = lambda_max(mesh, _h(K), _h(m), p.fixed)
    print(name, kinem, "lambda_bound", lam, "numpy", want, "dt / dt_exact", math.sqrt(lmax / lam))
    assert abs(lam - want) <= 1e-13 * want
    assert lam >= lmax * (1.0 - 1e-12)
    assert dt == 2.0 / math.sqrt(lam)
    assert ev.stable_dt(K, m, fixed) == (dt, lam)
    ekin = torch.zeros(1, dtype=torch.float64, device=dev)
    ev.centrdiff_step(0.0, 0.0, 0.0, f, f, m, fixed, f.clone(), f.clone(), ekin=ekin)
    assert ev.info.device_bytes == bytes1  # ... and allocated once, shared by the two entry points
    # without a mask no row is skipped
    assert abs(ev.stable_dt(K, m)[1] - row_sum_bound(mesh.rowptr, _h(K), _h(m), np.zeros(p.n, bool))) <= 1e-13 * want
    assert ev.stable_dt(K, m, torch.ones_like(fixed)) == (float("inf"), 0.0)
    # refusals: the lowest refused free row is named; a refused fixed row is not looked at
    free = np.nonzero(~p.fixed)[0]
    r0, r1 = int(free[3]), int(free[len(free) // 2])
    for bad_value in (0.0, -1.0, float("nan"), float("inf")):
        mb = m.clone()
        mb[r1] = bad_value
        mb[r0] = bad_value
        mb[int(p.dbc[0])] = bad_value
        with pytest.raises(fcg.FcgError, match=r"row %d\b" % r0) as ei:
            ev.stable_dt(K, mb, fixed)
        assert ei.value.code == fcg.FCG_ERR_ARG
    Kb = K.clone()
    Kb[int(mesh.rowptr[r1]) + 1] = float("nan")
    with pytest.raises(fcg.FcgError, match=r"row %d\b" % r1) as ei:
        ev.stable_dt(Kb, m, fixed)
    assert ei.value.code == fcg.FCG_ERR_ARG
    ev.check_error()  # nothing pending: the sticky flags are untouched
    f2 = torch.empty_like(f)
    ev.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f2)
    assert np.array_equal(_h(f2), _h(f))
    assert ev.stable_dt(K, m, fixed) == (dt, lam)


# ------------------------------------------------------------------------------ GPU: the driver
def _history(cd, nsteps):
    """initialize() has run; steps one at a time: D [nsteps + 1] (d_1 ..), VH, V, A [nsteps + 1]."""
    D, VH, V, A = [], [], [], []
    for n in range(nsteps + 1):
        if n:
            cd.run(1)
        for H, x in ((D, cd.d), (VH, cd.vhalf), (V, cd.v), (A, cd.a)):
            H.append(_h(x).copy())
    return np.array(D), np.array(VH), np.array(V), np.array(A)


def _parity(p, ev, fint, nsteps, fext, v0, label):
    """The driver at 0.8 stable_dt() against ref_centrdiff with the same dt; returns the relative
    deviations of d and v (maximum over steps and rows / maximum of the reference)."""
    cd = dynamics.CentralDifference(ev, p.rho, 1.0, fext, p.dbc)
    cd.dt = dt = cd.stable_dt(0.8)
    cd.initialize(v0=v0)
    D, VH, V, A = _history(cd, nsteps)
    zero = np.zeros(p.n)
    Dr, VHr, Vr, Ar = ref_centrdiff(lambda t: fext, fint, p.m, p.fixed, zero,
                                    zero if v0 is None else v0, dt, nsteps)
    dev_d = np.abs(D - Dr[1:]).max() / np.abs(Dr).max()
    dev_v = np.abs(V - Vr).max() / np.abs(Vr).max()
    print(label, "dt", dt, "max |u|", np.abs(Dr).max(), "deviation of d", dev_d, "of v", dev_v)
    assert np.all(D[:, p.fixed] == 0.0) and np.all(V[:, p.fixed] == 0.0) and np.all(A[:, p.fixed] == 0.0)
    assert cd.nstep == nsteps and abs(cd.t - nsteps * dt) <= 1e-12 * nsteps * dt
    # the same steps queued in one run(): the same bits
    cd2 = dynamics.CentralDifference(ev, p.rho, dt, fext, p.dbc)
    cd2.initialize(v0=v0)
    cd2.run(nsteps, check_every=7)
    assert np.array_equal(_h(cd2.d), D[-1]) and np.array_equal(_h(cd2.v), V[-1])
    assert cd2.energies() == cd.energies()
    return dev_d, dev_v


@gpu
@pytest.mark.parametrize("name", ["h8_422", "h27_221_renumbered"])
def test_linear_trajectory(name):
    """A step tip load on the clamped linear mesh, N = 40 steps at 0.8 stable_dt(): d and v follow
    ref_centrdiff driven by the oracle's K d to N 1e-10 (the project's internal-force parity
    figure; below the stability limit a per-step perturbation grows at most linearly in N).
    Measured on an MI355X (d / v): hex8 6.7e-15 / 2.3e-14, hex27 1.8e-13 / 4.4e-13."""
    p = _problem(name)
    N = 40
    dev_d, dev_v = _parity(p, _evaluator(p), lambda d: p.Kd @ d, N, p.fext, None, name)
    assert dev_d <= N * 1e-10 and dev_v <= N * 1e-10


@gpu
@pytest.mark.parametrize("name,material", [("h8_322", fcg.MAT_STVK),
                                           ("h27_221", fcg.MAT_ELASTHYPER_COUPNEOHOOKE)])
def test_nonlinear_trajectory(name, material):
    """TotLag, N = 20 steps from a v_0 that takes |u| to about 2e-2, against ref_centrdiff with the
    oracle's internal force at every step; the same N 1e-10 (the linearised recurrence is the same
    stable scheme while K(d) stays positive definite).  Measured on an MI355X (d / v, max |u|):
    hex8 5.7e-14 / 5.5e-13, 1.68e-2; hex27 2.4e-14 / 1.3e-13, 1.90e-2."""
    p = _problem(name)
    N = 20
    omat = orc.MAT_STVK if material == fcg.MAT_STVK else orc.MAT_NEOHOOKE
    ev = _evaluator(p, fcg.TOTLAG, material)
    dt = dynamics.CentralDifference(ev, p.rho, 1.0, np.zeros(p.n), p.dbc).stable_dt(0.8)
    # a bending velocity field, v_z ~ (x / L)^2: the run is short against the first period, so the
    # tip drifts by nearly N dt max |v_0|
    X = p.mesh.node_x
    shape = np.zeros(p.n)
    shape[p.mesh.node_dof_row + 2] = (X[:, 0] / X[:, 0].max()) ** 2
    shape[p.fixed] = 0.0
    v0 = shape * (2e-2 / (N * dt))

    def fint(d):
        err, _, _, f = p.oracle(fcg.TOTLAG, d, False, omat)
        assert err == 0
        return f

    dev_d, dev_v = _parity(p, ev, fint, N, np.zeros(p.n), v0, name)
    assert dev_d <= N * 1e-10 and dev_v <= N * 1e-10


@gpu
def test_discrete_invariant_on_the_device():
    """The CPU test's H_n from the driver's vhalf and d, the oracle's K and the reference mass:
    N = 100 steps at half of stable_dt(), |H_n - H_0| <= N 1e-12 x the size of its terms."""
    p = _problem("h8_322")
    N = 100
    cd = dynamics.CentralDifference(_evaluator(p), p.rho, 1.0, np.zeros(p.n), p.dbc)
    cd.dt = cd.stable_dt(0.5)
    v0 = np.random.default_rng(11).standard_normal(p.n)
    cd.initialize(v0=v0)
    D, VH, _, _ = _history(cd, N)
    H, scale = invariant(VH, np.vstack([np.zeros((1, p.n)), D]), p.m, p.Kd)
    drift = float(np.abs(H - H[0]).max())
    print("dt", cd.dt, "H_0", H[0], "max |H_n - H_0| / scale", drift / scale)
    assert H[0] > 0.0 and drift <= N * 1e-12 * scale


@gpu
def test_mass_damping_dissipates():
    p = _problem("h8_322")
    cd = dynamics.CentralDifference(_evaluator(p), p.rho, 1.0, np.zeros(p.n), p.dbc)
    cd.dt = cd.stable_dt(0.5)
    cd.damp_m = 0.02 / cd.dt
    cd.initialize(v0=np.random.default_rng(12).standard_normal(p.n))
    e0 = cd.energies()[0] + cd.internal_energy()
    # displacement() is d_1 - dt v_{1/2} = d_0 = 0 to rounding, its energy the square of that
    assert cd.energies()[1] is None and cd.internal_energy() <= 1e-24 * e0
    cd.run(50)
    e50 = cd.energies()[0] + cd.internal_energy()
    print("energy at step 0", e0, "at step 50", e50)
    assert cd.internal_energy() > 0.0 and 0.0 < e50 < e0


@gpu
def test_run_restores_the_async_setting():
    """run() queues the steps in async mode and puts the evaluator's setting back, also when an
    element error surfaces: a hex8 box whose corner node is pushed inwards has det J < 0 at that
    node (4C's nodal check, FCG_ERR_NODAL_DETJ from the evaluate) and det J > 0 at every Gauss
    point (the mass is fine) -- the library's own error code, no device fault."""
    p = _problem("h8_322")
    ev = _evaluator(p)
    for prev in (False, True):
        ev.set_async(prev)
        cd = dynamics.CentralDifference(ev, p.rho, 1e-3, p.fext, p.dbc)
        cd.run(5, check_every=2)
        assert ev.async_enabled == prev and cd.nstep == 5
        cd = dynamics.CentralDifference(ev, p.rho, 1e-3, lambda t: p.fext, p.dbc)
        cd.run(3)
        assert ev.async_enabled == prev and cd.nstep == 3
    ev.set_async(False)

    mesh = fcg.BoxMesh(fcg.HEX8, (2, 2, 2))
    corner = np.nonzero(np.all(np.isclose(mesh.node_x, 0.0), axis=1))[0][0]
    mesh.node_x[corner, :2] = 0.55 * 0.5
    bad = [int(g) for g, en in zip(mesh.ele_gid, mesh.ele_nodes)
           if orc.solid_evaluate(fcg.HEX8, fcg.LINEAR, E, NU, mesh.node_x[en], np.zeros((8, 3)),
                                 want_k=False)[0] == 1]
    assert len(bad) == 1
    evb = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    for prev in (False, True):
        evb.set_async(prev)
        cd = dynamics.CentralDifference(evb, RHO, 1e-3, np.zeros(mesh.n_rows), [])
        with pytest.raises(fcg.FcgError, match="steps 0..") as ei:
            cd.run(4, check_every=3)
        assert ei.value.code == fcg.FCG_ERR_NODAL_DETJ and ei.value.bad_ele_gid == bad[0]
        assert evb.async_enabled == prev
        evb.check_error()  # reported once
    evb.set_async(False)
