"""The one-step-theta pass (fcg_tsi_ost_combine) and the transient drivers on the device:
thermo.OneStepTheta and tsi.TsiMonolithic(thermal="ost"), against thermo_ref.py.

The combine kernel is judged like the capacity (test_tsi_capacity.py): against the longdouble
restatement thermo_ref.combine, e(device) <= 4 * max(e(f64 restatement), e_A(f64 restatement)) in both
measures, e_A on the benign state (T_n = T - 0.1 field, theta = 1, dt = 1) of the same mesh.

The drivers are compared with dense longdouble host steppings under a derived bound: with kappa the
condition number of the effective matrix (C/dt + theta K, Dirichlet rows applied; for TSI the stacked
effective matrix), a solve stopped at the relative residual lin_rtol has a forward error of at most
kappa lin_rtol, and |g| <= 1 for theta >= 1/2 carries the error of a step on unamplified, so after n
steps

    max |x_dev - x_ref| <= n kappa lin_rtol max|x| + 64 eps max|x|.

The heat content 1^T C T of the insulated box moves by at most (sum |C_ij|) times that bound.
"""

import functools
import importlib

import numpy as np
import pytest

import regimes_util
import thermo_ref as th
import tsi_ref as tr
from element_ref import EXTENDED, LD
from regimes_util import _entry
from thermo_ref import MAT, MESHES, mesh_of

pkg = importlib.import_module("4c_amd")
fcg = pkg.fcg
torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not EXTENDED, reason="np.longdouble has no 64-bit significand here")]

CAPA = 3.5
E, NU, ALPHA, T0, COND = MAT["youngs"], MAT["poisson"], MAT["thexpans"], MAT["inittemp"], MAT["conduct"]
EPS = float(np.finfo(np.float64).eps)
STATES = ("diff", "increment", "same")
THETAS, DTS = (0.5, 1.0), (1e-3, 1.0, 1e3)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


def _tev(mesh, g=None):
    return fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND, graph=g)


# ------------------------------------------------------------------------------ the combine kernel
def _combine_inputs(name):
    """Device K_TT, f_T and C at tsi_ref.smooth_fields, as float64 arrays, and the three T_n."""
    mesh, g = mesh_of(name)
    tev = _tev(mesh, g)
    _, v, Tn = tr.smooth_fields(mesh)
    T = np.zeros(g.n_cols_t)
    T[g.node_dof_col_t] = Tn
    field = np.zeros(g.n_cols_t)
    field[g.node_dof_col_t] = Tn - 293.0
    K, f = _nan(g.nnz_tt), _nan(g.n_rows_t)
    tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, _t(v), _t(T), fT=f, Ktt=K)
    C = tev.capacity(CAPA)
    rng = np.random.default_rng(11)
    h = rng.standard_normal(g.n_rows_t) * float(f.abs().mean())
    Tns = {"diff": T - 0.1 * field, "increment": T * (1 - 1e-9), "same": T.copy()}
    return tev, g, K.cpu().numpy(), f.cpu().numpy(), C, T, Tns, h


def _combine_entry(g, theta, dt, C, T, Tn, h, K, f):
    r = th.combine(g, theta, dt, C, T, Tn, h, K, f)
    K64, f64 = th.combine_f64(g, theta, dt, C, T, Tn, h, K, f)
    return {"K": _entry(r["K"], r["SK"], K64), "f": _entry(r["f"], r["Sf"], f64)}


@pytest.mark.parametrize("name", list(MESHES))
def test_combine_against_longdouble(name):
    _dev()
    tev, g, K, f, C, T, Tns, h = _combine_inputs(name)
    Cn = C.cpu().numpy()
    anchor = _combine_entry(g, 1.0, 1.0, Cn, T, Tns["diff"], h, K, f)
    Tt, ht = _t(T), _t(h)
    for state in STATES:
        Tnt = _t(Tns[state])
        for theta in THETAS:
            for dt in DTS:
                Kd, fd = _t(K), _t(f)
                tev.ost_combine(theta, dt, C, Tt, Tnt, h=ht, Ktt=Kd, fT=fd)
                K2, f2 = _t(K), _t(f)
                tev.ost_combine(theta, dt, C, Tt, Tnt, h=ht, Ktt=K2, fT=f2)
                assert torch.equal(Kd, K2) and torch.equal(fd, f2)        # two calls, the same bits
                # K only and f only: the halves of the full call
                K3, f3 = _t(K), _t(f)
                tev.ost_combine(theta, dt, C, Tt, Tnt, h=ht, Ktt=K3)
                tev.ost_combine(theta, dt, C, Tt, Tnt, h=ht, fT=f3)
                assert torch.equal(Kd, K3) and torch.equal(fd, f3)
                # h NULL is h = 0
                f4, f5 = _t(f), _t(f)
                tev.ost_combine(theta, dt, C, Tt, Tnt, fT=f4)
                tev.ost_combine(theta, dt, C, Tt, Tnt, h=torch.zeros_like(ht), fT=f5)
                assert torch.equal(f4, f5)
                if state == "same":   # the capacity term is exactly 0.0
                    assert np.array_equal(fd.cpu().numpy(), theta * f + h)
                    assert np.array_equal(f4.cpu().numpy(), theta * f)
                regimes_util.judge(f"ost_combine/{name}/{state}/theta{theta}/dt{dt}",
                                   _combine_entry(g, theta, dt, Cn, T, Tns[state], h, K, f), anchor,
                                   {"K": Kd.cpu().numpy(), "f": fd.cpu().numpy()}, {})
    tev.close()


def test_combine_argument_errors():
    _dev()
    mesh, g = mesh_of("h8")
    tev = _tev(mesh, g)
    C, K, f = tev.capacity(CAPA), _nan(g.nnz_tt), _nan(g.n_rows_t)
    T = _t(np.full(g.n_cols_t, 300.0))
    bad = [dict(theta=0.0), dict(theta=-0.5), dict(theta=1.5), dict(theta=float("nan")), dict(dt=0.0),
           dict(dt=-1.0), dict(dt=float("inf")), dict(dt=float("nan")), dict(Ktt=None, fT=None)]
    for kw in bad:
        a = dict(theta=0.5, dt=0.1, C=C, T=T, Tn=T, Ktt=K, fT=f)
        a.update(kw)
        with pytest.raises(fcg.FcgError) as e:
            tev.ost_combine(**a)
        assert e.value.code == 3, kw
    with pytest.raises(fcg.FcgError) as e:
        tev.ost_combine(0.5, 0.1, C, None, T, fT=f)   # a residual needs both temperatures
    assert e.value.code == 3
    torch.cuda.synchronize()
    assert torch.isnan(K).all() and torch.isnan(f).all()   # a refused call writes nothing
    tev.close()


# ------------------------------------------------------------------------------ conduction drivers
def _dense_tt(mesh, g):
    nt = g.n_rows_t
    K = th.dense(g.rowptr_tt, g.col_tt, th.conduction(mesh, g, COND), nt)
    C = th.dense(g.rowptr_tt, g.col_tt, th.capacity(mesh, g, CAPA)[0], nt)
    return K, C


def _kappa(K, C, theta, dt, dbc):
    A = (C / LD(dt) + LD(theta) * K).astype(np.float64)
    th.apply_dirichlet(A, np.zeros(len(A)), np.asarray(dbc, dtype=np.int64))
    return float(np.linalg.cond(A))


@pytest.mark.parametrize("theta", [0.5, 1.0])
def test_cosine_mode_on_the_device(theta):
    _dev()
    thermo = importlib.import_module("4c_amd.thermo")
    n, L, dt, A0, Tbar, nstep, rtol = 6, 3.0, 0.01, 25.0, 300.0, 8, 1e-13
    mesh = fcg.BoxMesh(fcg.HEX8, (n, 2, 2), lower=(0.0, 0.0, 0.0), upper=(L, 1.0, 1.0))
    g = fcg.TsiGraph(mesh)
    nt = g.n_rows_t
    K, C = _dense_tt(mesh, g)
    x = np.zeros(nt)
    x[g.node_dof_col_t] = np.asarray(mesh.node_x)[:, 0]
    pi = 4 * np.arctan(LD(1))
    mode = np.cos(pi * x.astype(LD) / LD(L))
    h = LD(L) / n
    phi = pi * h / LD(L)
    lam = LD(COND) / LD(CAPA) * 6 * (1 - np.cos(phi)) / (h * h * (2 + np.cos(phi)))
    gfac = (1 - (1 - LD(theta)) * LD(dt) * lam) / (1 + LD(theta) * LD(dt) * lam)
    T_init = (Tbar + A0 * mode).astype(np.float64)
    kappa = _kappa(K, C, theta, dt, [])
    tev = _tev(mesh, g)
    run = thermo.OneStepTheta(tev, CAPA, dt, theta, np.zeros(nt), [], T_init, lin_rtol=rtol)
    H0 = run.heat_content()
    sumC = float(np.abs(C).sum())
    for k in range(1, nstep + 1):
        run.step()
        want = Tbar + A0 * gfac ** k * mode
        tmax = float(np.abs(want).max())
        bound = k * kappa * rtol * tmax + 64 * EPS * tmax
        err = float(np.abs(run.T.cpu().numpy().astype(LD) - want).max())
        dH = abs(run.heat_content() - H0)
        print(f"OST cosine theta={theta} step={k} err={err:.3e} bound={bound:.3e} dH={dH:.3e} "
              f"kappa={kappa:.3e} iters={run.history[-1]['iterations']}")
        assert err <= bound
        assert dH <= sumC * bound
    assert len(run.history) == nstep and all(r["iterations"] >= 1 for r in run.history)
    tev.close()


def test_conduction_with_dirichlet_ends():
    _dev()
    thermo = importlib.import_module("4c_amd.thermo")
    amg = importlib.import_module("4c_amd.amg")
    theta, dt, nstep, rtol = 2.0 / 3.0, 0.02, 3, 1e-12
    mesh = fcg.BoxMesh(fcg.HEX27, (2, 2, 2), jitter=0.1)
    flat = fcg.BoxMesh(fcg.HEX27, (2, 2, 2))
    g = fcg.TsiGraph(mesh)
    nt = g.n_rows_t
    x0 = np.asarray(flat.node_x)[:, 0]
    ends = np.flatnonzero((x0 == x0.min()) | (x0 == x0.max()))
    dbc = np.sort(np.asarray(g.node_dof_row_t)[ends]).astype(np.int32)
    assert 0 < len(dbc) < nt
    X = np.asarray(mesh.node_x)
    T_init, fext = np.zeros(nt), np.zeros(nt)
    T_init[g.node_dof_col_t] = 293.0 + 40.0 * X[:, 0] + 5.0 * np.sin(3 * X[:, 1])
    fext[g.node_dof_row_t] = 2.0 * (1 + X[:, 2])
    K, C = _dense_tt(mesh, g)
    ref = th.ost_dense(K, C, theta, dt, T_init, fext, dbc, nstep)
    kappa = _kappa(K, C, theta, dt, dbc)
    got = {}
    for with_amg in (True, False):
        tev = _tev(mesh, g)
        at = amg.ScalarAMG(tev, dbc, coarse_max=8) if with_amg else None
        run = thermo.OneStepTheta(tev, CAPA, dt, theta, fext, dbc, T_init, amg_t=at, lin_rtol=rtol)
        for k in range(1, nstep + 1):
            run.step()
            tmax = float(np.abs(ref[k]).max())
            bound = k * kappa * rtol * tmax + 64 * EPS * tmax
            Td = run.T.cpu().numpy()
            err = float(np.abs(Td.astype(LD) - ref[k]).max())
            print(f"OST dirichlet amg={with_amg} step={k} err={err:.3e} bound={bound:.3e} kappa={kappa:.3e}")
            assert err <= bound
            assert np.array_equal(Td[dbc], T_init[dbc])   # prescribed temperatures keep their values
        got[with_amg] = Td
        if at is not None:
            at.close()
        tev.close()
    assert float(np.abs(got[True] - got[False]).max()) <= 2 * bound


# ------------------------------------------------------------------------------ transient TSI
TSI_MESHES = {"h8_322": ((3, 2, 2), fcg.PATH_AUTO, (False,)),
              "h8_653": ((6, 5, 3), fcg.PATH_STRUCTURED, (True, False))}
TSI_DT, TSI_STEPS, TSI_RTOL, TSI_TOL_INC = 0.1, 2, 1e-12, 1e-9


@functools.lru_cache(maxsize=None)
def _tsi_problem(name):
    iv = TSI_MESHES[name][0]
    mesh = fcg.BoxMesh(fcg.HEX8, iv, jitter=0.1, seed=4)
    flat = fcg.BoxMesh(fcg.HEX8, iv)
    g = fcg.TsiGraph(mesh)
    x0 = np.asarray(flat.node_x)[:, 0]
    lo, hi = np.flatnonzero(x0 == x0.min()), np.flatnonzero(x0 == x0.max())
    dbc_t = np.sort(np.asarray(g.node_dof_row_t)[lo]).astype(np.int32)
    dbc_s = np.sort((np.asarray(mesh.node_dof_row)[lo][:, None] + np.arange(3)).ravel()).astype(np.int32)
    fs, ft = np.zeros(mesh.n_rows), np.zeros(g.n_rows_t)
    fs[np.asarray(mesh.node_dof_row)[hi]] = 0.4          # a pull along x on the far face
    fs[np.asarray(mesh.node_dof_row)[hi] + 1] = -0.1
    ft[np.asarray(g.node_dof_row_t)[hi]] = 30.0          # a heat flux into the far face
    T_init = np.zeros(g.n_rows_t)
    T_init[g.node_dof_col_t] = T0 + 10.0 * np.asarray(mesh.node_x)[:, 0]
    return dict(mesh=mesh, g=g, dbc_s=dbc_s, dbc_t=dbc_t, fs=fs, ft=ft, T_init=T_init)


@functools.lru_cache(maxsize=None)
def _tsi_reference(name, theta):
    P = _tsi_problem(name)
    d, T, iters, A = th.tsi_ost_dense(P["mesh"], P["g"], E, NU, ALPHA, T0, COND, CAPA, theta, TSI_DT, P["fs"],
                                      P["ft"], P["dbc_s"], P["dbc_t"], P["T_init"], TSI_STEPS,
                                      tol_inc=TSI_TOL_INC)
    return d, T, iters, float(np.linalg.cond(A.astype(np.float64)))


TSI_CASES = [(n, f, t) for n, (_, _, fs) in TSI_MESHES.items() for f in fs for t in (0.5, 1.0)]


@pytest.mark.parametrize("name,fused,theta", TSI_CASES)
def test_transient_tsi(name, fused, theta):
    _dev()
    tsi = importlib.import_module("4c_amd.tsi")
    P = _tsi_problem(name)
    mesh, g = P["mesh"], P["g"]
    d_ref, T_ref, iters, kappa = _tsi_reference(name, theta)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=TSI_MESHES[name][1])
    tev = _tev(mesh, g)
    run = tsi.TsiMonolithic(ev, tev, TSI_DT, P["fs"], P["ft"], P["dbc_s"], P["dbc_t"], T_init=P["T_init"],
                            fused=fused, tol_inc=TSI_TOL_INC, lin_rtol=TSI_RTOL, thermal="ost", capa=CAPA,
                            theta=theta)
    d, T = run.run(TSI_STEPS)
    assert run.fused is fused
    x = np.concatenate([d.cpu().numpy(), T.cpu().numpy()]).astype(LD)
    x_ref = np.concatenate([d_ref, T_ref])
    xmax = float(np.abs(x_ref).max())
    bound = TSI_STEPS * kappa * TSI_RTOL * xmax + 64 * EPS * xmax
    err = float(np.abs(x - x_ref).max())
    err_d = float(np.abs(x - x_ref)[:len(d_ref)].max())
    got_iters = [r["iterations"] for r in run.history]
    print(f"OST tsi {name} fused={fused} theta={theta} err={err:.3e} err_d={err_d:.3e} "
          f"max|d|={float(np.abs(d_ref).max()):.3e} bound={bound:.3e} kappa={kappa:.3e} "
          f"newton={got_iters} host={iters}")
    tev.close()
    ev.close()
    assert err <= bound
    assert got_iters == iters


@pytest.mark.parametrize("name", list(TSI_MESHES))
def test_statics_is_untouched(name):
    _dev()
    tsi = importlib.import_module("4c_amd.tsi")
    P = _tsi_problem(name)
    mesh, g = P["mesh"], P["g"]
    out = []
    for kw in ({}, dict(thermal="statics"), dict(thermal="statics", capa=CAPA, theta=0.5)):
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=TSI_MESHES[name][1])
        tev = _tev(mesh, g)
        run = tsi.TsiMonolithic(ev, tev, TSI_DT, P["fs"], P["ft"], P["dbc_s"], P["dbc_t"], T_init=P["T_init"], **kw)
        d, T = run.run(1)
        out.append((d.clone(), T.clone(), [r["gmres_iterations"] for r in run.history]))
        tev.close()
        ev.close()
    for o in out[1:]:
        assert torch.equal(o[0], out[0][0]) and torch.equal(o[1], out[0][1]) and o[2] == out[0][2]
