"""thermo.OneStepTheta and tsi.TsiMonolithic with heat convection on surfaces (fcg.TsiSurface), on the
device against dense longdouble host solutions (thermo_ref.py, thermo_bc_ref.py).

The bound is the one test_tsi_ost.py derives: with kappa the condition number of the effective matrix
(convection included, Dirichlet rows applied; for TSI the stacked effective matrix), a solve stopped at
the relative residual lin_rtol has a forward error of at most kappa lin_rtol, and after n steps

    max |x_dev - x_ref| <= n kappa lin_rtol max|x| + 64 eps max|x|.

The rod.  tsi.TsiMonolithic(thermal="statics") on the rod of test_thermo_bc_ref_cpu.py: T = T_0 on the
end at 0, convection (h, T_inf) on the end at L, zero structural load.  So that the bound's kappa is
the one of the thermal system alone (the dense system of thermo_bc_ref.rod_dense, as asked), the
structure is held at every DOF and the thermal expansion coefficient of this context is 0: the blocks
K_ST and K_TS vanish, K_SS is the identity, the stacked residual is the thermal one, and the rate of
the volumetric strain, which would heat the rod while it expands, stays 0.  The closed form and the
figures of its dense solution are in test_thermo_bc_ref_cpu.py; here the dense solution is asserted
against it on the CPU before the device runs.

The heat balance.  Without Dirichlet rows and with theta = 1 a converged step satisfies
C (T_{n+1} - T_n)/dt + K T_{n+1} + A T_{n+1} - g - q = 0; K is symmetric with K 1 = 0, so the sum of the
rows, 1^T C (T_{n+1} - T_n)/dt + 1^T (A T_{n+1} - g) - 1^T q, vanishes: the heat stored is the heat that
crosses the surface.  It is evaluated in longdouble from the device temperatures and the reference's
C, A, g and q.
"""

import functools
import importlib

import numpy as np
import pytest

import thermo_bc_ref as bc
import thermo_ref as th
from element_ref import EXTENDED, LD
from thermo_ref import MAT, mesh_of

pkg = importlib.import_module("4c_amd")
fcg = pkg.fcg
torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not EXTENDED, reason="np.longdouble has no 64-bit significand here")]

CAPA = 3.5
E, NU, ALPHA, T0, COND = MAT["youngs"], MAT["poisson"], MAT["thexpans"], MAT["inittemp"], MAT["conduct"]
EPS = float(np.finfo(np.float64).eps)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _tev(mesh, g=None, alpha=ALPHA):
    return fcg.TsiEvaluator(mesh, E, NU, alpha, T0, COND, graph=g)


# ------------------------------------------------------------------------------ the rod
@pytest.mark.parametrize("celltype,iv", [(fcg.HEX8, (2, 2, 6)), (fcg.HEX27, (1, 1, 3))])
def test_rod_known_answer(celltype, iv):
    tsi = importlib.import_module("4c_amd.tsi")
    rtol = 1e-12
    P = bc.rod_problem(celltype, iv, COND)
    mesh, g, want = P["mesh"], P["g"], P["want"]
    T_ref, kappa = bc.rod_dense(mesh, g, COND, P["end"], P["h"], P["T_inf"], P["dbc"], P["T0"])
    tmax = float(np.abs(want).max())
    assert float(np.abs(T_ref - want).max()) <= 1e-15 * tmax     # on the CPU, before the device run
    _dev()
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    tev = _tev(mesh, g, alpha=0.0)
    surf = fcg.TsiSurface(tev, P["end"]).set(coeff=P["h"], surtemp=P["T_inf"])
    ns, nt = mesh.n_rows, g.n_rows_t
    run = tsi.TsiMonolithic(ev, tev, 1.0, np.zeros(ns), np.zeros(nt), np.arange(ns, dtype=np.int32), P["dbc"],
                            T_init=np.full(nt, P["T0"]), tol_inc=1e-9, lin_rtol=rtol, thermal="statics",
                            convection=surf)
    d, T = run.run(1)
    Td = T.cpu().numpy()
    err = float(np.abs(Td.astype(LD) - want).max())
    bound = kappa * rtol * tmax + 64 * EPS * tmax
    print(f"ROD {iv} err={err:.3e} bound={bound:.3e} kappa={kappa:.3e} T_L={float(want.max()):.6f} "
          f"newton={run.history[-1]['iterations']}")
    surf.close()
    tev.close()
    ev.close()
    assert not d.any()                                           # the structure is held
    assert np.array_equal(Td[P["dbc"]], np.full(len(P["dbc"]), P["T0"]))
    assert err <= bound


# ------------------------------------------------------------------------------ one-step-theta with convection
@functools.lru_cache(maxsize=None)
def _ost_problem(dirichlet=True):
    """h8 (3,3,3), jitter 0.1: convection on all six sides (two-valued coefficient, four-valued
    surrounding temperature), a flux on the side x = max, the side x = min prescribed."""
    mesh, g = mesh_of("h8")
    flat = fcg.BoxMesh(fcg.HEX8, (3, 3, 3))
    faces, _ = fcg.boundary_faces(mesh)
    x0 = np.asarray(flat.node_x)[:, 0]
    i = np.arange(len(faces))
    coeff = np.where(i % 3 == 0, 12.5, 7.25 * 12.5)
    surtemp = 300.0 + 5.0 * (i % 4)
    flux = np.where((x0[faces] == x0.max()).all(axis=1), 30.0, 0.0)
    assert (flux != 0).sum() == 9
    dbc = np.sort(np.asarray(g.node_dof_row_t)[np.flatnonzero(x0 == x0.min())]).astype(np.int32)
    if not dirichlet:
        dbc = dbc[:0]
    nt = g.n_rows_t
    X = np.asarray(mesh.node_x)
    T_init = np.zeros(nt)
    T_init[g.node_dof_col_t] = 293.0 + 40.0 * X[:, 0] + 5.0 * np.sin(3 * X[:, 1])
    K = th.dense(g.rowptr_tt, g.col_tt, th.conduction(mesh, g, COND), nt)
    C = th.dense(g.rowptr_tt, g.col_tt, th.capacity(mesh, g, CAPA)[0], nt)
    A, gv, qv = bc.dense_operator(mesh, g, faces, coeff, surtemp, flux)
    return dict(mesh=mesh, g=g, faces=faces, coeff=coeff, surtemp=surtemp, flux=flux, dbc=dbc, T_init=T_init,
                K=K, C=C, A=A, gv=gv, qv=qv)


def _kappa(S, dbc):
    S = S.astype(np.float64)
    th.apply_dirichlet(S, np.zeros(len(S)), np.asarray(dbc, dtype=np.int64))
    return float(np.linalg.cond(S))


def _ost_run(P, theta, dt, rtol, with_amg=False, surtemp_funct=None, convection=True):
    thermo = importlib.import_module("4c_amd.thermo")
    amg = importlib.import_module("4c_amd.amg")
    tev = _tev(P["mesh"], P["g"])
    surf = fcg.TsiSurface(tev, P["faces"]).set(P["coeff"], P["surtemp"], P["flux"])
    fext = torch.zeros(P["g"].n_rows_t, dtype=torch.float64, device=_dev())
    surf.flux(fext)                                              # the heat flux load, on the device
    at = amg.ScalarAMG(tev, P["dbc"], coarse_max=8) if with_amg else None
    conv = (surf, None, surtemp_funct) if surtemp_funct is not None else surf
    run = thermo.OneStepTheta(tev, CAPA, dt, theta, fext, P["dbc"], P["T_init"], amg_t=at, lin_rtol=rtol,
                              convection=conv if convection else None)
    return run, (tev, surf, at)


def _close(objs):
    tev, surf, at = objs
    if at is not None:
        at.close()
    surf.close()
    tev.close()


@pytest.mark.parametrize("theta", [2.0 / 3.0, 1.0])
def test_one_step_theta_with_convection(theta):
    _dev()
    dt, nstep, rtol = 0.02, 3, 1e-12
    P = _ost_problem()
    ref = th.ost_dense(P["K"] + P["A"], P["C"], theta, dt, P["T_init"], P["gv"] + P["qv"], P["dbc"], nstep)
    plain = th.ost_dense(P["K"], P["C"], theta, dt, P["T_init"], P["qv"], P["dbc"], nstep)
    kappa = _kappa(P["C"] / LD(dt) + LD(theta) * (P["K"] + P["A"]), P["dbc"])
    got = {}
    for with_amg in (False, True):
        run, objs = _ost_run(P, theta, dt, rtol, with_amg)
        for k in range(1, nstep + 1):
            run.step()
            tmax = float(np.abs(ref[k]).max())
            bound = k * kappa * rtol * tmax + 64 * EPS * tmax
            Td = run.T.cpu().numpy()
            err = float(np.abs(Td.astype(LD) - ref[k]).max())
            moved = float(np.abs(ref[k] - plain[k]).max())
            print(f"OST convection theta={theta:.3f} amg={with_amg} step={k} err={err:.3e} bound={bound:.3e} "
                  f"kappa={kappa:.3e} convection moves T by {moved:.3e}")
            assert err <= bound
            assert moved > 1e3 * bound                           # the condition is not lost in the bound
            assert np.array_equal(Td[P["dbc"]], P["T_init"][P["dbc"]])
        got[with_amg] = Td
        _close(objs)
    assert float(np.abs(got[True] - got[False]).max()) <= 2 * bound


def test_surrounding_temperature_changes_between_steps():
    """s_t(t) = 1 + 10 t scales the surrounding temperatures: f_ext(t) = s_t(t) g + q in the reference.
    With theta = 2/3 a third of every step's residual is the old f_int,n, which holds the old convection
    with the old scale: a driver that formed it with the new one, or without the convection, misses."""
    _dev()
    theta, dt, nstep, rtol = 2.0 / 3.0, 0.02, 3, 1e-12
    P = _ost_problem()
    s_t = lambda t: 1.0 + 10.0 * t
    ref = th.ost_dense(P["K"] + P["A"], P["C"], theta, dt, P["T_init"],
                       lambda t: LD(s_t(t)) * P["gv"] + P["qv"], P["dbc"], nstep)
    const = th.ost_dense(P["K"] + P["A"], P["C"], theta, dt, P["T_init"], P["gv"] + P["qv"], P["dbc"], nstep)
    kappa = _kappa(P["C"] / LD(dt) + LD(theta) * (P["K"] + P["A"]), P["dbc"])
    run, objs = _ost_run(P, theta, dt, rtol, surtemp_funct=s_t)
    for k in range(1, nstep + 1):
        run.step()
        tmax = float(np.abs(ref[k]).max())
        bound = k * kappa * rtol * tmax + 64 * EPS * tmax
        err = float(np.abs(run.T.cpu().numpy().astype(LD) - ref[k]).max())
        moved = float(np.abs(ref[k] - const[k]).max())
        print(f"OST surtemp(t) step={k} err={err:.3e} bound={bound:.3e} the time function moves T by {moved:.3e}")
        assert err <= bound
        assert moved > 1e3 * bound
    _close(objs)


def test_heat_balance():
    _dev()
    dt, nstep, rtol = 0.02, 3, 1e-12
    P = _ost_problem(dirichlet=False)
    assert len(P["dbc"]) == 0
    C, A, gv, qv = P["C"], P["A"], P["gv"], P["qv"]
    kappa = _kappa(C / LD(dt) + P["K"] + A, [])
    sumC = float(C.sum())
    run, objs = _ost_run(P, 1.0, dt, rtol)
    Tn = run.T.cpu().numpy().astype(LD)
    for k in range(1, nstep + 1):
        run.step()
        T1 = run.T.cpu().numpy().astype(LD)
        tmax = float(np.abs(T1).max())
        bound = k * kappa * rtol * tmax + 64 * EPS * tmax
        stored = (C @ (T1 - Tn)).sum() / LD(dt)
        crossing = (A @ T1 - gv).sum() - qv.sum()
        bal = abs(float(stored + crossing))
        print(f"OST balance step={k} stored={float(stored):.6e} crossing={float(crossing):.6e} sum={bal:.3e} "
              f"allowed={sumC * bound:.3e} kappa={kappa:.3e}")
        assert bal <= sumC * bound
        assert abs(float(stored)) > 1e3 * sumC * bound           # heat does cross the surface
        Tn = T1
    _close(objs)


# ------------------------------------------------------------------------------ transient TSI with convection
TSI_IV, TSI_DT, TSI_STEPS, TSI_RTOL, TSI_TOL_INC = (6, 5, 3), 0.1, 2, 1e-12, 1e-9


@functools.lru_cache(maxsize=None)
def _tsi_problem():
    """The h8_653 case of test_tsi_ost.py (clamped and prescribed at x = min, a pull and a heat flux on
    x = max) with a convection condition on the side y = min."""
    mesh = fcg.BoxMesh(fcg.HEX8, TSI_IV, jitter=0.1, seed=4)
    flat = fcg.BoxMesh(fcg.HEX8, TSI_IV)
    g = fcg.TsiGraph(mesh)
    x0, y0 = np.asarray(flat.node_x)[:, 0], np.asarray(flat.node_x)[:, 1]
    lo, hi = np.flatnonzero(x0 == x0.min()), np.flatnonzero(x0 == x0.max())
    dbc_t = np.sort(np.asarray(g.node_dof_row_t)[lo]).astype(np.int32)
    dbc_s = np.sort((np.asarray(mesh.node_dof_row)[lo][:, None] + np.arange(3)).ravel()).astype(np.int32)
    fs, ft = np.zeros(mesh.n_rows), np.zeros(g.n_rows_t)
    fs[np.asarray(mesh.node_dof_row)[hi]] = 0.4
    fs[np.asarray(mesh.node_dof_row)[hi] + 1] = -0.1
    ft[np.asarray(g.node_dof_row_t)[hi]] = 30.0
    T_init = np.zeros(g.n_rows_t)
    T_init[g.node_dof_col_t] = T0 + 10.0 * np.asarray(mesh.node_x)[:, 0]
    faces, _ = fcg.boundary_faces(mesh)
    side = faces[(y0[faces] == y0.min()).all(axis=1)]
    assert len(side) == TSI_IV[0] * TSI_IV[2]
    return dict(mesh=mesh, g=g, dbc_s=dbc_s, dbc_t=dbc_t, fs=fs, ft=ft, T_init=T_init, side=side, h=25.0,
                T_inf=T0 + 40.0)


@functools.lru_cache(maxsize=None)
def _tsi_reference(theta):
    P = _tsi_problem()
    Ac, gc, _ = bc.dense_operator(P["mesh"], P["g"], P["side"], P["h"], P["T_inf"], 0.0)
    d, T, iters, S = bc.tsi_ost_conv_dense(P["mesh"], P["g"], E, NU, ALPHA, T0, COND, CAPA, theta, TSI_DT, P["fs"],
                                           P["ft"], P["dbc_s"], P["dbc_t"], P["T_init"], TSI_STEPS, Ac, gc,
                                           tol_inc=TSI_TOL_INC)
    _, T_plain, _, _ = th.tsi_ost_dense(P["mesh"], P["g"], E, NU, ALPHA, T0, COND, CAPA, theta, TSI_DT, P["fs"],
                                        P["ft"], P["dbc_s"], P["dbc_t"], P["T_init"], TSI_STEPS,
                                        tol_inc=TSI_TOL_INC)
    return d, T, iters, float(np.linalg.cond(S.astype(np.float64))), float(np.abs(T - T_plain).max())


@pytest.mark.parametrize("theta", [0.5, 1.0])
def test_transient_tsi_with_convection(theta):
    _dev()
    tsi = importlib.import_module("4c_amd.tsi")
    P = _tsi_problem()
    mesh, g = P["mesh"], P["g"]
    d_ref, T_ref, iters, kappa, moved = _tsi_reference(theta)
    x_ref = np.concatenate([d_ref, T_ref])
    xmax = float(np.abs(x_ref).max())
    bound = TSI_STEPS * kappa * TSI_RTOL * xmax + 64 * EPS * xmax
    assert moved > 1e3 * bound                                   # the condition is not lost in the bound
    got = {}
    for fused in (True, False):
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
        tev = _tev(mesh, g)
        surf = fcg.TsiSurface(tev, P["side"]).set(coeff=P["h"], surtemp=P["T_inf"])
        run = tsi.TsiMonolithic(ev, tev, TSI_DT, P["fs"], P["ft"], P["dbc_s"], P["dbc_t"], T_init=P["T_init"],
                                fused=fused, tol_inc=TSI_TOL_INC, lin_rtol=TSI_RTOL, thermal="ost", capa=CAPA,
                                theta=theta, convection=[surf])
        d, T = run.run(TSI_STEPS)
        assert run.fused is fused
        x = np.concatenate([d.cpu().numpy(), T.cpu().numpy()])
        err = float(np.abs(x.astype(LD) - x_ref).max())
        got_iters = [r["iterations"] for r in run.history]
        print(f"OST tsi convection fused={fused} theta={theta} err={err:.3e} bound={bound:.3e} kappa={kappa:.3e} "
              f"newton={got_iters} host={iters} convection moves T by {moved:.3e}")
        surf.close()
        tev.close()
        ev.close()
        assert err <= bound
        assert got_iters == iters
        got[fused] = x
    assert float(np.abs(got[True] - got[False]).max()) <= 2 * bound


# ------------------------------------------------------------------------------ no convection, no change
def test_no_convection_is_untouched():
    _dev()
    tsi = importlib.import_module("4c_amd.tsi")
    thermo = importlib.import_module("4c_amd.thermo")
    P = _ost_problem()
    out = []
    for conv in (None, []):
        tev = _tev(P["mesh"], P["g"])
        run = thermo.OneStepTheta(tev, CAPA, 0.02, 2.0 / 3.0, P["qv"].astype(np.float64), P["dbc"], P["T_init"],
                                  lin_rtol=1e-12, convection=conv)
        out.append((run.run(2).clone(), [r["gmres_iterations"] for r in run.history]))
        tev.close()
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    mesh, g = P["mesh"], P["g"]
    lo = P["dbc"]
    dbc_s = np.sort((3 * lo[:, None] + np.arange(3)).ravel()).astype(np.int32)   # node-consistent numbering
    fs = np.zeros(mesh.n_rows)
    fs[-3:] = 0.2
    out = []
    for conv in (None, []):
        for kw in (dict(thermal="statics"), dict(thermal="ost", capa=CAPA, theta=0.5)):
            ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
            tev = _tev(mesh, g)
            run = tsi.TsiMonolithic(ev, tev, 0.1, fs, P["qv"].astype(np.float64), dbc_s, lo, T_init=P["T_init"],
                                    tol_inc=1e-9, lin_rtol=1e-12, convection=conv, **kw)
            d, T = run.run(1)
            out.append((d.clone(), T.clone(), [r["gmres_iterations"] for r in run.history]))
            tev.close()
            ev.close()
    for a, b in ((out[0], out[2]), (out[1], out[3])):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
