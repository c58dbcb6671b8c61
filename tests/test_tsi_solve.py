"""GPU tests of the monolithic TSI operator and solve (4c_amd/csrc/fcg_tsi_solve.hip,
4c_amd/tsi.py): fcg_tsi_block_apply, fcg_tsi_dirichlet_apply, fcg_tsi_gmres_solve and the resident
Newton loop tsi.TsiMonolithic on the reference's known-answer inputs.

Bounds as in tests/test_gmres.py: a product of one row against the extended-precision reference
within (terms + 2) 2^-53 |K||x|; a solve's residual within rtol |b| + sigma with sigma the
rounding of the FP64 product, its error within cond_2(A) rtol |x*|."""

import importlib
import json
import os
import types

import numpy as np
import pytest

import krylov_ref as kr
import solver_ref as sr
from solver_ref import LD, U
from tsi_driver import TsiProblem

torch = pytest.importorskip("torch")
fcg = importlib.import_module("4c_amd").fcg
tsi = importlib.import_module("4c_amd.tsi")
gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E, NU, ALPHA, T0, COND, DT = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.05
FCG_ERR_ARG = 3

MESHES = {
    "h8_322": (fcg.HEX8, (3, 2, 2), 0.1),
    "h8_333": (fcg.HEX8, (3, 3, 3), 0.1),  # an interior node with 27 neighbours
    "h27_221": (fcg.HEX27, (2, 2, 1), 0.02),
}
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t if dtype is None else t.to(dtype)


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


def _case(name):
    _dev()
    if name not in _cache:
        ct, iv, jitter = MESHES[name]
        mesh = fcg.BoxMesh(ct, iv, jitter=jitter, seed=4)
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
        tev = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND)
        face = kr.x0_face(ct, iv)
        rows_t = np.sort(np.asarray(mesh.node_dof_row)[face] // 3).astype(np.int32)
        rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
        _cache[name] = (mesh, ev, tev, rows_s, rows_t)
    return _cache[name]


def _blocks_graphs(mesh, g):
    return {"Kss": (mesh.rowptr, mesh.col_lid), "Kst": (g.rowptr_st, g.col_st),
            "Kts": (g.rowptr_ts, g.col_ts), "Ktt": (g.rowptr_tt, g.col_tt)}


def _stacked_ld(mesh, g, v, xs, xt):
    """([y_S; y_T], [|K||x|], terms per row) of the block operator in extended precision."""
    gr = _blocks_graphs(mesh, g)
    out = {}
    for k, x in (("Kss", xs), ("Kst", xt), ("Kts", xs), ("Ktt", xt)):
        out[k] = sr.csr_matvec_ld(gr[k][0], gr[k][1], v[k], x)
    y = np.concatenate([out["Kss"][0] + out["Kst"][0], out["Kts"][0] + out["Ktt"][0]])
    ay = np.concatenate([out["Kss"][1] + out["Kst"][1], out["Kts"][1] + out["Ktt"][1]])
    terms = np.concatenate([np.diff(gr["Kss"][0]) + np.diff(gr["Kst"][0]),
                            np.diff(gr["Kts"][0]) + np.diff(gr["Ktt"][0])])
    return y, ay, terms


# ------------------------------------------------------------------------------ 1. block apply
@gpu
@pytest.mark.parametrize("name", list(MESHES))
def test_block_apply_componentwise(name):
    mesh, ev, tev, _, _ = _case(name)
    g = tev.graph
    rng = np.random.default_rng(21)
    v = {"Kss": rng.standard_normal(mesh.nnz), "Kst": rng.standard_normal(g.nnz_st),
         "Kts": rng.standard_normal(g.nnz_ts), "Ktt": rng.standard_normal(g.nnz_tt)}
    xs, xt = rng.standard_normal(mesh.n_rows), rng.standard_normal(g.n_rows_t)
    dv = {k: _t(a) for k, a in v.items()}
    ys, yt = _nan(mesh.n_rows), _nan(g.n_rows_t)
    tev.block_apply(ev, dv["Kss"], dv["Kst"], dv["Kts"], dv["Ktt"], _t(xs), _t(xt), ys, yt)
    ys2, yt2 = _nan(mesh.n_rows), _nan(g.n_rows_t)
    tev.block_apply(ev, dv["Kss"], dv["Kst"], dv["Kts"], dv["Ktt"], _t(xs), _t(xt), ys2, yt2)
    torch.cuda.synchronize()
    assert torch.equal(ys, ys2) and torch.equal(yt, yt2)
    y = np.concatenate([ys.cpu().numpy(), yt.cpu().numpy()])
    yr, ay, terms = _stacked_ld(mesh, g, v, xs, xt)
    err = np.abs(y.astype(LD) - yr)
    bound = (terms + 2) * LD(U) * ay
    print(f"block apply {name}: worst error / bound = {float((err / bound).max()):.3f}, "
          f"longest row {int(terms.max())} terms")
    assert np.all(np.isfinite(y)) and np.all(err <= bound)


# -------------------------------------------------------------------------- 2. Dirichlet apply
@gpu
@pytest.mark.parametrize("name", ["h8_322", "h27_221"])
def test_dirichlet_apply_exact(name):
    mesh, ev, tev, rows_s, rows_t = _case(name)
    g = tev.graph
    rng = np.random.default_rng(22)
    v = {"Kst": rng.standard_normal(g.nnz_st), "Kts": rng.standard_normal(g.nnz_ts),
         "Ktt": rng.standard_normal(g.nnz_tt), "rhs": rng.standard_normal(g.n_rows_t)}
    d = {k: _t(a) for k, a in v.items()}
    tev.dirichlet_apply(_t(rows_s), _t(rows_t), d["Kst"], d["Kts"], d["Ktt"], d["rhs"])
    got = {k: a.cpu().numpy() for k, a in d.items()}
    ref = {k: a.copy() for k, a in v.items()}
    for r in rows_s:
        ref["Kst"][g.rowptr_st[r]:g.rowptr_st[r + 1]] = 0.0
    for t in rows_t:
        ref["Kts"][g.rowptr_ts[t]:g.rowptr_ts[t + 1]] = 0.0
        sl = slice(g.rowptr_tt[t], g.rowptr_tt[t + 1])
        ref["Ktt"][sl] = (g.col_tt[sl] == t).astype(np.float64)
        ref["rhs"][t] = 0.0
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k  # bitwise: named rows exact, the rest untouched
    # NULL pointers, either list alone
    tev.dirichlet_apply(_t(rows_s), None, None, None, None, None)
    tev.dirichlet_apply(None, _t(rows_t), None, None, None, None)
    k2 = _t(v["Ktt"])
    tev.dirichlet_apply(None, _t(rows_t), Ktt=k2)
    assert np.array_equal(k2.cpu().numpy(), ref["Ktt"])
    for bad_s, bad_t in ((np.array([mesh.n_rows], dtype=np.int32), None),
                         (None, np.array([-1], dtype=np.int32))):
        with pytest.raises(fcg.FcgError) as e:
            tev.dirichlet_apply(None if bad_s is None else _t(bad_s),
                                None if bad_t is None else _t(bad_t), d["Kst"], d["Kts"], d["Ktt"])
        assert e.value.code == FCG_ERR_ARG


# ----------------------------------------------------------------------- 3. solve against dense
def _device_system(name):
    """The four blocks at a random admissible state with v != 0, Dirichlet applied, on the device
    and the host, and a random admissible right-hand side."""
    mesh, ev, tev, rows_s, rows_t = _case(name)
    g = tev.graph
    rng = np.random.default_rng(23)
    u = 1e-3 * rng.standard_normal(mesh.n_cols)
    v = 1e-1 * rng.standard_normal(mesh.n_cols)
    T = T0 + 50.0 * rng.standard_normal(g.n_cols_t)
    z = lambda n: torch.zeros(int(n), dtype=torch.float64, device=_dev())
    fs, fT = z(mesh.n_rows), z(g.n_rows_t)
    d = {"Kss": z(mesh.nnz), "Kst": z(g.nnz_st), "Kts": z(g.nnz_ts), "Ktt": z(g.nnz_tt)}
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(u), fs, d["Kss"])
    tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, _t(v), _t(T), 1.0, 1.0 / DT, fs=fs, Kst=d["Kst"],
                        fT=fT, Ktt=d["Ktt"], Kts=d["Kts"])
    ev.dirichlet_apply(_t(rows_s), d["Kss"])
    tev.dirichlet_apply(_t(rows_s), _t(rows_t), d["Kst"], d["Kts"], d["Ktt"])
    bs, bt = rng.standard_normal(mesh.n_rows), rng.standard_normal(g.n_rows_t)
    bs[rows_s] = 0.0
    bt[rows_t] = 0.0
    return d, {k: a.cpu().numpy() for k, a in d.items()}, bs, bt


@gpu
@pytest.mark.parametrize("precond", ["diag", "bgs"])
@pytest.mark.parametrize("name", list(MESHES))
def test_solve_against_dense(name, precond):
    """restart 128, the library's largest: full GMRES on h8_322 (108 free unknowns); h8_333 (192)
    and h27_221 (240) restart."""
    mesh, ev, tev, rows_s, rows_t = _case(name)
    g = tev.graph
    d, h, bs, bt = _device_system(name)
    assert np.abs(h["Kts"]).max() > 0
    ns, nt = mesh.n_rows, g.n_rows_t
    xs, xt = _nan(ns), _nan(nt)
    rtol = 1e-10
    it, rel = tev.gmres_solve(ev, d["Kss"], d["Kst"], d["Kts"], d["Ktt"], _t(bs), _t(bt), xs, xt,
                              rtol=rtol, max_iter=3000, restart=128, precond=precond)
    xs, xt = xs.cpu().numpy(), xt.cpu().numpy()
    x, b = np.concatenate([xs, xt]), np.concatenate([bs, bt])
    assert np.all(np.isfinite(x)) and np.all(xs[rows_s] == 0.0) and np.all(xt[rows_t] == 0.0)
    y, ay, terms = _stacked_ld(mesh, g, h, xs, xt)
    r = b.astype(LD) - y
    res = float(np.sqrt((r * r).sum()))
    sigma = float(np.sqrt(((terms * LD(U) * ay) ** 2).sum()))
    nb = np.linalg.norm(b)
    gr = _blocks_graphs(mesh, g)
    A = np.block([[kr.csr_to_dense(*gr["Kss"], h["Kss"]), kr.csr_to_dense(*gr["Kst"], h["Kst"], nt)],
                  [kr.csr_to_dense(*gr["Kts"], h["Kts"], ns), kr.csr_to_dense(*gr["Ktt"], h["Ktt"])]])
    xd = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    err = np.linalg.norm(x - xd)
    print(f"tsi gmres {name} {precond}: {it} steps, rel {rel:.3e}, independent {res / nb:.3e}, "
          f"err/|x| {err / np.linalg.norm(xd):.2e}, cond {cond:.2e}")
    assert rel <= rtol and res <= rtol * nb + sigma, (rel, res / nb, sigma / nb)
    assert err <= cond * rtol * np.linalg.norm(xd), (err, cond)


# --------------------------------------------------------------------------------- 4. refusals
def _permuted_graph(mesh, seed=1):
    """The TSI graphs of `mesh` with the thermo DOFs numbered by a random permutation of the
    nodes: valid for fcg_tsi_create and its evaluates, not node-consistent."""
    g = fcg.TsiGraph(mesh)
    p = np.random.default_rng(seed).permutation(g.n_rows_t).astype(np.int32)
    inv = np.argsort(p)
    q = types.SimpleNamespace(n_rows_t=g.n_rows_t, n_cols_t=g.n_cols_t)
    q.node_dof_col_t = np.ascontiguousarray(p[g.node_dof_col_t], dtype=np.int32)
    q.node_dof_row_t = np.ascontiguousarray(p[g.node_dof_row_t], dtype=np.int32)
    q.rowptr_st = g.rowptr_st.copy()
    q.col_st = np.concatenate([np.sort(p[g.col_st[g.rowptr_st[r]:g.rowptr_st[r + 1]]])
                               for r in range(mesh.n_rows)]).astype(np.int32)
    tt = [np.sort(p[g.col_tt[g.rowptr_tt[t]:g.rowptr_tt[t + 1]]]) for t in inv]
    ts = [g.col_ts[g.rowptr_ts[t]:g.rowptr_ts[t + 1]] for t in inv]
    q.rowptr_tt = np.concatenate([[0], np.cumsum([len(c) for c in tt])]).astype(np.int64)
    q.rowptr_ts = np.concatenate([[0], np.cumsum([len(c) for c in ts])]).astype(np.int64)
    q.col_tt = np.concatenate(tt).astype(np.int32)
    q.col_ts = np.concatenate(ts).astype(np.int32)
    q.nnz_st, q.nnz_ts, q.nnz_tt = len(q.col_st), len(q.col_ts), len(q.col_tt)
    return q


def _all_three(ev, tev, mesh, g, dirichlet=True):
    """Every call of the section with well-formed buffers (the Dirichlet apply, which takes no
    structural context, on request); returns the error codes."""
    z = lambda n: torch.zeros(int(n), dtype=torch.float64, device=_dev())
    K = [z(mesh.nnz), z(g.nnz_st), z(g.nnz_ts), z(g.nnz_tt)]
    codes = []
    calls = [lambda: tev.block_apply(ev, *K, z(mesh.n_rows), z(g.n_rows_t), z(mesh.n_rows), z(g.n_rows_t)),
             lambda: tev.gmres_solve(ev, *K, z(mesh.n_rows), z(g.n_rows_t), z(mesh.n_rows), z(g.n_rows_t)),
             lambda: tev.dirichlet_apply(_t(np.zeros(1, dtype=np.int32)), None, K[1])]
    for call in calls[:3 if dirichlet else 2]:
        with pytest.raises(fcg.FcgError) as e:
            call()
        codes.append(e.value.code)
    return codes


@gpu
def test_refusals():
    mesh, ev, tev, _, _ = _case("h8_322")
    q = _permuted_graph(mesh)
    ptev = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND, graph=q)  # created, and evaluates
    assert _all_three(ev, ptev, mesh, q) == [FCG_ERR_ARG] * 3
    # a structural context of another mesh
    other = fcg.BoxMesh(fcg.HEX8, (3, 3, 2))
    oev = fcg.Evaluator(other, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    assert _all_three(oev, tev, mesh, tev.graph, dirichlet=False) == [FCG_ERR_ARG] * 2
    # a rank of a partition
    rank = fcg.BoxMesh(fcg.HEX8, (4, 2, 2), rank=0, nranks=2)
    rev = fcg.Evaluator(rank, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    rtev = fcg.TsiEvaluator(rank, E, NU, ALPHA, T0, COND)
    assert _all_three(rev, rtev, rank, rtev.graph) == [FCG_ERR_ARG] * 3
    # bad options, singular D_TT
    d, h, bs, bt = _device_system("h8_322")
    args = (ev, d["Kss"], d["Kst"], d["Kts"], d["Ktt"], _t(bs), _t(bt), _nan(len(bs)), _nan(len(bt)))
    for kw in ({"restart": 0}, {"restart": 129}, {"max_iter": -1}):
        with pytest.raises(fcg.FcgError) as e:
            tev.gmres_solve(*args, **kw)
        assert e.value.code == FCG_ERR_ARG
    with pytest.raises(fcg.FcgError) as e:
        tev.gmres_solve(ev, d["Kss"], d["Kst"], d["Kts"], torch.zeros_like(d["Ktt"]), *args[5:])
    assert e.value.code == 2


# ----------------------------------------------------------------------------- 5. known answers
_dense = {}


def _dense_answer(name):
    if name not in _dense:
        prob = TsiProblem(json.load(open(os.path.join(GOLD, name))))
        d, T = prob.solve()
        _dense[name] = (prob, d, T, sum(h["iterations"] for h in prob.history))
    return _dense[name]


@gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name,newton_total", [("tsi_heatflux_monolithic.json", 20),
                                               ("tsi_heatflux_flexoutsurf_monolithic.json", 25)])
def test_known_answers_resident(name, newton_total, fused):
    _dev()
    prob, d_ref, T_ref, n_ref = _dense_answer(name)
    assert n_ref == newton_total
    dis = fcg.Discretization.from_elements(prob.celltype, prob.elements, prob.X, lattice=fused)
    ev = fcg.Evaluator(dis, kinematics=fcg.LINEAR, youngs=prob.E, poisson=prob.nu,
                       path=fcg.PATH_STRUCTURED if fused else fcg.PATH_AUTO)
    tev = fcg.TsiEvaluator(dis, prob.E, prob.nu, prob.alpha, prob.T0, prob.conduct)
    run = tsi.TsiMonolithic(ev, tev, prob.dt, prob.fext_s, prob.fext_t, prob.dbc_s, prob.dbc_t,
                            T_init=prob.T_init, fused=fused)
    d, T = run.run(prob.nstep)
    assert run.fused is fused
    d, T = d.cpu().numpy(), T.cpu().numpy()
    for r in prob.fx["results"]:
        got = prob.result(d, T, r)
        assert abs(got - r["value"]) <= r["tol"], (r, got)
    ed = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    eT = np.linalg.norm(T - T_ref) / np.linalg.norm(T_ref)
    its = [n for h in run.history for n in h["gmres_iterations"]]
    print(f"{name} fused={fused}: |dd|/|d| {ed:.2e}, |dT|/|T| {eT:.2e}, GMRES steps per solve "
          f"max {max(its)}, Newton {sum(h['iterations'] for h in run.history)}")
    assert ed <= 1e-9 and eT <= 1e-10
    assert sum(h["iterations"] for h in run.history) == newton_total
    assert max(its) <= run.lin_max_iter
