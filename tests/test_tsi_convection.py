"""fcg_tsi_surface on the device -- the tables after set, the convection pass and the heat flux load --
against the extended-precision reference of thermo_bc_ref.py.

Criterion: the one of the regime tests (regimes_util.judge; the reason for its factor is in the
docstring of test_evaluate_regimes.py), with the float64 numpy restatements of thermo_bc_ref in the
oracle's place: with both measures e_n and e_c (element_ref.err_norm / err_comp against the scale sums
listed in thermo_bc_ref.py),

    e(device) <= 4 * max(e(restatement), e_A(restatement)),

e_A the restatement's error in the benign regime A on the same mesh.  Each case prints "REGIMES {json}".

Meshes and regimes: thermo_ref.MESHES x thermo_ref.REGIMES (test_tsi_capacity.py describes them).  On
the single-rank meshes the surface is the whole boundary (fcg.boundary_faces: 54 quad4 faces with
compact rows of 7 and 9 entries, 24 quad9 faces with rows of 9 to 25).  On h27_rank0 / h27_rank1 it is
the true boundary of the global (2,2,4) box: the faces of the single-rank build all of whose nodes are
column nodes of the rank, matched by their coordinates, which the two builds give bit for bit in all
four regimes (asserted), so no ranked case is left out.  Coefficient, surrounding temperature and flux
are two- and four-valued tables per face.
"""

import functools
import importlib

import numpy as np
import pytest

import regimes_util
import thermo_bc_ref as bc
from element_ref import EXTENDED
from regimes_util import _entry
from thermo_ref import MAT, MESHES, REGIMES, mesh_of

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not EXTENDED, reason="np.longdouble has no 64-bit significand here")]

COEFF = 12.5
S_C, S_T, S_Q = 0.75, 1.25, 0.6


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


def _tables(nf):
    i = np.arange(nf)
    return (np.where(i % 3 == 0, COEFF, 7.25 * COEFF), 300.0 + 5.0 * (i % 4), np.where(i % 2 == 0, 30.0, -4.0))


@functools.lru_cache(maxsize=None)
def _faces(name, regime="A"):
    mesh, g = mesh_of(name, regime)
    celltype, iv, rank, nranks, _ = MESHES[name]
    if nranks == 1:
        return fcg.boundary_faces(mesh)[0]
    p = dict(lower=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0), rotation=(0.0, 0.0, 0.0), edge=None)
    p.update(REGIMES[regime])
    if p["edge"] is not None:
        p["size"] = tuple(p["edge"] * n for n in iv)
    upper = tuple(lo + s for lo, s in zip(p["lower"], p["size"]))
    single = fcg.BoxMesh(celltype, iv, lower=p["lower"], upper=upper, rotation=p["rotation"], jitter=0.1)
    faces = bc.true_boundary_faces(mesh, single)
    assert faces is not None, "the ranked and the single-rank build differ in their coordinates"
    rows = np.asarray(g.node_dof_row_t)[faces]
    assert (rows >= 0).any() and (rows < 0).any()      # owned rows beside ghost columns
    return faces


@functools.lru_cache(maxsize=None)
def _problem(name, regime):
    mesh, g = mesh_of(name, regime)
    faces = _faces(name, regime)
    c, t, q = _tables(len(faces))
    assert len(set(c)) == 2 and len(set(q)) == 2
    r, r64 = bc.assemble(mesh, g, faces, c, t, q), bc.assemble_f64(mesh, g, faces, c, t, q)
    assert r["min_dA"] > 0
    return {k: _entry(r[k], r["S" + k], r64[k]) for k in ("A", "g", "q")}, r["layout"]


def _tev(name, regime="A"):
    _dev()
    mesh, g = mesh_of(name, regime)
    return fcg.TsiEvaluator(mesh, MAT["youngs"], MAT["poisson"], MAT["thexpans"], MAT["inittemp"],
                            MAT["conduct"], graph=g), mesh, g


def _surface(name, regime="A"):
    tev, mesh, g = _tev(name, regime)
    faces = _faces(name, regime)
    s = fcg.TsiSurface(tev, faces)
    s.set(*_tables(len(faces)))
    return tev, s, mesh, g


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name", list(MESHES))
def test_tables_against_longdouble(name, regime):
    tev, s, mesh, g = _surface(name, regime)
    prob, L = _problem(name, regime)
    a = s.tables()
    s.set(*_tables(s.n_faces))
    b = s.tables()
    info = s.info
    s.close()
    tev.close()
    assert _same(a, b)                                   # two sets, the same bits
    assert info["n_rows"] == L.nsr and info["n_entries"] == L.nse and info["device_bytes"] > 0
    for key, want in (("rows", L.s_row), ("ptr", L.s_ptr), ("col", L.s_col), ("pos", L.s_pos)):
        assert np.array_equal(a[key].cpu().numpy(), want), key
    regimes_util.judge(f"surface_tables/{name}/{regime}", prob, _problem(name, "A")[0],
                       {k: a[k].cpu().numpy() for k in ("A", "g", "q")}, {})


@pytest.mark.parametrize("name", ["h8", "h27_rank1"])
def test_equal_table_is_the_scalar_call(name):
    tev, s, mesh, g = _surface(name)
    s.set(COEFF, 310.0, -7.0)
    a = s.tables()
    n = s.n_faces
    s.set(np.full(n, COEFF), np.full(n, 310.0), np.full(n, -7.0))
    b = s.tables()
    s.set(0.0, 310.0, 0.0)                               # a coefficient of 0 is allowed
    z = s.tables()
    s.close()
    tev.close()
    assert _same(a, b)
    assert not torch.equal(a["A"], z["A"]) and not z["A"].any() and not z["g"].any() and not z["q"].any()


@functools.lru_cache(maxsize=None)
def _state(name, regime):
    """(v_col, T_col): the structure at rest and a smooth temperature field, tsi_ref.smooth_fields' shape
    in the coordinates of the mesh's bounding box (so that it varies alike in every regime)."""
    mesh, g = mesh_of(name, regime)
    X = np.asarray(mesh.node_x)
    U = (X - X.min(axis=0)) / np.ptp(X, axis=0)
    Tn = 293.0 + 50.0 * (np.sin(2 * np.pi * U[:, 0]) * np.cos(np.pi * U[:, 1]) + 0.2 * U[:, 2])
    T = np.zeros(g.n_cols_t)
    T[g.node_dof_col_t] = Tn
    assert float(np.ptp(Tn)) > 50.0                      # not a constant field
    return np.zeros(mesh.n_cols), T


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name", list(MESHES))
def test_convection_apply(name, regime):
    tev, s, mesh, g = _surface(name, regime)
    L = _problem(name, regime)[1]
    v, T = _state(name, regime)
    K0, f0 = _nan(g.nnz_tt), _nan(g.n_rows_t)
    tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, _t(v), _t(T), fT=f0, Ktt=K0)
    tab = s.tables()
    A, gv = tab["A"].cpu().numpy(), tab["g"].cpu().numpy()
    Tt = _t(T)
    K1, f1 = K0.clone(), f0.clone()
    s.convection(Tt, fT=f1, Ktt=K1, coeff_scale=S_C, surtemp_scale=S_T)
    K2, f2 = K0.clone(), f0.clone()
    s.convection(Tt, fT=f2, Ktt=K2, coeff_scale=S_C, surtemp_scale=S_T)
    assert torch.equal(K1, K2) and torch.equal(f1, f2)   # two runs, the same bits
    K3, f3 = K0.clone(), f0.clone()
    s.convection(Tt, fT=f3, coeff_scale=S_C, surtemp_scale=S_T)          # Ktt=None: the explicit variant
    s.convection(Tt, Ktt=K3, coeff_scale=S_C, surtemp_scale=S_T)         # fT=None: the tangent alone
    assert torch.equal(f3, f1) and torch.equal(K3, K1)
    # outside s_pos and outside the surface rows nothing is touched
    off_K = np.ones(g.nnz_tt, dtype=bool)
    off_K[L.s_pos] = False
    off_f = np.ones(g.n_rows_t, dtype=bool)
    off_f[L.s_row] = False
    K0n, f0n, K1n, f1n = (a.cpu().numpy() for a in (K0, f0, K1, f1))
    assert off_K.any() and np.array_equal(K1n[off_K], K0n[off_K])
    if off_f.any():
        assert np.array_equal(f1n[off_f], f0n[off_f])
    assert not np.array_equal(K1n[L.s_pos], K0n[L.s_pos]) and not np.array_equal(f1n[L.s_row], f0n[L.s_row])

    def entry():
        r = bc.apply(L, A, gv, S_C, S_T, K0n, f0n, T)
        K64, f64 = bc.apply_f64(L, A, gv, S_C, S_T, K0n, f0n, T)
        return {"K": _entry(r["K"], r["SK"], K64), "f": _entry(r["f"], r["Sf"], f64)}

    prob = entry()
    s.close()
    tev.close()
    regimes_util.judge(f"convection/{name}/{regime}", prob, _anchor_apply(name) if regime != "A" else prob,
                       {"K": K1n, "f": f1n}, {})


@functools.lru_cache(maxsize=None)
def _anchor_apply(name):
    """Regime A's entries of the pass on the same mesh: the restatement's errors there."""
    tev, s, mesh, g = _surface(name, "A")
    L = _problem(name, "A")[1]
    v, T = _state(name, "A")
    K0, f0 = _nan(g.nnz_tt), _nan(g.n_rows_t)
    tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, _t(v), _t(T), fT=f0, Ktt=K0)
    tab = s.tables()
    A, gv, qv = (tab[k].cpu().numpy() for k in ("A", "g", "q"))
    K0n, f0n = K0.cpu().numpy(), f0.cpu().numpy()
    s.close()
    tev.close()
    r = bc.apply(L, A, gv, S_C, S_T, K0n, f0n, T)
    K64, f64 = bc.apply_f64(L, A, gv, S_C, S_T, K0n, f0n, T)
    fq, Sq = bc.flux_apply(L, qv, S_Q, f0n)
    return {"K": _entry(r["K"], r["SK"], K64), "f": _entry(r["f"], r["Sf"], f64),
            "flux": _entry(fq, Sq, bc.flux_apply_f64(L, qv, S_Q, f0n))}


@pytest.mark.parametrize("name", list(MESHES))
def test_flux(name):
    tev, s, mesh, g = _surface(name)
    L = _problem(name, "A")[1]
    v, T = _state(name, "A")
    f0 = _nan(g.n_rows_t)
    tev.evaluate_device(fcg.TSI_THERMO_FINTCOND, fcg.OVERWRITE, _t(v), _t(T), fT=f0, Ktt=_nan(g.nnz_tt))
    qv = s.tables()["q"].cpu().numpy()
    f1, f2 = f0.clone(), f0.clone()
    s.flux(f1, scale=S_Q)
    s.flux(f2, scale=S_Q)
    s.close()
    tev.close()
    assert torch.equal(f1, f2)
    f0n, f1n = f0.cpu().numpy(), f1.cpu().numpy()
    off = np.ones(g.n_rows_t, dtype=bool)
    off[L.s_row] = False
    if off.any():
        assert np.array_equal(f1n[off], f0n[off])
    fq, Sq = bc.flux_apply(L, qv, S_Q, f0n)
    prob = {"flux": _entry(fq, Sq, bc.flux_apply_f64(L, qv, S_Q, f0n))}
    regimes_util.judge(f"surface_flux/{name}", prob, prob, {"flux": f1n}, {})


def test_create_refusals():
    tev, mesh, g = _tev("h8")
    faces = _faces("h8").copy()
    bad = faces.copy()
    bad[7, 2] = mesh.n_node
    with pytest.raises(fcg.FcgError) as e:
        fcg.TsiSurface(tev, bad)
    assert e.value.code == 3 and "face 7" in str(e.value)
    bad = faces.copy()
    bad[11, 3] = bad[11, 1]
    with pytest.raises(fcg.FcgError) as e:
        fcg.TsiSurface(tev, bad)
    assert e.value.code == 3 and "face 11" in str(e.value)
    empty = fcg.TsiSurface(tev, np.zeros((0, 4), dtype=np.int32))      # a surface without rows
    empty.set(COEFF, 300.0, 1.0)
    empty.convection(_t(np.zeros(g.n_cols_t)), fT=_nan(g.n_rows_t))
    assert empty.info["n_rows"] == 0
    empty.close()
    tev.close()


def test_set_refusals_keep_the_tables():
    tev, mesh, g = _tev("h8")
    faces = _faces("h8")
    s = fcg.TsiSurface(tev, faces)
    T = _t(300.0 + np.arange(g.n_cols_t) % 7)
    K, f = _nan(g.nnz_tt), _nan(g.n_rows_t)
    with pytest.raises(fcg.FcgError) as e:
        s.convection(T, fT=f, Ktt=K)                     # before any set
    assert e.value.code == 3
    with pytest.raises(fcg.FcgError) as e:
        s.flux(f)
    assert e.value.code == 3
    c, t, q = _tables(len(faces))
    s.set(c, t, q)
    with pytest.raises(fcg.FcgError) as e:
        s.convection(T)                                  # no output
    assert e.value.code == 3
    before = s.tables()
    K1, f1 = torch.zeros_like(K), torch.zeros_like(f)
    s.convection(T, fT=f1, Ktt=K1)
    for what, value in (("coeff", -1.0), ("coeff", float("nan")), ("coeff", float("inf")),
                        ("surtemp", float("nan")), ("flux", float("inf"))):
        tabs = dict(coeff=c.copy(), surtemp=t.copy(), flux=q.copy())
        tabs[what][5] = value
        with pytest.raises(fcg.FcgError) as e:
            s.set(**tabs)
        assert e.value.code == 3 and "face 5" in str(e.value) and e.value.bad_ele_gid == 5, (what, value)
        with pytest.raises(fcg.FcgError) as e:
            s.set(**{**dict(coeff=COEFF, surtemp=300.0, flux=0.0), what: value})   # the scalar form
        assert e.value.code == 3 and what in str(e.value)
    assert _same(before, s.tables())                     # the earlier tables stay
    K2, f2 = torch.zeros_like(K), torch.zeros_like(f)
    s.convection(T, fT=f2, Ktt=K2)
    assert torch.equal(K1, K2) and torch.equal(f1, f2)   # and give the earlier result
    torch.cuda.synchronize()
    assert torch.isnan(K).all() and torch.isnan(f).all()  # a refused call writes nothing
    s.close()
    tev.close()


@pytest.mark.parametrize("moved", [(33,), (50, 35)])
def test_collinear_face_reports_the_face(moved):
    """The four nodes of a boundary face moved onto the x axis in a copy of the coordinates: both tangent
    vectors are multiples of e_x, |dA| is exactly 0 at every Gauss point of that face, and set returns
    FCG_ERR_SINGULAR with its index; with two such faces the lower index is reported.  Every other face
    keeps an area element above 1e-3 at every Gauss point (asserted), far from any rounding."""
    _dev()
    box, g = mesh_of("h8")
    faces = _faces("h8")
    m = type("Moved", (), {})()
    for key in ("celltype", "n_ele", "n_node", "n_rows", "n_cols", "ele_nodes", "node_dof_row", "node_dof_col",
                "ele_gid"):
        setattr(m, key, getattr(box, key))
    X = np.array(box.node_x, dtype=np.float64)
    for face in moved:
        X[faces[face], 1:] = 0.0
    m.node_x = np.ascontiguousarray(X)
    dA = bc.face_matrices(4, X[faces], np.float64)[4]
    assert (dA[list(moved)] == 0).all() and float(np.delete(dA, moved, axis=0).min()) > 1e-3
    target = min(moved)
    tev = fcg.TsiEvaluator(m, MAT["youngs"], MAT["poisson"], MAT["thexpans"], MAT["inittemp"], MAT["conduct"],
                           graph=g)
    s = fcg.TsiSurface(tev, faces)
    with pytest.raises(fcg.FcgError) as e:
        s.set(COEFF, 300.0, 0.0)
    assert e.value.code == fcg.FCG_ERR_SINGULAR and e.value.bad_ele_gid == target
    assert f"face {target}" in str(e.value)
    K, f = _nan(g.nnz_tt), _nan(g.n_rows_t)
    with pytest.raises(fcg.FcgError) as e2:
        s.convection(_t(np.zeros(g.n_cols_t)), fT=f, Ktt=K)              # the surface counts as not set
    assert e2.value.code == 3
    torch.cuda.synchronize()
    assert torch.isnan(K).all() and torch.isnan(f).all()
    s.close()
    tev.close()
