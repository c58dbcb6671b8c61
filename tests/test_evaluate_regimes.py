"""The element evaluate (K and f_int of hex8 / hex27, linear or total Lagrangian, StVK or
CoupNeoHooke, on the structured, general, coloured and gather paths) and the other consumers of
the same element math (tangent_apply, tangent_diag, gp_stress, per-element materials, the mass)
outside the benign regime, judged against the extended-precision reference of element_ref.py.

Criterion.  For a quantity q with reference r and abs-sum scale S two errors are measured in
longdouble, e_n(q) = |q - r|_2 / |r|_2 and e_c(q) = max_i |q_i - r_i| / S_i.  With g the device
result and o the float64 oracle's on the same inputs, both measures must satisfy

    e(g) <= M * max(e(o), e_A(o)),

e_A(o) the oracle's error on the same mesh in the benign regime A (computed here, the floor).  M is
4: both sides are float64 evaluations of the same formulas in another order and association, so
their rounding errors are of one order, while a wrong term, index or constant is off by many.  A
case whose measured ratio exceeds 4 for a reason inherent to a legitimately different association
carries 2 x its measured ratio in MARGINS, with the cause in profiles/evaluate_regimes/README.md,
which lists every case's figures.  Every case also asserts finite output, that every measure
(the oracle's, the floor, the ratio) is a finite number, the path the context landed on, and that
two evaluates of one context agree bit for bit.

Regimes (displacement: BoxMesh.u_col(amp * h), h the smallest element edge of the unjittered box):
  A  benign: E = 210, nu = 0.3, unit box at the origin, jitter 0.1, amp 0.05 -- the anchor
  B  near-incompressible: nu = 0.499 and (StVK only) nu = 0.49999.  CoupNeoHooke at 0.49999 is
     left out: beta = 5e4 overflows I3^-beta for ordinary strains, in longdouble too
  C  the edges of the range fcg_create accepts: nu = 0 (lambda = 0) and nu = -0.5 (lambda < 0)
  D  far from the origin: lower = (1e4, -2e4, 3e4) with rotation (0.3, 0.5, 0.7) so that J is
     full, and lower = 1e6 (1, 1, 1)
  E  SI units: E = 2.1e11, the box 1e-3 wide, and the state of A scaled with it: the field of
     BoxMesh.node_displacement evaluated at X / 1e-3, times amp * h, so that the strains are A's
     (u_col itself has a fixed wavelength of 1 and would leave a box 1e-3 wide almost unstrained)
  F  large deformation: jitter 0.2, amp 0.3; the reference must show min det F >= 0.2 (and
     min I3 >= 0.04 for CoupNeoHooke) before the device is looked at (hex8: 0.62 / 0.39).
     hex27 takes jitter 0.12 and amp 0.2: BoxMesh's jitter is in units of the element edge, two
     node spacings of a hex27, and from 0.15 on the oracle refuses the mesh (err 1, det J < 0 at
     a node, though det J > 0 at every Gauss point), which the validity condition below forbids;
     0.12 is the largest of 0.1, 0.12, 0.15, 0.17, 0.2 that it accepts, and moves a hex27 node
     further, in node spacings, than 0.2 moves a hex8 node.  amp 0.3 inverts F on the hex27
     meshes (h is 1/3 and 1/2 there, 1/5 on the hex8 mesh); 0.2 gives det F / I3 0.27 / 0.071 on
     (3, 2, 2) and 0.22 / 0.050 on (2, 2, 1)
  G  near a converged Newton state: amp = 1e-8, TotLag
  H  thin elements: upper = (1, 1, 1e-3), aspect 1000 : 1.  h is the thin edge, so u is small
     against the long edges and the strains are about 1e-4: f carries the cancellation of a
     nearly undeformed state here as well as the geometry's
In every regime the reference must report det J > 0 at all Gauss points and the oracle err == 0.

Each test prints one line "REGIMES {json}" with its figures before it asserts.
"""

import functools
import importlib

import numpy as np
import pytest

import element_ref as er
import oracle_lib as orc
import regimes_util
import solver_ref as sr
from parity_util import oracle_evaluate
from regimes_util import _entry

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not er.EXTENDED, reason="np.longdouble has no 64-bit significand here")]

STVK, NEOHOOKE = fcg.MAT_STVK, fcg.MAT_ELASTHYPER_COUPNEOHOOKE
ORC_MAT = {STVK: orc.MAT_STVK, NEOHOOKE: orc.MAT_NEOHOOKE}
KINDS = {"linear": (fcg.LINEAR, STVK), "totlag": (fcg.TOTLAG, STVK), "neohooke": (fcg.TOTLAG, NEOHOOKE)}
RHO = 7.8

# mesh name -> (cell type, intervals, renumbered)
MESHES = {"h8": (fcg.HEX8, (5, 3, 2), False), "h8r": (fcg.HEX8, (5, 3, 2), True),
          "h27": (fcg.HEX27, (3, 2, 2), False), "h27c": (fcg.HEX27, (2, 2, 1), False)}
# configuration -> (mesh, path asked for == path the context must land on)
CONFIGS = {"h8_structured": ("h8", fcg.PATH_STRUCTURED), "h8_general": ("h8", fcg.PATH_GENERAL),
           "h8_gather": ("h8r", fcg.PATH_GATHER), "h27_general": ("h27", fcg.PATH_GENERAL),
           "h27_colored": ("h27c", fcg.PATH_COLORED)}
NEOHOOKE_CONFIGS = ("h8_general", "h8_gather", "h27_general")

BENIGN = dict(E=210.0, nu=0.3, lower=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0), rotation=(0.0, 0.0, 0.0),
              jitter=0.1, amp=0.05)
REGIMES = {
    "A": {},
    "B_nu0.499": dict(nu=0.499),
    "B_nu0.49999": dict(nu=0.49999),
    "C_nu0": dict(nu=0.0),
    "C_nu-0.5": dict(nu=-0.5),
    "D_1e4_rotated": dict(lower=(1e4, -2e4, 3e4), rotation=(0.3, 0.5, 0.7)),
    "D_1e6": dict(lower=(1e6, 1e6, 1e6)),
    "E_SI": dict(E=2.1e11, size=(1e-3, 1e-3, 1e-3), field_scale=1e-3),
    "F_large": dict(jitter=0.2, amp=0.3, jitter_hex27=0.12, amp_hex27=0.2),
    "G_converged": dict(amp=1e-8),
    "H_thin": dict(size=(1.0, 1.0, 1e-3)),
}

# case id -> margin in place of 4 (2 x the measured ratio, at most 64); causes in
# profiles/evaluate_regimes/README.md
MARGINS = {}


def _applies(kind, regime):
    if regime == "G_converged" and kind == "linear":
        return False
    return not (regime == "B_nu0.49999" and kind == "neohooke")


def _params(regime):
    p = dict(BENIGN)
    p.update(REGIMES[regime])
    return p


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=_dev())


def _h(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------ meshes, states
@functools.lru_cache(maxsize=None)
def _mesh(name, lower, size, rotation, jitter):
    celltype, iv, renumbered = MESHES[name]
    upper = tuple(lo + s for lo, s in zip(lower, size))
    box = fcg.BoxMesh(celltype, iv, lower=lower, upper=upper, rotation=rotation, jitter=jitter)
    h = min(s / n for s, n in zip(size, iv))
    if not renumbered:
        return box, None, h
    return fcg.Discretization.renumbered(box, seed=3), box, h


def _mesh_of(name, p):
    jitter = p.get("jitter_hex27", p["jitter"]) if MESHES[name][0] == fcg.HEX27 else p["jitter"]
    return _mesh(name, p["lower"], p["size"], p["rotation"], jitter)


def _state(name, p):
    """(mesh, u_col): u = BoxMesh.u_col(amp * h), carried to the new numbers on a renumbered mesh."""
    mesh, box, h = _mesh_of(name, p)
    amp = p.get("amp_hex27", p["amp"]) if mesh.celltype == fcg.HEX27 else p["amp"]
    src = mesh if box is None else box
    if "field_scale" in p:
        ub = _field_u_col(src, amp * h, p["field_scale"])
    else:
        ub = src.u_col(amp * h)
    if box is None:
        return mesh, ub
    u = np.zeros(box.n_cols)
    for d in range(3):
        u[3 * mesh.node_perm + d] = ub[3 * np.arange(box.n_node) + d]
    return mesh, u


def _field_u_col(box, amplitude, scale):
    """BoxMesh.u_col with the field of BoxMesh.node_displacement evaluated at node_x / scale."""
    X = np.asarray(box.node_x) / scale
    un = amplitude * np.stack([np.sin(2 * np.pi * X[:, 0]) * np.cos(np.pi * X[:, 1]),
                               np.sin(np.pi * X[:, 1]) * np.cos(2 * np.pi * X[:, 2]),
                               np.sin(2 * np.pi * X[:, 2]) * np.cos(np.pi * X[:, 0])], axis=1)
    u = np.zeros(box.n_cols)
    for d in range(3):
        u[box.node_dof_col + d] = un[:, d]
    return u


def _oracle_view(mesh):
    """What parity_util.oracle_evaluate reads, for a single-rank Discretization as for a BoxMesh."""
    if hasattr(mesh, "row_gid"):
        return mesh
    m = type("SingleRank", (), {})()
    m.row_gid = m.col_gid = np.arange(mesh.n_cols, dtype=np.int32)
    for k in ("nnz", "n_rows", "rowptr", "col_lid", "celltype", "n_ele", "ele_nodes", "n_node",
              "node_x", "node_dof_row"):
        setattr(m, k, getattr(mesh, k))
    m.node_gid = np.arange(mesh.n_node, dtype=np.int64)
    return m


def _checkerboard(mesh, p, iv):
    """0 / 1 by the parity of the element's lattice position, from its centroid."""
    c = np.asarray(mesh.node_x)[np.asarray(mesh.ele_nodes)].mean(axis=1)
    ijk = np.floor((c - np.asarray(p["lower"])) / np.asarray(p["size"]) * np.asarray(iv)).astype(np.int64)
    assert (ijk >= 0).all() and (ijk < np.asarray(iv)).all()
    return (ijk.sum(axis=1) % 2).astype(np.int32)


TABLE_E, TABLE_NU = [210.0, 2.1e8], [0.3, 0.499]


# ------------------------------------------------------------------------------ the judgement
def judge(case, prob, anchor, got):
    """regimes_util.judge with this file's MARGINS."""
    regimes_util.judge(case, prob, anchor, got, MARGINS)


# ------------------------------------------------------------------------------ 1. evaluate
@functools.lru_cache(maxsize=None)
def _evaluate_problem(meshname, kind, regime, table=False):
    """(mesh, u, label -> dict(r, S, eo) of K and f, the reference, the oracle's K, the element
    table or None): the reference with its scales and the oracle's errors, uniform material or
    (table=True) the checkerboard of TABLE_E / TABLE_NU.  The validity conditions are asserted
    here, before any device result exists."""
    p = _params(regime)
    kinem, material = KINDS[kind]
    mesh, u = _state(meshname, p)
    if table:
        em = _checkerboard(mesh, p, MESHES[meshname][1])
        assert 0 < em.sum() < len(em)
        eE, enu = np.asarray(TABLE_E)[em], np.asarray(TABLE_NU)[em]
        ref = er.assemble_ld(mesh, kinem, material, p["E"], p["nu"], u, ele_E=eE, ele_nu=enu)
        en = np.asarray(mesh.ele_nodes)
        X, un = np.asarray(mesh.node_x)[en], er.node_displacements(mesh, u)[en]
        Ke, fe = np.zeros(ref.el["Ke"].shape), np.zeros(ref.el["fe"].shape)
        for e in range(len(en)):
            err, Ke[e], fe[e] = orc.solid_evaluate(mesh.celltype, kinem, eE[e], enu[e], X[e], un[e],
                                                   material=ORC_MAT[material])
            assert err == 0
        Ko, fo = er.scatter_matrix(mesh, Ke), er.scatter_vector(mesh, fe)
    else:
        ref = er.assemble_ld(mesh, kinem, material, p["E"], p["nu"], u)
        err, _, Ko, fo = oracle_evaluate(_oracle_view(mesh), kinem, p["E"], p["nu"], u,
                                         material=ORC_MAT[material])
        assert err == 0
        em = None
    assert ref.min_detJ > 0
    if regime == "F_large":
        assert ref.min_detF >= 0.2, ref.min_detF
        assert material != NEOHOOKE or ref.min_I3 >= 0.04, ref.min_I3
    return mesh, u, dict(K=_entry(ref.K, ref.SK, Ko), f=_entry(ref.f, ref.Sf, fo)), ref, Ko, em


def _device_evaluate(ev, mesh, u):
    ut = _t(u)
    out = []
    for _ in range(2):
        f, K = _nan(mesh.n_rows), _nan(mesh.nnz)
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, ut, f, K)
        torch.cuda.synchronize()
        out.append((K, f))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    return dict(K=_h(out[0][0]), f=_h(out[0][1]))


EVALUATE_CASES = [(c, k, r) for c in CONFIGS for k in KINDS for r in REGIMES
                  if _applies(k, r) and (k != "neohooke" or c in NEOHOOKE_CONFIGS)]


@pytest.mark.parametrize("config,kind,regime", EVALUATE_CASES)
def test_evaluate(config, kind, regime):
    _dev()
    meshname, path = CONFIGS[config]
    mesh, u, prob, _, _, _ = _evaluate_problem(meshname, kind, regime)
    anchor = _evaluate_problem(meshname, kind, "A")[2]
    p = _params(regime)
    kinem, material = KINDS[kind]
    ev = fcg.Evaluator(mesh, kinematics=kinem, youngs=p["E"], poisson=p["nu"], path=path, material=material)
    assert ev.info.path == path
    got = _device_evaluate(ev, mesh, u)
    ev.close()
    judge(f"evaluate/{config}/{kind}/{regime}", prob, anchor, got)


# ------------------------------------------------------------------------------ 2. the other consumers
CONSUMER_REGIMES = ("A", "B_nu0.499", "D_1e4_rotated", "G_converged")


@functools.lru_cache(maxsize=None)
def _tangent_problem(regime):
    mesh, u, _, ref, Ko, _ = _evaluate_problem("h27", "totlag", regime)
    x = np.random.default_rng(6).uniform(-1, 1, mesh.n_cols)
    y, absy = sr.csr_matvec_ld(mesh.rowptr, mesh.col_lid, ref.K, x)
    yo, _ = sr.csr_matvec_ld(mesh.rowptr, mesh.col_lid, Ko, x)
    pos = sr.diag_block_positions(mesh)
    assert (pos >= 0).all()
    return mesh, u, x, pos, dict(y=_entry(y, absy, yo), diag=_entry(ref.K[pos], ref.SK[pos], Ko[pos]))


@pytest.mark.parametrize("regime", CONSUMER_REGIMES)
def test_tangent_apply_and_diag(regime):
    """hex27 TotLag, matrix-free: y = K(u) x against K_ref x scaled by |K_ref| |x|, the oracle's K
    applied in longdouble beside it; the nodal diagonal blocks against the reference's, scaled by
    the blocks of SK."""
    _dev()
    mesh, u, x, pos, prob = _tangent_problem(regime)
    p = _params(regime)
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=p["E"], poisson=p["nu"], path=fcg.PATH_GENERAL)
    assert ev.info.path == fcg.PATH_GENERAL
    ut, xt = _t(u), _t(x)
    runs = []
    for _ in range(2):
        y, D = _nan(mesh.n_rows), _nan(9 * (mesh.n_rows // 3))
        ev.tangent_apply(ut, xt, y)
        ev.tangent_diag(ut, None, diag=D)
        torch.cuda.synchronize()
        runs.append((y, D))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ev.close()
    judge(f"tangent/h27/totlag/{regime}", prob, _tangent_problem("A")[4],
          dict(y=_h(runs[0][0]), diag=_h(runs[0][1]).reshape(-1, 3, 3)))


STRESS_CASES = [(c, k, r) for c in ("h8_general", "h27_general") for k in ("totlag", "neohooke")
                for r in CONSUMER_REGIMES]


@functools.lru_cache(maxsize=None)
def _stress_problem(meshname, kind, regime):
    from test_stress import MeshReference
    p = _params(regime)
    kinem, material = KINDS[kind]
    mesh, u, _, ref, _, _ = _evaluate_problem(meshname, kind, regime)
    o = MeshReference(mesh, kinem, material, u, p["E"], p["nu"])
    el = ref.el
    prob = {k: _entry(er.voigt(el[k]), er.voigt(el[k + "_abs"]), getattr(o, k))
            for k in ("pk2", "cauchy", "gl", "ea")}
    prob["energy"] = _entry(el["energy"], el["energy_abs"], o.energy)
    return mesh, u, prob


@pytest.mark.parametrize("config,kind,regime", STRESS_CASES)
def test_gp_stress(config, kind, regime):
    """PK2, Cauchy, GL, EA at the Gauss points and the elements' strain energy against the
    reference's, each component scaled by the abs-sum of its terms; the oracle side is the float64
    reference of test_stress.py."""
    _dev()
    meshname, path = CONFIGS[config]
    mesh, u, prob = _stress_problem(meshname, kind, regime)
    p = _params(regime)
    kinem, material = KINDS[kind]
    ev = fcg.Evaluator(mesh, kinematics=kinem, youngs=p["E"], poisson=p["nu"], path=path, material=material)
    assert ev.info.path == path
    ut = _t(u)
    runs = []
    for _ in range(2):
        s1, e1, w = ev.gp_stress(ut, fcg.STRESS_PK2, fcg.STRAIN_GL, energy=True)
        s2, e2 = ev.gp_stress(ut, fcg.STRESS_CAUCHY, fcg.STRAIN_EA)
        runs.append(dict(pk2=s1, gl=e1, energy=w, cauchy=s2, ea=e2))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    ev.close()
    judge(f"gp_stress/{config}/{kind}/{regime}", prob, _stress_problem(meshname, kind, "A")[2],
          {k: _h(v) for k, v in runs[0].items()})


# the table replaces the uniform material, so regime B (a uniform nu) is regime A here
TABLE_CASES = [(c, r) for c in ("h8_general", "h27_general", "h8_gather")
               for r in ("A", "D_1e4_rotated", "G_converged")]


@pytest.mark.parametrize("config,regime", TABLE_CASES)
def test_element_materials(config, regime):
    """(E, nu) = (210, 0.3) and (2.1e8, 0.499) in a checkerboard, TotLag StVK: every interior row
    sums contributions six orders of magnitude apart, which e_c judges entry by entry in units of
    the terms behind each entry.  The oracle side is the oracle's element routine per element with
    that element's constants, scattered in float64."""
    _dev()
    meshname, path = CONFIGS[config]
    mesh, u, prob, _, _, em = _evaluate_problem(meshname, "totlag", regime, table=True)
    anchor = _evaluate_problem(meshname, "totlag", "A", table=True)[2]
    p = _params(regime)
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=p["E"], poisson=p["nu"], path=path)
    assert ev.info.path == path
    ev.set_element_materials(TABLE_E, TABLE_NU, em)
    got = _device_evaluate(ev, mesh, u)
    ev.close()
    judge(f"materials/{config}/totlag/{regime}", prob, anchor, got)


MASS_CASES = [(c, r) for c in ("h8_structured", "h8_gather", "h27_general", "h27_colored")
              for r in ("D_1e4_rotated", "D_1e6", "E_SI", "H_thin")]


@functools.lru_cache(maxsize=None)
def _mass_problem(meshname, regime):
    """The consistent mass on the graph, the compact node form and the lumped mass.  The float64
    counterpart: for hex8 the reference of test_mass.py; for hex27 that reference integrates with
    the stiffness rule's 13-digit constants and differs from the kernels' full-precision rule by
    1.5e-13 in every entry, so its formula is evaluated with the kernels' rule instead
    (_mass_f64): float64, the oracle's shape functions and numpy's determinant; of the
    longdouble reference it shares the index scatter only."""
    p = _params(regime)
    mesh = _mesh_of(meshname, p)[0]
    rule = er.mass_rule_full(mesh.celltype)
    M, SM, mindet = er.mass_ld(mesh, RHO, rule)
    assert mindet > 0
    if mesh.celltype == fcg.HEX8:
        from test_mass import MassRef
        Mo = MassRef(mesh, RHO).vals
    else:
        Mo = _mass_f64(mesh, RHO, rule)
    rowptr = np.asarray(mesh.rowptr)
    row0 = rowptr[0:-1:3]
    assert np.array_equal(np.sort(np.asarray(mesh.node_dof_row)), np.arange(0, mesh.n_rows, 3))
    idx = np.concatenate([s + 3 * np.arange((e - s) // 3) for s, e in zip(row0, rowptr[1::3])])
    rows = sr._rows_of(rowptr)
    lump = lambda v: _rowsum(rows, v, mesh.n_rows)  # noqa: E731
    prob = dict(M=_entry(M, SM, Mo), m_node=_entry(M[idx], SM[idx], Mo[idx]),
                m_lumped=_entry(lump(M), lump(SM), _rowsum(rows, Mo, mesh.n_rows)))
    return mesh, prob


def _mass_f64(mesh, rho, rule):
    """test_mass.element_mass's sum_g rho w det J N_a N_b with the Gauss rule `rule`, on the graph."""
    xi, w = rule
    en = np.asarray(mesh.ele_nodes)
    X = np.asarray(mesh.node_x)[en]
    ne, npe = en.shape
    m = np.zeros((ne, npe, npe))
    for g in range(len(w)):
        N = orc.shape(mesh.celltype, xi[g])
        J = np.einsum("ad,eak->edk", orc.shape_deriv(mesh.celltype, xi[g]), X)
        m += (w[g] * np.linalg.det(J))[:, None, None] * np.outer(N, N)
    Me = np.zeros((ne, npe, 3, npe, 3))
    for i in range(3):
        Me[:, :, i, :, i] = rho * m
    return er.scatter_matrix(mesh, Me.reshape(ne, 3 * npe, 3 * npe))


def _rowsum(rows, v, n):
    out = np.zeros(n, dtype=v.dtype)
    np.add.at(out, rows, v)
    return out


@pytest.mark.parametrize("config,regime", MASS_CASES)
def test_mass(config, regime):
    """mass_assemble and mass_nodal where det J degrades: far from the origin, at 1e-3 size, on
    thin elements.  The anchor is the same mesh in the benign regime."""
    _dev()
    meshname, path = CONFIGS[config]
    mesh, prob = _mass_problem(meshname, regime)
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=210.0, poisson=0.3, path=path)
    assert ev.info.path == path
    runs = []
    for _ in range(2):
        M = ev.mass(RHO, out=_nan(mesh.nnz))
        m_node, m_lumped = ev.mass_nodal(RHO)
        runs.append(dict(M=M, m_node=m_node, m_lumped=m_lumped))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    ev.close()
    judge(f"mass/{config}/{regime}", prob, _mass_problem(meshname, "A")[1],
          {k: _h(v) for k, v in runs[0].items()})
