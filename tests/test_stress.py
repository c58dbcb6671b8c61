"""Stress, strain and strain-energy output (fcg_gp_stress, fcg_gp_to_nodes) against a float64
numpy reference kept in this file, which shares nothing with the library: per element and Gauss
point oracle_lib's rule, shape functions and derivatives, J = dN^T X, grad_X N = dN J^-T,
H = u^T grad_X N, the strain E, then oracle_lib.stvk / oracle_lib.neohooke for S and
oracle_lib.stvk_energy (or the closed CoupNeoHooke form) for psi.

The CPU tests pin that reference first: sum_g fac B^T S reproduces the oracle's element force for
all six (cell type, kinematics, material) combinations, and a central difference of the neo-Hooke
energy reproduces it too.  The GPU tests then compare the device output with it.

The measure of every comparison is the largest absolute difference divided by the largest magnitude
of the quantity over the mesh; the tolerance is 1e-12, the figure of the project's other
float64-reference comparisons (test_mass.py, test_tangent_*.py).  Each test prints what it measured.
"""

import importlib

import numpy as np
import pytest

import oracle_lib as orc

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu
E, NU = 210.0, 0.3
E2, NU2 = 70.0, 0.2
TOL = 1e-12
STVK, NEOHOOKE = fcg.MAT_STVK, fcg.MAT_ELASTHYPER_COUPNEOHOOKE
STRESSES = {"pk2": fcg.STRESS_PK2, "cauchy": fcg.STRESS_CAUCHY}
STRAINS = {"gl": fcg.STRAIN_GL, "ea": fcg.STRAIN_EA}
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))  # xx yy zz xy yz xz


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(_dev())


def _h(t):
    return t.cpu().numpy()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=_dev())


def measure(got, ref):
    """max |got - ref| / max |ref|"""
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------ the reference
def voigt(T):
    return np.array([T[i, j] for i, j in VOIGT])


def tensor(v):
    T = np.zeros((3, 3))
    for k, (i, j) in enumerate(VOIGT):
        T[i, j] = T[j, i] = v[k]
    return T


def neohooke_energy(youngs, nu, Et):
    """psi = c (I1 - 3) + c / beta (J^(-2 beta) - 1), c = E / (4 (1 + nu)), beta = nu / (1 - 2 nu)"""
    c, beta = youngs / (4.0 * (1.0 + nu)), nu / (1.0 - 2.0 * nu)
    C = 2.0 * Et + np.eye(3)
    return c * (np.trace(C) - 3.0) + c / beta * (np.sqrt(np.linalg.det(C)) ** (-2.0 * beta) - 1.0)


def element_reference(celltype, kinem, material, youngs, nu, X, u):
    """One element: dict of pk2, cauchy, gl, ea [ngp][6] (tensor components), psi, fac [ngp],
    NX [ngp][npe][3], F [ngp][3][3], energy and the element force fe [npe][3] = sum_g fac B^T S."""
    xi, w = orc.gauss_points(celltype)
    ngp, npe = len(w), len(X)
    out = {k: np.zeros((ngp, 6)) for k in ("pk2", "cauchy", "gl", "ea")}
    out.update(psi=np.zeros(ngp), fac=np.zeros(ngp), NX=np.zeros((ngp, npe, 3)),
               F=np.zeros((ngp, 3, 3)), fe=np.zeros((npe, 3)))
    for g in range(ngp):
        dN = orc.shape_deriv(celltype, xi[g])
        J = dN.T @ X
        NX = dN @ np.linalg.inv(J).T
        H = u.T @ NX
        if kinem == fcg.TOTLAG:
            F = np.eye(3) + H
            Et = 0.5 * (F.T @ F - np.eye(3))
        else:
            F = np.eye(3)
            Et = 0.5 * (H + H.T)
        gl = voigt(Et) * np.array([1, 1, 1, 2, 2, 2.0])  # strain-like: doubled shears
        if material == STVK:
            S = orc.stvk(youngs, nu, gl)[0]
            psi = orc.stvk_energy(youngs, nu, gl)
        else:
            S = orc.neohooke(youngs, nu, gl)[0]
            psi = neohooke_energy(youngs, nu, Et)
        St = tensor(S)
        Fi = np.linalg.inv(F)
        out["pk2"][g] = S
        out["cauchy"][g] = voigt(F @ St @ F.T / np.linalg.det(F))
        out["gl"][g] = voigt(Et)
        out["ea"][g] = voigt(Fi.T @ Et @ Fi)
        out["psi"][g] = psi
        out["fac"][g] = w[g] * np.linalg.det(J)
        out["NX"][g], out["F"][g] = NX, F
        out["fe"] += out["fac"][g] * NX @ (F @ St).T
    out["energy"] = float(np.sum(out["fac"] * out["psi"]))
    return out


class MeshReference:
    """The reference of a whole mesh at u_col: pk2, cauchy, gl, ea [n_ele][ngp][6], energy [n_ele]."""

    def __init__(self, mesh, kinem, material, u_col, youngs=E, nu=NU):
        youngs = np.broadcast_to(np.asarray(youngs, dtype=np.float64), (mesh.n_ele,))
        nu = np.broadcast_to(np.asarray(nu, dtype=np.float64), (mesh.n_ele,))
        un = u_col[mesh.node_dof_col[:, None] + np.arange(3)]
        self.el = [element_reference(mesh.celltype, kinem, material, youngs[e], nu[e],
                                     mesh.node_x[en], un[en]) for e, en in enumerate(mesh.ele_nodes)]
        for k in ("pk2", "cauchy", "gl", "ea"):
            setattr(self, k, np.array([r[k] for r in self.el]))
        self.energy = np.array([r["energy"] for r in self.el])


def internal_force(mesh, ref, pk2):
    """sum_e sum_g fac B^T S on the owned rows from the given PK2 stresses [n_ele][ngp][6] and the
    reference's geometry (F^T for TOTLAG is in ref.el[e]["F"], the identity for LINEAR)."""
    f = np.zeros(mesh.n_rows)
    for e, en in enumerate(mesh.ele_nodes):
        r = ref.el[e]
        fe = np.zeros((len(en), 3))
        for g in range(len(r["fac"])):
            fe += r["fac"][g] * r["NX"][g] @ (r["F"][g] @ tensor(pk2[e, g])).T
        for a, n in enumerate(en):
            if mesh.node_dof_row[n] >= 0:
                f[mesh.node_dof_row[n]:mesh.node_dof_row[n] + 3] += fe[a]
    return f


def _unit_element(celltype, seed):
    rng = np.random.default_rng(seed)
    X = orc.node_param_coords(celltype) * 0.5 + 0.05 * rng.uniform(-1, 1, (8 if celltype == fcg.HEX8 else 27, 3))
    u = 0.05 * rng.uniform(-1, 1, X.shape)
    return X, u


COMBOS = [(ct, k, m) for ct in (fcg.HEX8, fcg.HEX27)
          for k, m in ((fcg.LINEAR, STVK), (fcg.TOTLAG, STVK), (fcg.TOTLAG, NEOHOOKE))]


@pytest.mark.parametrize("celltype,kinem,material", COMBOS)
def test_reference_reproduces_oracle_force(celltype, kinem, material):
    """The yardstick's sum_g fac B^T S is the oracle's element force.  Both are float64 sums of
    ngp x 6 products per entry in different orders: 1e-13 of the largest entry leaves two decades
    above the rounding of such sums (measured 6e-15 at most)."""
    X, u = _unit_element(celltype, 3)
    err, _, fe = orc.solid_evaluate(celltype, kinem, E, NU, X, u, want_k=False, material=material)
    assert err == 0
    ref = element_reference(celltype, kinem, material, E, NU, X, u)
    m = measure(ref["fe"].ravel(), fe)
    print("reference force vs oracle:", m)
    assert m <= 1e-13


@pytest.mark.parametrize("celltype", [fcg.HEX8, fcg.HEX27])
def test_reference_energy_is_the_force_potential(celltype):
    """A central difference of the neo-Hooke energy reproduces the oracle's element force.  With
    the step 1e-5 the difference's truncation error h^2 / 6 W''' is about 1e-9 of the force for this
    element (the third derivatives are O(100) per unit length^2 at element size 1), its rounding
    error eps W / h about 1e-13: the bound 1e-7 is the difference's accuracy with margin
    (measured 6e-9 at most), far below any error in the energy formula, which would show at O(1)."""
    X, u = _unit_element(celltype, 5)
    err, _, fe = orc.solid_evaluate(celltype, fcg.TOTLAG, E, NU, X, u, want_k=False, material=NEOHOOKE)
    assert err == 0
    h = 1e-5
    num = np.zeros_like(u)
    for a in range(u.shape[0]):
        for d in range(3):
            up, um = u.copy(), u.copy()
            up[a, d] += h
            um[a, d] -= h
            num[a, d] = (element_reference(celltype, fcg.TOTLAG, NEOHOOKE, E, NU, X, up)["energy"] -
                         element_reference(celltype, fcg.TOTLAG, NEOHOOKE, E, NU, X, um)["energy"]) / (2 * h)
    m = measure(num.ravel(), fe)
    print("dW/du vs oracle force:", m)
    assert m <= 1e-7


def extrapolation_matrix(celltype):
    xi, _ = orc.gauss_points(celltype)
    return np.array([orc.shape(celltype, x) for x in xi])  # X[g][a] = N_a(xi_g)


@pytest.mark.parametrize("celltype,cond", [(fcg.HEX8, 5.2), (fcg.HEX27, 13.5)])
def test_extrapolation_matrix(celltype, cond):
    """X[g][a] = N_a(xi_g) on the stiffness rule is square and well conditioned, and its inverse
    reproduces constants (rows sum to 1: the partition of unity)."""
    Xm = extrapolation_matrix(celltype)
    assert Xm.shape[0] == Xm.shape[1]
    c = np.linalg.cond(Xm)
    rows = np.abs(np.linalg.inv(Xm).sum(axis=1) - 1.0).max()
    print("cond", c, "row sums - 1", rows)
    assert abs(c - cond) <= 0.05
    assert rows <= 1e-14


# ------------------------------------------------------------------------------ the cases
def _h8():
    return fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1)


def _h27():
    return fcg.BoxMesh(fcg.HEX27, (2, 2, 1), jitter=0.1)


MESHES = {
    "h8_auto": (_h8, fcg.PATH_AUTO),
    "h8_gather": (_h8, fcg.PATH_GATHER),
    "h8_general": (_h8, fcg.PATH_GENERAL),
    "h8_renumbered": (lambda: fcg.Discretization.renumbered(_h8()), fcg.PATH_AUTO),
    "h27_general": (_h27, fcg.PATH_GENERAL),
    "h27_colored": (_h27, fcg.PATH_COLORED),
    "h8_rank0of2": (lambda: fcg.BoxMesh(fcg.HEX8, (4, 2, 2), jitter=0.1, rank=0, nranks=2), fcg.PATH_AUTO),
}
KINDS = {"linear": (fcg.LINEAR, STVK), "totlag": (fcg.TOTLAG, STVK), "neohooke": (fcg.TOTLAG, NEOHOOKE)}
# CoupNeoHooke wherever fcg_create accepts it: not on the gather path (hex8 St.Venant-Kirchhoff only)
CASES = [(m, k) for m in MESHES for k in KINDS if not (m == "h8_gather" and k == "neohooke")]

_mesh_cache, _ref_cache = {}, {}


def _mesh(name):
    if name not in _mesh_cache:
        _mesh_cache[name] = MESHES[name][0]()
    return _mesh_cache[name]


def _u_col(mesh, seed=11):
    """seeded random displacement of amplitude 0.05 h, h the shortest element edge"""
    en = mesh.ele_nodes[0]
    h = min(np.linalg.norm(mesh.node_x[en[a]] - mesh.node_x[en[0]]) for a in (1, 3, 4))
    rng = np.random.default_rng(seed)
    un = 0.05 * h * rng.uniform(-1, 1, (mesh.n_node, 3))
    u = np.zeros(mesh.n_cols)
    for d in range(3):
        u[mesh.node_dof_col + d] = un[:, d]
    return u


def _reference(name, kind):
    if (name, kind) not in _ref_cache:
        mesh = _mesh(name)
        _ref_cache[name, kind] = MeshReference(mesh, *KINDS[kind], _u_col(mesh))
    return _ref_cache[name, kind]


def _evaluator(name, kind):
    kinem, material = KINDS[kind]
    return fcg.Evaluator(_mesh(name), kinematics=kinem, youngs=E, poisson=NU, path=MESHES[name][1],
                         material=material)


# ------------------------------------------------------------------------------ GPU tests
@gpu
@pytest.mark.parametrize("name,kind", CASES)
def test_parity(name, kind):
    """PK2, Cauchy, GL, EA and the energy against the reference; outputs prefilled with NaN come
    back NaN-free; a second call gives the same bits."""
    _dev()
    mesh, ref = _mesh(name), _reference(name, kind)
    ev = _evaluator(name, kind)
    u = _t(_u_col(mesh))
    s1, e1, w = ev.gp_stress(u, fcg.STRESS_PK2, fcg.STRAIN_GL, energy=True)
    s2, e2 = ev.gp_stress(u, fcg.STRESS_CAUCHY, fcg.STRAIN_EA)
    assert s1.shape == (mesh.n_ele, ev.ngp, 6) and w.shape == (mesh.n_ele,)
    got = {"pk2": s1, "gl": e1, "cauchy": s2, "ea": e2, "energy": w}
    for k, v in got.items():
        m = measure(_h(v), getattr(ref, k))
        print(f"{name} {kind} {k}: {m:.3e}")
        assert m <= TOL, (k, m)
    # every entry is written
    sn, en_, wn = _nan(mesh.n_ele, ev.ngp, 6), _nan(mesh.n_ele, ev.ngp, 6), _nan(mesh.n_ele)
    ev.gp_stress_raw(fcg.STRESS_PK2, fcg.STRAIN_GL, u, sn, en_, wn)
    for v in (sn, en_, wn):
        assert not torch.isnan(v).any()
    # determinism
    assert torch.equal(sn, s1) and torch.equal(en_, e1) and torch.equal(wn, w)
    # the energy alone, and one buffer alone, are the same numbers
    assert torch.equal(ev.strain_energy(u), w)
    assert torch.equal(ev.gp_stress(u, fcg.STRESS_CAUCHY, fcg.STRAIN_NONE), s2)
    if KINDS[kind][0] == fcg.LINEAR:
        assert torch.equal(s1, s2) and torch.equal(e1, e2)  # EA equals GL, Cauchy equals PK2
        s0, e0 = ev.gp_stress(None)  # u = 0
        assert float(s0.abs().max()) == 0.0 and float(e0.abs().max()) == 0.0


G = np.array([[0.021, -0.013, 0.017], [0.009, -0.024, 0.011], [-0.015, 0.019, 0.023]])


@gpu
@pytest.mark.parametrize("kinem", [fcg.LINEAR, fcg.TOTLAG])
@pytest.mark.parametrize("name", list(MESHES))
def test_patch(name, kinem):
    """u = G X on the jittered meshes: every Gauss point's GL strain is 1/2 (G + G^T + G^T G)
    (TOTLAG) or 1/2 (G + G^T) (LINEAR), and so is every owned node's value after gp_to_nodes."""
    _dev()
    mesh = _mesh(name)
    ev = fcg.Evaluator(mesh, kinematics=kinem, youngs=E, poisson=NU, path=MESHES[name][1])
    un = mesh.node_x @ G.T
    u = np.zeros(mesh.n_cols)
    for d in range(3):
        u[mesh.node_dof_col + d] = un[:, d]
    want = voigt(0.5 * (G + G.T + (G.T @ G if kinem == fcg.TOTLAG else 0.0)))
    gl = ev.gp_stress(_t(u), fcg.STRESS_NONE, fcg.STRAIN_GL)
    m = measure(_h(gl), np.broadcast_to(want, gl.shape))
    nodes = _h(ev.gp_to_nodes(gl))
    owned = mesh.node_dof_row >= 0
    mn = measure(nodes[owned], np.broadcast_to(want, nodes[owned].shape))
    print(f"{name} kinem {kinem}: gauss points {m:.3e} nodes {mn:.3e}")
    assert m <= TOL and mn <= TOL


@gpu
@pytest.mark.parametrize("name,kind", CASES)
def test_consistent_with_evaluate(name, kind):
    """sum_e sum_g fac B^T S of the DEVICE's PK2 stresses, formed in numpy and scattered to the
    owned rows, is the internal force the context's evaluate assembles."""
    _dev()
    mesh, ref = _mesh(name), _reference(name, kind)
    ev = _evaluator(name, kind)
    u = _t(_u_col(mesh))
    pk2 = _h(ev.gp_stress(u, fcg.STRESS_PK2, fcg.STRAIN_NONE))
    f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=_dev())
    ev.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f)
    m = measure(internal_force(mesh, ref, pk2), _h(f))
    print(f"{name} {kind}: f_int from the device stresses vs evaluate {m:.3e}")
    assert m <= TOL


TABLE_CASES = [("h8_gather", "linear"), ("h8_gather", "totlag"), ("h8_general", "totlag"),
               ("h8_general", "neohooke"), ("h27_general", "linear"), ("h27_general", "neohooke")]


@gpu
@pytest.mark.parametrize("name,kind", TABLE_CASES)
def test_element_materials(name, kind):
    """A two-material table: each element's stress and energy follow its own constants (on the
    gather path the device table is in storage-slot order, this call walks column-element order);
    a table whose entries all equal the context's material gives the uniform call's bits."""
    _dev()
    mesh = _mesh(name)
    kinem, material = KINDS[kind]
    ev = _evaluator(name, kind)
    u_col = _u_col(mesh)
    u = _t(u_col)
    uniform = ev.gp_stress(u, fcg.STRESS_CAUCHY, fcg.STRAIN_GL, energy=True)
    ele_mat = np.random.default_rng(2).integers(0, 2, mesh.n_ele).astype(np.int32)
    ele_mat[:2] = (0, 1)
    ev.set_element_materials([E, E2], [NU, NU2], ele_mat)
    ref = MeshReference(mesh, kinem, material, u_col, np.where(ele_mat == 0, E, E2),
                        np.where(ele_mat == 0, NU, NU2))
    s, e, w = ev.gp_stress(u, fcg.STRESS_CAUCHY, fcg.STRAIN_GL, energy=True)
    for k, v in (("cauchy", s), ("gl", e), ("energy", w)):
        m = measure(_h(v), getattr(ref, k))
        print(f"{name} {kind} two materials {k}: {m:.3e}")
        assert m <= TOL, (k, m)
    assert not torch.equal(s, uniform[0])
    ev.set_element_materials([E2, E], [NU2, NU], np.ones(mesh.n_ele, dtype=np.int32))
    same = ev.gp_stress(u, fcg.STRESS_CAUCHY, fcg.STRAIN_GL, energy=True)
    for a, b in zip(same, uniform):
        assert torch.equal(a, b)
    ev.set_element_materials(None)
    for a, b in zip(ev.gp_stress(u, fcg.STRESS_CAUCHY, fcg.STRAIN_GL, energy=True), uniform):
        assert torch.equal(a, b)


def nodal_reference(mesh, gp):
    """the numpy mean over each node's elements of the per-element X^-1 gp, [n_node][6]"""
    Xi = np.linalg.inv(extrapolation_matrix(mesh.celltype))
    acc, cnt = np.zeros((mesh.n_node, 6)), np.zeros(mesh.n_node)
    for e, en in enumerate(mesh.ele_nodes):
        np.add.at(acc, en, Xi @ gp[e])
        np.add.at(cnt, en, 1.0)
    return acc / cnt[:, None]


@gpu
@pytest.mark.parametrize("name", ["h8_general", "h8_renumbered", "h27_general", "h27_colored", "h8_rank0of2"])
def test_nodal_average(name):
    """gp_to_nodes of seeded random Gauss-point data is the mean of the per-element X^-1 gp on the
    owned nodes; the rows of the other nodes are not touched (they stay NaN in a fresh output, and
    keep a caller's values); two calls give the same bits."""
    _dev()
    mesh = _mesh(name)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=MESHES[name][1])
    gp = np.random.default_rng(8).uniform(-1, 1, (mesh.n_ele, ev.ngp, 6))
    out = ev.gp_to_nodes(_t(gp))
    assert out.shape == (mesh.n_node, 6)
    got = _h(out)
    owned = mesh.node_dof_row >= 0
    if name == "h8_rank0of2":
        assert 0 < owned.sum() < mesh.n_node
    assert np.array_equal(np.isnan(got).any(axis=1), ~owned)
    assert not np.isnan(got[owned]).any()
    m = measure(got[owned], nodal_reference(mesh, gp)[owned])
    print(f"{name}: nodal average {m:.3e}")
    assert m <= TOL
    again = torch.full_like(out, 7.0)
    assert ev.gp_to_nodes(_t(gp), out=again) is again
    assert torch.equal(again[_t(owned, torch.bool)], out[_t(owned, torch.bool)])
    assert bool((again[_t(~owned, torch.bool)] == 7.0).all())


@gpu
def test_argument_errors():
    _dev()
    mesh = _mesh("h8_general")
    ev = _evaluator("h8_general", "totlag")
    u = _t(_u_col(mesh))
    buf, w = _nan(mesh.n_ele, 8, 6), _nan(mesh.n_ele)
    bad_calls = {
        "all outputs NULL": (fcg.STRESS_NONE, fcg.STRAIN_NONE, u, None, None, None),
        "stress buffer, type NONE": (fcg.STRESS_NONE, fcg.STRAIN_NONE, u, buf, None, w),
        "strain buffer, type NONE": (fcg.STRESS_NONE, fcg.STRAIN_NONE, u, None, buf, w),
        "stress type, no buffer": (fcg.STRESS_PK2, fcg.STRAIN_NONE, u, None, None, w),
        "strain type, no buffer": (fcg.STRESS_NONE, fcg.STRAIN_EA, u, None, None, w),
        "unknown stress type": (7, fcg.STRAIN_NONE, u, buf, None, None),
        "no displacement under TOTLAG": (fcg.STRESS_PK2, fcg.STRAIN_NONE, None, buf, None, None),
    }
    for what, args in bad_calls.items():
        with pytest.raises(fcg.FcgError) as ei:
            ev.gp_stress_raw(*args)
        assert ei.value.code == fcg.FCG_ERR_ARG, what
        assert "fcg_gp_stress" in str(ei.value), what
    assert torch.isnan(buf).all() and torch.isnan(w).all()  # nothing was written
    # the context still works
    assert measure(_h(ev.gp_stress(u, fcg.STRESS_PK2, fcg.STRAIN_NONE)), _reference("h8_general", "totlag").pk2) <= TOL


@gpu
def test_inverted_element():
    """One hex8 element with two nodes swapped: det J < 0 at a Gauss point is an error code with
    the element's GID, not a fault, and a healthy context is unaffected afterwards."""
    _dev()
    X = orc.node_param_coords(fcg.HEX8) * 0.5
    xi, _ = orc.gauss_points(fcg.HEX8)
    en = np.array([[1, 0, 2, 3, 4, 5, 6, 7]])
    dets = [np.linalg.det(orc.shape_deriv(fcg.HEX8, x).T @ X[en[0]]) for x in xi]
    assert min(dets) < 0.0
    dis = fcg.Discretization.from_elements(fcg.HEX8, en, X)
    dis.ele_gid = np.array([41], dtype=np.int32)
    healthy = _evaluator("h8_general", "linear")
    mesh = _mesh("h8_general")
    u = _t(_u_col(mesh))
    f0 = torch.zeros(mesh.n_rows, dtype=torch.float64, device=_dev())
    healthy.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f0)
    bad = fcg.Evaluator(dis, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_GENERAL)
    with pytest.raises(fcg.FcgError) as ei:
        bad.gp_stress(None)
    assert ei.value.code == fcg.FCG_ERR_NODAL_DETJ
    assert ei.value.bad_ele_gid == 41 and "41" in str(ei.value)
    f1 = torch.zeros_like(f0)
    healthy.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f1)
    assert torch.equal(f0, f1)
    assert measure(_h(healthy.gp_stress(u, fcg.STRESS_PK2, fcg.STRAIN_NONE)),
                   _reference("h8_general", "linear").pk2) <= TOL
