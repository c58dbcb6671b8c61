"""Consistent mass (fcg_mass_assemble / fcg_mass_nodal) and the effective tangent
(fcg_effective_tangent) against a float64 numpy reference that shares nothing with the library:
each element's m_ab = sum_g rho w_g det J_g N_a N_b from oracle_lib's Gauss rule and shape
functions and the mesh's node_x, scattered into the mesh's CSR by (row LID, column LID).

Total mass (test_total_mass) is asserted as rho V to 1e-13 relative.  The numpy reference meets
that for hex8 (measured on the CPU: 4e-16 and 7e-16 at (3,2,2) and (4,3,3)) but not for hex27: the
reference's hex_27point rule keeps 13-digit weights (0.5555555555556, 0.8888888888889) whose sum over
the 27 points is 8 (1 + 1.50e-13), so every integral of that rule carries the factor -- measured
1.4921e-13 at (2,2,1) and (3,2,2), test_reference_total_mass.  The library integrates the mass
with the same 27 points and weights in full double precision (sqrt(3/5), 5/9, 8/9), so its total is
rho V to rounding and its entries differ from this reference by 1.5e-13, inside the 1e-12 the
comparisons ask.
"""

import importlib

import numpy as np
import pytest

import oracle_lib as orc
import solver_ref as sr
from parity_util import rel_err

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu
E, NU = 210.0, 0.3
RHO = 7.8
EPS = np.finfo(np.float64).eps


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(_dev())


def _h(t):
    return t.cpu().numpy()


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


# ------------------------------------------------------------------------------ the reference
def element_mass(celltype, X):
    """[npe][npe] sum_g w_g det J_g N_a N_b of one element (unit density)."""
    xi, w = orc.gauss_points(celltype)
    m = np.zeros((len(X), len(X)))
    for g in range(len(w)):
        N = orc.shape(celltype, xi[g])
        J = orc.shape_deriv(celltype, xi[g]).T @ X
        m += w[g] * np.linalg.det(J) * np.outer(N, N)
    return m


class MassRef:
    """The reference mass of a mesh on its CSR graph: vals [nnz]; trip [pairs][3] the positions of
    the three diagonal entries of every (row node, element-neighbour node) block; pair_row0 the
    block's first row."""

    def __init__(self, mesh, rho):
        rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (mesh.n_ele,))
        self.vals = np.zeros(mesh.nnz)
        pos = {}
        for e, en in enumerate(mesh.ele_nodes):
            me = rho[e] * element_mass(mesh.celltype, mesh.node_x[en])
            for ia, a in enumerate(en):
                r0 = int(mesh.node_dof_row[a])
                if r0 < 0:
                    continue
                for ib, b in enumerate(en):
                    key = (r0, int(mesh.node_dof_col[b]))
                    if key not in pos:
                        pos[key] = [sr.entry_pos(mesh, r0 + d, key[1] + d) for d in range(3)]
                        assert min(pos[key]) >= 0
                    for j in pos[key]:
                        self.vals[j] += me[ia, ib]
        self.trip = np.array(list(pos.values()), dtype=np.int64).reshape(-1, 3)
        self.pair_row0 = np.array([k[0] for k in pos], dtype=np.int64)
        self.offdiag = np.ones(mesh.nnz, dtype=bool)
        self.offdiag[self.trip.ravel()] = False

    def lumped(self, n_rows):
        out = np.zeros(n_rows)
        for d in range(3):
            np.add.at(out, self.pair_row0 + d, self.vals[self.trip[:, d]])
        return out


def rule_weight(celltype):
    """sum of the rule's weights / 8: 1 for hex8, 1 + 1.5e-13 for the reference's hex_27point."""
    return float(np.sum(orc.gauss_points(celltype)[1])) / 8.0


# ------------------------------------------------------------------------------ the cases
def _renumbered():
    return fcg.Discretization.renumbered(fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1))


CASES = {
    "h8_322_auto": (lambda: fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1), fcg.PATH_AUTO, fcg.PATH_STRUCTURED),
    "h8_322_gather": (lambda: fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1), fcg.PATH_GATHER, fcg.PATH_GATHER),
    "h8_322_general": (lambda: fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1), fcg.PATH_GENERAL, fcg.PATH_GENERAL),
    "h8_433_general": (lambda: fcg.BoxMesh(fcg.HEX8, (4, 3, 3), jitter=0.1), fcg.PATH_GENERAL, fcg.PATH_GENERAL),
    "h8_renumbered": (_renumbered, fcg.PATH_AUTO, None),
    "h27_221_general": (lambda: fcg.BoxMesh(fcg.HEX27, (2, 2, 1), jitter=0.05), fcg.PATH_GENERAL, fcg.PATH_GENERAL),
    "h27_221_lattice": (lambda: fcg.BoxMesh(fcg.HEX27, (2, 2, 1), jitter=0.05), fcg.PATH_STRUCTURED, fcg.PATH_COLORED),
    "h27_322_general": (lambda: fcg.BoxMesh(fcg.HEX27, (3, 2, 2), jitter=0.05), fcg.PATH_GENERAL, fcg.PATH_GENERAL),
    "h27_322_lattice": (lambda: fcg.BoxMesh(fcg.HEX27, (3, 2, 2), jitter=0.05), fcg.PATH_STRUCTURED, fcg.PATH_COLORED),
}
SINGLE = list(CASES)
for _ct, _name, _iv in ((fcg.HEX8, "h8_433", (4, 3, 3)), (fcg.HEX27, "h27_222", (2, 2, 2))):
    for _r in range(2):
        for _strict in (False, True):
            CASES["%s_r%d_%s" % (_name, _r, "strict" if _strict else "ghost")] = (
                lambda ct=_ct, iv=_iv, r=_r, s=_strict: fcg.BoxMesh(
                    ct, iv, jitter=0.1 if ct == fcg.HEX8 else 0.05, rank=r, nranks=2, strict=s),
                fcg.PATH_AUTO, None)
ALL = list(CASES)

_cache = {}


def _case(name):
    """(mesh, evaluator, reference at density RHO), built once per case and left unchanged."""
    _dev()
    if name not in _cache:
        make, path, lands = CASES[name]
        mesh = make()
        ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU, path=path)
        if lands is not None:
            assert ev.info.path == lands, (name, ev.info.path)
        _cache[name] = (mesh, ev, MassRef(mesh, RHO))
    return _cache[name]


def _u(mesh):
    return 2e-2 * np.random.default_rng(3).standard_normal(mesh.n_cols)


def _expand(mesh, m_node):
    """The compact node form written onto the graph by numpy (the layout of fcg_mass_nodal)."""
    out = np.zeros(mesh.nnz)
    for row0 in np.sort(mesh.node_dof_row[mesh.node_dof_row >= 0]):
        s = int(mesh.rowptr[row0])
        ln = int(mesh.rowptr[row0 + 1]) - s
        assert s % 9 == 0 and ln % 3 == 0
        for t in range(ln // 3):
            for d in range(3):
                out[s + d * ln + 3 * t + d] = m_node[s // 9 + t]
    return out


# ------------------------------------------------------------------------------ CPU: the yardstick
@pytest.mark.parametrize("celltype,iv,jitter", [(fcg.HEX8, (3, 2, 2), 0.1), (fcg.HEX8, (4, 3, 3), 0.1),
                                                (fcg.HEX27, (2, 2, 1), 0.05), (fcg.HEX27, (3, 2, 2), 0.05)])
def test_reference_total_mass(celltype, iv, jitter):
    """The numpy reference integrates the unit box's volume to 1e-13 of V sum(w) / 8; for hex8
    sum(w) = 8 exactly, so that is V itself (see the module docstring for hex27)."""
    mesh = fcg.BoxMesh(celltype, iv, jitter=jitter)
    tot = sum(element_mass(celltype, mesh.node_x[en]).sum() for en in mesh.ele_nodes)
    print("reference total mass - V:", tot - 1.0, "rule weight - 1:", rule_weight(celltype) - 1.0)
    assert abs(tot - rule_weight(celltype)) <= 1e-13
    if celltype == fcg.HEX8:
        assert rule_weight(celltype) == 1.0 and abs(tot - 1.0) <= 1e-13


# ------------------------------------------------------------------------------ 1. the reference
@gpu
@pytest.mark.parametrize("name", ALL)
def test_mass_against_reference(name):
    mesh, ev, ref = _case(name)
    M = _h(ev.mass(RHO, out=_nan(mesh.nnz)))
    print(name, "rel_err", rel_err(M, ref.vals))
    assert np.all(np.isfinite(M))
    assert rel_err(M, ref.vals) <= 1e-12
    assert np.all(M[ref.offdiag] == 0.0)
    assert np.array_equal(M[ref.trip[:, 0]], M[ref.trip[:, 1]])
    assert np.array_equal(M[ref.trip[:, 0]], M[ref.trip[:, 2]])
    rnd = np.random.default_rng(7).standard_normal(mesh.nnz)
    A = _h(ev.mass(RHO, mode=fcg.ACCUMULATE, out=_t(rnd)))
    assert rel_err(A, rnd + ref.vals) <= 1e-12
    assert np.array_equal(A[ref.offdiag], rnd[ref.offdiag])


# ------------------------------------------------------------------------------ 2. total mass
@gpu
@pytest.mark.parametrize("name", [n for n in SINGLE if n != "h8_renumbered"])
def test_total_mass(name):
    """Sum over the x rows and x columns = rho V (unit box, interior jitter only) to 1e-13
    relative: a partition-of-unity sum, independent of the numpy reference."""
    mesh, ev, ref = _case(name)
    M = _h(ev.mass(RHO))
    tot = float(np.sum(M[ref.trip[:, 0]]))
    print(name, "total / (rho V) - 1:", tot / RHO - 1.0)
    assert abs(tot - RHO * 1.0) <= 1e-13 * RHO


# ------------------------------------------------------------------------------ 3. densities
@gpu
@pytest.mark.parametrize("name", ["h8_322_auto", "h8_322_gather", "h8_433_general", "h27_322_general",
                                  "h27_221_lattice", "h8_433_r1_ghost", "h27_222_r0_strict"])
def test_per_element_density(name):
    mesh, ev, ref = _case(name)
    cz = mesh.node_x[mesh.ele_nodes].mean(axis=1)[:, 2]
    rho = np.where(cz < np.median(cz) + 1e-9, 2.5, 11.0)  # two layers of elements
    assert len(np.unique(rho)) == 2
    M = _h(ev.mass(1.0, ele_density=rho))
    assert rel_err(M, MassRef(mesh, rho).vals) <= 1e-12
    Mu = _h(ev.mass(123.0, ele_density=np.full(mesh.n_ele, RHO)))
    assert np.array_equal(Mu, _h(ev.mass(RHO)))


# ------------------------------------------------------------------------------ 4. compact form
@gpu
@pytest.mark.parametrize("name", ALL)
def test_compact_form(name):
    mesh, ev, ref = _case(name)
    m_node, m_lumped = ev.mass_nodal(RHO)
    assert m_node.numel() == mesh.nnz // 9 and m_lumped.numel() == mesh.n_rows
    M = _h(ev.mass(RHO))
    assert np.array_equal(_expand(mesh, _h(m_node)), M)
    lum = _h(m_lumped)
    lref = ref.lumped(mesh.n_rows)
    assert rel_err(lum, lref) <= 1e-12
    assert np.all(lum > 0.0)
    r0 = mesh.node_dof_row[mesh.node_dof_row >= 0]
    assert np.array_equal(lum[r0], lum[r0 + 1]) and np.array_equal(lum[r0], lum[r0 + 2])
    # each form alone gives the same bits
    only_n, none_l = ev.mass_nodal(RHO, m_node=_nan(mesh.nnz // 9))
    assert none_l is None and np.array_equal(_h(only_n), _h(m_node))
    none_n, only_l = ev.mass_nodal(RHO, m_lumped=_nan(mesh.n_rows))
    assert none_n is None and np.array_equal(_h(only_l), lum)


# ------------------------------------------------------------------------------ 5. effective tangent
@gpu
@pytest.mark.parametrize("name", ALL)
def test_effective_tangent(name):
    mesh, ev, ref = _case(name)
    cK, cM = 0.5, 3.7e3
    f, K = _nan(mesh.n_rows), _nan(mesh.nnz)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(_u(mesh)), f, K)
    K0 = _h(K)
    assert np.all(np.isfinite(K0))
    m_node, _ = ev.mass_nodal(RHO, m_node=_nan(mesh.nnz // 9))
    Mt = ev.mass(RHO)
    M = _h(Mt)
    x = np.random.default_rng(11).standard_normal(mesh.n_cols)
    xt = _t(x)
    # fused
    Kf, yf = K.clone(), _nan(mesh.n_rows)
    ev.effective_tangent(cK, cM, m_node, Kf, xt, yf)
    Ke, y = _h(Kf), _h(yf)
    bound = 2 * EPS * (np.abs(cK * K0) + np.abs(cM * M))
    assert np.all(np.abs(Ke - (cK * K0 + cM * M)) <= bound)
    assert np.array_equal(Ke[ref.offdiag], (cK * K0)[ref.offdiag])
    # cK = 0 over garbage: exactly cM M
    Kn = _nan(mesh.nnz)
    ev.effective_tangent(0.0, cM, m_node, Kn)
    assert np.array_equal(_h(Kn), cM * M)
    # y = M x against the CSR operator and the numpy reference
    ys = _nan(mesh.n_rows)
    ev.spmv(Mt, xt, ys)
    print(name, "y vs spmv", rel_err(y, _h(ys)))
    assert rel_err(y, _h(ys)) <= 1e-13
    rows = np.repeat(np.arange(mesh.n_rows), np.diff(mesh.rowptr))
    yref = np.zeros(mesh.n_rows)
    np.add.at(yref, rows, ref.vals * x[mesh.col_lid])
    assert rel_err(y, yref) <= 1e-12
    # K only, y only
    Ko = K.clone()
    ev.effective_tangent(cK, cM, m_node, Ko)
    assert np.array_equal(_h(Ko), Ke)
    yo = _nan(mesh.n_rows)
    ev.effective_tangent(cK, cM, m_node, None, xt, yo)
    assert np.array_equal(_h(yo), y)
    # twice: the same bits
    K2, y2 = K.clone(), _nan(mesh.n_rows)
    ev.effective_tangent(cK, cM, m_node, K2, xt, y2)
    assert np.array_equal(_h(K2), Ke) and np.array_equal(_h(y2), y)


# ------------------------------------------------------------------------------ 6. refusals
@gpu
def test_refusals():
    mesh, ev, ref = _case("h8_322_general")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(fcg.FcgError, match="density") as ei:
            ev.mass(bad)
        assert ei.value.code == fcg.FCG_ERR_ARG
        with pytest.raises(fcg.FcgError, match="density") as ei:
            ev.mass_nodal(bad)
        assert ei.value.code == fcg.FCG_ERR_ARG
    rho = np.full(mesh.n_ele, 2.0)
    rho[5] = 0.0
    with pytest.raises(fcg.FcgError, match=r"ele_density\[5\]") as ei:
        ev.mass(1.0, ele_density=rho)
    assert ei.value.code == fcg.FCG_ERR_ARG
    m_node, _ = ev.mass_nodal(RHO)
    with pytest.raises(fcg.FcgError, match="all NULL") as ei:
        ev.effective_tangent(1.0, 1.0, m_node)
    assert ei.value.code == fcg.FCG_ERR_ARG
    # the refusals left the context usable
    assert rel_err(_h(ev.mass(RHO)), ref.vals) <= 1e-12


@gpu
def test_extra_columns():
    """A graph with foreign columns (solver_ref.extra): the CSR mass lands on the node columns,
    the foreign ones get 0; the node forms refuse the context."""
    _dev()
    mesh = sr.extra()
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    ref = MassRef(mesh, RHO)
    M = _h(ev.mass(RHO, out=_nan(mesh.nnz)))
    assert rel_err(M, ref.vals) <= 1e-12
    assert np.all(M[ref.offdiag] == 0.0)
    for a, b in mesh.added:
        for d in range(3):
            assert M[sr.entry_pos(mesh, 3 * a + d, 3 * b + 1)] == 0.0
    rnd = np.random.default_rng(2).standard_normal(mesh.nnz)
    A = _h(ev.mass(RHO, mode=fcg.ACCUMULATE, out=_t(rnd)))
    assert rel_err(A, rnd + ref.vals) <= 1e-12 and np.array_equal(A[ref.offdiag], rnd[ref.offdiag])
    with pytest.raises(fcg.FcgError, match="DOF triple") as ei:
        ev.mass_nodal(RHO)
    assert ei.value.code == fcg.FCG_ERR_ARG
    with pytest.raises(fcg.FcgError, match="DOF triple") as ei:
        ev.effective_tangent(1.0, 1.0, _nan(mesh.nnz // 9 + 1), _nan(mesh.nnz))
    assert ei.value.code == fcg.FCG_ERR_ARG


@gpu
def test_inverted_element():
    """x -> -x turns every element inside out (test_gpu_parity's construction): the mass calls
    return FCG_ERR_NODAL_DETJ with the lowest element GID through the solver flag word; evaluate's
    own error reporting is as before."""
    dev = _dev()
    mesh = fcg.BoxMesh(fcg.HEX8, (2, 2, 2))
    mesh.node_x[:, 0] *= -1.0
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    with pytest.raises(fcg.FcgError, match="element GID 0") as ei:
        ev.mass(RHO)
    assert ei.value.code == fcg.FCG_ERR_NODAL_DETJ
    with pytest.raises(fcg.FcgError, match="element GID 0") as ei:
        ev.mass_nodal(RHO)
    assert ei.value.code == fcg.FCG_ERR_NODAL_DETJ
    ev.check_error()  # nothing pending from the mass calls
    u = torch.zeros(mesh.n_cols, dtype=torch.float64, device=dev)
    with pytest.raises(fcg.FcgError) as ei:
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, _nan(mesh.n_rows), _nan(mesh.nnz))
    assert ei.value.code == fcg.FCG_ERR_NODAL_DETJ and ei.value.bad_ele_gid == 0


# ------------------------------------------------------------------------------ 7. side effects
@gpu
@pytest.mark.parametrize("name", ["h8_322_auto", "h8_322_gather", "h8_433_general", "h27_221_general",
                                  "h27_322_lattice", "h8_433_r0_ghost", "h27_222_r1_strict"])
def test_non_interference_and_reproducibility(name):
    make, path, _ = CASES[name]
    _dev()
    mesh = make()
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU, path=path)  # no mass plan yet
    u = _t(_u(mesh))

    def evaluate():
        f, K = _nan(mesh.n_rows), _nan(mesh.nnz)
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K)
        return _h(K), _h(f)

    K0, f0 = evaluate()
    bytes0 = ev.info.device_bytes
    M1 = _h(ev.mass(RHO))
    n1, l1 = ev.mass_nodal(RHO)
    assert ev.info.device_bytes > bytes0  # the plan is counted
    bytes1 = ev.info.device_bytes
    M2 = _h(ev.mass(RHO))
    n2, l2 = ev.mass_nodal(RHO)
    assert ev.info.device_bytes == bytes1  # and built once
    assert np.array_equal(M1, M2) and np.array_equal(_h(n1), _h(n2)) and np.array_equal(_h(l1), _h(l2))
    K1, f1 = evaluate()
    assert np.array_equal(K0, K1) and np.array_equal(f0, f1)
    ev.check_error()


@gpu
def test_rank_without_rows():
    """hex8 (3,2,2) split over 16 ranks leaves rank 2 without rows: every call is a no-op."""
    _dev()
    mesh = fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1, rank=2, nranks=16)
    assert mesh.n_rows == 0
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU)
    L = fcg.lib()
    assert L.fcg_mass_assemble(ev._h, RHO, None, fcg.OVERWRITE, None, None) == fcg.FCG_OK
    assert L.fcg_mass_nodal(ev._h, RHO, None, None, None, None) == fcg.FCG_OK
    assert L.fcg_effective_tangent(ev._h, 1.0, 1.0, None, None, None, None, None) == fcg.FCG_OK
