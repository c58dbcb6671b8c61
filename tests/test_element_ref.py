"""The extended-precision element reference (tests/element_ref.py) pinned on the CPU, three ways:

* against the oracle's element routine at the benign point, for both cell types, both kinematics
  and both materials: max |Ke_oracle - Ke_ref| / sum |terms| <= 128 * 2^-53 (fe: the same bound in
  units of the terms the oracle's formulation rounds);
* against itself, independently of the oracle: the reference K is the longdouble
  central-difference derivative of the reference f;
* against the oracle's material routines on a few strains.

It also pins what the other tests rely on: the shape functions against the oracle's, the mass
reference against the box volume, and the assembly against the oracle's.
"""

import importlib

import numpy as np
import pytest

import element_ref as er
import oracle_lib as orc
from parity_util import oracle_evaluate

fcg = importlib.import_module("4c_amd").fcg

LD = er.LD
needs_ld = pytest.mark.skipif(not er.EXTENDED, reason="np.longdouble has no 64-bit significand here")
E, NU = 210.0, 0.3
ORC_MAT = {er.STVK: orc.MAT_STVK, er.NEOHOOKE: orc.MAT_NEOHOOKE}
COMBOS = [(ct, k, m) for ct in (er.HEX8, er.HEX27)
          for k, m in ((er.LINEAR, er.STVK), (er.TOTLAG, er.STVK), (er.TOTLAG, er.NEOHOOKE))]


def _element(celltype, seed, jitter=0.05, amp=0.05):
    rng = np.random.default_rng(seed)
    npe = 8 if celltype == er.HEX8 else 27
    X = orc.node_param_coords(celltype) * 0.5 + jitter * rng.uniform(-1, 1, (npe, 3))
    return X, amp * rng.uniform(-1, 1, X.shape)


@pytest.mark.parametrize("celltype", [er.HEX8, er.HEX27])
def test_shape_functions(celltype):
    """Kronecker at the nodes exactly; N and dN equal the oracle's at its Gauss points and at
    random points to a few float64 roundings of values of magnitude <= 1.5."""
    P = orc.node_param_coords(celltype)
    N, dN = er.shape_ld(celltype, P)
    assert np.array_equal(N, np.eye(len(P)))
    assert np.abs(dN.sum(axis=1)).max() <= 8 * np.finfo(LD).eps
    pts = np.vstack([orc.gauss_points(celltype)[0], np.random.default_rng(1).uniform(-1, 1, (5, 3))])
    N, dN = er.shape_ld(celltype, pts)
    for g, x in enumerate(pts):
        assert np.abs(N[g] - orc.shape(celltype, x)).max() <= 8 * er.U
        assert np.abs(dN[g] - orc.shape_deriv(celltype, x)).max() <= 16 * er.U


@needs_ld
@pytest.mark.parametrize("seed", [3, 8])
@pytest.mark.parametrize("celltype,kinem,material", COMBOS)
def test_against_oracle_per_element(celltype, kinem, material, seed):
    """The oracle's Ke at the benign point lies within 128 * 2^-53 of the reference, entry by
    entry, in units of the sum of the absolute Gauss-point contributions of that entry: both
    evaluate the same sums of ngp terms, the oracle in float64 (measured here: at most 23 * 2^-53
    for hex27, 22 * 2^-53 for hex8; the bound leaves a factor of 5 for other seeds).

    fe with the same bound, in units of what the oracle's formulation rounds: for linear
    kinematics the Gauss-point contributions again; for TotLag the oracle forms E = 1/2 (F^T F - I)
    (CoupNeoHooke: C = F^T F), so E carries 2^-53 of the terms 1/2 (|F|^T |F| + I), not of |E|, and
    fe that error through |fac| |dE/du| : |CC| (in units of the contributions themselves the
    same differences measure up to 200 * 2^-53 at |E| ~ 0.05: the cancellation the regimes test
    looks at on purpose)."""
    X, u = _element(celltype, seed)
    err, Ke, fe = orc.solid_evaluate(celltype, kinem, E, NU, X, u, material=ORC_MAT[material])
    assert err == 0
    el = er.elements_ld(celltype, kinem, material, E, NU, X[None], u[None])
    assert el["detJ"].min() > 0
    eK = er.err_comp(Ke, el["Ke"][0], el["SKe"][0])
    Sf = el["Sfe"][0]
    if kinem == er.TOTLAG:
        aF = np.abs(el["F"])
        terms = (np.einsum("egki,egkj->egij", aF, aF) + er.I3x3) / 2
        FN = np.einsum("egiI,egaJ->egaiIJ", aF, np.abs(el["NX"]))
        dE = ((FN + np.swapaxes(FN, -1, -2)) / 2).reshape(1, -1, fe.size, 9)
        CE = np.einsum("egpq,egq->egp", np.abs(el["CC"]).reshape(1, -1, 9, 9), terms.reshape(1, -1, 9))
        Sf = (np.einsum("egpq,egq->egp", dE, CE) * np.abs(el["fac"])[..., None]).sum(axis=1)[0]
    ef = er.err_comp(fe, el["fe"][0], Sf)
    print(f"celltype {celltype} kinem {kinem} material {material}: K {eK / er.U:.1f} u, f {ef / er.U:.1f} u, "
          f"normwise K {er.err_norm(Ke, el['Ke'][0]):.2e} f {er.err_norm(fe, el['fe'][0]):.2e}")
    assert eK <= 128 * er.U and ef <= 128 * er.U
    assert er.err_comp(el["Ke"][0], el["Ke"][0].T, el["SKe"][0]) <= 64 * float(np.finfo(LD).eps)


@needs_ld
@pytest.mark.parametrize("celltype,kinem,material", COMBOS)
def test_tangent_is_the_derivative_of_the_force(celltype, kinem, material):
    """K_ref = d f_ref / d u by a longdouble central difference with step h = 2^-20 (9.5e-7; the
    element has size 1).  The difference is off by the truncation term h^2 / 6 |f'''| and the
    rounding term eps_LD |f| / h, eps_LD = 1.1e-19.  In units of the tangent's largest entry,
    |f'''| / |K| is at most a few hundred per unit length^2 here (every u-derivative brings one
    factor |grad N| <= 4 at element size 1/2 ... 1, CoupNeoHooke with beta = 0.75 a factor
    (beta + 2) more) and |f| / |K| is the displacement scale 0.05: truncation <= 9e-13 / 6 * 1e3 =
    1.5e-10, rounding 6e-15 times the number of terms.  The bound is 2e-10 of max |K|; measured
    1.3e-11 at most (hex27 CoupNeoHooke; hex8 7e-13), linear kinematics 7e-15 (f is linear: no
    truncation, rounding only).  A wrong term in K or f shows at O(1)."""
    X, u = _element(celltype, 5)
    el = er.elements_ld(celltype, kinem, material, E, NU, X[None], u[None])
    K = el["Ke"][0]
    h = LD(2.0) ** -20
    n = u.size
    up = np.repeat(u.astype(LD).reshape(1, -1), 2 * n, axis=0)
    up[np.arange(n), np.arange(n)] += h
    up[n + np.arange(n), np.arange(n)] -= h
    fe = er.elements_ld(celltype, kinem, material, E, NU, np.repeat(X[None], 2 * n, axis=0),
                        up.reshape(2 * n, -1, 3), want_k=False)["fe"]
    num = ((fe[:n] - fe[n:]) / (2 * h)).T   # column j = d f / d u_j
    m = float(np.abs(num - K).max() / np.abs(K).max())
    print(f"celltype {celltype} kinem {kinem} material {material}: |dK| / max|K| = {m:.2e}")
    assert m <= 2e-10


@needs_ld
@pytest.mark.parametrize("material", [er.STVK, er.NEOHOOKE])
def test_against_oracle_materials(material):
    """S and the 6 x 6 tangent of oracle_lib.stvk / oracle_lib.neohooke on a few strains, small to
    moderate: the reference's S_IJ and CC_IJKL on the Voigt pairs.  Both are short float64
    expressions (measured 7 * 2^-53 at most): the tangent within 64 * 2^-53 of its largest entry,
    the stress within 64 * 2^-53 of the abs-sum of the terms the oracle forms -- for CoupNeoHooke
    2c (I + I3^-beta |C^-1|), formed here, because the oracle's I - I3^-beta C^-1 cancels in float64
    at small strain (the reference's own scale follows its cancellation-free form and is smaller);
    StVK's stress, which does not cancel, also within 64 * 2^-53 of its own largest entry."""
    rng = np.random.default_rng(4)
    for scale in (1e-6, 1e-2, 0.3):
        A = rng.uniform(-1, 1, (3, 3))
        Eg = scale * (A + A.T) / 2
        gl = np.array([Eg[i, j] for i, j in er.VOIGT]) * np.array([1, 1, 1, 2, 2, 2.0])
        So, Co = (orc.stvk if material == er.STVK else orc.neohooke)(E, NU, gl)
        S, CC, _, S_abs, _ = er.material_ld(material, E, NU, Eg.astype(LD))
        Sv = er.voigt(S)
        Cv = np.array([[CC[i, j, k, l] for k, l in er.VOIGT] for i, j in er.VOIGT])
        if material == er.NEOHOOKE:  # the terms of the oracle's form, 2c (I - I3^-beta C^-1)
            Ci, I3 = er.inv3(er.I3x3 + 2 * Eg.astype(LD))
            S_abs = 2 * LD(E) / (4 * (1 + LD(NU))) * (er.I3x3 + I3 ** (-LD(NU) / (1 - 2 * LD(NU))) * np.abs(Ci))
        eS = float(np.abs(So - Sv).max() / np.abs(er.voigt(S_abs)).max())
        eC = float(np.abs(Co - Cv).max() / np.abs(Cv).max())
        print(f"material {material} |E| {scale:g}: S {eS / er.U:.1f} u of its terms, C {eC / er.U:.1f} u")
        assert eS <= 64 * er.U and eC <= 64 * er.U
        # the stress is not lost in the terms: relative to itself it is as good as float64 allows
        if material == er.STVK:
            assert float(np.abs(So - Sv).max() / np.abs(Sv).max()) <= 64 * er.U


@needs_ld
@pytest.mark.parametrize("celltype,iv", [(fcg.HEX8, (3, 2, 2)), (fcg.HEX27, (2, 2, 1))])
def test_assembly_and_energy(celltype, iv):
    """assemble_ld places the element entries where the oracle's Discretization::evaluate does (K
    in CSR order, f by row): the two agree to 256 * 2^-53 of the scales on a jittered box (sums of
    up to 8 elements' 8 or 27 Gauss-point terms).  The energy is the potential of f: a longdouble
    central difference of sum_e energy along a random direction d reproduces f . d.  StVK TotLag: W
    is a quartic in u; the difference's truncation h^2 / 6 D^3 W (d, d, d) measures 1.6e-8 of
    |f . d| at h = 2^-16 for this d (all DOFs moved at once), so 2.5e-13 at the h = 2^-24 used; its
    rounding eps_LD |W| / h is 1.8e-12 |W|, with |W| below |f . d|.  Bound 1e-11."""
    mesh = fcg.BoxMesh(celltype, iv, jitter=0.1)
    u = mesh.u_col(0.02)
    for kinem, material in ((er.LINEAR, er.STVK), (er.TOTLAG, er.NEOHOOKE)):
        ref = er.assemble_ld(mesh, kinem, material, E, NU, u)
        err, _, Ko, fo = oracle_evaluate(mesh, kinem, E, NU, u, material=ORC_MAT[material])
        assert err == 0 and ref.min_detJ > 0
        eK, ef = er.err_comp(Ko, ref.K, ref.SK), er.err_comp(fo, ref.f, ref.Sf)
        print(f"celltype {celltype} kinem {kinem}: assembled K {eK / er.U:.1f} u, f {ef / er.U:.1f} u")
        assert eK <= 256 * er.U and ef <= 256 * er.U
    d = np.random.default_rng(2).uniform(-1, 1, mesh.n_cols).astype(LD)
    h = LD(2.0) ** -24
    W = lambda v: er.assemble_ld(mesh, er.TOTLAG, er.STVK, E, NU, v, want_k=False)  # noqa: E731
    ul = u.astype(LD)
    num = (W(ul + h * d).el["energy"].sum() - W(ul - h * d).el["energy"].sum()) / (2 * h)
    fd = (W(ul).f * d[:mesh.n_rows]).sum()
    print("dW/dh vs f.d:", float(abs(num - fd) / abs(fd)))
    assert mesh.n_rows == mesh.n_cols and abs(num - fd) <= 1e-11 * abs(fd)


@needs_ld
@pytest.mark.parametrize("celltype,iv", [(fcg.HEX8, (3, 2, 2)), (fcg.HEX27, (2, 2, 1))])
def test_mass_reference(celltype, iv):
    """The longdouble mass of a jittered unit box sums to rho V times the rule's weight / 8
    (x rows and columns) to 1e-17, with the stiffness rule and with the mass kernels' own; the
    float64 evaluation of the same function is within 64 * 2^-53 of it entry by entry."""
    mesh = fcg.BoxMesh(celltype, iv, jitter=0.1)
    for rule in (None, er.mass_rule_full(celltype)):
        M, SM, mindet = er.mass_ld(mesh, 7.8, rule)
        w8 = np.sum(np.asarray((rule or orc.gauss_points(celltype))[1]).astype(LD)) / 8
        assert mindet > 0 and abs(float(M.sum() / 3 / LD(7.8) / w8 - 1)) <= 1e-17
        Md, _, _ = er.mass_ld(mesh, 7.8, rule, dtype=np.float64)
        assert Md.dtype == np.float64 and er.err_comp(Md, M, SM) <= 64 * er.U
        assert np.all(SM >= np.abs(M)) and (celltype == fcg.HEX27) == bool((M < 0).any())
    assert abs(float(np.sum(er.mass_rule_full(celltype)[1])) - 8.0) <= 8 * er.U * 8
