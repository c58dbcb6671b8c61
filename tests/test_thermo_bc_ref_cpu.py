"""thermo_bc_ref.py against things it shares no code with: the areas the face matrices sum to, the
symmetry and the row sums of the convection operator, and the closed form of a rod with a convection
end.

Areas.  The shape functions of a face sum to 1, so sum_ab M_f,ab = sum_g w_g |dA_g|.  On an axis-aligned
box |dA| = x'(r) y'(s) and the Gauss points are symmetric, so a face integrates to its area times
(sum of the 1D weights / 2)^2 whatever the float64 roundings of its mid nodes are, and the faces of a
side telescope to the side's extent: the six sides sum to the box's surface times that factor, which is
1 for quad4 and (1 + 0.5e-13)^2 for the 13-digit constants of quad9, up to the longdouble roundings
of the sum (one eps per added term).

The rod.  Conduction k along a rod of length L with T = T_0 at 0, a convection end (h, T_inf) at L and
adiabatic sides has the linear field T(z) = T_0 + (T_L - T_0) z / L with
T_L = (k T_0 / L + h T_inf) / (k / L + h); linear and quadratic elements hold it exactly -- in exact
arithmetic.  The tables of both rules are float64 products of the 13-digit constants, so the pattern
of the conduction flux at the end (the volume rule's w_i w_j w_k) and the one of the convection (the
face rule's w_i w_j) agree to a float64 rounding only, and the dense longdouble solution of the hex27
rod sits that far, amplified by the system's condition, from the closed form: 1.5e-14 of T_L - T_0.
With T_inf - T_0 = 10 K on T_0 = 293 K that is 3.5e-16 of max |T|, inside the 1e-15 asked of it (a
difference of 50 K on 300 K gave 1.6e-15)."""

import importlib

import numpy as np
import pytest

import thermo_bc_ref as bc
import thermo_ref as th
from element_ref import EXTENDED, LD

fcg = importlib.import_module("4c_amd").fcg

pytestmark = pytest.mark.skipif(not EXTENDED, reason="np.longdouble has no 64-bit significand here")

EPS_LD = float(np.finfo(LD).eps)
COND = 52.0
BOXES = [(fcg.HEX8, (3, 3, 3)), (fcg.HEX27, (2, 2, 2))]


def _weight_factor(nfn):
    """(sum of the rule's 1D weights / 2)^2 in longdouble."""
    if nfn == 4:
        return LD(1)
    return ((2 * LD(0.5555555555556) + LD(0.8888888888889)) / 2) ** 2


def _surface(mesh):
    X = np.asarray(mesh.node_x).astype(LD)
    ext = X.max(axis=0) - X.min(axis=0)
    return 2 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0])


@pytest.mark.parametrize("celltype,iv", BOXES)
def test_faces_sum_to_their_areas(celltype, iv):
    mesh = fcg.BoxMesh(celltype, iv)          # the unjittered unit box
    g = fcg.TsiGraph(mesh)
    faces, face_ele = fcg.boundary_faces(mesh)
    nfn = faces.shape[1]
    assert len(faces) == 2 * (iv[0] * iv[1] + iv[1] * iv[2] + iv[2] * iv[0])
    en = np.asarray(mesh.ele_nodes)
    assert all(set(f) <= set(en[e]) for f, e in zip(faces, face_ele))            # a face of its element
    r = bc.assemble(mesh, g, faces, 1.0, 0.0, 0.0)
    assert r["A"].dtype == LD and r["min_dA"] > 0
    terms = nfn * nfn * nfn
    wf = _weight_factor(nfn)
    X = np.asarray(mesh.node_x).astype(LD)[faces]
    ext = X.max(axis=1) - X.min(axis=1)       # one extent of an axis-aligned face is 0
    area = np.sort(ext, axis=1)[:, 1] * np.sort(ext, axis=1)[:, 2]
    assert float(np.abs(r["area"] - wf * area).max()) <= terms * EPS_LD * float(area.max())
    total = r["area"].sum()
    assert abs(float(total - wf * 6)) <= len(faces) * terms * EPS_LD * 6
    assert abs(float(total) - 6.0) <= 6 * 1.1e-13


@pytest.mark.parametrize("celltype,iv", BOXES)
def test_thin_box(celltype, iv):
    mesh = fcg.BoxMesh(celltype, iv, upper=th.REGIMES["H_thin"]["size"])
    g = fcg.TsiGraph(mesh)
    faces, _ = fcg.boundary_faces(mesh)
    nfn = faces.shape[1]
    total = bc.assemble(mesh, g, faces, 1.0, 0.0, 0.0)["area"].sum()
    want = _surface(mesh)
    assert abs(float(want) - (2 + 4e-3)) <= 4 * 2.0 ** -52      # the float64 of 1e-3
    assert abs(float(total - _weight_factor(nfn) * want)) <= len(faces) * nfn ** 3 * EPS_LD * float(want)


@pytest.mark.parametrize("celltype,iv", BOXES)
def test_operator_is_symmetric_with_the_row_sums_of_m(celltype, iv):
    mesh = fcg.BoxMesh(celltype, iv, jitter=0.1)
    g = fcg.TsiGraph(mesh)
    faces, _ = fcg.boundary_faces(mesh)
    coeff = np.where(np.arange(len(faces)) % 3 == 0, 12.5, 7.25 * 12.5)
    surtemp = 300.0 + 5.0 * (np.arange(len(faces)) % 4)
    flux = np.where(np.arange(len(faces)) % 2 == 0, 30.0, -4.0)
    r = bc.assemble(mesh, g, faces, coeff, surtemp, flux)
    L = r["layout"]
    nt = g.n_rows_t
    Ad = L.dense(r["A"], nt, g.n_cols_t)
    assert float(np.abs(Ad - Ad.T).max()) <= 8 * EPS_LD * float(np.abs(Ad).max())
    assert (r["SA"] >= np.abs(r["A"])).all() and (r["Sg"] >= np.abs(r["g"])).all() and (r["Sq"] >= np.abs(r["q"])).all()
    # sum_b M_f,ab = m_f,a: the rows of A sum to sum_f coeff_f m_f
    cm = L.scatter_rows(coeff.astype(LD)[:, None] * r["m"])
    assert float((np.abs(L.row_sum(r["A"]) - cm) / L.row_sum(r["SA"])).max()) <= 64 * EPS_LD
    # g and q with uniform surtemp / flux are multiples of that vector
    u = bc.assemble(mesh, g, faces, coeff, 300.0, 0.0)
    assert float((np.abs(u["g"] - 300 * cm) / u["Sg"]).max()) <= 8 * EPS_LD
    # the float64 restatement is the reference rounded, to a few units of float64
    r64 = bc.assemble_f64(mesh, g, faces, coeff, surtemp, flux)
    for k in ("A", "g", "q"):
        assert r64[k].dtype == np.float64
        assert float((np.abs(r64[k] - r[k]) / r["S" + k]).max()) <= 64 * 2.0 ** -53
    # the layout: rows ascending, columns ascending inside a row, positions name the entry of the graph
    assert np.all(np.diff(L.s_row) > 0)
    for i in range(L.nsr):
        c = L.s_col[L.s_ptr[i]:L.s_ptr[i + 1]]
        assert np.all(np.diff(c) > 0)
    assert np.array_equal(np.asarray(g.col_tt)[L.s_pos], L.s_col)
    rows_tt = np.repeat(np.arange(nt), np.diff(g.rowptr_tt))
    assert np.array_equal(rows_tt[L.s_pos], L.s_row[L.ent_row])


ROD_BOXES = [(fcg.HEX8, (2, 2, 6)), (fcg.HEX27, (1, 1, 3))]


@pytest.mark.parametrize("celltype,iv", ROD_BOXES)
def test_rod_with_a_convection_end(celltype, iv):
    P = bc.rod_problem(celltype, iv, COND)
    T, kappa = bc.rod_dense(P["mesh"], P["g"], COND, P["end"], P["h"], P["T_inf"], P["dbc"], P["T0"])
    err = float(np.abs(T - P["want"]).max() / np.abs(P["want"]).max())
    rise = float(P["want"].max()) - P["T0"]
    print(f"rod {iv}: dense longdouble against the closed form {err:.3e} of max|T|, "
          f"{err * float(P['want'].max()) / rise:.3e} of T_L - T_0, kappa {kappa:.3e}")
    assert err <= 1e-15
    assert float(P["want"].max()) > P["T0"] + 1.0       # the end is warmer: the convection acts
