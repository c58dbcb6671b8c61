"""Extended-precision reference of the thermo-structure interaction (TSI) blocks of hex8 / hex27
elements with geometrically linear kinematics, ThermoStVenantKirchhoff with a constant Young's
modulus and Fourier conduction: the element quantities of the fcg_tsi.hip header and their assembly
on a rank's TsiGraph.  TEST INFRASTRUCTURE ONLY.

Built on element_ref (shape_ld, inv3, LD, U, err_comp, err_norm, node_displacements and
assemble_ld for K_SS and the mechanical f_S).  With the oracle and the kernels it shares the Gauss
rule and the parametric node positions, nothing else.

Per element, with m = -(2 mu + 3 lambda) alpha formed in longdouble from the float64 inputs,
T_g = N.T, grad T_g = N_X T, tr(e')_g = sum_c N_c,d v_cd and fac = w det J:

    K_ST(ai,b)  = sum_g fac m N_a,i N_b
    K_TS(a,bj)  = -timefac timefac_d sum_g fac N_a T_g m N_b,j
    K_TT(a,b)   = sum_g fac (k grad N_a . grad N_b - m tr(e')_g N_a N_b)
    f_T(a)      = sum_g fac (k grad N_a . grad T_g - m tr(e')_g N_a T_g)
    f_S^th(ai)  = sum_g fac m (T_g - T_0) N_a,i

Scales: beside every quantity the same sum over the absolute values of the terms that a float64
evaluation rounds: T_g as sum_c |N_c T_c|, T_g - T_0 as that + |T_0|, grad T_g as
sum_c |N_c,d T_c|, tr(e') as sum_cd |N_c,d v_cd|, the products N_a,d N_b,d of the conduction term
one by one, the conduction and the thermoelastic term taken absolute separately.

Assembly: owned rows only, ghost nodes contribute columns, on the CSR graphs st, ts, tt of a
TsiGraph and the structural graph; a rectangular scatter (element_ref.scatter_plan is square).
"""

import numpy as np

import element_ref as er
import oracle_lib as orc
from element_ref import LD, U, err_comp, err_norm, inv3, node_displacements, shape_ld  # noqa: F401

EPS_LD = float(np.finfo(LD).eps)


def st_modulus_ld(E, nu, alpha):
    """m = -(2 mu + 3 lambda) alpha in longdouble from the float64 inputs."""
    lam, mu = er.lame(E, nu)
    return -(2 * mu + 3 * lam) * LD(alpha)


# ------------------------------------------------------------------------------ elements
def elements_tsi_ld(celltype, m, k, T0, timefac, timefac_d, X, v, T):
    """All elements at once.  X, v: [ne][npe][3]; T: [ne][npe]; m, k, T0, timefac, timefac_d
    scalars.  Returns a dict of longdouble arrays, DOF 3 a + i for the structural index:
    Kst [ne][3npe][npe], Kts [ne][npe][3npe], Ktt [ne][npe][npe], fT [ne][npe], fSth [ne][3npe],
    each with its abs-sum scale (key "S" + name), detJ [ne][ngp] at the Gauss points and
    detJ_node [ne][npe] at the nodes."""
    xi, w = orc.gauss_points(celltype)
    N, dN = shape_ld(celltype, xi)
    w = np.asarray(w, dtype=LD)
    X, v, T = (np.asarray(a, dtype=LD) for a in (X, v, T))
    m, k, T0 = LD(m), LD(k), LD(T0)
    tf = LD(timefac) * LD(timefac_d)
    ne, npe = X.shape[:2]
    J = np.einsum("gad,eak->egdk", dN, X)
    Ji, detJ = inv3(J)
    NX = np.einsum("egkd,gad->egak", Ji, dN)                  # grad_X N_a  [e][g][a][k]
    _, dNn = shape_ld(celltype, orc.node_param_coords(celltype))
    _, detJn = inv3(np.einsum("gad,eak->egdk", dNn, X))
    fac, aN, aNX = w[None, :] * detJ, np.abs(N), np.abs(NX)
    afac = np.abs(fac)
    Tg = np.einsum("gc,ec->eg", N, T)
    Tg_abs = np.einsum("gc,ec->eg", aN, np.abs(T))
    dT, dT_abs = Tg - T0, Tg_abs + abs(T0)
    gT = np.einsum("egcd,ec->egd", NX, T)
    gT_abs = np.einsum("egcd,ec->egd", aNX, np.abs(T))
    tr = np.einsum("egcd,ecd->eg", NX, v)
    tr_abs = np.einsum("egcd,ecd->eg", aNX, np.abs(v))
    out = dict(detJ=detJ, detJ_node=detJn, fac=fac)
    # K_ST
    out["Kst"] = (m * np.einsum("eg,egai,gb->eaib", fac, NX, N)).reshape(ne, 3 * npe, npe)
    out["SKst"] = (abs(m) * np.einsum("eg,egai,gb->eaib", afac, aNX, aN)).reshape(ne, 3 * npe, npe)
    # K_TS
    out["Kts"] = (-tf * m * np.einsum("eg,ga,eg,egbj->eabj", fac, N, Tg, NX)).reshape(ne, npe, 3 * npe)
    out["SKts"] = (abs(tf * m) * np.einsum("eg,ga,eg,egbj->eabj", afac, aN, Tg_abs, aNX)
                   ).reshape(ne, npe, 3 * npe)
    # K_TT
    out["Ktt"] = (k * np.einsum("eg,egad,egbd->eab", fac, NX, NX)
                  - m * np.einsum("eg,eg,ga,gb->eab", fac, tr, N, N))
    out["SKtt"] = (abs(k) * np.einsum("eg,egad,egbd->eab", afac, aNX, aNX)
                   + abs(m) * np.einsum("eg,eg,ga,gb->eab", afac, tr_abs, aN, aN))
    # f_T
    out["fT"] = (k * np.einsum("eg,egad,egd->ea", fac, NX, gT)
                 - m * np.einsum("eg,eg,ga,eg->ea", fac, tr, N, Tg))
    out["SfT"] = (abs(k) * np.einsum("eg,egad,egd->ea", afac, aNX, gT_abs)
                  + abs(m) * np.einsum("eg,eg,ga,eg->ea", afac, tr_abs, aN, Tg_abs))
    # f_S, thermal part
    out["fSth"] = (m * np.einsum("eg,eg,egai->eai", fac, dT, NX)).reshape(ne, 3 * npe)
    out["SfSth"] = (abs(m) * np.einsum("eg,eg,egai->eai", afac, dT_abs, aNX)).reshape(ne, 3 * npe)
    return out


# ------------------------------------------------------------------------------ assembly
def rect_positions(rowptr, col, rows, cols):
    """pos [ne][nr][nc]: the position in the CSR value array (rowptr, col) of the entry
    (rows[e][p], cols[e][q]); -1 where rows[e][p] < 0 (a node without a row).  Every other
    entry must be in the graph."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    width = int(max(col.max(initial=0), cols.max(initial=0))) + 1
    key = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr)) * width + col
    assert np.all(np.diff(key) > 0), "CSR columns are not sorted within their rows"
    want = rows[:, :, None] * width + cols[:, None, :]
    ok = np.broadcast_to(rows[:, :, None] >= 0, want.shape)
    pos = np.searchsorted(key, np.where(ok, want, 0))
    assert np.array_equal(key[np.minimum(pos, len(key) - 1)][ok], want[ok]), "entry not in the graph"
    return np.where(ok, pos, -1)


def scatter_rect(nnz, pos, Ke):
    K = np.zeros(int(nnz), dtype=Ke.dtype)
    ok = pos >= 0
    np.add.at(K, pos[ok], Ke[ok])
    return K


def scatter_rows(n, rows, fe):
    f = np.zeros(int(n), dtype=fe.dtype)
    ok = rows >= 0
    np.add.at(f, rows[ok], fe[ok])
    return f


class TsiAssembled:
    """assemble_tsi_ld's result: Kss, Kst, Kts, Ktt (the graphs' CSR order), fs (mechanical +
    thermal), fT, every one with its scale ("S" + name), the element dict `el`, and the smallest
    det J at the Gauss points and at the nodes."""

    NAMES = ("Kss", "Kst", "Kts", "Ktt", "fs", "fT")

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.min_detJ = float(self.el["detJ"].min())
        self.min_detJ_node = float(self.el["detJ_node"].min())

    def pairs(self):
        """name -> (reference, scale)"""
        return {k: (getattr(self, k), getattr(self, "S" + k)) for k in self.NAMES}


def assemble_tsi_ld(mesh, g, E, nu, alpha, T0, conduct, timefac, timefac_d, u_col, v_col, T_node):
    """The four blocks and both residuals of a BoxMesh rank or a Discretization `mesh` with its
    TsiGraph `g` in longdouble.  u_col, v_col: structural column map; T_node: nodal temperatures
    in the node order of the mesh."""
    en = np.asarray(mesh.ele_nodes)
    ne, npe = en.shape
    X = np.asarray(mesh.node_x)[en]
    v = node_displacements(mesh, v_col)[en]
    T = np.asarray(T_node)[en]
    el = elements_tsi_ld(mesh.celltype, st_modulus_ld(E, nu, alpha), conduct, T0, timefac,
                         timefac_d, X, v, T)
    mech = er.assemble_ld(mesh, er.LINEAR, er.STVK, E, nu, u_col)
    d3 = np.arange(3)
    ndr, ndc = np.asarray(mesh.node_dof_row), np.asarray(mesh.node_dof_col)
    rows_s = np.where(ndr[en][:, :, None] >= 0, ndr[en][:, :, None] + d3, -1).reshape(ne, 3 * npe)
    cols_s = (ndc[en][:, :, None] + d3).reshape(ne, 3 * npe)
    rows_t = np.asarray(g.node_dof_row_t)[en]
    cols_t = np.asarray(g.node_dof_col_t)[en]
    p_st = rect_positions(g.rowptr_st, g.col_st, rows_s, cols_t)
    p_ts = rect_positions(g.rowptr_ts, g.col_ts, rows_t, cols_s)
    p_tt = rect_positions(g.rowptr_tt, g.col_tt, rows_t, cols_t)
    out = dict(el=el, Kss=mech.K, SKss=mech.SK)
    for name, nnz, pos in (("Kst", g.nnz_st, p_st), ("Kts", g.nnz_ts, p_ts), ("Ktt", g.nnz_tt, p_tt)):
        out[name] = scatter_rect(nnz, pos, el[name])
        out["S" + name] = scatter_rect(nnz, pos, el["S" + name])
    out["fs"] = mech.f + scatter_rows(mesh.n_rows, rows_s, el["fSth"])
    out["Sfs"] = mech.Sf + scatter_rows(mesh.n_rows, rows_s, el["SfSth"])
    out["fT"] = scatter_rows(g.n_rows_t, rows_t, el["fT"])
    out["SfT"] = scatter_rows(g.n_rows_t, rows_t, el["SfT"])
    return TsiAssembled(**out)


def smooth_fields(mesh, T_mean=293.0, amp_u=1e-3, amp_v=1e-2, amp_T=50.0, scale=1.0):
    """(u_col, v_col, nodal T) as smooth functions of the node position X / scale alone, so that
    every numbering and every rank split of one geometry sees the same state: u is the field of
    BoxMesh.node_displacement, v and T those of test_tsi.py's _fields_xyz."""
    X = np.asarray(mesh.node_x) / np.asarray(scale, dtype=np.float64)
    ndc = np.asarray(mesh.node_dof_col)
    un = amp_u * np.stack([np.sin(2 * np.pi * X[:, 0]) * np.cos(np.pi * X[:, 1]),
                           np.sin(np.pi * X[:, 1]) * np.cos(2 * np.pi * X[:, 2]),
                           np.sin(2 * np.pi * X[:, 2]) * np.cos(np.pi * X[:, 0])], axis=1)
    vn = amp_v * np.stack([np.cos(3 * X[:, 0] + X[:, 1]), np.sin(2 * X[:, 1] - X[:, 2]),
                           np.cos(X[:, 0] * X[:, 2])], axis=1)
    u, v = np.zeros(mesh.n_cols), np.zeros(mesh.n_cols)
    for d in range(3):
        u[ndc + d], v[ndc + d] = un[:, d], vn[:, d]
    Tn = T_mean + amp_T * (np.sin(2 * np.pi * X[:, 0]) * np.cos(np.pi * X[:, 1]) + 0.2 * X[:, 2])
    return u, v, Tn


def oracle_view(mesh):
    """What parity_util.oracle_tsi_evaluate reads, for a single-rank Discretization as for a
    BoxMesh rank (DOF LID = GID, node GID = index)."""
    if hasattr(mesh, "row_gid"):
        return mesh
    m = type("SingleRank", (), {})()
    m.row_gid = m.col_gid = np.arange(mesh.n_cols, dtype=np.int32)
    for key in ("nnz", "n_rows", "n_cols", "rowptr", "col_lid", "celltype", "n_ele", "ele_nodes",
                "n_node", "node_x", "node_dof_row", "node_dof_col"):
        setattr(m, key, getattr(mesh, key))
    m.node_gid = np.arange(mesh.n_node, dtype=np.int64)
    return m
