"""Extended-precision reference of the thermal boundary conditions: the face "mass" matrices of a
surface, the convection operator A and the vectors g and q on the compact layout of fcg_tsi_surface,
the per-iteration pass of fcg_tsi_convection / fcg_tsi_surface_flux, and dense host solutions of the
driver tests (a rod with a convection end, the coupled TSI Newton loop with a transient thermal field
and convection).  TEST INFRASTRUCTURE ONLY.

Built on element_ref (LD), fe_driver (quad_rule, quad_shape: the rule and shape functions of
fcg_neumann_surface, evaluated here in longdouble from the same truncated constants), tsi_ref and
thermo_ref.

    M_f,ab = sum_g w_g |dA_g| N_a N_b      m_f,a = sum_g w_g |dA_g| N_a      |dA| = |X,r x X,s|
    A = sum_f coeff_f M_f                  scale: sum_f |coeff_f| sum_g w |dA| |N_a| |N_b|
    g = sum_f coeff_f surtemp_f m_f        scale: sum_f |coeff_f surtemp_f| sum_g w |dA| |N_a|
    q = sum_f flux_f m_f                   scale: sum_f |flux_f| sum_g w |dA| |N_a|
    K' = K0 + s_c A  at s_pos              scale: |K0| + s_c |A|
    f' = f0 + s_c (A T - s_t g)            scale: |f0| + s_c sum_j |A_ij| |T_j| + s_c |s_t g_i|
    f' = f0 + s_q q                        scale: |f0| + |s_q q_i|

The float64 restatements (`*_f64`) are the same formulas written the plain way in numpy float64: what
the device results are judged beside (regimes_util.judge's criterion, with them in the oracle's place).
"""

import importlib

import numpy as np

import thermo_ref as th
import tsi_ref as tr
from element_ref import LD
from fe_driver import quad_rule, quad_shape

fcg = importlib.import_module("4c_amd").fcg


# ------------------------------------------------------------------------------ faces
def quad_tables(nfn, dtype=LD):
    """N [ngp][nfn], dN/dr, dN/ds [ngp][nfn], w [ngp] of the quad4 / quad9 rule in `dtype`."""
    xg, w = quad_rule(nfn)
    N, dr, ds = [], [], []
    for r, s in xg:
        n, dn = quad_shape(nfn, dtype(r), dtype(s))
        N.append(np.asarray(n, dtype=dtype))
        dr.append(np.asarray(dn[0], dtype=dtype))
        ds.append(np.asarray(dn[1], dtype=dtype))
    return np.array(N), np.array(dr), np.array(ds), np.asarray(w).astype(dtype)


def face_matrices(nfn, Xf, dtype=LD):
    """(M [nf][nfn][nfn], m [nf][nfn], the same sums over the absolute values aM, am, |dA| [nf][ngp])
    of the faces with node coordinates Xf [nf][nfn][3], in `dtype`."""
    N, dr, ds, w = quad_tables(nfn, dtype)
    X = np.asarray(Xf).astype(dtype)
    t1 = np.einsum("gc,fcd->fgd", dr, X)
    t2 = np.einsum("gc,fcd->fgd", ds, X)
    n = np.stack([t1[..., 1] * t2[..., 2] - t1[..., 2] * t2[..., 1],
                  t1[..., 2] * t2[..., 0] - t1[..., 0] * t2[..., 2],
                  t1[..., 0] * t2[..., 1] - t1[..., 1] * t2[..., 0]], axis=-1)
    dA = np.sqrt((n * n).sum(axis=-1))
    fac = w[None, :] * dA
    aN = np.abs(N)
    return (np.einsum("fg,ga,gb->fab", fac, N, N), np.einsum("fg,ga->fa", fac, N),
            np.einsum("fg,ga,gb->fab", fac, aN, aN), np.einsum("fg,ga->fa", fac, aN), dA)


def true_boundary_faces(mesh, single):
    """The faces of the global box's boundary (fcg.boundary_faces of the single-rank build `single` of
    the same box) all of whose nodes are column nodes of the rank `mesh`, as column node ids of `mesh`,
    found by matching node coordinates bit by bit; None when a node of the rank has no node of the
    single-rank build at its coordinates (the two builds differ)."""
    key = lambda x: np.ascontiguousarray(x, dtype=np.float64).tobytes()
    local = {key(x): n for n, x in enumerate(np.asarray(mesh.node_x))}
    everywhere = {key(x) for x in np.asarray(single.node_x)}
    if len(local) != mesh.n_node or not set(local) <= everywhere:
        return None
    faces, _ = fcg.boundary_faces(single)
    Xs = np.asarray(single.node_x)
    out = []
    for f in faces:
        ids = [local.get(key(Xs[n]), -1) for n in f]
        if min(ids) >= 0:
            out.append(ids)
    return np.asarray(out, dtype=np.int32).reshape(-1, faces.shape[1])


# ------------------------------------------------------------------------------ the compact layout
class Layout:
    """The compact layout of fcg_tsi_surface rebuilt from the faces: s_row [nsr] (owned thermo rows on a
    face, ascending), s_ptr, s_col, s_pos (position in the k_TT value array), and for the scatter
    entry[f][a][b] (compact entry of face node pair (a, b), -1 where a has no row) and row[f][a]."""

    def __init__(self, g, face_nodes):
        fn = np.asarray(face_nodes, dtype=np.int64)
        self.nf, self.nfn = fn.shape
        rows = np.asarray(g.node_dof_row_t, dtype=np.int64)[fn]
        cols = np.asarray(g.node_dof_col_t, dtype=np.int64)[fn]
        W = int(g.n_cols_t)
        owned = rows >= 0
        keys = rows[:, :, None] * W + cols[:, None, :]
        ok = np.broadcast_to(owned[:, :, None], keys.shape)
        ukeys = np.unique(keys[ok])
        self.s_row = np.unique(rows[owned])
        self.s_col = ukeys % W
        krow = ukeys // W
        self.s_ptr = np.concatenate([[0], np.cumsum([(krow == r).sum() for r in self.s_row])]).astype(np.int64)
        rp = np.asarray(g.rowptr_tt, dtype=np.int64)
        gkeys = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp)) * W + np.asarray(g.col_tt, dtype=np.int64)
        assert np.all(np.diff(gkeys) > 0)
        self.s_pos = np.searchsorted(gkeys, ukeys)
        assert np.array_equal(gkeys[self.s_pos], ukeys), "a surface entry is not in the k_TT graph"
        self.entry = np.where(ok, np.searchsorted(ukeys, np.where(ok, keys, ukeys[0] if len(ukeys) else 0)), -1)
        self.row = np.where(owned, np.searchsorted(self.s_row, np.where(owned, rows, 0)), -1)
        self.nsr, self.nse = len(self.s_row), len(self.s_col)
        self.ent_row = np.repeat(np.arange(self.nsr), np.diff(self.s_ptr))   # surface row of every entry

    def scatter_entries(self, Me):
        return tr.scatter_rect(self.nse, self.entry, Me)

    def scatter_rows(self, me):
        return tr.scatter_rows(self.nsr, self.row, me)

    def row_sum(self, vals):
        out = np.zeros(self.nsr, dtype=vals.dtype)
        np.add.at(out, self.ent_row, vals)
        return out

    def dense(self, A, n_rows, n_cols):
        D = np.zeros((int(n_rows), int(n_cols)), dtype=np.asarray(A).dtype)
        D[self.s_row[self.ent_row], self.s_col] = A
        return D

    def vector(self, v, n_rows):
        out = np.zeros(int(n_rows), dtype=np.asarray(v).dtype)
        out[self.s_row] = v
        return out


def _per_face(v, nf, dtype):
    return np.broadcast_to(np.asarray(v).astype(dtype), (nf,))


def assemble(mesh, g, face_nodes, coeff, surtemp, flux, dtype=LD):
    """dict(A, SA, g, Sg, q, Sq, layout, area, min_dA) on the compact layout in `dtype`; coeff, surtemp,
    flux: scalars or [n_faces].  area [nf]: sum_ab M_f,ab."""
    L = Layout(g, face_nodes)
    fn = np.asarray(face_nodes)
    M, m, aM, am, dA = face_matrices(L.nfn, np.asarray(mesh.node_x)[fn], dtype)
    c, t, q = (_per_face(v, L.nf, dtype) for v in (coeff, surtemp, flux))
    ct = c * t
    return dict(A=L.scatter_entries(c[:, None, None] * M), SA=L.scatter_entries(np.abs(c)[:, None, None] * aM),
                g=L.scatter_rows(ct[:, None] * m), Sg=L.scatter_rows(np.abs(ct)[:, None] * am),
                q=L.scatter_rows(q[:, None] * m), Sq=L.scatter_rows(np.abs(q)[:, None] * am),
                layout=L, area=M.sum(axis=(1, 2)), min_dA=float(dA.min()) if dA.size else 0.0, M=M, m=m)


def assemble_f64(mesh, g, face_nodes, coeff, surtemp, flux):
    return assemble(mesh, g, face_nodes, coeff, surtemp, flux, dtype=np.float64)


# ------------------------------------------------------------------------------ the per-iteration pass
def apply(L, A, gv, s_c, s_t, K0, f0, T_col, dtype=LD):
    """dict(K, SK, f, Sf) of fcg_tsi_convection in `dtype` from the float64 inputs (A, gv: the surface's
    tables; K0, f0: the evaluate's outputs; T_col: thermo column map)."""
    c = lambda a: np.asarray(a).astype(dtype)
    A, gv, K0, f0, T = c(A), c(gv), c(K0), c(f0), c(T_col)
    s_c, s_t = dtype(s_c), dtype(s_t)
    K, SK = K0.copy(), np.abs(K0)
    K[L.s_pos] += s_c * A
    SK[L.s_pos] += s_c * np.abs(A)
    f, Sf = f0.copy(), np.abs(f0)
    Tc = T[L.s_col]
    f[L.s_row] += s_c * (L.row_sum(A * Tc) - s_t * gv)
    Sf[L.s_row] += s_c * L.row_sum(np.abs(A) * np.abs(Tc)) + s_c * np.abs(s_t * gv)
    return dict(K=K, SK=SK, f=f, Sf=Sf)


def apply_f64(L, A, gv, s_c, s_t, K0, f0, T_col):
    r = apply(L, A, gv, s_c, s_t, K0, f0, T_col, dtype=np.float64)
    return r["K"], r["f"]


def flux_apply(L, qv, s_q, f0, dtype=LD):
    """(f, Sf) of fcg_tsi_surface_flux in `dtype`."""
    qv, f0 = np.asarray(qv).astype(dtype), np.asarray(f0).astype(dtype)
    f, Sf = f0.copy(), np.abs(f0)
    f[L.s_row] += dtype(s_q) * qv
    Sf[L.s_row] += np.abs(dtype(s_q) * qv)
    return f, Sf


def flux_apply_f64(L, qv, s_q, f0):
    return flux_apply(L, qv, s_q, f0, dtype=np.float64)[0]


# ------------------------------------------------------------------------------ dense host solutions
def dense_operator(mesh, g, face_nodes, coeff, surtemp, flux):
    """(A [nt][nt], g [nt], q [nt]) of a surface on a single-rank mesh, dense longdouble."""
    r = assemble(mesh, g, face_nodes, coeff, surtemp, flux)
    L, nt = r["layout"], int(g.n_rows_t)
    return L.dense(r["A"], nt, g.n_cols_t), L.vector(r["g"], nt), L.vector(r["q"], nt)


def rod_problem(celltype, iv, conduct, length=3.0, h=40.0, T0=293.0, T_inf=303.0):
    """The rod along z: (mesh, graph, faces of the end at z = L, thermo rows at z = 0, the analytic T)."""
    mesh = fcg.BoxMesh(celltype, iv, upper=(1.0, 1.0, length))
    g = fcg.TsiGraph(mesh)
    faces, _ = fcg.boundary_faces(mesh)
    z = np.asarray(mesh.node_x)[:, 2]
    end = faces[(z[faces] == z.max()).all(axis=1)]
    assert len(end) == iv[0] * iv[1] and z.max() == length and z.min() == 0.0
    dbc = np.sort(np.asarray(g.node_dof_row_t)[np.flatnonzero(z == 0.0)]).astype(np.int32)
    k, Ll = LD(conduct), LD(length)
    TL = (k * LD(T0) / Ll + LD(h) * LD(T_inf)) / (k / Ll + LD(h))
    want = np.zeros(g.n_rows_t, dtype=LD)
    want[g.node_dof_row_t] = LD(T0) + (TL - LD(T0)) * z.astype(LD) / Ll
    return dict(mesh=mesh, g=g, end=end, dbc=dbc, want=want, h=h, T0=T0, T_inf=T_inf)


def rod_dense(mesh, g, conduct, faces_conv, h, T_inf, dbc_rows, T_dbc):
    """The stationary conduction problem (K + A) T = g with T = T_dbc on dbc_rows, solved densely in
    longdouble.  Returns (T, kappa of the float64 copy of the system with its Dirichlet rows)."""
    nt = int(g.n_rows_t)
    K = th.dense(g.rowptr_tt, g.col_tt, th.conduction(mesh, g, conduct), nt)
    A, gv, _ = dense_operator(mesh, g, faces_conv, h, T_inf, 0.0)
    S, b = K + A, gv.copy()
    rows = np.asarray(dbc_rows, dtype=np.int64)
    S[rows, :] = 0
    S[rows, rows] = 1
    b[rows] = LD(T_dbc)
    return th.solve_ld(S, b), float(np.linalg.cond(S.astype(np.float64)))


def tsi_ost_conv_dense(mesh, g, E, nu, alpha, T0ref, conduct, capa, theta, dt, fext_s, fext_t, dbc_s, dbc_t, T_init,
                       nstep, Ac, gc, tol_inc=1e-13, max_iter=30):
    """thermo_ref.tsi_ost_dense with a convection condition of constant scales: the dense longdouble
    operator Ac and vector gc (dense_operator) join the thermal internal force, f_T + Ac T - gc, and its
    tangent, K_TT + Ac, before the one-step-theta combine, and f_int,n.  Returns (d, T, Newton iterations
    per step, the last stacked effective matrix)."""
    ns, nt = int(mesh.n_rows), int(g.n_rows_t)
    assert ns == mesh.n_cols and nt == g.n_cols_t
    LDc = lambda a: np.asarray(a, dtype=LD)
    fes, fet = LDc(fext_s), LDc(fext_t)
    dbc_s, dbc_t = np.asarray(dbc_s, dtype=np.int64), np.asarray(dbc_t, dtype=np.int64)
    col_of_node = np.asarray(g.node_dof_col_t)
    Cd = th.dense(g.rowptr_tt, g.col_tt, th.capacity(mesh, g, capa)[0], nt)
    thl, ldt = LD(theta), LD(dt)

    def blocks(d, v, T):
        # the float64 state the device evaluates at; the reference takes it in longdouble from there
        T64 = np.asarray(T, dtype=np.float64)
        B = tr.assemble_tsi_ld(mesh, g, E, nu, alpha, T0ref, conduct, theta, 1.0 / dt,
                               np.asarray(d, dtype=np.float64), np.asarray(v, dtype=np.float64), T64[col_of_node])
        return B, B.fT + Ac @ T64.astype(LD) - gc

    d, T = np.zeros(ns, dtype=LD), LDc(T_init).copy()
    fint_n = blocks(d, np.zeros(ns), T)[1]
    fext_n = fet
    iters, S = [], None
    for _ in range(int(nstep)):
        d_n, T_n = d.copy(), T.copy()
        hvec = (1 - thl) * (fint_n - fext_n) - thl * fet
        for it in range(max_iter):
            v = (d - d_n) / ldt
            B, fT = blocks(d, v, T)
            rs = B.fs - fes
            rt = thl * fT + Cd @ (T - T_n) / ldt + hvec
            Kss = th.dense(mesh.rowptr, mesh.col_lid, B.Kss, ns)
            Kst = th.dense(g.rowptr_st, g.col_st, B.Kst, nt)
            Kts = th.dense(g.rowptr_ts, g.col_ts, B.Kts, ns)
            Ktt = thl * (th.dense(g.rowptr_tt, g.col_tt, B.Ktt, nt) + Ac) + Cd / ldt
            S = np.block([[Kss, Kst], [Kts, Ktt]])
            b = -np.concatenate([rs, rt])
            th.apply_dirichlet(S, b, np.concatenate([dbc_s, ns + dbc_t]))
            dx = th.solve_ld(S, b)
            d, T = d + dx[:ns], T + dx[ns:]
            nx = float(np.sqrt((d ** 2).sum() + (T ** 2).sum()))
            if float(np.sqrt((dx ** 2).sum())) <= tol_inc * max(1.0, nx):
                break
        else:
            raise RuntimeError("host TSI Newton did not converge")
        iters.append(it + 1)
        fint_n = blocks(d, (d - d_n) / ldt, T)[1]
        fext_n = fet
    return d, T, iters, S
