"""Extended-precision reference of the transient thermal field: the capacity matrix of the thermo
element, the one-step-theta combine of fcg_tsi_ost_combine, and dense host steppings of one-step-theta
conduction and of the coupled TSI Newton loop with a transient thermal field.  TEST INFRASTRUCTURE ONLY.

Built on element_ref (shape_ld, det3, LD), oracle_lib.gauss_points (the rule K_TT is integrated with)
and tsi_ref (rect_positions, scatter_rect, elements_tsi_ld, assemble_tsi_ld).

    C_ab  = sum_e sum_g capa_e w_g det J_g N_a N_b        scale: the same sum over |.|
    K_j  <- theta K_j + C_j / dt                          scale: theta |K_j| + |C_j| / dt
    f_i  <- theta f_i + sum_j C_ij (T_j - Tn_j) / dt + h_i
                                                          scale: sum_j |C_ij| |T_j - Tn_j| / dt + theta |f_i| + |h_i|

The float64 restatements (`*_f64`) are the same formulas written the plain way in numpy float64: what
the device results are judged beside (regimes_util.judge's criterion, with them in the oracle's place).
"""

import functools
import importlib

import numpy as np

import element_ref as er
import oracle_lib as orc
import tsi_ref as tr
from element_ref import LD

fcg = importlib.import_module("4c_amd").fcg

# ------------------------------------------------------------------------------ the meshes of the GPU tests
MAT = dict(youngs=210.0, poisson=0.3, thexpans=1.2e-5, inittemp=293.0, conduct=52.0)
# mesh name -> (cell type, intervals, rank, nranks, renumbered)
MESHES = {"h8": (fcg.HEX8, (3, 3, 3), 0, 1, False), "h8r": (fcg.HEX8, (3, 3, 3), 0, 1, True),
          "h27": (fcg.HEX27, (2, 2, 2), 0, 1, False),
          "h27_rank0": (fcg.HEX27, (2, 2, 4), 0, 2, False), "h27_rank1": (fcg.HEX27, (2, 2, 4), 1, 2, False)}
REGIMES = {"A": {}, "D_1e4_rotated": dict(lower=(1e4, -2e4, 3e4), rotation=(0.3, 0.5, 0.7)),
           "H_thin": dict(size=(1.0, 1.0, 1e-3)), "micro": dict(edge=3e-5)}


@functools.lru_cache(maxsize=None)
def mesh_of(name, regime="A"):
    celltype, iv, rank, nranks, renumbered = MESHES[name]
    p = dict(lower=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0), rotation=(0.0, 0.0, 0.0), edge=None)
    p.update(REGIMES[regime])
    if p["edge"] is not None:
        p["size"] = tuple(p["edge"] * n for n in iv)
    upper = tuple(lo + s for lo, s in zip(p["lower"], p["size"]))
    box = fcg.BoxMesh(celltype, iv, lower=p["lower"], upper=upper, rotation=p["rotation"], jitter=0.1,
                      rank=rank, nranks=nranks)
    mesh = fcg.Discretization.renumbered(box, seed=3) if renumbered else box
    g = fcg.TsiGraph(mesh)
    rows = np.diff(g.rowptr_tt)
    assert rows.max() == (27 if celltype == fcg.HEX8 else 125)
    if nranks > 1:
        assert (np.asarray(mesh.node_dof_row) < 0).any()
    return mesh, g


# ------------------------------------------------------------------------------ capacity
def element_capacity(celltype, X, dtype=LD):
    """[ne][npe][npe] sum_g w detJ N_a N_b (unit capacity), the same sum over the absolute values,
    and detJ [ne][ngp], in `dtype`."""
    xi, w = orc.gauss_points(celltype)
    N, dN = er.shape_ld(celltype, xi)
    N, dN, w = N.astype(dtype), dN.astype(dtype), np.asarray(w).astype(dtype)
    J = np.einsum("gad,eak->egdk", dN, np.asarray(X).astype(dtype))
    detJ = er.det3(J)
    fac = w[None, :] * detJ
    return (np.einsum("eg,ga,gb->eab", fac, N, N),
            np.einsum("eg,ga,gb->eab", np.abs(fac), np.abs(N), np.abs(N)), detJ)


def tt_positions(mesh, g):
    en = np.asarray(mesh.ele_nodes)
    return tr.rect_positions(g.rowptr_tt, g.col_tt, np.asarray(g.node_dof_row_t)[en],
                             np.asarray(g.node_dof_col_t)[en])


def capacity(mesh, g, capa, dtype=LD):
    """(C, SC, min detJ) on the k_TT graph of `g` in `dtype`: owned rows, ghost elements contribute.
    capa: a scalar or [n_ele]."""
    en = np.asarray(mesh.ele_nodes)
    ce, ca, detJ = element_capacity(mesh.celltype, np.asarray(mesh.node_x)[en], dtype)
    capa = np.broadcast_to(np.asarray(capa).astype(dtype), (len(en),))[:, None, None]
    pos = tt_positions(mesh, g)
    return (tr.scatter_rect(g.nnz_tt, pos, ce * capa), tr.scatter_rect(g.nnz_tt, pos, ca * np.abs(capa)),
            float(detJ.min()))


def capacity_f64(mesh, g, capa):
    return capacity(mesh, g, capa, dtype=np.float64)[0]


def conduction(mesh, g, k, dtype=LD):
    """K_TT of pure conduction (v = 0) on the k_TT graph, longdouble."""
    en = np.asarray(mesh.ele_nodes)
    X = np.asarray(mesh.node_x)[en]
    el = tr.elements_tsi_ld(mesh.celltype, 0.0, k, 0.0, 1.0, 1.0, X, np.zeros_like(X), np.zeros(en.shape))
    return tr.scatter_rect(g.nnz_tt, tt_positions(mesh, g), el["Ktt"])


# ------------------------------------------------------------------------------ the combine
def _row_sum(rowptr, vals, n):
    out = np.zeros(n, dtype=vals.dtype)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rowptr)))
    np.add.at(out, rows, vals)
    return out


def combine(g, theta, dt, C, T_col, Tn_col, h, K, f, dtype=LD):
    """dict(K, SK, f, Sf) of the one-step-theta pass in `dtype` from the float64 inputs."""
    c = lambda a: np.asarray(a).astype(dtype)
    C, T, Tn, K, f = c(C), c(T_col), c(Tn_col), c(K), c(f)
    h = np.zeros_like(f) if h is None else c(h)
    theta, dt = dtype(theta), dtype(dt)
    col = np.asarray(g.col_tt)
    n = int(g.n_rows_t)
    dT = T[col] - Tn[col]
    return dict(K=theta * K + C / dt, SK=theta * np.abs(K) + np.abs(C) / dt,
                f=theta * f + _row_sum(g.rowptr_tt, C * dT, n) / dt + h,
                Sf=_row_sum(g.rowptr_tt, np.abs(C) * np.abs(dT), n) / dt + theta * np.abs(f) + np.abs(h))


def combine_f64(g, theta, dt, C, T_col, Tn_col, h, K, f):
    r = combine(g, theta, dt, C, T_col, Tn_col, h, K, f, dtype=np.float64)
    return r["K"], r["f"]


# ------------------------------------------------------------------------------ dense host stepping
def dense(rowptr, col, vals, ncols):
    rowptr = np.asarray(rowptr)
    A = np.zeros((len(rowptr) - 1, int(ncols)), dtype=np.asarray(vals).dtype)
    A[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), np.asarray(col)] = vals
    return A


def solve_ld(A, b):
    """A x = b in longdouble: a float64 solve refined with longdouble residuals until the
    correction no longer shrinks (the float64 solve contracts by cond(A) eps each pass)."""
    A, b = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)
    # row equilibration keeps the float64 copy representable across unit Dirichlet rows and stiff ones
    s = np.abs(A).max(axis=1)
    A, b = A / s[:, None], b / s
    A64 = A.astype(np.float64)
    x = np.zeros_like(b)
    last = np.inf
    for _ in range(12):
        r = b - A @ x
        nr = float(np.abs(r).max())
        if nr == 0 or nr >= last:
            break
        last = nr
        x = x + np.linalg.solve(A64, r.astype(np.float64)).astype(LD)
    return x


def apply_dirichlet(A, b, rows):
    if len(rows):
        A[rows, :] = 0
        A[rows, rows] = 1
        b[rows] = 0


def ost_dense(K, C, theta, dt, T0, fext, dbc, nstep):
    """nstep one-step-theta steps of the linear conduction problem (dense longdouble K, C; f_int = K T)
    from T0; fext: t -> vector or a vector; dbc: rows that keep their T0 values.  Returns [nstep + 1][n]."""
    K, C = np.asarray(K, dtype=LD), np.asarray(C, dtype=LD)
    theta, dt = LD(theta), LD(dt)
    load = (lambda t: np.asarray(fext(t), dtype=LD)) if callable(fext) else (lambda t: np.asarray(fext, dtype=LD))
    dbc = np.asarray(dbc, dtype=np.int64)
    T = [np.asarray(T0, dtype=LD)]
    A = C / dt + theta * K
    apply_dirichlet(A, np.zeros(len(A), dtype=LD), dbc)
    for n in range(int(nstep)):
        Tn = T[-1]
        r = theta * (K @ Tn - load((n + 1) * float(dt))) + (1 - theta) * (K @ Tn - load(n * float(dt)))
        b = -r
        b[dbc] = 0
        T.append(Tn + solve_ld(A, b))
    return np.array(T)


def tsi_ost_dense(mesh, g, E, nu, alpha, T0ref, conduct, capa, theta, dt, fext_s, fext_t, dbc_s, dbc_t, T_init,
                  nstep, tol_inc=1e-13, max_iter=30):
    """The coupled Newton loop of tsi.TsiMonolithic(thermal="ost") on one rank in dense longdouble: the
    blocks of tsi_ref.assemble_tsi_ld with timefac = theta, timefac_d = 1 / dt and v = (d - d_n)/dt, the
    thermal rows combined as above.  Constant loads.  Returns (d, T, Newton iterations per step,
    the last stacked effective matrix)."""
    ns, nt = int(mesh.n_rows), int(g.n_rows_t)
    assert ns == mesh.n_cols and nt == g.n_cols_t
    LDc = lambda a: np.asarray(a, dtype=LD)
    fes, fet = LDc(fext_s), LDc(fext_t)
    dbc_s, dbc_t = np.asarray(dbc_s, dtype=np.int64), np.asarray(dbc_t, dtype=np.int64)
    col_of_node = np.asarray(g.node_dof_col_t)
    Cd = dense(g.rowptr_tt, g.col_tt, capacity(mesh, g, capa)[0], nt)
    th, ldt = LD(theta), LD(dt)

    def blocks(d, v, T):
        # the float64 state the device evaluates at; the reference takes it in longdouble from there
        return tr.assemble_tsi_ld(mesh, g, E, nu, alpha, T0ref, conduct, theta, 1.0 / dt,
                                  np.asarray(d, dtype=np.float64), np.asarray(v, dtype=np.float64),
                                  np.asarray(T, dtype=np.float64)[col_of_node])

    d, T = np.zeros(ns, dtype=LD), LDc(T_init).copy()
    fint_n = blocks(d, np.zeros(ns), T).fT
    fext_n = fet
    iters, A = [], None
    for _ in range(int(nstep)):
        d_n, T_n = d.copy(), T.copy()
        h = (1 - th) * (fint_n - fext_n) - th * fet
        for it in range(max_iter):
            v = (d - d_n) / ldt
            B = blocks(d, v, T)
            rs = B.fs - fes
            rt = th * B.fT + Cd @ (T - T_n) / ldt + h
            Kss = dense(mesh.rowptr, mesh.col_lid, B.Kss, ns)
            Kst = dense(g.rowptr_st, g.col_st, B.Kst, nt)
            Kts = dense(g.rowptr_ts, g.col_ts, B.Kts, ns)
            Ktt = th * dense(g.rowptr_tt, g.col_tt, B.Ktt, nt) + Cd / ldt
            A = np.block([[Kss, Kst], [Kts, Ktt]])
            b = -np.concatenate([rs, rt])
            apply_dirichlet(A, b, np.concatenate([dbc_s, ns + dbc_t]))
            dx = solve_ld(A, b)
            d, T = d + dx[:ns], T + dx[ns:]
            nx = float(np.sqrt((d ** 2).sum() + (T ** 2).sum()))
            if float(np.sqrt((dx ** 2).sum())) <= tol_inc * max(1.0, nx):
                break
        else:
            raise RuntimeError("host TSI Newton did not converge")
        iters.append(it + 1)
        fint_n = blocks(d, (d - d_n) / ldt, T).fT
        fext_n = fet
    return d, T, iters, A
