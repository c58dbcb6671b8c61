"""Host reference of the geometric multigrid (4c_amd/multigrid.py): the trilinear prolongation
derived from the node coordinates, the level operators assembled by element_ref in longdouble, the
V-/W-cycle of CycleFCG._vcycle rebuilt from dense level matrices, and the flexible CG around it, in
float64 or in longdouble.  TEST INFRASTRUCTURE ONLY.

Prolongation.  Nothing here reads node GIDs or calls multigrid.node_lattice / transfer_tables.  The
box's affine frame is taken from the coarse mesh's element 0: with the parametric corner positions p
(entries -1, 1) of oracle_lib.node_param_coords the edge vectors are h_d = sum_a p_ad X_a / 4, and
t = (X - X_0) H^-1 is a point's coordinate in coarse element edges, shifted so that the box's low
corner is 0.  Every fine node's t is solved in longdouble.  The node coordinates themselves are
float64 (rotated boxes carry their rounding, 1e-16), so t is then snapped to the lattice it is
checked to lie on: along each axis the fine nodes take N_f distinct values, the f-th of them must be
f (N_c - 1) / (N_f - 1) to 1e-9, and that quotient, formed in longdouble, is the coordinate the 1-D
hat functions are evaluated at.  The weight of coarse node c is the product of the three hats.  A
jittered mesh is replaced by its unjittered twin (same box, same numbering): the solver's transfers
ignore the jitter, "a preconditioner only".

Cycle.  Chebyshev in D^-1 S (D^-1 the 3 x 3 nodal block inverses handed in, S the smoother's
operator, which mixed=True rounds to float32) on A x = b, the residual b - A x restricted by R,
the coarse correction added through P, nu / coarse_nu degrees, one or ("W", below the fine level)
two coarse corrections, no fine post-smoothing when fine_post is False, a dense inverse on the
coarsest level.  R and P are taken as given (the masks already applied)."""

import importlib

import numpy as np

import element_ref as er
import oracle_lib as orc
import samg_ref
import solver_ref as sr
from samg_ref import LD

fcg = importlib.import_module("4c_amd").fcg


# ---------------------------------------------------------------------------------- geometry
def plain(mesh):
    """The mesh itself, or its unjittered twin (same box, same numbering)."""
    b = mesh.box
    if float(b.jitter) == 0.0:
        return mesh
    return fcg.BoxMesh(mesh.celltype, tuple(int(b.interval[d]) for d in range(3)),
                       lower=tuple(b.lower[d] for d in range(3)), upper=tuple(b.upper[d] for d in range(3)),
                       rotation=tuple(b.rotation[d] for d in range(3)), first_node_gid=int(b.first_node_gid))


def frame(mesh):
    """(X_0, H^-1) of the mesh's element 0 in longdouble: the node at p = (-1, -1, -1) and the
    inverse of the matrix whose rows are the element's edge vectors."""
    p = np.asarray(orc.node_param_coords(mesh.celltype))
    corner = np.all(np.abs(p) == 1, axis=1)
    assert corner.sum() == 8
    X = np.asarray(mesh.node_x)[np.asarray(mesh.ele_nodes)[0][corner]].astype(LD)
    pc = p[corner].astype(LD)
    H = (pc.T @ X) / 4
    return X[np.all(pc == -1, axis=1)][0], er.inv3(H)[0]


def edge_coords(mesh, ref):
    """(t [n_node][3], n [3]): the mesh's nodes in units of ref's element edges from the low corner
    of ref's box, and ref's interval counts, all from node coordinates."""
    o, Hi = frame(ref)
    tr = (np.asarray(ref.node_x).astype(LD) - o) @ Hi
    lo = np.rint(tr.min(axis=0))
    n = np.rint(tr.max(axis=0) - lo).astype(np.int64)
    return (np.asarray(mesh.node_x).astype(LD) - o) @ Hi - lo, n


def _snap(t, n):
    """Lattice index of every value of t (one axis, in [0, n]) among its distinct values, and their
    number; the values must be equispaced to 1e-9."""
    key = np.rint(t.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    uniq, idx = np.unique(key, return_inverse=True)
    idx = idx.ravel()
    m = len(uniq) - 1
    assert m >= 1
    c = idx.astype(LD) * LD(int(n)) / LD(m)
    assert float(np.abs(c - t).max()) <= 1e-9 * max(1, int(n)), "nodes off the lattice"
    return idx, m, c


def face_mask(mesh, axis=0, side=0):
    """Nodes on the low (side 0) or high (side 1) lattice face across `axis`, from coordinates."""
    m = plain(mesh)
    t, n = edge_coords(m, m)
    idx, cnt, _ = _snap(t[:, axis], n[axis])
    return idx == (0 if side == 0 else cnt)


def prolongation(fine, coarse):
    """Dense trilinear P [fine.n_rows][coarse.n_rows] in longdouble (identity 3 x 3 blocks)."""
    fine, coarse = plain(fine), plain(coarse)
    tf, nc = edge_coords(fine, coarse)
    tc, _ = edge_coords(coarse, coarse)
    ic = np.rint(tc).astype(np.int64)
    assert float(np.abs(tc - ic).max()) <= 1e-9
    assert (ic.min(axis=0) == 0).all() and (ic.max(axis=0) == nc).all()
    cnode = np.full(tuple(nc + 1), -1, dtype=np.int64)
    cnode[ic[:, 0], ic[:, 1], ic[:, 2]] = np.arange(len(ic))
    assert (cnode >= 0).all()
    lo, wt = [], []
    for d in range(3):
        _, _, c = _snap(tf[:, d], nc[d])
        i0 = np.minimum(np.floor(c).astype(np.int64), nc[d] - 1)
        lo.append(i0)
        wt.append(c - i0)
    frow, crow = np.asarray(fine.node_dof_row), np.asarray(coarse.node_dof_row)
    P = np.zeros((fine.n_rows, coarse.n_rows), dtype=LD)
    for a in range(len(frow)):
        if frow[a] < 0:
            continue
        for cx in range(2):
            for cy in range(2):
                for cz in range(2):
                    w = LD(1)
                    for d, cc in enumerate((cx, cy, cz)):
                        w = w * (wt[d][a] if cc else 1 - wt[d][a])
                    if w == 0:
                        continue
                    cn = cnode[lo[0][a] + cx, lo[1][a] + cy, lo[2][a] + cz]
                    for k in range(3):
                        P[frow[a] + k, crow[cn] + k] += w
    return P


def tables_dense(tab, n_out, n_in):
    """A transfer table (ptr, src_row0, w, dst_row0) of multigrid.transfer_tables as a dense
    float64 matrix [n_out][n_in]."""
    ptr, src, w, dst = tab
    D = np.zeros((n_out, n_in))
    for o in range(len(dst)):
        if dst[o] < 0:
            continue
        for j in range(ptr[o], ptr[o + 1]):
            for k in range(3):
                D[dst[o] + k, src[j] + k] += w[j]
    return D


def mask_of(mesh, rows):
    m = np.ones(mesh.n_rows)
    m[np.asarray(rows, dtype=np.int64)] = 0.0
    return m


def node_rows(mesh, nodes):
    """Row LIDs (int32, ascending) of all three DOFs of the nodes marked in the mask `nodes`."""
    ndr = np.asarray(mesh.node_dof_row)
    sel = np.nonzero(np.asarray(nodes) & (ndr >= 0))[0]
    return np.sort((ndr[sel][:, None] + np.arange(3)).ravel()).astype(np.int32)


# ---------------------------------------------------------------------------------- operators
def level_operator(mesh, E, nu, rows, kinem=er.LINEAR, u_col=None):
    """(A, SK) dense longdouble [n_rows][n_cols]: element_ref's StVK tangent of the mesh at u_col
    (default 0) with the rows `rows` replaced by unit rows (columns stay, as dirichlet_kernel and
    box_stencil_kernel leave them), and the abs-sum scale of every entry (unit rows: the 1)."""
    u = np.zeros(mesh.n_cols) if u_col is None else np.asarray(u_col)
    a = er.assemble_ld(mesh, kinem, er.STVK, E, nu, u)
    K = sr.apply_dirichlet_host(mesh, a.K, rows)
    SK = sr.apply_dirichlet_host(mesh, a.SK, rows)
    return (samg_ref.csr_dense(mesh.rowptr, mesh.col_lid, K, mesh.n_cols, LD),
            samg_ref.csr_dense(mesh.rowptr, mesh.col_lid, SK, mesh.n_cols, LD))


def pattern(mesh):
    """Boolean [n_rows][n_cols]: the entries of the mesh's CSR graph."""
    return samg_ref.csr_dense(mesh.rowptr, mesh.col_lid, np.ones(mesh.nnz), mesh.n_cols) != 0


def diag_blocks(A):
    """[n / 3][3][3] nodal diagonal blocks of a dense matrix whose rows come in node triples."""
    n = A.shape[0] // 3
    return np.stack([A[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(n)])


def block_inverses(A, dtype):
    """Inverses of diag_blocks(A) in `dtype` (cofactors)."""
    return er.inv3(diag_blocks(np.asarray(A)).astype(dtype))[0]


# ---------------------------------------------------------------------------------- the cycle
def block_apply(dinv, r):
    """D^-1 r for a vector r [n] or the columns of r [n][m]."""
    return np.einsum("kdc,kc...->kd...", dinv, r.reshape((-1, 3) + r.shape[1:])).reshape(r.shape)


def cheb(S, dinv, b, x, lmax, nu, ratio, boost, dtype):
    """nu Chebyshev degrees in D^-1 S on S x = b (CycleFCG._cheb); x None: from x = 0.  With
    lambda in [lmin, lmax] = boost lmax [1 / ratio, 1], theta the interval's centre and delta its
    half width, the degree-k iterate's error polynomial is T_k((theta - lambda) / delta) /
    T_k(theta / delta); the three-term recurrence of T_k gives, with sigma = theta / delta and
    rho_0 = 1 / sigma, rho_k = 1 / (2 sigma - rho_{k-1}),
        d_0 = D^-1 r / theta,   d_k = rho_k rho_{k-1} d_{k-1} + (2 rho_k / delta) D^-1 r."""
    lmax = dtype(boost) * dtype(lmax)
    lmin = lmax / dtype(ratio)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    r = b if x is None else b - S @ x
    d = block_apply(dinv, r) / theta
    x = d.copy() if x is None else x + d
    for _ in range(1, nu):
        r = b - S @ x
        rho_n = 1 / (2 * sigma - rho)
        d = (rho_n * rho) * d + (2 * rho_n / delta) * block_apply(dinv, r)
        x = x + d
        rho = rho_n
    return x


class Cycle:
    """A[l]: dense level operators (the residual's); S: the smoother's operators (None: A; for
    mixed, S[0] is K rounded to float32); P[l], R[l]: dense masked prolongation and restriction
    (len(A) - 1 of each); dinv[l]: [n_l / 3][3][3] block inverses (the coarsest level's unused);
    lmax[l] per level; cinv: the coarsest inverse (None: samg_ref.inverse of A[-1])."""

    def __init__(self, A, P, R, dinv, lmax, nu, ratio, boost, dtype, S=None, coarse_nu=None,
                 fine_post=True, cycle="V", cinv=None):
        t = self.dtype = dtype
        self.A = [np.asarray(a).astype(t) for a in A]
        self.S = self.A if S is None else [np.asarray(s).astype(t) for s in S]
        self.P = [np.asarray(p).astype(t) for p in P]
        self.R = [np.asarray(r).astype(t) for r in R]
        self.dinv = [None if d is None else np.asarray(d).reshape(-1, 3, 3).astype(t) for d in dinv]
        self.lmax, self.nu, self.ratio, self.boost = lmax, nu, ratio, boost
        self.coarse_nu, self.fine_post, self.cycle = coarse_nu, fine_post, cycle
        self.cinv = samg_ref.inverse(self.A[-1], t) if cinv is None else np.asarray(cinv).astype(t)

    def _cheb(self, l, b, x):
        nu = self.nu if l == 0 or self.coarse_nu is None else self.coarse_nu
        return cheb(self.S[l], self.dinv[l], b, x, self.lmax[l], nu, self.ratio, self.boost, self.dtype)

    def apply(self, b, l=0):
        b = np.asarray(b).astype(self.dtype)
        if l == len(self.A) - 1:
            return self.cinv @ b
        x = self._cheb(l, b, None)
        for _ in range(2 if l > 0 and self.cycle == "W" else 1):
            x = x + self.P[l] @ self.apply(self.R[l] @ (b - self.A[l] @ x), l + 1)
        if l > 0 or self.fine_post:
            x = self._cheb(l, b, x)
        return x

    def matrix(self, cols=None):
        n = self.A[0].shape[0]
        cols = np.arange(n) if cols is None else np.asarray(cols)
        return self.apply(np.eye(n, dtype=self.dtype)[:, cols])


def fcg_replay(A, cycle, b, rtol, max_iter, dtype):
    """CycleFCG._fcg on the host in `dtype`: flexible CG from x = 0 preconditioned by
    cycle.apply, Polak-Ribiere beta = (r.z - z.r_old) / (r.z)_old.  Returns (x, iterations,
    history of the recurrence residual |r| / |b| after every iteration)."""
    A = np.asarray(A).astype(dtype)
    b = np.asarray(b).astype(dtype)
    bn = np.sqrt(b @ b)
    x = np.zeros_like(b)
    r = b.copy()
    z = cycle.apply(r).astype(dtype)
    p = z.copy()
    rz = r @ z
    hist, it = [], 0
    while it < max_iter:
        it += 1
        q = A @ p
        alpha = rz / (p @ q)
        x = x + alpha * p
        r_old = r
        r = r - alpha * q
        z = cycle.apply(r).astype(dtype)
        hist.append(float(np.sqrt(r @ r) / bn))
        if hist[-1] <= rtol:
            break
        rz_new = r @ z
        p = ((rz_new - z @ r_old) / rz) * p + z
        rz = rz_new
    return x, it, hist
