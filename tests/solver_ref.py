"""Host-side references for the solver primitives of 4c_amd/csrc/fcg_solver.hip (the CSR operator,
Dirichlet rows, block Jacobi, the Chebyshev step, block-Jacobi PCG) in extended precision, and the
small meshes tests/test_solver_primitives.py runs them on.  TEST INFRASTRUCTURE ONLY.

Precision: np.longdouble with a 64-bit significand (x86 extended, eps 1.08e-19) where numpy has it
-- every float64 and float32 converts exactly, a product of two doubles is rounded to 64 bits, so a
reference sum of n terms is off by about n 2^-64 of sum |terms|, 2^-11 of the float64 bounds the
tests hold the kernels to.  Where longdouble is float64 (EXTENDED False) the component-wise
references (csr_matvec_ld, block_inverse_ld) are computed exactly in fractions.Fraction and rounded
once; the longdouble PCG replay then has no more digits than the float64 one and is refused.
"""

import importlib
from fractions import Fraction

import numpy as np

fcg = importlib.import_module("4c_amd").fcg

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63
U = 2.0 ** -53  # unit roundoff of float64


# ---------------------------------------------------------------------------------- references
def _rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def csr_matvec_ld(rowptr, col, vals, x):
    """(y, absy) = (K x, |K| |x|) of a CSR matrix, both longdouble.  vals may be float32 or
    float64 (converted exactly); rows without entries give 0."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col)
    n = len(rowptr) - 1
    rows = _rows_of(rowptr)
    if EXTENDED:
        prod = np.asarray(vals).astype(LD) * np.asarray(x).astype(LD)[col]
        y, absy = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
        np.add.at(y, rows, prod)
        np.add.at(absy, rows, np.abs(prod))
        return y, absy
    y, absy = [Fraction(0)] * n, [Fraction(0)] * n
    for r, c, v in zip(rows.tolist(), col.tolist(), np.asarray(vals).astype(np.float64).tolist()):
        t = Fraction(v) * Fraction(float(x[c]))
        y[r] += t
        absy[r] += abs(t)
    return np.array([float(t) for t in y], dtype=LD), np.array([float(t) for t in absy], dtype=LD)


def row_nodes(mesh):
    """(row0, col0) of the mesh's row nodes in ascending row order -- the order of the library's
    row nodes (fcg_create): first row LID and first column LID of each node's DOF triple."""
    ndr = np.asarray(mesh.node_dof_row)
    nodes = np.nonzero(ndr >= 0)[0]
    nodes = nodes[np.argsort(ndr[nodes], kind="stable")]
    return ndr[nodes].astype(np.int64), np.asarray(mesh.node_dof_col)[nodes].astype(np.int64)


def entry_pos(mesh, row, colid):
    """Position in the CSR value array of entry (row, colid), found by column id; -1 if absent."""
    s, e = int(mesh.rowptr[row]), int(mesh.rowptr[row + 1])
    j = s + int(np.searchsorted(mesh.col_lid[s:e], colid))
    return j if j < e and mesh.col_lid[j] == colid else -1


def diag_block_positions(mesh):
    """[n_rownodes][3][3] positions of every row node's own 3 x 3 block (row row0 + d, column
    col0 + c), picked by column id; -1 where the graph has no such entry."""
    row0, col0 = row_nodes(mesh)
    pos = np.full((len(row0), 3, 3), -1, dtype=np.int64)
    for k in range(len(row0)):
        for d in range(3):
            for c in range(3):
                pos[k, d, c] = entry_pos(mesh, row0[k] + d, col0[k] + c)
    return pos


def _adjugate_inverse(D):
    """Inverse of [n][3][3] blocks by the adjugate in D's dtype; zeros where det == 0."""
    a, b, c = D[:, 0, 0], D[:, 0, 1], D[:, 0, 2]
    d, e, f = D[:, 1, 0], D[:, 1, 1], D[:, 1, 2]
    g, h, i = D[:, 2, 0], D[:, 2, 1], D[:, 2, 2]
    adj = np.empty_like(D)
    adj[:, 0, 0], adj[:, 0, 1], adj[:, 0, 2] = e * i - f * h, c * h - b * i, b * f - c * e
    adj[:, 1, 0], adj[:, 1, 1], adj[:, 1, 2] = f * g - d * i, a * i - c * g, c * d - a * f
    adj[:, 2, 0], adj[:, 2, 1], adj[:, 2, 2] = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * adj[:, 0, 0] + b * adj[:, 1, 0] + c * adj[:, 2, 0]
    ok = det != 0
    inv = np.zeros_like(D)
    inv[ok] = adj[ok] / det[ok][:, None, None]
    return inv, ok


def block_inverse_ld(mesh, vals):
    """The 3 x 3 diagonal blocks of the CSR values `vals` on mesh's graph, picked by column id:
    (D, Dinv, kappa, ok) -- blocks and inverses longdouble [n][3][3], kappa = |D|_inf |D^-1|_inf
    (inf for a singular or incomplete block, whose inverse is returned as zeros)."""
    pos = diag_block_positions(mesh)
    v = np.asarray(vals, dtype=np.float64)
    D = np.where(pos >= 0, v[np.maximum(pos, 0)], 0.0).astype(LD)
    complete = (pos >= 0).all(axis=(1, 2))
    if EXTENDED:
        inv, ok = _adjugate_inverse(D)
    else:
        inv, ok = np.zeros_like(D), np.zeros(len(D), dtype=bool)
        for k in range(len(D)):
            F = [[Fraction(float(t)) for t in r] for r in D[k]]
            cof = lambda r, c: (F[(r + 1) % 3][(c + 1) % 3] * F[(r + 2) % 3][(c + 2) % 3]
                                - F[(r + 1) % 3][(c + 2) % 3] * F[(r + 2) % 3][(c + 1) % 3])
            det = sum(F[0][c] * cof(0, c) for c in range(3))
            if det != 0:
                ok[k] = True
                inv[k] = [[float(cof(c, r) / det) for c in range(3)] for r in range(3)]
    ok &= complete
    inv[~ok] = 0
    ninf = lambda M: np.abs(M).sum(axis=2).max(axis=1)
    kappa = np.where(ok, (ninf(D) * ninf(inv)).astype(np.float64), np.inf)
    return D, inv, kappa, ok


def cofactor_inverse_f64(D):
    """float64 replay of block_jacobi_kernel's cofactor formula (same products and differences,
    each rounded once, no fused multiply-add): row-major inverses [n][9] of the blocks D [n][3][3]."""
    D = np.asarray(D, dtype=np.float64)
    m = [D[:, q % 3, q // 3] for q in range(9)]  # column-major, m[d + 3 c] = D[d][c]
    c00 = m[4] * m[8] - m[7] * m[5]
    c01 = m[7] * m[2] - m[1] * m[8]
    c02 = m[1] * m[5] - m[4] * m[2]
    det = m[0] * c00 + m[3] * c01 + m[6] * c02
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = 1.0 / det
        o = np.stack([c00 * rd, (m[6] * m[5] - m[3] * m[8]) * rd, (m[3] * m[7] - m[6] * m[4]) * rd,
                      c01 * rd, (m[0] * m[8] - m[6] * m[2]) * rd, (m[6] * m[1] - m[0] * m[7]) * rd,
                      c02 * rd, (m[3] * m[2] - m[0] * m[5]) * rd, (m[0] * m[4] - m[3] * m[1]) * rd],
                     axis=1)
    o[~((det != 0) & np.isfinite(det))] = 0.0
    return o


def block_apply(dinv, row0, r, dtype=LD):
    """z[row0[k] + d] = sum_c dinv[k][d][c] r[row0[k] + c] in `dtype`; other rows 0."""
    dinv = np.asarray(dinv).reshape(-1, 3, 3).astype(dtype)
    idx = np.asarray(row0)[:, None] + np.arange(3)
    z = np.zeros(len(r), dtype=dtype)
    z[idx] = np.einsum("kdc,kc->kd", dinv, np.asarray(r).astype(dtype)[idx])
    return z


def apply_dirichlet_host(mesh, vals, rows):
    """A copy of the CSR values with the rows `rows` replaced by unit rows."""
    out = np.array(vals, copy=True)
    own = col_of_row(mesh)
    for r in np.asarray(rows).tolist():
        out[mesh.rowptr[r]:mesh.rowptr[r + 1]] = 0
        out[entry_pos(mesh, r, int(own[r]))] = 1
    return out


def col_of_row(mesh):
    """Column LID of every row's own DOF (-1 for a row no node owns)."""
    row0, col0 = row_nodes(mesh)
    c = np.full(mesh.n_rows, -1, dtype=np.int64)
    for d in range(3):
        c[row0 + d] = col0 + d
    return c


def _matvec(rowptr, col, vals, x):
    prod = vals * x[col]
    if np.all(np.diff(rowptr) > 0):
        return np.add.reduceat(prod, rowptr[:-1])
    y = np.zeros(len(rowptr) - 1, dtype=vals.dtype)
    np.add.at(y, _rows_of(rowptr), prod)
    return y


def pcg_replay(mesh, vals, b, dinv, rtol, max_iter, dtype=np.float64, check_every=8):
    """fcg_pcg_solve's iteration on the host in `dtype`: block-Jacobi PCG from x = 0 with the
    kernel's recurrences (alpha = rz / p.Kp, beta = rz_new / rz, the recurrence residual r.r
    compared with rtol^2 b.b after every burst of `check_every` iterations).  dinv: [n][3][3]
    inverses of the row nodes' blocks.  float64: what double arithmetic does in the library's
    order of operations but numpy's order of summation; longdouble: the truth for a fixed
    iteration count.  Returns (x, iterations, recurrence |r|/|b|, true |b - K x|/|b|)."""
    if dtype == LD and not EXTENDED:
        raise RuntimeError("the longdouble PCG replay needs a 64-bit significand")
    rowptr = np.asarray(mesh.rowptr, dtype=np.int64)
    col = np.asarray(mesh.col_lid)
    K = np.asarray(vals).astype(dtype)
    b = np.asarray(b).astype(dtype)
    row0, _ = row_nodes(mesh)
    x = np.zeros_like(b)
    r = b.copy()
    z = block_apply(dinv, row0, r, dtype)
    p = z.copy()
    rz, rr0 = r @ z, r @ r
    rr, it = rr0, 0
    if rr0 == 0:
        return x, 0, 0.0, 0.0
    target = dtype(rtol) * dtype(rtol) * rr0
    while it < max_iter and rr > target:
        for _ in range(min(check_every, max_iter - it)):
            q = _matvec(rowptr, col, K, p)
            pq = p @ q
            alpha = rz / pq if pq > 0 else dtype(0)
            x += alpha * p
            r -= alpha * q
            z = block_apply(dinv, row0, r, dtype)
            rzn, rr = r @ z, r @ r
            beta = rzn / rz if rz != 0 else dtype(0)
            rz = rzn
            p = z + beta * p
            it += 1
    return x, it, float(np.sqrt(rr / rr0)), true_residual(mesh, vals, b, x)


def true_residual(mesh, vals, b, x):
    """|b - K x|_2 / |b|_2 in longdouble."""
    y, _ = csr_matvec_ld(mesh.rowptr, mesh.col_lid, vals, x)
    bl = np.asarray(b).astype(LD)
    return float(np.sqrt(((bl - y) ** 2).sum() / (bl ** 2).sum()))


def random_values(mesh, seed):
    """Seeded standard-normal values on the mesh's graph with + 4 on the diagonal of every row
    node's own 3 x 3 block: all entries distinct, nothing symmetric."""
    v = np.random.default_rng(seed).standard_normal(mesh.nnz)
    pos = diag_block_positions(mesh)
    for d in range(3):
        p = pos[:, d, d]
        v[p[p >= 0]] += 4.0
    return v


# -------------------------------------------------------------------------------------- meshes
def h8box():
    """60 row nodes (not a multiple of the 16 a workgroup takes), rows 24 .. 81 long."""
    m = fcg.BoxMesh(fcg.HEX8, (4, 3, 2), jitter=0.1)
    m.face_nodes = _box_face(fcg.HEX8, (4, 3, 2), m)
    return m


def h27box():
    """125 row nodes, rows 81 .. 375 long (the centre row: two passes of the 64-lane x 3 stride)."""
    m = fcg.BoxMesh(fcg.HEX27, (2, 2, 2), jitter=0.02)
    m.face_nodes = _box_face(fcg.HEX27, (2, 2, 2), m)
    return m


def h8rank(strict=False):
    """Rank 1 of 2: more columns than rows, ghost columns (strict: extended rows as well)."""
    m = fcg.BoxMesh(fcg.HEX8, (4, 3, 4), rank=1, nranks=2, strict=strict)
    owned = np.asarray(m.node_dof_row) >= 0
    m.face_nodes = np.nonzero(np.isclose(m.node_x[:, 0], m.node_x[owned, 0].max()) & owned)[0]
    return m


def _box_face(celltype, iv, m):
    plain = fcg.BoxMesh(celltype, iv)  # same numbering, no jitter: the x = 0 face by coordinate
    return np.nonzero(np.isclose(plain.node_x[:, 0], 0.0) & (np.asarray(m.node_dof_row) >= 0))[0]


def h8renum():
    """h8box in input-file numbering (random node and element numbers, no lattice hint)."""
    box = h8box()
    m = fcg.Discretization.renumbered(box, seed=3)
    m.face_nodes = np.sort(m.node_perm[box.face_nodes])
    return m


def fan(layers=1, jitter=0.03, seed=11):
    """Five hex8 per layer around an axis: a regular pentagon (centre C, corners V_i, edge
    midpoints M_i) cut into the quads (C, M_{i-1}, V_i, M_i), extruded `layers` layers.  One layer:
    the axis nodes have 5 elements and all 22 nodes as neighbours (rows of 66), the others rows of
    24 and 36; two layers: the middle axis node has 33 neighbours, more than a hex8 row holds."""
    ang = 2 * np.pi * np.arange(5) / 5
    V = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    M = 0.5 * (V + np.roll(V, -1, axis=0))  # M_i between V_i and V_{i+1}
    plane = np.vstack([[0.0, 0.0], V, M])   # C = 0, V_i = 1 + i, M_i = 6 + i
    X = np.vstack([np.column_stack([plane, np.full(11, 0.8 * l)]) for l in range(layers + 1)])
    X = X + jitter * np.random.default_rng(seed).uniform(-1, 1, X.shape)
    quads = [(0, 6 + (i - 1) % 5, 1 + i, 6 + i) for i in range(5)]
    en = [[11 * l + q for q in quad] + [11 * (l + 1) + q for q in quad]
          for l in range(layers) for quad in quads]
    m = fcg.Discretization.from_elements(fcg.HEX8, np.array(en), X)
    side = np.array([1, 6, 2])  # V_0, M_0, V_1: one outer side face
    m.face_nodes = np.sort(np.concatenate([side + 11 * l for l in range(layers + 1)]))
    return m


def extra():
    """h8renum's graph with a foreign column: for three corner nodes a (rows of 24) the single
    column 3 b + 1 of a node b that is no neighbour of a, sorted into all three rows of a -- rows
    that are not made of node DOF triples only."""
    base = h8renum()
    rp, cl = base.rowptr, base.col_lid
    lens = rp[1::3] - rp[0:-1:3]
    corners = np.nonzero(lens == 24)[0][:3]
    rows, cols = [0], []
    added = []
    for r in range(base.n_rows):
        c = cl[rp[r]:rp[r + 1]].tolist()
        a = r // 3
        if a in corners:
            nbrs = set(x // 3 for x in c)
            b = next(n for n in range(base.n_node - 1, -1, -1) if n not in nbrs)
            c = sorted(c + [3 * b + 1])
            if r % 3 == 0:
                added.append((a, b))
        cols.extend(c)
        rows.append(len(cols))
    m = fcg.Discretization(fcg.HEX8, base.ele_nodes, base.node_x, base.node_dof_col,
                           base.node_dof_row, np.array(rows), np.array(cols))
    m.face_nodes, m.added = base.face_nodes, added
    return m


def orphan():
    """h8box's arrays plus one node no element holds: its three rows are empty (no diagonal)."""
    box = h8box()
    nn = box.n_node
    X = np.vstack([box.node_x, [[2.0, 2.0, 2.0]]])
    dof = np.concatenate([box.node_dof_col, [3 * nn]]).astype(np.int32)
    assert np.array_equal(box.node_dof_col, 3 * np.arange(nn)) and box.n_rows == 3 * nn
    rowptr = np.concatenate([box.rowptr, [box.rowptr[-1]] * 3])
    m = fcg.Discretization(fcg.HEX8, box.ele_nodes, X, dof, dof, rowptr, np.array(box.col_lid))
    m.face_nodes, m.orphan_row0 = box.face_nodes, 3 * nn
    return m


def dirichlet_rows(mesh, seed=5):
    """One clamped face (mesh.face_nodes, all three DOFs), rollers (one DOF each of four other
    owned nodes) and the middle DOF of one more free node, as shuffled distinct row LIDs (int32)."""
    ndr = np.asarray(mesh.node_dof_row)
    rng = np.random.default_rng(seed)
    face = np.asarray(mesh.face_nodes)
    others = np.setdiff1d(np.nonzero((ndr >= 0) & (np.diff(mesh.rowptr)[np.maximum(ndr, 0)] > 0))[0], face)
    pick = rng.choice(others, size=5, replace=False)
    rows = np.concatenate([(ndr[face][:, None] + np.arange(3)).ravel(),
                           ndr[pick] + np.array([0, 2, 1, 0, 1])])
    assert len(np.unique(rows)) == len(rows)
    return rng.permutation(rows).astype(np.int32)
