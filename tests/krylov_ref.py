"""Host-side reference for the restarted flexible GMRES of 4c_amd/csrc/fcg_krylov.hip and the block
preconditioners of fcg_tsi_solve.hip, in numpy float64.  TEST INFRASTRUCTURE ONLY.

fgmres() restates the library's algorithm step by step -- right preconditioning from x = 0,
classical Gram-Schmidt applied twice, Givens rotations, the estimate |g_{j+1}| as the stopping test
inside a cycle, the true residual b - A x at every restart and as the answer -- without its bursts:
it stops at the first step whose estimate is at the target, so the library's iteration count may
exceed this one by less than one burst.
"""

import importlib

import numpy as np

import oracle_lib as orc

fcg = importlib.import_module("4c_amd").fcg


def csr_to_dense(rowptr, col, vals, n_cols=None):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    D = np.zeros((n, n if n_cols is None else n_cols))
    D[np.repeat(np.arange(n), np.diff(rowptr)), np.asarray(col)] = vals
    return D


def as_operator(A):
    """A dense array, a (rowptr, col, vals) triple or a callable -> callable x -> A x."""
    if callable(A):
        return A
    if isinstance(A, tuple):
        rowptr, col, vals = A
        rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(np.asarray(rowptr, dtype=np.int64)))
        col, vals, n = np.asarray(col), np.asarray(vals, dtype=np.float64), len(rowptr) - 1
        return lambda x: np.bincount(rows, weights=vals * x[col], minlength=n)
    A = np.asarray(A, dtype=np.float64)
    return lambda x: A @ x


def fgmres(A, b, restart, rtol, max_iter, precond=None):
    """Returns (x, inner steps, true relative residual, steps per cycle)."""
    op = as_operator(A)
    P = precond or (lambda r: r.copy())
    b = np.asarray(b, dtype=np.float64)
    n, m = len(b), int(restart)
    x = np.zeros(n)
    bnorm = np.linalg.norm(b)
    target = rtol * bnorm
    beta, steps, cycles = bnorm, 0, []
    r = b.copy()
    while beta > target and steps < max_iter:
        V = np.zeros((m + 1, n))
        Z = np.zeros((m, n))
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = r / beta
        g[0] = beta
        k = 0
        for j in range(m):
            if steps >= max_iter:
                break
            Z[j] = P(V[j])
            w = op(Z[j])
            h1 = V[:j + 1] @ w
            w = w - h1 @ V[:j + 1]
            h2 = V[:j + 1] @ w
            w = w - h2 @ V[:j + 1]
            h = np.append(h1 + h2, np.linalg.norm(w))
            hn = h[j + 1]
            assert np.all(np.isfinite(h)), "non-finite Hessenberg column"
            for i in range(j):
                h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], -sn[i] * h[i] + cs[i] * h[i + 1]
            rr = np.hypot(h[j], hn)
            assert rr > 0.0, "zero Hessenberg column"
            cs[j], sn[j] = h[j] / rr, hn / rr
            h[j], h[j + 1] = rr, 0.0
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            H[:j + 2, j] = h
            steps += 1
            k = j + 1
            if abs(g[j + 1]) <= target or hn == 0.0:
                break
            V[j + 1] = w / hn
        y = np.linalg.solve(np.triu(H[:k, :k]), g[:k])
        x = x + y @ Z[:k]
        r = b - op(x)
        beta = np.linalg.norm(r)
        cycles.append(k)
    return x, steps, (beta / bnorm if bnorm > 0 else 0.0), cycles


def block_jacobi(A, bs=3):
    """z = D^-1 r with D the bs x bs diagonal blocks of the dense matrix A."""
    n = A.shape[0]
    assert n % bs == 0
    inv = np.stack([np.linalg.inv(A[i:i + bs, i:i + bs]) for i in range(0, n, bs)])
    return lambda r: np.einsum("bij,bj->bi", inv, r.reshape(-1, bs)).ravel()


def tsi_precond(Kss, Kts, Ktt, bgs, struct=None):
    """The 2 x 2 block preconditioner on [r_S; r_T]: z_S = P_S r_S (nodal block Jacobi of K_SS, or
    `struct`), z_T = D_TT^-1 (r_T - [bgs] K_TS z_S) with D_TT the diagonal of K_TT."""
    ns = Kss.shape[0]
    ps = struct or block_jacobi(Kss)
    dtt = np.diag(Ktt).copy()

    def apply(r):
        zs = ps(r[:ns])
        rt = r[ns:] - (Kts @ zs if bgs else 0.0)
        return np.concatenate([zs, rt / dtt])
    return apply


def apply_dirichlet_dense(A, rows):
    """Unit rows (columns stay), as fcg_dirichlet_apply / fcg_tsi_dirichlet_apply leave them."""
    A = A.copy()
    A[rows, :] = 0.0
    A[rows, rows] = 1.0
    return A


def x0_face(celltype, iv):
    """Node indices of a BoxMesh(celltype, iv)'s x = 0 face, by the coordinates of the same box
    without jitter (same numbering)."""
    return np.nonzero(np.isclose(fcg.BoxMesh(celltype, iv).node_x[:, 0], 0.0))[0]


def oracle_tsi_blocks(mesh, u, v, T, youngs, poisson, thexpans, inittemp, conduct, dt):
    """Dense K_SS, K_ST, K_TS, K_TT, f_S, f_T of a single-rank mesh with node-consistent thermo
    numbering (thermo LID = structural LID / 3) from the CPU oracle's element routines."""
    m = orc.st_modulus(youngs, poisson, thexpans)
    ns = int(mesh.n_rows)
    nt = ns // 3
    Kss, Kst = np.zeros((ns, ns)), np.zeros((ns, nt))
    Kts, Ktt = np.zeros((nt, ns)), np.zeros((nt, nt))
    fs, fT = np.zeros(ns), np.zeros(nt)
    for en in np.asarray(mesh.ele_nodes):
        sc = (np.asarray(mesh.node_dof_col)[en][:, None] + np.arange(3)).ravel()
        tc = np.asarray(mesh.node_dof_col)[en] // 3
        Xe, Te = np.asarray(mesh.node_x)[en], T[tc]
        err, Ke, fe, Kste = orc.tsi_solid_evaluate(mesh.celltype, youngs, poisson, thexpans, inittemp,
                                                   Xe, u[sc], Te)
        assert err == 0
        err, Ktte, fTe, Ktse = orc.tsi_thermo_evaluate(mesh.celltype, conduct, m, Xe, Te, v[sc], 1.0,
                                                      1.0 / dt)
        assert err == 0
        Kss[np.ix_(sc, sc)] += Ke
        Kst[np.ix_(sc, tc)] += Kste
        Kts[np.ix_(tc, sc)] += Ktse
        Ktt[np.ix_(tc, tc)] += Ktte
        fs[sc] += fe
        fT[tc] += fTe
    return Kss, Kst, Kts, Ktt, fs, fT
