"""Host reference of the scalar AMG's V-cycle (4c_amd/csrc/fcg_samg.hip): the cycle rebuilt in numpy
from the level matrices A_l and prolongators P_l the library reports (dense here), its lambda_max
estimates and its options -- the Chebyshev recurrence of ChebCoef in fcg_amg_shared.hpp (theta,
delta, sigma, rho), Jacobi scaling, the residual restricted by P^T, a dense inverse on the coarsest
level -- in float64 or in longdouble.  TEST INFRASTRUCTURE."""

import numpy as np

LD = np.longdouble


def csr_dense(ptr, col, vals, n_cols, dtype=np.float64):
    ptr = np.asarray(ptr, dtype=np.int64)
    n = len(ptr) - 1
    D = np.zeros((n, int(n_cols)), dtype=dtype)
    D[np.repeat(np.arange(n), np.diff(ptr)), np.asarray(col)] = np.asarray(vals).astype(dtype)
    return D


def inverse(A, dtype):
    """A^-1 in `dtype`: numpy's float64 inverse, refined by two Newton steps in longdouble."""
    X = np.linalg.inv(np.asarray(A, dtype=np.float64)).astype(dtype)
    if dtype is LD:
        A = A.astype(LD)
        I = np.eye(A.shape[0], dtype=LD)
        for _ in range(2):
            X = X + X @ (I - A @ X)
    return X


def cheb(A, dinv, b, x, lmax, nu, ratio, boost, dtype):
    """nu Chebyshev degrees in D^-1 A on A x = b; x None: from x = 0."""
    lmax = dtype(boost) * dtype(lmax)
    lmin = lmax / dtype(ratio)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    r = b if x is None else b - A @ x
    d = (r * dinv) / theta
    x = d.copy() if x is None else x + d
    for _ in range(1, nu):
        r = b - A @ x
        rho_n = 1 / (2 * sigma - rho)
        d = rho_n * rho * d + (2 * rho_n / delta) * (r * dinv)
        x = x + d
        rho = rho_n
    return x


class Cycle:
    """A[l] dense level matrices, P[l] dense prolongators (len(A) - 1 of them), lmax[l] the
    library's estimates, nu / ratio / boost its options."""

    def __init__(self, A, P, lmax, nu, ratio, boost, dtype):
        self.dtype = dtype
        self.A = [np.asarray(a).astype(dtype) for a in A]
        self.P = [np.asarray(p).astype(dtype) for p in P]
        self.dinv = [1 / np.diag(a) for a in self.A]
        self.lmax, self.nu, self.ratio, self.boost = lmax, nu, ratio, boost
        self.cinv = inverse(self.A[-1], dtype) if len(self.A) > 1 else None

    def apply(self, b, l=0):
        A, t = self.A[l], self.dtype
        b = np.asarray(b).astype(t)
        if len(self.A) == 1:
            return cheb(A, self.dinv[l], b, None, self.lmax[l], self.nu, self.ratio, self.boost, t)
        if l == len(self.A) - 1:
            return self.cinv @ b
        x = cheb(A, self.dinv[l], b, None, self.lmax[l], self.nu, self.ratio, self.boost, t)
        xc = self.apply(self.P[l].T @ (b - A @ x), l + 1)
        x = x + self.P[l] @ xc
        return cheb(A, self.dinv[l], b, x, self.lmax[l], self.nu, self.ratio, self.boost, t)

    def matrix(self):
        n = self.A[0].shape[0]
        I = np.eye(n, dtype=self.dtype)
        return np.stack([self.apply(I[:, j]) for j in range(n)], axis=1)
