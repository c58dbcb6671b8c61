"""Extended-precision reference of the SOLID element evaluate (hex8 / hex27, linear or total
Lagrangian kinematics, St.Venant-Kirchhoff or ElastHyper/CoupNeoHooke): K and f_int assembled on a
discretization's CSR graph, the Gauss-point stresses, strains and strain energy, and the consistent
mass.  TEST INFRASTRUCTURE ONLY.

Precision: np.longdouble with a 64-bit significand (x86 extended, eps 1.08e-19), as in solver_ref;
where longdouble is float64 (EXTENDED False) the reference has no more digits than what it judges
and the tests that need it skip.

What the reference shares with the oracle and the kernels is the input data only: the parametric
node positions (oracle_lib.node_param_coords, entries -1, 0, 1) and the Gauss rule
(oracle_lib.gauss_points, the same doubles the kernels use).  The shape functions are products of
1-D linear or quadratic Lagrange polynomials on those positions, evaluated in longdouble, so no node
ordering is typed in here.  The element formulas are written with tensors, not in Voigt notation:

    H = u^T grad_X N,  F = I + H (TotLag; F = I in dE for linear kinematics)
    E = 1/2 (H + H^T + H^T H)  (TotLag; the products of F^T F - I written out, so that a state
        with |H| ~ 1e-8 keeps its digits)  or  sym H (linear)
    dE_IJ / du_ai = sym(F_iI N_a,J)
    f_ai   = sum_g w detJ  dE/du_ai : S
    K_aibk = sum_g w detJ (dE/du_ai : CC : dE/du_bk  +  delta_ik N_a,I S_IJ N_b,J)   (geometric: TotLag)
    StVK:          S = lambda tr(E) I + 2 mu E,  CC = lambda dd + mu (dd + dd)
    CoupNeoHooke:  S = 2c (I - I3^-beta C^-1),   CC = 4 c beta I3^-beta C^-1 x C^-1 + 4 c I3^-beta C^-1 . C^-1
                   c = E / (4 (1 + nu)), beta = nu / (1 - 2 nu), C = I + 2 E, I3 = det C

For CoupNeoHooke I3 - 1 is formed from the invariants of 2E (no 1 + x - 1), I3^-beta - 1 as
expm1(-beta log1p(I3 - 1)) and S as 2c (2E - (I3^-beta - 1) I) C^-1: the same function, without
the cancellation of I - I3^-beta C^-1 near the undeformed state.

Scales: beside every assembled sum the reference returns the same sum over the absolute values of
the Gauss-point contributions (SK, Sf; the abs-sums of the terms of each Gauss-point quantity): the
magnitude that the rounding errors of any evaluation of the sum are proportional to.
"""

import numpy as np

import oracle_lib as orc

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63
U = 2.0 ** -53  # unit roundoff of float64

HEX8, HEX27 = 0, 1
LINEAR, TOTLAG = 0, 1
STVK, NEOHOOKE = 0, 1
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))  # xx yy zz xy yz xz
I3x3 = np.eye(3, dtype=LD)


# ------------------------------------------------------------------------------ shape functions
def _lagrange_1d(order, p, r):
    """(l, dl/dr) of the 1-D Lagrange polynomial of the node at p (-1, 0 or 1) at the points r:
    linear on {-1, 1} (order 1) or quadratic on {-1, 0, 1} (order 2).  p [npe], r [ng] -> [ng][npe]."""
    p = np.asarray(p, dtype=LD)[None, :]
    r = np.asarray(r, dtype=LD)[:, None]
    half = LD(1) / LD(2)
    if order == 1:
        return half * (1 + p * r), half * p + 0 * r
    end = half * r * (r + p), r + half * p      # p = +-1: r (r + p) / 2
    mid = 1 - r * r, -2 * r                     # p = 0
    return np.where(p == 0, mid[0], end[0]), np.where(p == 0, mid[1], end[1])


def shape_ld(celltype, xi):
    """N [ng][npe] and dN/dxi [ng][npe][3] at the points xi [ng][3] (doubles, converted exactly)."""
    P = orc.node_param_coords(celltype)
    assert set(np.unique(P).tolist()) <= {-1.0, 0.0, 1.0}
    order = 1 if celltype == HEX8 else 2
    xi = np.asarray(xi, dtype=np.float64).reshape(-1, 3)
    l, dl = zip(*[_lagrange_1d(order, P[:, d], xi[:, d]) for d in range(3)])
    N = l[0] * l[1] * l[2]
    dN = np.stack([dl[0] * l[1] * l[2], l[0] * dl[1] * l[2], l[0] * l[1] * dl[2]], axis=-1)
    return N, dN


# ------------------------------------------------------------------------------ 3 x 3 algebra
def det3(A):
    return (A[..., 0, 0] * (A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1])
            - A[..., 0, 1] * (A[..., 1, 0] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 0])
            + A[..., 0, 2] * (A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]))


def inv3(A):
    """(A^-1, det A) by cofactors in A's dtype."""
    adj = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            adj[..., j, i] = A[..., i1, j1] * A[..., i2, j2] - A[..., i1, j2] * A[..., i2, j1]
    det = A[..., 0, 0] * adj[..., 0, 0] + A[..., 0, 1] * adj[..., 1, 0] + A[..., 0, 2] * adj[..., 2, 0]
    return adj / det[..., None, None], det


def voigt(T):
    """[..., 3, 3] -> [..., 6] tensor components in the order xx yy zz xy yz xz."""
    return np.stack([T[..., i, j] for i, j in VOIGT], axis=-1)


def lame(E, nu):
    E, nu = np.asarray(E, dtype=LD), np.asarray(nu, dtype=LD)
    return E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))


# ------------------------------------------------------------------------------ materials
def _sym4(A, B):
    """(A . B)_IJKL = 1/2 (A_IK B_JL + A_IL B_JK)"""
    return (np.einsum("...ik,...jl->...ijkl", A, B) + np.einsum("...il,...jk->...ijkl", A, B)) / 2


def material_ld(material, E, nu, Eg, absE=None):
    """S [...,3,3], CC [...,3,3,3,3], psi [...] and the abs-sums of the terms of S and psi at the
    strains Eg [...,3,3] (longdouble); E, nu broadcast against the leading axes.  absE: the abs-sum
    of the terms of Eg (default |Eg|)."""
    Eg = np.asarray(Eg, dtype=LD)
    absE = np.abs(Eg) if absE is None else absE
    E = np.asarray(E, dtype=LD)[..., None, None]
    nu = np.asarray(nu, dtype=LD)[..., None, None]
    d = I3x3
    if material == STVK:
        lam, mu = lame(E, nu)
        tr = np.trace(Eg, axis1=-2, axis2=-1)[..., None, None]
        S = lam * tr * d + 2 * mu * Eg
        S_abs = np.abs(lam) * np.trace(absE, axis1=-2, axis2=-1)[..., None, None] * d + 2 * mu * absE
        dd = np.einsum("ij,kl->ijkl", d, d)
        CC = lam[..., None, None] * dd + mu[..., None, None] * 2 * _sym4(d, d)
        CC = np.broadcast_to(CC, Eg.shape + (3, 3)).copy()
        EE = np.einsum("...ij,...ij->...", Eg, Eg)
        t1, t2 = lam[..., 0, 0] * tr[..., 0, 0] ** 2 / 2, mu[..., 0, 0] * EE
        return S, CC, t1 + t2, S_abs, np.abs(t1) + np.abs(t2)
    c = E / (4 * (1 + nu))
    beta = nu / (1 - 2 * nu)
    A = 2 * Eg
    trA = np.trace(A, axis1=-2, axis2=-1)
    trAA = np.einsum("...ij,...ji->...", A, A)
    I3m1 = trA + (trA * trA - trAA) / 2 + det3(A)     # det(I + A) - 1
    Ci, _ = inv3(d + A)
    lnI3 = np.log1p(I3m1)[..., None, None]
    pm1 = np.expm1(-beta * lnI3)                       # I3^-beta - 1
    p = 1 + pm1
    S = 2 * c * np.einsum("...ik,...kj->...ij", A - pm1 * d, Ci)
    S = (S + np.swapaxes(S, -1, -2)) / 2
    # the abs-sum of the terms formed above, (2E - (I3^-beta - 1) I) C^-1 term by term
    S_abs = 2 * c * np.einsum("...ik,...kj->...ij", 2 * absE + np.abs(pm1) * d, np.abs(Ci))
    S_abs = (S_abs + np.swapaxes(S_abs, -1, -2)) / 2
    CC = ((4 * c * beta * p)[..., None, None] * np.einsum("...ij,...kl->...ijkl", Ci, Ci)
          + (4 * c * p)[..., None, None] * _sym4(Ci, Ci))
    c0, b0, pm10, ln0 = c[..., 0, 0], beta[..., 0, 0], pm1[..., 0, 0], lnI3[..., 0, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        vol = np.where(b0 != 0, pm10 / np.where(b0 != 0, b0, 1), -ln0)  # (I3^-beta - 1) / beta
    psi = c0 * trA + c0 * vol
    psi_abs = c0 * np.trace(2 * absE, axis1=-2, axis2=-1) + np.abs(c0 * vol)
    return S, CC, psi, S_abs, psi_abs


# ------------------------------------------------------------------------------ elements
def elements_ld(celltype, kinem, material, E, nu, X, u, want_k=True, rule=None):
    """All elements at once.  X, u: [ne][npe][3]; E, nu: scalars or [ne].  Returns a dict of
    longdouble arrays: Ke [ne][3npe][3npe] and fe [ne][3npe] (DOF 3 a + i), their abs-sum scales
    SKe, Sfe, detJ / detF / I3 [ne][ng], the Gauss-point tensors pk2, cauchy, gl, ea [ne][ng][3][3]
    with scales (key + "_abs"), psi [ne][ng] and energy [ne] with energy_abs."""
    xi, w = rule if rule is not None else orc.gauss_points(celltype)
    N, dN = shape_ld(celltype, xi)
    w = np.asarray(w, dtype=LD)
    X, u = np.asarray(X, dtype=LD), np.asarray(u, dtype=LD)
    ne, npe = X.shape[:2]
    En = np.broadcast_to(np.asarray(E, dtype=LD), (ne,))[:, None]
    nun = np.broadcast_to(np.asarray(nu, dtype=LD), (ne,))[:, None]
    J = np.einsum("gad,eak->egdk", dN, X)              # J[d][k] = dX_k / dxi_d
    Ji, detJ = inv3(J)
    NX = np.einsum("egkd,gad->egak", Ji, dN)           # grad_X N_a
    H = np.einsum("eai,egaj->egij", u, NX)
    Ht = np.swapaxes(H, -1, -2)
    out = dict(detJ=detJ)
    if kinem == TOTLAG:
        F = I3x3 + H
        HtH = np.einsum("egki,egkj->egij", H, H)
        Eg = (H + Ht + HtH) / 2
        absE = (np.abs(H) + np.abs(Ht) + np.einsum("egki,egkj->egij", np.abs(H), np.abs(H))) / 2
    else:
        F = np.broadcast_to(I3x3, H.shape)
        Eg = (H + Ht) / 2
        absE = (np.abs(H) + np.abs(Ht)) / 2
    S, CC, psi, S_abs, psi_abs = material_ld(material, En, nun, Eg, absE)
    Fi, detF = inv3(F + 0 * H)
    out.update(detF=detF, I3=det3(I3x3 + 2 * Eg), pk2=S, pk2_abs=S_abs, gl=Eg, gl_abs=absE, psi=psi)
    out["cauchy"] = np.einsum("egik,egkl,egjl->egij", F, S, F) / detF[..., None, None]
    out["cauchy_abs"] = np.einsum("egik,egkl,egjl->egij", np.abs(F), S_abs, np.abs(F)) / np.abs(detF)[..., None, None]
    out["ea"] = np.einsum("egki,egkl,eglj->egij", Fi, Eg, Fi)
    out["ea_abs"] = np.einsum("egki,egkl,eglj->egij", np.abs(Fi), absE, np.abs(Fi))
    fac = w[None, :] * detJ
    out.update(fac=fac, F=F, NX=NX, CC=CC)
    out["energy"] = (fac * psi).sum(axis=1)
    out["energy_abs"] = (np.abs(fac) * psi_abs).sum(axis=1)
    # dE_IJ / du_ai = 1/2 (F_iI N_a,J + F_iJ N_a,I)
    FN = np.einsum("egiI,egaJ->egaiIJ", F, NX)
    dE = (FN + np.swapaxes(FN, -1, -2)) / 2
    D = dE.reshape(ne, len(w), 3 * npe, 9)
    fg = np.einsum("egpq,egq->egp", D, S.reshape(ne, len(w), 9)) * fac[..., None]
    out["fe"], out["Sfe"] = fg.sum(axis=1), np.abs(fg).sum(axis=1)
    if want_k:
        DC = np.matmul(D, CC.reshape(ne, len(w), 9, 9))
        Kg = np.matmul(DC, np.swapaxes(D, -1, -2)).reshape(ne, len(w), npe, 3, npe, 3)
        if kinem == TOTLAG:
            G = np.einsum("egaI,egIJ,egbJ->egab", NX, S, NX)
            for i in range(3):
                Kg[:, :, :, i, :, i] += G
        Kg = Kg.reshape(ne, len(w), 3 * npe, 3 * npe) * fac[..., None, None]
        out["Ke"], out["SKe"] = Kg.sum(axis=1), np.abs(Kg).sum(axis=1)
    return out


# ------------------------------------------------------------------------------ assembly
def node_displacements(dis, u_col):
    return np.asarray(u_col)[np.asarray(dis.node_dof_col)[:, None] + np.arange(3)]


def scatter_plan(dis):
    """(pos [ne][3npe][3npe], rows [ne][3npe]): the position in the CSR value array of every
    element entry and the row LID of every element DOF; -1 for the DOFs of nodes without a row."""
    ndr, ndc = np.asarray(dis.node_dof_row), np.asarray(dis.node_dof_col)
    rowptr, col = np.asarray(dis.rowptr), np.asarray(dis.col_lid)
    en = np.asarray(dis.ele_nodes)
    ne, npe = en.shape
    d3 = np.arange(3)
    rows = np.where(ndr[en][:, :, None] >= 0, ndr[en][:, :, None] + d3, -1).reshape(ne, 3 * npe)
    cols = (ndc[en][:, :, None] + d3).reshape(ne, 3 * npe)
    pos = np.full((ne, 3 * npe, 3 * npe), -1, dtype=np.int64)
    for e in range(ne):
        for p in range(3 * npe):
            r = rows[e, p]
            if r < 0:
                continue
            s, t = rowptr[r], rowptr[r + 1]
            j = s + np.searchsorted(col[s:t], cols[e])
            assert np.array_equal(col[j], cols[e])
            pos[e, p] = j
    return pos, rows


def _plan_of(dis):
    if getattr(dis, "_element_ref_plan", None) is None:
        dis._element_ref_plan = scatter_plan(dis)
    return dis._element_ref_plan


def scatter_matrix(dis, Ke):
    """sum of the element matrices [ne][3npe][3npe] on the CSR graph, in Ke's dtype."""
    pos, _ = _plan_of(dis)
    K = np.zeros(int(dis.nnz), dtype=Ke.dtype)
    ok = pos >= 0
    np.add.at(K, pos[ok], Ke[ok])
    return K


def scatter_vector(dis, fe):
    _, rows = _plan_of(dis)
    f = np.zeros(int(dis.n_rows), dtype=fe.dtype)
    ok = rows >= 0
    np.add.at(f, rows[ok], fe[ok])
    return f


class Assembled:
    """assemble_ld's result: K, f, SK, Sf (longdouble, CSR order / row order) and the element
    dict `el` of elements_ld."""

    def __init__(self, K, f, SK, Sf, el):
        self.K, self.f, self.SK, self.Sf, self.el = K, f, SK, Sf, el
        self.min_detJ = float(el["detJ"].min())
        self.min_detF = float(el["detF"].min())
        self.min_I3 = float(el["I3"].min())


def assemble_ld(dis, kinem, material, E, nu, u_col, ele_E=None, ele_nu=None, want_k=True):
    """K (the discretization's CSR order) and f of Discretization::evaluate at u_col in longdouble,
    with the scales SK, Sf: the same assembly of the absolute values of every Gauss-point
    contribution.  ele_E / ele_nu: per-element constants [n_ele] in place of E / nu."""
    en = np.asarray(dis.ele_nodes)
    X = np.asarray(dis.node_x)[en]
    u = node_displacements(dis, u_col)[en]
    el = elements_ld(dis.celltype, kinem, material, E if ele_E is None else ele_E,
                     nu if ele_nu is None else ele_nu, X, u, want_k=want_k)
    K = scatter_matrix(dis, el["Ke"]) if want_k else None
    SK = scatter_matrix(dis, el["SKe"]) if want_k else None
    return Assembled(K, scatter_vector(dis, el["fe"]), SK, scatter_vector(dis, el["Sfe"]), el)


# ------------------------------------------------------------------------------ mass
def mass_rule_full(celltype):
    """The mass kernels' Gauss rule as doubles: the stiffness rule for hex8; for hex27 the 27
    points in the stiffness rule's order with sqrt(3/5), 5/9, 8/9 in full double precision
    (fcg_mass.hip, mass_gauss_rule) in place of the stiffness rule's 13-digit constants."""
    xi, w = orc.gauss_points(celltype)
    if celltype == HEX8:
        return xi, w
    a, w1, w2 = np.sqrt(0.6), 5.0 / 9.0, 8.0 / 9.0
    s = np.sign(xi)
    wd = np.where(s == 0, w2, w1)
    return a * s, wd[:, 0] * wd[:, 1] * wd[:, 2]


def element_mass_ld(celltype, X, rule=None, dtype=LD):
    """[ne][npe][npe] sum_g w detJ N_a N_b (unit density), the same sum of the absolute values
    (hex27 shape functions change sign) and [ne] min detJ, in `dtype`."""
    xi, w = rule if rule is not None else orc.gauss_points(celltype)
    N, dN = shape_ld(celltype, xi)
    N, dN, w = N.astype(dtype), dN.astype(dtype), np.asarray(w).astype(dtype)
    J = np.einsum("gad,eak->egdk", dN, np.asarray(X).astype(dtype))
    detJ = det3(J)
    fac = w[None, :] * detJ
    return (np.einsum("eg,ga,gb->eab", fac, N, N),
            np.einsum("eg,ga,gb->eab", np.abs(fac), np.abs(N), np.abs(N)), detJ.min(axis=1))


def mass_ld(dis, rho, rule=None, dtype=LD):
    """The consistent mass on the discretization's CSR graph (delta_ik m_ab on the entries
    (3a + i, 3b + i), zero elsewhere) in `dtype`, its abs-sum scale and the smallest det J:
    (M, SM, min detJ).  rho: scalar or [n_ele]."""
    en = np.asarray(dis.ele_nodes)
    ne, npe = en.shape
    m, ma, mindet = element_mass_ld(dis.celltype, np.asarray(dis.node_x)[en], rule, dtype)
    rho = np.broadcast_to(np.asarray(rho).astype(dtype), (ne,))[:, None, None]
    out = []
    for q in (m * rho, ma * np.abs(rho)):
        Me = np.zeros((ne, npe, 3, npe, 3), dtype=dtype)
        for i in range(3):
            Me[:, :, i, :, i] = q
        out.append(scatter_matrix(dis, Me.reshape(ne, 3 * npe, 3 * npe)))
    return out[0], out[1], float(mindet.min())


# ------------------------------------------------------------------------------ error measures
def err_norm(q, r):
    """e_n = |q - r|_2 / |r|_2 in longdouble."""
    q, r = np.asarray(q).astype(LD).ravel(), np.asarray(r).astype(LD).ravel()
    return float(np.sqrt(((q - r) ** 2).sum() / (r ** 2).sum()))


def err_comp(q, r, S):
    """e_c = max_i |q_i - r_i| / S_i in longdouble; an entry whose scale is 0 must be exact."""
    q, r, S = (np.asarray(a).astype(LD).ravel() for a in (q, r, S))
    d = np.abs(q - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(S > 0, d / np.where(S > 0, S, 1), np.where(d == 0, 0, np.inf))
    return float(e.max())
