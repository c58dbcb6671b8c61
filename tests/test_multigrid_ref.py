"""The geometric multigrid (4c_amd/multigrid.py; node_transfer_kernel, box_transfer_kernel and
box_stencil_kernel of fcg_solver.hip) pinned to an extended-precision rebuild: every operator of the
hierarchy against its definition in np.longdouble (tests/mg_ref.py), then the V-cycle of
CycleFCG._vcycle as a matrix and the flexible CG around it against mg_ref's cycle rebuilt from the
device's own operators in float64 and in longdouble.

Cases (fcg.BoxMesh, E = 210, nu = 0.3, clamped on the x = 0 lattice face unless stated):
  h8_422      hex8 (4,2,2), upper (2,1,1.5), rotation (0.3,-0.2,0.5), min_intervals 1 -> (2,1,1), (1,1,1)
  h8_444      hex8 (4,4,4) -> (2,2,2)
  h8_533      hex8 (5,3,3), min_intervals 1, max_levels 3 -> (3,2,2), (2,1,1)
  h27_222     hex27 (2,2,2), min_intervals 1 -> hex8 (2,2,2), (1,1,1)
  h8_444_jit  h8_444 with jitter 0.1      h8_444_x1  h8_444 clamped on x = max instead

Bounds (u = 2^-53):
  prolongation      the tables' weights against the geometric longdouble P: exactly 1, 1/2, 1/4, 1/8
                    on 2:1 pairs, |w - w_ld| <= 4u on non-nested pairs, rows sum to 1, R = P^T entry
                    for entry
  Galerkin, host    |A_c - P^T A_f P| <= GAL_FLOOR (|P|^T SK_f |P| + SK_c) in longdouble.  The
                    identity does NOT hold to longdouble rounding: the Gauss rules are doubles.  With
                    defect the largest relative error of the 1-D rule on the even monomials it must
                    integrate (hex8: fl(1/sqrt 3)^2 against 1/3, 2.42u; hex27: the 13-digit constants,
                    2393u) and dep the largest distance of a fine node from its interpolated coarse
                    position in fine edges (rotated boxes: node coordinates are rounded doubles),
                    GAL_FLOOR = 3 defect + 6 dep: three 1-D integrals per term, and a node moved by
                    dep changes the two gradients of a term by dep each, on both sides.  Measured
                    e_c: 0.59u (h8 444 -> 222), 1.72u (rotated 422 -> 211), 1.26u (rotated 211 -> 111),
                    304u = 3.4e-14 (hex27 222 -> hex8 222) against floors 7.3u, 43u, 19u, 7179u
  stencil           the stencil as a matrix (unit vectors, NaN-prefilled y) against the longdouble
                    level operator by test_evaluate_regimes.py's criterion: e_c, e_n at most 4 x the
                    larger of the float64 oracle's error on the same mesh and on the benign mesh
                    (unit box, jitter 0.1, same intervals); exact zeros outside the 27-point pattern;
                    |dinv D_s - I|_max <= kappa_inf 4u per node, D_s the stencil's own diagonal block
                    (10.6u on the (2,2,2) levels, DINV_MARGINS)
  transfers         per entry (len + 2) u (sum |w||x| + |y0|), len the number of terms; exact zeros
                    on the masked rows
  Galerkin, device  |A_c - P^T A_f P| <= (terms + 2) u |P|^T |A_f| |P| + GAL_FLOOR (...) on the free
                    rows and columns, P the longdouble one
  coarsest inverse  |coarse_inv - inv_ld|_F <= 8 |numpy inv - inv_ld|_F (test_amg_hierarchy.py's margin)
  lambda_max        a Ritz value: lmax <= lambda_max(D^-1/2 A_ff D^-1/2) (1 + 1e-10)
  V-cycle           |M - M_ld|_F <= 8 own, own = |M_f64 - M_ld|_F, |M_ff - M_ff^T|_F <= 8 own where the
                    cycle is symmetric, min eig(M A_ff) > 0, and max eig <= 1 + 8 own |A_ff|_2 on the
                    nested unjittered hierarchies (test_amg_hierarchy.py's argument; the coarse
                    operators are Galerkin there to GAL_FLOOR)
  flexible CG       iterations equal the float64 replay's, or differ by one with the replay's residual
                    at the deciding iteration within a factor 2 of rtol; true residual <= rtol + 10 g,
                    g the replay's gap between true and recurrence residual; the captured graph
                    against eager launches: same count, |x_g - x_e| <= 10 |x_f64 - x_ld|

Each test prints one line "MGREF {json}" with its figures before it asserts; all of them, measured
on one MI355X, are in profiles/multigrid_ref/README.md.  The main ones:
  case        DOFs per level   stencil e_n, e_c / oracle's   transfers    Galerkin, device    lmax / lambda_max   d_gpu / d_64
                               (worst level)                 err / bound  err / bound (u of   per level           (coarsest n)
                                                                          the scale | host)
  h8_422      135, 36, 24      0.94, 0.86                    0.316        0.102 (2.3 | 1.7)   0.9923 1.0000       1.000 (24)
  h8_444      375, 81          0.57, 0.53                    0.329        0.007 (1.1 | 0.59)  0.9877              1.000 (81)
  h8_533      288, 108, 36     0.74, 1.09                    0.535        not nested          1.0000 1.0000       1.000 (36)
  h27_222     375, 81, 24      0.57, 0.68                    0.329        0.041 (304 | 304)   0.9999 0.9999       1.000 (24)
  h8_444_jit  375, 81          0.57, 0.53                    0.329        not nested          0.9852              1.000 (81)
  h8_444_x1   375, 81          0.59, 0.37                    0.329        0.008 (1.4 | 0.59)  0.9985              1.000 (81)
  (coarse_inv is numpy's inverse of the fetched K: d_gpu = d_64.)  |dinv D_s - I| / (kappa u): at most
  2.84, except 5.30 on the (2,2,2) levels.

  cycle as a matrix            |M - M_ld|_F   own        |M_ff - M_ff^T|_F   [min, max] eig(M A_ff)
  h8_422                       1.74e-15       1.79e-15   2.60e-15            [0.47062, 1.000000000000]
  h8_444                       1.73e-14       1.73e-14   1.17e-14            [0.71264, 1.000000000000]
  h8_533                       2.74e-15       2.71e-15   3.74e-15            [0.53938, 1.001895965929]  (reported)
  h8_444_jit                   1.73e-14       1.73e-14   1.17e-14            [0.71226, 1.012082940704]  (reported)
  h8_444_x1                    1.06e-14       1.08e-14   7.76e-15            [0.71203, 1.000000000000]
  h8_444 nu 1 / nu 3           1.88e-14 / 1.64e-14, own 1.88e-14 / 1.65e-14, min eig 0.42872 / 0.83782
  h8_444 fine_post=False       1.95e-14       1.95e-14   0.195 (unsymmetric) [0.60042, 1.499560954039]
  h8_533 W                     7.44e-16       7.66e-16   1.06e-15            [0.53939, 1.001995012144]
  h8_422 W, coarse_nu 1        1.48e-15       1.52e-15   1.91e-15            [0.37676, 1.000000000000]
  h8_444 mixed                 1.73e-14       1.74e-14   2.76e-08 (unsymmetric), 1.18e-07 from the unmixed M
  h27_222, 16 right-hand sides, worst |z - z_ld| / own: 1.29 (default), 1.13 (W), 1.35 (coarse_nu 1), 1.71 (mixed),
  4.22 / 2.66 (matrix-free fine level, assembled / matrix-free outer operator)
  (the upper end allowed is 1 + 3e-12 .. 1 + 4e-11.)  FCG_MG_STENCIL=0: 7.0e-16 from the default on h8_422,
  identical on h8_444; FCG_MG_BOXT=0 and FCG_MG_FUSED=0: bit-identical.

  flexible CG, rtol 1e-10: h8_444 10 iterations, h27_222 12 -- graph, eager, float64 and longdouble replay
  alike; captured graph and eager launches bit-identical; g 2.2e-17 / 5.2e-17.  Graph reuse on h8_444:
  10, 14 (K scaled in place, same graph) and 15 (lambda_max changed, graph rebuilt) iterations, each
  bit-identical to eager.
"""

import importlib
import json

import numpy as np
import pytest
import scipy.linalg

import element_ref as er
import mg_ref
import oracle_lib as orc
import samg_ref
import solver_ref as sr
from parity_util import oracle_evaluate
from samg_ref import LD

torch = pytest.importorskip("torch")
fcg = importlib.import_module("4c_amd").fcg
mgm = importlib.import_module("4c_amd.multigrid")

pytestmark = pytest.mark.skipif(not er.EXTENDED, reason="np.longdouble has no 64-bit significand here")
gpu = pytest.mark.gpu

U = er.U
E, NU = 210.0, 0.3
RATIO, BOOST = 10.0, 1.1
UP, ROT = (2.0, 1.0, 1.5), (0.3, -0.2, 0.5)
CINV_MARGIN = 8.0
# case id -> margin in place of 4 for the stencil criterion (2 x measured, at most 64, cause in
# profiles/multigrid_ref/README.md)
MARGINS = {}
# case id -> factor in place of 4 in |dinv D_s - I| <= kappa_inf 4u (the same rule).  On the
# (2,2,2) level the largest figure is 5.30, at the one interior node: two roundings stack there --
# the kernel's cofactor inverse of the assembled K's block, and the stencil's block, the same eight
# element contributions summed in another order than the assembly's.  2 x 5.30.
DINV_MARGINS = {f"{c}/L1": 10.6 for c in ("h8_444", "h27_222", "h8_444_jit", "h8_444_x1")}

CASES = {
    "h8_422": dict(ct=fcg.HEX8, iv=(4, 2, 2), upper=UP, rot=ROT, mi=1, levels=[(2, 1, 1), (1, 1, 1)], nested=True),
    "h8_444": dict(ct=fcg.HEX8, iv=(4, 4, 4), mi=2, levels=[(2, 2, 2)], nested=True),
    "h8_533": dict(ct=fcg.HEX8, iv=(5, 3, 3), mi=1, max_levels=3, levels=[(3, 2, 2), (2, 1, 1)], nested=False),
    "h27_222": dict(ct=fcg.HEX27, iv=(2, 2, 2), mi=1, levels=[(2, 2, 2), (1, 1, 1)], nested=True),
    "h8_444_jit": dict(ct=fcg.HEX8, iv=(4, 4, 4), mi=2, jitter=0.1, levels=[(2, 2, 2)], nested=False),
    "h8_444_x1": dict(ct=fcg.HEX8, iv=(4, 4, 4), mi=2, side=1, levels=[(2, 2, 2)], nested=True),
}
ALL = list(CASES)
DEEP = ["h8_422", "h8_533", "h27_222"]  # three levels


def _say(**rec):
    print("MGREF " + json.dumps(rec))


def _f(x):
    return float(x)


def _fro(a):
    return float(np.sqrt((np.asarray(a).astype(LD) ** 2).sum()))


def _box(ct, iv, upper=(1.0, 1.0, 1.0), rot=(0.0, 0.0, 0.0), jitter=0.0):
    return fcg.BoxMesh(ct, iv, upper=upper, rotation=rot, jitter=jitter)


def _case_mesh(name):
    c = CASES[name]
    return _box(c["ct"], c["iv"], c.get("upper", (1.0, 1.0, 1.0)), c.get("rot", (0.0, 0.0, 0.0)),
                c.get("jitter", 0.0))


# ------------------------------------------------------------------------------------ CPU part
PAIRS = {
    # name: (fine, coarse, nested)
    "h8_422r": ((fcg.HEX8, (4, 2, 2), UP, ROT), ((2, 1, 1), UP, ROT), True),
    "h8_211r": ((fcg.HEX8, (2, 1, 1), UP, ROT), ((1, 1, 1), UP, ROT), True),
    "h8_444": ((fcg.HEX8, (4, 4, 4)), ((2, 2, 2),), True),
    "h8_222": ((fcg.HEX8, (2, 2, 2)), ((1, 1, 1),), True),
    "h27_222": ((fcg.HEX27, (2, 2, 2)), ((2, 2, 2),), True),
    "h27_212r": ((fcg.HEX27, (2, 1, 2), UP, ROT), ((2, 1, 2), UP, ROT), True),
    "h8_533": ((fcg.HEX8, (5, 3, 3)), ((3, 2, 2),), False),
    "h8_533r": ((fcg.HEX8, (5, 3, 3), UP, ROT), ((3, 2, 2), UP, ROT), False),
    "h8_322": ((fcg.HEX8, (3, 2, 2)), ((2, 1, 1),), False),
}


def _pair(name):
    f, c, nested = PAIRS[name]
    return _box(*f), _box(fcg.HEX8, *c), nested


@pytest.mark.parametrize("name", list(PAIRS))
def test_geometric_prolongation_against_tables(name):
    fine, coarse, nested = _pair(name)
    P = mg_ref.prolongation(fine, coarse)
    Pt, Rt = mgm.transfer_tables(fine, coarse)
    Pd = mg_ref.tables_dense(Pt, fine.n_rows, coarse.n_rows)
    Rd = mg_ref.tables_dense(Rt, coarse.n_rows, fine.n_rows)
    d = _f(np.abs(Pd.astype(LD) - P).max())
    rs = _f(np.abs(P.sum(axis=1) - 1).max())
    rs_t = _f(np.abs(Pd.sum(axis=1) - 1).max())
    _say(test="prolongation", pair=name, max_dw_u=d / U, rowsum_ld=rs, rowsum_tables=rs_t,
         nnz=int((Pd != 0).sum()))
    assert np.array_equal(Pd != 0, P != 0)
    if nested:
        assert set(np.unique(Pd).tolist()) <= {0.0, 0.125, 0.25, 0.5, 1.0}
        assert d == 0.0 and rs_t == 0.0
    else:
        assert 0 < d <= 4 * U
        assert rs_t <= 4 * U
    assert rs <= 8 * float(np.finfo(LD).eps)
    assert np.array_equal(Rd, Pd.T)


def test_geometric_prolongation_sees_an_axis_swap():
    """Three different edge lengths under a rotation: the geometric P of a box is not that of the box
    with two interval counts exchanged, and interpolates the coordinates themselves."""
    fine, coarse, _ = _pair("h8_422r")
    P = mg_ref.prolongation(fine, coarse)
    for d in range(3):
        xc = np.zeros(coarse.n_rows, dtype=LD)
        xc[coarse.node_dof_row] = coarse.node_x[:, d]
        assert _f(np.abs((P @ xc)[fine.node_dof_row] - fine.node_x[:, d]).max()) <= 8 * U * 3.0
    other = _box(fcg.HEX8, (2, 4, 2), UP, ROT)
    assert other.n_rows == fine.n_rows
    Po = mg_ref.prolongation(other, _box(fcg.HEX8, (1, 2, 1), UP, ROT))
    assert Po.shape != P.shape or not np.array_equal(Po, P)


def rule_defect(celltype):
    """Largest relative error of the 1-D Gauss rule (the doubles of oracle_lib.gauss_points) on the
    even monomials the stiffness integrand holds per axis: degree 2 (hex8) or up to 4 (hex27)."""
    xi, w = orc.gauss_points(celltype)
    a = np.unique(xi[:, 0])
    w1 = np.array([w[xi[:, 0] == v].sum() / 4 for v in a], dtype=LD)
    a = a.astype(LD)
    worst = 0.0
    for k in range(0, 3 if celltype == fcg.HEX8 else 5, 2):
        exact = LD(2) / LD(k + 1)
        worst = max(worst, _f(abs((w1 * a ** k).sum() - exact) / exact))
    return worst


def gal_floor(fine, coarse, P):
    """GAL_FLOOR of the module docstring for one pair (relative to |P|^T SK_f |P| + SK_c)."""
    fine = mg_ref.plain(fine)
    dep = 0.0
    for d in range(3):
        xc = np.zeros(coarse.n_rows, dtype=LD)
        xc[coarse.node_dof_row] = coarse.node_x[:, d]
        dep = max(dep, _f(np.abs((P @ xc)[fine.node_dof_row] - fine.node_x[:, d]).max()))
    en = fine.ele_nodes[0]
    h = min(np.linalg.norm(fine.node_x[en[a]] - fine.node_x[en[0]]) for a in range(1, len(en)))
    return 3 * max(rule_defect(fine.celltype), rule_defect(coarse.celltype)) + 6 * dep / h


NESTED_PAIRS = [k for k, v in PAIRS.items() if v[2]]


@pytest.mark.parametrize("name", NESTED_PAIRS)
def test_galerkin_identity_in_longdouble(name):
    """The rediscretised coarse operator against P^T A_f P, no Dirichlet rows, all in longdouble."""
    fine, coarse, _ = _pair(name)
    P = mg_ref.prolongation(fine, coarse)
    Af, Sf = mg_ref.level_operator(fine, E, NU, [])
    Ac, Sc = mg_ref.level_operator(coarse, E, NU, [])
    scale = np.abs(P).T @ Sf @ np.abs(P) + Sc
    e = er.err_comp(P.T @ Af @ P, Ac, scale)
    floor = gal_floor(fine, coarse, P)
    _say(test="galerkin_ld", pair=name, e_c_u=e / U, floor_u=floor / U, eps_ld_u=float(np.finfo(LD).eps) / U)
    assert np.isfinite(e) and e <= floor


def test_galerkin_identity_fails_off_the_nested_pairs():
    """The check above can fail: on the non-nested pair the rediscretised operator is not P^T A P."""
    fine, coarse, _ = _pair("h8_322")
    P = mg_ref.prolongation(fine, coarse)
    Af, Sf = mg_ref.level_operator(fine, E, NU, [])
    Ac, Sc = mg_ref.level_operator(coarse, E, NU, [])
    e = er.err_comp(P.T @ Af @ P, Ac, np.abs(P).T @ Sf @ np.abs(P) + Sc)
    assert e > 1e-3


def test_chebyshev_against_samg_ref_for_a_diagonal_dinv():
    rng = np.random.default_rng(4)
    n = 12
    B = rng.standard_normal((n, n))
    A = B @ B.T + n * np.eye(n)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    di = 1.0 / np.diag(A)
    blocks = np.zeros((n // 3, 3, 3))
    for k in range(n):
        blocks[k // 3, k % 3, k % 3] = di[k]
    lmax = float(np.linalg.eigvalsh(np.diag(di ** 0.5) @ A @ np.diag(di ** 0.5))[-1])
    for nu in (1, 2, 3, 4):
        for x in (None, x0):
            a = mg_ref.cheb(A, blocks, b, x, lmax, nu, RATIO, BOOST, np.float64)
            r = samg_ref.cheb(A, di, b, x, lmax, nu, RATIO, BOOST, np.float64)
            assert np.abs(a - r).max() <= 16 * U * np.abs(r).max()
    # the polynomial it is: at degree nu the error propagator's spectral radius on [lmin, lmax] is
    # 1 / T_nu(sigma), T_nu the Chebyshev polynomial
    lam, V = scipy.linalg.eigh(A, np.diag(1.0 / di))
    hi = BOOST * lmax
    lo = hi / RATIO
    sigma = (hi + lo) / (hi - lo)
    for nu in (1, 2, 3):
        Pm = np.stack([np.eye(n)[:, j] - mg_ref.cheb(A, blocks, A[:, j], None, lmax, nu, RATIO, BOOST, np.float64)
                       for j in range(n)], axis=1)  # I - q(D^-1 A) D^-1 A, columns
        got = np.linalg.solve(V, Pm @ V)
        want = np.cos(nu * np.arccos(((hi + lo) / 2 - lam) / ((hi - lo) / 2) + 0j)).real / np.cosh(nu * np.arccosh(sigma))
        assert np.abs(np.diag(got) - want).max() <= 1e-12
        assert np.abs(got - np.diag(np.diag(got))).max() <= 1e-12


def _host_hierarchy(fine_ct=fcg.HEX8):
    """A nested hierarchy on the host alone: hex8 (4,4,4) -> (2,2,2) -> (1,1,1) or hex27 (2,2,2) ->
    hex8 (2,2,2) -> (1,1,1), x = 0 clamped, lambda_max from dense eigen-solves."""
    ms = ([_box(fcg.HEX8, (4, 4, 4))] if fine_ct == fcg.HEX8 else [_box(fcg.HEX27, (2, 2, 2))])
    ms += [_box(fcg.HEX8, (2, 2, 2)), _box(fcg.HEX8, (1, 1, 1))]
    rows = [mg_ref.node_rows(m, mg_ref.face_mask(m)) for m in ms]
    A = [mg_ref.level_operator(m, E, NU, r)[0] for m, r in zip(ms, rows)]
    mk = [mg_ref.mask_of(m, r) for m, r in zip(ms, rows)]
    P = [mg_ref.prolongation(ms[i], ms[i + 1]) for i in range(2)]
    Pm = [mk[i][:, None] * P[i] for i in range(2)]
    Rm = [mk[i + 1][:, None] * P[i].T for i in range(2)]
    lmax = []
    for a in A[:-1]:
        a64 = a.astype(np.float64)
        D = scipy.linalg.block_diag(*mg_ref.diag_blocks(a64))
        lmax.append(float(np.linalg.eigvals(np.linalg.solve(D, a64)).real.max()))
    return ms, rows, A, Pm, Rm, lmax + [None]


def _spectrum(Mff, Aff):
    """eig(L^T sym(M_ff) L), A_ff = L L^T: the eigenvalues of M A on the free DOFs."""
    L = np.linalg.cholesky(0.5 * (Aff + Aff.T))
    return np.linalg.eigvalsh(L.T @ (0.5 * (Mff + Mff.T)) @ L)


@pytest.mark.parametrize("ct", [fcg.HEX8, fcg.HEX27])
@pytest.mark.parametrize("opts", [dict(), dict(cycle="W", coarse_nu=1)], ids=["V", "W_nu1"])
def test_reference_cycle_symmetric_with_spectrum_in_unit_interval(ct, opts):
    """mg_ref.Cycle in longdouble on a nested hierarchy: M_ff symmetric and eig(M A_ff) in (0, 1]
    (test_amg_hierarchy.py's argument: the same symmetric smoother before and after an exact
    Galerkin coarse correction).  The coarse operators are Galerkin only to GAL_FLOOR, which the
    upper end is allowed."""
    ms, rows, A, Pm, Rm, lmax = _host_hierarchy(ct)
    dinv = [mg_ref.block_inverses(a, LD) for a in A]
    cyc = {dt: mg_ref.Cycle(A, Pm, Rm, dinv, lmax, 2, RATIO, BOOST, dt, **opts) for dt in (np.float64, LD)}
    M64, Mld = cyc[np.float64].matrix(), cyc[LD].matrix()
    own = _fro(M64 - Mld)
    free = np.nonzero(mg_ref.mask_of(ms[0], rows[0]))[0]
    Mff = Mld[np.ix_(free, free)]
    asym = _fro(Mff - Mff.T)
    Aff = A[0][np.ix_(free, free)].astype(np.float64)
    ev = _spectrum(Mff.astype(np.float64), Aff)
    floor = 3 * rule_defect(ct)
    _say(test="reference_cycle", ct=int(ct), opts=opts, own=own, asym=asym, eig=[_f(ev.min()), _f(ev.max())],
         floor=floor)
    b = np.random.default_rng(3).standard_normal(M64.shape[0])
    assert np.abs(cyc[np.float64].apply(b) - M64 @ b).max() <= 64 * len(b) * U * np.linalg.norm(M64, 2) * np.abs(b).max()
    assert 0 < own and asym <= 8 * own
    cond = np.linalg.cond(Aff)
    assert ev.min() > 0 and ev.max() <= 1 + 8 * own * np.linalg.norm(Aff, 2) + cond * floor


def test_fcg_replay_converges_to_the_solution():
    ms, rows, A, Pm, Rm, lmax = _host_hierarchy(fcg.HEX8)
    dinv = [mg_ref.block_inverses(a, np.float64) for a in A]
    c = mg_ref.Cycle(A, Pm, Rm, dinv, lmax, 2, RATIO, BOOST, np.float64)
    b = np.random.default_rng(8).standard_normal(ms[0].n_rows) * mg_ref.mask_of(ms[0], rows[0])
    x, it, hist = mg_ref.fcg_replay(A[0], c, b, 1e-10, 100, np.float64)
    A64 = A[0].astype(np.float64)
    assert it < 30 and hist[-1] <= 1e-10 and len(hist) == it
    assert np.linalg.norm(b - A64 @ x) <= 2e-10 * np.linalg.norm(b)


def test_min_intervals_one_ends_at_one_unit_level():
    """The halving stops where it no longer changes the intervals: min_intervals=1 ends at one
    (1,1,1) level instead of repeating it up to max_levels; nothing else about the selection moves."""
    ci = mgm.coarse_intervals
    assert ci([4, 2, 2], False, 1, 8) == [(2, 1, 1), (1, 1, 1)]
    assert ci([2, 2, 2], True, 1, 8) == [(2, 2, 2), (1, 1, 1)]
    assert ci([5, 3, 3], False, 1, 3) == [(3, 2, 2), (2, 1, 1)]
    assert ci([5, 3, 3], False, 1, 50) == [(3, 2, 2), (2, 1, 1), (1, 1, 1)]
    for c in CASES.values():
        assert ci(list(c["iv"]), c["ct"] == fcg.HEX27, c["mi"], c.get("max_levels", 8)) == c["levels"]
    # as before the fix wherever min_intervals >= 2
    assert ci([4, 4, 4], False, 2, 8) == [(2, 2, 2)]
    assert ci([8, 8, 8], False, 2, 8) == [(4, 4, 4), (2, 2, 2)]
    assert ci([6, 6, 6], True, 2, 8) == [(6, 6, 6), (3, 3, 3), (2, 2, 2)]
    assert ci([100, 100, 100], True, 4, 8) == [(100,) * 3, (50,) * 3, (25,) * 3, (13,) * 3, (7,) * 3, (4,) * 3]
    assert ci([64, 64, 64], False, 2, 4) == [(32,) * 3, (16,) * 3, (8,) * 3]
    assert ci([3, 3, 3], False, 4, 8) == []


# ------------------------------------------------------------------------------------ GPU part
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _dense(mesh, vals, dtype=np.float64):
    return samg_ref.csr_dense(mesh.rowptr, mesh.col_lid, vals, mesh.n_cols, dtype)


def _sweep(fn, n_in, n_out, prefill):
    """The matrix of y = fn(x) from the unit vectors: column j is fn(e_j) into a prefilled y."""
    dev = _dev()
    X = torch.eye(n_in, dtype=torch.float64, device=dev)
    Y = torch.full((n_in, n_out), prefill, dtype=torch.float64, device=dev)
    for j in range(n_in):
        fn(X[j], Y[j])
    torch.cuda.synchronize()
    return np.ascontiguousarray(Y.cpu().numpy().T)


class _H:
    pass


_built = {}


def _build(name, env=(), totlag=False, cache=True, **opts):
    """The case's Multigrid set up for its K, with what the device holds fetched to the host."""
    key = (name, tuple(sorted(env)), totlag, tuple(sorted(opts.items())))
    if cache and key in _built:
        return _built[key]
    dev = _dev()
    c = CASES[name]
    side = c.get("side", 0)
    clamp = lambda m: mg_ref.face_mask(m, 0, side)  # noqa: E731
    h = _H()
    h.name, h.mesh = name, _case_mesh(name)
    mesh = h.mesh
    assert np.array_equal(mesh.node_dof_row, mesh.node_dof_col)
    assert np.array_equal(mesh.node_dof_row, 3 * np.arange(mesh.n_node))
    h.ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG if totlag else fcg.LINEAR, youngs=E, poisson=NU)
    iv = c["iv"]
    hmin = min(c.get("upper", (1.0, 1.0, 1.0))[d] / iv[d] for d in range(3))
    h.u = mesh.u_col(0.05 * hmin) if totlag else np.zeros(mesh.n_cols)
    f64 = dict(dtype=torch.float64, device=dev)
    h.ut = _t(h.u)
    h.K = torch.zeros(mesh.nnz, **f64)
    h.ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, h.ut, torch.zeros(mesh.n_rows, **f64), h.K)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        mg = mgm.Multigrid(mesh, h.ev, clamp, E, NU, min_intervals=c["mi"], max_levels=c.get("max_levels", 8),
                           ratio=RATIO, boost=BOOST, **opts)
    h.mg = mg
    h.rows = [np.asarray(l.rows) for l in mg.levels]
    h.ev.dirichlet_apply(_t(h.rows[0]), h.K)
    if opts.get("matrix_free"):
        mg.set_state(h.ut)
    mg._prepare(None if not mg.needs_matrix else h.K)
    torch.cuda.synchronize()
    h.meshes = [l.mesh for l in mg.levels]
    assert [tuple(int(m.box.interval[d]) for d in range(3)) for m in h.meshes[1:]] == c["levels"]
    for m, r in zip(h.meshes, h.rows):  # the solver's Dirichlet rows are the geometric face's
        assert np.array_equal(np.sort(r), mg_ref.node_rows(m, mg_ref.face_mask(m, 0, side)))
        assert np.array_equal(m.node_dof_row, 3 * np.arange(m.n_node))
    h.Kd = _dense(mesh, h.K.cpu().numpy())
    h.Klev = [h.Kd] + [_dense(l.mesh, l.K.cpu().numpy()) for l in mg.levels[1:]]
    h.masks = [mg_ref.mask_of(m, r) for m, r in zip(h.meshes, h.rows)]
    h.free = np.nonzero(h.masks[0])[0]
    h.lmax = [l.lmax for l in mg.levels]
    h.dinv = [l.dinv.cpu().numpy().reshape(-1, 3, 3) for l in mg.levels]
    h.cinv = None if mg.coarse_inv is None else mg.coarse_inv.cpu().numpy()
    if cache:
        _built[key] = h
    return h


def _stencils(h):
    """The level operators below the fine level as matrices, as the cycle applies them."""
    if getattr(h, "Ast", None) is None:
        h.Ast = [None] + [_sweep(l.spmv_exact, l.n, l.n, float("nan")) for l in h.mg.levels[1:]]
    return h.Ast


def _transfers(h):
    """(P, R) dense, as the cycle applies them (masks included), from the unit vectors."""
    if getattr(h, "Pd", None) is None:
        mg, L = h.mg, h.mg.levels
        h.Pd = [_sweep(lambda x, y, l=l: mg._prolong(l, x, y), L[l + 1].n, L[l].n, 0.0) for l in range(len(L) - 1)]
        h.Rd = [_sweep(lambda x, y, l=l: mg._restrict(l, x, y), L[l].n, L[l + 1].n, float("nan"))
                for l in range(len(L) - 1)]
    return h.Pd, h.Rd


_oracle_cache = {}


def _oracle_errors(mesh, rows):
    """(A_ld, SK, (e_n, e_c) of the float64 oracle) of a hex8 level with unit rows."""
    A, SK = mg_ref.level_operator(mesh, E, NU, rows)
    err, _, Kv, _ = oracle_evaluate(mesh, fcg.LINEAR, E, NU, np.zeros(mesh.n_cols))
    assert err == 0
    Ko = _dense(mesh, sr.apply_dirichlet_host(mesh, Kv, rows))
    return A, SK, (er.err_norm(Ko, A), er.err_comp(Ko, A, SK))


def _benign_floor(iv, side):
    key = (tuple(iv), side)
    if key not in _oracle_cache:
        m = _box(fcg.HEX8, iv, jitter=0.1)
        _oracle_cache[key] = _oracle_errors(m, mg_ref.node_rows(m, mg_ref.face_mask(m, 0, side)))[2]
    return _oracle_cache[key]


def _ratio(e, floor):
    return e / floor if floor > 0 else (0.0 if e == 0 else float("inf"))


@gpu
@pytest.mark.parametrize("name", ALL)
def test_describe_lists_decreasing_dofs(name):
    h = _build(name)
    d = h.mg.describe()
    dofs = [l["dofs"] for l in d]
    _say(test="describe", case=name, dofs=dofs, intervals=[l["intervals"] for l in d])
    assert all(a > b for a, b in zip(dofs, dofs[1:]))
    assert [tuple(l["intervals"]) for l in d[1:]] == CASES[name]["levels"]


@gpu
@pytest.mark.parametrize("name", ALL)
def test_stencil_as_a_matrix(name):
    h = _build(name)
    side = CASES[name].get("side", 0)
    Ast = _stencils(h)
    for l in range(1, len(h.mg.levels)):
        lvl, mesh, rows = h.mg.levels[l], h.meshes[l], h.rows[l]
        assert lvl.stencil is not None
        case = f"{name}/L{l}"
        q = Ast[l]
        A, SK, eo = _oracle_errors(mesh, rows)
        eA = _benign_floor(tuple(int(mesh.box.interval[d]) for d in range(3)), side)
        eg = (er.err_norm(q, A), er.err_comp(q, A, SK))
        ratio = [_ratio(eg[k], max(eo[k], eA[k])) for k in (0, 1)]
        # the level's block inverses (of the assembled K) against the stencil's own diagonal blocks
        D = mg_ref.diag_blocks(q).astype(LD)
        di = h.dinv[l].astype(LD)
        ninf = lambda M: np.abs(M).sum(axis=2).max(axis=1)  # noqa: E731
        kappa = (ninf(D) * ninf(mg_ref.block_inverses(q, LD))).astype(np.float64)
        ident = np.abs(np.matmul(di, D) - np.eye(3, dtype=LD)).max(axis=(1, 2)).astype(np.float64)
        # its two parts: the inverse against the assembled K's own block, and that block against
        # the stencil's (the same element contributions summed in another order)
        DK = mg_ref.diag_blocks(h.Klev[l]).astype(LD)
        ident_K = np.abs(np.matmul(di, DK) - np.eye(3, dtype=LD)).max(axis=(1, 2)).astype(np.float64)
        dD = (np.abs(D - DK).max(axis=(1, 2)) / np.abs(DK).max(axis=(1, 2))).astype(np.float64)
        margin, dmargin = MARGINS.get(case, 4.0), DINV_MARGINS.get(case, 4.0)
        _say(test="stencil", case=case, n=int(lvl.n), eo=eo, eA=eA, eg=eg, ratio=ratio, margin=margin,
             dinv_ident_over_kappa_u=_f((ident / (kappa * U)).max()), dinv_margin=dmargin,
             dinv_ident_own_block_over_kappa_u=_f((ident_K / (kappa * U)).max()),
             block_diff_u=_f(dD.max() / U), kappa_max=_f(kappa.max()))
        assert margin <= 64.0
        assert np.isfinite(q).all()
        assert np.array_equal(q[~mg_ref.pattern(mesh)], np.zeros((~mg_ref.pattern(mesh)).sum()))
        assert np.array_equal(q[rows], np.eye(lvl.n)[rows])  # unit rows
        assert np.isfinite(eo).all() and np.isfinite(eA).all()
        for r in ratio:
            assert np.isfinite(r) and not (r > margin), (case, ratio)
        assert dmargin <= 64.0 and (ident <= kappa * dmargin * U).all(), case


def _transfer_bound(Wabs, x, y0, length):
    return (length + 2) * U * (Wabs @ np.abs(x).astype(LD) + np.abs(y0).astype(LD))


def _check_transfer(case, what, got, W, x, y0, zero_rows, worst):
    """got against W x + y0 (longdouble W) by the per-entry bound; exact zeros on zero_rows."""
    assert np.isfinite(got).all(), (case, what)
    ref = W @ x.astype(LD) + y0.astype(LD)
    ref[zero_rows] = 0
    length = (W != 0).sum(axis=1)
    bound = _transfer_bound(np.abs(W), x, y0, length)
    err = np.abs(got.astype(LD) - ref)
    assert np.array_equal(got[zero_rows], np.zeros(len(zero_rows))), (case, what)
    keep = np.ones(len(ref), dtype=bool)
    keep[zero_rows] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
    worst.append((_f(rel[keep].max()) if keep.any() else 0.0, what))
    return rel[keep]


@gpu
@pytest.mark.parametrize("name,env", [(n, ()) for n in ALL] + [("h8_444", (("FCG_MG_BOXT", "0"),)),
                                                                ("h27_222", (("FCG_MG_BOXT", "0"),))],
                         ids=ALL + ["h8_444_tables", "h27_222_tables"])
def test_transfers_against_longdouble(name, env):
    """fcg_box_transfer (mask in the kernel) and fcg_node_transfer (no mask) on every pair of the
    case's hierarchy, both directions, accumulate on and off, x nonzero on the clamped rows."""
    h = _build(name, env=env)
    dev = _dev()
    mg = h.mg
    rng = np.random.default_rng(31)
    worst, fails = [], []
    for l in range(len(mg.levels) - 1):
        fm, cm = h.meshes[l], h.meshes[l + 1]
        P = mg_ref.prolongation(fm, cm)
        xc, xf = rng.standard_normal(cm.n_rows), rng.standard_normal(fm.n_rows)
        y0f = rng.standard_normal(fm.n_rows)
        assert np.abs(xc[h.rows[l + 1]]).min() > 0 and np.abs(xf[h.rows[l]]).min() > 0
        none = np.zeros(0, dtype=np.int64)
        nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
        runs = []
        if mg.BT[l] is not None:
            bt = mg.BT[l]
            assert mg.P[l] is None
            for acc in (1, 0):
                y = _t(y0f) if acc else nan(fm.n_rows)
                bt._run(0, bt.fzero, _t(xc), y, acc)
                runs.append((f"L{l} box prolong acc{acc}", y, P, xc, y0f if acc else 0 * y0f, h.rows[l]))
                # restriction overwrites whatever `accumulate` says (include/fourc_gpu.h)
                y = nan(cm.n_rows)
                bt._run(1, bt.czero, _t(xf), y, acc)
                runs.append((f"L{l} box restrict acc{acc}", y, P.T, xf, np.zeros(cm.n_rows), h.rows[l + 1]))
        else:
            for acc in (True, False):
                y = _t(y0f) if acc else nan(fm.n_rows)
                mg.P[l](_t(xc), y, accumulate=acc)
                runs.append((f"L{l} node prolong acc{int(acc)}", y, P, xc, y0f if acc else 0 * y0f, none))
                y0c = rng.standard_normal(cm.n_rows)
                y = _t(y0c) if acc else nan(cm.n_rows)
                mg.R[l](_t(xf), y, accumulate=acc)
                runs.append((f"L{l} node restrict acc{int(acc)}", y, P.T, xf, y0c if acc else 0 * y0c, none))
            # and as the cycle applies them: the mask after the kernel
            y = _t(y0f)
            mg._prolong(l, _t(xc), y)
            runs.append((f"L{l} cycle prolong", y, P, xc, y0f, h.rows[l]))
            y = nan(cm.n_rows)
            mg._restrict(l, _t(xf), y)
            runs.append((f"L{l} cycle restrict", y, P.T, xf, np.zeros(cm.n_rows), h.rows[l + 1]))
        torch.cuda.synchronize()
        for what, y, W, x, y0, zr in runs:
            rel = _check_transfer(name, what, y.cpu().numpy(), W, x, y0, np.asarray(zr, dtype=np.int64), worst)
            if not (rel <= 1).all():
                fails.append((what, _f(rel.max())))
    _say(test="transfers", case=name, env=dict(env), worst_err_over_bound=max(worst)[0], at=max(worst)[1],
         runs=len(worst))
    assert not fails, fails


def _terms(P, A):
    """Largest number of products in an entry of P^T A P."""
    Pb, Ab = (P != 0).astype(np.int64), (A != 0).astype(np.int64)
    return int((Pb.T @ Ab @ Pb).max())


@gpu
@pytest.mark.parametrize("name", [n for n in ALL if CASES[n]["nested"]])
def test_galerkin_identity_on_the_device(name):
    """The device's coarse stencil against P^T A_f P of the device's fine operator (K fetched on
    level 0, the stencil matrix below) with the longdouble P, on the free rows and columns."""
    h = _build(name)
    Ast = _stencils(h)
    recs = []
    for l in range(len(h.mg.levels) - 1):
        fm, cm = h.meshes[l], h.meshes[l + 1]
        P = mg_ref.prolongation(fm, cm)
        Af = (h.Kd if l == 0 else Ast[l]).astype(LD)
        Ac = Ast[l + 1].astype(LD)
        _, Sf = mg_ref.level_operator(fm, E, NU, h.rows[l])
        _, Sc = mg_ref.level_operator(cm, E, NU, h.rows[l + 1])
        Pa = np.abs(P)
        floor = gal_floor(fm, cm, P)
        bound = (_terms(P, Af) + 2) * U * (Pa.T @ np.abs(Af) @ Pa) + floor * (Pa.T @ Sf @ Pa + Sc)
        free = np.nonzero(h.masks[l + 1])[0]
        ix = np.ix_(free, free)
        err = np.abs(P.T @ Af @ P - Ac)[ix]
        b = bound[ix]
        assert (b[err > 0] > 0).all()
        rel = _f(np.where(b > 0, err / np.where(b > 0, b, 1), 0).max())
        recs.append(dict(level=l, err_over_bound=rel, terms=_terms(P, Af), floor_u=floor / U,
                         err_over_scale_u=er.err_comp(err, 0 * err, (Pa.T @ Sf @ Pa + Sc)[ix]) / U))
    _say(test="galerkin_device", case=name, levels=recs)
    assert all(r["err_over_bound"] <= 1 for r in recs), recs


@gpu
@pytest.mark.parametrize("name", ALL)
def test_coarsest_inverse_and_lambda_max(name):
    h = _build(name)
    A = h.Klev[-1]
    ref = samg_ref.inverse(A, LD)
    d_gpu, d_64 = _fro(h.cinv - ref), _fro(np.linalg.inv(A) - ref)
    Ast = _stencils(h)
    ratios = []
    for l in range(len(h.mg.levels) - 1):
        Al = h.Kd if l == 0 else Ast[l]
        free = np.nonzero(h.masks[l])[0]
        Aff = Al[np.ix_(free, free)]
        D = scipy.linalg.block_diag(*mg_ref.diag_blocks(Al))[np.ix_(free, free)]
        top = float(scipy.linalg.eigh(0.5 * (Aff + Aff.T), 0.5 * (D + D.T), eigvals_only=True)[-1])
        ratios.append(h.lmax[l] / top)
    _say(test="cinv_lmax", case=name, n_coarsest=int(A.shape[0]), d_gpu=d_gpu, d_64=d_64,
         d_ratio=_ratio(d_gpu, d_64), lmax_over_lambda_max=ratios)
    assert d_gpu <= CINV_MARGIN * d_64
    assert all(0 < r <= 1 + 1e-10 for r in ratios)
    assert h.lmax[-1] is None


# ------------------------------------------------------------------------------------ the cycle
def _ref_cycles(h, nu=2, mixed=False, stencil=True, **opts):
    """(float64, longdouble) mg_ref.Cycle from what the device holds.  float64: the device's block
    inverses and coarsest inverse; longdouble: the inverses of the same blocks and of the same
    coarsest K, refined."""
    Ast = _stencils(h) if stencil else h.Klev
    P, R = _transfers(h)
    A = [h.Kd] + [Ast[l] for l in range(1, len(h.Klev))]
    S = None
    if mixed:
        S = [h.Kd.astype(np.float32).astype(np.float64)] + A[1:]
    out = []
    for dt in (np.float64, LD):
        dinv = h.dinv if dt is np.float64 else [mg_ref.block_inverses(k, LD) for k in h.Klev]
        cinv = h.cinv if dt is np.float64 else samg_ref.inverse(h.Klev[-1], LD)
        out.append(mg_ref.Cycle(A, P, R, dinv, h.lmax, nu, RATIO, BOOST, dt, S=S, cinv=cinv, **opts))
    return out


def _device_M(h, cols):
    """Columns `cols` of the device's V-cycle: _vcycle(0, e_j, x) into a NaN-prefilled x."""
    dev = _dev()
    n = h.mesh.n_rows
    B = torch.zeros((len(cols), n), dtype=torch.float64, device=dev)
    B[torch.arange(len(cols), device=dev), _t(np.asarray(cols, dtype=np.int64))] = 1.0
    X = torch.full((len(cols), n), float("nan"), dtype=torch.float64, device=dev)
    for i in range(len(cols)):
        h.mg._vcycle(0, B[i], X[i])
    torch.cuda.synchronize()
    return np.ascontiguousarray(X.cpu().numpy().T)


def _device_apply(h, Bcols):
    dev = _dev()
    B = _t(np.ascontiguousarray(Bcols.T))
    X = torch.full(tuple(B.shape), float("nan"), dtype=torch.float64, device=dev)
    for i in range(B.shape[0]):
        h.mg._vcycle(0, B[i], X[i])
    torch.cuda.synchronize()
    return np.ascontiguousarray(X.cpu().numpy().T)


_ref_cache = {}


def _judge_cycle(label, h, ref_key, symmetric=True, eig_upper=None, **ref_opts):
    """The device cycle of build h against the reference with ref_opts: prints, then asserts the
    V-cycle bounds of the module docstring.  Returns (M_dev or z_dev, own)."""
    if ref_key not in _ref_cache:
        c64, cld = _ref_cycles(h, **ref_opts)
        if h.name == "h27_222":
            B = np.random.default_rng(77).standard_normal((h.mesh.n_rows, 16)) * h.masks[0][:, None]
            _ref_cache[ref_key] = (B, c64.apply(B), cld.apply(B))
        else:
            _ref_cache[ref_key] = (None, c64.matrix(h.free), cld.matrix(h.free))
    B, M64, Mld = _ref_cache[ref_key]
    eig_upper = CASES[h.name]["nested"] if eig_upper is None else eig_upper
    if B is not None:  # 16 seeded right-hand sides, judged columnwise
        Z = _device_apply(h, B)
        own = np.sqrt(((M64.astype(LD) - Mld) ** 2).sum(axis=0)).astype(np.float64)
        d = np.sqrt(((Z.astype(LD) - Mld) ** 2).sum(axis=0)).astype(np.float64)
        rz = (B * Z).sum(axis=0)
        _say(test="cycle", case=label, rows=int(h.mesh.n_rows), rhs=16, worst_d_over_own=_f((d / own).max()),
             own_max=_f(own.max()), min_rz=_f(rz.min()))
        assert np.isfinite(Z).all() and (own > 0).all()
        assert (d <= 8 * own).all(), (label, (d / own).max())
        assert (rz > 0).all()
        return Z, own
    M = _device_M(h, h.free)
    own = _fro(M64 - Mld)
    d = _fro(M - Mld)
    f = h.free
    Mff = M[f]
    asym = _fro(Mff - Mff.T)
    Aff = h.Kd[np.ix_(f, f)]
    ev = _spectrum(Mff, Aff)
    allowed = 1 + 8 * own * np.linalg.norm(Aff, 2)
    _say(test="cycle", case=label, rows=int(h.mesh.n_rows), d=d, own=own, d_over_own=_ratio(d, own), asym=asym,
         eig=[_f(ev.min()), _f(ev.max())], eig_allowed=allowed, symmetric=symmetric, eig_upper_asserted=eig_upper)
    assert np.isfinite(M).all() and own > 0
    assert np.array_equal(M[h.rows[0]], np.zeros((len(h.rows[0]), len(f))))  # nothing on the clamped rows
    assert d <= 8 * own, (label, d / own)
    if symmetric:
        assert asym <= 8 * own, (label, asym / own)
    assert ev.min() > 0
    if eig_upper and symmetric:
        assert ev.max() <= allowed
    return M, own


@gpu
@pytest.mark.parametrize("name", ALL)
def test_vcycle_as_a_matrix(name):
    h = _build(name)
    _judge_cycle(name, h, (name, "base"))


@gpu
@pytest.mark.parametrize("name", ["h8_422", "h8_444"])
@pytest.mark.parametrize("nu", [1, 3])
def test_vcycle_degree(name, nu):
    h = _build(name, nu=nu)
    _judge_cycle(f"{name} nu {nu}", h, (name, "nu", nu), nu=nu)


@gpu
@pytest.mark.parametrize("name", ["h8_422", "h8_444"])
def test_vcycle_without_fine_post_smoothing(name):
    h = _build(name, fine_post=False)
    M, own = _judge_cycle(f"{name} fine_post=False", h, (name, "nopost"), symmetric=False, fine_post=False)
    Mb, _ = _judge_cycle(name, _build(name), (name, "base"))
    assert _fro(M - Mb) > 8 * own  # the option took effect


@gpu
@pytest.mark.parametrize("name", DEEP)
@pytest.mark.parametrize("env,opts", [((("FCG_MG_CYCLE", "W"),), dict(cycle="W")),
                                      ((("FCG_MG_COARSE_NU", "1"),), dict(coarse_nu=1)),
                                      ((("FCG_MG_COARSE_NU", "1"), ("FCG_MG_CYCLE", "W")), dict(cycle="W", coarse_nu=1))],
                         ids=["W", "coarse_nu1", "W_coarse_nu1"])
def test_vcycle_w_cycle_and_coarse_degree(name, env, opts):
    h = _build(name, env=env)
    assert h.mg.cycle == opts.get("cycle", "V") and h.mg.coarse_nu == opts.get("coarse_nu")
    Z, own = _judge_cycle(f"{name} {opts}", h, (name,) + tuple(sorted(opts.items())), **opts)
    Zb, _ = _judge_cycle(name, _build(name), (name, "base"))
    diff = float(np.sqrt(((Z - Zb) ** 2).sum()))
    _say(test="cycle_option", case=f"{name} {opts}", diff_from_default=diff, own=_f(np.max(own)))
    # the option took effect.  A second coarse correction alone changes nothing on a nested
    # hierarchy: after an exact solve with the Galerkin operator the restricted residual is zero
    # (measured: |W - V|_F 2.3e-15 on h8_422, 7.4e-15 on h27_222), so W alone is told from V on
    # h8_533 only, whose (3,2,2) -> (2,1,1) pair is not nested
    if "coarse_nu" in opts or not CASES[name]["nested"]:
        assert diff > 8 * np.max(own)


@gpu
@pytest.mark.parametrize("name", ["h8_422", "h8_444", "h27_222"])
def test_vcycle_mixed(name):
    """mixed=True: the smoother reads K rounded to float32, the restricted residual stays float64."""
    h = _build(name, mixed=True)
    assert h.mg.levels[0].K32 is not None and h.mg.levels[0].K32.dtype == torch.float32
    # no symmetry: the smoother is a polynomial in D^-1 K32, the residual it corrects is K's
    Z, own = _judge_cycle(f"{name} mixed", h, (name, "mixed"), symmetric=False, mixed=True)
    Zb, ownb = _judge_cycle(name, _build(name), (name, "base"))
    diff = np.sqrt(((Z - Zb) ** 2).sum())
    _say(test="cycle_mixed", case=name, diff_from_unmixed=_f(diff), own=_f(np.max(own)))
    assert diff > np.max(own) and diff > np.max(ownb)
    # a residual restricted from the FP32 operator instead is another matrix, further from the
    # device than the bound allows: the reference can tell the two apart
    wrong = _ref_cycles(h, mixed=True)[1]
    wrong.A[0] = wrong.S[0]
    W = wrong.apply(_ref_cache[(name, "mixed")][0]) if name == "h27_222" else wrong.matrix(h.free)
    assert _fro(W - _ref_cache[(name, "mixed")][2]) > 8 * np.max(own) * (4 if name == "h27_222" else 1)


@gpu
@pytest.mark.parametrize("name", ["h8_422", "h8_444"])
@pytest.mark.parametrize("var", ["FCG_MG_STENCIL", "FCG_MG_BOXT", "FCG_MG_FUSED"])
def test_vcycle_switches(name, var, monkeypatch):
    """FCG_MG_STENCIL=0 (the assembled level K) and FCG_MG_BOXT=0 (the tables): within 8 own of the
    default, and of their own reference; FCG_MG_FUSED=0: bit-identical to the default."""
    hb = _build(name)
    Mb, ownb = _judge_cycle(name, hb, (name, "base"))
    if var == "FCG_MG_FUSED":
        monkeypatch.setenv(var, "0")  # read at every smoother call
        M = _device_M(hb, hb.free)
        same = bool(np.array_equal(M.view(np.uint64), Mb.view(np.uint64)))
        _say(test="cycle_switch", case=name, var=var, bit_identical=same, d=_fro(M - Mb))
        assert same
        return
    h = _build(name, env=((var, "0"),))
    if var == "FCG_MG_STENCIL":
        assert all(l.stencil is None for l in h.mg.levels)
        M, own = _judge_cycle(f"{name} {var}=0", h, (name, var), stencil=False)
    else:
        assert all(b is None for b in h.mg.BT) and all(p is not None for p in h.mg.P)
        M, own = _judge_cycle(f"{name} {var}=0", h, (name, var))
    d = _fro(M - Mb)
    _say(test="cycle_switch", case=name, var=var, d=d, own=ownb, d_over_own=d / ownb)
    assert d <= 8 * max(own, ownb)


@gpu
def test_vcycle_pcg_coarsest_level():
    """coarse_solver="pcg" is no fixed matrix: the coarsest residual meets coarse_rtol, and the
    cycle's output lies within the reference's spread between an exact coarse solve and one that is
    off by coarse_rtol: |z - z_exact| <= |L|_2 |A_c^-1|_2 coarse_rtol |b_c|, L the post-smoothing's
    propagator after the prolongation."""
    name = "h8_444"
    h = _build(name, coarse_solver="pcg")
    mg = h.mg
    assert mg.coarse_inv is None and not mg.graph_ok
    hb = _build(name)
    c64, cld = _ref_cycles(hb)
    Ac = h.Klev[-1].astype(LD)
    L = mg_ref.cheb(cld.S[0], cld.dinv[0], np.zeros_like(cld.P[0]), cld.P[0], h.lmax[0], 2, RATIO, BOOST, LD)
    nL = np.linalg.norm(L.astype(np.float64), 2)
    nAi = np.linalg.norm(np.linalg.inv(h.Klev[-1]), 2)
    rng = np.random.default_rng(5)
    dev = _dev()
    recs = []
    for _ in range(4):
        b = rng.standard_normal(h.mesh.n_rows) * h.masks[0]
        x = torch.full((h.mesh.n_rows,), float("nan"), dtype=torch.float64, device=dev)
        mg._vcycle(0, _t(b), x)
        torch.cuda.synchronize()
        bc, xc = mg.levels[-1].b.cpu().numpy().astype(LD), mg.levels[-1].x.cpu().numpy().astype(LD)
        res = _fro(Ac @ xc - bc) / _fro(bc)
        z = x.cpu().numpy()
        d = _fro(z - cld.apply(b))
        spread = nL * nAi * mg.coarse_rtol * _fro(bc)
        own = _fro(c64.apply(b) - cld.apply(b))
        recs.append(dict(coarse_res=res, d=d, spread=spread, own=own))
    _say(test="cycle_pcg", case=name, coarse_rtol=mg.coarse_rtol, runs=recs)
    for r in recs:
        assert r["coarse_res"] <= mg.coarse_rtol
        assert r["d"] <= r["spread"] + 8 * r["own"]
        assert r["d"] > 8 * r["own"]  # an iterative coarse solve, not the inverse


@gpu
@pytest.mark.parametrize("outer", [False, True], ids=["assembled_outer", "matrix_free_outer"])
def test_vcycle_matrix_free_fine_level(outer):
    """matrix_free=True on hex27 at a TotLag state of amplitude 0.05 h: the fine level applies
    fcg_tangent_apply (and, with outer_matrix_free, takes its blocks from fcg_tangent_diag); same
    bounds against the reference built from the assembled K of that state."""
    h = _build("h27_222", totlag=True, matrix_free=True, outer_matrix_free=outer)
    assert h.mg.levels[0].matrix_free and h.mg.needs_matrix == (not outer)
    _judge_cycle(f"h27_222 matrix_free outer={outer}", h, ("h27_222", "mf", outer))


# ------------------------------------------------------------------------------------ the solve
RTOL = 1e-10


def _true_res(Kd, b, x):
    r = b.astype(LD) - Kd.astype(LD) @ np.asarray(x).astype(LD)
    return _fro(r) / _fro(b)


def _solve(h, b, graph, monkeypatch, bt=None, xt=None):
    monkeypatch.setenv("FCG_MG_GRAPH", "1" if graph else "0")
    bt = _t(b) if bt is None else bt
    xt = torch.full_like(bt, float("nan")) if xt is None else xt
    it, rel = h.mg.solve(h.K, bt, xt, RTOL)
    torch.cuda.synchronize()
    return xt.cpu().numpy(), it, rel


def _replays(h, b, max_iter=200):
    c64, cld = _ref_cycles(h)
    x64, it64, h64 = mg_ref.fcg_replay(h.Kd, c64, b, RTOL, max_iter, np.float64)
    xld, itld, hld = mg_ref.fcg_replay(h.Kd, cld, b, RTOL, max_iter, LD)
    return (x64, it64, h64), (xld, itld, hld)


def _count_ok(it, it64, h64):
    if it == it64:
        return True
    k = min(it, it64)
    return abs(it - it64) == 1 and RTOL / 2 <= h64[k - 1] <= 2 * RTOL


@gpu
@pytest.mark.parametrize("name", ["h8_444", "h27_222"])
def test_flexible_cg_against_replay(name, monkeypatch):
    h = _build(name)
    b = np.random.default_rng(12).standard_normal(h.mesh.n_rows) * h.masks[0]
    (x64, it64, h64), (xld, itld, hld) = _replays(h, b)
    g = abs(_true_res(h.Kd, b, x64) - h64[-1])
    d_ref = float(np.linalg.norm((x64.astype(LD) - xld).astype(np.float64)))
    xg, itg, relg = _solve(h, b, True, monkeypatch)
    assert h.mg._graph["graph"] is not None
    xe, ite, rele = _solve(h, b, False, monkeypatch)
    tr_g, tr_e = _true_res(h.Kd, b, xg), _true_res(h.Kd, b, xe)
    same = bool(np.array_equal(xg.view(np.uint64), xe.view(np.uint64)))
    _say(test="fcg", case=name, it_graph=itg, it_eager=ite, it_f64=it64, it_ld=itld, rel_graph=relg,
         rel_eager=rele, true_graph=tr_g, true_eager=tr_e, g=g, replay_last=h64[-1],
         graph_vs_eager=float(np.linalg.norm(xg - xe)), f64_vs_ld=d_ref, bit_identical=same)
    for it, tr, rel in ((itg, tr_g, relg), (ite, tr_e, rele)):
        assert _count_ok(it, it64, h64), (it, it64, h64[-3:])
        assert rel <= RTOL and tr <= RTOL + 10 * g
    assert itg == ite
    assert np.linalg.norm(xg - xe) <= 10 * d_ref


@gpu
def test_captured_graph_is_reused_and_rebuilt(monkeypatch):
    """One Multigrid: solve; scale K in place by 2 and solve again into the same buffers (same
    graph, replayed); change the fine lambda_max and solve again (the graph's key changes).  Each
    solve matches eager launches by the bound above."""
    name = "h8_444"
    h = _build(name, cache=False)
    mg = h.mg
    b = np.random.default_rng(13).standard_normal(h.mesh.n_rows) * h.masks[0]
    (x64, it64, h64), (xld, _, _) = _replays(h, b)
    d_ref = float(np.linalg.norm((x64.astype(LD) - xld).astype(np.float64)))
    bt = _t(b)
    xt = torch.full_like(bt, float("nan"))
    recs = []

    def both(step, scale):
        xg, itg, _ = _solve(h, b, True, monkeypatch, bt, xt)
        key, graph = mg._graph["key"], mg._graph["graph"]
        xe, ite, _ = _solve(h, b, False, monkeypatch)
        assert mg._graph["graph"] is graph  # the eager solve leaves the captured one alone
        recs.append(dict(step=step, it_graph=itg, it_eager=ite, d=float(np.linalg.norm(xg - xe)),
                         bound=10 * d_ref / scale, bit_identical=bool(np.array_equal(xg, xe)),
                         true=_true_res(scale * h.Kd, b, xg)))
        return key, graph

    k1, g1 = both(1, 1.0)
    h.K.mul_(2.0)  # the same buffer: lambda_max of D^-1 K does not change, the block inverses do
    k2, g2 = both(2, 2.0)
    lm = mg.levels[0].lmax
    mg.levels[0].lmax = 1.03 * lm
    k3, g3 = both(3, 2.0)
    _say(test="fcg_graph_reuse", case=name, runs=recs, it_f64=it64, key_changed=[k2 != k1, k3 != k2])
    assert k2 == k1 and g2 is g1
    assert k3 != k2 and g3 is not g2 and k3[-1][0] == 1.03 * lm
    for r in recs:
        assert r["it_graph"] == r["it_eager"] and r["d"] <= r["bound"] and r["true"] <= 2 * RTOL
    assert _count_ok(recs[0]["it_graph"], it64, h64)
    h.ev.close()
