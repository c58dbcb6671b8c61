"""thermo_ref.py against things it shares no code with: the volume the capacity matrix sums to,
its symmetry, and the closed form of one-step-theta on the discrete cosine mode of an insulated box.

The cosine mode.  On an unjittered hex8 box of n elements of edge h along x (L = n h), all faces
insulated, T = Tbar + A cos(pi x / L) at the nodes is an eigenvector of (K_TT, C): the 1D stencils of
the trilinear element are (k/h)(-1, 2, -1) and (capa h/6)(1, 4, 1), the insulated ends halve both, so
with phi = pi h / L

    lambda = (k / capa) 6 (1 - cos phi) / (h^2 (2 + cos phi)),

and a one-step-theta step multiplies A by g = (1 - (1 - theta) dt lambda) / (1 + theta dt lambda) and leaves
Tbar alone (K 1 = 0)."""

import importlib

import numpy as np
import pytest

import thermo_ref as th
from element_ref import EXTENDED, LD

fcg = importlib.import_module("4c_amd").fcg

pytestmark = pytest.mark.skipif(not EXTENDED, reason="np.longdouble has no 64-bit significand here")

CAPA, COND = 3.5, 52.0


def _volume(mesh):
    """sum_e sum_g w_g det J_g from the oracle's own shape derivatives in float64."""
    import oracle_lib as orc
    xi, w = orc.gauss_points(mesh.celltype)
    vol = 0.0
    X = np.asarray(mesh.node_x)[np.asarray(mesh.ele_nodes)]
    for g in range(len(w)):
        dN = orc.shape_deriv(mesh.celltype, xi[g])
        J = np.einsum("ad,eak->edk", dN, X)
        vol += w[g] * np.linalg.det(J).sum()
    return vol


@pytest.mark.parametrize("celltype,iv", [(fcg.HEX8, (3, 3, 3)), (fcg.HEX27, (2, 2, 2))])
def test_capacity_sums_to_the_volume_and_is_symmetric(celltype, iv):
    mesh = fcg.BoxMesh(celltype, iv, jitter=0.1)
    g = fcg.TsiGraph(mesh)
    C, SC, mindet = th.capacity(mesh, g, CAPA)
    assert mindet > 0 and C.dtype == LD
    # the shape functions sum to 1, so the entries sum to capa times the integrated volume
    assert abs(float(C.sum()) - CAPA * _volume(mesh)) <= 1e-13 * CAPA
    Cd = th.dense(g.rowptr_tt, g.col_tt, C, g.n_cols_t)
    assert np.array_equal(Cd, Cd.T) or float(np.abs(Cd - Cd.T).max()) <= 8 * np.finfo(LD).eps * float(np.abs(Cd).max())
    assert (SC >= np.abs(C)).all()
    # the float64 restatement is the reference rounded, to a few units of float64
    C64 = th.capacity_f64(mesh, g, CAPA)
    assert C64.dtype == np.float64
    assert float((np.abs(C64 - C) / SC).max()) <= 64 * 2.0 ** -53
    # a per-element table scales element by element
    tab = np.where(np.arange(mesh.n_ele) % 2 == 0, CAPA, 2 * CAPA)
    Ct = th.capacity(mesh, g, tab)[0]
    assert abs(float(Ct.sum()) - float(th.capacity(mesh, g, tab - CAPA)[0].sum()) - CAPA) <= 1e-12 * CAPA


def test_combine_restatements_agree():
    mesh = fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1)
    g = fcg.TsiGraph(mesh)
    rng = np.random.default_rng(5)
    C = th.capacity_f64(mesh, g, CAPA)
    K = th.conduction(mesh, g, COND).astype(np.float64)
    T, f, h = 293 + rng.standard_normal(g.n_cols_t), rng.standard_normal(g.n_rows_t), rng.standard_normal(g.n_rows_t)
    Tn = T * (1 - 1e-9)
    r = th.combine(g, 0.5, 1e-3, C, T, Tn, h, K, f)
    K64, f64 = th.combine_f64(g, 0.5, 1e-3, C, T, Tn, h, K, f)
    assert float((np.abs(K64 - r["K"]) / r["SK"]).max()) <= 4 * 2.0 ** -53
    assert float((np.abs(f64 - r["f"]) / r["Sf"]).max()) <= 64 * 2.0 ** -53
    # T_n = T: the capacity term is exactly 0
    r0 = th.combine(g, 1.0, 1.0, C, T, T, None, K, f)
    assert np.array_equal(r0["f"], f.astype(LD))


@pytest.mark.parametrize("theta", [0.5, 2.0 / 3.0, 1.0])
def test_cosine_mode_closed_form(theta):
    n, L, dt, A0, Tbar, nstep = 6, 3.0, 0.01, 25.0, 300.0, 8
    mesh = fcg.BoxMesh(fcg.HEX8, (n, 2, 2), lower=(0.0, 0.0, 0.0), upper=(L, 1.0, 1.0))
    g = fcg.TsiGraph(mesh)
    nt = g.n_rows_t
    K = th.dense(g.rowptr_tt, g.col_tt, th.conduction(mesh, g, COND), nt)
    C = th.dense(g.rowptr_tt, g.col_tt, th.capacity(mesh, g, CAPA)[0], nt)
    x = np.zeros(nt, dtype=LD)
    x[np.asarray(g.node_dof_col_t)] = np.asarray(mesh.node_x)[:, 0]
    pi = 4 * np.arctan(LD(1))
    mode = np.cos(pi * x / LD(L))
    h = LD(L) / n
    phi = pi * h / LD(L)
    lam = LD(COND) / LD(CAPA) * 6 * (1 - np.cos(phi)) / (h * h * (2 + np.cos(phi)))
    # the mode is an eigenvector of the reference matrices
    assert float(np.abs(K @ mode - lam * (C @ mode)).max()) <= 1e-15 * float(np.abs(K @ mode).max())
    gfac = (1 - (1 - LD(theta)) * LD(dt) * lam) / (1 + LD(theta) * LD(dt) * lam)
    assert abs(gfac) <= 1
    T = th.ost_dense(K, C, theta, dt, Tbar + A0 * mode, np.zeros(nt), [], nstep)
    for k in range(nstep + 1):
        want = Tbar + A0 * gfac ** k * mode
        assert float(np.abs(T[k] - want).max()) <= 1e-13 * float(np.abs(want).max()), (theta, k)
