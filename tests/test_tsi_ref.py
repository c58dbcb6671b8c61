"""tsi_ref.py, the extended-precision TSI reference, pinned on the CPU: against the oracle's element
routines, by identities that hold independently of the oracle, and assembled against the oracle's
TSI::Monolithic element loop.  Each test prints its figures (in units of u = 2^-53, or of the
longdouble epsilon) before it asserts."""

import importlib

import numpy as np
import pytest

import oracle_lib as orc
import tsi_ref as tr
from parity_util import oracle_tsi_evaluate
from tsi_ref import EPS_LD, LD, U

fcg = importlib.import_module("4c_amd").fcg

pytestmark = pytest.mark.skipif(not tr.er.EXTENDED, reason="np.longdouble has no 64-bit significand here")

E, NU, ALPHA, T0, COND = 210.0, 0.3, 1.2e-5, 293.0, 52.0
TIMEFAC, TIMEFAC_D = 0.5, 3.7
QUANTITIES = ("Kst", "Kts", "Ktt", "fT", "fSth")


def _element(celltype, seed):
    """One jittered element (edge 1) with random velocity and a temperature near T_0."""
    rng = np.random.default_rng(seed)
    P = orc.node_param_coords(celltype)
    npe = len(P)
    X = 0.5 * P + (0.08 if celltype == fcg.HEX8 else 0.04) * rng.uniform(-1, 1, (npe, 3))
    v = 1e-2 * rng.standard_normal((npe, 3))
    T = T0 + 50.0 * rng.uniform(-1, 1, npe)
    return X, v, T


def _element_ld(celltype, X, v, T, timefac=TIMEFAC, timefac_d=TIMEFAC_D):
    m = tr.st_modulus_ld(E, NU, ALPHA)
    return tr.elements_tsi_ld(celltype, m, COND, T0, timefac, timefac_d, X[None], v[None], T[None])


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("celltype", [fcg.HEX8, fcg.HEX27])
def test_element_reference_against_oracle(celltype, seed):
    """The five element quantities against orc.tsi_solid_evaluate (at u = 0, where its f is the
    thermal part alone) and orc.tsi_thermo_evaluate: e_c <= 128 u."""
    X, v, T = _element(celltype, seed)
    el = _element_ld(celltype, X, v, T)
    assert el["detJ"].min() > 0 and el["detJ_node"].min() > 0
    npe = len(X)
    err, _, fe, Kst = orc.tsi_solid_evaluate(celltype, E, NU, ALPHA, T0, X, np.zeros((npe, 3)), T)
    assert err == 0
    m64 = orc.st_modulus(E, NU, ALPHA)
    assert abs(LD(m64) - tr.st_modulus_ld(E, NU, ALPHA)) <= 4 * U * abs(m64)
    err, Ktt, fT, Kts = orc.tsi_thermo_evaluate(celltype, COND, m64, X, T, v, TIMEFAC, TIMEFAC_D)
    assert err == 0
    got = dict(Kst=Kst, Kts=Kts, Ktt=Ktt, fT=fT, fSth=fe)
    fig = {}
    for q in QUANTITIES:
        assert np.asarray(got[q]).shape == el[q][0].shape, q
        fig[q] = (tr.err_comp(got[q], el[q][0], el["S" + q][0]) / U,
                  tr.err_norm(got[q], el[q][0]) / U)
    print(f"TSI_REF element celltype={celltype} seed={seed} (e_c / u, e_n / u): "
          + ", ".join(f"{q} {a:.1f} {b:.1f}" for q, (a, b) in fig.items()))
    for q, (ec, _) in fig.items():
        assert ec <= 128, (q, ec)


@pytest.mark.parametrize("celltype", [fcg.HEX8, fcg.HEX27])
def test_element_reference_identities(celltype):
    """Identities of the five formulas, in longdouble, each to 64 eps_LD of its scale:
    K_TT T = f_T (scale S f_T, which equals S K_TT |T| term by term);
    K_ST (T - T_0 1) = f_S^th by the partition of unity (scale S K_ST (|T| + |T_0|), the terms
    that the product rounds; for hex8 this is S f_S^th);
    K_TS(:, bj) = timefac timefac_d (f_T(v + e_bj) - f_T(v)), f_T being affine in v (scale
    S K_TS + timefac timefac_d (S f_T(v + e_bj) + S f_T(v)): the difference rounds both);
    at v = 0 K_TT is symmetric with zero row sums (scales S K_TT and its row sums)."""
    X, v, T = _element(celltype, 3)
    npe = len(X)
    el = _element_ld(celltype, X, v, T)
    tol = 64 * EPS_LD
    Tl = np.asarray(T, dtype=LD)
    fig = {}
    fig["Ktt T = fT"] = tr.err_comp(el["Ktt"][0] @ Tl, el["fT"][0], el["SfT"][0])
    fig["Kst (T - T0) = fSth"] = tr.err_comp(el["Kst"][0] @ (Tl - LD(T0)), el["fSth"][0],
                                             el["SKst"][0] @ (np.abs(Tl) + abs(LD(T0))))
    # f_T at v and at v + e_bj for every structural DOF: one batch of 3 npe + 1 "elements"
    vs = np.repeat(v[None], 3 * npe + 1, axis=0)
    for p in range(3 * npe):
        vs[p + 1, p // 3, p % 3] += 1.0
    m = tr.st_modulus_ld(E, NU, ALPHA)
    batch = tr.elements_tsi_ld(celltype, m, COND, T0, TIMEFAC, TIMEFAC_D,
                               np.repeat(X[None], len(vs), axis=0), vs, np.repeat(T[None], len(vs), axis=0))
    tf = LD(TIMEFAC) * LD(TIMEFAC_D)
    fd = tf * (batch["fT"][1:] - batch["fT"][0]).T                       # [a][bj]
    Sfd = el["SKts"][0] + tf * (batch["SfT"][1:] + batch["SfT"][0]).T
    fig["Kts = tf tfd dfT/dv"] = tr.err_comp(el["Kts"][0], fd, Sfd)
    el0 = _element_ld(celltype, X, np.zeros_like(v), T)
    fig["Ktt(v=0) symmetric"] = tr.err_comp(el0["Ktt"][0], el0["Ktt"][0].T, el0["SKtt"][0])
    fig["Ktt(v=0) row sums"] = tr.err_comp(el0["Ktt"][0].sum(axis=1), np.zeros(npe, dtype=LD),
                                           el0["SKtt"][0].sum(axis=1))
    print(f"TSI_REF identities celltype={celltype} (e_c / eps_LD): "
          + ", ".join(f"{k} {x / EPS_LD:.2f}" for k, x in fig.items()))
    for k, x in fig.items():
        assert x <= tol, (k, x / EPS_LD)
    # the thermoelastic term is there at all: K_TT(v) differs from K_TT(0), K_TS is not zero
    assert np.abs(el["Ktt"][0] - el0["Ktt"][0]).max() > 0 and np.abs(el["Kts"][0]).max() > 0


@pytest.mark.parametrize("celltype,iv,rank,nranks", [(fcg.HEX8, (3, 2, 2), 0, 1), (fcg.HEX27, (2, 2, 1), 0, 1),
                                                     (fcg.HEX8, (3, 2, 2), 0, 2), (fcg.HEX8, (3, 2, 2), 1, 2)])
def test_assembled_reference_against_oracle(celltype, iv, rank, nranks):
    """All six assembled quantities against parity_util.oracle_tsi_evaluate: e_c <= 256 u."""
    mesh = fcg.BoxMesh(celltype, iv, jitter=0.1, seed=5, rank=rank, nranks=nranks)
    g = fcg.TsiGraph(mesh)
    u, v, Tn = tr.smooth_fields(mesh, T_mean=T0)
    ref = tr.assemble_tsi_ld(mesh, g, E, NU, ALPHA, T0, COND, TIMEFAC, TIMEFAC_D, u, v, Tn)
    assert ref.min_detJ > 0 and ref.min_detJ_node > 0
    if nranks > 1:
        assert (np.asarray(mesh.node_dof_row) < 0).any()   # ghost nodes: columns without rows
    err, *o = oracle_tsi_evaluate(mesh, g, E, NU, ALPHA, T0, COND, TIMEFAC, TIMEFAC_D, u, v, Tn)
    assert err == 0
    fig = {}
    for (name, (r, S)), x in zip(ref.pairs().items(), o):
        assert x.shape == r.shape, name
        fig[name] = (tr.err_comp(x, r, S) / U, tr.err_norm(x, r) / U)
    print(f"TSI_REF assembled celltype={celltype} iv={iv} rank={rank}/{nranks} (e_c / u, e_n / u): "
          + ", ".join(f"{q} {a:.1f} {b:.1f}" for q, (a, b) in fig.items()))
    for q, (ec, _) in fig.items():
        assert ec <= 256, (q, ec)
