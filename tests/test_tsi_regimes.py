"""The TSI blocks on the device -- the two-kernel path (fcg_tsi_evaluate_device after the structural
evaluate) and the fused structured sweep (fcg_tsi_evaluate_fused, as the default split pair of
passes and as the one fused pass, FCG_TSI_SPLIT=0) -- outside the benign regime, judged against
the extended-precision reference of tsi_ref.py.

Criterion: the one of test_evaluate_regimes.py (its docstring gives the reason for the factor).
For K_SS, K_ST, K_TS, K_TT, f_S and f_T, with both measures e_n and e_c,

    e(device) <= 4 * max(e(o), e_A(o)),

o the float64 oracle on the same inputs (parity_util.oracle_tsi_evaluate), e_A its error in
regime A on the same mesh.  The fused pass forms the two residuals from the assembled blocks,
f_T = K_TT T and f_S = K_SS u + K_ST (T - T_0), where the oracle and the two-kernel path form
k grad N . grad T and T_g - T_0 at the Gauss points.  That is another formula with its own
rounding (T ~ 300 against rows that sum to 0), so for the fused configurations the float64
comparison value of the residuals is also formed the way the pass documents it, from the oracle's
float64 blocks with each row summed in CSR order in float64 on the CPU (o'), and the floor is
max(e(o), e(o')), in this case and in regime A.  MARGINS is empty; an entry needs a written cause
in profiles/tsi_regimes/README.md and is capped at 64.

Every case also asserts finite output and finite measures (regimes_util.judge), the path the
structural context landed on, that two evaluates agree bit for bit, and that the reference
reports det J > 0 at every Gauss point and node (and the oracle err == 0) before the device is
looked at.

Configurations (the smallest shapes at which the code can still go wrong):
  h8_two          BoxMesh hex8 (5,3,2), structural evaluate + evaluate_device(TSI_ALL)
  h8r_two         the same, Discretization.renumbered (input-file numbering)
  h27_two         hex27 (2,2,2): one row with all 125 neighbour nodes the LDS row image is sized for
  h27_rank0/1     hex27 (2,2,4) over 2 ranks: a 125-neighbour owned row beside ghost nodes
  h8_fused_split, h8_fused_one   hex8 (6,5,3): 7 x 6 node columns = 2 x 2 sweep tiles
  h8_fused_rank   (6,5,4) rank 1 of 2
  h8_fused_input_split / _one   (6,5,3) with one interior element column removed (a hole along
                  z), nodes and elements renumbered, three element frames rotated, no lattice
                  hint: PATH_AUTO must land on the structured sweep

Regimes.  Base: E = 210, nu = 0.3, alpha = 1.2e-5, T_0 = 293, k = 52, (timefac, timefac_d) =
(0.5, 3.7), jitter 0.1, u of amplitude 0.05 h; v (1e-2) and T (T_0 +- 50) smooth in the position.
  A              benign
  T_uniform      T = T_0 + 1e-6 x the field: the state of a converged thermal Newton step
  T0_zero        T_0 = 0, T = 20 +- 5
  v_zero         v = 0
  v_large        v of the scale 1e3
  nu0.49999, nu-0.5
  D_1e4_rotated, H_thin, E_SI   geometry and units of test_evaluate_regimes.py
  micro          element edge 3e-5: det J ~ 3e-15, just above the thermo element's 1e-16

Each test prints "REGIMES {json}" (regimes_util.judge) and, before it, "REGIMES_TSI {json}" with
e(o) and e(o') of the residuals.
"""

import functools
import importlib
import json

import numpy as np
import pytest

import regimes_util
import tsi_ref as tr
from parity_util import oracle_tsi_evaluate
from regimes_util import _entry, _measures

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not tr.er.EXTENDED, reason="np.longdouble has no 64-bit significand here")]

TIMEFAC, TIMEFAC_D = 0.5, 3.7
NAMES = tr.TsiAssembled.NAMES

# mesh name -> (cell type, intervals, rank, nranks, "box" | "renumbered" | "input")
MESHES = {"h8": (fcg.HEX8, (5, 3, 2), 0, 1, "box"), "h8r": (fcg.HEX8, (5, 3, 2), 0, 1, "renumbered"),
          "h27": (fcg.HEX27, (2, 2, 2), 0, 1, "box"),
          "h27_rank0": (fcg.HEX27, (2, 2, 4), 0, 2, "box"), "h27_rank1": (fcg.HEX27, (2, 2, 4), 1, 2, "box"),
          "h8f": (fcg.HEX8, (6, 5, 3), 0, 1, "box"), "h8f_rank": (fcg.HEX8, (6, 5, 4), 1, 2, "box"),
          "h8f_input": (fcg.HEX8, (6, 5, 3), 0, 1, "input")}
# configuration -> (mesh, path asked for, path the context must land on, fused, FCG_TSI_SPLIT)
S, GA, GE, AUTO = fcg.PATH_STRUCTURED, fcg.PATH_GATHER, fcg.PATH_GENERAL, fcg.PATH_AUTO
CONFIGS = {"h8_two": ("h8", S, S, False, None), "h8r_two": ("h8r", GA, GA, False, None),
           "h27_two": ("h27", GE, GE, False, None),
           "h27_rank0": ("h27_rank0", GE, GE, False, None), "h27_rank1": ("h27_rank1", GE, GE, False, None),
           "h8_fused_split": ("h8f", S, S, True, None), "h8_fused_one": ("h8f", S, S, True, "0"),
           "h8_fused_rank": ("h8f_rank", S, S, True, None),
           "h8_fused_input_split": ("h8f_input", AUTO, S, True, None),
           "h8_fused_input_one": ("h8f_input", AUTO, S, True, "0")}

BENIGN = dict(E=210.0, nu=0.3, alpha=1.2e-5, T0=293.0, k=52.0, lower=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0),
              rotation=(0.0, 0.0, 0.0), jitter=0.1, amp=0.05, T_mean=293.0, T_amp=50.0, v_amp=1e-2,
              field_scale=1.0, edge=None)
REGIMES = {
    "A": {},
    "T_uniform": dict(T_amp=50e-6),
    "T0_zero": dict(T0=0.0, T_mean=20.0, T_amp=5.0),
    "v_zero": dict(v_amp=0.0),
    "v_large": dict(v_amp=1e3),
    "nu0.49999": dict(nu=0.49999),
    "nu-0.5": dict(nu=-0.5),
    "D_1e4_rotated": dict(lower=(1e4, -2e4, 3e4), rotation=(0.3, 0.5, 0.7)),
    "H_thin": dict(size=(1.0, 1.0, 1e-3)),
    "E_SI": dict(E=2.1e11, size=(1e-3, 1e-3, 1e-3), field_scale=1e-3),
    "micro": dict(edge=3e-5),
}

# case id -> margin in place of 4 (at most 64); causes in profiles/tsi_regimes/README.md
MARGINS = {}


def _params(regime, iv):
    p = dict(BENIGN)
    p.update(REGIMES[regime])
    if p["edge"] is not None:   # the box that many elements of that edge fill; fields over its extent
        p["size"] = tuple(p["edge"] * n for n in iv)
        p["field_scale"] = p["size"]
    return p


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


# ------------------------------------------------------------------------------ meshes
def input_mesh(box, hole=(2, 2), seed=7):
    """The box as an input file could describe it: the element column at lattice (i, j) = hole
    removed (a hole along z; every node stays in use), nodes and elements renumbered at random,
    three element frames rotated (4C's numbering turned about a local axis), no lattice hint."""
    ijk = np.asarray(box.ele_ijk)
    keep = ~((ijk[:, 0] == hole[0]) & (ijk[:, 1] == hole[1]))
    assert 0 < (~keep).sum() == ijk[:, 2].max() + 1
    rng = np.random.default_rng(seed)
    perm = rng.permutation(box.n_node)           # new number of every box node
    X = np.empty_like(np.asarray(box.node_x))
    X[perm] = box.node_x
    en = perm[np.asarray(box.ele_nodes)[keep]]
    en = en[rng.permutation(len(en))]
    assert len(np.unique(en)) == box.n_node
    en[0, :4] = np.roll(en[0, :4], 1)
    en[0, 4:] = np.roll(en[0, 4:], 1)
    en[5] = en[5][[1, 5, 6, 2, 0, 4, 7, 3]]
    en[9] = en[9][[4, 7, 6, 5, 0, 3, 2, 1]]
    dis = fcg.Discretization.from_elements(fcg.HEX8, en, X)
    assert dis.ele_ijk is None
    return dis


@functools.lru_cache(maxsize=None)
def _mesh(name, lower, size, rotation, jitter):
    celltype, iv, rank, nranks, kind = MESHES[name]
    upper = tuple(lo + s for lo, s in zip(lower, size))
    box = fcg.BoxMesh(celltype, iv, lower=lower, upper=upper, rotation=rotation, jitter=jitter,
                      rank=rank, nranks=nranks)
    if kind == "renumbered":
        return fcg.Discretization.renumbered(box, seed=3)
    if kind == "input":
        return input_mesh(box)
    return box


def _check_shape_of_mesh(name, mesh, g):
    """What makes the configuration the smallest that can still go wrong."""
    rows = np.diff(g.rowptr_tt)
    if name == "h27":
        assert rows.max() == 125
    if name.startswith("h27_rank"):
        assert rows.max() == 125 and (np.asarray(mesh.node_dof_row) < 0).any()
    if name == "h8f_rank":
        assert (np.asarray(mesh.node_dof_row) < 0).any()
    if name.startswith("h8f"):
        assert rows.max() == 27


def _csr_rows_f64(rowptr, col, vals, x, acc):
    """acc[r] += sum_j vals[j] x[col[j]], every row in CSR order, in float64."""
    rowptr = np.asarray(rowptr)
    start, n = rowptr[:-1], np.diff(rowptr)
    for k in range(int(n.max(initial=0))):
        sel = n > k
        j = start[sel] + k
        acc[sel] += vals[j] * x[col[j]]
    return acc


# ------------------------------------------------------------------------------ the problem
@functools.lru_cache(maxsize=None)
def _problem(meshname, regime):
    """dict(mesh, g, p, u, v, T_col, ref, two, fused, extra): the state, the reference, and
    label -> dict(r, S, eo) for the two-kernel path (eo = e(o)) and for the fused pass
    (eo = max(e(o), e(o')) for the residuals).  The validity conditions are asserted here."""
    p = _params(regime, MESHES[meshname][1])
    mesh = _mesh(meshname, p["lower"], p["size"], p["rotation"], p["jitter"])
    g = fcg.TsiGraph(mesh)
    _check_shape_of_mesh(meshname, mesh, g)
    h = min(s / n for s, n in zip(p["size"], MESHES[meshname][1]))
    u, v, Tn = tr.smooth_fields(mesh, T_mean=p["T_mean"], amp_u=p["amp"] * h, amp_v=p["v_amp"],
                                amp_T=p["T_amp"], scale=p["field_scale"])
    ref = tr.assemble_tsi_ld(mesh, g, p["E"], p["nu"], p["alpha"], p["T0"], p["k"], TIMEFAC, TIMEFAC_D,
                             u, v, Tn)
    assert ref.min_detJ > 0 and ref.min_detJ_node > 0, (ref.min_detJ, ref.min_detJ_node)
    if regime == "micro":
        assert 1e-16 < ref.min_detJ < 1e-14, ref.min_detJ
    err, *o = oracle_tsi_evaluate(tr.oracle_view(mesh), g, p["E"], p["nu"], p["alpha"], p["T0"], p["k"],
                                  TIMEFAC, TIMEFAC_D, u, v, Tn)
    assert err == 0
    o = dict(zip(NAMES, o))
    T_col = np.zeros(g.n_cols_t)
    T_col[g.node_dof_col_t] = Tn
    two = {k: _entry(r, Sk, o[k]) for k, (r, Sk) in ref.pairs().items()}
    # the residuals as the fused pass documents them, from the oracle's float64 blocks
    fT1 = _csr_rows_f64(g.rowptr_tt, g.col_tt, o["Ktt"], T_col, np.zeros(g.n_rows_t))
    fs1 = _csr_rows_f64(mesh.rowptr, mesh.col_lid, o["Kss"], u, np.zeros(mesh.n_rows))
    fs1 = _csr_rows_f64(g.rowptr_st, g.col_st, o["Kst"], T_col - p["T0"], fs1)
    fused = {k: dict(e) for k, e in two.items()}
    extra = {}
    for k, x in (("fs", fs1), ("fT", fT1)):
        r, Sk = ref.pairs()[k]
        e1 = _measures(x, r, Sk)
        extra[k] = dict(eo=two[k]["eo"], eo_prime=e1)
        fused[k]["eo"] = tuple(max(a, b) for a, b in zip(two[k]["eo"], e1))
    return dict(mesh=mesh, g=g, p=p, u=u, v=v, T_col=T_col, ref=ref, two=two, fused=fused, extra=extra)


# ------------------------------------------------------------------------------ the device
def _device_two(ev, tev, P):
    mesh, g = P["mesh"], P["g"]
    ut, vt, Tt = _t(P["u"]), _t(P["v"]), _t(P["T_col"])
    runs = []
    for _ in range(2):
        o = dict(Kss=_nan(mesh.nnz), fs=_nan(mesh.n_rows), Kst=_nan(g.nnz_st), Kts=_nan(g.nnz_ts),
                 Ktt=_nan(g.nnz_tt), fT=_nan(g.n_rows_t))
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, ut, o["fs"], o["Kss"])
        tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, vt, Tt, TIMEFAC, TIMEFAC_D, fs=o["fs"],
                            Kst=o["Kst"], fT=o["fT"], Ktt=o["Ktt"], Kts=o["Kts"])
        torch.cuda.synchronize()
        runs.append(o)
    return runs


def _device_fused(ev, tev, P):
    mesh, g = P["mesh"], P["g"]
    ut, vt, Tt = _t(P["u"]), _t(P["v"]), _t(P["T_col"])
    runs = []
    for _ in range(2):
        o = dict(Kss=_nan(mesh.nnz), fs=_nan(mesh.n_rows), Kst=_nan(g.nnz_st), Kts=_nan(g.nnz_ts),
                 Ktt=_nan(g.nnz_tt), fT=_nan(g.n_rows_t))
        tev.evaluate_fused(ev, fcg.OVERWRITE, ut, vt, Tt, TIMEFAC, TIMEFAC_D, **o)
        torch.cuda.synchronize()
        runs.append(o)
    return runs


CASES = [(c, r) for c in CONFIGS for r in REGIMES]


@pytest.mark.parametrize("config,regime", CASES)
def test_tsi_regime(config, regime, monkeypatch):
    _dev()
    meshname, path, landed, is_fused, split = CONFIGS[config]
    P = _problem(meshname, regime)
    A = _problem(meshname, "A")
    if split is None:
        monkeypatch.delenv("FCG_TSI_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FCG_TSI_SPLIT", split)
    p, mesh = P["p"], P["mesh"]
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=p["E"], poisson=p["nu"], path=path)
    assert ev.info.path == landed
    tev = fcg.TsiEvaluator(mesh, p["E"], p["nu"], p["alpha"], p["T0"], p["k"], graph=P["g"])
    runs = (_device_fused if is_fused else _device_two)(ev, tev, P)
    for k in NAMES:
        assert torch.equal(runs[0][k], runs[1][k]), k
    got = {k: runs[0][k].cpu().numpy() for k in NAMES}
    tev.close()
    ev.close()
    case = f"tsi/{config}/{regime}"
    print("REGIMES_TSI " + json.dumps(dict(case=case, q=P["extra"], qA=A["extra"])))
    key = "fused" if is_fused else "two"
    regimes_util.judge(case, P[key], A[key], got, MARGINS)
