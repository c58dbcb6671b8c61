"""The calling contract of the TSI evaluates on the device: every subset of `parts` in both modes
(requested outputs as a full evaluate gives them, everything else untouched, unrequested pointers
NULL, f_S always `+=`), the time factors of k_TS, and the refusals (an inverted element, a mesh
below the thermo element's det J < 1e-16) with the oracle's code and the lowest bad element.
The values themselves are judged in test_tsi_regimes.py; here outputs are compared bit for bit.

hex8 (3,3,2) and hex27 (2,2,2), jitter 0.1.
"""

import functools
import importlib

import numpy as np
import pytest

import oracle_lib as orc
import tsi_ref as tr
from parity_util import oracle_tsi_evaluate

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

E, NU, ALPHA, T0, COND = 210.0, 0.3, 1.2e-5, 293.0, 52.0
TIMEFAC, TIMEFAC_D = 0.5, 3.7
FS, ST, TT, TS = 1, 2, 4, 8   # FCG_TSI_STRUCT_FORCE, _STIFFTEMP, _THERMO_FINTCOND, _COUPLTANG
OUTPUT_OF = {"fs": FS, "Kst": ST, "Ktt": TT, "fT": TT, "Kts": TS}
IV = {fcg.HEX8: (3, 3, 2), fcg.HEX27: (2, 2, 2)}
U = 2.0 ** -53


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


@functools.lru_cache(maxsize=None)
def _setup(celltype):
    """(mesh, graph, state A, state B, prefill): states as (v_col, T_col)."""
    mesh = fcg.BoxMesh(celltype, IV[celltype], jitter=0.1, seed=4)
    g = fcg.TsiGraph(mesh)

    def state(**kw):
        _, v, Tn = tr.smooth_fields(mesh, **kw)
        T_col = np.zeros(g.n_cols_t)
        T_col[g.node_dof_col_t] = Tn
        return v, T_col

    rng = np.random.default_rng(9)
    prefill = {k: rng.standard_normal(n) for k, n in _sizes(mesh, g).items()}
    return mesh, g, state(T_mean=T0), state(T_mean=310.0, amp_v=3e-2, amp_T=20.0), prefill


def _sizes(mesh, g):
    return dict(fs=mesh.n_rows, Kst=g.nnz_st, Ktt=g.nnz_tt, fT=g.n_rows_t, Kts=g.nnz_ts)


def _tev(mesh, g):
    return fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND, graph=g)


def _run(tev, parts, mode, state, prefill, timefac=TIMEFAC, timefac_d=TIMEFAC_D, drop=False):
    """One evaluate_device into buffers holding `prefill`; drop: the unrequested output pointers
    (and v_col unless FINTCOND is asked) are None.  Returns name -> numpy array or None."""
    v, T_col = state
    bufs = {k: (None if drop and not parts & OUTPUT_OF[k] else _t(prefill[k])) for k in OUTPUT_OF}
    vt = None if drop and not parts & TT else _t(v)
    tev.evaluate_device(parts, mode, vt, _t(T_col), timefac, timefac_d, **bufs)
    torch.cuda.synchronize()
    return {k: (None if b is None else b.cpu().numpy()) for k, b in bufs.items()}


@functools.lru_cache(maxsize=None)
def _fresh_all(celltype, mode, zero=False, timefac=TIMEFAC, timefac_d=TIMEFAC_D):
    """TSI_ALL on a fresh context at state A from the prefill (or from zeros)."""
    mesh, g, A, _, prefill = _setup(celltype)
    if zero:
        prefill = {k: np.zeros_like(x) for k, x in prefill.items()}
    tev = _tev(mesh, g)
    out = _run(tev, fcg.TSI_ALL, mode, A, prefill, timefac, timefac_d)
    tev.close()
    assert all(np.isfinite(x).all() for x in out.values())
    return out


# ------------------------------------------------------------------------------ subsets of parts
@pytest.mark.parametrize("parts", range(1, 16))
@pytest.mark.parametrize("mode", [fcg.OVERWRITE, fcg.ACCUMULATE])
@pytest.mark.parametrize("celltype", [fcg.HEX8, fcg.HEX27])
def test_parts_subset(celltype, mode, parts):
    """A subset of the parts on a context whose scratch records hold another state's full
    evaluate: the requested outputs are bit for bit those of TSI_ALL on a fresh context from the
    same prefill, the others keep their prefill, and the unrequested pointers may be NULL."""
    _dev()
    mesh, g, A, B, prefill = _setup(celltype)
    ref = _fresh_all(celltype, mode)
    tev = _tev(mesh, g)
    _run(tev, fcg.TSI_ALL, fcg.OVERWRITE, B, prefill)
    got = _run(tev, parts, mode, A, prefill)
    for k, bit in OUTPUT_OF.items():
        assert np.array_equal(got[k], ref[k] if parts & bit else prefill[k]), (k, bool(parts & bit))
    _run(tev, fcg.TSI_ALL, fcg.OVERWRITE, B, prefill)
    nul = _run(tev, parts, mode, A, prefill, drop=True)
    for k, bit in OUTPUT_OF.items():
        if parts & bit:
            assert np.array_equal(nul[k], ref[k]), k
        else:
            assert nul[k] is None
    tev.close()
    if parts & FS:
        # f_S is `+=` in both modes: prefill + the thermal part (the evaluate from zeros)
        f0 = _fresh_all(celltype, fcg.OVERWRITE, zero=True)["fs"]
        assert np.abs(f0).max() > 0
        assert np.array_equal(got["fs"], prefill["fs"] + f0)
    # the other outputs follow the mode
    z = _fresh_all(celltype, fcg.OVERWRITE, zero=True)
    for k in ("Kst", "Ktt", "fT", "Kts"):
        if parts & OUTPUT_OF[k]:
            want = z[k] if mode == fcg.OVERWRITE else prefill[k] + z[k]
            assert np.array_equal(got[k], want), k


# ------------------------------------------------------------------------------ time factors
def _assert_kts_scales(a, b, factor):
    """k_TS is the one multiple -timefac timefac_d of a sum that does not depend on them: the two
    results differ by the rounding of that product and of one multiplication per entry (the
    fused pass multiplies m in as well), a few u; 64 u normwise leaves no room for a wrong factor."""
    assert np.linalg.norm(a - factor * b) <= 64 * U * np.linalg.norm(a) and np.linalg.norm(a) > 0


@pytest.mark.parametrize("celltype", [fcg.HEX8, fcg.HEX27])
def test_time_factors_two_kernel(celltype):
    _dev()
    base = _fresh_all(celltype, fcg.OVERWRITE)
    one = _fresh_all(celltype, fcg.OVERWRITE, timefac=1.0, timefac_d=1.0)
    nod = _fresh_all(celltype, fcg.OVERWRITE, timefac=TIMEFAC, timefac_d=0.0)
    assert np.all(nod["Kts"] == 0.0)
    for k in ("fs", "Kst", "Ktt", "fT"):
        assert np.array_equal(base[k], one[k]) and np.array_equal(base[k], nod[k]), k
    _assert_kts_scales(base["Kts"], one["Kts"], TIMEFAC * TIMEFAC_D)


def _fused(mesh, g, u, state, timefac, timefac_d, ev=None, tev=None):
    v, T_col = state
    own = ev is None
    if own:
        ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
        assert ev.info.path == fcg.PATH_STRUCTURED
        tev = _tev(mesh, g)
    nan = lambda n: torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())  # noqa: E731
    o = dict(Kss=nan(mesh.nnz), **{k: nan(n) for k, n in _sizes(mesh, g).items()})
    try:
        tev.evaluate_fused(ev, fcg.OVERWRITE, _t(u), _t(v), _t(T_col), timefac, timefac_d, **o)
        torch.cuda.synchronize()
    finally:
        if own:
            tev.close()
            ev.close()
    return {k: x.cpu().numpy() for k, x in o.items()}


@pytest.mark.parametrize("split", [None, "0"])
def test_time_factors_fused(split, monkeypatch):
    _dev()
    if split is None:
        monkeypatch.delenv("FCG_TSI_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FCG_TSI_SPLIT", split)
    mesh, g, A, _, _ = _setup(fcg.HEX8)
    u = mesh.u_col(1e-3)
    base = _fused(mesh, g, u, A, TIMEFAC, TIMEFAC_D)
    one = _fused(mesh, g, u, A, 1.0, 1.0)
    nod = _fused(mesh, g, u, A, TIMEFAC, 0.0)
    assert all(np.isfinite(x).all() for x in base.values())
    assert np.all(nod["Kts"] == 0.0)
    for k in ("Kss", "fs", "Kst", "Ktt", "fT"):
        assert np.array_equal(base[k], one[k]) and np.array_equal(base[k], nod[k]), k
    _assert_kts_scales(base["Kts"], one["Kts"], TIMEFAC * TIMEFAC_D)


def test_fused_switch_is_read_at_each_call(monkeypatch):
    """FCG_TSI_SPLIT selects between two passes whose residuals differ in the last bits (another
    order of the same sums); one process reaches both."""
    _dev()
    mesh, g, A, _, _ = _setup(fcg.HEX8)
    u = mesh.u_col(1e-3)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
    tev = _tev(mesh, g)
    out = []
    for split in (None, "0", None):
        if split is None:
            monkeypatch.delenv("FCG_TSI_SPLIT", raising=False)
        else:
            monkeypatch.setenv("FCG_TSI_SPLIT", split)
        out.append(_fused(mesh, g, u, A, TIMEFAC, TIMEFAC_D, ev=ev, tev=tev))
    tev.close()
    ev.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[2][k]), k
    assert any(not np.array_equal(out[0][k], out[1][k]) for k in out[0])


# ------------------------------------------------------------------------------ refusals
def _oracle_code(celltype, X, T, v, parts):
    """What 4C's element actions behind `parts` answer for one element: the solid-scatra
    element first (struct_calc_nlnstiff, struct_calc_stifftemp), then the thermo element."""
    npe = len(X)
    if parts & (FS | ST):
        want = (("f",) if parts & FS else ()) + (("Kst",) if parts & ST else ())
        err = orc.tsi_solid_evaluate(celltype, E, NU, ALPHA, T0, X, np.zeros((npe, 3)), T, want=want)[0]
        if err:
            return err
    if parts & (TT | TS):
        return orc.tsi_thermo_evaluate(celltype, COND, orc.st_modulus(E, NU, ALPHA), X, T, v,
                                       TIMEFAC, TIMEFAC_D)[0]
    return 0


def _oracle_refusal(mesh, g, state, parts):
    """(code, lowest refused element gid) or (0, -1)."""
    v, T_col = state
    en = np.asarray(mesh.ele_nodes)
    vn = tr.node_displacements(mesh, v)
    Tn = T_col[g.node_dof_col_t]
    codes = [_oracle_code(mesh.celltype, mesh.node_x[n], Tn[n], vn[n], parts) for n in en]
    bad = [(int(gid), c) for gid, c in zip(mesh.ele_gid, codes) if c]
    if not bad:
        return 0, -1
    assert len({c for _, c in bad}) == 1   # one code: the expectation does not depend on an order
    return bad[0][1], min(gid for gid, _ in bad)


def _state_of(mesh, g):
    _, v, Tn = tr.smooth_fields(mesh, T_mean=T0)
    T_col = np.zeros(g.n_cols_t)
    T_col[g.node_dof_col_t] = Tn
    return v, T_col


def _check_refusals(mesh, g, subsets, valid_parts):
    """Every subset against the oracle's answer; after each refusal the valid subset on the same
    context gives what a fresh context gives."""
    state = _state_of(mesh, g)
    rng = np.random.default_rng(2)
    prefill = {k: rng.standard_normal(n) for k, n in _sizes(mesh, g).items()}
    assert _oracle_refusal(mesh, g, state, valid_parts) == (0, -1)
    fresh = _tev(mesh, g)
    want = _run(fresh, valid_parts, fcg.OVERWRITE, state, prefill)
    fresh.close()
    tev = _tev(mesh, g)
    refused = 0
    for parts in subsets:
        code, gid = _oracle_refusal(mesh, g, state, parts)
        if code == 0:
            _run(tev, parts, fcg.OVERWRITE, state, prefill)
            continue
        refused += 1
        with pytest.raises(fcg.FcgError) as ei:
            _run(tev, parts, fcg.OVERWRITE, state, prefill)
        assert (ei.value.code, ei.value.bad_ele_gid) == (code, gid), (parts, ei.value, code, gid)
        again = _run(tev, valid_parts, fcg.OVERWRITE, state, prefill)
        for k in OUTPUT_OF:
            assert np.array_equal(again[k], want[k]), (parts, k)
    tev.close()
    return refused


def _inverted(celltype, shift=1.5):
    """The box with one interior node moved `shift` element edges along x: elements at that node
    turn inside out."""
    mesh = fcg.BoxMesh(celltype, IV[celltype], jitter=0.1, seed=4)
    X = np.asarray(mesh.node_x)
    centre = np.array([1.0 / 3.0, 1.0 / 3.0, 0.5]) if celltype == fcg.HEX8 else np.array([0.5, 0.5, 0.5])
    node = int(np.argmin(np.linalg.norm(X - centre, axis=1)))
    assert np.linalg.norm(X[node] - centre) < 0.1
    mesh.node_x[node, 0] += shift / IV[celltype][0]
    return mesh


@pytest.mark.parametrize("celltype,shift,n_refused", [(fcg.HEX8, 1.5, 8), (fcg.HEX8, 2.5, 14),
                                                       (fcg.HEX27, 1.5, 14)])
def test_inverted_element_is_refused_two_kernel(celltype, shift, n_refused):
    """n_refused: how many of the 15 subsets the oracle refuses.  The thermal stress alone is never
    checked by 4C.  hex8 at 1.5 edges has det J < 0 at nodes only, so only the subsets with
    k_ST (the nodal check of struct_calc_stifftemp) are refused; at 2.5 edges, and for hex27, the
    Gauss points invert too and the thermo element refuses as well (hex27: in another element
    than the nodal check, so the lowest GID depends on the subset)."""
    _dev()
    mesh = _inverted(celltype, shift)
    g = fcg.TsiGraph(mesh)
    assert _check_refusals(mesh, g, range(1, 16), FS) == n_refused


@pytest.mark.parametrize("split", [None, "0"])
def test_inverted_element_is_refused_fused(split, monkeypatch):
    _dev()
    if split is None:
        monkeypatch.delenv("FCG_TSI_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FCG_TSI_SPLIT", split)
    mesh = _inverted(fcg.HEX8)
    g = fcg.TsiGraph(mesh)
    state = _state_of(mesh, g)
    u = np.zeros(mesh.n_cols)
    code, gid = _oracle_refusal(mesh, g, state, fcg.TSI_ALL)
    Tn = state[1][g.node_dof_col_t]
    assert code == 1 and oracle_tsi_evaluate(mesh, g, E, NU, ALPHA, T0, COND, TIMEFAC, TIMEFAC_D, u,
                                             state[0], Tn)[0] == code
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, path=fcg.PATH_STRUCTURED)
    assert ev.info.path == fcg.PATH_STRUCTURED
    tev = _tev(mesh, g)
    with pytest.raises(fcg.FcgError) as ei:
        _fused(mesh, g, u, state, TIMEFAC, TIMEFAC_D, ev=ev, tev=tev)
    assert (ei.value.code, ei.value.bad_ele_gid) == (code, gid), (ei.value, code, gid)
    # the TSI context goes on working: the one part 4C accepts on this mesh
    rng = np.random.default_rng(2)
    prefill = {k: rng.standard_normal(n) for k, n in _sizes(mesh, g).items()}
    again = _run(tev, FS, fcg.OVERWRITE, state, prefill)
    tev.close()
    ev.close()
    fresh = _tev(mesh, g)
    want = _run(fresh, FS, fcg.OVERWRITE, state, prefill)
    fresh.close()
    for k in OUTPUT_OF:
        assert np.array_equal(again[k], want[k]), k


@pytest.mark.parametrize("celltype", [fcg.HEX8, fcg.HEX27])
def test_thermo_det_threshold(celltype):
    """Element edge 4e-6, det J ~ 8e-18 < 1e-16: the structure evaluates; the thermo element's
    two actions are refused, alone and together; k_ST and the thermal stress are accepted."""
    _dev()
    iv = IV[celltype]
    mesh = fcg.BoxMesh(celltype, iv, upper=tuple(4e-6 * n for n in iv), jitter=0.1, seed=4)
    g = fcg.TsiGraph(mesh)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=_dev())
    K = torch.zeros(mesh.nnz, dtype=torch.float64, device=_dev())
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, _t(mesh.u_col(1e-9)), f, K)
    torch.cuda.synchronize()
    ev.close()
    assert torch.isfinite(K).all() and torch.isfinite(f).all()
    _, v, Tn = tr.smooth_fields(mesh, T_mean=T0, scale=tuple(4e-6 * n for n in iv))
    m = tr.st_modulus_ld(E, NU, ALPHA)
    en = np.asarray(mesh.ele_nodes)
    el = tr.elements_tsi_ld(celltype, m, COND, T0, TIMEFAC, TIMEFAC_D, mesh.node_x[en],
                            tr.node_displacements(mesh, v)[en], Tn[en])
    assert 0 < el["detJ"].min() and el["detJ"].max() < 1e-16 and el["detJ_node"].min() > 0
    refused = _check_refusals(mesh, g, (TT, TS, TT | TS, ST | FS, fcg.TSI_ALL), ST | FS)
    assert refused == 4
