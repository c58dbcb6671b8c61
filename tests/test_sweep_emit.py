"""The row-block sweep's emit path where the small parity meshes do not reach it.

Multi-plane segments.  fcg_create picks the z-segment length with the least rounds x layers
(fcg_create_plan.cpp, "tiles"): with `slots` = CUs x workgroups per CU resident workgroups, a split
into k segments of seg = ceil(NK / k) node planes costs ceil(tiles_xy ceil(NK / seg) / slots) x
(seg + 1).  Whenever all workgroups fit in one round the shortest segment wins, so the small parity
meshes all run one-plane segments and never carry the hold buffer (the lower-layer parts of the
in-plane blocks) or the kept residual part across three or more layers of one workgroup.  The box
here has 38 x 37 x 11 elements: 39 x 38 x 12 node columns, so 10 x 10 tiles of 4 x 4 columns
with partial last tiles in x and y, and NK = 12.  On 256 CUs the linear sweep (2 workgroups per
CU, 512 slots) costs 13 (k = 1), 7 (2), 5 (3), 4 (4: 400 workgroups of 3 planes, one round),
6 (6: 600 workgroups, two rounds) and 6 (12): four segments of three planes.  TotLag (1 workgroup
per CU, 256 slots) costs 13, 7 (k = 2: 200 workgroups of 6 planes), 10, 8, 9, 10: two segments
of six planes.  fcg_info does not expose the segment length; on a device with another CU count
the rule may choose differently, and the comparisons below hold for any choice.

The cold path.  An element with fac = det J w < 0 at some Gauss point takes the NEG instantiation
of the sweep's element visit, which no valid mesh reaches.  The (6, 5, 4) box with the coordinates
of two nodes of an interior element exchanged has such elements; the evaluate reports the lowest
rejected element and still writes all of K and f.  Their values are compared with those recorded
from the sweep before its emit path was trimmed (tests/golden/sweep_cold_654.npz: f, and K at the
indices `k_idx` = every entry of the rows of the exchanged nodes plus a seeded sample), equal
bit for bit up to the sign of a zero.
"""

import importlib
import os

import numpy as np
import pytest

from parity_util import oracle_evaluate, rel_err

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

E, NU = 210.0, 0.3
IV = (38, 37, 11)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_cold_654.npz")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run(mesh, kinem, u_col, action=fcg.CALC_NLNSTIFF, mode=fcg.OVERWRITE, ev=None, K0=None,
         f0=None):
    dev = _dev()
    ev = ev or fcg.Evaluator(mesh, kinematics=kinem, youngs=E, poisson=NU, device=0,
                             path=fcg.PATH_STRUCTURED)
    assert ev.info.path == fcg.PATH_STRUCTURED
    u = torch.from_numpy(u_col).to(dev)
    f = torch.from_numpy(f0).to(dev) if f0 is not None else torch.full(
        (mesh.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    K = None
    if action == fcg.CALC_NLNSTIFF:
        K = torch.from_numpy(K0).to(dev) if K0 is not None else torch.full(
            (mesh.nnz,), float("nan"), dtype=torch.float64, device=dev)
    ev.evaluate_device(action, mode, u, f, K)
    torch.cuda.synchronize()
    return (K.cpu().numpy() if K is not None else None), f.cpu().numpy(), ev


def _check(Kg, fg, Kr, fr):
    """The parity tolerances of test_gpu_parity.py."""
    assert np.all(np.isfinite(fg))
    assert rel_err(fg, fr) <= 1e-10, rel_err(fg, fr)
    if Kg is not None:
        assert np.all(np.isfinite(Kg))
        assert rel_err(Kg, Kr) <= 1e-12, rel_err(Kg, Kr)
        assert np.abs(Kg - Kr).max() <= 1e-12 * np.abs(Kr).max()


_CACHE = {}


def _box(kinem):
    """The 38 x 37 x 11 box, its u and the oracle's K, f -- computed once per kinematics."""
    if "mesh" not in _CACHE:
        _CACHE["mesh"] = fcg.BoxMesh(fcg.HEX8, IV, jitter=0.1, seed=20251015)
    if kinem not in _CACHE:
        mesh = _CACHE["mesh"]
        u = mesh.u_col(1e-3 if kinem == fcg.LINEAR else 5e-2)
        err, _, Kr, fr = oracle_evaluate(mesh, kinem, E, NU, u, nworkers=4)
        assert err == 0
        Kr.setflags(write=False)
        fr.setflags(write=False)
        _CACHE[kinem] = (mesh, u, Kr, fr)
    return _CACHE[kinem]


def test_multiplane_overwrite_matches_oracle_and_repeats_bitwise():
    mesh, u, Kr, fr = _box(fcg.LINEAR)
    assert mesh.n_ele == 38 * 37 * 11
    # K and f start as NaN: an entry the sweep does not write shows
    Kg, fg, ev = _run(mesh, fcg.LINEAR, u)
    _check(Kg, fg, Kr, fr)
    K2, f2, _ = _run(mesh, fcg.LINEAR, u, ev=ev)
    assert np.array_equal(K2, Kg) and np.array_equal(f2, fg)
    # a second context (its own plan and upload) computes the same bits
    K3, f3, _ = _run(mesh, fcg.LINEAR, u)
    assert np.array_equal(K3, Kg) and np.array_equal(f3, fg)


def test_multiplane_accumulate_onto_nonzero():
    mesh, u, Kr, fr = _box(fcg.LINEAR)
    rng = np.random.default_rng(11)
    # caller storage of the tangent's own size, so that the sums' rounding (one ulp of K0 + K)
    # stays far inside the parity tolerances
    K0 = rng.standard_normal(mesh.nnz) * np.abs(Kr).max()
    f0 = rng.standard_normal(mesh.n_rows) * np.abs(fr).max()
    Kg, fg, _ = _run(mesh, fcg.LINEAR, u, mode=fcg.ACCUMULATE, K0=K0.copy(), f0=f0.copy())
    _check(Kg - K0, fg - f0, Kr, fr)


def test_multiplane_internal_force_only():
    mesh, u, _, fr = _box(fcg.LINEAR)
    _, fg, _ = _run(mesh, fcg.LINEAR, u, action=fcg.CALC_INTERNALFORCE)
    _check(None, fg, None, fr)


def test_multiplane_deferred_blocks_bitwise(monkeypatch):
    """FCG_SWEEP_DEFER=1 (MODE 3: a row's lower-plane blocks written one layer later) stores the
    values of MODE 0, for OVERWRITE and ACCUMULATE."""
    mesh, u, _, _ = _box(fcg.LINEAR)
    rng = np.random.default_rng(12)
    K0, f0 = rng.standard_normal(mesh.nnz), rng.standard_normal(mesh.n_rows)
    out = {}
    for defer in ("0", "1"):
        monkeypatch.setenv("FCG_SWEEP_DEFER", defer)
        K1, f1, ev = _run(mesh, fcg.LINEAR, u)
        K2, f2, _ = _run(mesh, fcg.LINEAR, u, ev=ev, mode=fcg.ACCUMULATE, K0=K0.copy(), f0=f0.copy())
        out[defer] = (K1, f1, K2, f2)
    for a, b in zip(out["0"], out["1"]):
        assert np.array_equal(a, b)


def test_multiplane_totlag_matches_oracle():
    mesh, u, Kr, fr = _box(fcg.TOTLAG)
    Kg, fg, ev = _run(mesh, fcg.TOTLAG, u)
    _check(Kg, fg, Kr, fr)
    K2, f2, _ = _run(mesh, fcg.TOTLAG, u, ev=ev)
    assert np.array_equal(K2, Kg) and np.array_equal(f2, fg)


def _gauss_detj(X):
    """det J at the 2 x 2 x 2 Gauss points of a hex8 with node coordinates X [8, 3] (4C order)."""
    r = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1],
                  [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=float)
    d1, d2 = [1, 2, 0], [2, 0, 1]
    out = []
    for g in r / np.sqrt(3.0):
        dN = 0.125 * r * (1 + r[:, d1] * g[d1]) * (1 + r[:, d2] * g[d2])
        out.append(np.linalg.det(X.T @ dN))
    return out


def cold_case():
    """The (6, 5, 4) box with the coordinates of local nodes 0 and 1 of the interior element at
    lattice position (2, 2, 1) exchanged: (mesh, u, the two nodes, K indices compared)."""
    mesh = fcg.BoxMesh(fcg.HEX8, (6, 5, 4), jitter=0.1, seed=20251015)
    e = int(np.nonzero(np.all(mesh.ele_ijk == np.array([2, 2, 1]), axis=1))[0][0])
    n0, n1 = (int(n) for n in mesh.ele_nodes[e][:2])
    mesh.node_x[[n0, n1]] = mesh.node_x[[n1, n0]]
    u = mesh.u_col(1e-3)
    rows = np.concatenate([mesh.node_dof_row[n] + np.arange(3) for n in (n0, n1)])
    idx = [np.arange(mesh.rowptr[r], mesh.rowptr[r + 1]) for r in rows]
    idx.append(np.random.default_rng(654).choice(mesh.nnz, 4096, replace=False))
    return mesh, u, (n0, n1), np.unique(np.concatenate(idx))


def run_cold(mesh, u):
    """Evaluate the cold case: (FcgError, K, f) -- the sweep writes K and f in full, then the
    evaluate reports the rejected element."""
    dev = _dev()
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, device=0,
                       path=fcg.PATH_STRUCTURED)
    ut = torch.from_numpy(u).to(dev)
    f = torch.full((mesh.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    K = torch.full((mesh.nnz,), float("nan"), dtype=torch.float64, device=dev)
    with pytest.raises(fcg.FcgError) as ei:
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, ut, f, K)
    torch.cuda.synchronize()
    return ei.value, K.cpu().numpy(), f.cpu().numpy()


def test_negative_fac_visit_keeps_its_values():
    import oracle_lib as orc
    mesh, u, _, k_idx = cold_case()
    # what the reference rejects: det J <= 0 at a node (calc_lib.hpp:492-494); the evaluate names
    # the lowest such element
    zero = np.zeros((8, 3))
    codes = [orc.solid_evaluate(fcg.HEX8, fcg.LINEAR, E, NU, mesh.node_x[en], zero, want_k=False)[0]
             for en in mesh.ele_nodes]
    rejected = [int(g) for g, c in zip(mesh.ele_gid, codes) if c == 1]
    assert rejected
    # the case does reach the NEG visit: some element has fac < 0 at some Gauss points only
    dets = np.array([_gauss_detj(mesh.node_x[en]) for en in mesh.ele_nodes])
    assert np.any((dets < 0).any(axis=1) & (dets > 0).any(axis=1))
    err, K, f = run_cold(mesh, u)
    assert err.code == 1 and err.bad_ele_gid == min(rejected), (err, rejected)
    assert np.all(np.isfinite(K)) and np.all(np.isfinite(f))
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["k_idx"], k_idx)
    # array_equal compares values: equal bit for bit up to the sign of a zero
    assert np.array_equal(f, gold["f"])
    assert np.array_equal(K[k_idx], gold["K"])
