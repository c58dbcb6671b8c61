"""Whole K rows within one layer on lattice tiles, and the sweep's element-free layers.

The deferred sweep (MODE 3, FCG_SWEEP_DEFER=1 at fcg_create) parks each block with the plane below
one layer in LDS and writes it beside the row's other blocks.  On regular lattice tiles it takes the
closed-form row bookkeeping of the direct kernel (Evaluator.sweep_regular_layers), and the linear
structural sweep leaves out the layers that hold no element: the layer below the element box is not
run, the one on the top node plane runs its emits on zero accumulators (FCG_SWEEP_SKIP_EMPTY=0 runs
both as every other layer).  None of it changes the arithmetic or the summation order, so on every
mesh four contexts must store the same bits (np.array_equal):

* deferred with the regular emit (the context under test),
* FCG_SWEEP_DEFER=0: direct rows (MODE 0) with the regular emit,
* FCG_SWEEP_DEFER=1, FCG_SWEEP_REGULAR=0: deferred, plane records only,
* the first again with FCG_SWEEP_SKIP_EMPTY=0,

after OVERWRITE into NaN-filled K and f (every entry written, across run edges and segment ends),
ACCUMULATE onto seeded non-zero K and f (every entry written once) and internal force only in both
modes.  Meshes: the 38 x 37 x 11 box (10 x 10 tiles, bottom / middle / top segments, regular
interior tiles beside boundary and partial ones); the same without one interior element (held
blocks cross between regular and record layers); both ranks of its two-rank split (a ghost layer
under K0: the first layer is not empty); the 6 x 5 x 4 box (no regular tile, element-free layers at
both ends of every workgroup).  One case against the CPU oracle at test_gpu_parity's tolerances.
"""

import importlib

import numpy as np
import pytest

from parity_util import oracle_evaluate, rel_err

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

E, NU = 210.0, 0.3
BOX = (38, 37, 11)
SWITCHES = ("FCG_SWEEP_DEFER", "FCG_SWEEP_REGULAR", "FCG_SWEEP_SKIP_EMPTY")
# (name, environment at fcg_create, Evaluator.sweep_rows())
CONTEXTS = [
    ("deferred-regular", {"FCG_SWEEP_DEFER": "1"}, "deferred"),
    ("direct-regular", {"FCG_SWEEP_DEFER": "0"}, "direct"),
    ("deferred-records", {"FCG_SWEEP_DEFER": "1", "FCG_SWEEP_REGULAR": "0"}, "deferred"),
    ("deferred-regular-all-layers", {"FCG_SWEEP_DEFER": "1", "FCG_SWEEP_SKIP_EMPTY": "0"}, "deferred"),
]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _context(monkeypatch, mesh, env):
    _dev()
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, device=0, path=fcg.PATH_STRUCTURED)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return ev


def _evaluate(ev, mesh, u, action, mode, K0=None, f0=None):
    dev = _dev()
    ut = torch.from_numpy(u).to(dev)
    f = torch.from_numpy(f0).to(dev) if f0 is not None else torch.full(
        (mesh.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    K = None
    if action == fcg.CALC_NLNSTIFF:
        K = torch.from_numpy(K0).to(dev) if K0 is not None else torch.full(
            (mesh.nnz,), float("nan"), dtype=torch.float64, device=dev)
    ev.evaluate_device(action, mode, ut, f, K)
    torch.cuda.synchronize()
    return (K.cpu().numpy() if K is not None else None), f.cpu().numpy()


def _all_modes(ev, mesh, u):
    """OVERWRITE into NaN, ACCUMULATE onto non-zero K and f, internal force only (both modes)."""
    rng = np.random.default_rng(13)
    K0, f0 = rng.standard_normal(mesh.nnz), rng.standard_normal(mesh.n_rows)
    out = list(_evaluate(ev, mesh, u, fcg.CALC_NLNSTIFF, fcg.OVERWRITE))
    out += _evaluate(ev, mesh, u, fcg.CALC_NLNSTIFF, fcg.ACCUMULATE, K0.copy(), f0.copy())
    out.append(_evaluate(ev, mesh, u, fcg.CALC_INTERNALFORCE, fcg.OVERWRITE)[1])
    out.append(_evaluate(ev, mesh, u, fcg.CALC_INTERNALFORCE, fcg.ACCUMULATE, f0=f0.copy())[1])
    assert all(np.all(np.isfinite(a)) for a in out)
    return out


def _same_bits(monkeypatch, mesh, u):
    """The four contexts store the same bits; returns the (regular, total) counts by context."""
    ref, counts = None, {}
    for name, env, rows in CONTEXTS:
        ev = _context(monkeypatch, mesh, env)
        assert ev.info.path == fcg.PATH_STRUCTURED and ev.sweep_kernel() == "unchecked"
        assert ev.sweep_rows() == rows, name
        counts[name] = ev.sweep_regular_layers()
        out = _all_modes(ev, mesh, u)
        if ref is None:
            ref = out
        for i, (a, b) in enumerate(zip(ref, out)):
            assert np.array_equal(a, b), (name, i, int(np.count_nonzero(a != b)))
    assert counts["deferred-records"][0] == 0
    assert counts["deferred-regular"] == counts["direct-regular"] == counts["deferred-regular-all-layers"]
    return counts["deferred-regular"]


_MESH = {}


def _box(iv):
    if iv not in _MESH:
        _MESH[iv] = fcg.BoxMesh(fcg.HEX8, iv, jitter=0.1, seed=20251015)
    return _MESH[iv]


def test_box_with_regular_tiles(monkeypatch):
    mesh = _box(BOX)
    reg, total = _same_bits(monkeypatch, mesh, mesh.u_col(1e-3))
    assert 0 < reg < total


def _without_element(box, ijk):
    """The single-rank box without the element at lattice position ijk: its 8 corner nodes lose
    the coupling to the diagonally opposite corner, every other row keeps its columns."""
    assert np.array_equal(box.node_dof_col, 3 * np.arange(box.n_node))
    e = int(np.nonzero(np.all(box.ele_ijk == np.array(ijk), axis=1))[0][0])
    en = box.ele_nodes[e]
    keep = np.ones(box.nnz, dtype=bool)
    for a, b in enumerate((6, 7, 4, 5, 2, 3, 0, 1)):
        for r in range(3 * int(en[a]), 3 * int(en[a]) + 3):
            s, t = int(box.rowptr[r]), int(box.rowptr[r + 1])
            keep[s:t] &= box.col_lid[s:t] // 3 != int(en[b])
    rowlen = np.add.reduceat(keep.astype(np.int64), box.rowptr[:-1])
    rowptr = np.concatenate([[0], np.cumsum(rowlen)])
    sel = np.arange(box.n_ele) != e
    dis = fcg.Discretization(fcg.HEX8, box.ele_nodes[sel], box.node_x, box.node_dof_col,
                             box.node_dof_row, rowptr, box.col_lid[keep])
    dis.ele_ijk = np.ascontiguousarray(box.ele_ijk[sel], dtype=np.int32)
    assert dis.nnz == box.nnz - 8 * 9
    return dis


def test_box_with_a_hole(monkeypatch):
    box = _box(BOX)
    dis = _without_element(box, (18, 17, 5))
    u = np.random.default_rng(6).standard_normal(dis.n_cols) * 1e-3
    reg, total = _same_bits(monkeypatch, dis, u)
    full = _context(monkeypatch, box, {"FCG_SWEEP_DEFER": "1"}).sweep_regular_layers()
    # the tile that holds the hole's corner nodes loses regular layers, no other tile does
    assert total == full[1] and 0 < reg < full[0]


@pytest.mark.parametrize("rank", [0, 1])
def test_two_rank_split(monkeypatch, rank):
    mesh = fcg.BoxMesh(fcg.HEX8, BOX, jitter=0.1, seed=20251015, rank=rank, nranks=2)
    reg, total = _same_bits(monkeypatch, mesh, mesh.u_col(1e-3))
    assert 0 < reg < total


def test_box_without_a_regular_tile(monkeypatch):
    mesh = _box((6, 5, 4))
    reg, total = _same_bits(monkeypatch, mesh, mesh.u_col(1e-3))
    assert reg == 0 and total > 0


def test_mode_without_the_switch(monkeypatch):
    """Linear contexts take the deferred kernel, regular emit included; TotLag keeps direct rows."""
    _dev()
    mesh = _box(BOX)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    lin = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU, device=0)
    assert lin.info.path == fcg.PATH_STRUCTURED and lin.sweep_rows() == "deferred"
    assert lin.sweep_regular_layers()[0] > 0
    tot = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU, device=0)
    assert tot.sweep_rows() == "direct" and tot.sweep_regular_layers()[0] == 0


def test_deferred_regular_against_the_oracle(monkeypatch):
    mesh = _box((13, 12, 7))
    u = mesh.u_col(1e-3)
    ev = _context(monkeypatch, mesh, {"FCG_SWEEP_DEFER": "1"})
    assert ev.sweep_rows() == "deferred" and ev.sweep_kernel() == "unchecked"
    Kg, fg = _evaluate(ev, mesh, u, fcg.CALC_NLNSTIFF, fcg.OVERWRITE)
    err, _, Kr, fr = oracle_evaluate(mesh, fcg.LINEAR, E, NU, u)
    assert err == 0
    # the tolerances of test_gpu_parity._check
    assert rel_err(fg, fr) <= 1e-10, rel_err(fg, fr)
    assert np.all(np.isfinite(Kg))
    assert rel_err(Kg, Kr) <= 1e-12, rel_err(Kg, Kr)
    assert np.abs(Kg - Kr).max() <= 1e-12 * np.abs(Kr).max()
