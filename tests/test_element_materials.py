"""Per-element material parameters (fcg_set_element_materials): several materials of the context's
one material kind, selected per element -- 4C's element loop asks each element's So3Material
(Solid::evaluate -> So3Material::evaluate), and input files carry several MAT ids.

Reference: the oracle's element routine (oracle_lib.solid_evaluate) called per element with that
element's (E, nu), scattered in numpy into the mesh's CSR rows (owned rows only) and into f.
Bounds are the project's: K 1e-12, f 1e-10 relative (test_gpu_parity), the action 1e-12 against
the oracle and 1e-13 against fcg_spmv on the library's own K, the diagonal blocks 1e-12 / 1e-13
(test_tangent_apply, test_tangent_diag) -- norm-wise on all owned rows and, with the same bounds,
on the rows of the nodes whose elements all carry the softest material, so that an error there is
not hidden under the stiff region's norm.

* identity, bitwise: a table whose entries all equal the context's own (E, nu) gives the plain
  context's K, f, y and diagonal blocks bit for bit (the constants come from the same host
  arithmetic), and so does the context after set_element_materials(None);
* three materials (two for CoupNeoHooke) in layers and at random on jittered boxes, renumbered
  meshes (a table left in the wrong element order shows), a rank of a 2-rank partition (ghost
  elements), odd element counts (the two-elements-per-pass tails), and a mesh whose elements are
  all doubled on the same nodes (two overlapping materials): nodes with 16 elements, the gather
  path's records of nodes with more than 8;
* the matrix-free action and diagonal blocks on the hex27 cases;
* refusals: FcgError code 3, the context evaluating bitwise as before;
* Newton: a hex8 cantilever with a stiff half (NativeAMG) and a hex27 cantilever with a stiff
  layer (matrix-free multigrid, with and without the assembled tangent) converge to a state whose
  heterogeneous oracle residual vanishes.
"""

import ctypes
import functools
import importlib

import numpy as np
import pytest

import oracle_lib as orc

fcg = importlib.import_module("4c_amd").fcg
amg = importlib.import_module("4c_amd.amg")
mgm = importlib.import_module("4c_amd.multigrid")
newton = importlib.import_module("4c_amd.newton")

pytestmark = pytest.mark.gpu

E0, NU0 = 210.0, 0.3  # the contexts' own material: never one of the tables' below
MATS = {fcg.MAT_STVK: ([10.0, 50.0, 200.0], [0.25, 0.3, 0.45]),
        fcg.MAT_ELASTHYPER_COUPNEOHOOKE: ([10.0, 30.0], [0.25, 0.4])}
ORC_MAT = {fcg.MAT_STVK: orc.MAT_STVK, fcg.MAT_ELASTHYPER_COUPNEOHOOKE: orc.MAT_NEOHOOKE}


def _dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch, torch.device("cuda:0")


# ------------------------------------------------------------------------------------- meshes
def _renumbered(box, amp, seed):
    dis = fcg.Discretization.renumbered(box, seed=seed)
    ub, u = box.u_col(amp), np.zeros(box.n_cols)
    for d in range(3):
        u[3 * dis.node_perm + d] = ub[3 * np.arange(box.n_node) + d]
    return dis, u


def _doubled(box, amp):
    """Every element twice on the same nodes, the copies in shuffled order: interior nodes hold
    16 elements (two gather records), same graph as the box."""
    en = np.vstack([box.ele_nodes, box.ele_nodes])
    en = en[np.random.default_rng(8).permutation(len(en))]
    dis = fcg.Discretization.from_elements(fcg.HEX8, en, box.node_x)
    assert np.bincount(dis.ele_nodes.ravel()).max() == 16
    return dis, box.u_col(amp)


# name -> (celltype, material, path, builder(amp) -> (mesh, u_col))
CASES = {
    "h8-gather-4x3x2": (fcg.HEX8, fcg.MAT_STVK, fcg.PATH_GATHER,
                        lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX8, (4, 3, 2), jitter=0.1, seed=3))),
    "h8-gather-renumbered": (fcg.HEX8, fcg.MAT_STVK, fcg.PATH_GATHER,
                             lambda amp: _renumbered(fcg.BoxMesh(fcg.HEX8, (3, 3, 2)), amp, 4)),
    "h8-gather-rank1of2": (fcg.HEX8, fcg.MAT_STVK, fcg.PATH_GATHER,
                           lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX8, (4, 2, 2), rank=1, nranks=2))),
    # (rank 1 of that split holds no ghost elements, rank 0 does: 12 column elements, 8 of them its own)
    "h8-gather-rank0of2": (fcg.HEX8, fcg.MAT_STVK, fcg.PATH_GATHER,
                           lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX8, (4, 2, 2), rank=0, nranks=2))),
    "h27-rank0of2": (fcg.HEX27, fcg.MAT_STVK, fcg.PATH_GENERAL,
                     lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX27, (4, 2, 2), rank=0, nranks=2))),
    "h8-gather-doubled": (fcg.HEX8, fcg.MAT_STVK, fcg.PATH_GATHER,
                          lambda amp: _doubled(fcg.BoxMesh(fcg.HEX8, (3, 3, 3), jitter=0.1, seed=6), amp)),
    "h8-general-3x2x2": (fcg.HEX8, fcg.MAT_STVK, fcg.PATH_GENERAL,
                         lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1, seed=3))),
    "h27-3x2x2": (fcg.HEX27, fcg.MAT_STVK, fcg.PATH_GENERAL,
                  lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX27, (3, 2, 2), jitter=0.1, seed=11))),
    "h27-renumbered": (fcg.HEX27, fcg.MAT_STVK, fcg.PATH_GENERAL,
                       lambda amp: _renumbered(fcg.BoxMesh(fcg.HEX27, (3, 3, 2)), amp, 3)),
    "nh-h8-4x3x3": (fcg.HEX8, fcg.MAT_ELASTHYPER_COUPNEOHOOKE, fcg.PATH_GENERAL,
                    lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX8, (4, 3, 3), jitter=0.1, seed=3))),
    "nh-h27-2x2x1": (fcg.HEX27, fcg.MAT_ELASTHYPER_COUPNEOHOOKE, fcg.PATH_GENERAL,
                     lambda amp: (lambda m: (m, m.u_col(amp)))(fcg.BoxMesh(fcg.HEX27, (2, 2, 1), jitter=0.1, seed=3))),
}
STVK_CASES = [c for c in CASES if CASES[c][1] == fcg.MAT_STVK]
NH_CASES = [c for c in CASES if CASES[c][1] != fcg.MAT_STVK]
H27_CASES = ["h27-3x2x2", "h27-renumbered", "h27-rank0of2"]
SOFT_NODES_EXPECTED = {"h8-gather-4x3x2", "h27-3x2x2"}  # the layered assignment leaves an all-soft face


def _assign(mesh, n_mat, how):
    """ele_mat: layers by element-centroid x, or random (seeded)."""
    if how == "random":
        return np.random.default_rng(17).integers(0, n_mat, mesh.n_ele).astype(np.int32)
    cx = mesh.node_x[mesh.ele_nodes][:, :, 0].mean(axis=1)
    x0, x1 = mesh.node_x[:, 0].min(), mesh.node_x[:, 0].max()
    return np.minimum(n_mat - 1, np.floor(n_mat * (cx - x0) / (x1 - x0)).astype(np.int64)).astype(np.int32)


def _oracle_hetero(mesh, celltype, kin, material, Es, nus, em, u_col, want_k=True):
    """The oracle's element routine per element with its own (E, nu), scattered into the mesh's
    CSR (owned rows) and f."""
    K, f = np.zeros(mesh.nnz), np.zeros(mesh.n_rows)
    d3 = np.arange(3)
    for e in range(mesh.n_ele):
        nodes = mesh.ele_nodes[e]
        cols = (mesh.node_dof_col[nodes][:, None] + d3).ravel()
        err, Ke, fe = orc.solid_evaluate(celltype, kin, Es[em[e]], nus[em[e]], mesh.node_x[nodes],
                                         u_col[cols].reshape(-1, 3), want_k=want_k,
                                         material=ORC_MAT[material])
        assert err == 0
        for a, nd in enumerate(nodes):
            r0 = mesh.node_dof_row[nd]
            if r0 < 0:
                continue
            for i in range(3):
                f[r0 + i] += fe[3 * a + i]
                if want_k:
                    s, t = mesh.rowptr[r0 + i], mesh.rowptr[r0 + i + 1]
                    pos = s + np.searchsorted(mesh.col_lid[s:t], cols)
                    assert np.array_equal(mesh.col_lid[pos], cols)
                    K[pos] += Ke[3 * a + i]
    return K, f


def _soft_rows(mesh, em):
    """Owned rows of the nodes whose elements all carry material 0 (the softest)."""
    stiff = np.zeros(mesh.n_node, dtype=bool)
    stiff[mesh.ele_nodes[em != 0].ravel()] = True
    held = np.zeros(mesh.n_node, dtype=bool)
    held[mesh.ele_nodes.ravel()] = True
    nodes = np.nonzero(held & ~stiff & (mesh.node_dof_row >= 0))[0]
    return np.sort((mesh.node_dof_row[nodes][:, None] + np.arange(3)).ravel())


@functools.lru_cache(maxsize=None)
def _reference(case, kin, how):
    """(mesh, u, Es, nus, ele_mat, oracle K, oracle f, soft rows): computed once, read-only."""
    celltype, material, _, build = CASES[case]
    mesh, u = build(1e-3 if kin == fcg.LINEAR else 5e-2)
    Es, nus = MATS[material]
    em = _assign(mesh, len(Es), how)
    assert len(np.unique(em)) >= 2  # (a rank may hold only part of the layers)
    K, f = _oracle_hetero(mesh, celltype, kin, material, Es, nus, em, u)
    for a in (u, em, K, f):
        a.setflags(write=False)
    return mesh, u, Es, nus, em, K, f, _soft_rows(mesh, em)


def _evaluate(ev, mesh, u, action=fcg.CALC_NLNSTIFF):
    torch, dev = _dev()
    f = torch.full((mesh.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    K = torch.full((mesh.nnz,), float("nan"), dtype=torch.float64, device=dev) \
        if action == fcg.CALC_NLNSTIFF else None
    ev.evaluate_device(action, fcg.OVERWRITE, torch.from_numpy(np.array(u)).to(dev), f, K)
    torch.cuda.synchronize()
    return (K.cpu().numpy() if K is not None else None), f.cpu().numpy()


def _apply(ev, u, x):
    torch, dev = _dev()
    y = torch.full((ev.info.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    ev.tangent_apply(torch.from_numpy(np.array(u)).to(dev), torch.from_numpy(x).to(dev), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _diag(ev, u, dbc=None, want="diag"):
    torch, dev = _dev()
    n = ev.info.n_rows // 3
    out = torch.full((9 * n,), float("nan"), dtype=torch.float64, device=dev)
    rows = None if dbc is None else torch.from_numpy(np.asarray(dbc, dtype=np.int32)).to(dev)
    ev.tangent_diag(torch.from_numpy(np.array(u)).to(dev), rows, **{want: out})
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, 3, 3)


def _rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _csr_rows(mesh):
    return np.repeat(np.arange(mesh.n_rows), np.diff(mesh.rowptr))


def _csr_mult(mesh, K, x):
    return np.bincount(_csr_rows(mesh), weights=K * x[mesh.col_lid], minlength=mesh.n_rows)


def _blocks_of(mesh, K):
    """The 3 x 3 nodal diagonal blocks of CSR values K (block k = rows 3k..3k+2)."""
    row_gid = getattr(mesh, "row_gid", None)
    if row_gid is None:
        col_of_row = np.arange(mesh.n_rows)
    else:
        order = np.argsort(mesh.col_gid)
        col_of_row = order[np.searchsorted(mesh.col_gid[order], row_gid)]
    D = np.empty((mesh.n_rows // 3, 3, 3))
    for i in range(mesh.n_rows):
        s, e = mesh.rowptr[i], mesh.rowptr[i + 1]
        want = col_of_row[3 * (i // 3):3 * (i // 3) + 3]
        j = s + np.searchsorted(mesh.col_lid[s:e], want)
        assert np.array_equal(mesh.col_lid[j], want)
        D[i // 3, i % 3] = K[j]
    return D


# ------------------------------------------------------------------------- 1. identity, bitwise
IDENTITY = {
    "h8-gather-linear": (fcg.HEX8, (3, 2, 2), fcg.LINEAR, fcg.MAT_STVK, fcg.PATH_GATHER, None),
    "h8-gather-totlag": (fcg.HEX8, (3, 2, 2), fcg.TOTLAG, fcg.MAT_STVK, fcg.PATH_GATHER, None),
    "h8-general-totlag": (fcg.HEX8, (3, 2, 2), fcg.TOTLAG, fcg.MAT_STVK, fcg.PATH_GENERAL, None),
    "h27-linear": (fcg.HEX27, (3, 3, 1), fcg.LINEAR, fcg.MAT_STVK, fcg.PATH_GENERAL, None),
    "h27-totlag": (fcg.HEX27, (3, 3, 1), fcg.TOTLAG, fcg.MAT_STVK, fcg.PATH_GENERAL, None),
    "h27-slab-linear": (fcg.HEX27, (3, 3, 1), fcg.LINEAR, fcg.MAT_STVK, fcg.PATH_GENERAL, 2),
    "h27-slab-totlag": (fcg.HEX27, (3, 3, 1), fcg.TOTLAG, fcg.MAT_STVK, fcg.PATH_GENERAL, 2),
    "nh-h8": (fcg.HEX8, (3, 2, 2), fcg.TOTLAG, fcg.MAT_ELASTHYPER_COUPNEOHOOKE, fcg.PATH_GENERAL, None),
    "nh-h27": (fcg.HEX27, (2, 2, 1), fcg.TOTLAG, fcg.MAT_ELASTHYPER_COUPNEOHOOKE, fcg.PATH_GENERAL, None),
}


@pytest.mark.parametrize("name", list(IDENTITY))
def test_uniform_table_and_reset_are_bitwise_the_plain_context(monkeypatch, name):
    _dev()
    celltype, shape, kin, material, path, slab = IDENTITY[name]
    if slab is not None:
        monkeypatch.setenv("FCG_H27_SLAB", str(slab))  # as tests/test_h27_slab.py forces it
    mesh = fcg.BoxMesh(celltype, shape, jitter=0.1, seed=7)
    u = mesh.u_col(1e-3 if kin == fcg.LINEAR else 5e-2)
    x = np.random.default_rng(3).standard_normal(mesh.n_cols)
    free = celltype == fcg.HEX27 and material == fcg.MAT_STVK  # the matrix-free entry points

    def results(ev):
        K, f = _evaluate(ev, mesh, u)
        _, fi = _evaluate(ev, mesh, u, fcg.CALC_INTERNALFORCE)
        return [K, f, fi] + ([_apply(ev, u, x), _diag(ev, u)] if free else [])

    mk = lambda: fcg.Evaluator(mesh, kinematics=kin, youngs=E0, poisson=NU0, path=path, material=material)  # noqa: E731
    plain = mk()
    assert plain.info.path == path
    if slab is not None:
        assert plain.info.h27_slabs > 1
    ref = results(plain)
    assert all(np.all(np.isfinite(r)) for r in ref)
    ev = mk()
    results(ev)  # (the matrix-free entry points allocate their buffers on first use)
    fcg.lib().fcg_get_info(ev._h, ctypes.byref(ev.info))
    bytes0 = ev.info.device_bytes
    assert ev.n_materials == 0
    em = np.random.default_rng(5).integers(0, 2, mesh.n_ele).astype(np.int32)
    ev.set_element_materials([E0, E0], [NU0, NU0], em)
    assert ev.n_materials == 2
    assert ev.info.device_bytes == bytes0 + 32 * mesh.n_ele
    for r, g in zip(ref, results(ev)):
        assert np.array_equal(r, g)
    # a real table changes the results; the reset is again the plain context
    Es, nus = MATS[material]
    ev.set_element_materials(Es, nus, _assign(mesh, len(Es), "random"))
    assert ev.n_materials == len(Es)
    assert ev.info.device_bytes == bytes0 + 32 * mesh.n_ele
    other = results(ev)
    assert not np.array_equal(other[0], ref[0]) and not np.array_equal(other[1], ref[1])
    ev.set_element_materials(None)
    assert ev.n_materials == 0 and ev.info.device_bytes == bytes0
    for r, g in zip(ref, results(ev)):
        assert np.array_equal(r, g)
    ev.close()
    plain.close()


# --------------------------------------------------------------- 2. against the oracle
def _check_k_f(mesh, Kg, fg, Kr, fr, soft, tag):
    rows = _csr_rows(mesh)
    ek, ef = _rel(Kg, Kr), _rel(fg, fr)
    print(f"{tag}: |dK|/|K| = {ek:.3e}  |df|/|f| = {ef:.3e}  soft rows {len(soft)}")
    assert np.all(np.isfinite(Kg)) and np.all(np.isfinite(fg))
    assert ek <= 1e-12 and ef <= 1e-10
    if len(soft):
        sel = np.isin(rows, soft)
        eks, efs = _rel(Kg[sel], Kr[sel]), _rel(fg[soft], fr[soft])
        print(f"{tag}: soft rows |dK|/|K| = {eks:.3e}  |df|/|f| = {efs:.3e}")
        assert np.linalg.norm(Kr[sel]) > 0 and np.linalg.norm(fr[soft]) > 0
        assert eks <= 1e-12 and efs <= 1e-10


def _run_case(case, kin, how):
    mesh, u, Es, nus, em, Kr, fr, soft = _reference(case, kin, how)
    if how == "layers" and case in SOFT_NODES_EXPECTED:
        assert len(soft) > 0
    celltype, material, path, _ = CASES[case]
    ev = fcg.Evaluator(mesh, kinematics=kin, youngs=E0, poisson=NU0, path=path, material=material)
    assert ev.info.path == path
    ev.set_element_materials(Es, nus, em)
    Kg, fg = _evaluate(ev, mesh, u)
    _check_k_f(mesh, Kg, fg, Kr, fr, soft, f"{case} kin {kin} {how}")
    _, fi = _evaluate(ev, mesh, u, fcg.CALC_INTERNALFORCE)
    assert _rel(fi, fr) <= 1e-10
    assert _rel(fi, fg) <= 1e-13  # the same sums, with or without the blocks beside them
    if len(soft):
        assert _rel(fi[soft], fr[soft]) <= 1e-10
    ev.close()


@pytest.mark.parametrize("how", ["layers", "random"])
@pytest.mark.parametrize("kin", [fcg.LINEAR, fcg.TOTLAG], ids=["linear", "totlag"])
@pytest.mark.parametrize("case", STVK_CASES)
def test_three_materials_match_the_oracle(case, kin, how):
    _dev()
    _run_case(case, kin, how)


@pytest.mark.parametrize("how", ["layers", "random"])
@pytest.mark.parametrize("case", NH_CASES)
def test_two_coupneohooke_materials_match_the_oracle(case, how):
    _dev()
    _run_case(case, fcg.TOTLAG, how)


# ------------------------------------------------------------------------------ 3. matrix-free
def _dbc_rows(mesh):
    """All DOFs of the owned nodes on the x-min face, the x-DOF alone of those on the x-max face."""
    x = mesh.node_x[:, 0]
    own = mesh.node_dof_row >= 0
    lo = np.nonzero(np.isclose(x, x.min()) & own)[0]
    hi = np.nonzero(np.isclose(x, x.max()) & own)[0]
    rows = np.concatenate([(mesh.node_dof_row[lo][:, None] + np.arange(3)).ravel(), mesh.node_dof_row[hi]])
    assert len(rows) > 0
    return np.sort(rows).astype(np.int32)


@pytest.mark.parametrize("how", ["layers", "random"])
@pytest.mark.parametrize("kin", [fcg.LINEAR, fcg.TOTLAG], ids=["linear", "totlag"])
@pytest.mark.parametrize("case", H27_CASES)
def test_matrix_free_action_and_diagonal_honour_the_table(case, kin, how):
    torch, dev = _dev()
    mesh, u, Es, nus, em, Kr, fr, soft = _reference(case, kin, how)
    ev = fcg.Evaluator(mesh, kinematics=kin, youngs=E0, poisson=NU0, path=fcg.PATH_GENERAL)
    ev.set_element_materials(Es, nus, em)
    x = np.random.default_rng(3).standard_normal(mesh.n_cols)
    # the action against oracle-K x and against fcg_spmv on the library's own K
    y = _apply(ev, u, x)
    yo = _csr_mult(mesh, Kr, x)
    assert np.all(np.isfinite(y))
    print(f"{case} kin {kin} {how}: |y - y_oracle| / |y_oracle| = {_rel(y, yo):.3e}")
    assert np.linalg.norm(y - yo) <= 1e-12 * np.linalg.norm(yo)
    if len(soft):
        assert np.linalg.norm(y[soft] - yo[soft]) <= 1e-12 * np.linalg.norm(yo[soft])
    Kg, _ = _evaluate(ev, mesh, u)
    ys = torch.empty(mesh.n_rows, dtype=torch.float64, device=dev)
    ev.spmv(torch.from_numpy(Kg).to(dev), torch.from_numpy(x).to(dev), ys)
    torch.cuda.synchronize()
    assert np.linalg.norm(y - ys.cpu().numpy()) <= 1e-13 * np.linalg.norm(yo)
    assert np.array_equal(y, _apply(ev, u, x))
    # the diagonal blocks against the blocks of both K, with Dirichlet rows
    dbc = _dbc_rows(mesh)

    def unit_rows(D):
        D = D.copy()
        for r in dbc:
            D[r // 3, r % 3] = np.eye(3)[r % 3]
        return D

    Do, Dk = _blocks_of(mesh, Kr), _blocks_of(mesh, Kg)
    D = _diag(ev, u)
    nrm = np.linalg.norm(Do)
    print(f"{case} kin {kin} {how}: |D - D_oracle| / |D_oracle| = {np.linalg.norm(D - Do) / nrm:.3e}")
    assert np.linalg.norm(D - Do) <= 1e-12 * nrm
    assert np.linalg.norm(D - Dk) <= 1e-13 * nrm
    if len(soft):
        sb = np.unique(soft // 3)
        assert np.linalg.norm(D[sb] - Do[sb]) <= 1e-12 * np.linalg.norm(Do[sb])
    Dd = _diag(ev, u, dbc)
    ref = unit_rows(Do)
    assert np.linalg.norm(Dd - ref) <= 1e-12 * np.linalg.norm(ref)
    for r in dbc:
        assert np.array_equal(Dd[r // 3, r % 3], np.eye(3)[r % 3])
    assert np.array_equal(Dd, _diag(ev, u, dbc))
    # the inverses: |D (D + dD)^-1 - I| <= cond(D) |dD| / |D| with the 1e-12 on D
    Di = _diag(ev, u, dbc, want="dinv")
    cond = np.linalg.cond(ref)
    res = np.abs(ref @ Di - np.eye(3)).max(axis=(1, 2))
    assert np.all(res <= 1e-12 * cond)
    assert np.array_equal(Di, _diag(ev, u, dbc, want="dinv"))
    ev.close()


# -------------------------------------------------------------------------------- 4. refusals
def _refused(ev, mesh, u, call, needle):
    before = _evaluate(ev, mesh, u)
    info = fcg.FcgInfo()
    fcg.lib().fcg_get_info(ev._h, ctypes.byref(info))
    n_before, bytes_before = ev.n_materials, info.device_bytes
    with pytest.raises(fcg.FcgError) as ei:
        call()
    assert ei.value.code == 3
    assert needle in str(ei.value), str(ei.value)
    assert ev.n_materials == n_before
    fcg.lib().fcg_get_info(ev._h, ctypes.byref(info))
    assert info.device_bytes == bytes_before
    after = _evaluate(ev, mesh, u)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_lattice_paths_refuse_a_table():
    _dev()
    h8 = fcg.BoxMesh(fcg.HEX8, (3, 2, 2))
    ev = fcg.Evaluator(h8, kinematics=fcg.LINEAR, youngs=E0, poisson=NU0, path=fcg.PATH_STRUCTURED)
    assert ev.info.path == fcg.PATH_STRUCTURED
    em = np.zeros(h8.n_ele, dtype=np.int32)
    _refused(ev, h8, h8.u_col(1e-3), lambda: ev.set_element_materials([10.0], [0.25], em), "FCG_PATH_GATHER")
    ev.set_element_materials(None)  # the reset is no table: accepted everywhere
    ev.close()
    h27 = fcg.BoxMesh(fcg.HEX27, (2, 2, 2))
    ev = fcg.Evaluator(h27, kinematics=fcg.TOTLAG, youngs=E0, poisson=NU0, path=fcg.PATH_COLORED)
    assert ev.info.path == fcg.PATH_COLORED
    em = np.zeros(h27.n_ele, dtype=np.int32)
    _refused(ev, h27, h27.u_col(5e-2), lambda: ev.set_element_materials([10.0], [0.25], em), "FCG_PATH_GENERAL")
    ev.close()


def test_bad_tables_are_refused_and_leave_the_table_in_force():
    _dev()
    mesh = fcg.BoxMesh(fcg.HEX8, (3, 2, 2), jitter=0.1, seed=3)
    u = mesh.u_col(5e-2)
    Es, nus = MATS[fcg.MAT_STVK]
    em = _assign(mesh, 3, "layers")
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E0, poisson=NU0, path=fcg.PATH_GATHER)
    ev.set_element_materials(Es, nus, em)
    bad = em.copy()
    bad[5] = 3
    _refused(ev, mesh, u, lambda: ev.set_element_materials(Es, nus, bad), "ele_mat[5]")
    bad[5] = -1
    _refused(ev, mesh, u, lambda: ev.set_element_materials(Es, nus, bad), "ele_mat[5]")
    _refused(ev, mesh, u, lambda: ev.set_element_materials([10.0, 0.0, 200.0], nus, em), "youngs[1]")
    _refused(ev, mesh, u, lambda: ev.set_element_materials([10.0, -5.0, 200.0], nus, em), "youngs[1]")
    _refused(ev, mesh, u, lambda: ev.set_element_materials(Es, [0.25, 0.3, 0.5], em), "poisson[2]")
    _refused(ev, mesh, u, lambda: ev.set_element_materials(Es, [-1.5, 0.3, 0.45], em), "poisson[0]")
    _refused(ev, mesh, u, lambda: ev.set_element_materials(Es, None, em), "NULL")
    _refused(ev, mesh, u, lambda: ev.set_element_materials(Es, nus, None), "NULL")
    # the C entry point itself with a NULL youngs
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    nu_a = np.array(nus)
    rc = fcg.lib().fcg_set_element_materials(ev._h, 3, None, nu_a.ctypes.data_as(dp), em.ctypes.data_as(ip))
    assert rc == 3
    rc = fcg.lib().fcg_set_element_materials(ev._h, -1, None, None, None)
    assert rc == 3
    # still the table set at the start
    Kr, fr = _oracle_hetero(mesh, fcg.HEX8, fcg.TOTLAG, fcg.MAT_STVK, Es, nus, em, u)
    Kg, fg = _evaluate(ev, mesh, u)
    assert _rel(Kg, Kr) <= 1e-12 and _rel(fg, fr) <= 1e-10
    ev.close()


def test_fused_tsi_refuses_a_tabled_structural_context():
    torch, dev = _dev()
    mesh = fcg.BoxMesh(fcg.HEX8, (3, 3, 3))
    tev = fcg.TsiEvaluator(mesh, E0, NU0, 1.2e-5, 293.0, 50.0)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E0, poisson=NU0, path=fcg.PATH_GATHER)
    ev.set_element_materials([E0, 2.0 * E0], [NU0, NU0], _assign(mesh, 2, "layers"))
    g = tev.graph
    z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    out = {k: z(n) for k, n in (("Kss", mesh.nnz), ("fs", mesh.n_rows), ("Kst", g.nnz_st),
                                ("Kts", g.nnz_ts), ("Ktt", g.nnz_tt), ("fT", g.n_rows_t))}
    with pytest.raises(fcg.FcgError) as ei:
        tev.evaluate_fused(ev, fcg.OVERWRITE, z(mesh.n_cols), z(mesh.n_cols), z(g.n_cols_t), 1.0, 1.0, **out)
    assert ei.value.code == 3
    assert "fcg_set_element_materials" in str(ei.value)
    ev.close()


# ---------------------------------------------------------------------------------- 5. Newton
def _free_residual(mesh, celltype, Es, nus, em, u_row, fext, dbc):
    """|f_int(u) - f_ext| on the free rows from the heterogeneous oracle (single rank: row = column)."""
    _, f = _oracle_hetero(mesh, celltype, fcg.TOTLAG, fcg.MAT_STVK, Es, nus, em, u_row, want_k=False)
    r = f - fext
    r[dbc] = 0.0
    return np.linalg.norm(r)


def test_newton_hex8_cantilever_with_a_stiff_half_native_amg():
    _dev()
    box = fcg.BoxMesh(fcg.HEX8, (6, 3, 3), upper=(3.0, 1.0, 1.0))
    dis = fcg.Discretization.renumbered(box, seed=2)
    x = dis.node_x[:, 0]
    clamp, tip = np.nonzero(np.isclose(x, x.min()))[0], np.nonzero(np.isclose(x, x.max()))[0]
    dbc = np.sort((dis.node_dof_row[clamp][:, None] + np.arange(3)).ravel()).astype(np.int32)
    fext = np.zeros(dis.n_rows)
    fext[dis.node_dof_row[tip] + 2] = -0.5 / len(tip)
    Es, nus = [E0, 10.0 * E0], [NU0, 0.25]
    cx = dis.node_x[dis.ele_nodes][:, :, 0].mean(axis=1)
    em = (cx < 1.5).astype(np.int32)  # the clamped half is the stiff one
    assert 0 < em.sum() < dis.n_ele

    def solve(table):
        ev = fcg.Evaluator(dis, kinematics=fcg.TOTLAG, youngs=E0, poisson=NU0, path=fcg.PATH_GATHER)
        if table:
            ev.set_element_materials(Es, nus, em)
        solver = amg.NativeAMG(dis, ev, dbc)
        nt = newton.StaticNewton(ev, fext, dbc, tol_res=1e-10 * np.linalg.norm(fext), tol_inc=1e-9,
                                 lin_rtol=1e-12, linear_solver=solver)
        u = nt.solve().cpu().numpy()
        solver.close()
        ev.close()
        return u

    u = solve(True)
    res = _free_residual(dis, fcg.HEX8, Es, nus, em, u, fext, dbc)
    print(f"hex8 stiff half: |f_int - f_ext| / |f_ext| = {res / np.linalg.norm(fext):.3e}")
    assert res <= 1e-8 * np.linalg.norm(fext)
    # the stiff half shows: the tip moves less than that of the uniform beam
    tz = dis.node_dof_row[tip] + 2
    assert np.abs(u[tz]).mean() < 0.9 * np.abs(solve(False)[tz]).mean()


def test_newton_hex27_cantilever_with_a_stiff_layer_matrix_free():
    _dev()
    n = 6
    mesh = fcg.BoxMesh(fcg.HEX27, (n, n, n), upper=(2.0, 1.0, 1.0))
    clamp = lambda m: np.isclose(m.node_x[:, 0], 0.0)  # noqa: E731
    nodes = np.nonzero(clamp(mesh))[0]
    dbc = np.sort((mesh.node_dof_row[nodes][:, None] + np.arange(3)).ravel()).astype(np.int32)
    faces = mesh.ele_nodes[mesh.ele_ijk[:, 0] == n - 1][:, [1, 2, 6, 5, 9, 14, 17, 13, 22]]
    fext = np.zeros(mesh.n_rows)
    fcg.neumann_surface(fcg.HEX27, faces, mesh.node_x, mesh.node_dof_row, [1, 1, 1], [0.0, 0.0, -2.0], fext)
    Es, nus = [E0, 4.0 * E0], [NU0, 0.25]
    em = (mesh.ele_ijk[:, 2] == n - 1).astype(np.int32)  # the top layer is the stiff one
    res = {}
    for asm in (True, False):
        ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E0, poisson=NU0)
        ev.set_element_materials(Es, nus, em)
        mg = mgm.Multigrid(mesh, ev, clamp, E0, NU0, min_intervals=2, matrix_free=True, outer_matrix_free=True)
        nt = newton.StaticNewton(ev, fext, dbc, tol_res=1e-10 * np.linalg.norm(fext), tol_inc=1e-9,
                                 lin_rtol=1e-10, linear_solver=mg, assemble_tangent=asm)
        res[asm] = nt.solve().cpu().numpy()
        assert (nt.K is None) == (not asm)
        ev.close()
    assert np.linalg.norm(res[False] - res[True]) <= 1e-9 * np.linalg.norm(res[True])
    r = _free_residual(mesh, fcg.HEX27, Es, nus, em, res[False], fext, dbc)
    print(f"hex27 stiff layer: |f_int - f_ext| / |f_ext| = {r / np.linalg.norm(fext):.3e}")
    assert r <= 1e-8 * np.linalg.norm(fext)
