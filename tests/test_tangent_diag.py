"""Matrix-free nodal diagonal blocks of hex27 StVK (fcg_tangent_diag, fcg_hex27.hip) and the
Newton loop that never assembles K (newton.StaticNewton(assemble_tangent=False)).

The 3 x 3 block an element adds at its node a, with d = dN_a(xi_g), n = J^-T d, v = F n:

    K_aa = sum_g fac [ (lambda + mu) v v^T + mu |n|^2 F F^T + (n . S n) I ],   S = C E(u)

* CPU: the closed form against an independent numpy element tangent sum_g fac (B_a^T C B_a +
  K_geo,aa) (4C_solid_3D_ele_calc_lib.hpp:872-927) on one jittered element, 1e-12 per block;
* GPU: the blocks against the oracle's assembled K (`oracle/`, Dirichlet rows applied in numpy) at
  1e-12, against the library's own K at 1e-13, bitwise reproducible; the inverses against numpy;
* the hex27 TotLag cantilever solved by Multigrid(matrix_free=True, outer_matrix_free=True) with
  and without the assembled tangent: same displacement (1e-9), steps, reactions (1e-9), FCG
  iteration totals within 10 %.
"""

import ctypes
import functools
import importlib

import numpy as np
import pytest

E, NU = 210.0, 0.3
LAM = E * NU / ((1.0 + NU) * (1.0 - 2.0 * NU))
MU = E / (2.0 * (1.0 + NU))


# ------------------------------------------------------------------------------ CPU: the formula
def _element(seed):
    """One hex27 element in lattice node order: jittered X, a random u, dN at the 27 Gauss points
    and their weights."""
    rng = np.random.default_rng(seed)
    L = lambda r: np.array([0.5 * r * (r - 1.0), 1.0 - r * r, 0.5 * r * (r + 1.0)])  # noqa: E731
    dL = lambda r: np.array([r - 0.5, -2.0 * r, r + 0.5])  # noqa: E731
    lat = np.array([(i, j, k) for k in range(3) for j in range(3) for i in range(3)])
    X = (lat - 1.0) * np.array([0.6, 0.5, 0.45]) + rng.uniform(-0.06, 0.06, (27, 3))
    u = rng.uniform(-0.03, 0.03, (27, 3))
    gp, gw = np.array([-np.sqrt(0.6), 0.0, np.sqrt(0.6)]), np.array([5.0, 8.0, 5.0]) / 9.0
    dN, w = np.empty((27, 27, 3)), np.empty(27)
    for g, (p, q, r) in enumerate(lat):
        l0, l1, l2 = L(gp[p]), L(gp[q]), L(gp[r])
        d0, d1, d2 = dL(gp[p]), dL(gp[q]), dL(gp[r])
        for a, (i, j, k) in enumerate(lat):
            dN[g, a] = (d0[i] * l1[j] * l2[k], l0[i] * d1[j] * l2[k], l0[i] * l1[j] * d2[k])
        w[g] = gw[p] * gw[q] * gw[r]
    return X, u, dN, w


def _point(X, u, dN_g, totlag):
    """n_a = grad_X N_a (27 x 3), F, S (3 x 3) and det J at one Gauss point."""
    J = dN_g.T @ X  # J[d, k] = dX_k / dxi_d
    n = np.linalg.solve(J, dN_g.T).T
    F = np.eye(3) + (u.T @ n if totlag else 0.0)
    Eg = 0.5 * (F.T @ F - np.eye(3)) if totlag else np.zeros((3, 3))
    S = LAM * np.trace(Eg) * np.eye(3) + 2.0 * MU * Eg
    return n, F, S, np.linalg.det(J)


def _closed_form(X, u, dN, w, totlag):
    K = np.zeros((27, 3, 3))
    for g in range(27):
        n, F, S, det = _point(X, u, dN[g], totlag)
        b = F @ F.T
        for a in range(27):
            v = F @ n[a]
            K[a] += det * w[g] * ((LAM + MU) * np.outer(v, v) + MU * (n[a] @ n[a]) * b +
                                  (n[a] @ S @ n[a]) * np.eye(3))
    return K


def _b_matrix_form(X, u, dN, w, totlag):
    """sum_g fac (B_a^T C B_a + K_geo,aa) with the 6 x 3 B operator and the 6 x 6 Voigt C
    (strains xx yy zz xy yz xz, engineering shear), written out independently of the closed form."""
    C = np.zeros((6, 6))
    C[:3, :3] = LAM
    C[np.arange(3), np.arange(3)] = LAM + 2.0 * MU
    C[np.arange(3, 6), np.arange(3, 6)] = MU
    K = np.zeros((27, 3, 3))
    for g in range(27):
        n, F, S, det = _point(X, u, dN[g], totlag)
        for a in range(27):
            B = np.empty((6, 3))
            for i in range(3):
                B[0, i] = F[i, 0] * n[a, 0]
                B[1, i] = F[i, 1] * n[a, 1]
                B[2, i] = F[i, 2] * n[a, 2]
                B[3, i] = F[i, 0] * n[a, 1] + F[i, 1] * n[a, 0]
                B[4, i] = F[i, 1] * n[a, 2] + F[i, 2] * n[a, 1]
                B[5, i] = F[i, 2] * n[a, 0] + F[i, 0] * n[a, 2]
            K[a] += det * w[g] * (B.T @ C @ B + (n[a] @ S @ n[a]) * np.eye(3))
    return K


@pytest.mark.parametrize("totlag", [False, True])
def test_closed_form_equals_b_matrix_form(totlag):
    X, u, dN, w = _element(7)
    assert abs(dN.sum(axis=1)).max() < 1e-14  # a partition of unity
    Kc, Kb = _closed_form(X, u, dN, w, totlag), _b_matrix_form(X, u, dN, w, totlag)
    if totlag:
        assert np.linalg.norm(Kc - _closed_form(X, 0.0 * u, dN, w, True)) > 1e-3 * np.linalg.norm(Kc)
    for a in range(27):
        assert np.linalg.norm(Kc[a] - Kb[a]) <= 1e-12 * np.linalg.norm(Kb[a]), a
        assert np.array_equal(Kc[a], Kc[a].T)


# ------------------------------------------------------------------------------------------ GPU
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pkg = importlib.import_module("4c_amd")
    return (torch, torch.device("cuda:0"), pkg.fcg, importlib.import_module("4c_amd.multigrid"),
            importlib.import_module("4c_amd.newton"))


CASES = {
    "1x1x1": dict(shape=(1, 1, 1), jitter=0.0),          # fewer chunks than XCDs
    "3x2x2": dict(shape=(3, 2, 2), jitter=0.1),
    "2x3x1": dict(shape=(2, 3, 1), jitter=0.0),
    "3x3x1": dict(shape=(3, 3, 1), jitter=0.05),          # odd element count: a one-element last pass
    "5x5x5": dict(shape=(5, 5, 5), jitter=0.05),
    "renumbered": dict(shape=(3, 3, 2), jitter=0.1, renumbered=True),
    "ghosted": dict(shape=(4, 2, 2), jitter=0.0, rank=1, nranks=2),
}


def _make_mesh(fcg, case, jitter=None):
    c = CASES[case]
    kw = dict(jitter=c["jitter"] if jitter is None else jitter, seed=5 if c.get("renumbered") else 11)
    if "rank" in c:
        kw.update(rank=c["rank"], nranks=c["nranks"])
    box = fcg.BoxMesh(fcg.HEX27, c["shape"], **kw)
    return fcg.Discretization.renumbered(box, seed=3) if c.get("renumbered") else box


def _blocks_of(mesh, K):
    """The 3 x 3 nodal diagonal blocks of CSR values K: block k = rows 3k..3k+2 at the columns of
    the same DOFs (columns sorted within a row)."""
    row_gid = getattr(mesh, "row_gid", None)
    if row_gid is None:
        col_of_row = np.arange(mesh.n_rows)
    else:
        order = np.argsort(mesh.col_gid)
        col_of_row = order[np.searchsorted(mesh.col_gid[order], row_gid)]
        assert np.array_equal(mesh.col_gid[col_of_row], row_gid)
    D = np.empty((mesh.n_rows // 3, 3, 3))
    for i in range(mesh.n_rows):
        s, e = mesh.rowptr[i], mesh.rowptr[i + 1]
        k, d = divmod(i, 3)
        want = col_of_row[3 * k:3 * k + 3]
        j = s + np.searchsorted(mesh.col_lid[s:e], want)
        assert np.array_equal(mesh.col_lid[j], want)
        D[k, d] = K[j]
    return D


@functools.lru_cache(maxsize=None)
def _reference(case, kin):
    """(mesh, u, oracle blocks of K(u) before Dirichlet rows): computed once per case, read-only."""
    from parity_util import oracle_evaluate, oracle_evaluate_single
    fcg = importlib.import_module("4c_amd").fcg
    mesh = _make_mesh(fcg, case)
    if CASES[case].get("renumbered"):
        u = np.random.default_rng(9).uniform(-1e-2, 1e-2, mesh.n_cols)
        err, _, Ko, _ = oracle_evaluate_single(mesh, kin, E, NU, u)
    else:
        u = mesh.u_col(2e-2)
        err, _, Ko, _ = oracle_evaluate(mesh, kin, E, NU, u)
    assert err == 0
    Do = _blocks_of(mesh, Ko)
    Do.setflags(write=False)
    u.setflags(write=False)
    return mesh, u, Do


def _diag(ev, u, torch, dev, dbc=None, want="diag"):
    n = ev.info.n_rows // 3
    out = torch.full((9 * n,), float("nan"), dtype=torch.float64, device=dev)
    rows = None if dbc is None else torch.from_numpy(np.asarray(dbc, dtype=np.int32)).to(dev)
    ev.tangent_diag(None if u is None else torch.from_numpy(np.array(u)).to(dev), rows, **{want: out})
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, 3, 3)


def _unit_rows(D, dbc):
    D = D.copy()
    for r in dbc:
        D[r // 3, r % 3] = np.eye(3)[r % 3]
    return D


def _face_rows(fcg, case, axis, side, dofs):
    """Owned rows of the DOFs `dofs` of the nodes on a face of the (unjittered) box."""
    flat = _make_mesh(fcg, case, jitter=0.0)
    x = flat.node_x[:, axis]
    nodes = np.nonzero(np.isclose(x, x.min() if side == 0 else x.max()) & (flat.node_dof_row >= 0))[0]
    assert len(nodes) > 0
    return np.sort((flat.node_dof_row[nodes][:, None] + np.asarray(dofs)).ravel()).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("kin", [0, 1], ids=["linear", "totlag"])
@pytest.mark.parametrize("case", list(CASES))
def test_tangent_diag_matches_oracle(case, kin):
    torch, dev, fcg, _, _ = _gpu()
    mesh, u, Do = _reference(case, kin)
    ev = fcg.Evaluator(mesh, kinematics=kin, youngs=E, poisson=NU)
    D = _diag(ev, u, torch, dev)
    assert np.all(np.isfinite(D))
    nrm = np.linalg.norm(Do)
    print(f"{case} kin {kin}: |D - D_oracle| / |D_oracle| = {np.linalg.norm(D - Do) / nrm:.3e}")
    assert np.linalg.norm(D - Do) <= 1e-12 * nrm
    # the blocks of the library's own assembled K at the same state
    f64 = dict(dtype=torch.float64, device=dev)
    K = torch.zeros(mesh.nnz, **f64)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, torch.from_numpy(np.array(u)).to(dev),
                       torch.zeros(mesh.n_rows, **f64), K)
    torch.cuda.synchronize()
    Dk = _blocks_of(mesh, K.cpu().numpy())
    print(f"{case} kin {kin}: |D - D_K| / |D_oracle| = {np.linalg.norm(D - Dk) / nrm:.3e}")
    assert np.linalg.norm(D - Dk) <= 1e-13 * nrm
    # deterministic; linear kinematics do not read u
    assert np.array_equal(D, _diag(ev, u, torch, dev))
    if kin == fcg.LINEAR:
        assert np.array_equal(D, _diag(ev, None, torch, dev))
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kin", [0, 1], ids=["linear", "totlag"])
@pytest.mark.parametrize("which", ["clamped_face", "x_dof_only"])
def test_tangent_diag_dirichlet_rows(which, kin):
    """(a) all three DOFs of the x = 0 face; (b) only the x-DOF of the nodes of the x = max face:
    a partly constrained node, a nonsymmetric block.  Unit rows, columns kept."""
    torch, dev, fcg, _, _ = _gpu()
    case = "3x2x2"
    mesh, u, Do = _reference(case, kin)
    dbc = _face_rows(fcg, case, 0, 0, [0, 1, 2]) if which == "clamped_face" else _face_rows(fcg, case, 0, 1, [0])
    ref = _unit_rows(Do, dbc)
    if which == "x_dof_only":
        k = dbc[0] // 3
        assert not np.allclose(ref[k], ref[k].T)
    ev = fcg.Evaluator(mesh, kinematics=kin, youngs=E, poisson=NU)
    D = _diag(ev, u, torch, dev, dbc)
    assert np.linalg.norm(D - ref) <= 1e-12 * np.linalg.norm(ref)
    for r in dbc:  # the unit rows are exact
        assert np.array_equal(D[r // 3, r % 3], np.eye(3)[r % 3])
    # the rows are per call: the next call without them gives the unmodified blocks
    assert np.linalg.norm(_diag(ev, u, torch, dev) - Do) <= 1e-12 * np.linalg.norm(Do)
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kin", [0, 1], ids=["linear", "totlag"])
@pytest.mark.parametrize("case", ["3x2x2", "renumbered", "ghosted"])
def test_tangent_diag_inverse(case, kin):
    torch, dev, fcg, _, _ = _gpu()
    mesh, u, Do = _reference(case, kin)
    dbc = _face_rows(fcg, case, 0, 1, [0]) if case == "3x2x2" else np.zeros(0, dtype=np.int32)
    ref = _unit_rows(Do, dbc)
    ev = fcg.Evaluator(mesh, kinematics=kin, youngs=E, poisson=NU)
    n = mesh.n_rows // 3
    f64 = dict(dtype=torch.float64, device=dev)
    diag, dinv = torch.empty(9 * n, **f64), torch.empty(9 * n, **f64)
    ev.tangent_diag(torch.from_numpy(np.array(u)).to(dev), torch.from_numpy(dbc).to(dev), diag=diag, dinv=dinv)
    Di = dinv.cpu().numpy().reshape(n, 3, 3)
    assert np.array_equal(diag.cpu().numpy().reshape(n, 3, 3), _diag(ev, u, torch, dev, dbc))
    cond = np.linalg.cond(ref)
    # first order: |D^-1 (D + dD) - I| <= cond(D) |dD| / |D| with the 1e-12 on D
    res = np.abs(ref @ Di - np.eye(3)).max(axis=(1, 2))
    print(f"{case} kin {kin}: max |D dinv - I| / cond = {(res / cond).max():.3e}, max cond {cond.max():.2e}")
    assert np.all(res <= 1e-12 * cond)
    # independent of the block order: z = D^-1 r through fcg_block_jacobi_apply
    r = np.random.default_rng(2).standard_normal(mesh.n_rows)
    rt, z = torch.from_numpy(r).to(dev), torch.empty(mesh.n_rows, **f64)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = fcg.lib().fcg_block_jacobi_apply(ev._h, vp(dinv), vp(rt), vp(z), ctypes.c_double(1.0), 0,
                                          ev._stream(None))
    assert rc == 0
    torch.cuda.synchronize()
    zr = np.linalg.solve(ref, r.reshape(n, 3, 1)).reshape(n, 3)
    dz = np.linalg.norm(z.cpu().numpy().reshape(n, 3) - zr, axis=1)
    assert np.all(dz <= 1e-12 * cond * np.linalg.norm(zr, axis=1))
    ev.close()


@pytest.mark.gpu
def test_tangent_diag_refusals():
    torch, dev, fcg, mgm, newton = _gpu()
    f64 = dict(dtype=torch.float64, device=dev)
    h8 = fcg.BoxMesh(fcg.HEX8, (2, 2, 2))
    ev = fcg.Evaluator(h8, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    with pytest.raises(fcg.FcgError):
        ev.tangent_diag(None, diag=torch.empty(3 * h8.n_rows, **f64))
    ev.close()
    h27 = fcg.BoxMesh(fcg.HEX27, (2, 2, 2))
    ev = fcg.Evaluator(h27, kinematics=fcg.TOTLAG, youngs=10.0, poisson=0.25,
                       material=fcg.MAT_ELASTHYPER_COUPNEOHOOKE)
    with pytest.raises(fcg.FcgError):
        ev.tangent_diag(torch.zeros(h27.n_cols, **f64), diag=torch.empty(3 * h27.n_rows, **f64))
    ev.close()
    ev = fcg.Evaluator(h27, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    with pytest.raises(fcg.FcgError):
        ev.tangent_diag(None)
    # a solver that reads K refuses K = None, and the Newton loop refuses such a solver
    clamp = lambda m: np.isclose(m.node_x[:, 0], 0.0)  # noqa: E731
    ev.close()
    h27 = fcg.BoxMesh(fcg.HEX27, (4, 4, 4))
    ev = fcg.Evaluator(h27, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    mg = mgm.Multigrid(h27, ev, clamp, E, NU, min_intervals=2, matrix_free=True, outer_matrix_free=False)
    assert mg.needs_matrix
    b = torch.zeros(h27.n_rows, **f64)
    with pytest.raises(ValueError):
        mg.solve(None, b, torch.zeros_like(b), 1e-8)
    fext, dbc = np.zeros(h27.n_rows), np.zeros(0, dtype=np.int32)
    with pytest.raises(ValueError):
        newton.StaticNewton(ev, fext, dbc, linear_solver=mg, assemble_tangent=False)
    with pytest.raises(ValueError):
        newton.StaticNewton(ev, fext, dbc, linear_solver=None, assemble_tangent=False)
    ev.close()


@pytest.mark.gpu
def test_newton_without_assembled_tangent():
    """The cantilever of test_newton_multigrid_matrix_free_fine_smoother (hex27 6^3, TotLag) with
    the fully matrix-free multigrid, with and without the assembled tangent."""
    torch, dev, fcg, mgm, newton = _gpu()
    n = 6
    mesh = fcg.BoxMesh(fcg.HEX27, (n, n, n), upper=(2.0, 1.0, 1.0))
    clamp = lambda m: np.isclose(m.node_x[:, 0], 0.0)  # noqa: E731
    nodes = np.nonzero(clamp(mesh))[0]
    dbc = np.sort((mesh.node_dof_row[nodes][:, None] + np.arange(3)).ravel()).astype(np.int32)
    faces = mesh.ele_nodes[mesh.ele_ijk[:, 0] == n - 1][:, [1, 2, 6, 5, 9, 14, 17, 13, 22]]
    fext = np.zeros(mesh.n_rows)
    fcg.neumann_surface(fcg.HEX27, faces, mesh.node_x, mesh.node_dof_row, [1, 1, 1],
                        [0.0, 0.0, -2.0], fext)
    res = {}
    for asm in (True, False):
        ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU)
        mg = mgm.Multigrid(mesh, ev, clamp, E, NU, min_intervals=2, matrix_free=True,
                           outer_matrix_free=True)
        assert mg.needs_matrix is False
        nt = newton.StaticNewton(ev, fext, dbc, tol_res=1e-10 * np.linalg.norm(fext), tol_inc=1e-9,
                                 lin_rtol=1e-10, linear_solver=mg, assemble_tangent=asm)
        u = nt.solve().cpu().numpy()
        res[asm] = (u, [h.get("lin_iter") for h in nt.history], nt.freact.cpu().numpy(),
                    [sorted(h) for h in nt.history])
        assert mg.describe()[0]["diag"] == ("assembled K" if asm else "matrix-free")
        if asm:
            assert nt.K.numel() == mesh.nnz
        else:  # no nnz-sized tensor anywhere on the loop object
            assert nt.K is None
            assert not any(torch.is_tensor(v) and v.numel() >= mesh.nnz for v in vars(nt).values())
            assert mg.levels[0].K is None
        ev.close()
    (u0, it0, fr0, keys0), (u1, it1, fr1, keys1) = res[True], res[False]
    assert np.linalg.norm(u1 - u0) <= 1e-9 * np.linalg.norm(u0)
    assert len(it0) == len(it1)
    assert keys0 == keys1  # the history layout
    n0, n1 = sum(i for i in it0 if i), sum(i for i in it1 if i)
    assert abs(n1 - n0) <= 0.1 * n0, (it0, it1)
    assert np.linalg.norm(fr0) > 0.0
    assert np.linalg.norm(fr1 - fr0) <= 1e-9 * np.linalg.norm(fr0)
