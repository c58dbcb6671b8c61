"""GenAlpha.internal_energy(): the strain energy of the integrator's current displacement from the
elements' Gauss points (fcg_gp_stress), against 1/2 d^T (K d) with K d from fcg_spmv."""

import importlib

import numpy as np
import pytest

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")
dynamics = importlib.import_module("4c_amd.dynamics")

gpu = pytest.mark.gpu
E, NU, RHO = 210.0, 0.3, 0.05


@gpu
def test_internal_energy_of_linear_cantilever():
    """A (4,2,2) linear hex8 box clamped at x = 0 under a step tip load: after a few steps the
    strain energy summed over the elements is 1/2 d^T K d.  For linear kinematics and StVK both are
    the same quadratic form, summed in different orders: 1e-12 relative, the project's figure for
    float64 comparisons.  energies() keeps returning (kinetic, None)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    iv = (4, 2, 2)
    mesh = fcg.BoxMesh(fcg.HEX8, iv, upper=(float(iv[0]), 1.0, 1.0))
    X = mesh.node_x
    clamped = np.nonzero(np.isclose(X[:, 0], 0.0))[0]
    dbc = np.sort((mesh.node_dof_row[clamped][:, None] + np.arange(3)).ravel()).astype(np.int32)
    tip = np.nonzero(np.isclose(X[:, 0], float(iv[0])))[0]
    fext = np.zeros(mesh.n_rows)
    fext[mesh.node_dof_row[tip] + 2] = -1e-2 / len(tip)
    ev = fcg.Evaluator(mesh, kinematics=fcg.LINEAR, youngs=E, poisson=NU)
    ga = dynamics.GenAlpha(ev, RHO, 0.5, fext, dbc, tol_res=1e-12, tol_inc=1e-10)
    ga.initialize()
    assert ga.internal_energy() == 0.0
    for _ in range(3):
        ga.step()
    assert float(ga.d.abs().max()) > 0.0
    K = torch.empty(mesh.nnz, dtype=torch.float64, device=dev)
    f = torch.empty(mesh.n_rows, dtype=torch.float64, device=dev)
    y = torch.empty(mesh.n_rows, dtype=torch.float64, device=dev)
    ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, ga.d, f, K)
    ev.spmv(K, ga.d, y)
    want = 0.5 * float(torch.dot(ga.d, y))
    got = ga.internal_energy()
    rel = abs(got - want) / abs(want)
    print("internal energy", got, "1/2 d^T K d", want, "relative difference", rel)
    assert want > 0.0 and rel <= 1e-12
    kin, internal = ga.energies()
    assert kin > 0.0 and internal is None
