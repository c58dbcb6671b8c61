"""The scalar AMG's entry points where no usable device stands behind them: an error code, never a
crash, and no sticky HIP status (tests/test_missing_device.py).  fcg_samg_create takes a thermo
context, which cannot exist without a device, so on a machine without a GPU the path to it ends
at the context's own FCG_ERR_DEVICE; the handle-free kernels (fcg_scsr_spmv,
fcg_scsr_chebyshev_step) report FCG_ERR_DEVICE themselves before they touch a pointer."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

fcg = importlib.import_module("4c_amd").fcg
amg = importlib.import_module("4c_amd.amg")

FCG_ERR_ARG = 3
MISSING = 1 << 20


def test_create_without_a_context_is_refused():
    L = fcg.lib()
    ptr, col = np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32)
    h = ctypes.c_void_p(12345)
    rc = L.fcg_samg_create(None, ptr.ctypes.data, col.ctypes.data, 0, None, None, ctypes.byref(h))
    assert rc == FCG_ERR_ARG and not h.value
    assert L.fcg_samg_levels(None) == 0 and L.fcg_samg_destroy(None) == 0
    assert L.fcg_samg_last_error(None) == b""
    assert L.fcg_samg_level_matrix(None, 0, 0, None, None, None, 0) == -1


def test_scalar_amg_on_a_machine_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_samg.py runs the device path")
    mesh = fcg.BoxMesh(fcg.HEX8, (2, 2, 2))
    with pytest.raises(fcg.FcgError) as e:
        amg.ScalarAMG(fcg.TsiEvaluator(mesh, 210.0, 0.3, 1.2e-5, 293.0, 52.0), np.zeros(0, dtype=np.int32))
    assert e.value.code == fcg.FCG_ERR_DEVICE


def test_level_kernels_reject_a_missing_device():
    L = fcg.lib()
    one = ctypes.c_void_p(8)  # never dereferenced: the device is looked up first
    rc = L.fcg_scsr_spmv(MISSING, 1, 1, one, one, one, one, None, one, 1.0, 0, None)
    assert rc == fcg.FCG_ERR_DEVICE
    rc = L.fcg_scsr_chebyshev_step(MISSING, 1, 1, one, one, one, one, one, one, one, ctypes.c_void_p(16),
                                   0.0, 1.0, 0, None)
    assert rc == fcg.FCG_ERR_DEVICE
    if torch.cuda.is_available():  # no sticky status: torch's next call succeeds
        x = torch.arange(1024, dtype=torch.float64, device="cuda:0")
        assert float((x * 2).sum().item()) == 2.0 * 1023 * 1024 / 2
