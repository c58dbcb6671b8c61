"""Time the matrix-free nodal diagonal blocks of hex27 (fcg_tangent_diag) against the matrix-free
action (fcg_tangent_apply) at the same state; also the workload of a counter pass of
h27_diag_kernel: python tools/probes/diag_timing.py --n 100 --kinem totlag"""

import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
fcg = importlib.import_module("4c_amd").fcg

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=40)
ap.add_argument("--kinem", default="totlag")
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
kin = fcg.TOTLAG if a.kinem == "totlag" else fcg.LINEAR
dev = torch.device("cuda:0")
mesh = fcg.BoxMesh(fcg.HEX27, (a.n, a.n, a.n))
ev = fcg.Evaluator(mesh, kinematics=kin, youngs=210.0, poisson=0.3)
f64 = dict(dtype=torch.float64, device=dev)
u = torch.from_numpy(mesh.u_col(1e-2)).to(dev)
nodes = np.nonzero(np.isclose(mesh.node_x[:, 0], 0.0))[0]
dbc = torch.from_numpy(np.sort((mesh.node_dof_row[nodes][:, None] + np.arange(3)).ravel()).astype(np.int32)).to(dev)
x = torch.randn(mesh.n_cols, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
y = torch.empty(mesh.n_rows, **f64)
diag, dinv = torch.empty(3 * mesh.n_rows, **f64), torch.empty(3 * mesh.n_rows, **f64)


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


ms_apply = timed(lambda: ev.tangent_apply(u, x, y))
ms_diag = timed(lambda: ev.tangent_diag(u, dbc, diag=diag))
ms_dinv = timed(lambda: ev.tangent_diag(u, dbc, dinv=dinv))  # drains the stream each call
info = fcg.FcgInfo()
fcg.lib().fcg_get_info(ev._h, ctypes.byref(info))  # after the first calls: their buffers counted
print(json.dumps({"config": f"hex27-{a.kinem}-{a.n}^3", "elements": mesh.n_ele,
                  "ms_tangent_apply": ms_apply, "ms_tangent_diag_blocks": ms_diag,
                  "ms_tangent_diag_inverse_sync": ms_dinv,
                  "device_bytes": int(info.device_bytes)}), flush=True)
