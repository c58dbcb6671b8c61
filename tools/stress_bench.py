"""Timings of the stress output on one GPU (profiles/stress/README.md), one JSON line per mesh:
  gp_stress_all     fcg_gp_stress with PK2 + GL + energy
  gp_stress_energy  fcg_gp_stress with the energy only
  gp_to_nodes       fcg_gp_to_nodes of the PK2 stresses
each beside the time its compulsory bytes would take at the copy bandwidth fcg_measure_hbm reports
in the same run, and beside one FCG_CALC_INTERNALFORCE evaluate of the same context.  Bytes counted
per call (npe nodes and ngp Gauss points per element):
  gp_stress     n_ele (4 npe [ele_nodes] + 96 ngp [stress + strain] + 8 [energy])
                + n_node (24 [X] + 4 [dof] + 24 [u]), every node read once
  energy only   the same without the 96 ngp
  gp_to_nodes   n_ele 48 ngp [gp, read once] + 8 incidences + 12 n_node [plan] + 48 owned nodes
hipEvents around windows of repeated calls after a warm-up; the window is sized from a pilot so
that it lasts about `--seconds`, and the median of `--windows` windows is reported with their range.
usage: stress_bench.py [--hex8-n 100] [--hex27-n 40] [--kinematics totlag] [--seconds 0.5]"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fcg = importlib.import_module("4c_amd").fcg

ap = argparse.ArgumentParser()
ap.add_argument("--hex8-n", type=int, default=100, help="the benchmark's hex8 mesh (0: skip)")
ap.add_argument("--hex27-n", type=int, default=40, help="bench.py --full's hex27 mesh (0: skip)")
ap.add_argument("--kinematics", default="totlag")
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--windows", type=int, default=5)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_bench.py needs a GPU")
dev = torch.device("cuda:0")
kin = fcg.TOTLAG if a.kinematics == "totlag" else fcg.LINEAR
E, NU = 210.0, 0.3
s = torch.cuda.current_stream(dev)
f64 = dict(dtype=torch.float64, device=dev)


def timed(fn):
    """ms per call: (median, min, max) over the windows"""
    def window(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for _ in range(3):
        fn()
    pilot = window(5)
    reps = int(min(max(math.ceil(a.seconds * 1e3 / max(pilot, 1e-3)), 5), 5000))
    t = sorted(window(reps) for _ in range(a.windows))
    return t[len(t) // 2], t[0], t[-1], reps


copy_gbs, write_gbs = fcg.measure_hbm(0)
for name, ct, n in (("hex8", fcg.HEX8, a.hex8_n), ("hex27", fcg.HEX27, a.hex27_n)):
    if n <= 0:
        continue
    m = fcg.BoxMesh(ct, (n, n, n), jitter=0.02, seed=20251015)
    ev = fcg.Evaluator(m, kinematics=kin, youngs=E, poisson=NU)
    npe = ngp = ev.ngp
    u = torch.from_numpy(m.u_col(1e-3)).to(dev)
    stress = torch.empty(m.n_ele, ngp, 6, **f64)
    strain = torch.empty(m.n_ele, ngp, 6, **f64)
    energy = torch.empty(m.n_ele, **f64)
    nodes = torch.empty(m.n_node, 6, **f64)
    f = torch.zeros(m.n_rows, **f64)
    n_inc = int(np.count_nonzero(m.node_dof_row[m.ele_nodes] >= 0))
    n_owned = int(np.count_nonzero(m.node_dof_row >= 0))
    bytes_in = m.n_ele * 4 * npe + m.n_node * 52
    byt = {"gp_stress_all": bytes_in + m.n_ele * (96 * ngp + 8),
           "gp_stress_energy": bytes_in + m.n_ele * 8,
           "gp_to_nodes": m.n_ele * 48 * ngp + 8 * n_inc + 12 * m.n_node + 48 * n_owned}
    calls = {
        "gp_stress_all": lambda: ev.gp_stress_raw(fcg.STRESS_PK2, fcg.STRAIN_GL, u, stress, strain, energy, stream=s),
        "gp_stress_energy": lambda: ev.gp_stress_raw(fcg.STRESS_NONE, fcg.STRAIN_NONE, u, None, None, energy, stream=s),
        "gp_to_nodes": lambda: ev.gp_to_nodes(stress, out=nodes, stream=s),
    }
    out = {"config": f"{name}-{n}^3-{a.kinematics}", "path": int(ev.info.path), "n_ele": int(m.n_ele),
           "hbm_copy_gbs": copy_gbs, "hbm_write_gbs": write_gbs}
    for what, fn in calls.items():
        med, lo, hi, reps = timed(fn)
        out[what] = {"ms": med, "ms_min": lo, "ms_max": hi, "reps_per_window": reps,
                     "bytes": byt[what], "ms_at_copy_bandwidth": byt[what] / copy_gbs / 1e6,
                     "gbs": byt[what] / med / 1e6}
    med, lo, hi, reps = timed(lambda: ev.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f, stream=s))
    out["evaluate_internalforce"] = {"ms": med, "ms_min": lo, "ms_max": hi, "reps_per_window": reps}
    out["strain_energy_total"] = float(energy.sum())
    print(json.dumps(out), flush=True)
    del ev, stress, strain, energy, nodes
    torch.cuda.empty_cache()
