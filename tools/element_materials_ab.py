#!/usr/bin/env python3
"""What a per-element material table (fcg_set_element_materials) costs, and that contexts without
one are what they were.

    python tools/element_materials_ab.py [--n 100] [--hex27-n 40] [--reps 20] [--tag NAME]

Three workloads, each one JSON line: the renumbered n^3 hex8 box on the node-row gather path
(TotLag K + f), the hex27 hex27-n^3 box on the general path (TotLag K + f) and the matrix-free
action fcg_tangent_apply on that box.  Per workload: the uniform context's kernel time (hipEvents;
median, min, max over --reps evaluates after 5 warm-up ones) and the SHA-256 of its outputs -- run
it with FCG_LIB=<name> on a library built from another commit (4c_amd/lib/libfourc_gpu_<name>.so)
and compare the digests and times; then, when the library has the entry point, the same context
with a 2-material table in layers along x (the stiff half 10 E) and the ratio tabled / uniform.
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fcg = importlib.import_module("4c_amd").fcg

E, NU = 210.0, 0.3


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def stats(ts):
    ts = np.asarray(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


def layers(mesh):
    cx = mesh.node_x[mesh.ele_nodes][:, :, 0].mean(axis=1)
    return (cx > 0.5 * (mesh.node_x[:, 0].min() + mesh.node_x[:, 0].max())).astype(np.int32)


def time_evaluate(ev, u, f, K, reps):
    for _ in range(5):
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K)
    ev.set_timing(True)
    ts = []
    for _ in range(reps):
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K)
        ts.append(sum(ev.timing()))
    ev.set_timing(False)
    return stats(ts)


def time_apply(ev, u, x, y, reps):
    for _ in range(5):
        ev.tangent_apply(u, x, y)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ev.tangent_apply(u, x, y)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


def workload(name, mesh, path, reps, tag, apply=False):
    dev = torch.device("cuda:0")
    has_table = hasattr(fcg.lib(), "fcg_set_element_materials")
    ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG, youngs=E, poisson=NU, path=path)
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.standard_normal(mesh.n_cols) * 5e-2 / 10).to(dev)
    out = {"tag": tag, "workload": name, "elements": int(mesh.n_ele), "path": int(ev.info.path)}
    if apply:
        x = torch.from_numpy(rng.standard_normal(mesh.n_cols)).to(dev)
        y = torch.zeros(mesh.n_rows, dtype=torch.float64, device=dev)
        run = lambda: time_apply(ev, u, x, y, reps)  # noqa: E731
        outs = (y,)
    else:
        f = torch.zeros(mesh.n_rows, dtype=torch.float64, device=dev)
        K = torch.zeros(mesh.nnz, dtype=torch.float64, device=dev)
        run = lambda: time_evaluate(ev, u, f, K, reps)  # noqa: E731
        outs = (K, f)
    out["uniform"] = run()
    out["uniform"]["sha256"] = digest(*outs)
    if has_table:
        ev.set_element_materials([E, 10.0 * E], [NU, 0.25], layers(mesh))
        out["tabled"] = run()
        out["tabled"]["sha256"] = digest(*outs)
        out["tabled_over_uniform"] = out["tabled"]["median_ms"] / out["uniform"]["median_ms"]
        ev.set_element_materials(None)
        run()
        out["after_reset_sha256"] = digest(*outs)
    ev.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--hex27-n", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", default=os.environ.get("FCG_LIB", "this"))
    a = ap.parse_args()
    box = fcg.BoxMesh(fcg.HEX8, (a.n, a.n, a.n), jitter=0.1, seed=20251015)
    dis = fcg.Discretization.renumbered(box, seed=1)
    del box
    workload(f"hex8-{a.n}^3 renumbered gather totlag K+f", dis, fcg.PATH_GATHER, a.reps, a.tag)
    del dis
    h27 = fcg.BoxMesh(fcg.HEX27, (a.hex27_n,) * 3, jitter=0.02, seed=5)
    workload(f"hex27-{a.hex27_n}^3 general totlag K+f", h27, fcg.PATH_GENERAL, a.reps, a.tag)
    workload(f"hex27-{a.hex27_n}^3 tangent_apply totlag", h27, fcg.PATH_GENERAL, a.reps, a.tag, apply=True)


if __name__ == "__main__":
    main()
