"""hex8 ElastHyper/CoupNeoHooke: the general path against the node-row gather, on one GPU
(profiles/neohooke_gather/README.md).

Without a configuration name this is the driver: it runs the three configurations below as child
processes, alternating them over `--rounds` rounds, each child under its own time limit; it stops
at the first that fails and leaves one JSON line per child in `--out`/neohooke_gather_ab.jsonl.

  general  CoupNeoHooke TotLag on PATH_GENERAL (what PATH_AUTO gives the material)
  gather   CoupNeoHooke TotLag on PATH_GATHER
  stvk     StVK TotLag on PATH_GATHER: what the gather's record traffic alone costs

The mesh is the renumbered box (n^3 hex8, jitter 0.02, no lattice hint) at u_col(2e-2).  Each child
times CALC_NLNSTIFF in OVERWRITE mode and CALC_INTERNALFORCE with hipEvents around `reps` queued
calls after a warm-up, and records fcg_info's device_bytes and scratch_bytes.
usage: neohooke_gather_ab.py [general|gather|stvk] [--n 100] [--reps 20] [--rounds 3] [--out bench_out]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"general": 180, "gather": 180, "stvk": 180}  # seconds per child

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="?", choices=list(LIMITS))
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"))
a = ap.parse_args()

if a.what is None:
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "neohooke_gather_ab.jsonl")
    open(path, "w").close()
    for rnd in range(a.rounds):
        for what, limit in LIMITS.items():
            cmd = [sys.executable, os.path.abspath(__file__), what, "--n", str(a.n), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"neohooke_gather_ab.py {what}: no result within {limit} s")
            if r.returncode != 0:
                sys.exit(f"neohooke_gather_ab.py {what}: exit status {r.returncode}")
            line = json.dumps(dict(json.loads(r.stdout.strip().splitlines()[-1]), round=rnd))
            print(line, flush=True)
            with open(path, "a") as fh:
                fh.write(line + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
fcg = importlib.import_module("4c_amd").fcg

if not torch.cuda.is_available():
    sys.exit("neohooke_gather_ab.py needs a GPU")
dev = torch.device("cuda:0")
E, NU = 10.0, 0.25
material, path = {"general": (fcg.MAT_ELASTHYPER_COUPNEOHOOKE, fcg.PATH_GENERAL),
                  "gather": (fcg.MAT_ELASTHYPER_COUPNEOHOOKE, fcg.PATH_GATHER),
                  "stvk": (fcg.MAT_STVK, fcg.PATH_GATHER)}[a.what]
box = fcg.BoxMesh(fcg.HEX8, (a.n, a.n, a.n), jitter=0.02)
dis = fcg.Discretization.renumbered(box, seed=1)
ub, uh = box.u_col(2e-2), np.zeros(box.n_cols)
for d in range(3):
    uh[3 * dis.node_perm + d] = ub[3 * np.arange(box.n_node) + d]
ev = fcg.Evaluator(dis, kinematics=fcg.TOTLAG, youngs=E, poisson=NU, path=path, material=material)
if ev.info.path != path:
    sys.exit(f"neohooke_gather_ab.py {a.what}: the context took path {ev.info.path}, not {path}")
f64 = dict(dtype=torch.float64, device=dev)
s = torch.cuda.current_stream(dev)
u = torch.from_numpy(uh).to(dev)
f = torch.zeros(dis.n_rows, **f64)
K = torch.empty(dis.nnz, **f64)


def timed(fn, reps=a.reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K)  # synchronous once: raises on an error
ev.set_async(1)  # queued, as a driver would: no drain and host round trip between the calls
ms_k = timed(lambda: ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K))
ms_f = timed(lambda: ev.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f))
ev.check_error()
ev.set_async(0)
print(json.dumps(dict(config=a.what, mesh=f"renumbered hex8-{a.n}^3", material=int(material),
                      path=int(ev.info.path), rows=int(dis.n_rows), nnz=int(dis.nnz), reps=a.reps,
                      ms_nlnstiff_overwrite=ms_k, ms_internalforce=ms_f,
                      device_bytes=int(ev.info.device_bytes), scratch_bytes=int(ev.info.scratch_bytes),
                      norm_f=float(torch.linalg.vector_norm(f)), norm_K=float(torch.linalg.vector_norm(K)))))
