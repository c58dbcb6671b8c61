"""Timings of the explicit-dynamics pieces on one GPU (profiles/explicit/README.md).

Without a measurement name this is the driver: it runs the three measurements below as child
processes, each under its own time limit, stops at the first that fails and leaves one JSON line
per measurement in `--out` (explicit_update.json, explicit_step.json, explicit_stable_dt.json).

  update     fcg_centrdiff_step (all outputs, with the kinetic energy) against the same update
             written as the unfused torch elementwise sequence in the same process, and
             fcg_measure_hbm's copy figure; bytes counted per fused call and row: 5 doubles and the
             mask byte read, 4 doubles written = 73; once on one state set (cache-warm at 1M
             elements) and once rotating over four (every call from and to HBM)
  step       the CALC_INTERNALFORCE evaluate alone, and a whole queued step of
             dynamics.CentralDifference.run (evaluate + update, async, no host synchronisation)
  stable_dt  fcg_stable_dt on an assembled K (host clock: the call drains the stream), beside the
             CALC_NLNSTIFF evaluate that assembles it
hipEvents around `reps` calls after a warm-up unless stated.
usage: explicit_bench.py [update|step|stable_dt] [--n 100] [--reps 20] [--out bench_out]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"update": 300, "step": 300, "stable_dt": 300}  # seconds per child

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="?", choices=list(LIMITS))
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--kinematics", default="totlag")
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"))
a = ap.parse_args()

if a.what is None:
    os.makedirs(a.out, exist_ok=True)
    for what, limit in LIMITS.items():
        cmd = [sys.executable, os.path.abspath(__file__), what, "--n", str(a.n), "--reps", str(a.reps),
               "--kinematics", a.kinematics]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"explicit_bench.py {what}: no result within {limit} s")
        if r.returncode != 0:
            sys.exit(f"explicit_bench.py {what}: exit status {r.returncode}")
        sys.stdout.write(r.stdout)
        with open(os.path.join(a.out, f"explicit_{what}.json"), "w") as fh:
            fh.write(r.stdout)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
fcg = importlib.import_module("4c_amd").fcg
dynamics = importlib.import_module("4c_amd.dynamics")

if not torch.cuda.is_available():
    sys.exit("explicit_bench.py needs a GPU")
dev = torch.device("cuda:0")
kin = fcg.TOTLAG if a.kinematics == "totlag" else fcg.LINEAR
RHO, E, NU = 1e-3, 210.0, 0.3
m = fcg.BoxMesh(fcg.HEX8, (a.n, a.n, a.n), jitter=0.02)
ev = fcg.Evaluator(m, kinematics=kin, youngs=E, poisson=NU)
f64 = dict(dtype=torch.float64, device=dev)
s = torch.cuda.current_stream(dev)
n = m.n_rows
base = {"config": f"hex8-{a.n}^3", "rows": n, "nnz": m.nnz, "path": int(ev.info.path)}
clamped = np.nonzero(np.isclose(m.node_x[:, 0], 0.0))[0]
dbc = np.sort((m.node_dof_row[clamped][:, None] + np.arange(3)).ravel()).astype(np.int32)


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


if a.what == "update":
    _, m_l = ev.mass_nodal(RHO, m_lumped=torch.empty(n, **f64))
    fixed = torch.zeros(n, dtype=torch.uint8, device=dev)
    idx = torch.as_tensor(dbc.astype(np.int64)).to(dev)
    fixed[idx] = 1
    g = torch.Generator(device=dev).manual_seed(1)
    fext, fint = (1e-6 * torch.randn(n, generator=g, **f64) for _ in range(2))
    dt, damp = 1e-5, 10.0
    st = [{k: torch.zeros(n, **f64) for k in ("d", "vhalf", "v", "a")} for _ in range(2)]
    ekin = torch.zeros(1, **f64)

    def fused(x=st[0]):
        ev.centrdiff_step(dt, dt, damp, fext, fint, m_l, fixed, x["d"], x["vhalf"], x["v"], x["a"],
                          ekin, stream=s)

    def fused_no_ekin(x=st[0]):
        ev.centrdiff_step(dt, dt, damp, fext, fint, m_l, fixed, x["d"], x["vhalf"], x["v"], x["a"],
                          None, stream=s)

    tmp = torch.empty(n, **f64)

    def unfused(x=st[1]):
        d, vh, v, acc = x["d"], x["vhalf"], x["v"], x["a"]
        torch.sub(fext, fint, out=acc)
        acc.div_(m_l)
        acc.sub_(vh, alpha=damp)
        acc.index_fill_(0, idx, 0.0)
        torch.add(vh, acc, alpha=0.5 * dt, out=v)
        torch.add(v, acc, alpha=0.5 * dt, out=vh)
        d.add_(vh, alpha=dt)
        torch.mul(m_l, v, out=tmp)
        return 0.5 * torch.dot(tmp, v)

    ms_fused = timed(fused)
    ms_noe = timed(fused_no_ekin)
    ms_torch = timed(unfused)
    # One state set is 73 n bytes -- 226 MB at 1M elements, inside the 256 MiB Infinity Cache, so
    # the figures above are cache-warm.  Rotating over four sets (state, loads and mass each
    # their own: 0.9 GB) makes every call read and write HBM.
    cold = [dict({k: torch.zeros(n, **f64) for k in ("d", "vhalf", "v", "a")},
                 fext=fext.clone(), fint=fint.clone(), m=m_l.clone()) for _ in range(4)]
    turn = [0]

    def fused_cold():
        x = cold[turn[0] % 4]
        turn[0] += 1
        ev.centrdiff_step(dt, dt, damp, x["fext"], x["fint"], x["m"], fixed, x["d"], x["vhalf"],
                          x["v"], x["a"], ekin, stream=s)

    def unfused_cold():
        x = cold[turn[0] % 4]
        turn[0] += 1
        d, vh, v, acc = x["d"], x["vhalf"], x["v"], x["a"]
        torch.sub(x["fext"], x["fint"], out=acc)
        acc.div_(x["m"])
        acc.sub_(vh, alpha=damp)
        acc.index_fill_(0, idx, 0.0)
        torch.add(vh, acc, alpha=0.5 * dt, out=v)
        torch.add(v, acc, alpha=0.5 * dt, out=vh)
        d.add_(vh, alpha=dt)
        torch.mul(x["m"], v, out=tmp)
        return 0.5 * torch.dot(tmp, v)

    ms_fused_cold = timed(fused_cold, warm=4)
    ms_torch_cold = timed(unfused_cold, warm=4)
    # the same number of calls from the same start on both sides: do they agree?
    for x in st:
        for t in x.values():
            t.zero_()
    for _ in range(5):
        fused()
        e_torch = unfused()
    torch.cuda.synchronize()
    dev_d = float((st[0]["d"] - st[1]["d"]).abs().max() / st[1]["d"].abs().max())
    copy_gbs, write_gbs = fcg.measure_hbm(0)
    byt = 73 * n
    print(json.dumps(dict(base, what="update", ms_fused=ms_fused, ms_fused_without_ekin=ms_noe,
                          ms_torch_sequence=ms_torch, bytes_counted=byt, gbs_fused=byt / ms_fused / 1e6,
                          ms_fused_rotating=ms_fused_cold, ms_torch_sequence_rotating=ms_torch_cold,
                          gbs_fused_rotating=byt / ms_fused_cold / 1e6,
                          # seven 2-read 1-write passes and the dot
                          bytes_torch_sequence=8 * n * 23, hbm_copy_gbs=copy_gbs, hbm_write_gbs=write_gbs,
                          d_vs_torch=dev_d, ekin_fused=float(ekin), ekin_torch=float(e_torch))))

if a.what == "step":
    u = torch.from_numpy(m.u_col(1e-3)).to(dev)
    f = torch.zeros(n, **f64)
    ev.set_async(1)  # as the driver queues it: no drain and host round trip between the calls
    ms_eval = timed(lambda: ev.evaluate_device(fcg.CALC_INTERNALFORCE, fcg.OVERWRITE, u, f), reps=a.reps)
    ev.check_error()
    ev.set_async(0)
    fext = np.zeros(n)
    fext[2::3] = -1e-6
    cd = dynamics.CentralDifference(ev, RHO, 1e-5, fext, dbc)
    t0 = time.perf_counter()
    cd.dt = cd.stable_dt(0.8)
    ms_stable = (time.perf_counter() - t0) * 1e3
    cd.initialize()
    cd.run(5)  # warm-up
    reps = max(a.reps, 50)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(s)
    cd.run(reps, check_every=reps)
    e1.record(s)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    print(json.dumps(dict(base, what="step", kinematics=a.kinematics, ms_evaluate_internalforce=ms_eval,
                          ms_whole_step_events=e0.elapsed_time(e1) / reps, ms_whole_step_wall=wall,
                          steps=reps, dt=cd.dt, ms_driver_stable_dt_with_assembly=ms_stable,
                          kinetic_energy=cd.energies()[0], max_abs_d=float(cd.d.abs().max()))))

if a.what == "stable_dt":
    u = torch.from_numpy(m.u_col(1e-3)).to(dev)
    f = torch.zeros(n, **f64)
    K = torch.empty(m.nnz, **f64)
    ms_eval = timed(lambda: ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, u, f, K), reps=5, warm=2)
    _, m_l = ev.mass_nodal(RHO, m_lumped=torch.empty(n, **f64))
    fixed = torch.zeros(n, dtype=torch.uint8, device=dev)
    fixed[torch.as_tensor(dbc.astype(np.int64)).to(dev)] = 1
    ev.stable_dt(K, m_l, fixed)  # warm-up: allocates the partial buffer
    torch.cuda.synchronize()
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        dt_crit, lam = ev.stable_dt(K, m_l, fixed)
    ms = (time.perf_counter() - t0) * 1e3 / reps
    copy_gbs, _ = fcg.measure_hbm(0)
    print(json.dumps(dict(base, what="stable_dt", ms_stable_dt=ms, gb_K=8 * m.nnz / 1e9,
                          gbs_stable_dt=8 * m.nnz / ms / 1e6, ms_evaluate_nlnstiff=ms_eval,
                          hbm_copy_gbs=copy_gbs, dt_crit=dt_crit, lambda_bound=lam)))
