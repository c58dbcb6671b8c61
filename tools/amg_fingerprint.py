#!/usr/bin/env python3
"""SHA-256 fingerprints of what the two native AMGs compute, for comparing two builds bit by bit.

    tools/amg_fingerprint.py [--root CHECKOUT] > fingerprint.txt      (one MI355X, a few seconds)
    tools/amg_fingerprint.py --compare OLD.txt NEW.txt                 (no GPU)

The first form imports 4c_amd from CHECKOUT (default: this repository) and prints one line per
(case, item): the SHA-256 of the raw bytes of
  structural AMG (amg.NativeAMG), the meshes of tests/test_amg_hierarchy.py, with FCG_AMG_REORDER
  1 and 0: every level's fetched A and P (pattern and values), the smoother's block inverses and
  lambda_max; the coarsest inverse; one V-cycle (apply) of a fixed right-hand side; solve's x,
  iteration count and reported residual -- the solve once more with FCG_AMG_GRAPH=1 where the
  coarsest level is dense;
  scalar AMG (amg.ScalarAMG), meshes of tests/test_samg.py (4-, 16- and 64-lane rows): the
  fetched levels, lambda_max, apply, solve.
The second form prints the side-by-side table and exits 1 when a line differs or is missing.
"""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

E, NU, ALPHA, T0, COND, DT = 210.0, 0.3, 1.2e-5, 293.0, 52.0, 0.05

STRUCTURAL = {
    "h8_633": dict(ct="HEX8", iv=(6, 3, 3), jitter=0.1, seed=1, bc="xmin", opts={"coarse_max": 12}),
    "h8_633_totlag": dict(ct="HEX8", iv=(6, 3, 3), jitter=0.1, seed=1, bc="xmin", opts={"coarse_max": 12},
                          totlag=True),
    "h27_322": dict(ct="HEX27", iv=(3, 2, 2), jitter=0.02, seed=2, bc="xmin", opts={"coarse_max": 6}),
    "line_12": dict(ct="HEX8", iv=(12, 2, 2), jitter=0.0, seed=4, bc="lateral", opts={}),
    "h8_1244": dict(ct="HEX8", iv=(12, 4, 4), jitter=0.0, seed=6, bc="xmin", opts={}),
}
SCALAR = {
    "h8_322": dict(ct="HEX8", iv=(3, 2, 2), jitter=0.1, opts={"coarse_max": 8}),
    "h27_333": dict(ct="HEX27", iv=(3, 3, 3), jitter=0.02, opts={"coarse_max": 8}),
    "h8_654": dict(ct="HEX8", iv=(6, 5, 4), jitter=0.1, opts={"coarse_max": 4}),
}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fingerprint(root):
    sys.path.insert(0, root)
    import torch

    fcg = importlib.import_module("4c_amd").fcg
    amg = importlib.import_module("4c_amd.amg")
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zeros = lambda n: torch.zeros(int(n), dtype=torch.float64, device=dev)
    out = []

    def solve_lines(tag, a, K, b):
        x = zeros(len(b))
        it, rel = a.solve(K, t(b), x, 1e-10, 200, setup=False)
        torch.cuda.synchronize()
        out.append((tag, "solve x", sha(x.cpu().numpy())))
        out.append((tag, "solve iterations, residual", sha(np.int64(it), np.float64(rel))))

    def apply_line(tag, a, K, b):
        z = zeros(len(b))
        a.apply(K, t(b), z)
        torch.cuda.synchronize()
        out.append((tag, "apply", sha(z.cpu().numpy())))

    for name, spec in STRUCTURAL.items():
        ct = getattr(fcg, spec["ct"])
        flat = fcg.BoxMesh(ct, spec["iv"])
        mesh = fcg.Discretization.renumbered(fcg.BoxMesh(ct, spec["iv"], jitter=spec["jitter"]), seed=spec["seed"])
        X = flat.node_x
        fix0 = np.zeros((flat.n_node, 3), dtype=bool)
        if spec["bc"] == "xmin":
            fix0[np.isclose(X[:, 0], 0.0)] = True
        else:  # the four lateral faces
            fix0[np.isclose(X[:, 1], 0.0) | np.isclose(X[:, 1], 1.0) | np.isclose(X[:, 2], 0.0) | np.isclose(X[:, 2], 1.0)] = True
        fix = np.zeros_like(fix0)
        fix[mesh.node_perm] = fix0
        ndr = np.asarray(mesh.node_dof_row, dtype=np.int64)
        node, d = np.nonzero(fix & (ndr >= 0)[:, None])
        rows = np.sort(ndr[node] + d).astype(np.int32)
        totlag = spec.get("totlag", False)
        ev = fcg.Evaluator(mesh, kinematics=fcg.TOTLAG if totlag else fcg.LINEAR, youngs=E, poisson=NU)
        u = 1e-3 * np.random.default_rng(17).standard_normal(mesh.n_cols) if totlag else np.zeros(mesh.n_cols)
        K, f = zeros(ev.info.nnz), zeros(mesh.n_rows)
        ev.evaluate_device(fcg.CALC_NLNSTIFF, fcg.OVERWRITE, t(u), f, K)
        ev.dirichlet_apply(t(rows), K)
        b = np.random.default_rng(5).standard_normal(mesh.n_rows)
        b[rows] = 0.0
        for reorder in ("1", "0"):
            tag = f"structural {name} reorder {reorder}"
            os.environ["FCG_AMG_REORDER"] = reorder
            os.environ.pop("FCG_AMG_GRAPH", None)
            a = amg.NativeAMG(mesh, ev, rows, **spec["opts"])
            a.setup(K)
            info, dense = a.describe(), a.stats()["coarse_dense"]
            out.append((tag, "level sizes", sha(np.array([[i["dofs"], i["blocks"]] for i in info], dtype=np.int64))))
            out.append((tag, "order", sha(a.order())))
            for l in range(len(info)):
                out.append((tag, f"A_{l}", sha(*a.level_matrix(l, 0))))
                out.append((tag, f"block inverses {l}", sha(a.level_matrix(l, 3))))
                if l + 1 < len(info):
                    out.append((tag, f"P_{l}", sha(*a.level_matrix(l, 1))))
                    out.append((tag, f"lmax_{l}", sha(np.float64(info[l]["lmax"]))))
            if dense:
                out.append((tag, "coarsest inverse", sha(a.level_matrix(len(info) - 1, 4))))
            apply_line(tag, a, K, b)
            solve_lines(tag, a, K, b)
            if dense and reorder == "1":
                os.environ["FCG_AMG_GRAPH"] = "1"
                solve_lines(tag + " graph", a, K, b)
                out.append((tag + " graph", "graph launches", sha(np.int64(a.stats()["graph_launches"]))))
                os.environ.pop("FCG_AMG_GRAPH")
            a.close()
        os.environ.pop("FCG_AMG_REORDER")

    for name, spec in SCALAR.items():
        tag = f"scalar {name}"
        ct = getattr(fcg, spec["ct"])
        mesh = fcg.BoxMesh(ct, spec["iv"], jitter=spec["jitter"], seed=4)
        tev = fcg.TsiEvaluator(mesh, E, NU, ALPHA, T0, COND)
        face = np.nonzero(np.isclose(fcg.BoxMesh(ct, spec["iv"]).node_x[:, 0], 0.0))[0]
        rows_t = np.sort(np.asarray(mesh.node_dof_row)[face] // 3).astype(np.int32)
        rows_s = np.sort((3 * rows_t[:, None] + np.arange(3)).ravel()).astype(np.int32)
        g = tev.graph
        rng = np.random.default_rng(23)
        v = 1e-1 * rng.standard_normal(mesh.n_cols)
        T = T0 + 50.0 * rng.standard_normal(g.n_cols_t)
        fs, fT = zeros(mesh.n_rows), zeros(g.n_rows_t)
        Kst, Kts, Ktt = zeros(g.nnz_st), zeros(g.nnz_ts), zeros(g.nnz_tt)
        tev.evaluate_device(fcg.TSI_ALL, fcg.OVERWRITE, t(v), t(T), 1.0, 1.0 / DT, fs=fs, Kst=Kst, fT=fT, Ktt=Ktt, Kts=Kts)
        tev.dirichlet_apply(t(rows_s), t(rows_t), Kst, Kts, Ktt)
        b = rng.standard_normal(g.n_rows_t)
        b[rows_t] = 0.0
        a = amg.ScalarAMG(tev, rows_t, **spec["opts"])
        a.setup(Ktt)
        info = a.describe()
        out.append((tag, "level sizes", sha(np.array([[i["rows"], i["nnz"]] for i in info], dtype=np.int64))))
        for l in range(len(info)):
            out.append((tag, f"A_{l}", sha(*a.level_matrix(l, 0))))
            if l + 1 < len(info):
                out.append((tag, f"P_{l}", sha(*a.level_matrix(l, 1))))
                out.append((tag, f"lmax_{l}", sha(np.float64(info[l]["lmax"]))))
        apply_line(tag, a, Ktt, b)
        solve_lines(tag, a, Ktt, b)
        a.close()

    for tag, item, h in out:
        print(f"{tag}\t{item}\t{h}")


def compare(old, new):
    def read(p):
        with open(p) as fh:
            return {tuple(l.rstrip("\n").split("\t")[:2]): l.rstrip("\n").split("\t")[2] for l in fh if l.count("\t") == 2}

    o, n = read(old), read(new)
    keys = list(o) + [k for k in n if k not in o]
    bad = 0
    print(f"{'case':44s}{'item':30s}{'parent sha256':>14s}  {'branch sha256':>14s}  vs parent")
    for k in keys:
        a, b = o.get(k), n.get(k)
        verdict = "identical" if a == b else "DIFFERENT" if a and b else "MISSING"
        bad += verdict != "identical"
        print(f"{k[0]:44s}{k[1]:30s}{(a or '-')[:12]:>14s}  {(b or '-')[:12]:>14s}  {verdict}")
    print(f"{len(keys)} lines, {bad} different")
    return 1 if bad or not keys else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else fingerprint(os.path.abspath(a.root)))
