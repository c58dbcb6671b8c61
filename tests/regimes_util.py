"""The judgement shared by the regime tests (test_evaluate_regimes.py, test_tsi_regimes.py): a
device result against an extended-precision reference, measured beside the float64 oracle's error
on the same inputs.  The criterion and the reason for its factor are in the docstring of
test_evaluate_regimes.py.  TEST INFRASTRUCTURE ONLY."""

import json

import numpy as np

import element_ref as er


def _measures(q, r, S):
    return er.err_norm(q, r), er.err_comp(q, r, S)


def _entry(r, S, o):
    return dict(r=r, S=S, eo=_measures(o, r, S))


def _ratio(e, floor):
    return e / floor if floor > 0 else (0.0 if e == 0 else float("inf"))


def judge(case, prob, anchor, got, MARGINS):
    """prob / anchor: label -> dict(r, S, eo) of this case and of regime A on the same mesh;
    got: label -> device array; MARGINS: case id -> margin in place of 4.  Prints the figures,
    then asserts the criterion on every label."""
    margin = MARGINS.get(case, 4.0)
    assert margin <= 64.0
    rec, worst = dict(case=case, margin=margin, q={}), 0.0
    for label, p in prob.items():
        g = np.asarray(got[label], dtype=np.float64)
        assert g.shape == np.asarray(p["r"]).shape, label
        eg = _measures(g, p["r"], p["S"])
        floor = [max(p["eo"][k], anchor[label]["eo"][k]) for k in (0, 1)]
        ratio = [_ratio(eg[k], floor[k]) for k in (0, 1)]
        rec["q"][label] = dict(finite=bool(np.isfinite(g).all()), eo=p["eo"], eA=anchor[label]["eo"],
                               eg=eg, ratio=ratio)
        worst = max([worst] + [r if np.isfinite(r) else float("inf") for r in ratio])
    rec["ratio"] = worst
    print("REGIMES " + json.dumps(rec))
    for label, q in rec["q"].items():
        assert q["finite"], (case, label)
        # a measure that is not a finite number -- the oracle's, the floor's or the device's --
        # judges nothing: it fails the case
        assert np.isfinite(q["eo"]).all() and np.isfinite(q["eA"]).all(), (case, label, q)
        for r in q["ratio"]:
            assert np.isfinite(r) and not (r > margin), (case, label, q)
