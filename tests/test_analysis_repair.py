"""Group metrics, causal detector, hybrid routing, counterexample export, repair (CPU)."""
import os

import numpy as np
import pytest

from fairify_amd import presets
from fairify_amd.analysis.causal import CausalDiscriminationDetector
from fairify_amd.analysis.hybrid import V_SAT, V_UNSAT, VerdictTable, hybrid_predict
from fairify_amd.analysis.metrics import consistency, group_metrics, theil_index
from fairify_amd.engine.pipeline import VerifyConfig
from fairify_amd.engine.runner import run_preset
from fairify_amd.models.mlp import random_mlp


def test_group_metrics_hand_computed():
    y = np.array([1, 1, 0, 0, 1, 0, 1, 0])
    p = np.array([1, 0, 0, 1, 1, 1, 1, 0])
    a = np.array([1, 1, 1, 1, 0, 0, 0, 0])      # privileged = 1
    m = group_metrics(y, p, a)
    # priv: pos rate 2/4, unpriv: 3/4 ; TPR priv 1/2, unpriv 2/2 ; FPR priv 1/2, unpriv 1/2
    assert m["SPD"] == pytest.approx(0.25)
    assert m["DI"] == pytest.approx(1.5)
    assert m["EOD"] == pytest.approx(0.5)
    assert m["AOD"] == pytest.approx(0.25)


def test_consistency_matches_bruteforce():
    rng = np.random.default_rng(0)
    X = rng.integers(0, 10, (200, 4)).astype(float) + rng.random((200, 4)) * 1e-3
    yp = rng.integers(0, 2, 200)
    d = ((X[:, None] - X[None]) ** 2).sum(-1)
    nn = np.argsort(d, axis=1)[:, :5]
    ref = 1 - np.mean(np.abs(yp - yp[nn].mean(1)))
    assert consistency(X, yp, chunk=37) == pytest.approx(ref)
    assert theil_index(np.array([1, 0, 1]), np.array([1, 0, 1])) == pytest.approx(0.0)


def test_causal_detector_extremes():
    names = ["a", "s", "b"]
    X = np.array([[0, 0, 0], [1, 1, 1], [2, 0, 2]], dtype=float)
    fair = CausalDiscriminationDetector.from_data(lambda Z: (Z[:, 0] > 0).astype(int), X, names, max_samples=300)
    assert fair.causal_discrimination(["s"])[1] == 0.0
    unfair = CausalDiscriminationDetector.from_data(lambda Z: Z[:, 1].astype(int), X, names, max_samples=300)
    assert unfair.causal_discrimination(["s"])[1] == 1.0


def test_verdict_table_and_hybrid():
    pre = presets.get("src/GC-age")
    g = pre.grid()
    t = VerdictTable(g)
    t.set(np.array([0, 1]), ["sat", "unsat"])
    lo, hi = g.decode(np.array([0, 1, 2]))
    v = t.lookup(lo)
    assert v.tolist() == [V_SAT, V_UNSAT, -1]
    yh = hybrid_predict(lo, t, lambda X: np.zeros(len(X), int), lambda X: np.ones(len(X), int))
    assert yh.tolist() == [1, 0, 0]


def test_export_and_repair_roundtrip(tmp_path):
    from fairify_amd.report.counterexamples import export_counterexamples
    from fairify_amd.repair.retrain import activation_deltas, masked_finetune, map_neurons, relabel_pairs

    out = str(tmp_path)
    run_preset(presets.get("src/GC-age"), models=["GC-1"], out_dir=out, accuracy=False, verbose=False,
               cfg=VerifyConfig(sim_size=200, node_budget=256, smt_backend="none"), max_partitions=12, weights="zoo")
    path = export_counterexamples("src/GC-age", "GC-1", out, weights="zoo")
    z = np.load(os.path.splitext(path)[0] + ".npz")
    assert z["x"].shape == z["xp"].shape and len(z["x"]) > 0
    from fairify_amd.models.zoo import get_model

    m = get_model("GC-1", weights="zoo")
    X = np.stack([z["x"], z["xp"]], 1).reshape(-1, 20)
    sc = activation_deltas(m, X, pa_index=11)
    assert sc.shape == (m.n_neurons,) and sc.max() > 0
    neurons = map_neurons(m, np.argsort(-sc)[:3])
    y = relabel_pairs(X, m.predict(X))
    rep = masked_finetune(m, X, y, neurons, epochs=2)
    # only the selected neurons' incoming weights changed
    changed = [np.nonzero(np.any(a != b, axis=0))[0].tolist() for a, b in zip(m.weights, rep.weights)]
    for l, cols in enumerate(changed):
        assert set(cols) <= {j for (ll, j) in neurons if ll == l}


def test_analyze_writes_hybrid_and_case_csvs(tmp_path):
    """analyze with a fairer model + a verification results dir writes the fork's
    hybrid_approach_results.csv and debug_case_breakdown.csv (src/AC/Verify-AC-experiment-new.py:760-816)."""
    import csv

    from fairify_amd.analysis.report import analyze_model

    out = str(tmp_path)
    run_preset(presets.get("src/GC-age"), models=["GC-1"], out_dir=out, accuracy=False, verbose=False,
               cfg=VerifyConfig(sim_size=200, node_budget=256, smt_backend="none"), max_partitions=40, weights="zoo")
    res = analyze_model("src/GC-age", "GC-1", fairer="GC-2", results=out, out_dir=out, causal_samples=50)
    rows = list(csv.reader(open(os.path.join(out, "hybrid_approach_results.csv"))))
    assert rows[0] == ["Approach", "Accuracy", "DI", "SPD", "EOD", "AOD", "ERD", "CNT", "TI"]
    assert [r[0] for r in rows[1:]] == ["Hybrid", "GC-1 Original", "GC-2 Fairer"]
    assert abs(float(rows[1][1]) - res["hybrid"]["accuracy"]) < 1e-12
    dbg = list(csv.reader(open(os.path.join(out, "debug_case_breakdown.csv"))))
    assert dbg[0] == ["Case", "Description", "Model Used", "Count", "Percentage"]
    counts = {r[0]: int(r[3]) for r in dbg[1:5]}
    assert sum(counts.values()) == res["n_test"]
    assert counts["Case 3"] == res["cases"]["sat_fairer"]


def test_ac3_group_metrics_pinned_to_reference_log(adult_data):
    """AC-3 on the Adult test split vs the fork's logged AIF360 values (AC-3.ipynb:752-762 at 3 dp,
    and the 4-dp "Original CNT: 0.8890" of :2086, reproduced by AIF360's ball-tree kNN)."""
    from fairify_amd.analysis.metrics import all_metrics, consistency
    from fairify_amd.data import tabular
    from fairify_amd.models.zoo import get_model

    ds = tabular.load("adult", allow_synthetic=False)
    m = get_model("AC-3", weights="zoo")
    yp = m.predict(ds.X_test)
    r = all_metrics(ds.X_test, ds.y_test, yp, 8)
    want = {"accuracy": 0.845, "f1": 0.660, "DI": 0.486, "SPD": -0.131, "EOD": 0.040, "AOD": -0.002, "ERD": -0.099,
            "CNT": 0.889, "TI": 0.121}
    for k, v in want.items():
        assert round(r[k], 3) == v, (k, r[k])
    assert round(r["CNT"], 4) == 0.8890
    assert round(consistency(ds.X_test, yp, method="gemm"), 4) == 0.8886    # index tie-breaking


def test_experiment_metrics_csv(tmp_path):
    """experiment/* presets write synthetic-<ds>-predicted-<family>-metrics.csv with one row per
    partition (src/AC/Verify-AC-experiment-new.py:482-542); Pruned F1 from the agreement counts."""
    import csv

    out = str(tmp_path)
    run_preset(presets.get("experiment/GC-1"), out_dir=out, accuracy=False, verbose=False,
               cfg=VerifyConfig(sim_size=200, node_budget=256, smt_backend="none"), max_partitions=16, weights="zoo")
    rows = list(csv.reader(open(os.path.join(out, "synthetic-german-predicted-GC-metrics.csv"))))
    assert rows[0] == ["Partition ID", "Original Accuracy", "Original F1 Score", "Pruned Accuracy", "Pruned F1",
                       "DI", "SPD", "EOD", "AOD", "ERD", "CNT", "TI"]
    assert len(rows) == 17 and [int(r[0]) for r in rows[1:]] == list(range(1, 17))
    for r in rows[1:]:
        acc, f1 = float(r[3]), float(r[4])
        assert 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
        assert r[1] == rows[1][1] and r[5:] == rows[1][5:]          # model-level columns


def test_decode_undecodable_codes_follow_reference():
    """A code outside the LabelEncoder's classes: Adult / German keep the row with the string
    f"{col}_{value}" (src/GC/Verify-GC-experiment-new2.py:355-356, src/AC/...-new2.py:373-374),
    Bank drops the pair (src/BM/...-new2.py:360-368); KBins bins decode to int((a + b) / 2) and
    past the last bin to the last edge (src/AC/...-new2.py:360-370)."""
    from types import SimpleNamespace

    from fairify_amd.report.counterexamples import _decode_column

    le = SimpleNamespace(classes_=np.array(["A", "B", "C"], dtype=object))
    out = _decode_column(np.array([0.0, 2.0, 3.0, -1.0]), le, "purpose")
    assert out.tolist() == ["A", "C", "purpose_3", "purpose_-1"]
    out = _decode_column(np.array([1.0, 7.0]), le, "job", keep_undecodable=False)
    assert out.tolist() == ["B", None]
    kb = SimpleNamespace(bin_edges_=[np.array([0.0, 5.0, 15.0])])
    assert _decode_column(np.array([0.0, 1.0, 2.0]), kb, "capital-gain").tolist() == [2, 10, 15]
