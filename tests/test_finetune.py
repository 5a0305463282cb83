"""GC/BM fine-tune on synthetic data with early stopping (src/GC/new_model.py:8-58) on the
reference's own synthetic GC CSV (stored under tests/golden/experimentData)."""
import os

import numpy as np
import pandas as pd

from fairify_amd.models.zoo import get_model
from fairify_amd.repair.finetune import SUITE_SPECS, encode_synthetic, finetune_csv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# experimentData/task2/TabFPN/GC2/2000-100/synthetic-german-predicted-gpt2.csv of the reference
REF_CSV = os.path.join(GOLDEN, "experimentData", "synthetic-german-predicted-gpt2.csv")


def test_finetune_early_stopping_restores_best():
    m = get_model("GC-2", weights="zoo")
    r = finetune_csv(m, REF_CSV, "german", epochs=30, seed=0)
    assert r.train_rows > 0 and r.val_rows > 0
    assert r.best_epoch == int(np.argmin(r.val_loss)) + 1          # restore_best_weights
    stopped = r.epochs_run < 30
    if stopped:                                                     # patience 3 after the best epoch
        assert r.epochs_run == r.best_epoch + 3
    assert r.model.n_in == m.n_in and r.model.widths == m.widths
    assert 0.0 <= r.val_acc <= 1.0


def test_encode_synthetic_fresh_label_encoders():
    df = pd.DataFrame({"status": ["A11", "A14", "A11"], "month": [6, 12, 24], "credit": [1, 0, 1]})
    X, y = encode_synthetic(df, "credit", SUITE_SPECS["german"]["categorical"])
    assert X[:, 0].tolist() == [0, 1, 0] and X[:, 1].tolist() == [6, 12, 24] and y.tolist() == [1, 0, 1]


# experimentData/task5/AC/counterexamples-AC-3.csv of the reference, gzipped
REF_CE = os.path.join(GOLDEN, "experimentData", "counterexamples-AC-3.csv.gz")


def test_reencode_decoded_counterexamples_ac3(adult_data):
    """src/AC/detect_bias.py:140-167 on the fork's own decoded AC-3 counterexamples: rows come
    back in the model's feature order, consecutive rows differ only in sex, labels kept."""
    from fairify_amd.repair.retrain import load_pairs

    X, y = load_pairs(REF_CE, 13, 8, suite="adult")
    assert X.shape[1] == 13 and len(X) % 2 == 0 and len(X) > 1000
    assert y is not None and set(np.unique(y)) <= {0, 1}
    other = [i for i in range(13) if i != 8]
    same = (X[0::2][:, other] == X[1::2][:, other]).all(axis=1)
    assert same.mean() > 0.99
    assert set(np.unique(X[:, 8])) <= {0.0, 1.0}
    m = get_model("AC-3", weights="zoo")
    assert np.isfinite(m.logits(X[:10])).all()


def test_gc_reverse_map_codes():
    from fairify_amd.report.counterexamples import gc_reverse_map

    df = pd.DataFrame({"sex": [1, 0], "status": ["<200", "None"], "savings": ["500+", "x"],
                       "credit_history": ["Delay", "Other"], "employment": ["Unemployed", "4+ years"]})
    out = gc_reverse_map(df)
    assert out["sex"].tolist() == ["A91", "A92"]
    assert out["status"].tolist() == ["A11", "A14"]
    assert out["savings"].tolist() == ["A63", "x"]
    assert out["credit_history"].tolist() == ["A33", "A34"]
    assert out["employment"].tolist() == ["A71", "A74"]
