"""Parity pins against the reference's published results (Appendix-Result.pdf Table V) and logs.

GC-3 / GC-4 decided all 201 partitions in the paper, so their exact SAT/UNSAT splits are a
model-level oracle: (age) GC3 195 SAT / 6 UNSAT, GC4 2 SAT / 199 UNSAT; identical for sex.
AC-3's test accuracy 0.8452 is printed in experimentData/task5/results/AC/AC-3.ipynb:2082-2084.
"""
import pytest

from fairify_amd import presets
from fairify_amd.engine.pipeline import VerifyConfig
from fairify_amd.engine.runner import model_accuracy, run_preset
from fairify_amd.models.zoo import get_model


@pytest.mark.parametrize("preset", ["src/GC-age", "src/GC-sex"])
@pytest.mark.parametrize("model,sat,unsat", [("GC-3", 195, 6), ("GC-4", 2, 199)])
def test_table_v_gc_exact_counts(tmp_path, preset, model, sat, unsat):
    rows = run_preset(presets.get(preset), models=[model], out_dir=str(tmp_path), accuracy=False, verbose=False,
                      cfg=VerifyConfig(sim_size=1000, node_budget=100000, heuristic=False, smt_backend="none"))
    r = rows[0]
    assert (r["SAT"], r["UNSAT"], r["UNK"]) == (sat, unsat, 0)


def test_ac3_test_accuracy_matches_reference_log(adult_data):
    acc = model_accuracy(get_model("AC-3"), "adult")
    assert abs(acc - 0.8452) < 5e-5
