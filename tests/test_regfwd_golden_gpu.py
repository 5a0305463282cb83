"""``fa_point_kernel``, the fused falsifier and ``fa_agree_kernel`` against outputs recorded from an
earlier build (``tools/record_regfwd_golden.py``, ``tests/golden/regfwd_*.npz``; the commit is named
in ``profiles/r9/regfwd/README.md``): bitwise.  Five network shapes (one per tile count, non-zero
biases of both signs), 1 / 15 / 16 / 17 / 701 points (samples per partition for the falsifier and the
agreement kernel), with and without a dead mask where the kernel takes one.  Inputs come from the
recorder's seeds, so the recorder's case list is the test's.
"""
import importlib.util
import os

import numpy as np
import pytest

from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location(
    "record_regfwd_golden", os.path.join(os.path.dirname(HERE), "tools", "record_regfwd_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    return {kind: np.load(os.path.join(GOLDEN, f)) for kind, f in rec.FILES.items()}


@pytest.mark.parametrize("hidden", rec.SHAPES, ids=rec.shape_key)
@pytest.mark.parametrize("kind", list(rec.FILES))
def test_regfwd_kernels_match_recorded_outputs(cuda, golden, kind, hidden):
    be = Backend(rec.model(hidden), cuda)
    assert be.hip
    n = 0
    for k, h, key, run in rec.cases():
        if k != kind or h != hidden:
            continue
        out = run(be, cuda)
        for name, arr in out.items():
            want = golden[kind][f"{key}/{name}"]
            assert arr.dtype == want.dtype and arr.shape == want.shape, (key, name)
            assert arr.tobytes() == want.tobytes(), (key, name)
        n += 1
    assert n == len(rec.POINTS) * (1 if kind == "falsify" else 2)
