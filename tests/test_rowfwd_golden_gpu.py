"""The six rigorous row-forward kernels (``fa_rate_kernel``, ``fa_count_enum_kernel``,
``fa_gap_enum_kernel``, ``fa_audit_kernel``, ``fa_neighbour_kernel``, ``fa_causal_kernel``) against
outputs recorded from the kernels before they shared ``csrc/rowfwd.h`` (``tools/record_rowfwd_golden.py``,
``tests/golden/rowfwd_parent.npz``, recorded on an MI355X from commit 18b92e5 "Certify the largest score
gap between counterparts per partition"): bitwise.  One net per tile bucket (1, 2, 4, 7, 10 tiles), a
three-layer net and the zero-bias net; PA-only and relaxed queries everywhere, two PA dims and a
three-valued PA on the narrow nets; 17 and 65 rows, 70 samples, leaves of 15, 17 and 65 points, two
launch shapes per kernel and a neighbour table spanning two words.  Inputs come from the recorder's
builders, so the recorder's case list is the test's.
"""
import importlib.util
import os

import numpy as np
import pytest

from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "record_rowfwd_golden", os.path.join(os.path.dirname(HERE), "tools", "record_rowfwd_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", rec.FILE))


def test_every_recorded_array_has_a_case(golden):
    assert len(set(golden.files)) > 0
    assert {k.rsplit("/", 1)[0] for k in golden.files} == {key for _, _, key, _ in rec.cases()}


@pytest.mark.parametrize("net", list(rec.NETS))
@pytest.mark.parametrize("kernel", rec.KERNELS)
def test_rowfwd_kernels_match_recorded_outputs(cuda, golden, kernel, net):
    be = Backend(rec.model(net), cuda)
    assert be.hip
    n = 0
    for k, m, key, run in rec.cases():
        if k != kernel or m != net:
            continue
        out = run(be, cuda)
        for name, arr in out.items():
            want = golden[f"{key}/{name}"]
            assert arr.dtype == want.dtype and arr.shape == want.shape, (key, name)
            assert arr.tobytes() == want.tobytes(), (key, name)
        n += 1
    assert n >= 3
