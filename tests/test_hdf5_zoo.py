"""Own HDF5 reader vs shipped weights; zoo architectures."""
import glob
import json
import os

import numpy as np

from fairify_amd.models.zoo import SUITE_MODELS, ZOO, get_model, has_weights

# the reference's models/*/*.h5 (Keras weights) and the sums h5py computes from them
REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")


def test_zoo_shapes():
    assert len(ZOO) >= 53
    for name, (suite, n_in, hidden) in ZOO.items():
        m = get_model(name, weights="random")
        assert m.n_in == n_in and tuple(m.hidden) == hidden
        if has_weights(name):
            z = get_model(name)
            assert z.n_in == n_in and tuple(z.hidden) == hidden


def test_reader_matches_assets():
    from fairify_amd.models.keras_io import load_keras_h5

    paths = sorted(glob.glob(os.path.join(REF, "*", "*.h5")))
    assert len(paths) == 53
    for path in paths:
        name = os.path.basename(path)[:-3]
        a = load_keras_h5(path)
        b = get_model(name)
        for wa, wb in zip(a.weights + a.biases, b.weights + b.biases):
            assert np.array_equal(wa, wb)


def test_reader_matches_h5py_oracle():
    """Sum of |weights| per file against what h5py reads (float64 sums recorded with ``repr`` in
    golden/models/h5py_abs_weight_sums.json: h5py is not importable from the framework's Python)."""
    from fairify_amd.models.keras_io import load_keras_h5

    with open(os.path.join(REF, "h5py_abs_weight_sums.json")) as f:
        want = json.load(f)
    paths = sorted(glob.glob(os.path.join(REF, "*", "*.h5")))
    assert sorted(want) == sorted(os.path.basename(p)[:-3] for p in paths)
    for path in paths:
        m = load_keras_h5(path)
        s = sum(float(np.abs(x).astype(np.float64).sum()) for x in m.weights + m.biases)
        assert abs(s - float(want[os.path.basename(path)[:-3]])) <= 1e-9 * max(1.0, s)


def test_npz_roundtrip(tmp_path):
    m = get_model("BM-4", weights="random", seed=3)
    p = tmp_path / "m.npz"
    m.save_npz(str(p))
    from fairify_amd.models.mlp import MLP

    m2 = MLP.load_npz(str(p))
    assert all(np.array_equal(a, b) for a, b in zip(m.weights, m2.weights))


def test_prune_equals_masked_forward():
    m = get_model("AC-4", weights="random", seed=1)
    rng = np.random.default_rng(0)
    dead = [rng.random(w) < 0.3 for w in m.widths[:-1]] + [np.zeros(1, bool)]
    x = rng.integers(0, 20, size=(64, 13))
    assert np.allclose(m.prune(dead).logits(x), m.masked(dead).logits(x), atol=1e-9)
