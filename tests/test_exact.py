"""Exact sign of the logit (counterexample confirmation): fp64 + rigorous bound vs Fraction."""
import numpy as np

from fairify_amd.engine import exact
from fairify_amd.models.mlp import MLP, random_mlp


def _frac_sign(net, x):
    v = exact.exact_logit_fraction(net, x)
    return (v > 0) - (v < 0)


def test_signs_match_fraction_including_exact_zeros():
    rng = np.random.default_rng(0)
    zeros = 0
    for t in range(40):
        net = random_mlp(6, [5] * (1 + t % 4), seed=t, bias_scale=0.0 if t % 2 else 0.3)
        X = rng.integers(-3, 4, size=(50, 6))
        s = exact.exact_signs(net, X)
        ref = np.array([_frac_sign(net, x) for x in X])
        assert np.array_equal(s, ref), t
        zeros += int((ref == 0).sum())
    assert zeros > 0          # zero-bias nets with dead layers give exact-zero logits


def test_dead_layer_decided_without_fraction(monkeypatch):
    """A certainly-dead hidden layer makes the logit exactly 0: decided in fp64 (no Fraction)."""
    W1 = -np.ones((3, 4), np.float32)
    net = MLP([W1, np.ones((4, 1), np.float32)], [np.zeros(4, np.float32), np.zeros(1, np.float32)], name="d")
    monkeypatch.setattr(exact, "exact_logit_fraction", lambda *a: (_ for _ in ()).throw(AssertionError("slow path")))
    assert exact.exact_signs(net, np.array([[1, 2, 3], [0, 0, 1]])).tolist() == [0, 0]
    assert not exact.is_violation(net, np.array([[1, 2, 3]]), np.array([[1, 2, 4]]))[0]


def test_make_confirm_matches_the_inline_formula():
    """exact.make_confirm (the native runtimes' confirmation callback): the booleans of the formula
    the three solvers used to spell out -- pair constraints in the partition's box, then the exact
    violation test on the shared network or, with ``exact_models``, on the partition's own."""
    from types import SimpleNamespace

    rng = np.random.default_rng(5)
    n0, P, N = 3, 4, 200
    net = random_mlp(n0, [4], seed=2, bias_scale=0.3)
    models = [net if p % 2 == 0 else random_mlp(n0, [4], seed=10 + p, bias_scale=0.3) for p in range(P)]
    lo = rng.integers(0, 3, size=(P, n0))
    hi = lo + rng.integers(1, 5, size=(P, n0))
    parts = rng.integers(0, P, size=N)
    X = rng.integers(lo[parts], hi[parts] + 1)
    XP = X.copy()
    XP[:, 1] = rng.integers(lo[parts, 1], hi[parts, 1] + 1)        # PA dim: differs in most rows
    XP[:, 2] += rng.integers(-2, 3, size=N)                        # RA dim: |diff| <= 1 in some rows
    XP[::7, 0] += 1                                                # shared dim broken
    X[::11, 0] = hi[parts[::11], 0] + 1                            # x outside its box
    buf = np.concatenate([X, XP], axis=1).astype(np.float32)
    buf += rng.uniform(-0.2, 0.2, size=buf.shape).astype(np.float32)   # the callback rounds to integers
    for q in (SimpleNamespace(pa_idx=[1], ra_idx=[2], tau=1), SimpleNamespace(pa_idx=[1], ra_idx=[], tau=0)):
        ok = exact.check_pair_constraints(X, XP, lo[parts], hi[parts], q.pa_idx, q.ra_idx, q.tau)
        want = ok & exact.is_violation(net, X, XP)
        assert np.array_equal(exact.make_confirm(net, lo, hi, q)(parts, buf), want)
        want_m = np.array([ok[k] and exact.is_violation(models[parts[k]], X[k:k + 1], XP[k:k + 1])[0]
                           for k in range(N)])
        got_m = exact.make_confirm(net, lo, hi, q, exact_models=models)(parts, buf)
        assert got_m.dtype == bool and np.array_equal(got_m, want_m)
        assert 0 < ok.sum() < N and want.any() and want_m.any() and not np.array_equal(want, want_m)
    assert exact.make_confirm(net, lo, hi, q)(parts[:0], buf[:0]).shape == (0,)
