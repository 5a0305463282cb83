"""Discrimination-rate measurement, CPU tier: the reference classification is sound
(certain => exact => possible), the resolved count is the brute-force exact count on every path,
and the stratified estimator / soundness monitor / CLI behave as documented."""
import csv
import itertools
import json
import math

import numpy as np
import pytest
import torch

from fairify_amd.analysis import rate as AR
from fairify_amd.analysis.hybrid import VerdictTable
from fairify_amd.engine import exact
from fairify_amd.engine.rate import exact_flags, measure_partitions
from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import rate as R
from fairify_amd.ops import reference as ref
from fairify_amd.ops.backend import Backend
from fairify_amd.partition import Grid, processing_order

import rate_cases as C


def _pa_tensors(q, lo, hi):
    values = q.pa_values(lo[0].numpy().astype(np.int64), hi[0].numpy().astype(np.int64))
    return torch.from_numpy(values), torch.from_numpy(q.pa_pairs(values))


@pytest.mark.parametrize("name", list(C.EXPECTED))
def test_reference_is_sound_and_resolution_exact(name):
    q = C.query()
    lo, hi, pids = C.boxes()
    values, pairs = _pa_tensors(q, lo, hi)
    total = amb_total = 0
    for k in range(6):
        m = C.family_net(name, k)
        be = Backend(m, "cpu")
        X = ref.sample_points(lo, hi, pids, C.S, C.SEED)
        cert, poss = R.rate_flags_ref(be, q, X.reshape(-1, 5), values, pairs)
        cert, poss = cert.view(C.P, C.S).numpy(), poss.view(C.P, C.S).numpy()
        ex = C.brute_flags(m, q, lo, hi, pids, C.S, C.SEED)
        assert not (cert & ~ex).any(), "a certain profile does not flip exactly"
        assert not (ex & ~poss).any(), "an exact flip is not even possible"
        flips, amb, mask = R.rate_counts_ref(be, q, lo, hi, pids, C.S, C.SEED, values, pairs)
        assert np.array_equal(flips.numpy(), cert.sum(1)) and np.array_equal(mask.numpy(), poss & ~cert)
        assert np.array_equal(amb.numpy(), mask.numpy().sum(1))
        r = measure_partitions(be, q, lo, hi, pids, C.S, C.SEED)
        assert np.array_equal(r.flips_exact, ex.sum(1))
        assert not r.ambiguous_left.any()
        assert np.array_equal(r.flips_exact, C.cpu_counts(name, k))
        total += int(ex.sum())
        amb_total += int(amb.sum())
    print(f"{name}: exact flips {total}, ambiguous {amb_total} of {6 * C.P * C.S}")
    assert (total, amb_total) == C.EXPECTED[name]
    if name in C.BIAS_FAMILIES:
        assert amb_total <= 0.001 * 6 * C.P * C.S     # not "sound" by calling everything ambiguous
    else:
        assert amb_total > 0                          # the zero-bias family exercises the resolution


def test_all_ambiguous_fixture():
    q = C.query()
    lo, hi, pids = C.ambiguous_boxes()
    be = Backend(C.ambiguous_net(), "cpu")
    S = 40
    assert C.brute_flags(be.mlp, q, lo, hi, pids, S, 3).all()
    r = measure_partitions(be, q, lo, hi, pids, S, 3, resolve=False)
    assert (r.flips == 0).all() and (r.ambiguous_left == S).all() and r.flips_exact is None
    r = measure_partitions(be, q, lo, hi, pids, S, 3)
    assert (r.flips == 0).all() and (r.flips_exact == S).all() and not r.ambiguous_left.any()


@pytest.mark.parametrize("pa,ra,tau", [(("f2",), ("f1",), 1), (("f2", "f4"), (), 0)], ids=["relaxed", "two-pa"])
@pytest.mark.parametrize("net", [("17x9x4", 2), ("5x5", 5)], ids=["bias", "zero-bias"])
def test_relaxed_and_two_pa_match_brute_force(pa, ra, tau, net):
    q = C.query(pa, ra, tau)
    lo, hi, pids = C.boxes()
    if ra:
        # unclipped counterparts: some box touches the f1 edge, so x'_1 = -1 or 8 occurs
        assert bool((lo[:, 1] == 0).any()) or bool((hi[:, 1] == 7).any())
        assert R.offset_vectors(q).tolist() == [[-1], [0], [1]]
    m = C.family_net(*net)
    r = measure_partitions(Backend(m, "cpu"), q, lo, hi, pids, 100, C.SEED)
    ex = C.brute_flags(m, q, lo, hi, pids, 100, C.SEED)
    assert np.array_equal(r.flips_exact, ex.sum(1))
    assert ex.any()


def test_multi_valued_pa_matches_brute_force():
    q = C.query(("f3",))
    lo, hi, pids = C.boxes()
    lo[:, 3], hi[:, 3] = 0, 2
    values, pairs = _pa_tensors(q, lo, hi)
    assert values.shape[0] == 3 and pairs.shape[0] == 6
    for net in (("17x9x4", 2), ("5x5", 5)):
        m = C.family_net(*net)
        r = measure_partitions(Backend(m, "cpu"), q, lo, hi, pids, 100, C.SEED)
        ex = C.brute_flags(m, q, lo, hi, pids, 100, C.SEED)
        assert np.array_equal(r.flips_exact, ex.sum(1))
        assert ex.any()


def test_offset_limit_raises():
    q = C.query(("f2",), ("f0", "f1"), 3)            # 7^2 = 49 offset vectors
    lo, hi, pids = C.boxes()
    with pytest.raises(ValueError, match="launch-shape limit"):
        measure_partitions(Backend(C.family_net("8x6", 0), "cpu"), q, lo, hi, pids, 10, 0)


def test_chunking_independence():
    q = C.query()
    lo, hi, pids = C.boxes()
    be = Backend(C.family_net("5x5", 5), "cpu")
    full = measure_partitions(be, q, lo, hi, pids, C.S, C.SEED).flips_exact
    a = measure_partitions(be, q, lo[:12], hi[:12], pids[:12], C.S, C.SEED).flips_exact
    b = measure_partitions(be, q, lo[12:], hi[12:], pids[12:], C.S, C.SEED).flips_exact
    assert np.array_equal(np.concatenate([a, b]), full)
    rev = measure_partitions(be, q, lo.flip(0), hi.flip(0), pids.flip(0), C.S, C.SEED).flips_exact
    assert np.array_equal(rev[::-1], full)
    assert full.sum() > 0


def test_estimator_against_full_lattice():
    """p_hat at S = 4 000 against the rate over the whole profile lattice of one toy box
    (net [8, 6] seed 109, stream seed 0, partition id 5: p = 216 / 2352 = 0.0918, p_hat = 0.095)."""
    q = C.query()
    m = random_mlp(5, [8, 6], seed=109, bias_scale=0.5)
    pts = np.array(list(itertools.product(range(7), range(8), [0], range(6), range(7))))
    values = np.array([[0], [1]])
    p = float(exact_flags(m, q, pts, values, q.pa_pairs(values)).mean())
    assert 0.05 < p < 0.95
    S = 4000
    lo, hi, _ = C.ambiguous_boxes(1)
    r = measure_partitions(Backend(m, "cpu"), q, lo, hi, torch.tensor([5]), S, 0)
    p_hat = r.flips_exact[0] / S
    print(f"p = {p:.6f}, p_hat = {p_hat:.6f}")
    assert abs(p_hat - p) <= 4 * math.sqrt(p * (1 - p) / S)


def _toy_grid():
    grid = Grid.reference(C.DOM, 3)
    return grid, processing_order(grid, seed=0)


def test_stratified_summary_closed_form():
    q = C.query()
    grid, order = _toy_grid()
    order = order[:3]
    m = C.family_net("17x9x4", 2)
    be = Backend(m, "cpu")
    table = VerdictTable(grid)
    table.set(order, ["unsat", "sat", "unknown"])
    S = 200
    out, verdict, samples, flips = AR.measure_grid(grid, q, be, order, table, n_samples=S, seed=0)
    lo, hi = grid.decode(order)
    w = [int(np.prod([hi[k, d] - lo[k, d] + 1 for d in range(5) if d != 2])) for k in range(3)]
    assert samples.tolist() == [0, S, S] and flips[0] == 0
    ex = C.brute_flags(m, q, torch.from_numpy(lo).float(), torch.from_numpy(hi).float(), torch.from_numpy(order), S, 0)
    assert flips[1:].tolist() == ex.sum(1)[1:].tolist()
    p = [0.0, flips[1] / S, flips[2] / S]
    W = sum(w)
    assert out["certified_upper"] == (w[1] + w[2]) / W
    assert out["rate"] == pytest.approx((w[1] * p[1] + w[2] * p[2]) / W, rel=1e-14, abs=0)
    assert out["stderr"] == pytest.approx(math.sqrt(sum(w[k] ** 2 * p[k] * (1 - p[k]) / S for k in (1, 2))) / W,
                                          rel=1e-14, abs=0)
    assert out["verdicts"] == {"sat": 1, "unsat": 1, "unknown": 1, "not_attempted": 0}
    assert out["ambiguous_left"] == 0
    no_table, *_ = AR.measure_grid(grid, q, be, order, None, n_samples=S, seed=0)
    assert no_table["certified_upper"] == 1.0


def test_check_unsat_raises_with_confirmed_pair():
    q = C.query()
    grid, order = _toy_grid()
    order = order[:12]
    m = C.family_net("17x9x4", 2)
    be = Backend(m, "cpu")
    lo, hi = grid.decode(order)
    ex = C.brute_flags(m, q, torch.from_numpy(lo).float(), torch.from_numpy(hi).float(), torch.from_numpy(order),
                       100, 0)
    wrong = np.nonzero(ex.any(1))[0]
    assert wrong.size, "the fixture needs a partition with a sampled flip"
    table = VerdictTable(grid)
    table.set(order, ["unknown"] * len(order))
    table.set(order[wrong[:1]], ["unsat"])             # marked fair although a sampled profile flips
    # without the monitor the partition is trusted: rate 0, not sampled
    out, _, samples, _ = AR.measure_grid(grid, q, be, order, table, n_samples=100, seed=0)
    assert samples[wrong[0]] == 0
    with pytest.raises(AR.SoundnessError) as ei:
        AR.measure_grid(grid, q, be, order, table, n_samples=100, seed=0, check_unsat=True)
    err = ei.value
    assert err.grid_id == int(order[wrong[0]])
    blo, bhi = grid.decode(np.array([err.grid_id]))
    assert exact.is_violation(m, err.x[None], err.xp[None])[0]
    assert exact.check_pair_constraints(err.x[None], err.xp[None], blo, bhi, q.pa_idx, q.ra_idx, q.tau)[0]


def test_cli_round_trip(tmp_path, capsys):
    from fairify_amd import cli, presets

    outs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        cli.main(["measure", "--preset", "src/GC-age", "--model", "GC-1", "--max-partitions", "16", "--samples", "200",
                  "--device", "cpu", "--out", str(out)])
        printed = json.loads(capsys.readouterr().out)
        with open(out / "rate.json") as f:
            assert json.load(f) == printed
        outs.append(((out / "rate.csv").read_bytes(), (out / "rate.json").read_bytes()))
    assert outs[0] == outs[1]
    with open(tmp_path / "run0" / "rate.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == AR.CSV_HEADER
    order = processing_order(presets.get("src/GC-age").grid(), seed=0)[:16]
    assert [int(r["Partition_ID"]) for r in rows] == list(range(1, 17))
    assert [int(r["grid_id"]) for r in rows] == order.tolist()
    assert all(int(r["samples"]) == 200 and float(r["rate"]) == int(r["flips"]) / 200 for r in rows)
    assert printed["certified_upper"] == 1.0 and printed["partitions"] == 16 and printed["ambiguous_left"] == 0
