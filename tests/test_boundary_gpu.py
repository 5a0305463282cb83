"""The Python/C++ boundary (csrc/kwargs.h, the fillers of csrc/bindings.cpp, the preparers of
ops/hip.py): a binding that fills an args.h struct refuses a misspelt, missing or bad keyword in host
code while it reads its arguments -- none of the refusals below reaches a launch --, an optional
pointer left out is a null pointer, and every converted wrapper computes bit for bit what the
positional bindings of the parent commit computed (tests/golden/boundary_parent.npz, recorded with
tools/dump_boundary.py from the parent's build on an MI355X, twice, bitwise repeatable).
"""
import os
import sys

import numpy as np
import pytest
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import ext, hip
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 3


@pytest.fixture(scope="module")
def be(cuda):
    return Backend(random_mlp(13, [8, 6, 4], seed=3, bias_scale=0.5), cuda)


def _boxes(cuda):
    g = torch.Generator().manual_seed(5)
    lo = torch.randint(0, 6, (R, 13), generator=g).float()
    return lo.to(cuda), (lo + torch.randint(0, 3, (R, 13), generator=g).float()).to(cuda)


def _bounds_kw(be, cuda):
    """Complete keywords of a symbolic ``bounds`` launch on R rows, and the tensors they point into."""
    lo, hi = _boxes(cuda)
    f32 = dict(dtype=torch.float32, device=cuda)
    res = hip.ref.BoundResult(out_lb=torch.empty(R, **f32), out_ub=torch.empty(R, **f32))
    for k, shape in (("Lc", (R, 13)), ("L0", (R,)), ("Le", (R,)), ("Uc", (R, 13)), ("U0", (R,)), ("Ue", (R,))):
        setattr(res, k, torch.empty(shape, **f32))
    kw, keep = hip._bound_kw(be, lo, hi, None, res)
    return dict(kw, symbolic=1), (keep, res)


def _beta_kw(be, cuda):
    """Complete keywords of a ``beta_level`` launch on R rows (every pointer valid), and their tensors."""
    lo, hi = _boxes(cuda)
    NH = be.n_hidden
    f32 = dict(dtype=torch.float32, device=cuda)
    z = lambda *s: torch.zeros(*s, **f32)  # noqa: E731
    ph = torch.zeros(R, NH, dtype=torch.int8, device=cuda)
    kw, keep = hip._beta_rows(be, lo, hi, [1], z(R, 1), z(R, 1) + 1, z(R, NH) - 1, z(R, NH) + 1, z(R, NH) - 1,
                              z(R, NH) + 1, ph, ph, None, None)
    out = dict(wt=hip._beta_wt(be), par=z(R, 4, NH), t=z(R) + 0.5, scratch=z(R * 16 * NH),
               bound=torch.zeros(R, dtype=torch.float64, device=cuda),
               split=torch.zeros(R, dtype=torch.int32, device=cuda), xstar=z(R, 13), binit=z(R, 2), xpstar=z(R, 13))
    kw.update(hip._ptrs(**out), iters=2, lr_a=0.1, lr_b=0.5, lr_t=0.1, decay=1.0, lookahead=0, beta_pos=1, flags=1)
    return kw, (keep, out)


def test_unknown_key_is_refused(be, cuda):
    kw, _keep = _bounds_kw(be, cuda)
    with pytest.raises(TypeError, match="Lcc"):
        ext().bounds(hip._net(be), **kw, Lcc=kw["Lc"])


def test_missing_required_key_is_refused(be, cuda):
    kw, _keep = _bounds_kw(be, cuda)
    del kw["out_lb"]
    with pytest.raises(TypeError, match="out_lb"):
        ext().bounds(hip._net(be), **kw)
    kw, _keep = _beta_kw(be, cuda)
    del kw["par"]
    with pytest.raises(TypeError, match="par"):
        ext().beta_level(hip._net(be), **kw)


def test_bad_values_still_raise_value_error(be, cuda):
    kw, _keep = _beta_kw(be, cuda)
    with pytest.raises(ValueError, match="mode must be 0..3"):
        ext().beta_feas(hip._net(be), **kw, mode=4)
    with pytest.raises(ValueError, match="fpar required"):
        ext().beta_feas(hip._net(be), **kw, mode=1)
    with pytest.raises(ValueError, match="RA mask"):
        ext().beta_level(hip._net(be), **{**kw, "ramask": 1 << 2})


def test_omitted_optional_pointers_are_null(be, cuda):
    """``dead_in``, ``phase_in``, ``layer_lb`` / ``layer_ub`` left out: the plain symbolic pass, which
    gives the logit bounds of the pass that also writes the layer bounds, bit for bit."""
    lo, hi = _boxes(cuda)
    kw, (_keep, res) = _bounds_kw(be, cuda)
    assert not {"dead_in", "phase_in", "layer_lb", "layer_ub", "infeas"} & set(kw)
    ext().bounds(hip._net(be), **kw)
    a, b = hip.bounds(be, lo, hi), hip.bounds(be, lo, hi, keep_layers=True)
    torch.cuda.synchronize()
    for k in ("out_lb", "out_ub"):
        assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), k
        assert torch.equal(getattr(res, k).view(torch.int32), getattr(a, k).view(torch.int32)), k


def test_every_converted_wrapper_matches_the_parent_bitwise(cuda):
    """tools/dump_boundary.py in this process against the parent commit's recorded dump."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import dump_boundary
    finally:
        sys.path.pop(0)
    new = dump_boundary.dump(cuda)
    old = np.load(os.path.join(ROOT, "tests", "golden", "boundary_parent.npz"))
    assert sorted(new) == sorted(old.files)
    bad = [k for k in old.files if not dump_boundary.same_bits(new[k], old[k])]
    assert not bad, bad
