"""The point kernel's closed-node skip (csrc/points.hip): a workgroup none of whose tiles holds a point
of an open node returns before it stages the weights.  What the launch writes must be exactly what it
wrote before: nothing for tiles without an open point, the unmasked run's bounds for every other tile."""
import numpy as np
import pytest
import torch

from fairify_amd.models.mlp import random_mlp
from fairify_amd.ops import ext
from fairify_amd.ops import hip as H
from fairify_amd.ops.backend import Backend

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _run(be, x, row_open=None, open_mod=0):
    R = x.shape[0]
    lb = torch.full((R,), SENTINEL, dtype=torch.float32, device=x.device)
    ub = torch.full((R,), SENTINEL, dtype=torch.float32, device=x.device)
    kw = H._ptrs(flat=be.flat, x=x, out_lb=lb, out_ub=ub, row_open=row_open)
    if row_open is not None:
        kw["open_mod"] = open_mod
    ext().point_bounds(H._net(be), **kw, R=R, stream=H._stream(x.device))
    torch.cuda.synchronize()
    return lb.cpu().numpy(), ub.cpu().numpy()


# nodes: 3 (one tile), 17 (three tiles, one workgroup), 350 (44 tiles over 11 workgroups, most closed)
@pytest.mark.parametrize("nodes", [3, 17, 350])
@pytest.mark.parametrize("hidden", [[100, 100], [5, 5]], ids=["13,100,100,1", "13,5,5,1"])
def test_point_kernel_closed_node_skip(cuda, hidden, nodes):
    m = random_mlp(13, hidden, seed=7 + hidden[0], bias_scale=0.3)
    be = Backend(m, cuda)
    g = np.random.default_rng(nodes)
    R = 2 * nodes                                   # x rows then x' rows: point r belongs to node r % nodes
    x = torch.from_numpy(g.integers(-5, 20, size=(R, 13)).astype(np.float32)).to(cuda)
    full_lb, full_ub = _run(be, x)
    assert (full_lb != SENTINEL).all() and (full_lb <= full_ub).all()
    # every node closed: nothing is written
    closed = torch.zeros(nodes, dtype=torch.uint8, device=cuda)
    lb, ub = _run(be, x, closed, nodes)
    assert (lb == SENTINEL).all() and (ub == SENTINEL).all()
    # the first ninth of the nodes open (at least one): tiles with an open point equal the unmasked run bit
    # for bit, the others keep the sentinel -- whole workgroups of them at 350 nodes
    op = np.zeros(nodes, np.uint8)
    op[: max(1, nodes // 9)] = 1
    lb, ub = _run(be, x, torch.from_numpy(op).to(cuda), nodes)
    pt_open = op[np.arange(R) % nodes].astype(bool)
    tile_open = np.zeros(R, bool)
    for t0 in range(0, R, 16):
        tile_open[t0:t0 + 16] = pt_open[t0:t0 + 16].any()
    assert tile_open.any() and (nodes < 350 or not tile_open.all())
    assert np.array_equal(lb[tile_open], full_lb[tile_open]) and np.array_equal(ub[tile_open], full_ub[tile_open])
    assert (lb[~tile_open] == SENTINEL).all() and (ub[~tile_open] == SENTINEL).all()
