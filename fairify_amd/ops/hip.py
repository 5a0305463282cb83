"""Thin Python wrappers launching the HIP kernels of ``fairify_amd._C`` on torch's stream.

Every wrapper allocates its outputs with torch (caching allocator, current device), checks
shapes/dtypes/contiguity on the host before launch (a mis-shaped launch must never reach the
GPU), and passes raw pointers + ``torch.cuda.current_stream().cuda_stream``.
"""
from __future__ import annotations

import os
import threading
from typing import Optional, Sequence

import numpy as np
import torch

from . import ext
from . import reference as ref


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


# Per-backend / per-grid lazy device state is created under this lock: the runner's worker threads share
# one Backend per model, and a second thread that built its own copy and published it over the first
# freed the first thread's tensor while a native runtime still held its device pointer (the beta
# runtime's transposed weights: whole chunks of beta roots bounded with freed memory, exp R6 W/X).
_LAZY_LOCK = threading.Lock()


def _net(be):
    n = getattr(be, "_hipnet", None)
    if n is None:
        with _LAZY_LOCK:
            n = getattr(be, "_hipnet", None)
            if n is None:
                dims = [be.mlp.n_in] + be.mlp.widths
                n = ext().Net(dims, be.unit)
                assert n.total_floats == be.flat.numel(), (n.total_floats, be.flat.numel())
                be._hipnet = n
    return n


def _c(t: torch.Tensor, dtype, shape=None, name="tensor") -> torch.Tensor:
    if t.dtype != dtype:
        t = t.to(dtype)
    t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _fold_mask(fold: Sequence[int], n0: int) -> int:
    m = 0
    for d in fold:
        if not 0 <= int(d) < min(n0, 64):
            raise ValueError(f"fold dim {d} out of range")
        m |= 1 << int(d)
    return m


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _ptrs(**tensors) -> dict:
    """Keyword pointers for the struct-filling bindings (key = the ``args.h`` field name); a ``None``
    tensor's key is left out, which the binding reads as a null pointer."""
    return {k: t.data_ptr() for k, t in tensors.items() if t is not None}


def _bound_kw(be, lo, hi, dead=None, res=None, layer_lb=None, layer_ub=None, rows=None):
    """The block the bound-family bindings share: ``(keywords, tensors)`` -- row boxes, forced-dead
    mask, ``res``'s logit bounds and forms, layer bounds, R and the stream.  The checked contiguous
    ``tensors`` (same keys) must stay alive until the launch is enqueued."""
    B, n0 = lo.shape
    R = B if rows is None else rows       # rows: node-row expansion, R = V rows per box
    t = dict(flat=be.flat, lo=_c(lo, torch.float32, (B, n0), "lo"), hi=_c(hi, torch.float32, (B, n0), "hi"),
             dead_in=None if dead is None else _c(dead, torch.uint8, (R, be.n_hidden), "dead"),
             layer_lb=layer_lb, layer_ub=layer_ub)
    if res is not None:
        t.update(out_lb=res.out_lb, out_ub=res.out_ub, Lc=res.Lc, L0=res.L0, Le=res.Le, Uc=res.Uc, U0=res.U0,
                 Ue=res.Ue)
    return dict(_ptrs(**t), R=R, stream=_stream(lo.device)), t


def _layer_views(be, lay_lb, lay_ub):
    """Per-layer column views of [R, n_neurons] layer bounds."""
    offs = [0]
    for w in be.mlp.widths:
        offs.append(offs[-1] + w)
    n = len(be.mlp.widths)
    return [lay_lb[:, offs[i]:offs[i + 1]] for i in range(n)], [lay_ub[:, offs[i]:offs[i + 1]] for i in range(n)]


# ------------------------------------------------------------------------------------------------
def decode(grid, ids: torch.Tensor):
    """K1: grid-linear partition ids (int64, on the device) -> boxes ``lo, hi`` float32 [P, n0]
    decoded by ``fa_decode_kernel`` (the chunk tables are uploaded once per grid and device)."""
    dev = ids.device
    ids = _c(ids, torch.int64, (ids.shape[0],), "ids")
    tabs = grid.__dict__.setdefault("_dev_decode", {})
    key = str(dev)
    if key not in tabs:
        with _LAZY_LOCK:
            if key not in tabs:
                d = grid.decode_desc()
                cl = torch.from_numpy(d["chunk_lo"]).to(dev) if d["chunk_lo"].size else torch.zeros(1, device=dev)
                ch = torch.from_numpy(d["chunk_hi"]).to(dev) if d["chunk_hi"].size else torch.zeros(1, device=dev)
                torch.cuda.current_stream(dev).synchronize()     # published tables are complete for every stream
                tabs[key] = (d, cl, ch)
    d, cl, ch = tabs[key]
    n0 = int(d["radix"].shape[0])
    Pn = int(ids.shape[0])
    lo = torch.empty(Pn, n0, dtype=torch.float32, device=dev)
    hi = torch.empty(Pn, n0, dtype=torch.float32, device=dev)
    if Pn:
        ext().decode(d["radix"].tolist(), d["div"].tolist(), d["chunk_off"].tolist(), d["base_lo"].tolist(),
                     d["base_hi"].tolist(), ids.data_ptr(), Pn, cl.data_ptr(), ch.data_ptr(), lo.data_ptr(),
                     hi.data_ptr(), _stream(dev))
    return lo, hi


def pack_masks(masks: torch.Tensor, sel: int = 0xFF):
    """K6: [P, N] uint8 masks (dead where ``mask & sel``) -> (packed [P, ceil(N/8)] uint8 in
    ``numpy.packbits`` order, row hashes [P] int64) via ``fa_pack_masks_kernel``."""
    m = _c(masks, torch.uint8, name="masks")
    if m.dim() != 2:
        raise ValueError("masks: expected [P, N]")
    Pn, N = m.shape
    NB = (N + 7) // 8
    out = torch.empty(Pn, NB, dtype=torch.uint8, device=m.device)
    hsh = torch.empty(Pn, dtype=torch.int64, device=m.device)
    if Pn and N:
        ext().pack_masks(m.data_ptr(), Pn, N, N, int(sel), out.data_ptr(), NB, hsh.data_ptr(), _stream(m.device))
    return out, hsh


KNN_K = (1, 2, 3, 4, 5, 6, 7, 8, 10, 16)


def knn(X: torch.Tensor, k: int):
    """K10: indices [n, k] int32 of every row's k nearest rows of ``X`` (squared Euclidean, the
    row itself first, ties to the lower index) and their squared distances (``fa_knn_kernel``)."""
    X = _c(X, torch.float32, name="X")
    n, d = X.shape
    if not 1 <= d <= 64 or k not in KNN_K or k > n:
        raise ValueError(f"knn: unsupported shape n={n} d={d} k={k}")
    idx = torch.empty(n, k, dtype=torch.int32, device=X.device)
    dist = torch.empty(n, k, dtype=torch.float32, device=X.device)
    ext().knn(X.data_ptr(), n, d, k, idx.data_ptr(), dist.data_ptr(), _stream(X.device))
    return idx, dist


def activation_delta_sum(be, x: torch.Tensor, xp: torch.Tensor) -> torch.Tensor:
    """K13: sum over pairs of |act(x) - act(x')| per neuron [N] (hidden ReLU outputs, then the
    logit) via ``fa_actdiff_kernel``."""
    P_ = x.shape[0]
    x = _c(x, torch.float32, (P_, be.n0), "x")
    xp = _c(xp, torch.float32, (P_, be.n0), "xp")
    out = torch.zeros(be.mlp.n_neurons, dtype=torch.float32, device=x.device)
    if P_:
        ext().actdiff(_net(be), be.flat.data_ptr(), x.data_ptr(), xp.data_ptr(), P_, out.data_ptr(),
                      _stream(x.device))
    return out


def trace_marker(dev, tag: int) -> None:
    """Launch ``fa_trace_marker_kernel`` (a named one-thread kernel) on the current stream: the
    kernel trace's time-window delimiter (tools/trace_busy.py --window)."""
    ext().trace_marker(int(tag), 0, _stream(dev))


# ------------------------------------------------------------------------------------------------
def forward(be, x: torch.Tensor, dead: Optional[torch.Tensor] = None) -> torch.Tensor:
    shp = x.shape[:-1]
    x2 = _c(x.reshape(-1, be.n0), torch.float32, name="x")
    B = x2.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    if B == 0:
        return out.view(shp)
    d = None
    if dead is not None:
        d = _c(dead.reshape(-1, be.n_hidden), torch.uint8, (B, be.n_hidden), "dead")
    ext().forward(_net(be), be.flat.data_ptr(), x2.data_ptr(), B, _ptr(d), out.data_ptr(), _stream(x.device))
    return out.view(shp)


def activation_counts(be, x: torch.Tensor) -> torch.Tensor:
    # generic rows: run the forward per layer through the reference on-device (rarely used on the
    # GPU path; the fused sim kernel counts activations itself)
    return ref.activation_counts(be.ws, be.bs, x)


# ------------------------------------------------------------------------------------------------
def point_bounds(be, x: torch.Tensor, dead: Optional[torch.Tensor] = None):
    R = x.shape[0]
    x2 = _c(x, torch.float32, (R, be.n0), "x")
    lb = torch.empty(R, dtype=torch.float32, device=x.device)
    ub = torch.empty(R, dtype=torch.float32, device=x.device)
    d = None
    if dead is not None:
        d = _c(dead, torch.uint8, (R, be.n_hidden), "dead")
    if R:
        ext().point_bounds(_net(be), **_ptrs(flat=be.flat, x=x2, dead_in=d, out_lb=lb, out_ub=ub), R=R,
                           stream=_stream(x.device))
    return lb, ub


# ------------------------------------------------------------------------------------------------
def bounds(be, lo: torch.Tensor, hi: torch.Tensor, mode: str = "symbolic", dead: Optional[torch.Tensor] = None,
           keep_layers: bool = False, G: int = 0, fold: Sequence[int] = (),
           phase: Optional[torch.Tensor] = None, *, dead_out: bool = True, V: int = 0, pa: Sequence[int] = (),
           values: Optional[torch.Tensor] = None, skip_status: Optional[torch.Tensor] = None,
           skip_part: Optional[torch.Tensor] = None, fill: Optional[float] = None) -> ref.BoundResult:
    """``fold``: input dims with lo == hi in EVERY row (folded into the constant column of the
    register-resident symbolic kernel; the caller guarantees degeneracy).

    The keyword-only arguments give tests the launch form of the native BaB runtimes:
    ``dead_out=False`` passes no stable-inactive output (with no ``dead`` / ``phase``: a launch
    without any mask); ``V`` > 0 with ``pa`` and ``values`` [V, len(pa)] float32 expands every box
    of ``lo`` / ``hi`` into V rows whose PA dims take ``values[r % V]``; ``skip_status`` int8 [P] and
    ``skip_part`` int32 [boxes] skip the rows of partitions whose status is neither 3 nor 4;
    ``fill`` pre-fills every float output with a sentinel (0xEE for the byte outputs): skipped rows
    keep it."""
    R, n0 = lo.shape
    if n0 != be.n0:
        raise ValueError(f"box width {n0} != network input {be.n0}")
    if V < 0 or (V > 0 and (values is None or not len(pa))):
        raise ValueError("bounds: V > 0 needs pa and values [V, len(pa)]")
    if (skip_status is None) != (skip_part is None):
        raise ValueError("bounds: skip_status and skip_part go together")
    if V > 0:
        R *= V
    dev = lo.device
    sym = 1 if mode == "symbolic" else 0
    f32 = dict(dtype=torch.float32, device=dev)

    def new(*shape, dtype=torch.float32):
        if fill is None:
            return torch.empty(*shape, dtype=dtype, device=dev)
        return torch.full(shape, fill if dtype.is_floating_point else 0xEE, dtype=dtype, device=dev)

    res = ref.BoundResult(out_lb=new(R), out_ub=new(R))
    if sym:
        res.Lc = new(R, n0)
        res.L0 = new(R)
        res.Le = new(R)
        res.Uc = new(R, n0)
        res.U0 = new(R)
        res.Ue = new(R)
    N = be.mlp.n_neurons
    lay_lb = lay_ub = None
    if keep_layers:
        lay_lb = new(R, N)
        lay_ub = new(R, N)
    dead_out = new(R, be.n_hidden, dtype=torch.uint8) if be.n_hidden and dead_out else None
    ph = infeas = None
    if phase is not None:
        ph = _c(phase, torch.int8, (R, be.n_hidden), "phase")
        infeas = torch.zeros(R, dtype=torch.uint8, device=dev)
    kw, _keep = _bound_kw(be, lo, hi, dead, res, lay_lb, lay_ub, rows=R)
    bab = {}
    if V > 0:
        vals = _c(values, torch.float32, (V, len(pa)), "values")
        bab.update(V=V, pa=[int(d) for d in pa], values=vals.data_ptr())
    if skip_status is not None:
        st = _c(skip_status, torch.int8, None, "skip_status")
        sp = _c(skip_part, torch.int32, (lo.shape[0],), "skip_part")
        if st.dim() != 1 or (sp.numel() and (int(sp.min()) < 0 or int(sp.max()) >= st.shape[0])):
            raise ValueError("bounds: skip_part indexes outside skip_status")
        bab.update(skip_status=st.data_ptr(), skip_part=sp.data_ptr())
    if R:
        ext().bounds(_net(be), **kw, **_ptrs(dead_out=dead_out, phase_in=ph, infeas=infeas), symbolic=sym, G=G,
                     fold=_fold_mask(fold, n0), **bab)
    if infeas is not None:
        res.infeasible = infeas.bool()
    if keep_layers:
        res.layer_lb, res.layer_ub = _layer_views(be, lay_lb, lay_ub)
        res.lay_lb_full, res.lay_ub_full = lay_lb, lay_ub
    if dead_out is not None:
        res.dead_u8 = dead_out
        res.dead = dead_out.view(torch.bool)
    return res


# ------------------------------------------------------------------------------------------------
def crown(be, lo: torch.Tensor, hi: torch.Tensor, res: ref.BoundResult, dead: Optional[torch.Tensor] = None):
    """Backward output bounds (csrc/crown.hip) refining ``res`` in place: ``res`` must come from
    :func:`bounds` with mode='symbolic' and keep_layers=True on the same rows."""
    R, n0 = lo.shape
    N = be.mlp.n_neurons
    if res.Lc is None or res.layer_lb is None:
        raise ValueError("crown needs symbolic bounds with keep_layers=True")
    lay_lb = torch.cat(res.layer_lb, dim=1).contiguous() if isinstance(res.layer_lb, list) else res.layer_lb
    lay_ub = torch.cat(res.layer_ub, dim=1).contiguous() if isinstance(res.layer_ub, list) else res.layer_ub
    if lay_lb.shape[1] != N:          # keep_layers splits off the output neuron: append a pad column
        pad = torch.zeros(R, N - lay_lb.shape[1], dtype=torch.float32, device=lo.device)
        lay_lb = torch.cat([lay_lb, pad], dim=1).contiguous()
        lay_ub = torch.cat([lay_ub, pad], dim=1).contiguous()
    kw, _keep = _bound_kw(be, lo, hi, dead, res, lay_lb, lay_ub)
    if R:
        ext().crown(_net(be), **kw)
    return res


# ------------------------------------------------------------------------------------------------
def refine(be, lo: torch.Tensor, hi: torch.Tensor, res: ref.BoundResult, dead: Optional[torch.Tensor] = None,
           phase: Optional[torch.Tensor] = None):
    """Back-substituted hidden-layer bounds (csrc/refine.hip) tightening ``res.layer_lb/ub`` in place
    (ref.crown_refine): ``res`` must come from :func:`bounds` with mode='symbolic' and
    keep_layers=True on the same rows.  Networks the kernel cannot hold keep the forward bounds.
    ``phase`` [R, n_hidden] int8 (ReLU-phase rows: +1 active / -1 inactive fixed, 0 free): the
    bounds hold on the region where the fixed phases hold, and ``res.infeasible`` [R] also marks rows
    whose refined bounds contradict a fixed phase (empty region)."""
    R, n0 = lo.shape
    if res.lay_lb_full is None:
        raise ValueError("refine needs symbolic bounds with keep_layers=True (HIP layout)")
    kw, _keep = _bound_kw(be, lo, hi, dead, None, res.lay_lb_full, res.lay_ub_full)
    ph = _c(phase, torch.int8, (R, be.n_hidden), "phase") if phase is not None else None
    infeas = torch.zeros(R, dtype=torch.uint8, device=lo.device) if phase is not None else None
    if R:
        ext().refine(_net(be), **kw, **_ptrs(phase_in=ph, infeas=infeas))
    if infeas is not None:
        res.infeasible = infeas.bool() if res.infeasible is None else (res.infeasible | infeas.bool())
    Nh = be.n_hidden
    if Nh:
        res.dead = res.lay_ub_full[:, :Nh] <= 0
        res.dead_u8 = res.dead.to(torch.uint8)
        res.active = res.lay_lb_full[:, :Nh] >= 0
    return res


# ------------------------------------------------------------------------------------------------
def backward_bounds(be, lo: torch.Tensor, hi: torch.Tensor, dead: Optional[torch.Tensor] = None,
                    keep_layers: bool = True) -> Optional[ref.BoundResult]:
    """Every neuron's bounds and the logit's forms by back-substitution alone (csrc/refine.hip mode
    FULL, ref.backward_bounds).  ``None`` when the network does not fit the kernel."""
    R, n0 = lo.shape
    f32 = dict(dtype=torch.float32, device=lo.device)
    res = ref.BoundResult(out_lb=torch.empty(R, **f32), out_ub=torch.empty(R, **f32),
                          Lc=torch.empty(R, n0, **f32), L0=torch.empty(R, **f32), Le=torch.empty(R, **f32),
                          Uc=torch.empty(R, n0, **f32), U0=torch.empty(R, **f32), Ue=torch.empty(R, **f32))
    N = be.mlp.n_neurons
    lay_lb = torch.empty(R, N, **f32) if keep_layers else None
    lay_ub = torch.empty(R, N, **f32) if keep_layers else None
    kw, keep = _bound_kw(be, lo, hi, dead, res, lay_lb, lay_ub)
    if R and ext().backward_bounds(_net(be), **kw) == -1:
        return None
    if keep_layers:
        res.layer_lb, res.layer_ub = _layer_views(be, lay_lb, lay_ub)
        res.lay_lb_full, res.lay_ub_full = lay_lb, lay_ub
        Nh = be.n_hidden
        res.dead = lay_ub[:, :Nh] <= 0
        d = keep["dead_in"]
        if d is not None:
            res.dead = res.dead | d.bool()
        res.active = (lay_lb[:, :Nh] >= 0) & ~res.dead
    return res


# ------------------------------------------------------------------------------------------------
def crown_phase(be, lo: torch.Tensor, hi: torch.Tensor, res: ref.BoundResult, phase: Optional[torch.Tensor] = None):
    """ReLU-phase backward bounds (csrc/relu.hip: fa_crown_phase_kernel) on rows bounded by
    :func:`bounds` (symbolic, keep_layers, same ``phase``).  Refines ``res`` (logit bounds, forms)
    in place like ref.crown_phase + the caller's intersection, and returns
    (ref.PhaseCrown, None) -- the kernel writes the better input forms into ``res`` directly."""
    R, n0 = lo.shape
    dev = lo.device
    if res.lay_lb_full is None:
        raise ValueError("crown_phase needs bounds(..., keep_layers=True) from the HIP path")
    kw, _keep = _bound_kw(be, lo, hi, None, res, res.lay_lb_full, res.lay_ub_full)
    ph = _c(phase, torch.int8, (R, be.n_hidden), "phase") if phase is not None else None
    split = torch.full((R, 2), -1, dtype=torch.int32, device=dev)
    score = torch.zeros(R, 2, dtype=torch.float32, device=dev)
    low = torch.zeros(R, 2, dtype=torch.float32, device=dev)
    infeas = res.infeasible.to(torch.uint8).contiguous() if res.infeasible is not None else None
    if R:
        ext().crown_phase(_net(be), **kw, **_ptrs(phase=ph, infeas=infeas, split=split, score=score, low=low))
    return ref.PhaseCrown(low=low, split=split.long(), score=score), None


# ------------------------------------------------------------------------------------------------
def smear_w0t(W0: torch.Tensor) -> torch.Tensor:
    """``CertArgs.W0T`` of first-layer weights ``W0`` [n0, n1]: [n1, NM] rows of ``|W0[:, j]|``, zero
    padded to the certify kernel's register width (NM = 16 for n0 <= 16, else 32)."""
    n0, n1 = W0.shape
    if n0 > 32:
        raise ValueError("smear scores need n0 <= 32")
    out = torch.zeros(n1, 16 if n0 <= 16 else 32, dtype=torch.float32, device=W0.device)
    out[:, :n0] = W0.to(torch.float32).abs().T
    return out


def pair_certify(be, res_x, res_xp, xlo, xhi, xplo, xphi, pairs, values, pa, shared, relaxed, *, ra=(), tau=0.0,
                 skip_closed=False, status=None, part=None, smear=False, lay_lb=None, lay_ub=None, W0T=None,
                 prefill=None, full=False):
    """The pair certificate of ``Nn`` nodes (csrc/certify.hip) -> ref.PairDecision.

    The keyword-only arguments are the ``CertArgs`` fields the native BaB runtime sets; the defaults
    are the torch loop's call.  ``ra`` / ``tau``: the candidate x' is clipped to within tau of x on
    these dims.  ``status`` [P] int8 with ``part`` [Nn] int32: nodes of partitions that are not
    RUNNING / STOPPING are closed unevaluated.  ``skip_closed``: closed nodes write only open, score
    and leaf.  ``smear`` with ``lay_lb`` / ``lay_ub`` [Nn*V, lay_N] (layer 0 first) and ``W0T``
    (:func:`smear_w0t`): first-layer smear split scores.  ``prefill``: the outputs start filled with
    this value (what a skipped node leaves behind).  ``full``: also return a dict with ``gmin`` and
    ``tstar`` [Nn, Q] (written by the two-kernel path only), ``scores`` [Nn, 2 n0], ``leaf`` and the
    uint8 open flags ``open_u8``."""
    Nn, n0 = xlo.shape
    dev = xlo.device
    V = values.shape[0]
    Pp = pairs.shape[0]
    norient = 2 if relaxed else 1
    ra = [int(i) for i in ra]
    if any(not 0 <= i < n0 for i in ra):
        raise ValueError("ra dim out of range")
    extra = {}
    if (status is None) != (part is None):
        raise ValueError("status and part go together")
    if status is not None:
        status = _c(status, torch.int8, None, "status")
        part = _c(part, torch.int32, (Nn,), "part")
        if status.dim() != 1 or (Nn and not 0 <= int(part.min()) <= int(part.max()) < status.shape[0]):
            raise ValueError("part indexes status [P]")
        extra.update(_ptrs(status=status, part=part))
    if skip_closed:
        extra["skip_closed"] = 1
    if smear:
        if lay_lb is None or lay_ub is None or W0T is None or lay_lb.dim() != 2:
            raise ValueError("smear needs lay_lb, lay_ub and W0T")
        lay_N, n1 = lay_lb.shape[1], W0T.shape[0]
        lay_lb = _c(lay_lb, torch.float32, (Nn * V, lay_N), "lay_lb")
        lay_ub = _c(lay_ub, torch.float32, (Nn * V, lay_N), "lay_ub")
        W0T = _c(W0T, torch.float32, (n1, 16 if n0 <= 16 else 32), "W0T")
        if not 0 < n1 <= lay_N:
            raise ValueError("smear: the first layer's n1 neurons lead the lay_N layer bounds")
        extra.update(_ptrs(lay_lb=lay_lb, lay_ub=lay_ub, W0T=W0T), smear=1, lay_N=lay_N, n1=n1)
    xlo = _c(xlo, torch.float32, (Nn, n0), "xlo")
    xhi = _c(xhi, torch.float32, (Nn, n0), "xhi")
    xplo = _c(xplo, torch.float32, (Nn, n0), "xplo")
    xphi = _c(xphi, torch.float32, (Nn, n0), "xphi")
    for r in (res_x, res_xp):
        if r.Lc is None or tuple(r.Lc.shape) != (Nn * V, n0):
            raise ValueError("pair_certify needs symbolic forms for Nn*V rows")
    pairs_c = _c(pairs, torch.int64, (Pp, 2), "pairs")
    values_c = _c(values, torch.int64, None, "values")
    sh = _c(shared, torch.uint8, (n0,), "shared")
    Q = Pp * norient

    def new(*shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device=dev)
        return t if prefill is None else t.fill_(prefill)

    gmin = new(Nn, Q)
    tstar = new(Nn, Q)
    open_ = new(Nn, dtype=torch.uint8)
    score = new(Nn)
    split = new(Nn, dtype=torch.int64)
    cx = new(Nn, n0)
    cxp = new(Nn, n0)
    cv = new(Nn, dtype=torch.int64)
    co = new(Nn, dtype=torch.int64)
    # the forms and logit bounds of the x rows, and (key + "p") of the x' rows
    forms = {}
    for r, p in ((res_x, ""), (res_xp, "p")):
        for key, t in (("Lc", r.Lc), ("L0", r.L0), ("Le", r.Le), ("Uc", r.Uc), ("U0", r.U0), ("Ue", r.Ue),
                       ("olb", r.out_lb), ("oub", r.out_ub)):
            forms[key + p] = _c(t, torch.float32)
    scores = new(Nn, 2 * n0)
    leaf = new(Nn, dtype=torch.uint8)
    if Nn:
        pa_l = [int(i) for i in pa.tolist()]
        if any(not 0 <= i < n0 for i in pa_l) or tuple(values_c.shape) != (V, len(pa_l)):
            raise ValueError("pa dims out of range or values not [V, npa]")
        ext().certify(Nn=Nn, n0=n0, V=V, Pp=Pp, norient=norient, pa=pa_l, ra=ra,
                      tau=float(tau), unit=be.unit, gmarg=ref.gamma(2 * n0 + 4, be.unit), stream=_stream(dev), **extra,
                      **_ptrs(xlo=xlo, xhi=xhi, xplo=xplo, xphi=xphi, pairs=pairs_c, values=values_c, shared=sh,
                              gmin=gmin, tstar=tstar, open=open_, score=score, split_dim=split, cand_x=cx,
                              cand_xp=cxp, cand_v=cv, cand_o=co, scores=scores, leaf=leaf, **forms))
    dec = ref.PairDecision(open_=open_.bool(), score=score, split_dim=split, cand_x=cx, cand_xp=cxp,
                           cand_v=cv, cand_orient=co)
    if full:
        return dec, dict(gmin=gmin, tstar=tstar, scores=scores, leaf=leaf, open_u8=open_)
    return dec


# ------------------------------------------------------------------------------------------------
# BaB level kernels (csrc/bab.hip), one launch at a time.  The native runtime launches them itself; these
# wrappers exist so that one level can be run on hand-made state and compared with a plain oracle
# (tests/split_cases.py).  Per-partition state and counters are updated in place, so nothing is converted
# or copied here: a tensor of the wrong dtype, shape, device or layout raises.
def _inplace(t, dtype, shape, name, dev=None):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device.type != "cuda":
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor on the GPU")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name}: on {t.device}, the launch runs on {dev}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _settle_kw(P, dev, pre, *, status, lvl_open, part_nodes, nodes_start, prev_start, counters_cur, counters_next,
               host_counts, budget2, max_open, esc_budget=(), esc_open=(), part_open=None, pbudget=None, prob=None,
               done=None):
    """Keywords of a SettleArgs block (keys prefixed with ``pre``); the tensors are checked."""
    i32, t = torch.int32, {}
    t["status"] = _inplace(status, torch.int8, (P,), "status", dev)
    for name, v in (("lvl_open", lvl_open), ("part_nodes", part_nodes), ("nodes_start", nodes_start),
                    ("prev_start", prev_start)):
        t[name] = _inplace(v, i32, (P,), name, dev)
    for name, v in (("counters_cur", counters_cur), ("counters_next", counters_next), ("host_counts", host_counts)):
        t[name] = _inplace(v, i32, (2,), name, dev)
    if part_open is not None:
        t["part_open"] = _inplace(part_open, i32, (P,), "part_open", dev)
    if (pbudget is None) != (prob is None):
        raise ValueError("pbudget and prob go together")
    if prob is not None:
        t["pbudget"] = _inplace(pbudget, i32, (P,), "pbudget", dev)
        t["prob"] = _inplace(prob, torch.uint8, (P,), "prob", dev)
    if done is not None:
        t["done"] = _inplace(done, i32, (1,), "done", dev)
    esc_budget, esc_open = [int(v) for v in esc_budget], [int(v) for v in esc_open]
    if len(esc_budget) != len(esc_open) or len(esc_budget) > 4:
        raise ValueError("esc_budget / esc_open: the same number of steps, at most 4")
    kw = dict(_ptrs(**t), P=P, budget2=int(budget2), max_open=int(max_open), esc_budget=esc_budget,
              esc_open=esc_open)
    return {pre + k: v for k, v in kw.items()}


def settle(*, status, **state):
    """Level end in its own launch (fa_settle_kernel) on per-partition state [P], in place: ``status``
    int8, ``lvl_open`` / ``part_nodes`` / ``nodes_start`` / ``prev_start`` int32 (``part_open``,
    ``pbudget`` with ``prob`` uint8: optional), the level's counters ``counters_cur`` [2] int32, the
    next slot ``counters_next`` [2] (cleared), ``budget2``, ``max_open``, ``esc_budget`` / ``esc_open``
    (the escalation steps).  ``host_counts`` [2] int32 (device memory; allocated when left out) gets the
    level counters and is returned."""
    P, dev = status.shape[0], status.device
    if P < 1:
        raise ValueError("settle needs at least one partition")
    if state.get("host_counts") is None:
        state["host_counts"] = torch.zeros(2, dtype=torch.int32, device=dev)
    if state.get("done") is not None:
        raise ValueError("done belongs to the fused level end")
    ext().settle(stream=_stream(dev), **_settle_kw(P, dev, "", status=status, **state))
    return state["host_counts"]


def split_level(*, xlo, xhi, part, open, leaf, scores, cand_x, cand_xp, pe_lb, pe_ub, olb, oub, olbp, oubp, pairs,
                values, pa, status, part_nodes, nodes_start, prev_start, budget, budget2, m, target, cap, cand_cap,
                xplo=None, xphi=None, ra=(), tau=0.0, shared=None, norient=None, lvl_open=None, part_open=None,
                pbudget=None, prob=None, counters=None, pool=None, cand_buf=None, prefill=None, settle=None):
    """One sub-batch of a BaB level (fa_split_kernel / fa_split_group_kernel) -> (pool, cand_buf, counters).

    Inputs per node: boxes ``xlo`` / ``xhi`` [Nn, n0] float32 (relaxed: with ``xplo`` / ``xphi``, ``ra``,
    ``tau`` and ``shared`` [n0] uint8), ``part`` [Nn] int32, ``open`` / ``leaf`` [Nn] uint8, ``scores``
    [Nn, 2 n0], ``cand_x`` / ``cand_xp`` [Nn, n0], ``pe_lb`` / ``pe_ub`` [2 Nn], the row bounds ``olb``
    ... ``oubp`` [Nn V]; ``pairs`` [Pp, 2] / ``values`` [V, npa] int64, ``pa`` the PA dims.  Per-partition
    state [P], updated in place: ``status`` int8, ``part_nodes`` int32 (``lvl_open`` int32, ``prob``
    uint8: optional); read: ``nodes_start``, ``prev_start`` (``pbudget``: optional).

    ``pool``: dict of ``oxlo`` / ``oxhi`` (relaxed: ``oxplo`` / ``oxphi``) [cap, n0] float32 and ``opart``
    [cap] int32; ``cand_buf`` [cand_cap, 2 n0 + 1] float32 (at least that many rows, and at least one);
    ``counters`` [2] int32 (children, candidates).  Each is allocated when left out (the buffers filled with ``prefill``, the counters
    zero) and returned, so a level's later sub-batches pass the first one's back in.

    ``settle``: dict of the remaining :func:`settle` keywords (``counters_next``, ``host_counts``,
    ``max_open``, ``esc_budget``, ``esc_open``, ``done`` [1] int32 zero) fuses the level end into this
    launch; the per-partition state and ``budget2`` are this call's."""
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    if xlo.dim() != 2 or xlo.shape[0] < 1:
        raise ValueError("xlo: expected [Nn, n0] with at least one node")
    Nn, n0 = xlo.shape
    dev = xlo.device
    relaxed = xplo is not None
    if norient is None:
        norient = 2 if relaxed else 1
    P = status.shape[0]
    V, Pp = values.shape[0], pairs.shape[0]
    pa, ra = [int(i) for i in pa], [int(i) for i in ra]
    if any(not 0 <= i < n0 for i in pa + ra) or len(pa) > 8 or len(ra) > 8 or n0 > 64:
        raise ValueError("PA / RA dims out of range, more than 8 of them, or n0 > 64")
    if norient not in (1, 2) or V < 1 or cap < 0 or cand_cap < 0:
        raise ValueError("norient, V, cap or cand_cap out of range")
    t = dict(xlo=_inplace(xlo, f32, (Nn, n0), "xlo"), xhi=_inplace(xhi, f32, (Nn, n0), "xhi", dev),
             part=_inplace(part, i32, (Nn,), "part", dev), open=_inplace(open, u8, (Nn,), "open", dev),
             leaf=_inplace(leaf, u8, (Nn,), "leaf", dev), scores=_inplace(scores, f32, (Nn, 2 * n0), "scores", dev),
             cand_x=_inplace(cand_x, f32, (Nn, n0), "cand_x", dev),
             cand_xp=_inplace(cand_xp, f32, (Nn, n0), "cand_xp", dev),
             pe_lb=_inplace(pe_lb, f32, (2 * Nn,), "pe_lb", dev), pe_ub=_inplace(pe_ub, f32, (2 * Nn,), "pe_ub", dev),
             pairs=_inplace(pairs, torch.int64, (Pp, 2), "pairs", dev),
             values=_inplace(values, torch.int64, (V, len(pa)), "values", dev),
             status=_inplace(status, torch.int8, (P,), "status", dev),
             part_nodes=_inplace(part_nodes, i32, (P,), "part_nodes", dev),
             nodes_start=_inplace(nodes_start, i32, (P,), "nodes_start", dev),
             prev_start=_inplace(prev_start, i32, (P,), "prev_start", dev))
    for name, v in (("olb", olb), ("oub", oub), ("olbp", olbp), ("oubp", oubp)):
        t[name] = _inplace(v, f32, (Nn * V,), name, dev)
    if relaxed:
        if xphi is None or shared is None:
            raise ValueError("a relaxed level needs xplo, xphi and shared")
        t.update(xplo=_inplace(xplo, f32, (Nn, n0), "xplo", dev), xphi=_inplace(xphi, f32, (Nn, n0), "xphi", dev),
                 shared=_inplace(shared, u8, (n0,), "shared", dev))
    elif xphi is not None or ra:
        raise ValueError("xphi / ra without xplo")
    for name, v, dt in (("lvl_open", lvl_open, i32), ("part_open", part_open, i32), ("pbudget", pbudget, i32),
                        ("prob", prob, u8)):
        if v is not None:
            t[name] = _inplace(v, dt, (P,), name, dev)
    if Nn and not 0 <= int(part.min()) <= int(part.max()) < P:
        raise ValueError("part indexes the per-partition state [P]")
    if Pp and not 0 <= int(pairs.min()) <= int(pairs.max()) < V:
        raise ValueError("pairs index values [V, npa]")

    def new(*shape, dtype=f32):
        o = torch.empty(*shape, dtype=dtype, device=dev)
        return o if prefill is None else o.fill_(prefill)

    rows, crows = max(cap, 1), max(cand_cap, 1)     # a capacity of 0 still gets a buffer: no null pointers
    if pool is None:
        pool = dict(oxlo=new(rows, n0), oxhi=new(rows, n0), opart=new(rows, dtype=i32))
        if relaxed:
            pool.update(oxplo=new(rows, n0), oxphi=new(rows, n0))
    for name in ("oxlo", "oxhi") + (("oxplo", "oxphi") if relaxed else ()):
        t[name] = _inplace(pool[name], f32, None, name, dev)
    t["opart"] = _inplace(pool["opart"], i32, None, "opart", dev)
    if cand_buf is None:
        cand_buf = new(crows, 2 * n0 + 1)
    t["cand_buf"] = _inplace(cand_buf, f32, None, "cand_buf", dev)
    # buffers may be longer than the capacity (guard rows that must stay untouched), never shorter
    for name, v in t.items():
        if name in ("oxlo", "oxhi", "oxplo", "oxphi") and (v.dim() != 2 or v.shape[1] != n0 or v.shape[0] < rows):
            raise ValueError(f"{name}: expected [>= {rows}, {n0}], got {tuple(v.shape)}")
    if t["opart"].dim() != 1 or t["opart"].shape[0] < rows:
        raise ValueError(f"opart: expected at least {rows} entries")
    if cand_buf.dim() != 2 or cand_buf.shape[1] != 2 * n0 + 1 or cand_buf.shape[0] < crows:
        raise ValueError(f"cand_buf: expected [>= {crows}, {2 * n0 + 1}], got {tuple(cand_buf.shape)}")
    if counters is None:
        counters = torch.zeros(2, dtype=i32, device=dev)
    _inplace(counters, i32, (2,), "counters", dev)
    extra = {}
    if settle is not None:
        extra = _settle_kw(P, dev, "settle_", status=status, lvl_open=lvl_open, part_nodes=part_nodes,
                           nodes_start=nodes_start, prev_start=prev_start, counters_cur=counters,
                           part_open=part_open, pbudget=pbudget, prob=prob, budget2=budget2, **settle)
        if "settle_done" not in extra:
            raise ValueError("the fused level end needs done")
    ext().split_level(Nn=Nn, n0=n0, relaxed=int(relaxed), V=V, Pp=Pp, norient=norient, ra=ra, tau=float(tau), pa=pa,
                      budget=int(budget), budget2=int(budget2), m=int(m), target=int(target), cap=int(cap),
                      cand_cap=int(cand_cap), count_out=counters.data_ptr(), cand_count=counters[1:].data_ptr(),
                      stream=_stream(dev), **_ptrs(**t), **extra)
    return pool, cand_buf, counters


def bab_init(status0, run, lo, hi, *, budget, ra=(), tau=0.0, relaxed=False, escalate=False):
    """Solve start (fa_bab_init_kernel) from the staged block of ``status0`` [P] int8 (host), the running
    partition ids ``run`` [n_run] and their boxes ``lo`` / ``hi`` [n_run, n0] -> dict of the device state:
    ``status``, ``nodes``, ``open_left``, ``lvl_open``, ``nodes_start``, ``prev_start`` [P], the root pool
    ``part``, ``xlo``, ``xhi`` (relaxed: ``xplo``, ``xphi``), ``counters`` [5] and, with ``escalate``,
    ``pbudget`` / ``prob``.  Everything starts filled with a sentinel (-7 / 0xF9) the kernel must
    overwrite."""
    import numpy as np

    dev = torch.device("cuda", torch.cuda.current_device())
    st = np.ascontiguousarray(status0, np.int8)
    run = np.ascontiguousarray(run, np.int32)
    lo, hi = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32)
    P, n_run = st.shape[0], run.shape[0]
    if lo.ndim != 2 or lo.shape != hi.shape or lo.shape[0] != n_run or P < 1 or n_run < 1:
        raise ValueError("lo / hi: expected [n_run, n0], with at least one partition running")
    n0 = lo.shape[1]
    ra = [int(i) for i in ra]
    if any(not 0 <= i < n0 for i in ra) or len(ra) > 8:
        raise ValueError("RA dims out of range")
    if n_run and not 0 <= int(run.min()) <= int(run.max()) < P:
        raise ValueError("run indexes the partitions")
    block = st.tobytes() + b"\0" * (-P % 4) + run.tobytes() + lo.tobytes() + hi.tobytes()
    stage = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(dev)

    def new(*shape, dtype=torch.int32):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    s = dict(status=new(P, dtype=torch.int8), nodes=new(P), open_left=new(P), lvl_open=new(P), nodes_start=new(P),
             prev_start=new(P), part=new(n_run), xlo=new(n_run, n0, dtype=torch.float32),
             xhi=new(n_run, n0, dtype=torch.float32), counters=new(5))
    if relaxed:
        s.update(xplo=new(n_run, n0, dtype=torch.float32), xphi=new(n_run, n0, dtype=torch.float32))
    if escalate:
        s.update(pbudget=new(P), prob=torch.full((P,), 0xF9, dtype=torch.uint8, device=dev))
    ext().bab_init(P=P, n_run=n_run, n0=n0, ra=ra if relaxed else [], tau=float(tau), budget=int(budget),
                   stream=_stream(dev), stage=stage.data_ptr(), **_ptrs(**s))
    torch.cuda.current_stream(dev).synchronize()      # the staged block lives until the kernel has read it
    return s


def bab_finish(status, nodes, open_left):
    """Solve end (fa_bab_finish_kernel): [3, P] int32 = status, nodes, open_left."""
    P, dev = status.shape[0], status.device
    _inplace(status, torch.int8, (P,), "status")
    _inplace(nodes, torch.int32, (P,), "nodes", dev)
    _inplace(open_left, torch.int32, (P,), "open_left", dev)
    out = torch.full((3, P), -7, dtype=torch.int32, device=dev)
    if P:
        ext().bab_finish(P=P, stream=_stream(dev), **_ptrs(status=status, nodes=nodes, open_left=open_left, out=out))
    return out


def mark_unknown(part, status):
    """Time budget hit (fa_mark_unknown_kernel): the RUNNING / STOPPING partitions among ``part`` [n]
    int32 become UNKNOWN in ``status`` [P] int8, in place."""
    n, P, dev = part.shape[0], status.shape[0], status.device
    _inplace(status, torch.int8, (P,), "status")
    _inplace(part, torch.int32, (n,), "part", dev)
    if n and not 0 <= int(part.min()) <= int(part.max()) < P:
        raise ValueError("part indexes status [P]")
    if n:
        ext().mark_unknown(n=n, stream=_stream(dev), **_ptrs(part=part, status=status))


def set_status(idx, status, v: int):
    """``status[idx] = v`` (fa_set_status_kernel), in place; ``idx`` [n] int32."""
    n, P, dev = idx.shape[0], status.shape[0], status.device
    _inplace(status, torch.int8, (P,), "status")
    _inplace(idx, torch.int32, (n,), "idx", dev)
    if n and not 0 <= int(idx.min()) <= int(idx.max()) < P:
        raise ValueError("idx indexes status [P]")
    if not -128 <= int(v) <= 127:
        raise ValueError("v: an int8 status")
    if n:
        ext().set_status(n=n, v=int(v), stream=_stream(dev), **_ptrs(idx=idx, status=status))


# ------------------------------------------------------------------------------------------------
def _parse_sim_blocks(v: Optional[str]) -> int:
    if v is None or v.strip() == "":
        return 0
    try:
        n = int(v)
    except ValueError:
        raise ValueError(f"FAIRIFY_SIM_BLOCKS={v!r}: expected a non-negative integer") from None
    if n < 0:
        raise ValueError(f"FAIRIFY_SIM_BLOCKS={v!r}: expected a non-negative integer")
    return n


# parsed once at import (a bad value fails here, not inside a worker thread mid-run); tests that
# change the variable at run time set _SIM_BLOCKS_ENV = "dynamic" to re-read it per call
_SIM_BLOCKS = _parse_sim_blocks(os.environ.get("FAIRIFY_SIM_BLOCKS"))
_SIM_BLOCKS_ENV: Optional[str] = None


def _sim_split(P: int, n_samples: int) -> int:
    """Workgroups per partition for ``fa_sim_kernel``: with ``FAIRIFY_SIM_BLOCKS=B`` a short list
    of partitions with a large sample budget (the residual falsifier on a per-rank residue) is
    spread over about B workgroups instead of one per partition walking its 64-sample tiles
    serially.  Results are bit-identical either way (tests/test_kernels_gpu.py).  Off by default:
    with 8 concurrent host streams the extra blocks only contend with the other streams' bound
    kernels (A/B in profiles/r1_sim_split_ab.md)."""
    target = _SIM_BLOCKS if _SIM_BLOCKS_ENV is None else _parse_sim_blocks(os.environ.get("FAIRIFY_SIM_BLOCKS"))
    if not P or target <= P:
        return 1
    tiles = (n_samples + 63) // 64
    return max(1, min(tiles, -(-target // P)))


# FAIRIFY_SIM_REGCOUNT=0: every network runs the run-time-shape simulation kernel (A/B against the
# compile-time-shape instances that count activations in registers, csrc/forward.hip); passed per
# call, parsed once at import like FAIRIFY_SIM_BLOCKS (_SIM_REGCOUNT_ENV = "dynamic": re-read per call)
_SIM_REGCOUNT = os.environ.get("FAIRIFY_SIM_REGCOUNT", "1").strip() != "0"
_SIM_REGCOUNT_ENV: Optional[str] = None


def _sim_regcount() -> bool:
    if _SIM_REGCOUNT_ENV is None:
        return _SIM_REGCOUNT
    return os.environ.get("FAIRIFY_SIM_REGCOUNT", "1").strip() != "0"


def _query_kw(be, q, lo, hi, pids, values, pairs):
    """The query block the sampling-family bindings share: ``(keywords, tensors)`` -- boxes, PA table
    and pairs, P / V / Pp, the stream and, with ``pids`` (the kernels that draw their samples), the RA
    dims and tau of a relaxed query.  The checked contiguous ``tensors`` (same keys) must stay alive
    until the launch is enqueued."""
    P, n0 = lo.shape
    Pp = pairs.shape[0]
    t = dict(flat=be.flat, lo=_c(lo, torch.float32, (P, n0), "lo"), hi=_c(hi, torch.float32, (P, n0), "hi"),
             values=_c(values, torch.int64, None, "values"), pairs=_c(pairs, torch.int64, (Pp, 2), "pairs"))
    kw = dict(P=P, V=int(values.shape[0]), pa=list(q.pa_idx), Pp=int(Pp), stream=_stream(lo.device))
    if pids is not None:
        t["pids"] = _c(pids, torch.int64, (P,), "pids")
        kw.update(ra=list(q.ra_idx) if q.relaxed else [], tau=int(q.tau) if q.relaxed else 0)
    kw.update(_ptrs(**t))
    return kw, t


def simulate(be, q, lo, hi, pids, n_samples, seed, values, pairs, bisect_pairs, bisect_steps, return_z0=False):
    from ..engine.sim import SimResult, boundary_walk

    P, n0 = lo.shape
    dev = lo.device
    kw, t = _query_kw(be, q, lo, hi, pids, values, pairs)
    split = _sim_split(P, n_samples)
    counts = (torch.zeros if split > 1 else torch.empty)(P, be.mlp.n_neurons, dtype=torch.int32, device=dev)
    keys = torch.full((P,), 0x7FFFFFFF, dtype=torch.int32, device=dev) if split > 1 else None
    found = torch.zeros(P, dtype=torch.uint8, device=dev)
    wx = torch.zeros(P, n0, dtype=torch.float32, device=dev)
    wxp = torch.zeros(P, n0, dtype=torch.float32, device=dev)
    walk = bool(bisect_pairs and bisect_steps)
    z0 = torch.empty(P, n_samples, dtype=torch.float32, device=dev) if (walk or return_z0) else None
    if P and n_samples:
        kw["tau"] = int(q.tau)          # as given, also where the query is not relaxed (no RA dims then)
        ext().sim(_net(be), **kw, **_ptrs(counts=counts, found=found, wit_x=wx, wit_xp=wxp, z0=z0, keys=keys),
                  n_samples=n_samples, seed=int(seed) & 0xFFFFFFFF, split=split, regcount=int(_sim_regcount()))
    res = SimResult(counts=counts, found=found.bool(), wit_x=wx, wit_xp=wxp)
    if return_z0:
        res.z0 = z0
    if walk:
        boundary_walk(be, q, t["lo"], t["hi"], t["pids"], n_samples, seed, t["values"], t["pairs"], res, z0,
                      bisect_pairs, bisect_steps)
    return res


def _rowfwd_covers(be) -> bool:
    """The net shape of the row-forward kernels (csrc/rowfwd.h): no layer over 160 wide, at most 32 inputs."""
    return max([be.n0] + list(be.widths)) <= 160 and be.n0 <= 32


def _pairs_kw(q, E: int) -> dict:
    """The ``pa`` / ``ra`` / ``tau`` / ``E`` keywords of the bindings that take a query (RA dims and tau
    only of a relaxed one)."""
    return dict(pa=list(q.pa_idx), ra=list(q.ra_idx) if q.relaxed else [], tau=int(q.tau) if q.relaxed else 0, E=E)


def _row_inputs(be, q, X, own, values, pairs, what):
    """Checks of the rows, own indices and PA tables that ``audit_masks`` and ``neighbour_masks`` share:
    the checked contiguous ``(X, own, values, pairs)`` and ``(N, V, Pp, E)``."""
    from .audit import MAX_VALUES
    from .rate import MAX_OFFSETS, offset_vectors

    if X.dim() != 2 or X.shape[1] != be.n0:
        raise ValueError(f"X: expected [N, {be.n0}], got {tuple(X.shape)}")
    N = int(X.shape[0])
    dev = X.device
    npa = len(q.pa_idx)
    if values.dim() != 2 or values.shape[1] != npa:
        raise ValueError(f"values: expected [V, {npa}], got {tuple(values.shape)}")
    V, Pp = int(values.shape[0]), int(pairs.shape[0])
    if not 1 <= V <= MAX_VALUES:
        raise ValueError(f"{what}: {V} PA assignments, the kernel covers 1..{MAX_VALUES}")
    X = _c(X, torch.float32, (N, be.n0), "X")
    own = _c(own, torch.int32, (N,), "own")
    values = _c(values, torch.int64, (V, npa), "values")
    pairs = _c(pairs, torch.int64, (Pp, 2), "pairs")
    if any(t.device != dev for t in (own, values, pairs, be.flat)):
        raise ValueError(f"{what}: X, own, values, pairs and the network must be on one device")
    if Pp and (int(pairs.min()) < 0 or int(pairs.max()) >= V):
        raise ValueError("pairs: index outside [0, V)")
    if N:
        omin, omax = torch.stack(torch.aminmax(own)).tolist()           # one read-back
        if omin < -1 or omax >= V:
            raise ValueError("own: index outside [-1, V)")
    E = int(offset_vectors(q).shape[0])                    # raises over MAX_OFFSETS
    assert E <= MAX_OFFSETS
    return (X, own, values, pairs), (N, V, Pp, E)


_RATE_BLOCKS = 1024      # workgroups a short partition list is spread over (4 per CU)
_RATE_EMPTY = 0x7FFFFFFF


def rate_split_max(n_samples: int) -> int:
    """Largest workgroups-per-partition value of ``fa_rate_kernel``: one per 64-profile pass."""
    return max(1, (n_samples + 63) // 64)


def _rate_split(P: int, n_samples: int) -> int:
    if not P or P >= _RATE_BLOCKS:
        return 1
    return max(1, min(rate_split_max(n_samples), _RATE_BLOCKS // P))


def rate_counts(be, q, lo, hi, pids, n_samples, seed, values, pairs, split: Optional[int] = None):
    """Discrimination-rate counts of ``P`` partitions in one fused launch (``fa_rate_kernel``,
    definitions in ops/rate.py): (certain profiles [P], ambiguous profiles [P], ambiguous sample
    indices [P, 32]) int32.  An index row is sorted ascending and padded with INT32_MAX; the row of
    a partition with more than 32 ambiguous profiles is not trusted and returned all padding.
    ``split``: workgroups per partition (default: by the list length); every value gives the same
    outputs."""
    from .rate import AMB_SLOTS, MAX_OFFSETS, offset_vectors

    P, n0 = lo.shape
    dev = lo.device
    if n0 != be.n0:
        raise ValueError(f"lo: expected [P, {be.n0}], got {tuple(lo.shape)}")
    npa = len(q.pa_idx)
    if values.dim() != 2 or values.shape[1] != npa:
        raise ValueError(f"values: expected [V, {npa}], got {tuple(values.shape)}")
    V = int(values.shape[0])
    Pp = int(pairs.shape[0])
    kw, t = _query_kw(be, q, lo, hi, pids, values, pairs)
    pairs_c = t["pairs"]
    if not 1 <= V <= 32:
        raise ValueError(f"rate: {V} PA assignments, the kernel covers 1..32")
    if Pp and (int(pairs_c.min()) < 0 or int(pairs_c.max()) >= V):
        raise ValueError("pairs: index outside [0, V)")
    E = int(offset_vectors(q).shape[0])                    # raises over MAX_OFFSETS
    assert E <= MAX_OFFSETS
    n_samples = int(n_samples)
    if n_samples < 0 or n_samples >= _RATE_EMPTY:
        raise ValueError(f"rate: bad sample count {n_samples}")
    if not _rowfwd_covers(be):
        raise ValueError("rate: the kernel covers layers up to 160 wide and up to 32 inputs")
    if split is None:
        split = _rate_split(P, n_samples)
    if not 1 <= int(split) <= rate_split_max(n_samples):
        raise ValueError(f"rate: split {split} outside 1..{rate_split_max(n_samples)}")
    flips = torch.zeros(P, dtype=torch.int32, device=dev)
    amb = torch.zeros(P, dtype=torch.int32, device=dev)
    idx = torch.full((P, AMB_SLOTS), _RATE_EMPTY, dtype=torch.int32, device=dev)
    if P and n_samples:
        ext().rate(_net(be), **kw, **_ptrs(flips=flips, amb=amb, amb_idx=idx), n_samples=n_samples,
                   seed=int(seed) & 0xFFFFFFFF, E=E, split=int(split))
        # slots are taken in atomic order: canonical form, and nothing from an overflowed row
        idx = idx.masked_fill((amb > AMB_SLOTS)[:, None], _RATE_EMPTY).sort(dim=1).values
    return flips, amb, idx


_AUDIT_BLOCKS = 1024     # workgroups a long table of rows is walked by (4 per CU); W is staged once each


def audit_passes(N: int) -> int:
    """64-row passes of ``fa_audit_kernel``: the largest workgroup count."""
    return max(1, (int(N) + 63) // 64)


def audit_masks(be, q, X, own, values, pairs, blocks: Optional[int] = None):
    """Per-row audit masks of rows ``X`` [N, n0] in one fused launch (``fa_audit_kernel``, definitions
    in ops/audit.py): (cert int32 [N], poss int32 [N], own_sign int8 [N]), or ``None`` when the kernel
    does not cover the shape (a layer over 160 wide, over 32 inputs, more than 64 KB of LDS): the
    caller takes ``ops/audit.audit_masks_ref``.  ``blocks``: workgroups (default: one per 64-row
    pass, at most 1 024); every value gives the same outputs."""
    (X, own, values, pairs), (N, V, Pp, E) = _row_inputs(be, q, X, own, values, pairs, "audit")
    dev = X.device
    if blocks is None:
        blocks = min(audit_passes(N), _AUDIT_BLOCKS)
    if not 1 <= int(blocks) <= audit_passes(N):
        raise ValueError(f"audit: {blocks} workgroups outside 1..{audit_passes(N)}")
    cert = torch.zeros(N, dtype=torch.int32, device=dev)
    poss = torch.zeros(N, dtype=torch.int32, device=dev)
    sign = torch.zeros(N, dtype=torch.int8, device=dev)
    if not _rowfwd_covers(be):
        return None
    if N:
        ok = ext().audit(_net(be), **_ptrs(flat=be.flat, x=X, own=own, values=values, pairs=pairs if Pp else None,
                                           cert=cert, poss=poss, own_sign=sign),
                         N=N, V=V, Pp=Pp, **_pairs_kw(q, E), blocks=int(blocks), stream=_stream(dev))
        if not ok:
            return None
    return cert, poss, sign


def neighbours_fused() -> bool:
    """``FAIRIFY_NEIGHBOURS_FUSED=0`` (read per call) sends ``engine/neighbours.py`` down the composed
    path -- the audit kernel fed materialised neighbours -- for A/B runs; anything else the fused kernel."""
    return os.environ.get("FAIRIFY_NEIGHBOURS_FUSED", "1").strip() != "0"


def neighbour_items(N: int, M: int) -> int:
    """(64-row pass, word) work items of ``fa_neighbour_kernel``: the largest workgroup count."""
    return audit_passes(N) * max(1, (int(M) + 31) // 32)


def neighbour_masks(be, q, X, own, values, pairs, table, radii=None, blocks: Optional[int] = None):
    """Per-(row, neighbour) bits of rows ``X`` [N, n0] in one fused launch (``fa_neighbour_kernel``,
    definitions in ops/neighbours.py): (cert, poss) int32 [N, W], or ``None`` when the kernel does not
    cover the shape (the audit kernel's conditions): the caller takes
    ``ops/neighbours.neighbour_masks_ref``.  ``table``: an ``ops/neighbours.NeighbourTable``;
    ``radii``: [n0] per-feature radii (default: the table's).  ``blocks``: workgroups (default: one
    per work item, at most 1 024); every value gives the same outputs."""
    from .neighbours import FULL, MAX_NEIGHBOURS

    (X, own, values, pairs), (N, V, Pp, E) = _row_inputs(be, q, X, own, values, pairs, "neighbours")
    dev = X.device
    M, W = table.M, table.W
    if M > MAX_NEIGHBOURS:
        raise ValueError(f"neighbours: {M} table entries, at most {MAX_NEIGHBOURS}")
    radii = table.radius if radii is None else np.asarray(radii, dtype=np.int64)
    if radii.shape != (be.n0,) or table.lo.shape != (be.n0,) or table.hi.shape != (be.n0,):
        raise ValueError(f"neighbours: radii and the domain range must have {be.n0} entries")
    if radii.min(initial=0) < 0 or radii.max(initial=0) > FULL:
        raise ValueError(f"neighbours: radius outside 0..{FULL}")
    if M and (int(table.dim.min()) < 0 or int(table.dim.max()) >= be.n0 or set(table.dim.tolist()) & set(q.pa_idx)):
        raise ValueError("neighbours: table dimension outside the non-PA inputs")
    if blocks is None:
        blocks = min(neighbour_items(N, M), _AUDIT_BLOCKS)
    if not 1 <= int(blocks) <= neighbour_items(N, M):
        raise ValueError(f"neighbours: {blocks} workgroups outside 1..{neighbour_items(N, M)}")
    cert = torch.zeros(N, W, dtype=torch.int32, device=dev)
    poss = torch.zeros(N, W, dtype=torch.int32, device=dev)
    if not _rowfwd_covers(be):
        return None
    if N and M:
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).clip(-FULL - 1, FULL)
                                         .astype(np.int32)).to(dev)
        tabs = dict(nb_dim=i32(table.dim), nb_off=i32(table.off), nb_abs=i32(table.abs), dom_lo=i32(table.lo),
                    dom_hi=i32(table.hi), radius=i32(radii))
        ok = ext().neighbours(_net(be), **_ptrs(flat=be.flat, x=X, own=own, values=values,
                                                pairs=pairs if Pp else None, cert=cert, poss=poss, **tabs),
                              N=N, V=V, Pp=Pp, **_pairs_kw(q, E), M=M, W=W, blocks=int(blocks), stream=_stream(dev))
        if not ok:
            return None
    return cert, poss


def causal_fused() -> bool:
    """``FAIRIFY_CAUSAL_FUSED=0`` (read per call) sends ``engine/causal.py`` down the composed path --
    ``point_bounds`` fed materialised altered rows -- for A/B runs; anything else the fused kernel,
    the default on the shapes it covers (profiles/r20/causal/README.md)."""
    return os.environ.get("FAIRIFY_CAUSAL_FUSED", "1").strip() != "0"


def causal_items(S: int, T: int) -> int:
    """(64-row pass, attribute set) work items of ``fa_causal_kernel``: the largest workgroup count."""
    return audit_passes(S) * max(1, int(T))


def causal_codes(be, X, table, blocks: Optional[int] = None):
    """Per-(base row, attribute set) bytes of rows ``X`` [S, n0] in one fused launch
    (``fa_causal_kernel``, definitions in ops/causal.py): ``code`` uint8 [S, T] in the table's set
    order, or ``None`` when the kernel does not cover the shape (a layer over 160 wide, over 32
    inputs, more than 64 KB of LDS): the caller takes ``ops/causal.causal_codes_ref``.  ``table``: an
    ``ops/causal.SetTable``.  ``blocks``: workgroups (default: one per work item, at most 1 024);
    every value gives the same bytes.  The sets are launched by descending ``A_t``, so that the long
    items start first."""
    from .causal import MAX_DIMS, MAX_VALUE

    if X.dim() != 2 or X.shape[1] != be.n0:
        raise ValueError(f"X: expected [S, {be.n0}], got {tuple(X.shape)}")
    S, T = int(X.shape[0]), table.T
    dev = X.device
    X = _c(X, torch.float32, (S, be.n0), "X")
    if be.flat.device != dev:
        raise ValueError("causal: X and the network must be on one device")
    dims = np.ascontiguousarray(table.dims, dtype=np.int32)
    vals = np.ascontiguousarray(table.vals, dtype=np.int32)
    voff = np.ascontiguousarray(table.voff, dtype=np.int32)
    if dims.ndim != 2 or dims.shape[1] != MAX_DIMS:
        raise ValueError(f"causal: dims must be [T, {MAX_DIMS}], got {dims.shape}")
    if voff.shape != (be.n0 + 1,) or voff[0] != 0 or voff[-1] != vals.size or (np.diff(voff) < 1).any():
        raise ValueError(f"causal: voff must hold {be.n0 + 1} increasing offsets spanning vals")
    if vals.size and int(np.abs(vals.astype(np.int64)).max()) > MAX_VALUE:
        raise ValueError("causal: a value beyond +-2^24 (not exact in fp32)")
    for t in range(T):
        s = [int(d) for d in dims[t] if d != -1]
        if not s or s != [int(d) for d in dims[t, :len(s)]] or any(not 0 <= d < be.n0 for d in s) \
                or any(b <= a for a, b in zip(s, s[1:])):
            raise ValueError(f"causal: set {dims[t].tolist()} is not a strictly increasing tuple padded with -1")
    if blocks is None:
        blocks = min(causal_items(S, T), _AUDIT_BLOCKS)
    if not 1 <= int(blocks) <= causal_items(S, T):
        raise ValueError(f"causal: {blocks} workgroups outside 1..{causal_items(S, T)}")
    code = torch.zeros(S, T, dtype=torch.uint8, device=dev)
    if not _rowfwd_covers(be):
        return None
    if S and T:
        order = np.argsort(-table.count.astype(np.int64), kind="stable")
        ld = np.ascontiguousarray(dims[order])
        out = torch.zeros(S, T, dtype=torch.uint8, device=dev)
        tabs = dict(dims=torch.from_numpy(ld).to(dev), vals=torch.from_numpy(vals).to(dev),
                    voff=torch.from_numpy(voff).to(dev))
        ok = ext().causal(_net(be), **_ptrs(flat=be.flat, x=X, code=out, **tabs),
                          S=S, T=T, D=MAX_DIMS, nvals=int(vals.size), set_dims=ld.reshape(-1).tolist(),
                          value_off=voff.tolist(), blocks=int(blocks), stream=_stream(dev))
        if not ok:
            return None
        code[:, torch.from_numpy(order).to(dev)] = out
    return code


# Workgroups of a leaf list: at least 1 024 (4 per CU), and enough that a workgroup enumerates about
# _ENUM_POINTS points per staging of W -- leaves of 1 000 points measured 4 - 13 % faster one per
# workgroup than eight per workgroup (profiles/r12/count/README.md); only small leaves share a workgroup
_ENUM_BLOCKS = 1024
_ENUM_POINTS = 1024


def _count_shape(be, q, values, pairs, what):
    """Launch-shape checks of the counting kernels; returns (V, Pp, E)."""
    from .rate import offset_vectors

    npa = len(q.pa_idx)
    if values.dim() != 2 or values.shape[1] != npa:
        raise ValueError(f"values: expected [V, {npa}], got {tuple(values.shape)}")
    V, Pp = int(values.shape[0]), int(pairs.shape[0])
    if not 1 <= V <= 32:
        raise ValueError(f"{what}: {V} PA assignments, the kernels cover 1..32")
    if Pp and (int(pairs.min()) < 0 or int(pairs.max()) >= V):
        raise ValueError("pairs: index outside [0, V)")
    E = int(offset_vectors(q).shape[0])                    # raises over MAX_OFFSETS
    return V, Pp, E


def count_enum(be, q, lo, hi, values, pairs, max_vol: Optional[int] = None, blocks: Optional[int] = None):
    """Leaf enumeration in one launch (``fa_count_enum_kernel``, definitions in ops/count.py):
    (certain points [L], ambiguous points [L], ambiguous point indices [L, 32]) int32.  An index row
    is sorted ascending and padded with INT32_MAX; the row of a leaf with more than 32 ambiguous
    points is returned all padding.  ``max_vol``: the caller's bound of the leaves' volumes
    (default: computed from the boxes); ``blocks``: workgroups (every value gives the same outputs)."""
    from .count import MAX_LEAF_POINTS, free_dims, volumes
    from .rate import AMB_SLOTS

    L, n0 = lo.shape
    dev = lo.device
    if n0 != be.n0:
        raise ValueError(f"lo: expected [L, {be.n0}], got {tuple(lo.shape)}")
    lo = _c(lo, torch.float32, (L, n0), "lo")
    hi = _c(hi, torch.float32, (L, n0), "hi")
    values = _c(values, torch.int64, None, "values")
    pairs = _c(pairs, torch.int64, (pairs.shape[0], 2), "pairs")
    V, Pp, E = _count_shape(be, q, values, pairs, "count_enum")
    if not _rowfwd_covers(be):
        raise ValueError("count_enum: the kernel covers layers up to 160 wide and up to 32 inputs")
    if max_vol is None:
        max_vol = int(volumes(lo, hi, free_dims(q)).max()) if L else 1
    if not 1 <= int(max_vol) <= MAX_LEAF_POINTS:
        raise ValueError(f"count_enum: leaf volume {max_vol} outside 1..{MAX_LEAF_POINTS}")
    if blocks is None:
        blocks = min(max(L, 1), max(_ENUM_BLOCKS, L * int(max_vol) // _ENUM_POINTS))
    if L and not 1 <= int(blocks) <= L:
        raise ValueError(f"count_enum: {blocks} workgroups outside 1..{L}")
    cert = torch.zeros(L, dtype=torch.int32, device=dev)
    amb = torch.zeros(L, dtype=torch.int32, device=dev)
    idx = torch.full((L, AMB_SLOTS), _RATE_EMPTY, dtype=torch.int32, device=dev)
    if L:
        ext().count_enum(_net(be), **_ptrs(flat=be.flat, lo=lo, hi=hi, values=values, pairs=pairs if Pp else None,
                                           cert=cert, amb=amb, amb_idx=idx),
                         L=L, V=V, Pp=Pp, **_pairs_kw(q, E), max_vol=int(max_vol), blocks=int(blocks),
                         stream=_stream(dev))
        idx = idx.masked_fill((amb > AMB_SLOTS)[:, None], _RATE_EMPTY).sort(dim=1).values
    return cert, amb, idx


def gap_fused() -> bool:
    """``FAIRIFY_GAP_FUSED=1`` (read per call) makes ``engine/gap.py`` run the level step and the
    leaf enumeration on the kernels of csrc/gap.hip where they cover the shape; ``0`` or unset takes
    the composed path -- ``ops/gap.level_ref``, materialised leaf points, ``point_bounds`` and the
    torch reduction.  Opt-in: the kernel is 5 - 17 times faster on
    the leaves alone, but the whole call gained 2 - 7 % in the median, inside its spread
    (profiles/r21/gap/README.md)."""
    return os.environ.get("FAIRIFY_GAP_FUSED", "0").strip() == "1"


def gap_enum(be, q, lo, hi, values, pairs, max_vol: Optional[int] = None, blocks: Optional[int] = None):
    """Score-gap leaf enumeration in one launch (``fa_gap_enum_kernel``, definitions in ops/gap.py):
    (``leaf_lo`` [L] fp64, ``leaf_hi`` [L] fp64, ``arg_s``, ``arg_pair``, ``arg_e`` [L] int32), or
    ``None`` when the kernel does not cover the shape (a layer over 160 wide, over 32 inputs, more
    than 64 KB of LDS): the caller takes ``ops/gap.enum_gap_ref``.  ``max_vol``: the caller's bound of
    the leaves' volumes (default: computed from the boxes; a leaf over it gets ``arg_s = -2``);
    ``blocks``: workgroups (every value gives the same outputs)."""
    from .count import MAX_LEAF_POINTS, free_dims, volumes

    L, n0 = lo.shape
    dev = lo.device
    if n0 != be.n0:
        raise ValueError(f"lo: expected [L, {be.n0}], got {tuple(lo.shape)}")
    lo = _c(lo, torch.float32, (L, n0), "lo")
    hi = _c(hi, torch.float32, (L, n0), "hi")
    values = _c(values, torch.int64, None, "values")
    pairs = _c(pairs, torch.int64, (pairs.shape[0], 2), "pairs")
    V, Pp, E = _count_shape(be, q, values, pairs, "gap_enum")
    if Pp < 1:
        raise ValueError("gap_enum: no pair")
    if max_vol is None:
        max_vol = int(volumes(lo, hi, free_dims(q)).max()) if L else 1
    if not 1 <= int(max_vol) <= MAX_LEAF_POINTS:
        raise ValueError(f"gap_enum: leaf volume {max_vol} outside 1..{MAX_LEAF_POINTS}")
    if blocks is None:
        blocks = min(max(L, 1), max(_ENUM_BLOCKS, L * int(max_vol) // _ENUM_POINTS))
    if L and not 1 <= int(blocks) <= L:
        raise ValueError(f"gap_enum: {blocks} workgroups outside 1..{L}")
    if not _rowfwd_covers(be):
        return None
    leaf_lo = torch.zeros(L, dtype=torch.float64, device=dev)
    leaf_hi = torch.zeros(L, dtype=torch.float64, device=dev)
    arg = torch.full((3, L), -1, dtype=torch.int32, device=dev)
    if L:
        ok = ext().gap_enum(_net(be), **_ptrs(flat=be.flat, lo=lo, hi=hi, values=values, pairs=pairs, leaf_lo=leaf_lo,
                                              leaf_hi=leaf_hi, arg_s=arg[0], arg_pair=arg[1], arg_e=arg[2]),
                            L=L, V=V, Pp=Pp, **_pairs_kw(q, E), max_vol=int(max_vol), blocks=int(blocks),
                            stream=_stream(dev))
        if not ok:
            return None
    return leaf_lo, leaf_hi, arg[0], arg[1], arg[2]


def gap_level(be, q, lo, hi, part, rx, rp, values, pairs, thr, score, leaf_points):
    """Level step of the score-gap search over ``N`` nodes (``fa_gap_level_kernel``, definitions in
    ops/gap.py) from the bound results ``rx`` / ``rp`` of the node rows [N V]: returns ``None`` when
    the kernel does not cover the shape (over 32 inputs or PA assignments, no pair), else a dict with
    ``ub`` [N] fp32, ``code`` [N] uint8, ``pair``, ``orient``, ``sdim`` [N] int32, ``c``, ``cand_x``,
    ``cand_xp`` [N, n0], the child pool ``kids = (clo, chi, cpart, cub, ckey)`` (capacity 2 N), the
    leaf list ``leaves = (llo, lhi, lpart, lkey)`` (capacity N) and ``counters`` [3] int32 on the
    device (children, leaves, nodes that did not fit).  The lists are filled up to the counters in
    atomic order; the keys (``2 k``, ``2 k + 1`` for the children of node ``k``, ``k`` for a leaf)
    restore the node order.  ``thr`` [P] fp64: ``inc_start + tol``.  ``pairs`` is not
    range-checked here (no synchronisation per launch): the kernel skips an index outside [0, V)."""
    N, n0 = lo.shape
    dev = lo.device
    V, Pp = int(values.shape[0]), int(pairs.shape[0])
    if n0 > 32 or not 1 <= V <= 32 or Pp < 1:
        return None
    lo = _c(lo, torch.float32, (N, n0), "lo")
    hi = _c(hi, torch.float32, (N, n0), "hi")
    part = _c(part, torch.int32, (N,), "part")
    vals = _c(values, torch.float32, (V, len(q.pa_idx)), "values")
    pairs = _c(pairs, torch.int64, (Pp, 2), "pairs")
    thr = _c(thr, torch.float64, None, "thr")
    score = _c(score.to(dev), torch.float32, (n0,), "score")
    forms = {}
    for r, sfx in ((rx, ""), (rp, "p")):
        for name, t, shape in (("Lc", r.Lc, (N * V, n0)), ("L0", r.L0, (N * V,)), ("Le", r.Le, (N * V,)),
                               ("Uc", r.Uc, (N * V, n0)), ("U0", r.U0, (N * V,)), ("Ue", r.Ue, (N * V,)),
                               ("lb", r.out_lb, (N * V,)), ("ub", r.out_ub, (N * V,))):
            forms[name + sfx] = _c(t, torch.float32, shape, name + sfx)
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(ub=torch.empty(N, **f32), code=torch.empty(N, dtype=torch.uint8, device=dev), pair=torch.empty(N, **i32),
               orient=torch.empty(N, **i32), sdim=torch.empty(N, **i32), c=torch.zeros(N, n0, **f32),
               cand_x=torch.empty(N, n0, **f32), cand_xp=torch.empty(N, n0, **f32))
    kids = (torch.empty(2 * N, n0, **f32), torch.empty(2 * N, n0, **f32), torch.empty(2 * N, **i32),
            torch.empty(2 * N, **f32), torch.empty(2 * N, **i32))
    leaves = (torch.empty(N, n0, **f32), torch.empty(N, n0, **f32), torch.empty(N, **i32), torch.empty(N, **i32))
    counters = torch.zeros(3, **i32)
    if N:
        ok = ext().gap_level(**_ptrs(lo=lo, hi=hi, part=part, values=vals, pairs=pairs, thr=thr, score=score,
                                     out_ub=out["ub"], code=out["code"], best_pair=out["pair"], orient=out["orient"],
                                     sdim=out["sdim"], coef=out["c"], cand_x=out["cand_x"], cand_xp=out["cand_xp"],
                                     olo=kids[0], ohi=kids[1], opart=kids[2], oub=kids[3], okey=kids[4],
                                     leaf_lo=leaves[0], leaf_hi=leaves[1], leaf_part=leaves[2], leaf_key=leaves[3],
                                     counters=counters, **forms),
                             N=N, n0=n0, V=V, pa=list(q.pa_idx), ra=list(q.ra_idx) if q.relaxed else [],
                             tau=float(q.tau) if q.relaxed else 0.0, Pp=Pp, leaf_points=int(leaf_points), cap=2 * N,
                             leaf_cap=N, stream=_stream(dev))
        if not ok:
            return None
    out.update(kids=kids, leaves=leaves, counters=counters)
    return out


def count_rows(be, q, lo, hi, values):
    """Node boxes [N, n0] -> x rows ``rlo, rhi`` [N V, n0] and counterpart rows ``plo, phi`` (the x
    rows themselves for a PA-only query) via ``fa_count_rows_kernel`` (ops/count.py:node_rows)."""
    N, n0 = lo.shape
    dev = lo.device
    lo = _c(lo, torch.float32, (N, n0), "lo")
    hi = _c(hi, torch.float32, (N, n0), "hi")
    npa = len(q.pa_idx)
    values = _c(values, torch.float32, None, "values")
    if values.dim() != 2 or values.shape[1] != npa or values.shape[0] < 1:
        raise ValueError(f"values: expected [V, {npa}], got {tuple(values.shape)}")
    if any(not 0 <= d < n0 for d in list(q.pa_idx) + list(q.ra_idx)):
        raise ValueError("count_rows: PA / RA dim outside the inputs")
    V = int(values.shape[0])
    f32 = dict(dtype=torch.float32, device=dev)
    rlo, rhi = torch.empty(N * V, n0, **f32), torch.empty(N * V, n0, **f32)
    plo = phi = None
    if q.relaxed:
        plo, phi = torch.empty(N * V, n0, **f32), torch.empty(N * V, n0, **f32)
    if N:
        ext().count_rows(**_ptrs(lo=lo, hi=hi, values=values, rlo=rlo, rhi=rhi, plo=plo, phi=phi), N=N, n0=n0, V=V,
                         pa=list(q.pa_idx), ra=list(q.ra_idx) if q.relaxed else [],
                         tau=float(q.tau) if q.relaxed else 0.0, stream=_stream(dev))
    return (rlo, rhi, plo, phi) if q.relaxed else (rlo, rhi, rlo, rhi)


def count_level(be, q, lo, hi, part, lx, ux, lxp, uxp, pairs, score, leaf_points, fair, unfair, child_cnt,
                part_checked: bool = False):
    """Level step of the counting branch-and-bound over ``N`` nodes (``fa_count_level_kernel``):
    box test, volumes of the FAIR / UNFAIR nodes added to ``fair`` / ``unfair`` [P] int64, children
    counted into ``child_cnt`` [P] int32.  Returns (class codes [N] uint8, child pool ``clo, chi``
    [2 N, n0] and ``cpart`` [2 N], leaf list ``llo, lhi`` [N, n0] and ``lpart`` [N], counters [3]
    int32 on the device: children, leaves, nodes that did not fit); the lists are filled up to the
    counters, in atomic order.  ``part_checked``: the caller vouches for ``part`` in [0, P) (the level
    loop's pools come from this kernel; checking them would cost a synchronisation per slice)."""
    N, n0 = lo.shape
    dev = lo.device
    lo = _c(lo, torch.float32, (N, n0), "lo")
    hi = _c(hi, torch.float32, (N, n0), "hi")
    part = _c(part, torch.int32, (N,), "part")
    V = lx.numel() // max(N, 1)
    t = {k: _c(v, torch.float32, (N * V,), k) for k, v in dict(lx=lx.reshape(-1), ux=ux.reshape(-1),
                                                                lxp=lxp.reshape(-1), uxp=uxp.reshape(-1)).items()}
    pairs = _c(pairs, torch.int64, (pairs.shape[0], 2), "pairs")
    Pp = int(pairs.shape[0])
    score = _c(score.to(dev), torch.float32, (n0,), "score")
    P = fair.shape[0]
    for name, x, dt in (("fair", fair, torch.int64), ("unfair", unfair, torch.int64), ("child_cnt", child_cnt, torch.int32)):
        if x.dtype != dt or tuple(x.shape) != (P,) or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"{name}: expected a contiguous [{P}] {dt} tensor on {dev}")
    if N and not part_checked and (int(part.min()) < 0 or int(part.max()) >= P):
        raise ValueError("part: partition index outside [0, P)")
    if N and V < 1:
        raise ValueError("count_level: no rows")
    if any(not 0 <= d < n0 for d in q.pa_idx):
        raise ValueError("count_level: PA dim outside the inputs")
    if not 1 <= int(leaf_points) < 2 ** 62:
        raise ValueError(f"count_level: bad leaf size {leaf_points}")
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    code = torch.empty(N, dtype=torch.uint8, device=dev)
    clo, chi, cpart = torch.empty(2 * N, n0, **f32), torch.empty(2 * N, n0, **f32), torch.empty(2 * N, **i32)
    llo, lhi, lpart = torch.empty(N, n0, **f32), torch.empty(N, n0, **f32), torch.empty(N, **i32)
    counters = torch.zeros(3, **i32)
    if N:
        ext().count_level(**_ptrs(lo=lo, hi=hi, part=part, pairs=pairs if Pp else None, score=score, code=code,
                                  fair=fair, unfair=unfair, child_cnt=child_cnt, olo=clo, ohi=chi, opart=cpart,
                                  leaf_lo=llo, leaf_hi=lhi, leaf_part=lpart, counters=counters, **t),
                          N=N, n0=n0, V=V, pa=list(q.pa_idx), Pp=Pp, leaf_points=int(leaf_points), cap=2 * N,
                          leaf_cap=N, stream=_stream(dev))
    return code, (clo, chi, cpart), (llo, lhi, lpart), counters


def ascent(be, q, lo, hi, x0, f0, q0, iters, values, pairs, free_dims):
    """Lattice coordinate ascent of the residual falsifier in one launch (``fa_ascent_kernel``).

    ``x0`` [P, K, n0] start points, ``f0`` [P, K] their margins, ``q0`` [P, K] pair indices.
    Returns ``(found [P] bool, wit_x [P, n0], wit_xp [P, n0])``, or ``None`` when one partition's
    candidate rows do not fit in LDS (the caller then runs the PyTorch loop)."""
    P, K, n0 = x0.shape
    dev = x0.device
    if tuple(lo.shape) != (P, n0):
        raise ValueError(f"lo: expected shape {(P, n0)}, got {tuple(lo.shape)}")
    kw, _keep = _query_kw(be, q, lo, hi, None, values, pairs)
    x0_c = _c(x0, torch.float32, (P, K, n0), "x0")
    f0_c = _c(f0, torch.float32, (P, K), "f0")
    q0_c = _c(q0, torch.int32, (P, K), "q0")
    found = torch.zeros(P, dtype=torch.uint8, device=dev)
    wx = torch.zeros(P, n0, dtype=torch.float32, device=dev)
    wxp = torch.zeros(P, n0, dtype=torch.float32, device=dev)
    if P == 0:
        return found.bool(), wx, wxp
    ok = ext().ascent(_net(be), **kw, **_ptrs(x0=x0_c, f0=f0_c, q0=q0_c, found=found, wit_x=wx, wit_xp=wxp), K=K,
                      iters=int(iters), free=[int(d) for d in free_dims])
    if not ok:
        return None
    return found.bool(), wx, wxp


def falsify(be, q, lo, hi, pids, values, pairs, seed, n_samples, n_local, walk_k, walk_steps, k_starts, iters,
            free_dims, dseed: int = 0):
    """Fused residual falsifier (``csrc/falsify.hip``): heavy sampling, boundary walk, lattice
    coordinate ascent in one launch.  Relaxed queries: x' carries RA offsets in [-tau, tau] (hash
    stream ``dseed`` per sample, moved by the ascent), both orientations of every pair count.
    Returns ``(found [P] bool, wit_x [P, n0], wit_xp [P, n0], how [P] int8)`` or ``None`` when the
    network shape is not supported by the kernel (the caller keeps the PyTorch path)."""
    P, n0 = lo.shape
    dev = lo.device
    Pp = pairs.shape[0]
    kw, t = _query_kw(be, q, lo, hi, pids, values, pairs)
    if t["values"].numel() != kw["V"] * len(q.pa_idx):
        raise ValueError("values: expected [V, n_pa]")
    found = torch.zeros(P, dtype=torch.uint8, device=dev)
    wx = torch.zeros(P, n0, dtype=torch.float32, device=dev)
    wxp = torch.zeros(P, n0, dtype=torch.float32, device=dev)
    how = torch.zeros(P, dtype=torch.int8, device=dev)
    if P == 0 or Pp == 0 or n_samples <= 0:
        return found.bool(), wx, wxp, how
    ok = ext().falsify(_net(be), **kw, **_ptrs(found=found, wit_x=wx, wit_xp=wxp, how=how), n_samples=int(n_samples),
                       n_local=int(n_local), seed=int(seed) & 0xFFFFFFFF, walk_k=int(walk_k),
                       walk_steps=int(walk_steps), K=int(k_starts), iters=int(iters),
                       free=[int(d) for d in free_dims], dseed=int(dseed) & 0xFFFFFFFF)
    if not ok:
        return None
    return found.bool(), wx, wxp, how


# ------------------------------------------------------------------------------------------------
def prune_masks(be, counts: torch.Tensor, lay_ub: torch.Tensor, sym_dead: Optional[torch.Tensor]):
    """Sound-prune mask algebra of the pipeline's stage 2 in one launch (``csrc/prune.hip``).

    ``counts`` [P, N] int32 simulation activation counts, ``lay_ub`` [P, N] IBP upper bounds,
    ``sym_dead`` [P, N_hidden] uint8 symbolic stable-inactive flags (or None).  Returns
    ``(code [P, N] uint8, cnt [P, 3] int32)``: per neuron bit 0 candidate, 1 bound-dead, 2
    symbolic-dead, 3 merged sound dead, 4 symbolic candidate; per partition the B/S/ST dead
    counts."""
    P, N = counts.shape
    dev = counts.device
    counts_c = _c(counts, torch.int32, (P, be.mlp.n_neurons), "counts")
    ub_c = _c(lay_ub, torch.float32, (P, N), "lay_ub")
    sd = None
    if sym_dead is not None:
        sd = _c(sym_dead, torch.uint8, (P, be.n_hidden), "sym_dead")
    code = torch.empty(P, N, dtype=torch.uint8, device=dev)
    cnt = torch.empty(P, 3, dtype=torch.int32, device=dev)
    if P:
        ext().prune_masks(_net(be), P, counts_c.data_ptr(), ub_c.data_ptr(), N, _ptr(sd), code.data_ptr(),
                          cnt.data_ptr(), _stream(dev))
    return code, cnt


PM_CAND, PM_B, PM_S, PM_ST, PM_SCAND = 1, 2, 4, 8, 16


def heuristic(be, rows: torch.Tensor, lay_lb: torch.Tensor, lay_ub: torch.Tensor, code: torch.Tensor, perc: float):
    """The reference's heuristic pruning (utils/prune.py:862-939) for partitions ``rows`` of the
    stage-2 arrays, one wave per partition (K5).  Returns ``(new [Pu, N] uint8, merged [Pu, N]
    uint8, cnt [Pu, 2] int32 = (#new, #merged))``."""
    Pu = rows.shape[0]
    P, N = lay_ub.shape
    dev = lay_ub.device
    rows_c = _c(rows, torch.int64, (Pu,), "rows")
    lb_c = _c(lay_lb, torch.float32, (P, N), "lay_lb")
    ub_c = _c(lay_ub, torch.float32, (P, N), "lay_ub")
    code_c = _c(code, torch.uint8, (P, N), "code")
    hnew = torch.empty(Pu, N, dtype=torch.uint8, device=dev)
    hmerged = torch.empty(Pu, N, dtype=torch.uint8, device=dev)
    cnt = torch.empty(Pu, 2, dtype=torch.int32, device=dev)
    if Pu:
        ext().heuristic(_net(be), Pu, rows_c.data_ptr(), lb_c.data_ptr(), ub_c.data_ptr(), N, code_c.data_ptr(),
                        50.0 / 100.0, float(perc) / 100.0, (100.0 - float(perc)) / 100.0, hnew.data_ptr(),
                        hmerged.data_ptr(), cnt.data_ptr(), _stream(dev))
    return hnew, hmerged, cnt


def agree(be, rows: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, pids: torch.Tensor, dead: torch.Tensor,
          n_samples: int, seed: int):
    """Pruned-acc / Pruned-F1 counts: per partition ``rows[k]``, over its ``n_samples``
    simulation points, (points where the full network and the network with ``dead[k]``
    [N_hidden] forced to zero agree in sign, points positive for both, points positive only for
    the pruned network).  Returns int32 [Pm, 3] or ``None`` (shape unsupported: caller keeps
    PyTorch)."""
    Pm = rows.shape[0]
    P, n0 = lo.shape
    dev = lo.device
    rows_c = _c(rows, torch.int64, (Pm,), "rows")
    lo_c = _c(lo, torch.float32, (P, n0), "lo")
    hi_c = _c(hi, torch.float32, (P, n0), "hi")
    pids_c = _c(pids, torch.int64, (P,), "pids")
    dead_c = _c(dead, torch.uint8, (Pm, be.n_hidden), "dead")
    out = torch.zeros(Pm, 3, dtype=torch.int32, device=dev)
    if Pm == 0:
        return out
    ok = ext().agree(_net(be), be.flat.data_ptr(), Pm, rows_c.data_ptr(), lo_c.data_ptr(), hi_c.data_ptr(),
                     pids_c.data_ptr(), dead_c.data_ptr(), int(n_samples), int(seed) & 0xFFFFFFFF, out.data_ptr(),
                     _stream(dev))
    return out if ok else None


# ------------------------------------------------------------------------------------------------
def _beta_wt(be) -> torch.Tensor:
    """Per layer W_l transposed ([out][in] row-major) at the flat offsets of W_l (csrc/beta.hip's
    backward-operand copy), cached on the backend."""
    wt = getattr(be, "_beta_wt", None)
    if wt is None:
        import numpy as np

        with _LAZY_LOCK:          # built once: native runtimes keep its device pointer for the backend's life
            wt = getattr(be, "_beta_wt", None)
            if wt is None:
                parts = []
                for w, b in zip(be.mlp.weights, be.mlp.biases):
                    parts += [np.ascontiguousarray(np.asarray(w, np.float32).T).reshape(-1),
                              np.zeros(np.size(b), np.float32)]
                wt = torch.from_numpy(np.concatenate(parts)).to(be.device)
                if wt.is_cuda:
                    torch.cuda.current_stream(wt.device).synchronize()   # complete for every stream
                be._beta_wt = wt
    return wt


def beta_batched_fits(be) -> bool:
    """Can the batched optimiser (``fa_beta_opt16_kernel``, csrc/beta_opt16.hip) run this network?
    (hidden widths <= 112, inputs <= 32, a single logit, both operand orders of W within LDS)"""
    return bool(ext().beta_batched_fits(_net(be)))


def _beta_rows(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, rx, osg):
    """The rows of one beta level: ``(keywords, tensors)`` of the ``BetaArgs`` inputs the beta bindings
    share -- node boxes, PA dims and values, partition bounds and phases of both copies, the
    orientations, a relaxed level's ``rx`` tuple as ramask / plo / phi / gtie ([R, 2, n0], the tie's
    multipliers in / out) / tau, R and the stream.  The checked contiguous ``tensors`` (same keys)
    must stay alive until the launch is enqueued."""
    R, n0 = lo.shape
    NH = be.n_hidden
    npa = len(pa)
    t = dict(flat=be.flat, lo=_c(lo, torch.float32, (R, n0), "lo"), hi=_c(hi, torch.float32, (R, n0), "hi"),
             va=_c(va, torch.float32, (R, npa), "va"), vb=_c(vb, torch.float32, (R, npa), "vb"))
    for x, nm in ((LBA, "LBA"), (UBA, "UBA"), (LBB, "LBB"), (UBB, "UBB")):
        t[nm] = _c(x, torch.float32, (R, NH), nm)
    t.update(phA=_c(phA, torch.int8, (R, NH), "phA"), phB=_c(phB, torch.int8, (R, NH), "phB"), plo=None, phi=None,
             gtie=None, osg=None if osg is None else _c(osg, torch.int8, (R,), "osg"))
    ramask, tau = 0, 0.0
    if rx is not None:          # relaxed: copy B's RA dims over [plo, phi]
        for d in torch.nonzero(rx[0].cpu()).flatten().tolist():
            ramask |= 1 << int(d)
        t["plo"] = _c(rx[1], torch.float32, (R, n0), "plo")
        t["phi"] = _c(rx[2], torch.float32, (R, n0), "phi")
        if len(rx) > 3 and rx[4] is not None:       # the tau tie's multipliers (in / out)
            tau = float(rx[3])
            for x, nm in ((rx[4], "gP"), (rx[5], "gM")):
                if tuple(x.shape) != (R, n0) or x.dtype != torch.float32:
                    raise ValueError(f"{nm}: expected float32 [{R}, {n0}]")
            t["gtie"] = torch.stack([rx[4], rx[5]], 1).contiguous()
    kw = dict(_ptrs(**t), R=R, pa=[int(d) for d in pa], ramask=int(ramask), tau=tau, stream=_stream(lo.device))
    return kw, t


def _beta_steps(iters, lr_a, lr_b, lr_t, decay):
    return dict(iters=int(iters), lr_a=float(lr_a), lr_b=float(lr_b), lr_t=float(lr_t), decay=float(decay))


def beta_opt16(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, alA, alB, beA, beB, t, iters, lr_a, lr_b, lr_t,
               decay=1.0, beta_pos=True, rx=None, pgap=0, osg=None):
    """Phase 1 of the batched level alone (``fa_beta_opt16_kernel``): projected Adam on 16 nodes per
    wave.  Nothing is modified in place; returns ``(par [R, 4, NH], t [R], gP, gM ([R, n0] or None),
    pgsum [R, 4, NH], pgn [R])`` -- the best iterate (alpha_A, alpha_B, beta_A, beta_B), its pair
    weight and tie multipliers, and the weighted primal sums (zA, zB, hA, hB) with their weight sum."""
    R, n0 = lo.shape
    NH = be.n_hidden
    dev = lo.device
    if list(pa) != sorted(pa):
        raise ValueError("beta_opt16: PA dims must be increasing")
    if not beta_batched_fits(be):
        raise RuntimeError("fa_beta_opt16_kernel: network not supported by the batched beta optimiser")
    f32 = dict(dtype=torch.float32, device=dev)
    kw, keep = _beta_rows(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, rx, osg)
    for x, nm in ((alA, "alA"), (alB, "alB"), (beA, "beA"), (beB, "beB")):
        if tuple(x.shape) != (R, NH) or x.dtype != torch.float32:
            raise ValueError(f"{nm}: expected float32 [{R}, {NH}]")
    if tuple(t.shape) != (R,) or t.dtype != torch.float32:
        raise ValueError("t: expected float32 [R]")
    par = torch.stack([alA, alB, beA, beB], 1).contiguous()
    t_o = t.clone().contiguous()
    gt = keep["gtie"]
    pgsum = torch.zeros(R, 4, NH, **f32)
    pgn = torch.zeros(R, **f32)
    if R:
        scratch = torch.empty(max(int(ext().beta_opt16_scratch(_net(be), R)), 1), **f32)
        rc = ext().beta_opt16(_net(be), **kw, **_ptrs(par=par, t=t_o, scratch=scratch, pgsum=pgsum, pgn=pgn),
                              **_beta_steps(iters, lr_a, lr_b, lr_t, decay), beta_pos=int(bool(beta_pos)),
                              flags=(int(pgap) & 3) << 1)
        if rc != 0:
            raise RuntimeError(f"fa_beta_opt16_kernel launch failed ({rc})")
    return par, t_o, (None if gt is None else gt[:, 0]), (None if gt is None else gt[:, 1]), pgsum, pgn


def beta_flags(stall, pgap, feas: bool = False) -> int:
    """The flags word of the ``beta_level`` bindings: bit 0 stall, bits 1-2 the primal-gap weights
    (0 .. 3), bit 3 the infeasibility pass.  A ``pgap`` outside 0 .. 3 would spill into the pass's bit
    (and the launch would then leave the main pass's outputs unwritten): it raises."""
    pg = int(pgap)
    if not 0 <= pg <= 3:
        raise ValueError(f"beta: pgap (BetaConfig.pgap_weights) must be 0, 1, 2 or 3, got {pgap!r}")
    return int(bool(stall)) | ((pg & 3) << 1) | (8 if feas else 0)


def _feas_buffers(be, R, n0, NH, tie, batched, dev):
    """(scratch, fpar, fgt) of an infeasibility pass on R rows (fpar / fgt: the two-phase pass only)."""
    f32 = dict(dtype=torch.float32, device=dev)
    nscr = R * 16 * NH
    fpar = fgt = None
    if batched:
        nscr = max(nscr, int(ext().beta_opt16_scratch(_net(be), R)))
        fpar = torch.zeros(R, 4, NH, **f32)
        fgt = torch.zeros(R, 2, n0, **f32) if tie else None
    return torch.empty(max(nscr, 1), **f32), fpar, fgt


def beta_feas(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, alA, alB, t, bound, iters, lr, batched: bool,
              decay=1.0, rx=None, osg=None, proposal=None, return_proposal=False):
    """The infeasibility pass alone (ops/beta.py:feasibility_ref) on rows whose main pass is done:
    ``alA / alB / t`` (and ``rx``'s tie multipliers, which the pass only needs to exist) are the main
    pass's best, ``bound`` [R] float64 its bounds -- rows with ``bound < 0`` and a fixed phase run.
    ``lr`` = (lr_a, lr_b, lr_t).  ``batched`` False: the per-node pass (``fa_beta_kernel``, feas = 1);
    True: the two-phase pass -- proposals by the feas mode of ``fa_beta_opt16_kernel``, 16 nodes per
    wave, then ``fa_beta_kernel`` at iters = 0 decides on its rigorous fp64 value at them.
    ``proposal`` = (fpar [R, 4, NH], fgt [R, 2, n0] or None): the rigorous phase alone on these
    (untrusted) parameters.  Nothing is modified in place.  Returns ``(closed [R] bool, value [R]
    float64)`` -- value NaN on the rows that did not run --, with ``return_proposal`` also
    ``(fpar, fgt)`` as the proposal phase wrote them (zero where it wrote nothing)."""
    R, n0 = lo.shape
    NH = be.n_hidden
    dev = lo.device
    if list(pa) != sorted(pa):
        raise ValueError("beta_feas: PA dims must be increasing")
    two_phase = bool(batched) or proposal is not None
    if two_phase and not beta_batched_fits(be):
        raise RuntimeError("fa_beta_opt16_kernel: network not supported by the batched beta optimiser")
    kw, keep = _beta_rows(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, rx, osg)
    for x, nm in ((alA, "alA"), (alB, "alB")):
        if tuple(x.shape) != (R, NH) or x.dtype != torch.float32:
            raise ValueError(f"{nm}: expected float32 [{R}, {NH}]")
    z = torch.zeros_like(alA)
    par = torch.stack([alA, alB, z, z], 1).contiguous()
    t_c = _c(t, torch.float32, (R,), "t").clone()
    bnd_o = _c(bound, torch.float64, (R,), "bound").clone()
    gt = keep["gtie"]
    fval = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
    scratch, fpar, fgt = _feas_buffers(be, R, n0, NH, gt is not None, two_phase, dev)
    mode = 1 if batched else 0
    if proposal is not None:
        mode = 3
        fpar = _c(proposal[0], torch.float32, (R, 4, NH), "fpar").clone()
        if gt is not None:
            fgt = _c(proposal[1], torch.float32, (R, 2, n0), "fgt").clone()
    if R:
        rc = ext().beta_feas(_net(be), **kw, **_beta_steps(iters, lr[0], lr[1], lr[2], decay), mode=mode,
                             **_ptrs(wt=_beta_wt(be), par=par, t=t_c, scratch=scratch, bound=bnd_o, fpar=fpar, fgt=fgt,
                                     fval=fval))
        if rc != 0:
            raise RuntimeError(f"beta_feas launch failed ({rc})")
    closed = torch.isinf(bnd_o) & (bnd_o > 0) & ~(torch.isinf(bound) & (bound > 0))
    if return_proposal:
        return closed, fval, (fpar, fgt)
    return closed, fval


def beta_level(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, alA, alB, beA, beB, t, iters, lr_a, lr_b, lr_t,
               decay=1.0, lookahead=0, beta_pos=True, rx=None, stall=True, pgap=False, osg=None, feas_iters=0,
               feas_lr=None, batched=False, batched_feas=False):
    """One beta-CROWN BaB level on the device (``fa_beta_kernel``, csrc/beta.hip): the rows'
    (alpha, beta, t) are optimised IN PLACE (kept at the best iterate) and their rigorous fp64
    bounds, branching decisions, concretising vertices and child multipliers returned
    (:class:`ops.beta.BetaLevel`).  ``batched``: the two-phase level -- the optimisation on MFMA, 16
    nodes per wave (csrc/beta_opt16.hip), then this kernel at ``iters = 0`` for the rigorous bound and
    the branching; a network the batched kernel cannot run raises.  ``batched_feas`` (with ``batched``):
    the infeasibility pass in two phases too (:func:`beta_feas`)."""
    from . import beta as B

    flags = beta_flags(stall, pgap)
    batched_feas = bool(batched and batched_feas and feas_iters > 0)

    R, n0 = lo.shape
    NH = be.n_hidden
    dev = lo.device
    if list(pa) != sorted(pa):
        raise ValueError("beta_level: PA dims must be increasing")
    f32 = dict(dtype=torch.float32, device=dev)
    kw, keep = _beta_rows(be, lo, hi, pa, va, vb, LBA, UBA, LBB, UBB, phA, phB, rx, osg)
    gt = keep["gtie"]
    for x, nm in ((alA, "alA"), (alB, "alB"), (beA, "beA"), (beB, "beB")):
        if tuple(x.shape) != (R, NH) or x.dtype != torch.float32:
            raise ValueError(f"{nm}: expected float32 [{R}, {NH}]")
    if tuple(t.shape) != (R,) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("t: expected contiguous float32 [R]")
    par = torch.stack([alA, alB, beA, beB], 1).contiguous()          # [R, 4, NH]
    nscr = R * (16 if feas_iters > 0 else 12) * NH
    pgsum = pgn = None
    if batched:
        if not beta_batched_fits(be):
            raise RuntimeError("fa_beta_opt16_kernel: network not supported by the batched beta optimiser")
        nscr = max(nscr, int(ext().beta_opt16_scratch(_net(be), R)))
        pgsum = torch.empty(R, 4, NH, **f32)
        pgn = torch.empty(R, **f32)
    scratch = torch.empty(max(nscr, 1), **f32)
    fpar = fgt = None
    if batched_feas:
        fpar = torch.empty(R, 4, NH, **f32)
    bound = torch.empty(R, dtype=torch.float64, device=dev)
    split = torch.empty(R, dtype=torch.int32, device=dev)
    xstar = torch.empty(R, n0, **f32)
    binit = torch.empty(R, 2, **f32)
    xpstar = torch.empty(R, n0, **f32)
    if batched_feas and gt is not None:
        fgt = torch.empty(R, 2, n0, **f32)
    if R:
        net = _net(be)
        kw.update(_ptrs(wt=_beta_wt(be), par=par, t=t, scratch=scratch, bound=bound, split=split, xstar=xstar,
                        binit=binit, xpstar=xpstar),
                  **_beta_steps(iters, lr_a, lr_b, lr_t, decay), lookahead=int(lookahead),
                  beta_pos=int(bool(beta_pos)), flags=flags)
        if batched:
            rc = ext().beta_level16(net, **kw, **_ptrs(pgsum=pgsum, pgn=pgn))
        else:
            rc = ext().beta_level(net, **kw)
        if rc == 0 and feas_iters > 0:
            # the infeasibility pass on the nodes left open: only their bounds can change
            fkw = {**kw, **_beta_steps(feas_iters, *(feas_lr or (lr_a, lr_b, lr_t)), decay)}
            if batched_feas:        # in two phases: proposals on MFMA, the rigorous decision per node
                rc = ext().beta_feas(net, **fkw, **_ptrs(fpar=fpar, fgt=fgt), mode=1)
            else:                   # per node (bit 3 of the flags)
                rc = ext().beta_level(net, **{**fkw, "flags": beta_flags(False, 0, feas=True)})
        if rc != 0:
            raise RuntimeError(f"fa_beta_kernel launch failed ({rc}): network not supported by the beta kernel")
        if gt is not None:
            rx[4].copy_(gt[:, 0])
            rx[5].copy_(gt[:, 1])
        alA.copy_(par[:, 0])
        alB.copy_(par[:, 1])
        beA.copy_(par[:, 2])
        beB.copy_(par[:, 3])
    return B.BetaLevel(bound=bound, split=split.long(), xstar=xstar, binit=binit, xpstar=xpstar)
