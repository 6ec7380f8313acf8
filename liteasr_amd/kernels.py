"""Torch-tensor front end of the HIP kernels (thin: strides/pointers/stream only).

Every function here launches kernels from libliteasr_hip.so on the current HIP stream
(``torch.cuda.current_stream()``) and never synchronises, so a training step built
from them can be captured into a hipGraph.  Tensors must live on the GPU; there is
no CPU path (the CPU restatement lives in ``oracle/`` and is test-only).

The one part that is not thin is the queue of a backward node's deferred work (``_Deferred``,
``deferred_reductions``): it orders every weight-gradient launch and parameter-gradient reduction
of a training step.  ``gemm`` hands it the dW GEMMs (``_queue_dw``); the backward wrappers hand it
their partial sums (``_partials``, ``_defer`` / ``_reduce_or_defer``).
"""

from __future__ import annotations

import contextlib
import os
import ctypes as C
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from . import _native as N

_DT = {torch.float32: N.F32, torch.bfloat16: N.BF16}


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}") from None


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ workspace ---
class _Workspace:
    """One growing fp32 scratch buffer per device (stream-ordered reuse)."""

    def __init__(self):
        self.buf = {}
        self.frozen = False

    def get(self, nfloats: int, device) -> torch.Tensor:
        nfloats = max(int(nfloats), 1)
        key = torch.device(device).index
        b = self.buf.get(key)
        if b is None or b.numel() < nfloats:
            if self.frozen or torch.cuda.is_current_stream_capturing():
                raise RuntimeError(
                    "workspace growth during graph capture; run a warm-up step first"
                )
            b = torch.empty(int(nfloats * 1.25) + 1024, dtype=torch.float32, device=device)
            self.buf[key] = b
        return b


WS = _Workspace()


# --------------------------------------------------------- deferred reductions ---
# The queue's policy switches are read from the module at call time (tests and tools set them).
# Grouped weight gradients: dW GEMMs marked group=True inside a deferred_reductions block are
# queued and launched at its end, one lasr_gemm_dw_group launch per planned tile (<= 32
# problems each), before the reductions (tests set DW_GROUP = False to compare with lone launches).
DW_GROUP = True
# plan tile -> group (lasr_gemm_dw_group runs the 64 x 128 / 128 x 64 plans, the FFN-sized
# weights, on 128 x 128 tiles)
_GROUP_TILES = {(64, 64): (64, 64), (64, 128): (128, 128), (128, 64): (128, 128)}
_GROUP_MAX = 32  # problems per lasr_gemm_dw_group launch (LASR_DW_GROUP_MAX)
# grouped problems fill the chip together: each takes 1/div of the K slices the planner gives
# a lone launch (fewer fp32 partial slabs to write and reduce); 128 x 128 groups keep half
# (the other divisors measured slower)
DW_GROUP_SPLIT_DIV = {(64, 64): 4, (128, 128): 2}
# Direct grouped weight gradients: FFN-sized problems with >= this many full-K 128 x 128 tiles
# (the d 512 FFN weights: 64 each, a group of four = 256 tiles) skip the K split and write the
# gradient itself (beta = 1), no fp32 partial slab to write and reduce.  Measured at config 4
# (VERDICT r05 item 3): 20.13 -> 20.74 ms per step, the full-K 128 x 128 tiles are L2-feed bound
# where the 256 x 128 split-2 tiles are not (profiles/r06/step_ab_dw_direct_large_rejected.jsonl,
# DESIGN §4); 0 = off.  tests/test_kernels_gpu.py::test_gemm_dw_group_direct pins the path.
DW_DIRECT_MIN_TILES = 0
# grouped dW blocks laid out longest K slice first (lasr_gemm_dw_group_order; same bits)
DW_GROUP_LPT = True
# Held weight-gradient GEMMs: inside a hold block the grouped dW GEMMs are queued without a
# slab and launched where the held reductions are (tests set False to compare).
DW_HOLD_GEMMS = True
# A held family (one group tile) whose tiles at the flush fill the chip (>= the CU count) runs
# serial-slice: one block per tile runs the planned K slices in order and writes the gradient
# itself, the bits of slabs + lasr_reduce_multi.  Smaller families get their slabs
# at the flush and take the slab path.  Counts only: the same on every step and rank.
DW_SERIAL_MIN_TILES = 256
# the waiting GEMMs are launched after this many hold blocks even inside a segment; 0 = at the
# segment's end only.  4 layers of the small model are one full round of FFN tiles (256) and
# measured best of 4 / 6 / whole segment on small, large and long (DESIGN §4,
# profiles/r07/dw_held_serial_ab.jsonl)
DW_HOLD_LAYERS = 4


class Seg(NamedTuple):
    """One parked reduction, a lasr_reduce_multi segment: the P rows of part [P, ncols] are summed
    into out0 (added to it when accumulate), the columns from `split` on into out1."""

    part: torch.Tensor
    P: int
    ncols: int
    out0: torch.Tensor
    out1: Optional[torch.Tensor]
    split: int
    accumulate: int

    @classmethod
    def of(cls, part, P, ncols, out0, out1=None, split=None, accumulate=True):
        return cls(part, int(P), int(ncols), out0, out1, int(ncols if split is None else split), int(accumulate))


class Refs(NamedTuple):
    """What a queued GEMM keeps alive until it is launched: its operands, and where the launch or
    a slab made later writes through them, its output and bias rowsum (else None)."""

    a: Optional[torch.Tensor]
    b: Optional[torch.Tensor]
    c: Optional[torch.Tensor] = None
    rowsum: Optional[torch.Tensor] = None


class QueuedGemm(NamedTuple):
    """A dW GEMM waiting for its lasr_gemm_dw_group launch.  key is its family, the problems that
    may share a launch: the group tile (tm, tn), or DIRECT_FAMILY."""

    key: object
    args: N.GemmArgs
    refs: Refs


# family of the full-K direct problems (DW_DIRECT_MIN_TILES): 128 x 128 tiles, but never in a
# launch with the split problems of that tile
DIRECT_FAMILY = "direct"


def _group_div(key):
    """DW_GROUP_SPLIT_DIV of a group tile: a dict by tile, or one number for every tile."""
    d = DW_GROUP_SPLIT_DIV
    return max(1, d.get(key, 1) if isinstance(d, dict) else int(d))


def _serial_tiles(key, M, Nn):
    """Output tiles of a problem on its family's group tile (lasr_gemm_dw_group)."""
    if key == (64, 64):
        return -(-M // 64) * -(-Nn // 64)
    if M >= 256 and Nn >= 256:
        return -(-M // 256) * -(-Nn // 128)
    return -(-M // 128) * -(-Nn // 128)


def _dw_slab(sp, M, Nn, rowsum, device):
    """The fp32 partials of a dW GEMM split sp ways, alive until their reduction: sp slabs of C,
    then the rowsum partials (fused) or the column-sum scratch (unfused, fp32 operands)."""
    nrs = (sp + 128) * M if rowsum is not None else 0
    return torch.empty(sp * M * Nn + nrs, dtype=torch.float32, device=device)


_PUSHED = {}  # library setter -> the last value pushed through it


def _pushed(setter, value):
    """Keep a library-side setting equal to its switch here: call the setter when the value changes."""
    if _PUSHED.get(setter) != value:
        N.call(setter, int(value))
        _PUSHED[setter] = value


def _launch_dw_groups(q, before_family=None):
    """Launch queued dW GEMMs family by family, families in the order of their first problem,
    <= _GROUP_MAX problems per lasr_gemm_dw_group launch.  before_family(key, problems, launches)
    runs ahead of each family's launches.  The operand references die with q in the caller,
    after the launches were enqueued."""
    _pushed("lasr_gemm_dw_group_order", DW_GROUP_LPT)
    families = {}
    for g in q:
        families.setdefault(g.key, []).append(g)
    for key, fam in families.items():
        chunks = [fam[i:i + _GROUP_MAX] for i in range(0, len(fam), _GROUP_MAX)]
        if before_family is not None:
            before_family(key, fam, chunks)
        for ch in chunks:
            arr = (N.GemmArgs * len(ch))(*[g.args for g in ch])
            N.call("lasr_gemm_dw_group", arr, len(ch), stream())


def _reduce(segs):
    """One lasr_reduce_multi launch over the segments."""
    arr = (N.ReduceSeg * len(segs))()
    for i, s in enumerate(segs):
        arr[i] = N.ReduceSeg(ptr(s.part), s.ncols, s.P, s.accumulate, ptr(s.out0), ptr(s.out1), s.split)
    N.call("lasr_reduce_multi", arr, len(segs), stream())


def _flush_node_end(segs):
    """What the end of a backward node launches: its grouped dW GEMMs, then every reduction."""
    if _DEFER.gemms:
        _DEFER.flush_gemms()
    if segs:
        _reduce(segs)


class _Deferred:
    """Parameter-gradient reductions parked until the end of a backward node: the
    partial-sum buffers of LayerNorm gamma/beta, the positional biases and the split-K
    weight gradients (+ their bias rowsums) are collected and finished by ONE
    lasr_reduce_multi launch, with each reduction's usual summation order.  The node's
    grouped dW GEMMs are queued here too (kernels._queue_dw decides which list takes one)."""

    def __init__(self):
        self.depth = 0  # open deferred_reductions blocks
        self.holding = False  # inside an outermost hold block
        self.segs = []  # the open block's reductions (Seg)
        self.gemms = []  # its dW GEMMs that launch at its end: slab made, or direct (QueuedGemm)
        self.waiting = []  # its dW GEMMs that have no slab yet: they join held_gemms at its end
        self.held = []  # reductions of finished hold blocks, not yet launched
        self.held_gemms = []  # dW GEMMs of finished hold blocks, not yet launched (no slab yet)
        self.held_layers = 0  # hold blocks whose GEMMs wait in held_gemms
        self.done = []  # on_done callbacks of the blocks in held, in block order

    def enter(self, hold, on_done):
        if self.depth and (hold or on_done is not None):
            raise RuntimeError("deferred_reductions: hold / on_done inside another deferred block would be dropped")
        if self.depth == 0:
            self.holding = bool(hold)
        self.depth += 1

    def exit(self, hold, on_done, ok):
        """End of a block (ok: without an exception).  An inner block leaves everything to the
        outermost one, which queues its work (hold) or launches all that is queued."""
        self.depth -= 1
        if self.depth:
            return
        self.holding = False
        waiting, self.waiting = self.waiting, []
        if hold and ok:
            if self.gemms:
                self.flush_gemms()
            self.held.extend(self.segs)
            self.segs = []
            if on_done is not None:
                self.done.append(on_done)
            if waiting:
                self.held_gemms.extend(waiting)
                self.held_layers += 1
                if DW_HOLD_LAYERS and self.held_layers >= DW_HOLD_LAYERS:
                    self.flush_held_gemms()
        else:
            # the block that ends the hold (a segment's lowest layer) adds its own GEMMs to
            # the families it flushes; a raising block's are dropped here, unlaunched
            if ok:
                self.held_gemms.extend(waiting)
            if on_done is not None:
                self.done.append(on_done)
            self.flush()

    def defer(self, *segs):
        self.segs.extend(segs)

    def queue_gemm(self, key, args, refs, slab=True):
        """Queue a dW GEMM (a copy of args) for a grouped launch: at the block's end, or
        slab=False (no partial buffer yet) where the held reductions are flushed."""
        (self.gemms if slab else self.waiting).append(QueuedGemm(key, N.GemmArgs.from_buffer_copy(args), refs))

    def flush_gemms(self):
        q, self.gemms = self.gemms, []
        _launch_dw_groups(q)

    def flush_held_gemms(self):
        """Launch the hold blocks' waiting dW GEMMs, family by family in queue order."""
        q, self.held_gemms = self.held_gemms, []
        self.held_layers = 0
        _launch_dw_groups(q, self._slabs_unless_serial)

    def _slabs_unless_serial(self, key, fam, chunks):
        """A held family runs serial-slice, without slabs, when its tiles fill the chip
        (DW_SERIAL_MIN_TILES); else it takes the slab path: the partial buffers are made here
        and reduced with the held reductions."""
        tiles = [sum(_serial_tiles(key, g.args.M, g.args.N) for g in ch) for ch in chunks]
        # (every launch but a family's last fills the chip; the 128 x 128 tile of an FFN-family
        # problem narrower than 256 has no serial instance)
        serial = (sum(tiles) >= DW_SERIAL_MIN_TILES and all(t >= DW_SERIAL_MIN_TILES for t in tiles[:-1])
                  and (key == (64, 64) or all(g.args.M >= 256 and g.args.N >= 256 for g in fam)))
        if serial:
            return
        for g in fam:
            args, c, rowsum = g.args, g.refs.c, g.refs.rowsum
            sp, M, Nn = -args.split_k, args.M, args.N
            part = _dw_slab(sp, M, Nn, rowsum, c.device)
            args.workspace, args.workspace_bytes = ptr(part), part.numel() * 4
            self.held.append(Seg.of(part, sp, M * Nn, c, accumulate=args.beta == 1.0))
            if rowsum is not None:
                self.held.append(Seg.of(part[sp * M * Nn:], sp, M, rowsum))

    def flush(self):
        """Launch everything queued: the held GEMMs, the open block's, one reduction of all the
        segments, then the callbacks in block order."""
        if self.held_gemms:  # before the reductions: the slab families' segments join self.held
            self.flush_held_gemms()
        segs = self.held + self.segs
        self.held, self.segs = [], []
        done, self.done = self.done, []
        if segs or self.gemms:
            _flush_node_end(segs)
        for fn in done:
            fn()
        # the partial buffers are released here; the caching allocator hands their memory only
        # to work stream-ordered after the reduction

    def held_count(self):
        return len(self.held) + len(self.held_gemms)


_DEFER = _Deferred()


@contextlib.contextmanager
def deferred_reductions(hold=False, on_done=None):
    """Within the block, gradient outputs of layernorm_bwd / qbias_bwd / split-K weight
    GEMMs (split_k=0, beta 0 or 1, fp32 contiguous C) are only complete after the block
    exits; nothing inside may read them.  on_done() runs once they are complete.

    hold=True (the encoder layers' backward nodes): the block's reductions wait in a queue
    (their partial buffers alive) for the next block that does not hold, or flush_reductions():
    the reductions of several layers then share lasr_reduce_multi launches, each with its usual
    summation order, and the held blocks' on_done callbacks run after them, in order.  Its
    grouped weight-gradient GEMMs wait too (DW_HOLD_GEMMS; their operands alive, so the caller
    must not modify them before that flush): they launch there, before the reductions, in
    queue order, and a family with enough tiles by then runs serial-slice, without slabs
    (_Deferred.flush_held_gemms).  A held block that raises drops its waiting GEMMs unlaunched.

    Only an outermost block can hold or take a callback (its end is where reductions are
    launched or queued): asking for either inside another block raises."""
    _DEFER.enter(hold, on_done)
    ok = False
    try:
        yield
        ok = True
    finally:
        _DEFER.exit(hold, on_done, ok)


def flush_reductions():
    _DEFER.flush()


def held_reductions():
    """Number of reductions and weight-gradient GEMMs queued by hold blocks and not yet launched."""
    return _DEFER.held_count()


def _defer(part, P, ncols, out0, out1=None, split=None, accumulate=True):
    _DEFER.defer(Seg.of(part, P, ncols, out0, out1, split, accumulate))


def _partials(nfloats, device, outlives):
    """The fp32 buffer a kernel writes its partial sums to: a fresh one when it outlives the call
    (parked for the block's reduction, or used beside the workspace), else the shared workspace."""
    return torch.empty(nfloats, dtype=torch.float32, device=device) if outlives else WS.get(nfloats, device)


def _reduce_or_defer(*segs):
    """Inside a deferred_reductions block park the segments for its reduction; outside one,
    reduce them now, in one launch."""
    if _DEFER.depth:
        _DEFER.defer(*segs)
    else:
        _reduce(segs)


# ----------------------------------------------------------------------- GEMM ---
# the planner's 64 x 64 tiles for outputs at most 64 wide (lasr_gemm_narrow_tiles; same bits)
GEMM_NARROW_TILES = True
# GEMMs whose 64 x 64 grid cannot fill half the chip and whose K is long are split over K
# (lasr_gemm autosplit; the split-K reduction applies the epilogue).
SMALL_GRID_SPLIT = True
SMALL_GRID_TILES = 128  # (64 x 64 tiles below which a K >= 1024 GEMM is split)


def _split(t: torch.Tensor):
    """(batch strides (s1, s2), batch shape (z1, z2), row stride, col stride)."""
    nb = t.dim() - 2
    assert 0 <= nb <= 2, "gemm operands take at most 2 batch dims"
    st = t.stride()
    sh = t.shape
    if nb == 0:
        return (0, 0), (1, 1), st[0], st[1]
    if nb == 1:
        return (st[0], 0), (sh[0], 1), st[1], st[2]
    return (st[0], st[1]), (sh[0], sh[1]), st[2], st[3]


def _gemm_args(a, b, c):
    """GemmArgs with the shapes, strides, pointers and dtypes of the logical views a (..,M,K),
    b (..,K,N), c (..,M,N); marshalling only, the epilogue fields are the caller's."""
    M, K = a.shape[-2], a.shape[-1]
    K2, Nn = b.shape[-2], b.shape[-1]
    assert K == K2 and c.shape[-2] == M and c.shape[-1] == Nn, (a.shape, b.shape, c.shape)
    assert a.dtype == b.dtype
    (sa1, sa2), (za1, za2), a_m, a_k = _split(a)
    (sb1, sb2), (zb1, zb2), b_k, b_n = _split(b)
    (sc1, sc2), (z1, z2), c_m, c_n = _split(c)
    assert c_n == 1, "C must be row-contiguous"
    assert (za1, za2) == (z1, z2) and (zb1, zb2) == (z1, z2), "batch shapes differ"
    if a_k != 1 and a_m != 1:
        raise ValueError("A needs a unit stride")
    if b_k != 1 and b_n != 1:
        raise ValueError("B needs a unit stride")
    args = N.GemmArgs()
    args.M, args.N, args.K = M, Nn, K
    args.batch, args.batch_div = z1 * z2, z2
    args.A, args.lda_m, args.lda_k, args.sa1, args.sa2 = ptr(a), a_m, a_k, sa1, sa2
    # B logical [K,N]: kernel wants ldb_n (stride along n) and ldb_k (stride along k)
    args.B, args.ldb_n, args.ldb_k, args.sb1, args.sb2 = ptr(b), b_n, b_k, sb1, sb2
    args.C, args.ldc, args.sc1, args.sc2 = ptr(c), c_m, sc1, sc2
    if a_k == 1 and a_m == 1:
        args.lda_k = 1
    if b_k == 1 and b_n == 1:
        args.ldb_k = 1
    args.in_dtype, args.c_dtype = dt(a), dt(c)
    return args


def _auto_split(a, M, Nn, K, batch, split_k, rowsum, zout, group):
    """Small grid, long K (the decoder's B*(L+1)-row GEMMs): split K, reduce with the epilogue."""
    return (split_k == 1 and SMALL_GRID_SPLIT and rowsum is None and zout is None and not group
            and a.dtype == torch.bfloat16 and batch == 1 and K >= 1024
            and ((M + 63) // 64) * ((Nn + 63) // 64) < SMALL_GRID_TILES)


def _plan(args):
    """(tile_m, tile_n, K slices, LASR_PLAN_* bits) lasr_gemm would use; nothing is launched."""
    tm, tn, sp, fl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    N.call("lasr_gemm_plan", C.byref(args), C.byref(tm), C.byref(tn), C.byref(sp), C.byref(fl))
    return tm.value, tn.value, sp.value, fl.value


def _queue_dw(args, a, b, c, rowsum, group):
    """A split-K weight gradient inside a deferred_reductions block (the caller checked: split_k=0
    asked for, no epilogue but beta 0 / 1, one contiguous fp32 C): its reduction, and the launch of
    a grouped one, wait for the block's end.  False: the plan does not split K, launch it as usual."""
    M, Nn = args.M, args.N
    tm, tn, sp, fl = _plan(args)
    grouped = (group and DW_GROUP and (tm, tn) in _GROUP_TILES and (fl & 1) and args.lda_m == 1 and args.ldb_n == 1
               and a.dtype == torch.bfloat16)
    if (grouped and DW_DIRECT_MIN_TILES > 0 and _GROUP_TILES[(tm, tn)] == (128, 128)
            and ((M + 127) // 128) * ((Nn + 127) // 128) >= DW_DIRECT_MIN_TILES):
        # full-K direct problem of the group: C itself (beta 0 / 1), its bias rowsum direct
        args.split_k = 1
        args.workspace, args.workspace_bytes = None, 0
        _DEFER.queue_gemm(DIRECT_FAMILY, args, Refs(a, b, c, rowsum))
        return True
    div = _group_div(_GROUP_TILES[(tm, tn)]) if grouped else 1
    if grouped and (div > 1 or sp < 2):
        # short K too (the positional-projection weight, K = T'): two slices join the group
        sp = max(2, sp // div)
        args.split_k = -sp
        tm, tn, _, fl = _plan(args)
        grouped = (tm, tn) in _GROUP_TILES and bool(fl & 1)
    if sp <= 1:
        return False
    # the explicit slice count from here on: a slab is sized for sp slices, and a re-derived
    # auto split (-1) could differ from sp after the group adjustment
    args.split_k = -sp
    if (grouped and (_DEFER.holding or _DEFER.held_gemms) and DW_HOLD_GEMMS and sp <= 64
            and (M * Nn) % 4 == 0 and (rowsum is None or (M % 4 == 0 and fl & 2))):
        # a hold block, or the block that ends the hold: the GEMM waits, without a slab, for the
        # flush of the held reductions (_Deferred.flush_held_gemms: serial-slice, or the slab path
        # with the slab made there).  The shapes kept out are those whose reduction is not
        # lasr_reduce_multi's slice-order sum.
        args.workspace, args.workspace_bytes = None, 0
        _DEFER.queue_gemm(_GROUP_TILES[(tm, tn)], args, Refs(a, b, c, rowsum), slab=False)
        return True
    # partials-only launch (split_k < 0) into a buffer that lives until the flush
    part = _dw_slab(sp, M, Nn, rowsum, c.device)
    args.workspace, args.workspace_bytes = ptr(part), part.numel() * 4
    if grouped:
        _DEFER.queue_gemm(_GROUP_TILES[(tm, tn)], args, Refs(a, b))
    else:
        N.call("lasr_gemm", C.byref(args), stream())
    _defer(part, sp, M * Nn, c, accumulate=args.beta == 1.0)
    if rowsum is not None and fl & 2:  # LASR_PLAN_ROWSUM_FUSED: partials follow C's
        _defer(part[sp * M * Nn:], sp, M, rowsum)
    return True


def _gemm_ln_fwd(args, c, rowsum, ln_fwd):
    """lasr_gemm_ln_fwd: the GEMM, then the LayerNorm of c's rows."""
    g_, b_, eps, y, mean, rstd = ln_fwd
    assert c.dtype == torch.float32 and c.is_contiguous() and args.batch == 1 and rowsum is None
    N.call("lasr_gemm_ln_fwd", C.byref(args), ptr(g_), ptr(b_), float(eps), ptr(y), dt(y), ptr(mean), ptr(rstd),
           stream())


def _gemm_qbias_bwd(args, c, qbias):
    """lasr_gemm_qbias_bwd: the GEMM with qbias_bwd's blocks beside its split-K reduction."""
    dqu, dqv, B_, T_, H_, dk_, dqkv, du, dv = qbias
    assert c.dtype == dqu.dtype == dqv.dtype == dqkv.dtype
    D_ = H_ * dk_
    nchunk = (B_ * T_ + 63) // 64  # QB_ROWS (csrc/qbias.h)
    part = _partials(nchunk * 2 * D_, c.device, outlives=True)  # (the GEMM's split-K partials live in WS)
    N.call("lasr_gemm_qbias_bwd", C.byref(args), ptr(dqu), ptr(dqv), dt(dqu), B_, T_, H_, dk_, ptr(dqkv),
           dqkv.stride(0), ptr(part), part.numel(), stream())
    _reduce_or_defer(Seg.of(part, nchunk, 2 * D_, du, dv, split=D_))


def _gemm_ln_bwd(args, c, rowsum, q):
    """lasr_gemm_ln_bwd: the GEMM, then the LayerNorm backward of c = dln."""
    assert c.is_contiguous() and args.batch == 1 and rowsum is None
    M, Nn = args.M, args.N
    nblk = (M + 15) // 16  # lasr_layernorm_bwd's 16-row blocks
    # (its own buffer: the GEMM's split-K partials live in WS)
    part = _partials(nblk * 2 * Nn, c.device, outlives=True)
    N.call("lasr_gemm_ln_bwd", C.byref(args), ptr(q.x), dt(q.x), ptr(q.g), ptr(q.mean), ptr(q.rstd),
           ptr(q.dres), dt(q.dres) if q.dres is not None else 0, ptr(q.dx), dt(q.dx), ptr(part), part.numel(),
           ptr(q.gb), dt(q.gb) if q.gb is not None else 0, float(q.bscale), float(q.bp), int(q.bseed), stream())
    if q.dgamma is not None or q.dbeta is not None:
        assert q.dgamma is not None and q.dbeta is not None
        _reduce_or_defer(Seg.of(part, nblk, 2 * Nn, q.dgamma, q.dbeta, split=Nn))


def gemm(
    a: torch.Tensor,
    b: torch.Tensor,
    c: torch.Tensor,
    *,
    alpha: float = 1.0,
    alpha_dev: Optional[torch.Tensor] = None,
    beta: float = 0.0,
    bias: Optional[torch.Tensor] = None,
    act: int = N.ACT_NONE,
    zout: Optional[torch.Tensor] = None,
    aux: Optional[torch.Tensor] = None,
    aux_act: int = N.ACT_NONE,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    res: Optional[torch.Tensor] = None,
    res_scale: float = 1.0,
    split_k: int = 1,
    rowsum: Optional[torch.Tensor] = None,
    plan_only: bool = False,
    zout_mode: int = 0,
    group: bool = False,
    tile: Optional[tuple] = None,
    ksub: int = 0,
    ln_fwd: Optional[tuple] = None,
    ln_bwd: Optional[object] = None,
    qbias: Optional[tuple] = None,
):
    """c = epilogue(alpha * a @ b) for logical views a (..,M,K), b (..,K,N), c (..,M,N).

    Views may be arbitrarily strided as long as each operand has one unit stride
    (the kernel handles K-contiguous and M/N-contiguous operands).

    tile=(tile_m, tile_n) / ksub: per-call plan overrides of the LDS-DMA tile and ring-stage depth
    (A/B tools, bit-identity tests); None / 0 = the planner.

    group=True (a split-K weight gradient inside deferred_reductions): the launch itself may
    be deferred to the end of the block and grouped with the block's other dW GEMMs, so
    the caller must not modify a or b before the block exits (a hold block: before the held
    reductions are flushed; the queue keeps a, b, c and rowsum referenced until then).

    ln_fwd=(gamma, beta, eps, y, mean, rstd): the LayerNorm of c's rows follows
    (lasr_gemm_ln_fwd: in the split-K reduction launch when K is split).  ln_bwd=lnb (an
    object with x, g, mean, rstd, dx, dgamma, dbeta, dres, gb, bscale, bp, bseed): the
    LayerNorm backward of c = dln follows (lasr_gemm_ln_bwd), its dgamma / dbeta partials
    deferred or reduced like layernorm_bwd's.  qbias=(dqu, dqv, B, T, H, dk, dqkv, du, dv):
    qbias_bwd's work runs beside this GEMM's split-K reduction (lasr_gemm_qbias_bwd).

    plan_only: nothing is launched; returns the plan (tile_m, tile_n, K slices, LASR_PLAN_* bits)."""
    _pushed("lasr_gemm_narrow_tiles", GEMM_NARROW_TILES)
    args = _gemm_args(a, b, c)
    M, Nn, K, batch = args.M, args.N, args.K, args.batch
    args.alpha, args.alpha_dev, args.beta = alpha, ptr(alpha_dev), beta
    args.bias = ptr(bias)
    args.act = act
    args.zout = ptr(zout)
    args.zout_mode = zout_mode
    if aux is not None:
        args.aux, args.aux_dtype, args.ldaux, args.aux_act = ptr(aux), dt(aux), aux.stride(0), aux_act
    args.drop_p, args.drop_seed = drop_p, drop_seed
    if tile is not None:
        args.tile_m, args.tile_n = int(tile[0]), int(tile[1])
    args.ksub = int(ksub)
    if res is not None:
        args.res, args.res_dtype, args.ldres, args.res_scale = ptr(res), dt(res), res.stride(0), res_scale
    auto_split = _auto_split(a, M, Nn, K, batch, split_k, rowsum, zout, group)
    if auto_split:
        split_k = 0
    args.split_k = split_k
    if rowsum is not None:
        # fused bias gradient rowsum[m] += sum_k a[m, k] (fp32, a M-contiguous)
        assert rowsum.dtype == torch.float32 and rowsum.is_contiguous() and rowsum.numel() == M
        assert batch == 1 and args.lda_m == 1, "rowsum needs batch 1 and an M-contiguous A"
        args.rowsum = ptr(rowsum)
    if split_k != 1 or rowsum is not None:
        ns = 64 if split_k <= 0 else split_k
        need = ns * batch * M * Nn + (ns + 128) * M if rowsum is not None else ns * batch * M * Nn
        ws = WS.get(need, c.device)
        args.workspace, args.workspace_bytes = ptr(ws), ws.numel() * 4
    if plan_only:
        return _plan(args)
    if (_DEFER.depth and split_k == 0 and not auto_split and beta in (0.0, 1.0) and alpha == 1.0 and alpha_dev is None
            and bias is None and act == N.ACT_NONE and zout is None and aux is None and res is None
            and drop_p <= 0.0 and batch == 1 and c.dtype == torch.float32 and c.is_contiguous()
            and _queue_dw(args, a, b, c, rowsum, group)):
        return c  # (a weight gradient whose reduction, or launch too, waits for the block's end)
    if ln_fwd is not None:
        _gemm_ln_fwd(args, c, rowsum, ln_fwd)
    elif qbias is not None:
        _gemm_qbias_bwd(args, c, qbias)
    elif ln_bwd is not None:
        _gemm_ln_bwd(args, c, rowsum, ln_bwd)
    else:
        N.call("lasr_gemm", C.byref(args), stream())
    return c


def gemm_plan(a, b, c, flags=False, **kw):
    """(tile_m, tile_n, split_k) lasr_gemm would use for this call (nothing is launched);
    flags=True appends the LASR_PLAN_* bits (LDS-DMA path, fused rowsum, 64-deep stages)."""
    plan = gemm(a, b, c, plan_only=True, **kw)
    return plan if flags else plan[:3]


def linear(x, w, out, bias=None, **kw):
    """out[M,N] = x[M,K] @ w[N,K]^T (+bias, epilogue kw)."""
    return gemm(x, w.t(), out, bias=bias, **kw)


def dropout_scale(p: float) -> float:
    """Multiplier of kept elements at drop probability p (1 when p <= 0)."""
    return float(N.load().lasr_dropout_scale(float(p))) if p > 0 else 1.0


def colsum(x2d: torch.Tensor, out: torch.Tensor, accumulate=True):
    M, Nn = x2d.shape
    nchunk = max(1, min((M + 63) // 64, 128))  # colsum_chunks in norm.hip
    ws = WS.get(nchunk * Nn, x2d.device)
    N.call("lasr_colsum", ptr(x2d), dt(x2d), M, Nn, x2d.stride(0), ptr(out), int(accumulate),
           ptr(ws), ws.numel(), stream())


# ------------------------------------------------------------------ LayerNorm ---
def layernorm_fwd(x, gamma, beta, eps, y, mean, rstd, y2=None, p2=0.0, seed2=0):
    rows, D = x.shape
    N.call("lasr_layernorm_fwd", ptr(x), dt(x), rows, D, ptr(gamma), ptr(beta), eps, ptr(y),
           dt(y), ptr(mean), ptr(rstd), ptr(y2), dt(y2) if y2 is not None else 0, p2, seed2,
           stream())


def layernorm2_fwd(x, g1, b1, g2, b2, eps, y, mean1, rstd1, z, mean2, rstd2):
    """y = LN1(x) (fp32), z = LN2(y) (bf16), one launch (lasr_layernorm2_fwd)."""
    rows, D = x.shape
    N.call("lasr_layernorm2_fwd", ptr(x), rows, D, ptr(g1), ptr(b1), ptr(g2), ptr(b2), eps, ptr(y), ptr(mean1),
           ptr(rstd1), ptr(z), ptr(mean2), ptr(rstd2), stream())


def layernorm_bwd(x, dy, gamma, mean, rstd, dx, dgamma, dbeta, dres=None, gb=None,
                  bscale=1.0, bp=0.0, bseed=0):
    rows, D = x.shape
    nblk = (rows + 15) // 16  # LN_ROWS_PER_BLOCK (norm.hip)
    defer = _DEFER.depth and dgamma is not None and dbeta is not None
    ws = _partials(nblk * 2 * D, x.device, outlives=defer)
    og, ob = (None, None) if defer else (dgamma, dbeta)  # (not deferred: the kernel reduces into them)
    N.call("lasr_layernorm_bwd", ptr(x), dt(x), ptr(dy), dt(dy), rows, D, ptr(gamma), ptr(mean),
           ptr(rstd), ptr(dres), dt(dres) if dres is not None else 0, ptr(dx), dt(dx),
           ptr(og), ptr(ob), ptr(ws), ws.numel(), ptr(gb),
           dt(gb) if gb is not None else 0, bscale, bp, bseed, stream())
    if defer:
        _defer(ws, nblk, 2 * D, dgamma, dbeta, split=D)


def layernorm2_bwd(x1, dy1, dres1, g1, mean1, rstd1, dgamma1, dbeta1, x2, g2, mean2, rstd2, dx2, dgamma2, dbeta2,
                   gb2=None, bscale=1.0, bp=0.0, bseed=0):
    """Two LayerNorm backwards per row (lasr_layernorm2_bwd): dx1 = dres1 + LN1'(dy1) (not
    stored), dx2 = LN2'(dx1), gb2 = bscale * drop(dx2); both norms' gamma / beta gradients
    accumulate (deferred inside deferred_reductions)."""
    rows, D = x1.shape
    assert x1.dtype == x2.dtype == dres1.dtype == dx2.dtype == torch.float32
    assert dy1.shape == x1.shape == x2.shape == dres1.shape == dx2.shape
    nblk = (rows + 15) // 16  # LN_ROWS_PER_BLOCK (norm.hip)
    # (two buffers alive at once: not the one workspace)
    part1 = _partials(nblk * 2 * D, x1.device, outlives=True)
    part2 = _partials(nblk * 2 * D, x1.device, outlives=True)
    N.call("lasr_layernorm2_bwd", ptr(x1), ptr(dy1), dt(dy1), ptr(dres1), rows, D, ptr(g1), ptr(mean1), ptr(rstd1),
           ptr(part1), ptr(x2), ptr(g2), ptr(mean2), ptr(rstd2), ptr(dx2), ptr(part2), ptr(gb2),
           dt(gb2) if gb2 is not None else 0, bscale, bp, bseed, stream())
    _reduce_or_defer(Seg.of(part1, nblk, 2 * D, dgamma1, dbeta1, split=D),
                     Seg.of(part2, nblk, 2 * D, dgamma2, dbeta2, split=D))


# ------------------------------------------------- full-row GEMM + LayerNorm ---
def _al16(t):
    return t is None or t.data_ptr() % 16 == 0


# The row kernel's main loop ingests the whole weight per 32-row workgroup, one workgroup per CU:
# measured faster than GEMM + norm up to K = 768 (tools/row_ln_bench.py, profiles/r03), slower at
# K = 2048, where the 64 x 64 GEMM's 2-3 workgroups per CU keep more of the LDS-DMA in flight
# (whole step with the FFN fc2 + norm on the row kernel: 9.83 -> 9.98 ms,
# profiles/r05/step_ab_row_ln_k2048.jsonl).
ROW_LN_MAX_K = 1024
# widest output the product runs on the row kernel: at d 512 (config 4) a 32-row tile streams the
# whole 512 x K weight per tile and the GEMM + LayerNorm launches are faster (whole large step
# 19.25 -> 18.95 ms with the row kernels off, profiles/r06/step_ab_row_ln_large.jsonl); the
# kernels still take D 512 (tests/test_row_ln_gpu.py)
ROW_LN_MAX_D = 256


def row_ln_ok(a, w, D, max_k=None, max_d=None):
    """Whether lasr_linear_res_ln / lasr_linear_dx_ln_bwd take a GEMM with A = a [M, K] and the
    D-wide output: bf16, D in (256, 512), K % 64 == 0, unit column strides, 16-B rows; and
    (the product policy) K <= max_k (default ROW_LN_MAX_K), D <= max_d (ROW_LN_MAX_D)."""
    Kd = a.shape[-1]
    return (a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and D in (256, 512)
            and D <= (ROW_LN_MAX_D if max_d is None else max_d) and a.dim() == 2
            and Kd % 64 == 0 and Kd <= (ROW_LN_MAX_K if max_k is None else max_k) and a.stride(1) == 1
            and a.stride(0) % 8 == 0 and w.is_contiguous() and _al16(a) and _al16(w))


def linear_res_ln(x, w, out, y1, mean1, rstd1, g1, b1, eps, *, bias=None, res, res_scale=1.0, drop_p=0.0,
                  drop_seed=0, g2=None, b2=None, y2=None, mean2=None, rstd2=None):
    """out = res + res_scale * dropout(x @ w^T + bias) (fp32), y1 = LN1(out), optionally
    y2 = LN2(y1): one launch (lasr_linear_res_ln), bit-identical to linear(..., res=...) +
    layernorm_fwd / layernorm2_fwd.  x [M, K] bf16, w [D, K]; [M, D] buffers contiguous."""
    M, Kd = x.shape
    D = w.shape[0]
    a = N.RowLnArgs()
    a.M, a.D, a.K = M, D, Kd
    a.A, a.lda, a.W, a.ldw = ptr(x), x.stride(0), ptr(w), w.stride(0)
    a.gamma1, a.beta1, a.eps, a.mean1, a.rstd1 = ptr(g1), ptr(b1), eps, ptr(mean1), ptr(rstd1)
    a.bias, a.res, a.res_scale, a.drop_p, a.drop_seed = ptr(bias), ptr(res), res_scale, drop_p, drop_seed
    a.out, a.y1, a.y1_dtype = ptr(out), ptr(y1), dt(y1)
    if g2 is not None:
        a.gamma2, a.beta2, a.y2, a.mean2, a.rstd2 = ptr(g2), ptr(b2), ptr(y2), ptr(mean2), ptr(rstd2)
    N.call("lasr_linear_res_ln", C.byref(a), stream())


def linear_dx_ln_bwd(dy, w, x, gamma, mean, rstd, dx, dgamma, dbeta, dres=None, gb=None, bscale=1.0, bp=0.0,
                     bseed=0):
    """dln = bf16(dy @ w) (dy [M, K] bf16, w [K, D]) and the LayerNorm backward of it in one
    launch (lasr_linear_dx_ln_bwd): bit-identical to gemm(dy, w, dln) + layernorm_bwd(x, dln,
    ...).  The dgamma / dbeta partials are reduced like layernorm_bwd's (deferred inside a
    deferred_reductions block)."""
    M, Kd = dy.shape
    D = w.shape[1]
    nblk = (M + 15) // 16
    defer = _DEFER.depth and dgamma is not None and dbeta is not None
    part = _partials(nblk * 2 * D, dy.device, outlives=defer)
    a = N.RowLnArgs()
    a.M, a.D, a.K = M, D, Kd
    a.A, a.lda, a.W, a.ldw = ptr(dy), dy.stride(0), ptr(w), w.stride(0)
    a.gamma1, a.mean1, a.rstd1 = ptr(gamma), ptr(mean), ptr(rstd)
    a.x, a.dres, a.dx, a.gb, a.bscale, a.bp, a.bseed = ptr(x), ptr(dres), ptr(dx), ptr(gb), bscale, bp, bseed
    a.part = ptr(part)
    if not defer:  # reduced in the same call, as layernorm_bwd's immediate path
        a.dgamma, a.dbeta = ptr(dgamma), ptr(dbeta)
    N.call("lasr_linear_dx_ln_bwd", C.byref(a), stream())
    if defer:
        _defer(part, nblk, 2 * D, dgamma, dbeta, split=D)


def branch_grad(dx, gb, scale, p=0.0, seed=0):
    N.call("lasr_branch_grad", ptr(dx), dt(dx), dx.numel(), ptr(gb), dt(gb), scale, p, seed,
           stream())


# ------------------------------------------------------------------------ CTC ---
def _rows_ld(x, lead):
    """Row stride of a logits view whose rows are (possibly padded) vocab vectors."""
    ld = x.stride(-2)
    assert x.stride(-1) == 1 and ld >= x.shape[-1], "logits rows must be unit-stride"
    for d in range(lead):
        assert x.stride(d) == ld * math.prod(x.shape[d + 1:-1]), "logits rows must be evenly spaced"
    return ld


def ctc_fwd(logits, targets, ilen, tlen, lse, lp, alpha, nll, beta=None):
    """beta given: the beta recursion runs in the forward launch too (then ctc_bwd with
    beta_ready=True)."""
    B, T, V = logits.shape
    Lmax = targets.shape[1]
    N.call("lasr_ctc_fwd", ptr(logits), dt(logits), B, T, V, _rows_ld(logits, 1), ptr(targets), Lmax,
           ptr(ilen), ptr(tlen), ptr(lse), ptr(lp), ptr(alpha), ptr(beta), ptr(nll), stream())


def ctc_bwd(logits, targets, ilen, tlen, lse, lp, alpha, nll, beta, grad, gscale, gdev=None,
            beta_ready=False):
    B, T, V = logits.shape
    Lmax = targets.shape[1]
    ld = _rows_ld(logits, 1)
    assert grad.shape == logits.shape and _rows_ld(grad, 1) == ld
    N.call("lasr_ctc_bwd", ptr(logits), dt(logits), B, T, V, ld, ptr(targets), Lmax, ptr(ilen),
           ptr(tlen), ptr(lse), ptr(lp), ptr(alpha), ptr(nll), ptr(beta), int(beta_ready), ptr(grad),
           dt(grad), gscale, ptr(gdev), stream())


# CTC forced alignment (csrc/ctc_align.hip).  A move takes 2 bits: one dword per lattice state and
# 16 frames.  The score vectors and every move word of the launch's T x (2 Lmax + 1) lattice stay
# in LDS when they fit 64 KB; otherwise the words are spilled to the workspace.
CTC_ALIGN_FRAMES_PER_WORD = 16
CTC_ALIGN_LDS = 64 * 1024


def ctc_align_workspace(B, T, Lmax):
    """Bytes of workspace ``ctc_align`` needs (0: the moves stay in LDS); the formula of
    lasr_ctc_align_workspace restated, and held to it."""
    S = 2 * Lmax + 1
    words = -(-T // CTC_ALIGN_FRAMES_PER_WORD)
    if B <= 0 or T <= 0 or Lmax < 0 or S > 1024 or 4 * S * (2 + words) <= CTC_ALIGN_LDS:
        need = 0
    else:
        need = 4 * B * words * S
    native = N.load().lasr_ctc_align_workspace(B, T, Lmax)
    assert need == native, f"ctc_align_workspace({B}, {T}, {Lmax}): {need} here, {native} in the library"
    return need


def ctc_align(lp, targets, ilen, tlen):
    """Viterbi alignment of every row (lasr_ctc_align): ``lp`` fp32 (B, T, Lmax + 1) as ``ctc_fwd``
    with ``alpha=None`` leaves it, ``targets`` int32 (B, Lmax), ``ilen`` / ``tlen`` int32 (B,).
    Returns ``(states, spans, score)``: int32 (B, T), int32 (B, Lmax, 2) and fp32 (B,) on the
    device; -1 past a row's lengths and in every entry of a row whose score is not finite."""
    if lp.dtype != torch.float32 or lp.dim() != 3 or not lp.is_contiguous():
        raise TypeError("ctc_align: lp must be a contiguous fp32 (B, T, Lmax + 1) tensor")
    B, T, L1 = lp.shape
    Lmax = L1 - 1
    for name, t, shape in (("targets", targets, (B, Lmax)), ("ilen", ilen, (B,)), ("tlen", tlen, (B,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != lp.device:
            raise TypeError(f"ctc_align: {name} must be a contiguous int32 {shape} tensor on the device of lp")
    states = torch.empty(B, T, dtype=torch.int32, device=lp.device)
    spans = torch.empty(B, Lmax, 2, dtype=torch.int32, device=lp.device)
    score = torch.empty(B, dtype=torch.float32, device=lp.device)
    need = ctc_align_workspace(B, T, Lmax)
    ws = WS.get((need + 3) // 4, lp.device) if need else None
    N.call("lasr_ctc_align", B, T, Lmax, ptr(targets), ptr(ilen), ptr(tlen), ptr(lp), ptr(ws), need, ptr(states),
           ptr(spans), ptr(score), stream())
    return states, spans, score


def lsm_kl_fwd(logits, target, ignore, smoothing, lse, loss_rows):
    R, V = logits.shape
    N.call("lasr_lsm_kl_fwd", ptr(logits), dt(logits), R, V, _rows_ld(logits, 0), ptr(target), ignore,
           smoothing, ptr(lse), ptr(loss_rows), stream())


def lsm_kl_bwd(logits, target, ignore, smoothing, lse, grad, gscale, gdev=None):
    R, V = logits.shape
    ld = _rows_ld(logits, 0)
    assert grad.shape == logits.shape and _rows_ld(grad, 0) == ld
    N.call("lasr_lsm_kl_bwd", ptr(logits), dt(logits), R, V, ld, ptr(target), ignore, smoothing,
           ptr(lse), ptr(grad), dt(grad), gscale, ptr(gdev), stream())


def padded_rows(rows, V, dtype, device, align=8):
    """[rows, V] view of a [rows, roundup(V, align)] buffer (16-B aligned vocab rows)."""
    Vp = (V + align - 1) // align * align
    return torch.empty(rows, Vp, dtype=dtype, device=device)[:, :V]


def loss_combine(a, wa, b, wb, out):
    N.call("lasr_loss_combine", ptr(a), a.numel(), wa, ptr(b), b.numel() if b is not None else 0,
           wb, ptr(out), stream())


# ------------------------------------------------------------------ attention ---
def qbias_fwd(qkv, B, T, H, dk, bu, bv, qu, qv):
    N.call("lasr_qbias_fwd", ptr(qkv), dt(qkv), B, T, H, dk, qkv.stride(0), ptr(bu), ptr(bv),
           ptr(qu), ptr(qv), stream())


def qbias_bwd(dqu, dqv, B, T, H, dk, dqkv, du, dv):
    rows = B * T
    D = H * dk
    nchunk = (rows + 63) // 64  # QB_ROWS (csrc/qbias.h)
    defer = bool(_DEFER.depth)
    ws = _partials(nchunk * 2 * D, dqu.device, outlives=defer)
    ou, ov = (None, None) if defer else (du, dv)  # (not deferred: the kernel reduces into them)
    N.call("lasr_qbias_bwd", ptr(dqu), ptr(dqv), dt(dqu), B, T, H, dk, ptr(dqkv), dqkv.stride(0),
           ptr(ou), ptr(ov), ptr(ws), ws.numel(), stream())
    if defer:
        _defer(ws, nchunk, 2 * D, du, dv, split=D)


def attn_softmax_fwd(s_ac, s_bd, B, H, Tq, Tk, ldS, mask, msb, msq, P, drop_p=0.0, seed=0,
                     Praw=None):
    N.call("lasr_attn_softmax_fwd", ptr(s_ac), ptr(s_bd), int(s_bd is not None), B, H, Tq, Tk,
           ldS, ptr(mask), msb, msq, ptr(P), dt(P), drop_p, seed, ptr(Praw), stream())


def attn_softmax_bwd(P, dPd, B, H, Tq, Tk, ldS, mask, msb, msq, dS, drop_p=0.0, seed=0):
    N.call("lasr_attn_softmax_bwd", ptr(P), dt(P), ptr(dPd), B, H, Tq, Tk, ldS, ptr(mask), msb,
           msq, drop_p, seed, ptr(dS), dt(dS), stream())


def relshift_bwd(dS, Z, T, ldS, dBD):
    N.call("lasr_relshift_bwd", ptr(dS), dt(dS), Z, T, ldS, ptr(dBD), stream())


def pad_mask16(mask, B, Tq, Tk):
    """A query-dependent mask [B, Tq, Tk] (u8, any layout) as a view of a buffer whose rows are
    16-B aligned (the forward kernels stage its tiles by LDS-DMA): (view, msb, msq).  Padding
    columns are 1 (masked); the view is the same tensor when already aligned."""
    if mask.stride(-1) == 1 and mask.stride(-2) % 16 == 0 and mask.stride(0) % 16 == 0 and mask.data_ptr() % 16 == 0:
        return mask, mask.stride(0), mask.stride(-2)
    P = (Tk + 15) // 16 * 16
    buf = torch.ones(B, Tq, P, dtype=torch.uint8, device=mask.device)
    buf[:, :, :Tk] = mask
    v = buf[:, :, :Tk]
    return v, v.stride(0), v.stride(1)


def _fwd_mask(mask, msb, msq, B, Tq, Tk):
    """(mask, msb, msq) for the forward kernels: query-dependent masks re-laid out with 16-B
    aligned rows when they are not (callers that build masks per step pre-align them)."""
    if mask is None or msq == 0:
        return mask, msb, msq
    if msq % 16 == 0 and msb % 16 == 0 and mask.data_ptr() % 16 == 0:
        return mask, msb, msq
    # element (b, i, j) sits at data_ptr + b*msb + i*msq + j of the caller's storage (the kernels'
    # addressing): view that storage directly -- a reshape of a non-contiguous mask would copy it
    # and leave msb / msq describing the original
    m = torch.as_strided(mask, (B, Tq, Tk), (msb, msq, 1), mask.storage_offset())
    return pad_mask16(m, B, Tq, Tk)


def relattn_fwd(qu, qv, k, v, pos, B, H, T, mask, msb, msq, scale, stats, ctx):
    """Fused rel-pos self-attention (bf16, d_k 32 or 64); 2-D row-major operands (row
    strides read from the tensors), stats [B*H*T*2] fp32 out, ctx [B*T, H*d_k] out."""
    mask, msb, msq = _fwd_mask(mask, msb, msq, B, T, T)
    N.call("lasr_relattn_fwd", ptr(qu), ptr(qv), qu.stride(0), ptr(k), ptr(v), k.stride(0), ptr(pos),
           pos.stride(0), B, H, T, qu.shape[1] // H, ptr(mask), msb, msq, scale, ptr(stats), ptr(ctx),
           ctx.stride(0), stream())


def relattn_fwd_qb(q, bu, bv, qu, qv, k, v, pos, B, H, T, mask, msb, msq, scale, stats, ctx):
    """relattn_fwd with qbias_fwd folded in: q (the qkv projection's q slot) and the fp32
    pos_bias_u / v in; qu = q + u and qv = q + v are formed by the attention kernel and written
    to qu / qv (same strides) for the backward (lasr_relattn_fwd_qb)."""
    assert qv.stride(0) == qu.stride(0) and bu.dtype == torch.float32 and bv.dtype == torch.float32
    mask, msb, msq = _fwd_mask(mask, msb, msq, B, T, T)
    N.call("lasr_relattn_fwd_qb", ptr(q), q.stride(0), ptr(bu), ptr(bv), ptr(qu), ptr(qv), qu.stride(0), ptr(k),
           ptr(v), k.stride(0), ptr(pos), pos.stride(0), B, H, T, qu.shape[1] // H, ptr(mask), msb, msq, scale,
           ptr(stats), ptr(ctx), ctx.stride(0), stream())


def relattn_bwd(qu, qv, k, v, pos, B, H, T, mask, msb, msq, scale, stats, ctx, dctx, Dbuf, dqu,
                dbd, ldS, dk, dv, dbd_head_major=False):
    assert qv.stride(0) == qu.stride(0) and dqu.stride(0) == qu.stride(0)
    assert v.stride(0) == k.stride(0) and dv.stride(0) == dk.stride(0) and dctx.stride(0) == ctx.stride(0)
    mask, msb, msq = _fwd_mask(mask, msb, msq, B, T, T)
    N.call("lasr_relattn_bwd", ptr(qu), ptr(qv), qu.stride(0), ptr(k), ptr(v), k.stride(0), ptr(pos),
           pos.stride(0), B, H, T, qu.shape[1] // H, ptr(mask), msb, msq, scale, ptr(stats), ptr(ctx), ptr(dctx),
           ctx.stride(0), ptr(Dbuf), ptr(dqu), ptr(dbd), ldS, int(dbd_head_major), ptr(dk), ptr(dv), dk.stride(0),
           stream())


def attn_split(B, H, Tq, Tk, nsplit=None):
    """Key-split count of lasr_attn_fwd_split / _bwd_split for a shape (the library's
    heuristic unless given; 1 = the one-pass entries)."""
    ns = N.load().lasr_attn_split_count(B, H, Tq, Tk) if nsplit is None else int(nsplit)
    return ns


def attn_fwd(q, k, v, B, H, Tq, Tk, mask, msb, msq, scale, stats, ctx, nsplit=None):
    """Plain attention on the fused kernels (lasr_attn_fwd): q [B*Tq, H*d_k], k / v
    [B*Tk, H*d_k] row-major views (k and v share a row stride), stats [B*H*Tq*2] fp32.
    Long key runs over few query blocks (the decoder's source attention at T' 999) split
    the keys over workgroups (lasr_attn_fwd_split; nsplit overrides the heuristic)."""
    assert v.stride(0) == k.stride(0)
    mask, msb, msq = _fwd_mask(mask, msb, msq, B, Tq, Tk)
    dk_ = q.shape[1] // H
    ns = attn_split(B, H, Tq, Tk, nsplit)
    if ns > 1:
        nw = N.load().lasr_attn_split_work(B, H, Tq, dk_, ns)
        ws = WS.get(nw, q.device)
        N.call("lasr_attn_fwd_split", ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), B, H, Tq, Tk, dk_,
               ptr(mask), msb, msq, scale, ptr(stats), ptr(ctx), ctx.stride(0), ns, ptr(ws), ws.numel(), stream())
        return
    N.call("lasr_attn_fwd", ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), B, H, Tq, Tk, dk_,
           ptr(mask), msb, msq, scale, ptr(stats), ptr(ctx), ctx.stride(0), stream())


def attn_bwd(q, k, v, B, H, Tq, Tk, mask, msb, msq, scale, stats, ctx, dctx, Dbuf, dq, dk, dv, nsplit=None):
    assert dq.stride(0) == q.stride(0) and v.stride(0) == k.stride(0) and dv.stride(0) == dk.stride(0)
    assert dctx.stride(0) == ctx.stride(0)
    mask, msb, msq = _fwd_mask(mask, msb, msq, B, Tq, Tk)
    dk_ = q.shape[1] // H
    ns = attn_split(B, H, Tq, Tk, nsplit)
    if ns > 1:
        nw = N.load().lasr_attn_split_work(B, H, Tq, dk_, ns)
        ws = WS.get(nw, q.device)
        N.call("lasr_attn_bwd_split", ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), B, H, Tq, Tk, dk_,
               ptr(mask), msb, msq, scale, ptr(stats), ptr(ctx), ptr(dctx), ctx.stride(0), ptr(Dbuf), ptr(dq),
               ptr(dk), ptr(dv), dk.stride(0), ns, ptr(ws), ws.numel(), stream())
        return
    N.call("lasr_attn_bwd", ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), B, H, Tq, Tk, dk_,
           ptr(mask), msb, msq, scale, ptr(stats), ptr(ctx), ptr(dctx), ctx.stride(0), ptr(Dbuf), ptr(dq),
           ptr(dk), ptr(dv), dk.stride(0), stream())


def reduce_batch(src, B, H, T, dk, dst):
    N.call("lasr_reduce_batch", ptr(src), B, H, T, dk, ptr(dst), dt(dst), stream())


# ----------------------------------------------------------------------- conv ---
def conv1_fwd(x, w, bias, y1):
    B, T, F = x.shape
    Cc = w.shape[0]
    N.call("lasr_conv1_fwd", ptr(x), B, T, F, Cc, ptr(w), ptr(bias), ptr(y1), dt(y1), stream())


def conv1_bwd(x, dy1, dw, db):
    B, T, F = x.shape
    Cc = dw.shape[0]
    T1 = (T - 3) // 2 + 1
    nparts = (B * T1 + 7) // 8  # the partial rows of the smallest block lasr_conv1_bwd may use
    ws = WS.get((nparts + 1) * 10 * Cc, x.device)
    N.call("lasr_conv1_bwd", ptr(x), B, T, F, Cc, ptr(dy1), dt(dy1), ptr(dw), ptr(db), ptr(ws),
           ws.numel(), stream())


def im2col(y1, col):
    B, T1, F1, Cc = y1.shape
    N.call("lasr_im2col3x3s2", ptr(y1), dt(y1), B, T1, F1, Cc, ptr(col), stream())


def col2im(dcol, y1, dy1):
    B, T1, F1, Cc = y1.shape
    N.call("lasr_col2im3x3s2", ptr(dcol), dt(dcol), B, T1, F1, Cc, ptr(y1), ptr(dy1), stream())


def conv2_dy2_rows(M2):
    """Rows of the dy2 buffer lasr_conv2_gemm's backward modes need (rows M2.. zero)."""
    return ((M2 + 1 + 31) // 32) * 32


def _conv2(mode, y1, out, w2p=None, bias=None, dy2=None, rowsum=None, x=None, dw1=None, db1=None):
    B, T1, F1, Cc = y1.shape
    assert y1.dtype == torch.bfloat16 and y1.is_contiguous() and (out is None or out.is_contiguous())
    a = N.Conv2Args()
    a.mode, a.B, a.T1, a.F1, a.C = mode, B, T1, F1, Cc
    a.y1, a.out = ptr(y1), ptr(out)
    if w2p is not None:
        assert w2p.dtype == torch.bfloat16 and w2p.is_contiguous() and tuple(w2p.shape) == (Cc, 9 * Cc)
        a.w2p = ptr(w2p)
    if bias is not None:
        a.bias = ptr(bias)
    if dy2 is not None:
        assert dy2.dtype == torch.bfloat16 and dy2.is_contiguous() and dy2.shape[1] == Cc
        a.dy2, a.dy2_rows = ptr(dy2), dy2.shape[0]
    if rowsum is not None:
        assert rowsum.dtype == torch.float32 and rowsum.is_contiguous() and rowsum.numel() == Cc
        a.rowsum = ptr(rowsum)
    if mode == N.CONV2_DW:
        ws = WS.get(32 * (9 * Cc * Cc + Cc), y1.device)  # K slices: <= 32 (gemm_conv.hip caps to fit)
        a.workspace, a.workspace_bytes = ptr(ws), ws.numel() * 4
    if mode == N.CONV2_DX_W1:
        assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] == B
        assert dw1.dtype == torch.float32 and dw1.is_contiguous() and tuple(dw1.shape) == (Cc, 9)
        assert db1.dtype == torch.float32 and db1.is_contiguous() and db1.numel() == Cc
        nbytes = N.load().lasr_conv2_dx_w1_workspace(B, T1, F1, Cc)
        ws = WS.get((nbytes + 3) // 4, y1.device)
        a.workspace, a.workspace_bytes = ptr(ws), ws.numel() * 4
        a.x, a.T, a.F = ptr(x), x.shape[1], x.shape[2]
        a.dw1, a.db1 = ptr(dw1), ptr(db1)
    N.call("lasr_conv2_gemm", C.byref(a), stream())


def conv2_fwd(y1, w2p, bias, y2):
    """y2 [B*T2*F2, C] = relu(conv3x3s2(y1) + bias), y1 channels-last [B, T1, F1, C] bf16."""
    _conv2(N.CONV2_FWD, y1, y2, w2p=w2p, bias=bias)


def conv2_dw(dy2, y1, dw, rowsum=None):
    """dw [C, 9C] fp32 = dy2^T im2col(y1) (dy2: conv2_dy2_rows(M2) rows, tail zero)."""
    _conv2(N.CONV2_DW, y1, dw, dy2=dy2, rowsum=rowsum)


def conv2_dx(dy2, w2p, y1, dy1):
    """dy1 [B, T1, F1, C] bf16 = col2im(dy2 w2p) * relu'(y1)."""
    _conv2(N.CONV2_DX, y1, dy1, w2p=w2p, dy2=dy2)


def conv2_dx_w1_ok(Cc):
    """lasr_conv2_gemm's LASR_CONV2_DX_W1 mode serves this channel count."""
    return Cc % 256 == 0


def conv2_dx_w1(dy2, w2p, y1, x, dw1, db1):
    """conv2_dx's dy1 consumed in place by conv1's weight gradient (dy1 never stored):
    dw1 [C, 9] += sum dy1 (x) patch3x3s2(x), db1 [C] += sum dy1; x [B, T, F] fp32."""
    _conv2(N.CONV2_DX_W1, y1, None, w2p=w2p, dy2=dy2, x=x, dw1=dw1, db1=db1)


def permute_last2(src, Nn, A, Bd, dst, reverse=False, accumulate=False):
    N.call("lasr_permute_last2", ptr(src), dt(src), Nn, A, Bd, ptr(dst), dt(dst), int(reverse),
           int(accumulate), stream())


def dwconv_nparts(B, T):
    return N.load().lasr_dwconv_nparts(B, T)


def glu_dwconv_fwd(z1, B, T, Cc, K, w, bias, y, stats):
    N.call("lasr_glu_dwconv_fwd", ptr(z1), dt(z1), B, T, Cc, K, ptr(w), ptr(bias), ptr(y), dt(y),
           ptr(stats), stream())


def bn_finalize(stats, nparts, Cc, eps, momentum, gamma, beta, rmean, rvar, nbt, mean, rstd,
                scale, shift, update):
    """update: 0 batch stats, 1 batch stats + running update (train), 2 eval (running stats)."""
    N.call("lasr_bn_finalize", ptr(stats), nparts, Cc, eps, momentum, ptr(gamma), ptr(beta),
           ptr(rmean), ptr(rvar), ptr(nbt), ptr(mean), ptr(rstd), ptr(scale), ptr(shift),
           int(update), stream())


def bn_act_fwd(y, scale, shift, h, act=N.ACT_SWISH):
    """h = act(y * scale + shift) (the conv module's BatchNorm + Swish / ReLU)."""
    rows, Cc = y.shape
    N.call("lasr_bn_act_fwd", ptr(y), dt(y), rows, Cc, ptr(scale), ptr(shift), ptr(h), dt(h), act, stream())


def bn_act_bwd(y, dh, scale, shift, mean, rstd, gamma, dgamma, dbeta, dy, batch_stats=True, act=N.ACT_SWISH):
    """batch_stats False: eval-mode BN (mean/rstd are the running statistics)."""
    rows, Cc = y.shape
    ws = WS.get(((rows + 63) // 64 + 1) * 2 * Cc, y.device)
    N.call("lasr_bn_act_bwd", ptr(y), dt(y), ptr(dh), dt(dh), rows, Cc, ptr(scale), ptr(shift),
           ptr(mean), ptr(rstd), ptr(gamma), ptr(dgamma), ptr(dbeta), ptr(dy), dt(dy), ptr(ws),
           ws.numel(), int(bool(batch_stats)), act, stream())


def _dwconv_partials(nparts, K, Cc, device, dw, db):
    """(partials buffer, dw and db as the kernel gets them) of the depthwise backwards.  Deferred:
    nparts rows of [C*K + C] parked for the block's reduction, no outputs; else the workspace,
    one row more, and the kernel reduces into dw / db."""
    if _DEFER.depth:
        return _partials(nparts * (K + 1) * Cc, device, outlives=True), None, None
    return _partials((nparts + 1) * (K + 1) * Cc, device, outlives=False), dw, db


def glu_dwconv_bwd(z1, dy, B, T, Cc, K, w, dz1, dw, db):
    """dw [C, K] and db [C] accumulate; partials are [nparts][C*K + C] in their layout."""
    nparts = dwconv_nparts(B, T)
    ws, ow, ob = _dwconv_partials(nparts, K, Cc, z1.device, dw, db)
    N.call("lasr_glu_dwconv_bwd", ptr(z1), dt(z1), ptr(dy), dt(dy), B, T, Cc, K, ptr(w), ptr(dz1),
           ptr(ow), ptr(ob), ptr(ws), ws.numel(), stream())
    if _DEFER.depth:
        _defer(ws, nparts, (K + 1) * Cc, dw, db, split=K * Cc)


def bn_act_glu_dwconv_bwd(y, dh, scale, shift, mean, rstd, gamma, dgamma, dbeta, z1, B, T, Cc, K, w, dz1, dw, db,
                          batch_stats=True, act=N.ACT_SWISH):
    """bn_act_bwd + glu_dwconv_bwd in one call (lasr_bn_act_glu_dwconv_bwd): the BN backward's dy
    is computed inside the depthwise backward's window load, never stored.  Same outputs."""
    rows = y.shape[0]
    assert rows == B * T and y.shape[1] == Cc and dh.shape == y.shape and z1.shape == (rows, 2 * Cc)
    # (its own buffer: the depthwise partials below may take WS)
    bn_ws = _partials(((rows + 63) // 64 + 1) * 2 * Cc, y.device, outlives=True)
    nparts = dwconv_nparts(B, T)
    ws, ow, ob = _dwconv_partials(nparts, K, Cc, z1.device, dw, db)
    N.call("lasr_bn_act_glu_dwconv_bwd", ptr(y), dt(y), ptr(dh), dt(dh), B, T, Cc, ptr(scale), ptr(shift), ptr(mean),
           ptr(rstd), ptr(gamma), ptr(dgamma), ptr(dbeta), ptr(bn_ws), bn_ws.numel(), int(bool(batch_stats)), act,
           ptr(z1), dt(z1), K, ptr(w), ptr(dz1), ptr(ow), ptr(ob), ptr(ws), ws.numel(), stream())
    if _DEFER.depth:
        _defer(ws, nparts, (K + 1) * Cc, dw, db, split=K * Cc)


# ---------------------------------------------------------------- elementwise ---
def cast(src, dst):
    N.call("lasr_cast", ptr(src), dt(src), ptr(dst), dt(dst), src.numel(), stream())


def pcm_to_float(pcm, out=None):
    """16-bit PCM -> fp32 waveform, pcm * 2^-15 (lasr_pcm_to_float).  ``pcm``: a contiguous int16
    device tensor (any 2-byte-aligned view); returns ``out`` (fp32, the same shape)."""
    if pcm.dtype != torch.int16 or not pcm.is_contiguous() or pcm.device.type != "cuda":
        raise TypeError("pcm_to_float: a contiguous int16 device tensor is needed")
    if out is None:
        out = torch.empty(pcm.shape, dtype=torch.float32, device=pcm.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != pcm.numel():
        raise TypeError("pcm_to_float: out must be a contiguous fp32 tensor of the same size")
    N.call("lasr_pcm_to_float", ptr(pcm), pcm.numel(), ptr(out), stream())
    return out


# Kaldi fbank front end (csrc/fbank.hip).  The Kaldi options are fixed: 16 kHz, 25 ms / 10 ms
# frames, snip-edges, no dither, DC removal, pre-emphasis 0.97, povey window, 512-point FFT,
# power spectrum, mel filters from 20 Hz to the Nyquist frequency, no energy, no VTLN.
FBANK_FRAME_LEN, FBANK_FRAME_SHIFT, FBANK_NFFT, FBANK_FS = 400, 160, 512, 16000
FBANK_LOW_FREQ, FBANK_MAX_BINS = 20.0, 128
_FBANK_TABLES = {}


def fbank_num_frames(nsamples: int) -> int:
    """snip-edges frame count of an utterance of ``nsamples`` samples."""
    return 0 if nsamples < FBANK_FRAME_LEN else 1 + (nsamples - FBANK_FRAME_LEN) // FBANK_FRAME_SHIFT


def fbank_tables(num_mel_bins: int):
    """The kernel's tables, computed in float64 on the host: (tab float32 [2048], seg int32 [F + 2]).
    tab: the povey window padded to 512; exp(-2 pi i m / 256) and exp(-2 pi i k / 512) for m, k <
    256, interleaved (re, im); then per FFT bin k < 256 its rising and its falling mel weight.
    The F + 2 mel edges cut the bins into F + 1 runs, run j = the bins with edge[j] < mel(bin) <=
    edge[j + 1] (the last run stops below the last edge) starting at seg[j], seg[F + 1] its end;
    filter f sums its rising weights over run f and its falling weights over run f + 1, so a
    bin lies in at most two triangles and carries one weight for each."""
    import numpy as np

    F = int(num_mel_bins)
    if not 1 <= F <= FBANK_MAX_BINS:
        raise ValueError(f"fbank: num_mel_bins must be in 1..{FBANK_MAX_BINS}, got {F}")
    half = FBANK_NFFT // 2
    tab = np.zeros(2048, dtype=np.float64)
    i = np.arange(FBANK_FRAME_LEN, dtype=np.float64)
    tab[:FBANK_FRAME_LEN] = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FBANK_FRAME_LEN - 1))) ** 0.85
    k = np.arange(half, dtype=np.float64)
    for base, n in ((512, half), (1024, FBANK_NFFT)):
        tab[base:base + 512:2] = np.cos(2.0 * np.pi * k / n)
        tab[base + 1:base + 512:2] = -np.sin(2.0 * np.pi * k / n)

    def mel(f):
        return 1127.0 * np.log(1.0 + f / 700.0)

    edges = np.linspace(mel(FBANK_LOW_FREQ), mel(FBANK_FS / 2.0), F + 2)
    m = mel(k * (FBANK_FS / FBANK_NFFT))
    seg = np.searchsorted(m, edges, side="right").astype(np.int32)  # first bin with mel > edge
    seg[F + 1] = np.searchsorted(m, edges[F + 1], side="left")  # the last edge itself is outside
    for j in range(F + 1):
        lo, hi = int(seg[j]), int(seg[j + 1])
        width = edges[j + 1] - edges[j]
        tab[1536 + lo:1536 + hi] = (m[lo:hi] - edges[j]) / width
        tab[1792 + lo:1792 + hi] = (edges[j + 1] - m[lo:hi]) / width
    return tab.astype(np.float32), seg


def _fbank_device_tables(F: int, device):
    key = (int(F), torch.device(device).index)
    t = _FBANK_TABLES.get(key)
    if t is None:
        tab, seg = fbank_tables(F)
        t = (torch.from_numpy(tab).to(device), torch.from_numpy(seg).to(device))
        _FBANK_TABLES[key] = t
    return t


def fbank(pcm, nframes, num_mel_bins=80, cmvn=None, out=None, max_frames=None):
    """Kaldi log-mel filterbank features of a batch of 16-bit PCM (lasr_fbank): ``pcm`` an int16
    device tensor (B, S) with contiguous rows (any row stride), ``nframes`` int32 [B] on the
    device, ``cmvn`` None or (mean, istd) fp32 [F] device tensors.  Returns ``out``, fp32
    (B, Tmax, F) contiguous, every element written: rows t >= nframes[b] are zero.  Tmax is
    out.shape[1], or the largest frame count.  ``max_frames``: the caller's host-side bound on
    nframes (frame counts above it are clamped by the kernel); None reads it back from the
    device, one synchronisation.  S must hold the samples of max_frames frames."""
    if (pcm.dtype != torch.int16 or pcm.dim() != 2 or pcm.device.type != "cuda"
            or (pcm.shape[1] > 1 and pcm.stride(1) != 1)):
        raise TypeError("fbank: an int16 (B, S) device tensor with contiguous rows is needed")
    B, S = pcm.shape
    if (nframes.dtype != torch.int32 or nframes.device != pcm.device or nframes.shape != (B,)
            or not nframes.is_contiguous()):
        raise TypeError("fbank: nframes must be an int32 [B] tensor on the device of pcm")
    F = int(num_mel_bins)
    tab, seg = _fbank_device_tables(F, pcm.device)
    if max_frames is None:
        max_frames = int(nframes.max()) if B else 0
    max_frames = max(int(max_frames), 0)
    if max_frames and S < FBANK_FRAME_SHIFT * (max_frames - 1) + FBANK_FRAME_LEN:
        raise ValueError(f"fbank: {S} samples per row cannot hold {max_frames} frames")
    mean = istd = None
    if cmvn is not None:
        mean, istd = cmvn
        for v in (mean, istd):
            if v.dtype != torch.float32 or v.device != pcm.device or v.shape != (F,) or not v.is_contiguous():
                raise TypeError("fbank: cmvn must be two fp32 [F] tensors on the device of pcm")
    if out is None:
        out = torch.empty(B, max_frames, F, dtype=torch.float32, device=pcm.device)
    elif (out.dtype != torch.float32 or out.device != pcm.device or out.dim() != 3 or out.shape[0] != B
          or out.shape[2] != F or not out.is_contiguous()):
        raise TypeError("fbank: out must be a contiguous fp32 (B, Tmax, F) tensor on the device of pcm")
    N.call("lasr_fbank", ptr(pcm), pcm.stride(0) if B > 1 else S, B, S, ptr(nframes), max_frames, ptr(tab),
           ptr(seg), F, ptr(mean), ptr(istd), ptr(out), out.shape[1], stream())
    return out


# Speed perturbation (csrc/resample.hip): the Hann-windowed sinc of Kaldi's LinearResample, filter
# width 6 and roll-off 0.99, per row by a speed factor p / q.
RESAMPLE_WIDTH, RESAMPLE_ROLLOFF, RESAMPLE_MAX_PQ = 6, 0.99, 32


def resample_ratio(speed):
    """The speed factor as the reduced fraction (p, q) = Fraction(str(speed)); factors outside
    [0.5, 2] or with p or q above 32 are refused."""
    from fractions import Fraction

    try:
        f = Fraction(str(speed))
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"speed factor {speed!r} is not a number") from None
    p, q = f.numerator, f.denominator
    if not (Fraction(1, 2) <= f <= 2 and p <= RESAMPLE_MAX_PQ and q <= RESAMPLE_MAX_PQ):
        raise ValueError(f"speed factor {speed!r} is not supported: a factor in [0.5, 2] that reduces to p / q with "
                         f"p, q <= {RESAMPLE_MAX_PQ} is needed (0.9, 1.0, 1.1)")
    return p, q


def resample_tables(ratios, dtype="float32"):
    """The kernel's tables for the distinct (p, q) of ``ratios``, computed in float64 on the host:
    (table int32 [R, 4], taps float32 [n_taps]).  Row r of the table is p, q, width = ceil(L / c)
    and the offset of the ratio's taps, q x (2 width + p) phase-major: tap[i][k] weighs input
    j p - width + k in output j q + i,
      tap[i][k] = c sinc(u) cos^2(pi u / 2L),  u = c (k - width - i p / q),  0 where |u| >= L,
    c = 0.99 min(1, q / p), L = 6.  p = q is width 0 and the single tap 1: a copy.  ``dtype``
    float64 gives the taps before their rounding to the kernel's float32."""
    import numpy as np

    table, blocks, off = [], [], 0
    for p, q in ratios:
        p, q = int(p), int(q)
        if not (1 <= p <= RESAMPLE_MAX_PQ and 1 <= q <= RESAMPLE_MAX_PQ and p <= 2 * q and q <= 2 * p):
            raise ValueError(f"resample: ratio {p}/{q} is outside [0.5, 2] with p, q <= {RESAMPLE_MAX_PQ}")
        if np.gcd(p, q) != 1:
            raise ValueError(f"resample: ratio {p}/{q} is not reduced")
        if p == q:
            width, tap = 0, np.ones((1, 1), dtype=np.float64)
        else:
            L = float(RESAMPLE_WIDTH)
            c = RESAMPLE_ROLLOFF * min(1.0, q / p)
            width = int(np.ceil(L / c))
            i = np.arange(q, dtype=np.float64)[:, None]
            k = np.arange(2 * width + p, dtype=np.float64)[None, :]
            u = c * (k - width - i * p / q)
            tap = np.where(np.abs(u) < L, c * np.sinc(u) * np.cos(np.pi * u / (2.0 * L)) ** 2, 0.0)
        table.append((p, q, width, off))
        blocks.append(tap.reshape(-1))
        off += tap.size
    if not table:
        raise ValueError("resample: no ratio")
    return np.asarray(table, dtype=np.int32), np.concatenate(blocks).astype(dtype)


def resample_i16(pcm, plan, ratios, taps, out=None, max_out=None):
    """Rows of 16-bit PCM resampled by their own speed factors (lasr_resample_i16): ``pcm`` an
    int16 device tensor (B, S_in) with contiguous rows (any row stride), ``plan`` int32 (B, 3) on
    the device (n_in, n_out, ratio index per row), ``ratios`` int32 (R, 4) and ``taps`` fp32 [n]
    the device copies of ``resample_tables``.  Returns ``out``, int16 (B, S_out) with contiguous
    rows, every element written: samples m >= n_out[b] are zero.  S_out is out.shape[1], or
    ``max_out``, the caller's host-side bound on n_out (larger counts are clamped by the
    kernel); None reads it back from the device, one synchronisation."""
    if (pcm.dtype != torch.int16 or pcm.dim() != 2 or pcm.device.type != "cuda"
            or (pcm.shape[1] > 1 and pcm.stride(1) != 1)):
        raise TypeError("resample_i16: an int16 (B, S) device tensor with contiguous rows is needed")
    B, S = pcm.shape
    if (plan.dtype != torch.int32 or plan.device != pcm.device or plan.shape != (B, 3) or not plan.is_contiguous()):
        raise TypeError("resample_i16: plan must be a contiguous int32 (B, 3) tensor on the device of pcm")
    if (ratios.dtype != torch.int32 or ratios.device != pcm.device or ratios.dim() != 2 or ratios.shape[1] != 4
            or ratios.shape[0] < 1 or not ratios.is_contiguous()):
        raise TypeError("resample_i16: ratios must be a contiguous int32 (R, 4) tensor on the device of pcm")
    if taps.dtype != torch.float32 or taps.device != pcm.device or taps.dim() != 1 or not taps.is_contiguous():
        raise TypeError("resample_i16: taps must be a contiguous fp32 vector on the device of pcm")
    if out is None:
        if max_out is None:
            max_out = int(plan[:, 1].max()) if B else 0
        if int(max_out) < 0:
            raise ValueError(f"resample_i16: max_out = {max_out} is negative")
        out = torch.empty(B, int(max_out), dtype=torch.int16, device=pcm.device)
    elif (out.dtype != torch.int16 or out.device != pcm.device or out.dim() != 2 or out.shape[0] != B
          or (out.shape[1] > 1 and out.stride(1) != 1) or (B > 1 and out.shape[1] and out.stride(0) < out.shape[1])):
        raise TypeError("resample_i16: out must be an int16 (B, S_out) tensor with contiguous rows on the device of "
                        "pcm")
    elif max_out is not None and int(max_out) > out.shape[1]:
        raise ValueError(f"resample_i16: out holds {out.shape[1]} samples per row, max_out is {max_out}")
    N.call("lasr_resample_i16", ptr(pcm), pcm.stride(0) if B > 1 else S, B, S, ptr(plan), ptr(ratios),
           ratios.shape[0], ptr(taps), taps.numel(), ptr(out), out.stride(0) if B > 1 else out.shape[1],
           out.shape[1], stream())
    return out


# Additive noise (csrc/mix.hip): up to MIX_MAX_SOURCES recordings of a resident bank per row.
MIX_MAX_SOURCES = 8


def mix_plan(ns, sources):
    """The kernel's two host tables for a batch: ``ns`` the samples of every row, ``sources`` per
    row a list of (offset, length, start, r): the recording at bank[offset : offset + length],
    read from ``start`` and wrapped, and r = 10^(-snr / 10) as a float64.  Returns (rows int32
    [B, 3]: n, first source, count; table int64 [n_src, 4]: offset, length, start and the bits of
    r), the sources of the rows back to back in row order."""
    import numpy as np

    if len(ns) != len(sources):
        raise ValueError(f"mix_plan: {len(ns)} rows, source lists for {len(sources)}")
    rows = np.zeros((len(ns), 3), dtype=np.int32)
    flat = []
    for b, (n, srcs) in enumerate(zip(ns, sources)):
        if len(srcs) > MIX_MAX_SOURCES:
            raise ValueError(f"mix_plan: row {b} has {len(srcs)} sources, at most {MIX_MAX_SOURCES} are mixed")
        rows[b] = (int(n), len(flat), len(srcs))
        flat.extend(srcs)
    table = np.zeros((len(flat), 4), dtype=np.int64)
    if flat:
        table[:, :3] = np.asarray([s[:3] for s in flat], dtype=np.int64)
        table[:, 3] = np.asarray([s[3] for s in flat], dtype=np.float64).view(np.int64)
    return rows, table


def mix_i16(pcm, bank, rows, sources, out=None, gains=None):
    """Rows of 16-bit PCM with noise of a resident bank mixed in at host-drawn SNRs (lasr_mix_i16):
    ``pcm`` an int16 device tensor (B, S) with contiguous rows (any row stride), ``bank`` the
    int16 vector of recordings on that device, ``rows`` int32 (B, 3) and ``sources`` int64
    (n_src, 4) the device copies of ``mix_plan``.  Returns ``out``, int16 (B, S) with contiguous
    rows, every element written: samples m >= n[b] are zero.  ``out`` None makes a new tensor;
    ``out`` may be ``pcm`` itself (in place), otherwise it must not overlap it.  ``gains``: an
    fp32 [n_src] device tensor that receives the gain of every source."""
    if (pcm.dtype != torch.int16 or pcm.dim() != 2 or pcm.device.type != "cuda"
            or (pcm.shape[1] > 1 and pcm.stride(1) != 1)):
        raise TypeError("mix_i16: an int16 (B, S) device tensor with contiguous rows is needed")
    B, S = pcm.shape
    if B > 1 and S and pcm.stride(0) < S:
        raise TypeError("mix_i16: the rows of pcm overlap")
    if bank.dtype != torch.int16 or bank.device != pcm.device or bank.dim() != 1 or not bank.is_contiguous():
        raise TypeError("mix_i16: bank must be a contiguous int16 vector on the device of pcm")
    if rows.dtype != torch.int32 or rows.device != pcm.device or rows.shape != (B, 3) or not rows.is_contiguous():
        raise TypeError("mix_i16: rows must be a contiguous int32 (B, 3) tensor on the device of pcm")
    if (sources.dtype != torch.int64 or sources.device != pcm.device or sources.dim() != 2 or sources.shape[1] != 4
            or not sources.is_contiguous()):
        raise TypeError("mix_i16: sources must be a contiguous int64 (n_src, 4) tensor on the device of pcm")
    n_src = sources.shape[0]
    if gains is not None and (gains.dtype != torch.float32 or gains.device != pcm.device or gains.shape != (n_src,)
                              or not gains.is_contiguous()):
        raise TypeError("mix_i16: gains must be a contiguous fp32 [n_src] tensor on the device of pcm")
    if out is None:
        out = torch.empty(B, S, dtype=torch.int16, device=pcm.device)
    elif (out.dtype != torch.int16 or out.device != pcm.device or out.dim() != 2 or out.shape[0] != B
          or (out.shape[1] > 1 and out.stride(1) != 1) or (B > 1 and out.shape[1] and out.stride(0) < out.shape[1])):
        raise TypeError("mix_i16: out must be an int16 (B, S) tensor with contiguous rows on the device of pcm")
    elif out.shape[1] != S:
        raise ValueError(f"mix_i16: out holds {out.shape[1]} samples per row, pcm {S}")
    nbytes = N.load().lasr_mix_ws_bytes(B, S)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=pcm.device)
    N.call("lasr_mix_i16", ptr(pcm), pcm.stride(0) if B > 1 else S, B, S, ptr(bank) if bank.numel() else None,
           bank.numel(), ptr(rows), ptr(sources) if n_src else None, n_src, ptr(out),
           out.stride(0) if B > 1 else S, ptr(gains), ptr(ws), ws.numel() * 8, stream())
    return out


# Room reverberation (csrc/reverb.hip): uniformly partitioned overlap-save at one fixed block size.
REVERB_BLOCK, REVERB_MAX_TAPS = 2048, 65536


def reverb_tables():
    """The kernel's twiddle table, computed in float64 on the host: float32 [4 REVERB_BLOCK], the
    complex numbers exp(-2 pi i m / (2 REVERB_BLOCK)), m < 2 REVERB_BLOCK, as (re, im) pairs."""
    import numpy as np

    ang = -2.0 * np.pi * np.arange(2 * REVERB_BLOCK, dtype=np.float64) / (2 * REVERB_BLOCK)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32).reshape(-1)


def reverb_plan(ns, rir_ids):
    """The kernel's host table for a batch, int32 [B, 2]: per row its samples ``ns[b]`` and the
    index ``rir_ids[b]`` of its RIR in the ``rirs`` table, -1 for a row that is only copied."""
    import numpy as np

    if len(ns) != len(rir_ids):
        raise ValueError(f"reverb_plan: {len(ns)} rows, RIR indices for {len(rir_ids)}")
    rows = np.zeros((len(ns), 2), dtype=np.int32)
    for b, (n, i) in enumerate(zip(ns, rir_ids)):
        rows[b] = (int(n), int(i))
    return rows


_reverb_tab = {}


def reverb_i16(pcm, bank, rows, rirs, out=None, gains=None, max_taps=None):
    """Rows of 16-bit PCM convolved with room impulse responses of a resident bank, shifted to the
    RIR's peak, cut to the row's own samples and scaled back to the row's energy (lasr_reverb_i16):
    ``pcm`` an int16 device tensor (B, S) with contiguous rows (any row stride), ``bank`` the int16
    vector of RIRs on that device, ``rows`` int32 (B, 2) the device copy of ``reverb_plan`` and
    ``rirs`` int64 (n_rir, 3) on the device: offset, length and peak index of every RIR.  Returns
    ``out``, int16 (B, S) with contiguous rows, every element written: samples m >= n[b] are zero.
    ``out`` None makes a new tensor; ``out`` may be ``pcm`` itself (in place), otherwise it must
    not overlap it.  ``gains``: an fp32 [B] device tensor that receives the gain of every row (1
    for a copied row).  ``max_taps``: the caller's host-side bound on the lengths in ``rirs`` (a
    longer RIR gives a zero row); None reads it back from the device, one synchronisation.  The
    workspace is made here."""
    if (pcm.dtype != torch.int16 or pcm.dim() != 2 or pcm.device.type != "cuda"
            or (pcm.shape[1] > 1 and pcm.stride(1) != 1)):
        raise TypeError("reverb_i16: an int16 (B, S) device tensor with contiguous rows is needed")
    B, S = pcm.shape
    if B > 1 and S and pcm.stride(0) < S:
        raise TypeError("reverb_i16: the rows of pcm overlap")
    if bank.dtype != torch.int16 or bank.device != pcm.device or bank.dim() != 1 or not bank.is_contiguous():
        raise TypeError("reverb_i16: bank must be a contiguous int16 vector on the device of pcm")
    if rows.dtype != torch.int32 or rows.device != pcm.device or rows.shape != (B, 2) or not rows.is_contiguous():
        raise TypeError("reverb_i16: rows must be a contiguous int32 (B, 2) tensor on the device of pcm")
    if (rirs.dtype != torch.int64 or rirs.device != pcm.device or rirs.dim() != 2 or rirs.shape[1] != 3
            or not rirs.is_contiguous()):
        raise TypeError("reverb_i16: rirs must be a contiguous int64 (n_rir, 3) tensor on the device of pcm")
    n_rir = rirs.shape[0]
    if gains is not None and (gains.dtype != torch.float32 or gains.device != pcm.device or gains.shape != (B,)
                              or not gains.is_contiguous()):
        raise TypeError("reverb_i16: gains must be a contiguous fp32 [B] tensor on the device of pcm")
    if out is None:
        out = torch.empty(B, S, dtype=torch.int16, device=pcm.device)
    elif (out.dtype != torch.int16 or out.device != pcm.device or out.dim() != 2 or out.shape[0] != B
          or (out.shape[1] > 1 and out.stride(1) != 1) or (B > 1 and out.shape[1] and out.stride(0) < out.shape[1])):
        raise TypeError("reverb_i16: out must be an int16 (B, S) tensor with contiguous rows on the device of pcm")
    elif out.shape[1] != S:
        raise ValueError(f"reverb_i16: out holds {out.shape[1]} samples per row, pcm {S}")
    if max_taps is None:
        max_taps = int(rirs[:, 1].max()) if n_rir else 1
    max_taps = min(max(int(max_taps), 1), REVERB_MAX_TAPS)
    if pcm.device not in _reverb_tab:
        _reverb_tab[pcm.device] = torch.from_numpy(reverb_tables()).to(pcm.device)
    nbytes = N.load().lasr_reverb_ws_bytes(B, S, max_taps)
    ws = torch.empty(max(nbytes // 8, 2), dtype=torch.int64, device=pcm.device)
    N.call("lasr_reverb_i16", ptr(pcm), pcm.stride(0) if B > 1 else S, B, S, ptr(bank) if bank.numel() else None,
           bank.numel(), ptr(rows), ptr(rirs) if n_rir else None, n_rir, ptr(_reverb_tab[pcm.device]), ptr(out),
           out.stride(0) if B > 1 else S, ptr(gains), ptr(ws), ws.numel() * 8, stream())
    return out


def scale_add(a, b, sa, sb, out):
    N.call("lasr_scale_add", ptr(a), dt(a), ptr(b), dt(b) if b is not None else 0, sa, sb,
           ptr(out), dt(out), out.numel(), stream())


def pe_fwd(x, rows, T, D, pe, xscale, y, p=0.0, seed=0):
    N.call("lasr_pe_fwd", ptr(x), dt(x) if x is not None else 0, rows, T, D, ptr(pe), xscale, p,
           seed, ptr(y), dt(y), stream())


def embed_pe_fwd(ids, L, E, pe, xscale, y, p=0.0, seed=0):
    R = ids.numel()
    D = E.shape[1]
    N.call("lasr_embed_pe_fwd", ptr(ids), R, L, D, ptr(E), ptr(pe), xscale, p, seed, ptr(y),
           dt(y), stream())


def embed_bwd(ids, dy, xscale, dE, p=0.0, seed=0):
    R = ids.numel()
    D = dE.shape[1]
    N.call("lasr_embed_bwd", ptr(ids), R, D, ptr(dy), dt(dy), xscale, p, seed, ptr(dE), stream())


def fill(t, value):
    N.call("lasr_fill", ptr(t), dt(t), t.numel(), float(value), stream())


CHUNK_NONE, CHUNK_FIXED, CHUNK_DEVICE, CHUNK_SAMPLE = 0, 1, 2, 3


def u2_prep(xlens, ys, ylens, Tx, Tsub, sos, eos, chunk, out, chunk_mode=None, chunk_dev=None, ctr=None,
            chunk_seed=0, chunk_max=25):
    """One lasr_u2_prep_chunk launch: out["dec_mask"] [B, L+1, ld >= L+1] (the last dimension
    is the row stride; columns past L+1 come out 1 = masked), out["enc_mask"] [B, T'] (key
    padding), the targets and lengths, and -- unless chunk_mode is CHUNK_NONE -- the
    streaming chunk mask out["chunk_mask"] [B, T', ld >= T'] (padding columns masked).
    chunk_mode defaults to CHUNK_FIXED for chunk > 0, else CHUNK_NONE; CHUNK_DEVICE reads c
    from the int32 device scalar ``chunk_dev``, CHUNK_SAMPLE draws it from (chunk_seed, the
    uint64 step counter ``ctr``) and writes it to ``chunk_dev``; c <= 0 or c >= T' is full
    context."""
    B, L = ys.shape
    if chunk_mode is None:
        chunk_mode = CHUNK_FIXED if chunk > 0 else CHUNK_NONE
    dm, em = out["dec_mask"], out["enc_mask"]
    assert dm.is_contiguous() and dm.dim() == 3 and tuple(dm.shape[:2]) == (B, L + 1) and dm.shape[-1] >= L + 1
    assert em.is_contiguous() and em.dtype == torch.uint8 and em.numel() == B * Tsub
    cm, cld = None, 0
    if chunk_mode != CHUNK_NONE:
        cm = out["chunk_mask"]
        assert cm.is_contiguous() and cm.dim() == 3 and tuple(cm.shape[:2]) == (B, Tsub) and cm.shape[-1] >= Tsub
        cld = cm.shape[-1]
    if chunk_mode in (CHUNK_DEVICE, CHUNK_SAMPLE):
        assert chunk_dev is not None and chunk_dev.dtype == torch.int32 and chunk_dev.is_cuda
    if chunk_mode == CHUNK_SAMPLE:
        assert ctr is not None and ctr.dtype == torch.int64 and ctr.is_cuda
    for k, n in (("ys_in", B * (L + 1)), ("tgt", B * (L + 1)), ("tgt_ctc", B * L), ("pred_len", B), ("ylen", B)):
        assert out[k].dtype == torch.int32 and out[k].numel() == n and out[k].is_contiguous(), k
    N.call("lasr_u2_prep_chunk", ptr(xlens), ptr(ys), ptr(ylens), B, L, Tsub, sos, eos, chunk_mode,
           int(chunk) if chunk_mode == CHUNK_FIXED else 0, ptr(chunk_dev), ptr(ctr), int(chunk_seed), int(chunk_max),
           ptr(out["ys_in"]), ptr(out["tgt"]), ptr(out["tgt_ctc"]), ptr(dm), dm.shape[-1],
           ptr(em), ptr(cm), cld, ptr(out["pred_len"]), ptr(out["ylen"]), stream())


def spec_augment(x, xlens, plan, replace_with_zero=False, out=None):
    """Batched SpecAugment (csrc/specaug.hip) on a padded fp32 [B, T, F] device batch."""
    B, T, F = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert xlens.dtype == torch.int64 and xlens.numel() == B and xlens.device == x.device
    assert plan.dtype == torch.int32 and plan.dim() == 2 and plan.shape[0] == B and plan.is_contiguous()
    assert plan.device == x.device
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous()
    nbytes = N.load().lasr_spec_augment_ws_bytes(B, T)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    N.call("lasr_spec_augment", ptr(x), ptr(out), ptr(xlens), ptr(plan), plan.shape[1], B, T, F,
           int(bool(replace_with_zero)), ptr(ws), nbytes, stream())
    return out


def sumsq_nparts(n):
    return N.load().lasr_sumsq_nparts(n)


def sumsq_partial(g, ws):
    N.call("lasr_sumsq_partial", ptr(g), g.numel(), ptr(ws), ws.numel(), stream())


def adam_step(param, param_lp, grad, m, v, ws, nparts, state, max_norm, lr_mode, lr, factor,
              model_dim, warmup, beta1, beta2, eps, weight_decay):
    N.call("lasr_adam_step", ptr(param), ptr(param_lp),
           dt(param_lp) if param_lp is not None else 0, ptr(grad), ptr(m), ptr(v), param.numel(),
           ptr(ws), nparts, ptr(state), max_norm, lr_mode, lr, factor, model_dim, warmup, beta1,
           beta2, eps, weight_decay, stream())


def set_dropout_counter(ctr):
    N.call("lasr_set_dropout_counter", ptr(ctr))


def counter_add(ctr, v=1):
    N.call("lasr_counter_add", ptr(ctr), int(v), stream())


def logsoftmax_topk(logits, k, rows=None, ld=None, gather_idx=None):
    """Per row of ``logits`` (2-D, unit column stride; ``rows``/``ld`` override the row
    count/stride to walk a strided subset): log_softmax, then the k largest log-probs
    (descending, ties to the smaller index) and/or log_softmax gathered at
    ``gather_idx[r]`` (int32, -inf outside [0,V)).  Returns (vals f32 [rows,k],
    idx i32 [rows,k], gathered f32 [rows] or None)."""
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logsoftmax_topk: logits must be 2-D with unit column stride")
    rows = logits.shape[0] if rows is None else int(rows)
    ld = logits.stride(0) if ld is None else int(ld)
    V = logits.shape[1]
    dev = logits.device
    if (rows - 1) * ld + V > logits.untyped_storage().nbytes() // logits.element_size() - logits.storage_offset():
        raise ValueError("logsoftmax_topk: rows/ld walk past the logits storage")
    vals = torch.empty(rows, k, dtype=torch.float32, device=dev)
    idx = torch.empty(rows, k, dtype=torch.int32, device=dev)
    gat = None
    if gather_idx is not None:
        if gather_idx.dtype != torch.int32 or gather_idx.numel() != rows or not gather_idx.is_contiguous():
            raise ValueError("logsoftmax_topk: gather_idx must be contiguous int32 [rows]")
        gat = torch.empty(rows, dtype=torch.float32, device=dev)
    N.call("lasr_logsoftmax_topk", ptr(logits), dt(logits), rows, V, ld, k, ptr(gather_idx),
           ptr(vals) if k > 0 else None, ptr(idx) if k > 0 else None, ptr(gat), stream())
    return vals, idx, gat


# ------------------------------------------------------------ Paraformer CIF ---
def cif_fwd(z, plen, ylen, h, B, T, U, st):
    """Integrate-and-fire forward (lasr_cif_fwd); st: SimpleNamespace receiving alpha, acc,
    fired, row, sum_alpha, mae and out ([B, U, D] fp32)."""
    D = h.shape[-1]
    a = N.CifArgs()
    a.B, a.T, a.D, a.U = B, T, D, U
    a.z, a.plen, a.ylen, a.h = ptr(z), ptr(plen), ptr(ylen), ptr(h)
    a.alpha, a.acc, a.fired, a.row = ptr(st.alpha), ptr(st.acc), ptr(st.fired), ptr(st.row)
    a.sum_alpha, a.mae, a.out = ptr(st.sum_alpha), ptr(st.mae), ptr(st.out)
    N.call("lasr_cif_fwd", C.byref(a), stream())


def cif_bwd(plen, ylen, h, B, T, U, st, gout, gsum, dz, dh):
    D = h.shape[-1]
    a = N.CifArgs()
    a.B, a.T, a.D, a.U = B, T, D, U
    a.plen, a.ylen, a.h = ptr(plen), ptr(ylen), ptr(h)
    a.alpha, a.acc, a.fired, a.row, a.sum_alpha = ptr(st.alpha), ptr(st.acc), ptr(st.fired), ptr(st.row), \
        ptr(st.sum_alpha)
    a.gout, a.gsum, a.dz, a.dh = ptr(gout), ptr(gsum), ptr(dz), ptr(dh)
    N.call("lasr_cif_bwd", C.byref(a), stream())


def cif_infer(z, plen, h, st=None):
    """Inference-mode integrate-and-fire (lasr_cif_infer): z fp32 [B*T'] (any shape with B*T'
    elements), plen int32 [B], h fp32 [B, T', D] -> SimpleNamespace(alpha, acc, fired, row
    [B*T'], sum_alpha [B], ulen, count int32 [B], out [B, T', D] fp32), all on the device.
    st: a namespace of those buffers to write into (graph replays); allocated when None."""
    B, T, D = h.shape
    dev = h.device
    if z.dtype != torch.float32 or h.dtype != torch.float32 or plen.dtype != torch.int32:
        raise ValueError("cif_infer: z / h fp32 and plen int32")
    if z.numel() != B * T or plen.numel() != B or not (z.is_contiguous() and h.is_contiguous()):
        raise ValueError("cif_infer: z [B*T'], plen [B], h [B, T', D] contiguous")
    if st is None:
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        st = SimpleNamespace(alpha=e(B * T, torch.float32), acc=e(B * T, torch.float32), fired=e(B * T, torch.uint8),
                             row=e(B * T, torch.int32), sum_alpha=e(B, torch.float32), ulen=e(B, torch.int32),
                             count=e(B, torch.int32), out=e((B, T, D), torch.float32))
    a = N.CifInferArgs()
    a.B, a.T, a.D = B, T, D
    a.z, a.plen, a.h = ptr(z), ptr(plen), ptr(h)
    a.alpha, a.acc, a.fired, a.row = ptr(st.alpha), ptr(st.acc), ptr(st.fired), ptr(st.row)
    a.sum_alpha, a.ulen, a.count, a.out = ptr(st.sum_alpha), ptr(st.ulen), ptr(st.count), ptr(st.out)
    N.call("lasr_cif_infer", C.byref(a), stream())
    return st


def glancing_mix(replace, a, b, out, out2=None, backward=False):
    """fwd: out = replace ? a : b; bwd (a = incoming gradient): out / out2 = the
    embedding / CIF branch gradients.  fp32 [rows, D], replace u8 [rows]."""
    rows, D = out.shape
    N.call("lasr_glancing_mix", rows, D, ptr(replace), ptr(a), ptr(b), ptr(out), ptr(out2), int(backward),
           stream())


# ------------------------------------------------------------------ transducer ---
def rnnt_fwd(logits, targets, ilen, tlen, blank, lse, lp, alpha, beta, nll):
    """RNN-T lattice forward (lasr_rnnt_fwd): logits [B, T, U1, V] (rows unit-stride, evenly
    spaced), targets int32 [B, Lmax >= U1-1], ilen / tlen int32 [B]."""
    B, T, U1, V = logits.shape
    N.call("lasr_rnnt_fwd", ptr(logits), dt(logits), B, T, U1, V, _rows_ld(logits, 3), ptr(targets), targets.shape[1],
           ptr(ilen), ptr(tlen), blank, ptr(lse), ptr(lp), ptr(alpha), ptr(beta), ptr(nll), stream())


def rnnt_bwd(logits, targets, ilen, tlen, blank, lse, lp, alpha, beta, nll, grad, gscale, gdev=None):
    B, T, U1, V = logits.shape
    ld = _rows_ld(logits, 3)
    assert grad.shape == logits.shape and _rows_ld(grad, 3) == ld
    N.call("lasr_rnnt_bwd", ptr(logits), dt(logits), B, T, U1, V, ld, ptr(targets), targets.shape[1], ptr(ilen),
           ptr(tlen), blank, ptr(lse), ptr(lp), ptr(alpha), ptr(beta), ptr(nll), ptr(grad), dt(grad), gscale,
           ptr(gdev), stream())


def joint_fwd(e, d, B, T, U1, z):
    """z[(b T + t) U1 + u] = tanh(e[b T + t] + d[u B + b]) (lasr_joint_fwd); e, d fp32."""
    J = e.shape[1]
    assert e.is_contiguous() and d.is_contiguous() and z.is_contiguous() and e.dtype == d.dtype == torch.float32
    N.call("lasr_joint_fwd", ptr(e), ptr(d), B, T, U1, J, ptr(z), dt(z), stream())


def joint_reduce(dz, B, T, U1, de, dd):
    J = dz.shape[1]
    assert dz.is_contiguous() and de.is_contiguous() and dd.is_contiguous() and de.dtype == dd.dtype
    N.call("lasr_joint_reduce", ptr(dz), dt(dz), B, T, U1, J, ptr(de), ptr(dd), dt(de), stream())


def lstm_cell_fwd(gates, bias, c_prev, c_out, h_out):
    """gates [B, >=4H] fp32 (row stride any), h_out [B, H] (row stride any)."""
    B, H = c_out.shape
    N.call("lasr_lstm_cell_fwd", ptr(gates), gates.stride(0), ptr(bias), ptr(c_prev), B, H, ptr(c_out), ptr(h_out),
           dt(h_out), h_out.stride(0), stream())


def lstm_cell_bwd(gates, bias, c, c_prev, dh_out, dh_rec, dc_next, dgates, dc_prev):
    B, H = c.shape
    N.call("lasr_lstm_cell_bwd", ptr(gates), gates.stride(0), ptr(bias), ptr(c), ptr(c_prev), ptr(dh_out),
           dt(dh_out) if dh_out is not None else 0, dh_out.stride(0) if dh_out is not None else 0, ptr(dh_rec),
           ptr(dc_next), B, H, ptr(dgates), dt(dgates), dgates.stride(0), ptr(dc_prev), stream())


# -------------------------------------------------- transducer beam search ---
def rnnt_search_workspace(Tcap, layers, H, J, V, node_cap=0, slot_cap=0):
    """Arena bytes of the device-resident transducer search (lasr_rnnt_search_workspace;
    host only).  node_cap / slot_cap <= 0: the worst case 100 Tcap + 1 / 10 Tcap + 1."""
    return int(N.load().lasr_rnnt_search_workspace(Tcap, layers, H, J, V, node_cap, slot_cap))


def rnnt_search_args(arena, Tcap, node_cap, slot_cap, embed, layers, Wd, Wj, bj, enc_proj):
    """The argument block of lasr_rnnt_search_init / _expand (transducer.py:137-206).
    layers: [(Wih, Whh, bih, bhh)]; Wih / Whh / Wd / Wj share one dtype (fp32 or bf16), embed,
    the biases and enc_proj [Tcap, J] are fp32; arena: uint8 tensor of
    rnnt_search_workspace(...) bytes.  The block holds raw pointers: the caller keeps the
    tensors alive."""
    a = N.RnntSearchArgs()
    H, J, V = layers[0][1].shape[1], Wd.shape[0], Wj.shape[0]
    if len(layers) > N.RNNT_SEARCH_MAX_LAYERS:
        raise ValueError(f"rnnt_search: at most {N.RNNT_SEARCH_MAX_LAYERS} LSTM layers")
    ws = [w for l in layers for w in l[:2]] + [Wd, Wj]
    if any(w.dtype != Wd.dtype or not w.is_contiguous() for w in ws):
        raise ValueError("rnnt_search: the weight matrices must be contiguous and share one dtype")
    f32 = [embed, bj, enc_proj] + [b for l in layers for b in l[2:]]
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in f32):
        raise ValueError("rnnt_search: embed, biases and enc_proj must be contiguous fp32")
    if tuple(enc_proj.shape) != (Tcap, J) or Wd.shape[1] != H or Wj.shape[1] != J or embed.shape[0] != V:
        raise ValueError("rnnt_search: inconsistent shapes")
    if arena.dtype != torch.uint8 or arena.numel() < rnnt_search_workspace(Tcap, len(layers), H, J, V, node_cap,
                                                                           slot_cap):
        raise ValueError("rnnt_search: arena too small")
    a.Tcap, a.layers, a.dec_dim, a.H, a.J, a.V = Tcap, len(layers), embed.shape[1], H, J, V
    a.node_cap, a.slot_cap, a.w_dtype = node_cap, slot_cap, dt(Wd)
    a.arena, a.arena_bytes = ptr(arena), arena.numel()
    a.embed = ptr(embed)
    for i, (Wih, Whh, bih, bhh) in enumerate(layers):
        if tuple(Wih.shape) != (4 * H, embed.shape[1] if i == 0 else H) or tuple(Whh.shape) != (4 * H, H):
            raise ValueError("rnnt_search: inconsistent LSTM shapes")
        a.Wih[i], a.Whh[i], a.bih[i], a.bhh[i] = ptr(Wih), ptr(Whh), ptr(bih), ptr(bhh)
    a.Wd, a.Wj, a.bj, a.enc_proj = ptr(Wd), ptr(Wj), ptr(bj), ptr(enc_proj)
    return a


def rnnt_search_init(args, Tp):
    """Empty trie, root hypothesis [0] popped (one launch)."""
    N.call("lasr_rnnt_search_init", C.byref(args), Tp, stream())


def rnnt_search_expand(args, mode=0):
    """The launches of one expansion (LSTM layers + lin_dec + joint + finalise); mode 1
    stops after the candidates (host-loop driver)."""
    N.call("lasr_rnnt_search_expand", C.byref(args), mode, stream())


# ----------------------------------------------- attention rescoring on the device ---
def rescore_workspace(Tcap, Lcap):
    """Arena bytes of the device-resident rescoring (lasr_rescore_workspace)."""
    return int(N.load().lasr_rescore_workspace(int(Tcap), int(Lcap)))


def _rescore_arena(arena, Tcap, Lcap, who, *others):
    """The arena's size, and that it and every other tensor handed to the kernel live on one HIP
    device (the kernels take raw pointers)."""
    if arena.dtype != torch.uint8 or not arena.is_contiguous() or arena.numel() < rescore_workspace(Tcap, Lcap):
        raise ValueError(f"{who}: arena must be contiguous uint8 of rescore_workspace(Tcap, Lcap) bytes")
    if not arena.is_cuda or any(t.device != arena.device for t in others):
        raise ValueError(f"{who}: the arena and every tensor must be on the same HIP device")


def rescore_search(arena, Tcap, Lcap, vals, idx, tp_dev, blank, beam=10):
    """CTC prefix beam search over the candidates vals / idx [>= Tcap, k] (lasr_rescore_search);
    tp_dev: int32 device word holding T'.  The result block at the head of the arena receives
    n, the lengths, double scores and tokens."""
    _rescore_arena(arena, Tcap, Lcap, "rescore_search", vals, idx, tp_dev)
    if vals.dtype != torch.float32 or idx.dtype != torch.int32 or vals.shape != idx.shape or vals.dim() != 2 \
            or not vals.is_contiguous() or not idx.is_contiguous():
        raise ValueError("rescore_search: vals f32 / idx i32, contiguous [rows, k]")
    if vals.shape[0] < Tcap:
        raise ValueError(f"rescore_search: {vals.shape[0]} candidate rows < Tcap = {Tcap}")
    if tp_dev.dtype != torch.int32 or tp_dev.numel() < 1:
        raise ValueError("rescore_search: tp_dev must be an int32 device word")
    N.call("lasr_rescore_search", ptr(arena), arena.numel(), Tcap, Lcap, vals.shape[1], int(blank), int(beam),
           ptr(vals), ptr(idx), ptr(tp_dev), stream())


def rescore_prep(arena, Tcap, Lcap, sos, eos, ys_in, dec_mask, gather_idx, mem_mask):
    """Decoder inputs of the n-best in the arena (lasr_rescore_prep): ys_in i32 [10, L1cap],
    dec_mask u8 [10, L1cap, >= L1cap] (row stride = its stride(1)), gather_idx i32 [10 L1cap],
    mem_mask u8 [10, Tcap]."""
    _rescore_arena(arena, Tcap, Lcap, "rescore_prep", ys_in, dec_mask, gather_idx, mem_mask)
    L1 = Lcap + 1
    ld = dec_mask.stride(1)
    if (ys_in.dtype != torch.int32 or tuple(ys_in.shape) != (10, L1) or not ys_in.is_contiguous()
            or gather_idx.dtype != torch.int32 or gather_idx.numel() != 10 * L1 or not gather_idx.is_contiguous()
            or mem_mask.dtype != torch.uint8 or tuple(mem_mask.shape) != (10, Tcap) or not mem_mask.is_contiguous()
            or dec_mask.dtype != torch.uint8 or tuple(dec_mask.shape[:2]) != (10, L1) or dec_mask.shape[2] < L1
            or dec_mask.stride(2) != 1 or dec_mask.stride(0) != L1 * ld or ld < L1):
        raise ValueError("rescore_prep: output shapes / dtypes")
    if (10 * L1 - 1) * ld + ld > dec_mask.untyped_storage().nbytes() - dec_mask.storage_offset():
        raise ValueError("rescore_prep: dec_mask rows walk past its storage")
    N.call("lasr_rescore_prep", ptr(arena), arena.numel(), Tcap, Lcap, int(sos), int(eos), ptr(ys_in), ptr(dec_mask),
           ld, ptr(gather_idx), ptr(mem_mask), stream())


def rescore_pick(arena, Tcap, Lcap, gathered, ctc_weight):
    """Best hypothesis from the gathered attention log-probs f32 [10 L1cap] (lasr_rescore_pick)."""
    _rescore_arena(arena, Tcap, Lcap, "rescore_pick", gathered)
    if gathered.dtype != torch.float32 or gathered.numel() != 10 * (Lcap + 1) or not gathered.is_contiguous():
        raise ValueError("rescore_pick: gathered must be contiguous f32 [10 (Lcap + 1)]")
    N.call("lasr_rescore_pick", ptr(arena), arena.numel(), Tcap, Lcap, ptr(gathered), float(ctc_weight), stream())


def rescore_workspace_batch(B, Tcap, Lcap):
    """Bytes of the batch arena: B single-utterance arenas laid end to end, stride
    rescore_workspace(Tcap, Lcap) (lasr_rescore_workspace_batch)."""
    return int(N.load().lasr_rescore_workspace_batch(int(B), int(Tcap), int(Lcap)))


def _rescore_arena_batch(arena, B, Tcap, Lcap, who, *others):
    need = rescore_workspace_batch(B, Tcap, Lcap)
    if B < 1 or need == 0:
        raise ValueError(f"{who}: B = {B} is not a batch the kernels take")
    if arena.dtype != torch.uint8 or not arena.is_contiguous() or arena.numel() < need:
        raise ValueError(f"{who}: arena must be contiguous uint8 of rescore_workspace_batch(B, Tcap, Lcap) bytes")
    if not arena.is_cuda or any(t.device != arena.device for t in others):
        raise ValueError(f"{who}: the arena and every tensor must be on the same HIP device")


def rescore_search_batch(arena, B, Tcap, Lcap, vals, idx, tp_dev, blank, beam=10):
    """B CTC prefix beam searches in one launch (lasr_rescore_search_batch): utterance b reads the
    candidates vals / idx [b Tcap, (b + 1) Tcap) of [>= B Tcap, k] and T' = tp_dev[b] (int32 [>= B]
    on the device) and writes arena b of the batch arena."""
    _rescore_arena_batch(arena, B, Tcap, Lcap, "rescore_search_batch", vals, idx, tp_dev)
    if vals.dtype != torch.float32 or idx.dtype != torch.int32 or vals.shape != idx.shape or vals.dim() != 2 \
            or not vals.is_contiguous() or not idx.is_contiguous():
        raise ValueError("rescore_search_batch: vals f32 / idx i32, contiguous [rows, k]")
    if vals.shape[0] < B * Tcap:
        raise ValueError(f"rescore_search_batch: {vals.shape[0]} candidate rows < B Tcap = {B * Tcap}")
    if tp_dev.dtype != torch.int32 or tp_dev.numel() < B or not tp_dev.is_contiguous():
        raise ValueError("rescore_search_batch: tp_dev must be B contiguous int32 device words")
    N.call("lasr_rescore_search_batch", ptr(arena), arena.numel(), B, Tcap, Lcap, vals.shape[1], int(blank),
           int(beam), ptr(vals), ptr(idx), ptr(tp_dev), stream())


def rescore_prep_batch(arena, B, Tcap, Lcap, sos, eos, ys_in, dec_mask, gather_idx, mem_mask, mem_len):
    """Decoder inputs of the B n-bests (lasr_rescore_prep_batch): ys_in i32 [10 B, L1cap], dec_mask
    u8 [10 B, L1cap, >= L1cap] (row stride = its stride(1)), gather_idx i32 [10 B L1cap], mem_mask
    u8 [10 B, Tcap]; utterance b owns rows [10 b, 10 b + 10), and its memory mask is 1 at frames
    >= mem_len[b] (int32 [B] on the device)."""
    _rescore_arena_batch(arena, B, Tcap, Lcap, "rescore_prep_batch", ys_in, dec_mask, gather_idx, mem_mask, mem_len)
    L1, R = Lcap + 1, 10 * B
    ld = dec_mask.stride(1)
    if (ys_in.dtype != torch.int32 or tuple(ys_in.shape) != (R, L1) or not ys_in.is_contiguous()
            or gather_idx.dtype != torch.int32 or gather_idx.numel() != R * L1 or not gather_idx.is_contiguous()
            or mem_mask.dtype != torch.uint8 or tuple(mem_mask.shape) != (R, Tcap) or not mem_mask.is_contiguous()
            or dec_mask.dtype != torch.uint8 or tuple(dec_mask.shape[:2]) != (R, L1) or dec_mask.shape[2] < L1
            or dec_mask.stride(2) != 1 or dec_mask.stride(0) != L1 * ld or ld < L1
            or mem_len.dtype != torch.int32 or mem_len.numel() != B or not mem_len.is_contiguous()):
        raise ValueError("rescore_prep_batch: output shapes / dtypes")
    if R * L1 * ld > dec_mask.untyped_storage().nbytes() - dec_mask.storage_offset():
        raise ValueError("rescore_prep_batch: dec_mask rows walk past its storage")
    N.call("lasr_rescore_prep_batch", ptr(arena), arena.numel(), B, Tcap, Lcap, int(sos), int(eos), ptr(ys_in),
           ptr(dec_mask), ld, ptr(gather_idx), ptr(mem_mask), ptr(mem_len), stream())


def rescore_pick_batch(arena, B, Tcap, Lcap, gathered, ctc_weight):
    """Best hypothesis of each utterance from the gathered attention log-probs f32 [10 B L1cap]
    (lasr_rescore_pick_batch)."""
    _rescore_arena_batch(arena, B, Tcap, Lcap, "rescore_pick_batch", gathered)
    if gathered.dtype != torch.float32 or gathered.numel() != 10 * B * (Lcap + 1) or not gathered.is_contiguous():
        raise ValueError("rescore_pick_batch: gathered must be contiguous f32 [10 B (Lcap + 1)]")
    N.call("lasr_rescore_pick_batch", ptr(arena), arena.numel(), B, Tcap, Lcap, ptr(gathered), float(ctc_weight),
           stream())


# ------------------------------------------------------------------ wav2vec 2.0 ---
def w2v_conv0_fwd(x, w, bias, k, s, y):
    """Extractor layer 0 (lasr_w2v_conv0_fwd): x [B, T_in] fp32 -> y [B, T_out, C] fp32."""
    B, Tin = x.shape
    N.call("lasr_w2v_conv0_fwd", ptr(x), B, Tin, y.shape[2], k, s, ptr(w), ptr(bias), ptr(y), stream())


def w2v_conv0_dw(x, dy, k, s, dw):
    """dw [C, k] += layer 0's weight gradient, fixed order (lasr_w2v_conv0_dw)."""
    B, Tin = x.shape
    Cc = dy.shape[2]
    ws = WS.get(N.load().lasr_w2v_conv0_dw_parts(B, dy.shape[1]) * Cc * k, x.device)
    N.call("lasr_w2v_conv0_dw", ptr(x), ptr(dy), dt(dy), B, Tin, Cc, k, s, ptr(dw), ptr(ws), ws.numel(), stream())


def w2v_ln_act_fwd(x, gamma, beta, eps, act, y, mean, rstd):
    """y = act(LayerNorm(x)) over the last dim, fp32 statistics; act 1 = exact GELU."""
    Cc = x.shape[-1]
    N.call("lasr_w2v_ln_act_fwd", ptr(x), dt(x), x.numel() // Cc, Cc, ptr(gamma), ptr(beta), float(eps), int(act),
           ptr(y), dt(y), ptr(mean), ptr(rstd), stream())


def w2v_ln_act_bwd(x, dy, gamma, beta, mean, rstd, act, dx, dgamma, dbeta):
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    ws = WS.get((rows + 63) // 64 * 2 * Cc, x.device)
    N.call("lasr_w2v_ln_act_bwd", ptr(x), dt(x), ptr(dy), dt(dy), rows, Cc, ptr(gamma), ptr(beta), ptr(mean),
           ptr(rstd), int(act), ptr(dx), dt(dx), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream())


def w2v_col2im1d(dcol, Tin, Cc, k, s, dx):
    B, Tout = dcol.shape[0], dcol.shape[1]
    N.call("lasr_w2v_col2im1d", ptr(dcol), dt(dcol), B, Tin, Tout, Cc, k, s, ptr(dx), stream())


def w2v_group_pack(src, G, front, dst, yg=None, bias=None):
    """dst [G, B, Tp, cg] <- src [B, T, G cg] fp32 at rows front.., zeros elsewhere (x GELU'(yg + bias))."""
    B, T, d = src.shape
    N.call("lasr_w2v_group_pack", ptr(src), B, T, G, d // G, front, dst.shape[2], ptr(yg),
           dt(yg) if yg is not None else 0, ptr(bias), ptr(dst), dt(dst), stream())


def w2v_group_unpack(yg, bias, act, res, out):
    G, B, T, cg = yg.shape
    N.call("lasr_w2v_group_unpack", ptr(yg), dt(yg), ptr(bias), int(act), ptr(res), B, T, G, cg, ptr(out), stream())


def w2v_group_colsum(x, out):
    G, cg = x.shape[0], x.shape[-1]
    N.call("lasr_w2v_group_colsum", ptr(x), dt(x), G, x.numel() // (G * cg), cg, ptr(out), stream())


def w2v_mask_fwd(x, midx, emb):
    B, T, d = x.shape
    N.call("lasr_w2v_mask_fwd", ptr(x), ptr(midx), B, T, midx.shape[1], d, ptr(emb), stream())


def w2v_mask_bwd(dx, midx, demb):
    B, T, d = dx.shape
    N.call("lasr_w2v_mask_bwd", ptr(dx), ptr(midx), B, T, midx.shape[1], d, ptr(demb), stream())


def w2v_gather_rows(src, midx, dst, time_major=False):
    """dst [B, M, d] = rows midx of src ([B, T, d], or [T, B, d] when time_major)."""
    d = src.shape[2]
    B, T = (src.shape[1], src.shape[0]) if time_major else (src.shape[0], src.shape[1])
    sb, st = (d, B * d) if time_major else (T * d, d)
    N.call("lasr_w2v_gather_rows", ptr(src), dt(src), sb, st, ptr(midx), B, T, midx.shape[1], d, ptr(dst), dt(dst),
           stream())


def w2v_scatter_rows(src, midx, dst, time_major=False, accumulate=False):
    d = dst.shape[2]
    B, T = (dst.shape[1], dst.shape[0]) if time_major else (dst.shape[0], dst.shape[1])
    sb, st = (d, B * d) if time_major else (T * d, d)
    N.call("lasr_w2v_scatter_rows", ptr(src), dt(src), ptr(midx), B, T, midx.shape[1], d, ptr(dst), sb, st,
           int(accumulate), stream())


def w2v_gumbel_fwd(logits, G, vars_, tau, hard, out, codes, noise=None, seed=0):
    R = logits.shape[0]
    V = logits.shape[1] // G
    N.call("lasr_w2v_gumbel_fwd", ptr(logits), dt(logits), ptr(noise), seed, float(tau), int(hard), R, G, V,
           ptr(vars_), vars_.shape[-1], ptr(out), dt(out), ptr(codes), stream())


def w2v_gumbel_bwd(logits, G, vars_, tau, hard, dout, codes, dlogits, dvars, noise=None, seed=0):
    R = logits.shape[0]
    V = logits.shape[1] // G
    N.call("lasr_w2v_gumbel_bwd", ptr(logits), dt(logits), ptr(noise), seed, float(tau), int(hard), R, G, V,
           ptr(vars_), vars_.shape[-1], ptr(dout), dt(dout), ptr(codes), ptr(dlogits), dt(dlogits), ptr(dvars),
           stream())


def w2v_contrast_fwd(x, y, neg, codes, Nneg, temp, logits, lse, row_loss, loss):
    B, M, D = x.shape
    N.call("lasr_w2v_contrast_fwd", ptr(x), ptr(y), ptr(neg), ptr(codes), codes.shape[-1], B, M, Nneg, D,
           float(temp), ptr(logits), ptr(lse), ptr(row_loss), ptr(loss), stream())


def w2v_contrast_bwd(x, y, neg, codes, Nneg, temp, lse, gout, dx, dy):
    B, M, D = x.shape
    ws = torch.empty(B * M * (Nneg + 1) * 2, dtype=torch.float32, device=x.device)
    N.call("lasr_w2v_contrast_bwd", ptr(x), ptr(y), ptr(neg), ptr(codes), codes.shape[-1], B, M, Nneg, D,
           float(temp), ptr(lse), ptr(gout), ptr(dx), ptr(dy), ptr(ws), ws.numel(), stream())
