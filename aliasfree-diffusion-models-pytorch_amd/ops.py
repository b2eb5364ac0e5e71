"""torch.autograd.Function shells around the C ABI (include/afd.h).

torch is used for device memory, the current HIP stream and the autograd graph -- every FLOP and
every byte moved on the device goes through libafd_hip.so.  All tensors are fp32, NCHW,
contiguous, on a HIP device; anything else raises (there is no CPU / eager fallback).
"""
import weakref

import numpy as np
import os
import torch

from ._lib import AfdError, lib

GN_EPS = 1e-5
LN_EPS = 1e-5
NULL_LABEL = -1      # class label of a row that carries none (classifier-free guidance): UNet.forward adds no label embedding to it


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def _stream():
    """Raw handle of torch's current HIP stream.  torch.cuda.current_stream() builds a Stream object and walks the
    device-index helpers on every call: 2.5 ms of host time per train step over ~470 launches (tools/host_profile.py);
    the raw getter is one C call."""
    if _raw_stream is not None:
        return _raw_stream(_get_device())
    return torch.cuda.current_stream().cuda_stream


def _chk(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise AfdError("afdm: the HIP engine needs tensors on a HIP device (got a CPU tensor); "
                           "there is no CPU fallback -- move the model and its inputs to 'cuda'")
        if t.dtype != torch.float32:
            raise AfdError(f"afdm: fp32 only (got {t.dtype})")


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


class Taps:
    """Host copy of an N x N filter: the kernels take taps as launch arguments, so there is no
    per-call H2D copy (the reference does one per call: filtrs.py:73,91)."""

    def __init__(self, k):
        a = k.detach().cpu().numpy() if isinstance(k, torch.Tensor) else np.asarray(k)
        self.arr = np.ascontiguousarray(a, dtype=np.float32)
        assert self.arr.ndim == 2 and self.arr.shape[0] == self.arr.shape[1]
        self.N = int(self.arr.shape[0])
        self.ptr = self.arr.ctypes.data

    @staticmethod
    def of(k):
        return k if isinstance(k, Taps) else Taps(k)


# ---------------------------------------------------------------------------------------------
# F2 / F3 filtered resampling
# ---------------------------------------------------------------------------------------------

class _NoCtx:
    """Stand-in for the autograd context when gradients are off (sampling): forward() may set attributes and call
    save_for_backward; nothing is kept."""
    needs_input_grad = (False,) * 16

    def save_for_backward(self, *tensors):
        pass

    def mark_non_differentiable(self, *tensors):
        pass

    def mark_dirty(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


class _Fn(torch.autograd.Function):
    """autograd.Function whose apply() skips the autograd machinery under no_grad: Function.apply costs ~8 us of host
    time per call, and with four sampling trajectories in flight (4 x ~130 calls per round) the host is the bound."""

    @classmethod
    def apply(cls, *args):
        if torch.is_grad_enabled():
            return super().apply(*args)
        return cls.forward(_NoCtx(), *args)

class FiltUp2(_Fn):
    @staticmethod
    def forward(ctx, x, taps):
        _chk(x)
        x = _c(x)
        B, C, H, W = x.shape
        y = torch.empty(B, C, 2 * H, 2 * W, device=x.device, dtype=torch.float32)
        lib().afd_filt_up2_fwd(_p(x), _p(y), B, C, H, W, 0, 0, taps.ptr, taps.N, _stream())
        ctx.taps, ctx.shape = taps, (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _c(dy)
        dx = torch.empty(B, C, H, W, device=dy.device, dtype=torch.float32)
        lib().afd_filt_up2_bwd(_p(dy), _p(dx), B, C, H, W, 0, 0, ctx.taps.ptr, ctx.taps.N, _stream())
        return dx, None


class FiltDown2(_Fn):
    @staticmethod
    def forward(ctx, x, taps):
        _chk(x)
        x = _c(x)
        B, C, H, W = x.shape
        y = torch.empty(B, C, (H + 1) // 2, (W + 1) // 2, device=x.device, dtype=torch.float32)
        lib().afd_filt_down2_fwd(_p(x), _p(y), B, C, H, W, 0, 0, taps.ptr, taps.N, _stream())
        ctx.taps, ctx.shape = taps, (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _c(dy)
        dx = torch.empty(B, C, H, W, device=dy.device, dtype=torch.float32)
        lib().afd_filt_down2_bwd(_p(dy), _p(dx), B, C, H, W, 0, 0, ctx.taps.ptr, ctx.taps.N, _stream())
        return dx, None


def _act_ws(B, C, H, W, N, backward, device):
    nbytes = lib().afd_filt_act_workspace_bytes(B, C, H, W, N, backward)
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32) if nbytes else None


class FiltAct(_Fn):
    """y = down2(GELU(up2(x)))   (ddpm_utils.py:123-125) with no fused prologue."""

    @staticmethod
    def forward(ctx, x, tu, td):
        _chk(x)
        x = _c(x)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        ws = _act_ws(B, C, H, W, tu.N, 0, x.device)
        lib().afd_filt_act_fwd(_p(x), _p(y), B, C, H, W, None, None, None, None, tu.ptr, td.ptr, tu.N, _p(ws), _stream())
        ctx.save_for_backward(x)
        ctx.tu, ctx.td = tu, td
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, C, H, W = x.shape
        dy = _c(dy)
        dx = torch.empty_like(x)
        ws = _act_ws(B, C, H, W, ctx.tu.N, 1, x.device)
        lib().afd_filt_act_bwd(_p(x), _p(dy), _p(dx), B, C, H, W, None, None, None, None,
                               ctx.tu.ptr, ctx.td.ptr, ctx.tu.N, _p(ws), None, _stream())
        return dx, None, None


# ---------------------------------------------------------------------------------------------
# F6 GroupNorm(1, C) with fused epilogues / fused filtered GELU
# ---------------------------------------------------------------------------------------------
class _GradMode:
    """When `inplace` is set (by TrainStep around backward) the weight-gradient kernels ADD straight into
    the parameters' preallocated `.grad` (FlatParams views) and backward returns None for them: this skips
    ~180 tiny autograd accumulate-adds and as many allocations per step.  Off by default, so
    torch.autograd.grad / plain .backward() keep their usual semantics.

    `side` (a HIP stream, set by `inplace_param_grads(side_stream=...)`): the weight-gradient kernels of the
    convolutions are not on the critical path of backward (nothing downstream consumes dW), so they are launched on
    that stream -- forked after dY exists, joined by the caller before the optimizer -- and fill the CUs that the
    dependent chain of small dgrad / norm kernels leaves idle.  Legal under stream capture (fork / join by events)."""
    inplace = False
    side = None           # first side stream (None: no side stream) -- what the ops test to decide whether to defer
    sides = []            # all side streams: queued launches are dealt to them in turn (one in-order stream runs ONE
    #                       weight-gradient kernel at a time; two let a layer's slab reduce overlap the next layer's multiplies)
    turn = 0
    pending = []          # (launch closure, tensors it reads, params): parameter-gradient kernels not launched yet
    launched = []         # the same triples after launch, held until the join (their buffers are in use on the side stream)
    batch = 8             # fork the side stream once per this many layers (few cross-stream edges in a captured graph)
    on_write = None       # callable(list of Parameters): their .grad is complete as far as ENQUEUED work goes -- the
    #                       data-parallel exchange's readiness hook (training.GradAllReduce.wrote)
    fold_hint = None      # callable(list of Parameters) -> bool: would reporting these complete a data-parallel bucket?
    folds = []            # per side stream: [packed afd_fold_desc bytes, ...] of producers already launched there
    fold_writes = []      # params whose .grad is complete once the queued folds have been launched
    flushes = 0           # flushes since the last fold launch
    lane_of = {}          # data pointer of a .grad -> index of the side stream that writes it (for the life of the scope)
    fold_every = 2        # launch the queued folds every this many flushes (and at the join, and when a bucket completes)


def _wrote(*params):
    """Report parameters whose gradient the kernels enqueued so far (current stream + side stream) have fully written."""
    cb = _GradMode.on_write
    if cb is not None:
        cb([q for q in params if q is not None])


FOLD_DESC = "<QQqqqqii"      # afd_fold_desc: part, dst, n, stride, inner, rstride, splits, accumulate (56 bytes)


def fold_desc(part_ptr, dst_ptr, n, splits, stride=None, inner=None, rstride=1, accumulate=1):
    import struct
    return struct.pack(FOLD_DESC, part_ptr, dst_ptr, n, n if stride is None else stride, n if inner is None else inner, rstride,
                       splits, accumulate)


def fold_now(descs, stream=None):
    """One afd_fold_batched launch for packed descriptors (bytes)."""
    import ctypes
    buf = ctypes.create_string_buffer(descs, len(descs))
    lib().afd_fold_batched(ctypes.addressof(buf), len(descs) // 56, _stream() if stream is None else stream)


def defer_to_side_stream(fn, *keep, writes=()):
    """Queue fn(stream_handle) -- a launch whose result nothing downstream of backward consumes (a parameter gradient) --
    for the side stream.  `keep`: the tensors it reads; they are held until the join, so autograd cannot add into them
    in place and the allocator cannot recycle them while the side stream still reads them.  `writes`: the Parameters
    whose .grad the launch completes (reported to `on_write` once it is launched).
    fn may RETURN packed afd_fold_desc bytes: the deterministic fold that finishes its gradient.  Those are not launched
    per layer: they queue up on the producer's stream and ONE afd_fold_batched launch folds every `fold_every` flushes'
    worth of them (csrc/fold.hip; `writes` are then reported when that launch is enqueued).  fn = None with
    keep[0] = descriptor bytes queues a fold whose partials a main-stream kernel has already produced."""
    _GradMode.pending.append((fn, keep, writes))
    if len(_GradMode.pending) >= _GradMode.batch:
        flush_wgrads()


FOLD_MAX = 56                # descriptors per afd_fold_batched launch (kFoldMax of csrc/fold.hip)


def fold_batches(descs, limit=FOLD_MAX):
    """Partition packed afd_fold_desc bytes into the batches that may each travel in ONE afd_fold_batched launch: the order
    is kept, a batch holds at most `limit` descriptors, and no two descriptors of a batch have the same `dst`.  A fold
    reads dst, adds and writes it back without atomics (fold_batched_k), so two folds into one gradient -- a parameter used
    twice in one backward -- must be two launches on one stream.  A descriptor whose dst is already in the open batch closes
    it and starts the next.  Without repeats this is what fold_launch does by itself: cuts of `limit`, one batch for <= limit."""
    assert len(descs) % 56 == 0 and limit > 0
    out, cur, seen = [], [], set()
    for o in range(0, len(descs), 56):
        d = descs[o:o + 56]
        dst = d[8:16]
        if dst in seen or len(cur) == limit:
            out.append(b"".join(cur))
            cur, seen = [], set()
        cur.append(d)
        seen.add(dst)
    if cur:
        out.append(b"".join(cur))
    return out


def deal_lane(keys, lane_of, turn, n_lanes):
    """Side stream of one queued producer.  `keys`: the gradients it writes (data pointers); `lane_of`: pointer -> lane of
    everything queued before it in this scope (updated here).  The first writer of a gradient takes the round-robin lane
    `turn % n_lanes`; every later writer of the same gradient follows it, so all read-modify-writes of one .grad are on one
    in-order stream, in queue order.  -> (lane, conflict): conflict = the gradients it writes already live on DIFFERENT
    lanes (say a weight shared with one module and a bias shared with another); the caller must then order the lanes
    against each other before it launches this producer."""
    known = [lane_of[k] for k in keys if k in lane_of]
    lane = known[0] if known else turn % n_lanes
    conflict = any(l != lane for l in known)
    for k in keys:
        lane_of[k] = lane
    return lane, conflict


def _grad_keys(params):
    return [q.grad.data_ptr() for q in params if q is not None and q.grad is not None]


def _launch_folds():
    """Launch every queued fold, per side stream, in as many launches as fold_batches asks for."""
    G = _GradMode
    for k, side in enumerate(G.sides):
        if G.folds[k]:
            for batch in fold_batches(b"".join(G.folds[k])):
                fold_now(batch, side.cuda_stream)
            G.folds[k] = []
    done = G.fold_writes
    G.fold_writes, G.flushes = [], 0
    return done


def _launch_lanes(lanes, done):
    """Launch dealt producers, lane by lane (one fork per side stream); queue or launch the folds they return."""
    G = _GradMode
    cur = torch.cuda.current_stream()
    for k, (side, items) in enumerate(zip(G.sides, lanes)):
        if not items:
            continue
        side.wait_stream(cur)                                                 # fork: every queued dY (and the zeroed .grad) exists
        with torch.cuda.stream(side):
            h = side.cuda_stream
            for fn, keep, ws in items:
                descs = fn(h) if fn is not None else keep[0]
                if descs and G.fold_every == 0:                               # (A/B hook: one fold launch per producer, as in round 2)
                    for batch in fold_batches(descs):
                        fold_now(batch, h)
                    done.extend(ws)
                elif descs:
                    G.folds[k].append(descs)
                    G.fold_writes.extend(ws)
                else:
                    done.extend(ws)


def flush_wgrads(final=False):
    """Launch the queued parameter-gradient kernels on the side stream (one fork for the whole batch), then the queued
    folds if it is time: every `fold_every` flushes, at the join (final) and whenever they would complete a bucket."""
    G = _GradMode
    sides, q = G.sides, G.pending
    if not q and not (final and any(G.folds)):
        return
    if len(G.folds) != len(sides):
        G.folds = [[] for _ in sides]
    done = []
    lanes = [[] for _ in sides]
    for item in q:
        lane, conflict = deal_lane(_grad_keys(item[2]), G.lane_of, G.turn, len(sides))
        G.turn += 1
        if conflict:
            # its gradients were written on different lanes: finish what is dealt and folded so far, then order every
            # side stream behind every other one -- whatever comes later, on any lane, follows all earlier writes
            _launch_lanes(lanes, done)
            done.extend(_launch_folds())
            lanes = [[] for _ in sides]
            for a in sides:
                for b in sides:
                    if a is not b:
                        a.wait_stream(b)
        lanes[lane].append(item)
    _launch_lanes(lanes, done)
    G.launched.extend(q)
    G.pending = []
    G.flushes += 1
    if any(G.folds) and (final or G.flushes >= max(1, G.fold_every) or (G.fold_hint is not None and G.fold_hint(G.fold_writes + done))):
        done.extend(_launch_folds())
    if G.on_write is not None and done:
        _wrote(*done)


class inplace_param_grads:
    """Scope in which the parameter-gradient kernels ADD into the preallocated `.grad` tensors (see _GradMode), optionally
    queued for one or more side streams and finished by batched folds.

    A parameter used twice in one backward (tied weights, a module called twice) is safe: every queued producer and fold
    that writes one `.grad` runs on the side stream its first writer was dealt to, in queue order (deal_lane), and two folds
    into one `.grad` never share a launch (fold_batches).  A model without repeated parameters sees the same streams,
    the same launch order and the same number of launches as before.  Not ordered against the queued work: a producer
    that must run on the main stream because the same launch produces a gradient the chain consumes (SiluLinear with a
    time embedding that needs a gradient, EmbedAdd) -- tie such a parameter only with other main-stream uses.

    `on_write` / `fold_hint` (the data-parallel readiness hook) know nothing of repeated parameters: a tied parameter is
    reported after EACH of its uses, so a bucket that holds it may be reported before its last contribution is enqueued.

    A parameter without a preallocated contiguous fp32 `.grad`, or a plain tensor in a parameter's place, takes the
    out-of-place path inside the scope: its gradient is returned to autograd."""

    def __init__(self, side_stream=None, batch=8, on_write=None, fold_hint=None, fold_every=None):
        self.side_stream, self.batch, self.on_write, self.fold_hint = side_stream, batch, on_write, fold_hint
        self.fold_every = int(os.environ.get("AFD_FOLD_EVERY", 2)) if fold_every is None else fold_every

    def __enter__(self):
        G = _GradMode
        self.prev = (G.inplace, G.side, G.sides, G.on_write, G.fold_hint, G.fold_every)
        ss = self.side_stream
        self.streams = [] if ss is None else (list(ss) if isinstance(ss, (list, tuple)) else [ss])
        G.inplace, G.batch, G.on_write, G.fold_hint, G.fold_every = True, self.batch, self.on_write, self.fold_hint, max(0, self.fold_every)
        G.sides, G.side, G.turn = self.streams, (self.streams[0] if self.streams else None), 0
        G.folds, G.fold_writes, G.flushes, G.lane_of = [[] for _ in self.streams], [], 0, {}

    def __exit__(self, exc_type, *a):
        G = _GradMode
        if self.streams:
            if exc_type is not None:
                G.pending, G.folds, G.fold_writes = [], [[] for _ in self.streams], []      # backward failed: drop what was queued
            flush_wgrads(final=True)
            for st in self.streams:
                torch.cuda.current_stream().wait_stream(st)                  # join: every dW is in .grad
            G.launched = []                                                  # buffers may be freed now (main-stream order)
        G.lane_of = {}
        G.inplace, G.side, G.sides, G.on_write, G.fold_hint, G.fold_every = self.prev


def _direct(*params):
    """True if every given parameter has a contiguous preallocated .grad we may accumulate into."""
    if not _GradMode.inplace:
        return False
    for q in params:
        if q is None:
            continue
        g = q.grad
        if g is None or not g.is_contiguous() or g.dtype != torch.float32:
            return False
    return True


def _gn_param_targets(C, gamma, beta, device):
    """Where a normalisation backward's tail writes dgamma / dbeta: straight into the parameters' .grad (in-place
    mode, accumulate = 1) or into a fresh (2, C) pair returned to autograd.  -> (dg, db, accumulate, returned pair)"""
    if gamma is not None and beta is not None and _direct(gamma, beta):
        return gamma.grad, beta.grad, 1, (None, None)
    out = torch.empty(2, C, device=device, dtype=torch.float32)
    return out[0], out[1], 0, (out[0], out[1])


class GroupNorm1(_Fn):
    """y = act(GroupNorm(1,C)(x)*gamma + beta + res) + emb[b,c]      (one HBM round trip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, emb, act):
        _chk(x, gamma, beta, res, emb)
        x, res, emb = _c(x), _c(res), _c(emb)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        stats = torch.empty(B, 2, device=x.device, dtype=torch.float32)
        lib().afd_groupnorm1_fwd(_p(x), _p(y), _p(stats), B, C, H * W, GN_EPS, _p(gamma), _p(beta), _p(res), act,
                                 _p(emb), _stream())
        ctx.save_for_backward(x, gamma, beta, res, stats)
        ctx.act, ctx.has_emb = act, emb is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, res, stats = ctx.saved_tensors
        B, C, H, W = x.shape
        dy = _c(dy)
        dx = torch.empty_like(x)
        dres = None
        if res is not None:
            dres = dy if ctx.act == 0 else torch.empty_like(x)      # act == 0: d(res) is dy itself
        part = torch.empty(B * C * 2, device=x.device, dtype=torch.float32)
        demb = torch.empty(B, C, device=x.device, dtype=torch.float32) if ctx.has_emb else None
        dg, db, acc, (dgamma, dbeta) = _gn_param_targets(C, gamma, beta, x.device)
        defer = acc and _GradMode.side is not None          # the two column sums of part (B, 2, C): folded with the other layers'
        lib().afd_groupnorm1_bwd(_p(x), _p(dy), _p(stats), B, C, H * W, _p(gamma), _p(beta), _p(res), ctx.act,
                                 _p(dx), _p(dres) if (res is not None and ctx.act == 1) else None, _p(part), _p(demb), 0,
                                 None if defer else _p(dg), None if defer else _p(db), acc, _stream())
        if defer:
            pp = _p(part)
            defer_to_side_stream(None, fold_desc(pp, _p(dg), C, B, stride=2 * C) + fold_desc(pp + 4 * C, _p(db), C, B, stride=2 * C),
                                 part, writes=(gamma, beta))
        elif acc:
            _wrote(gamma, beta)
        return dx, dgamma, dbeta, dres, demb, None


class GroupNormFiltAct(_Fn):
    """y = down2(GELU(up2(GroupNorm(1,C)(x)*gamma + beta + res)))    (ddpm_utils.py:122-125,127-131).

    Forward: a stats-only pass over x (4 B/elem) then the fused kernel applies the normalisation
    and the residual inside its load (8 B/elem [+4 with res]); the normalised tensor and the 2x
    intermediate never exist in memory."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, tu, td):
        _chk(x, gamma, beta, res)
        x, res = _c(x), _c(res)
        B, C, H, W = x.shape
        stats = torch.empty(B, 2, device=x.device, dtype=torch.float32)
        L = lib()
        y = torch.empty_like(x)
        if L.afd_filt_act_fwd_gn_supported(C, H, W, tu.N):
            # small samples: one workgroup holds a whole sample and computes the statistics itself (no statistics launch)
            L.afd_filt_act_fwd_gn(_p(x), _p(y), B, C, H, W, GN_EPS, _p(stats), _p(gamma), _p(beta), _p(res), tu.ptr, td.ptr, tu.N,
                                  _stream())
        else:
            L.afd_groupnorm1_fwd(_p(x), None, _p(stats), B, C, H * W, GN_EPS, None, None, None, 0, None, _stream())
            ws = _act_ws(B, C, H, W, tu.N, 0, x.device)
            L.afd_filt_act_fwd(_p(x), _p(y), B, C, H, W, _p(stats), _p(gamma), _p(beta), _p(res), tu.ptr, td.ptr, tu.N,
                               _p(ws), _stream())
        ctx.save_for_backward(x, gamma, beta, res, stats)
        ctx.tu, ctx.td = tu, td
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, res, stats = ctx.saved_tensors
        B, C, H, W = x.shape
        dy = _c(dy)
        L = lib()
        if L.afd_filt_act_fwd_gn_supported(C, H, W, ctx.tu.N):
            # small samples: one workgroup holds a sample, the same launch finishes GroupNorm's backward (dx leaves instead of dv)
            dx = torch.empty_like(x)
            dres = torch.empty_like(x) if res is not None else None
            part = torch.empty(B * C * 2, device=x.device, dtype=torch.float32)
            L.afd_filt_act_bwd_gn(_p(x), _p(dy), _p(dx), _p(dres), B, C, H, W, _p(stats), _p(gamma), _p(beta), _p(res),
                                  ctx.tu.ptr, ctx.td.ptr, ctx.tu.N, _p(part), _stream())
            dg, db, acc, (dgamma, dbeta) = _gn_param_targets(C, gamma, beta, x.device)
            if acc and _GradMode.side is not None:                     # the two column sums: folds, batched with the other layers'
                pp = _p(part)                                          # part is (B, 2, C)
                defer_to_side_stream(None, fold_desc(pp, _p(dg), C, B, stride=2 * C) + fold_desc(pp + 4 * C, _p(db), C, B, stride=2 * C),
                                     part, writes=(gamma, beta))
            else:
                L.afd_colsum2(_p(part), _p(dg), _p(db), B, C, acc, _stream())
                if acc:
                    _wrote(gamma, beta)
            return dx, dgamma, dbeta, dres, None, None
        dv = torch.empty_like(x)
        ws = _act_ws(B, C, H, W, ctx.tu.N, 1, x.device)
        part = torch.empty(B * C * 2, device=x.device, dtype=torch.float32)
        fused = ws is None                 # fast path: the filtered-GELU backward also emits the GroupNorm plane sums
        L.afd_filt_act_bwd(_p(x), _p(dy), _p(dv), B, C, H, W, _p(stats), _p(gamma), _p(beta), _p(res),
                           ctx.tu.ptr, ctx.td.ptr, ctx.tu.N, _p(ws), _p(part) if fused else None, _stream())
        dx = torch.empty_like(x)
        dg, db, acc, (dgamma, dbeta) = _gn_param_targets(C, gamma, beta, x.device)
        L.afd_groupnorm1_bwd(_p(x), _p(dv), _p(stats), B, C, H * W, _p(gamma), _p(beta), None, 0,
                             _p(dx), None, _p(part), None, 1 if fused else 0, _p(dg), _p(db), acc, _stream())
        if acc:
            _wrote(gamma, beta)
        return dx, dgamma, dbeta, (dv if res is not None else None), None, None


# ---------------------------------------------------------------------------------------------
# F5 / F10 convolution (3x3 pad 1, 1x1)
# ---------------------------------------------------------------------------------------------
def _kind_of(kinds, dgrad):
    """Form of one pass's weight image in an afd_conv3x3_weight_kinds value: 0 = Winograd, 1 = direct f16x2, 5 = direct bf16x3."""
    direct = kinds >> dgrad & 1
    return direct | (kinds & 4 if direct else 0)


class _WinoWeights:
    """Transformed 3x3 weights (G g G^T, forward and dgrad forms) kept per weight tensor while the weights do not
    change: keyed by the tensor object AND the HIP stream that asks (the transform launch and every kernel reading the
    image are then ordered on that one stream: trajectories of `Diffusion.sample_concurrent` running on other streams
    fill and read their own copies, and an evicted buffer returns to the pool of the only stream that used it),
    stamped with its autograd version and a global epoch that every raw in-place update of the parameters
    (FusedAdamW.step) bumps.  Never used under stream capture: a captured step must contain its own transform
    launches, because a replay runs after the weights moved."""
    epoch = 0
    store = {}
    max_entries = 4096
    recording = None          # dict filled with the requests of one step (TrainStep's first step), see WinoStepPlan
    active_plan = None        # WinoStepPlan whose buffers were filled at the start of the current step

    @classmethod
    def get(cls, w, nbytes, dgrad, kinds=0):
        plan = cls.active_plan
        if plan is not None:
            u = plan.lookup(w, nbytes, dgrad, kinds)
            if u is not None:
                return u, 1
        if cls.recording is not None:
            rec = cls.recording.setdefault(id(w), [w, 0, 0, 0])
            rec[1 + dgrad] = nbytes
            rec[3] = kinds
        capturing = torch.cuda.is_current_stream_capturing()
        key = (id(w), dgrad, _stream())
        stamp = (w._version, cls.epoch, w.data_ptr(), nbytes, _kind_of(kinds, dgrad))   # (the image's form follows the batch size)
        if not capturing:
            hit = cls.store.get(key)
            if hit is not None and hit[0]() is w and hit[2] == stamp:
                return hit[1], 1
        u = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
        if not capturing:
            if len(cls.store) > cls.max_entries:
                cls.store.clear()
            try:
                cls.store[key] = (weakref.ref(w), u, stamp)
            except TypeError:
                pass
        return u, 0


class WinoStepPlan:
    """Every transformed-weight image a train step needs, produced by ONE launch at the start of the step
    (afd_conv3x3_wino_weights_batched) instead of one launch per layer on the critical path.  Built from the requests
    recorded during a first step ({id(w): [w, forward bytes, dgrad bytes]}); valid while the weights keep their
    addresses (FlatParams views do)."""

    def __init__(self, requests):
        import struct
        reqs = [r for r in requests.values() if r[1] or r[2]]
        self.ok = bool(reqs)
        if not self.ok:
            return
        dev = reqs[0][0].device
        self.buf = torch.empty(sum(r[1] + r[2] for r in reqs) // 4, device=dev, dtype=torch.float32)
        self.map, descs, wg, off = {}, b"", [], 0
        for i, (w, nf, nd, kinds) in enumerate(reqs):
            Cout, Cin = w.shape[0], w.shape[1]
            uf = self.buf[off:off + nf // 4] if nf else None
            off += nf // 4
            ud = self.buf[off:off + nd // 4] if nd else None
            off += nd // 4
            self.map[id(w)] = (weakref.ref(w), w.data_ptr(), uf, ud, kinds)
            n_wg = (Cin * Cout // 64 + 3) // 4
            descs += struct.pack("<QQQiiii", w.data_ptr(), uf.data_ptr() if nf else 0, ud.data_ptr() if nd else 0, Cin, Cout, len(wg), kinds)
            wg += [i] * n_wg
        self.n_wg = len(wg)
        self.descs = torch.frombuffer(bytearray(descs), dtype=torch.uint8).to(dev)
        self.wg = torch.tensor(wg, dtype=torch.int32).to(dev)

    def valid(self):
        return self.ok and all(r() is not None and r().data_ptr() == ptr for (r, ptr, _, _, _) in self.map.values())

    def launch(self):
        lib().afd_conv3x3_wino_weights_batched(_p(self.descs), _p(self.wg), self.n_wg, _stream())

    def lookup(self, w, nbytes, dgrad, kinds=0):
        e = self.map.get(id(w))
        if e is None or e[0]() is not w or _kind_of(e[4], dgrad) != _kind_of(kinds, dgrad):   # (another batch size may want the other form)
            return None
        u = e[3] if dgrad else e[2]
        return u if (u is not None and u.numel() * 4 == nbytes) else None


def bump_param_epoch():
    """Call after parameters were modified through raw device pointers (the fused optimizer).  Every cached weight image is
    stale from here on: the store is emptied (each buffer goes back to the pool of the one stream that used it), so a
    sampling run after training does not pin images of streams that no longer exist."""
    _WinoWeights.epoch += 1
    if _WinoWeights.store:
        _WinoWeights.store.clear()


def _conv_fwd(x, w, bias, res, y, B, Cin, Cout, H, W, ks, act, want_dgrad=False):
    """3x3 layers the Winograd kernel covers go there (the library says which: a non-zero workspace size);
    everything else takes the direct implicit-GEMM kernels.  With want_dgrad the transformed weights of the
    backward pass are produced by the same launch as the forward ones and returned for Conv.backward."""
    L = lib()
    nb = L.afd_conv3x3_wino_workspace_bytes(B, Cin, Cout, H, W, 0) if ks == 3 else 0
    nd = L.afd_conv3x3_wino_workspace_bytes(B, Cin, Cout, H, W, 1) if (ks == 3 and want_dgrad) else 0
    ud = None
    if nb:
        kinds = L.afd_conv3x3_weight_kinds(B, Cin, Cout, H, W)     # which passes run the direct bf16x3 form (their image differs)
        u, ready = _WinoWeights.get(w, nb, 0, kinds)
        if nd:
            ud, dready = _WinoWeights.get(w, nd, 1, kinds)
            if not (ready and dready):
                L.afd_conv3x3_wino_weights(_p(w), _p(u), _p(ud), Cin, Cout, kinds, _stream())
                ready = 1
        L.afd_conv3x3_wino_fwd(_p(x), _p(w), _p(bias), _p(res), _p(y), B, Cin, Cout, H, W, act, _p(u), ready, kinds, _stream())
    else:
        L.afd_conv_fwd(_p(x), _p(w), _p(bias), _p(res), _p(y), B, Cin, Cout, H, W, ks, act, _stream())
    return (ud, kinds) if ud is not None else None


class Conv(_Fn):
    """y = conv(x, w) + bias + res.  (The GELU epilogue is only used by `conv_infer`.)

    fork=True returns (y, x again): the residual branch of a block that STARTS with this convolution takes x from
    here, so backward receives both gradients of x and the dgrad kernel's epilogue adds them (no autograd add)."""

    @staticmethod
    def forward(ctx, x, w, bias, res, w_param=None, b_param=None, fork=False):
        # w may be a reshaped VIEW of a parameter (Linear weights used as 1x1 kernels); w_param / b_param are
        # the leaf Parameters whose .grad the in-place mode accumulates into
        _chk(x, w, bias, res)
        x, w, res = _c(x), _c(w), _c(res)
        B, Cin, H, W = x.shape
        Cout, ks = w.shape[0], w.shape[-1]
        y = torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32)
        ctx.u_dgrad = _conv_fwd(x, w, bias, res, y, B, Cin, Cout, H, W, ks, 0, want_dgrad=x.requires_grad)
        ctx.save_for_backward(x, w)
        ctx.has_bias, ctx.has_res = bias is not None, res is not None
        ctx.w_param, ctx.b_param = w_param, b_param
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dfork=None):
        x, w = ctx.saved_tensors
        B, Cin, H, W = x.shape
        Cout, ks = w.shape[0], w.shape[-1]
        dy = _c(dy)
        L = lib()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            dfork = _c(dfork)
            nb = L.afd_conv3x3_wino_workspace_bytes(B, Cin, Cout, H, W, 1) if ks == 3 else 0
            if nb:
                if ctx.u_dgrad is not None:            # produced together with the forward image
                    (u, kinds), ready = ctx.u_dgrad, 1
                else:
                    kinds = L.afd_conv3x3_weight_kinds(B, Cin, Cout, H, W)
                    u, ready = _WinoWeights.get(w, nb, 1, kinds)
                L.afd_conv3x3_wino_dgrad(_p(dy), _p(w), _p(dx), _p(dfork), B, Cin, Cout, H, W, _p(u), ready, kinds, _stream())
            else:
                L.afd_conv_dgrad(_p(dy), _p(w), _p(dx), B, Cin, Cout, H, W, ks, _stream())
                if dfork is not None:                      # (the direct kernels have no add-to-dx epilogue)
                    L.afd_add(_p(dx), _p(dfork), _p(dx), dx.numel(), _stream())
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            nbytes = L.afd_conv_wgrad_workspace_bytes(B, Cin, Cout, H, W, ks)
            ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
            wp, bp = ctx.w_param, ctx.b_param
            # (a plain tensor as weight, or as the bias of a Parameter weight, has no .grad to add into: out of place)
            if wp is not None and (bp is not None or not ctx.has_bias) and _direct(wp, bp) and wp.grad.numel() == w.numel():
                side = _GradMode.side
                if side is None:
                    L.afd_conv_wgrad(_p(x), _p(dy), _p(wp.grad), _p(bp.grad) if bp is not None else None,
                                     B, Cin, Cout, H, W, ks, 1, _p(ws), _stream())
                    _wrote(wp, bp)
                else:
                    dwp, dbp = _p(wp.grad), (_p(bp.grad) if bp is not None else None)
                    defer_to_side_stream(lambda st, x=x, dy=dy, ws=ws: _wgrad_partials(x, dy, dwp, dbp, B, Cin, Cout, H, W, ks, ws, st),
                                         x, dy, ws, writes=(wp, bp))
            else:
                dw = torch.empty_like(w)
                db = torch.empty(Cout, device=x.device, dtype=torch.float32) if ctx.has_bias else None
                L.afd_conv_wgrad(_p(x), _p(dy), _p(dw), _p(db), B, Cin, Cout, H, W, ks, 0, _p(ws), _stream())
        return dx, dw, db, (dy if ctx.has_res else None), None, None, None


def conv(x, w, bias=None, res=None, w_param=None, b_param=None, fork=False):
    """w_param / b_param: the leaf Parameters behind `w` / `bias` (enables in-place grad accumulation).
    fork: also return x (for the residual of the block this convolution opens), see Conv."""
    if w_param is None and isinstance(w, torch.nn.Parameter):
        w_param = w
    if b_param is None and isinstance(bias, torch.nn.Parameter):
        b_param = bias
    return Conv.apply(x, w, bias, res, w_param, b_param, fork)


def conv_infer(x, w, bias=None, res=None, act=0):
    """No-grad convolution with the fused GELU epilogue."""
    _chk(x, w, bias, res)
    x, w, res = _c(x), _c(w), _c(res)
    B, Cin, H, W = x.shape
    Cout, ks = w.shape[0], w.shape[-1]
    y = torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32)
    _conv_fwd(x, w, bias, res, y, B, Cin, Cout, H, W, ks, act)
    return y


# ---------------------------------------------------------------------------------------------
# F10 attention block pieces
# ---------------------------------------------------------------------------------------------
class LayerNormC(_Fn):
    """nn.LayerNorm([C]) applied to the (B, L, C) token view of an NCHW tensor, without the transposes.

    Returns (y, x_res): x_res is x again, for the residual branch that every LayerNorm of the attention block sits
    beside (y -> ... -> + x).  Routing the residual through this node means backward receives BOTH gradients of x
    and the kernel writes LN'(dy) + d(x_res) in one pass, instead of autograd launching a separate add."""

    @staticmethod
    def forward(ctx, x, gamma, beta):
        _chk(x, gamma, beta)
        x = _c(x)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        stats = torch.empty(B, H * W, 2, device=x.device, dtype=torch.float32)
        lib().afd_layernorm_c_fwd(_p(x), _p(y), _p(stats), B, C, H * W, LN_EPS, _p(gamma), _p(beta), _stream())
        ctx.save_for_backward(x, gamma, stats)
        ctx.beta_param = beta
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, gamma, stats = ctx.saved_tensors
        B, C, H, W = x.shape
        if dy is None:                                   # only the residual output was used
            return dres, None, None
        dy, dres = _c(dy), _c(dres)
        dx = torch.empty_like(x)
        L = lib()
        if _direct(gamma, ctx.beta_param):
            # in-place mode: dx now; dgamma / dbeta (plane sums + fold) as a separate call, on the side stream when
            # there is one (the same arithmetic either way: the two-stream step stays bit-identical)
            L.afd_layernorm_c_bwd(_p(x), _p(dy), _p(stats), B, C, H * W, _p(gamma), _p(dx), _p(dres), None, None, None, 0, _stream())
            _ln_param_grads(x, dy, stats, gamma, ctx.beta_param, B, C, H * W)
            return dx, None, None
        part = torch.empty(B, 2, C, device=x.device, dtype=torch.float32)
        dg, db, acc, (dgamma, dbeta) = _gn_param_targets(C, gamma, ctx.beta_param, x.device)
        L.afd_layernorm_c_bwd(_p(x), _p(dy), _p(stats), B, C, H * W, _p(gamma), _p(dx), _p(dres), _p(part), _p(dg), _p(db), acc,
                              _stream())
        return dx, dgamma, dbeta


def layernorm_c(x, gamma, beta):
    """y only (no residual routed through the node)."""
    return LayerNormC.apply(x, gamma, beta)[0]


class Attention(_Fn):
    """softmax(QK^T/sqrt(d))V on qkv (B, 3C, H, W) -> (B, C, H, W); scores never materialised."""

    @staticmethod
    def forward(ctx, qkv, heads):
        _chk(qkv)
        qkv = _c(qkv)
        B, C3, H, W = qkv.shape
        C, L = C3 // 3, H * W
        o = torch.empty(B, C, H, W, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(B, heads, L, device=qkv.device, dtype=torch.float32)
        lib().afd_attn_fwd(_p(qkv), _p(o), _p(lse), B, heads, C // heads, L, _stream())
        ctx.save_for_backward(qkv, o, lse)
        ctx.heads = heads
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        B, C3, H, W = qkv.shape
        C, L = C3 // 3, H * W
        do = _c(do)
        dqkv = torch.empty_like(qkv)
        delta = torch.empty_like(lse)
        lib().afd_attn_bwd(_p(qkv), _p(o), _p(do), _p(lse), _p(dqkv), _p(delta), B, ctx.heads, C // ctx.heads, L, _stream())
        return dqkv, None


def tok_supported(C):
    """True if the fused token-chain kernels (csrc/tok.hip) cover channel width C."""
    return bool(lib().afd_tok_supported(int(C)))


def _wgrad_partials(x, dy, dwp, dbp, B, Cin, Cout, H, W, ks, ws, st):
    """afd_conv_wgrad_partials: the slab producer now, its fold descriptor(s) returned for the batched fold."""
    import ctypes
    buf = ctypes.create_string_buffer(112)
    n = ctypes.c_int(0)
    lib().afd_conv_wgrad_partials(_p(x), _p(dy), dwp, dbp, B, Cin, Cout, H, W, ks, 1, _p(ws), ctypes.addressof(buf), ctypes.addressof(n), st)
    return buf.raw[:56 * n.value]


def _linear_grads(x, dy, w, b, B, C_in, C_out, H, W, need_w=True):
    """Weight / bias gradients of a token-wise Linear (= 1x1 convolution) y = w x + b from its input x (B,C_in,H,W) and
    dy (B,C_out,H,W).  In-place mode: accumulated straight into w.grad / b.grad, on the side stream when there is one
    (returns (None, None)); otherwise returns fresh (dw, db) for autograd."""
    L = lib()
    nbytes = L.afd_conv_wgrad_workspace_bytes(B, C_in, C_out, H, W, 1)
    ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
    if _direct(w, b):
        dwp, dbp = _p(w.grad), (_p(b.grad) if b is not None else None)
        if _GradMode.side is not None:
            defer_to_side_stream(lambda st, x=x, dy=dy, ws=ws: _wgrad_partials(x, dy, dwp, dbp, B, C_in, C_out, H, W, 1, ws, st),
                                 x, dy, ws, writes=(w, b))
        else:
            L.afd_conv_wgrad(_p(x), _p(dy), dwp, dbp, B, C_in, C_out, H, W, 1, 1, _p(ws), _stream())
            _wrote(w, b)
        return None, None
    dw = torch.empty_like(w)
    db = torch.empty(C_out, device=x.device, dtype=torch.float32) if b is not None else None
    L.afd_conv_wgrad(_p(x), _p(dy), _p(dw), _p(db), B, C_in, C_out, H, W, 1, 0, _p(ws), _stream())
    return dw, db


def _ln_param_grads(x, dy, stats, gamma, beta, B, C, HW):
    """LayerNorm-over-channels parameter gradients from the LayerNorm input x, the gradient at its output dy and the
    saved statistics; same in-place / side-stream convention as _linear_grads."""
    L = lib()
    part = torch.empty(B, 2, C, device=x.device, dtype=torch.float32)
    dg, db, acc, (dgamma, dbeta) = _gn_param_targets(C, gamma, beta, x.device)
    pdg, pdb = _p(dg), _p(db)
    if acc and _GradMode.side is not None:
        def fn(st, x=x, dy=dy, stats=stats, part=part):                  # the plane pass now, the two column sums with the batched fold
            L.afd_layernorm_c_bwd_partials(_p(x), _p(dy), _p(stats), B, C, HW, _p(part), st)
            pp = _p(part)
            return fold_desc(pp, pdg, C, B, stride=2 * C) + fold_desc(pp + 4 * C, pdb, C, B, stride=2 * C)
        defer_to_side_stream(fn, x, dy, stats, part, writes=(gamma, beta))
    else:
        L.afd_layernorm_c_bwd_params(_p(x), _p(dy), _p(stats), B, C, HW, _p(part), pdg, pdb, acc, _stream())
        if acc:
            _wrote(gamma, beta)
    return dgamma, dbeta


class AttnHead(_Fn):
    """qkv = in_proj(LayerNorm(x)) in ONE launch (ddpm_utils.py:70-71, csrc/tok.hip); also returns x again for the residual
    branch, so backward receives both gradients of x and the fused backward kernel adds them."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w_in, b_in):
        _chk(x, gamma, beta, w_in, b_in)
        x = _c(x)
        B, C, H, W = x.shape
        train = not isinstance(ctx, _NoCtx)             # (forward itself always runs with grad mode off)
        qkv = torch.empty(B, 3 * C, H, W, device=x.device, dtype=torch.float32)
        h = torch.empty_like(x) if train else None
        stats = torch.empty(B, H * W, 2, device=x.device, dtype=torch.float32) if train else None
        lib().afd_tok_head_fwd(_p(x), _p(gamma), _p(beta), _p(w_in), _p(b_in), _p(h), _p(stats), _p(qkv), B, C, H * W, LN_EPS, _stream())
        ctx.save_for_backward(x, h, stats, gamma, w_in)
        ctx.params = (beta, b_in)
        return qkv, x.view_as(x)

    @staticmethod
    def backward(ctx, dqkv, dres):
        x, h, stats, gamma, w_in = ctx.saved_tensors
        beta, b_in = ctx.params
        B, C, H, W = x.shape
        dqkv = _c(dqkv)
        if dres is None:
            dres = torch.zeros_like(x)
        dres = _c(dres)
        dx = torch.empty_like(x)
        dh = torch.empty_like(x)
        lib().afd_tok_head_bwd(_p(dqkv), _p(x), _p(stats), _p(gamma), _p(w_in), _p(dres), _p(dh), _p(dx), B, C, H * W, _stream())
        dw, db = _linear_grads(h, dqkv, w_in, b_in, B, C, 3 * C, H, W)
        dgamma, dbeta = _ln_param_grads(x, dh, stats, gamma, beta, B, C, H * W)
        return dx, dgamma, dbeta, dw, db


class AttnTail(_Fn):
    """out = FF(LayerNorm(a)) + a with a = out_proj(att) + x, in ONE launch (ddpm_utils.py:71-73, csrc/tok.hip)."""

    @staticmethod
    def forward(ctx, att, x, wo, bo, gamma, beta, w1, b1, w2, b2):
        _chk(att, x, wo, bo, gamma, beta, w1, b1, w2, b2)
        att, x = _c(att), _c(x)
        B, C, H, W = att.shape
        out = torch.empty_like(att)
        if not isinstance(ctx, _NoCtx):
            a, f, u, g = (torch.empty_like(att) for _ in range(4))
            stats = torch.empty(B, H * W, 2, device=att.device, dtype=torch.float32)
        else:
            a = f = u = g = stats = None
        lib().afd_tok_tail_fwd(_p(att), _p(x), _p(wo), _p(bo), _p(gamma), _p(beta), _p(w1), _p(b1), _p(w2), _p(b2),
                               _p(a), _p(stats), _p(f), _p(u), _p(g), _p(out), B, C, H * W, LN_EPS, _stream())
        ctx.save_for_backward(att, a, stats, f, u, g, gamma, wo, w1, w2)
        ctx.params = (bo, beta, b1, b2)
        return out

    @staticmethod
    def backward(ctx, dout):
        att, a, stats, f, u, g, gamma, wo, w1, w2 = ctx.saved_tensors
        bo, beta, b1, b2 = ctx.params
        B, C, H, W = att.shape
        dout = _c(dout)
        du, df, da, datt = (torch.empty_like(att) for _ in range(4))
        lib().afd_tok_tail_bwd(_p(dout), _p(u), _p(a), _p(stats), _p(gamma), _p(w2), _p(w1), _p(wo),
                               _p(du), _p(df), _p(da), _p(datt), B, C, H * W, _stream())
        dw2, db2 = _linear_grads(g, dout, w2, b2, B, C, C, H, W)
        dw1, db1 = _linear_grads(f, du, w1, b1, B, C, C, H, W)
        dwo, dbo = _linear_grads(att, da, wo, bo, B, C, C, H, W)
        dgamma, dbeta = _ln_param_grads(a, df, stats, gamma, beta, B, C, H * W)
        return datt, da, dwo, dbo, dgamma, dbeta, dw1, db1, dw2, db2


class Gelu(_Fn):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        x = _c(x)
        y = torch.empty_like(x)
        lib().afd_gelu_fwd(_p(x), _p(y), x.numel(), _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(x)
        lib().afd_gelu_bwd(_p(x), _p(dy), _p(dx), x.numel(), _stream())
        return dx


# ---------------------------------------------------------------------------------------------
# resampling of variants 0 / 2, concat
# ---------------------------------------------------------------------------------------------
class MaxPool2(_Fn):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        x = _c(x)
        B, C, H, W = x.shape
        y = torch.empty(B, C, H // 2, W // 2, device=x.device, dtype=torch.float32)
        lib().afd_maxpool2_fwd(_p(x), _p(y), B, C, H, W, _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, C, H, W = x.shape
        dy = _c(dy)
        dx = torch.empty_like(x)
        lib().afd_maxpool2_bwd(_p(x), _p(dy), _p(dx), B, C, H, W, _stream())
        return dx


class UpCat(_Fn):
    """cat([skip, up2x(x)], dim=1) in one buffer: the upsampler writes straight into the channel
    slice (ddpm_utils.py:241-242 / :354-355 / :413-414).  mode 'filt' = custom_upsample,
    'bilinear' = nn.Upsample(2, bilinear, align_corners=True)."""

    @staticmethod
    def forward(ctx, x, skip, taps, mode):
        _chk(x, skip)
        x, skip = _c(x), _c(skip)
        B, C, H, W = x.shape
        Cs = skip.shape[1]
        assert skip.shape[2] == 2 * H and skip.shape[3] == 2 * W
        plane = 4 * H * W
        out = torch.empty(B, Cs + C, 2 * H, 2 * W, device=x.device, dtype=torch.float32)
        L = lib()
        up_ptr = out.data_ptr() + 4 * Cs * plane
        bs = (Cs + C) * plane
        if mode == "filt":
            L.afd_filt_up2_fwd(_p(x), up_ptr, B, C, H, W, 0, bs, taps.ptr, taps.N, _stream())
        else:
            L.afd_bilinear_up2_fwd(_p(x), up_ptr, B, C, H, W, bs, _stream())
        L.afd_copy_batched(_p(skip), _p(out), B, Cs * plane, 0, bs, _stream())
        ctx.taps, ctx.mode, ctx.dims = taps, mode, (B, C, Cs, H, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, Cs, H, W = ctx.dims
        dout = _c(dout)
        plane = 4 * H * W
        bs = (Cs + C) * plane
        L = lib()
        dx = torch.empty(B, C, H, W, device=dout.device, dtype=torch.float32)
        up_ptr = dout.data_ptr() + 4 * Cs * plane
        if ctx.mode == "filt":
            L.afd_filt_up2_bwd(up_ptr, _p(dx), B, C, H, W, bs, 0, ctx.taps.ptr, ctx.taps.N, _stream())
        else:
            L.afd_bilinear_up2_bwd(up_ptr, _p(dx), B, C, H, W, bs, _stream())
        # the skip's gradient is a channel slice of dout: returned as a VIEW.  Every skip tensor has a second consumer (the next
        # encoder stage), so autograd adds the two gradients anyway -- its add reads the slice in place and writes a contiguous
        # sum; the copy that used to materialise the slice first (3 launches, 2 tensor passes per step) is gone (8.54 -> 8.48 ms/step, same box).
        return dx, dout[:, :Cs], None, None


# ---------------------------------------------------------------------------------------------
# F9 time embedding
# ---------------------------------------------------------------------------------------------
def pos_encoding(t, inv_freq):
    """(B,) int64 timesteps -> (B, 2*half) fp32 [sin | cos]   (ddpm_models.py:261-269)."""
    if not t.is_cuda:
        raise AfdError("afdm: timesteps must live on the HIP device")
    t = t.contiguous()
    B, half = t.shape[0], inv_freq.shape[0]
    out = torch.empty(B, 2 * half, device=t.device, dtype=torch.float32)
    lib().afd_pos_encoding(_p(t), _p(inv_freq), _p(out), B, half, _stream())
    return out


class EmbedAdd(_Fn):
    """t_emb + label_emb(y)  (ddpm_models.py:276-277): nn.Embedding lookup and the add in one launch; backward is the
    deterministic row scatter into the table's gradient (the positional encoding itself carries no gradient).
    A negative label (NULL_LABEL) marks a row without a label: it keeps t_emb as it is and sends no gradient to the table."""

    @staticmethod
    def forward(ctx, temb, table, y):
        _chk(temb, table)
        if not y.is_cuda or y.dtype != torch.long:
            raise AfdError("afdm: class labels must be an int64 tensor on the HIP device")
        temb, table, y = _c(temb), _c(table), _c(y)
        B, D = temb.shape
        if table.shape[1] != D or y.shape[0] != B:
            raise AfdError(f"afdm: label embedding shape mismatch (temb {tuple(temb.shape)}, table {tuple(table.shape)}, y {tuple(y.shape)})")
        out = torch.empty_like(temb)
        lib().afd_label_embed_add_fwd(_p(temb), _p(table), _p(y), _p(out), B, D, table.shape[0], _stream())
        ctx.save_for_backward(y)
        ctx.table = table if isinstance(table, torch.nn.Parameter) else None
        ctx.K = table.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        (y,) = ctx.saved_tensors
        dout = _c(dout)
        B, D = dout.shape
        dtemb = dout if ctx.needs_input_grad[0] else None
        if not ctx.needs_input_grad[1]:
            return dtemb, None, None
        tp = ctx.table
        if tp is not None and _direct(tp):
            lib().afd_embed_add_bwd(_p(dout), _p(y), _p(tp.grad), B, D, ctx.K, 1, _stream())
            _wrote(tp)
            return dtemb, None, None
        dtable = torch.empty(ctx.K, D, device=dout.device, dtype=torch.float32)
        lib().afd_embed_add_bwd(_p(dout), _p(y), _p(dtable), B, D, ctx.K, 0, _stream())
        return dtemb, dtable, None


class SiluLinear(_Fn):
    """emb_layer = nn.Sequential(nn.SiLU(), nn.Linear(emb_dim, C))   (ddpm_utils.py:208-214).  bias may be None."""

    @staticmethod
    def forward(ctx, temb, w, bias):
        _chk(temb, w, bias)
        temb, w = _c(temb), _c(w)
        B, K = temb.shape
        N = w.shape[0]
        out = torch.empty(B, N, device=temb.device, dtype=torch.float32)
        lib().afd_silu_linear_fwd(_p(temb), _p(w), _p(bias), _p(out), B, K, N, _stream())
        ctx.save_for_backward(temb, w)
        ctx.params = (w if isinstance(w, torch.nn.Parameter) else None, bias if isinstance(bias, torch.nn.Parameter) else None)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        temb, w = ctx.saved_tensors
        dout = _c(dout)
        dtemb = torch.zeros_like(temb) if ctx.needs_input_grad[0] else None
        return (dtemb,) + _silu_linear_param_grads(temb, w, dout, dtemb, ctx.params, ctx.has_bias)


def _silu_linear_param_grads(temb, w, dout, dtemb, params, has_bias):
    """dW / dbias of SiluLinear (and dtemb += ..., when given, in the same call).  In-place mode with Parameters that own a
    .grad: accumulated there, on the side stream when nothing the chain consumes comes out of the launch -> (None, None);
    otherwise (out of place, a plain tensor in a Parameter's place, no .grad): fresh (dw, db) for autograd."""
    B, K = temb.shape
    N = w.shape[0]
    wp, bp = params
    if wp is not None and (bp is not None or not has_bias) and _direct(wp, bp):
        pw, pb = _p(wp.grad), (_p(bp.grad) if bp is not None else None)
        if dtemb is None and _GradMode.side is not None:          # parameter gradients only: off the critical path
            defer_to_side_stream(lambda st, temb=temb, w=w, dout=dout: lib().afd_silu_linear_bwd(
                _p(temb), _p(w), _p(dout), pw, pb, None, B, K, N, 1, st), temb, w, dout, writes=(wp, bp))
        else:
            lib().afd_silu_linear_bwd(_p(temb), _p(w), _p(dout), pw, pb, _p(dtemb), B, K, N, 1, _stream())
            _wrote(wp, bp)
        return None, None
    dw = torch.empty_like(w)
    db = torch.empty(N, device=w.device, dtype=torch.float32) if has_bias else None
    lib().afd_silu_linear_bwd(_p(temb), _p(w), _p(dout), _p(dw), _p(db), _p(dtemb), B, K, N, 0, _stream())
    return dw, db


def silu_linear_batched(temb, layers):
    """The emb_layer of several stages (each nn.Sequential(nn.SiLU(), nn.Linear(emb_dim, C_i)), ddpm_utils.py:208-214) on the SAME
    time embedding: ONE forward launch for all of them (the input exists as soon as the UNet forward starts, so one launch
    replaces six small dependent ones) -> [out_0, out_1, ...] (plain tensors, no autograd history).  `layers` = [(weight,
    bias), ...]; temb must not need a gradient (the conditional model keeps the per-stage op).  Backward stays PER STAGE:
    the stage wraps its output in its own autograd node WHEN ITS FORWARD RUNS (SiluLinearPre, see blocks._Stage._emb).
    One node for all six would hold every stage's gradient (and with it three of the four data-parallel buckets) back
    until the first encoder stage's backward; and six nodes created here, at the start of the forward, would carry the
    lowest sequence numbers of the graph -- autograd runs ready nodes highest-sequence first, so they would all run at
    the very END of backward (measured: the decoder bucket became ready at flush 24 of 25)."""
    import ctypes, struct
    ws, bs = [w for w, _ in layers], [b for _, b in layers]
    _chk(temb, *ws, *bs)
    temb = _c(temb)
    B, K = temb.shape
    with torch.no_grad():
        outs = [torch.empty(B, w.shape[0], device=temb.device, dtype=torch.float32) for w in ws]
    desc = b"".join(struct.pack("<QQQi4x", _p(w) or 0, _p(b) or 0, _p(o), w.shape[0]) for w, b, o in zip(ws, bs, outs))
    buf = ctypes.create_string_buffer(desc, len(desc))
    lib().afd_silu_linear_fwd_batched(_p(temb), ctypes.addressof(buf), len(ws), B, K, _stream())
    return outs


def gather_rows_batched(idx, tables):
    """[table_i[idx] for table_i in tables] in one launch (idx (B,) int64 on the device; tables (rows, N_i) fp32)."""
    import ctypes, struct
    _chk(*tables)
    B, rows = idx.shape[0], tables[0].shape[0]
    outs = [torch.empty(B, t.shape[1], device=t.device, dtype=torch.float32) for t in tables]
    desc = b"".join(struct.pack("<QQQi4x", _p(t), 0, _p(o), t.shape[1]) for t, o in zip(tables, outs))
    buf = ctypes.create_string_buffer(desc, len(desc))
    lib().afd_gather_rows_batched(_p(idx), ctypes.addressof(buf), len(tables), B, rows, _stream())
    return outs


class SiluLinearPre(_Fn):
    """Autograd node of ONE stage's emb_layer whose forward value was computed by silu_linear_batched: forward hands the
    precomputed output on, backward is SiluLinear's parameter-gradient part."""

    @staticmethod
    def forward(ctx, out, temb, w, bias):
        ctx.save_for_backward(temb, w)
        ctx.params = (w if isinstance(w, torch.nn.Parameter) else None, bias if isinstance(bias, torch.nn.Parameter) else None)
        ctx.has_bias = bias is not None
        return out.view_as(out)

    @staticmethod
    def backward(ctx, dout):
        temb, w = ctx.saved_tensors
        return (None, None) + _silu_linear_param_grads(temb, w, _c(dout), None, ctx.params, ctx.has_bias)


# ---------------------------------------------------------------------------------------------
# F14 / F15 / F16
# ---------------------------------------------------------------------------------------------
def noise_images(x, eps, t, alpha_hat):
    _chk(x, eps, alpha_hat)
    x, eps = _c(x), _c(eps)
    out = torch.empty_like(x)
    lib().afd_noise_images(_p(x), _p(eps), _p(t.contiguous()), _p(alpha_hat), _p(out), x.shape[0],
                           x.numel() // x.shape[0], _stream())
    return out


def _step_args(what, x, eps, noise, table, out, out2=None, guided=False, x0=None, mask=None, masked=False):
    """The argument check of every step wrapper -> n = x.numel().  eps holds n elements (2n when guided); noise, out, out2 and,
    when masked, x0 (fp32) and mask (uint8) hold n; `table` (alpha_hat, DPM++'s coef; None: not checked) any number."""
    _chk(x, eps, noise, table, out, out2, x0)
    n = x.numel()
    ne = 2 * n if guided else n
    if eps.numel() != ne:
        raise AfdError(f"afdm: {what} needs eps{'2' if guided else ''} of {ne} elements (got {eps.numel()})")
    for o in (x, eps, noise, table, out, out2):
        if o is not None and not o.is_contiguous():
            raise AfdError(f"afdm: {what}: every tensor must be contiguous")
        if o is not None and o is not eps and o is not table and o.numel() != n:
            raise AfdError(f"afdm: {what}: x / noise / outputs must hold {n} elements")
    if masked:
        if x0.numel() != n or not x0.is_contiguous():
            raise AfdError(f"afdm: {what}: x0 must be a contiguous tensor of {n} elements")
        if not mask.is_cuda or mask.dtype != torch.uint8 or mask.numel() != n or not mask.is_contiguous():
            raise AfdError(f"afdm: {what}: mask must be a contiguous uint8 device tensor of {n} elements")
    return n


def _ddim_host_t(what, alpha_hat, t, t_prev, eta):
    t, t_prev, eta = int(t), int(t_prev), float(eta)
    if not 0 <= t_prev < t < alpha_hat.numel():
        raise AfdError(f"afdm: {what} needs 0 <= t_prev < t < {alpha_hat.numel()} (got t = {t}, t_prev = {t_prev})")
    if not eta >= 0:
        raise AfdError(f"afdm: {what} needs eta >= 0 (got {eta})")
    return t, t_prev, eta


def _ddim_dev_t(what, t_dev, t_prev_dev):
    for v in (t_dev, t_prev_dev):
        if not v.is_cuda or v.dtype != torch.long or v.numel() < 1:
            raise AfdError(f"afdm: {what}: t_dev / t_prev_dev must be int64 device tensors (element 0 is read)")


def _step(what, x, eps, noise, tables, index, out, eta=None, cfg_scale=None, out2=None, x0=None, mask=None, masked=False, dev=False,
          var=False):
    """One DDPM step (eta None; tables = (alpha, alpha_hat, beta), index = (i,)) or DDIM step (tables = (alpha_hat,), index =
    (t, t_prev); var: tables = (alpha_hat, sig), the step whose sigma is sig[t]): checks the arguments and calls
    afd_{denoise,ddim}_step[_var][_masked][_cfg][_dev], whose arguments run
    x, eps, noise, [x0, mask], tables, index, [eta], [cfg_scale], x_out, [x_out2], n, stream.  dev: index holds device tensors."""
    ddim, guided = eta is not None, cfg_scale is not None
    out = torch.empty_like(x) if out is None else out
    n = _step_args(what, x, eps, noise, tables[0] if ddim else None, out, out2, guided, x0, mask, masked)
    if var:
        sig = tables[1]
        _chk(sig)
        if tuple(sig.shape) != tuple(tables[0].shape) or not sig.is_contiguous():
            raise AfdError(f"afdm: {what}: sig must be a contiguous table of alpha_hat's shape {tuple(tables[0].shape)}")
    if ddim and dev:
        _ddim_dev_t(what, *index)
        eta = float(eta)
    elif ddim:
        *index, eta = _ddim_host_t(what, tables[0], *index, eta)
    index = [_p(v) if dev else int(v) for v in index]
    name = ("afd_ddim_step" if ddim else "afd_denoise_step") + "_var" * var + "_masked" * masked + "_cfg" * guided + "_dev" * dev
    args = [_p(x), _p(eps), _p(noise)] + ([_p(x0), _p(mask)] if masked else []) + [_p(t) for t in tables] + index
    args += ([eta] if ddim else []) + ([float(cfg_scale)] if guided else []) + [_p(out)] + ([_p(out2)] if guided else [])
    getattr(lib(), name)(*args, n, _stream())
    return out


def denoise_step(x, eps_pred, noise, alpha, alpha_hat, beta, i, out=None):
    return _step("denoise step", _c(x), _c(eps_pred), _c(noise), (alpha, alpha_hat, beta), (i,), out)


def denoise_step_dev(x, eps_pred, noise, alpha, alpha_hat, beta, t_dev, out):
    """Denoise update whose step index is t_dev[0] on the device (graph-replayable)."""
    return _step("denoise step", x, eps_pred, noise, (alpha, alpha_hat, beta), (t_dev,), out, dev=True)


def denoise_step_cfg(x, eps2, noise, alpha, alpha_hat, beta, i, cfg_scale, out=None, out2=None):
    """Classifier-free guided update: eps2 = the forward over [conditional rows ; unconditional rows] (2n images),
    e = torch.lerp(eps2[n:], eps2[:n], cfg_scale) and then exactly `denoise_step(x, e, ...)`, in one launch.  `out` may be
    x (in place); `out2` (optional) receives the same values."""
    return _step("guided denoise step", x, eps2, noise, (alpha, alpha_hat, beta), (i,), out, cfg_scale=cfg_scale, out2=out2)


def denoise_step_cfg_dev(x, eps2, noise, alpha, alpha_hat, beta, t_dev, cfg_scale, out, out2=None):
    """denoise_step_cfg with the step index t_dev[0] read on the device (graph-replayable)."""
    return _step("guided denoise step", x, eps2, noise, (alpha, alpha_hat, beta), (t_dev,), out, cfg_scale=cfg_scale, out2=out2, dev=True)


def ddim_step(x, eps, noise, alpha_hat, t, t_prev, eta, out=None):
    """DDIM update t -> t_prev (include/afd.h: afd_ddim_step gives the exact expression).  noise: None (the last step, or
    eta = 0) or n standard-normal values scaled by sigma.  `out` may be x (in place)."""
    return _step("DDIM step", x, eps, noise, (alpha_hat,), (t, t_prev), out, eta=eta)


def ddim_step_dev(x, eps, noise, alpha_hat, t_dev, t_prev_dev, eta, out):
    """ddim_step with t = t_dev[0] and t_prev = t_prev_dev[0] read on the device (graph-replayable)."""
    return _step("DDIM step", x, eps, noise, (alpha_hat,), (t_dev, t_prev_dev), out, eta=eta, dev=True)


def ddim_step_cfg(x, eps2, noise, alpha_hat, t, t_prev, eta, cfg_scale, out=None, out2=None):
    """Classifier-free guided DDIM update: e = torch.lerp(eps2[n:], eps2[:n], cfg_scale), then exactly `ddim_step(x, e, ...)`,
    in one launch.  `out` may be x (in place); `out2` (optional) receives the same values."""
    return _step("guided DDIM step", x, eps2, noise, (alpha_hat,), (t, t_prev), out, eta=eta, cfg_scale=cfg_scale, out2=out2)


def ddim_step_cfg_dev(x, eps2, noise, alpha_hat, t_dev, t_prev_dev, eta, cfg_scale, out, out2=None):
    """ddim_step_cfg with the step indices read on the device (graph-replayable)."""
    return _step("guided DDIM step", x, eps2, noise, (alpha_hat,), (t_dev, t_prev_dev), out, eta=eta, cfg_scale=cfg_scale, out2=out2,
                 dev=True)


def ddim_step_var(x, eps, noise, alpha_hat, sig, t, t_prev, eta, out=None):
    """The DDIM update t -> t_prev with the noise scaled by sig[t], a (T,) fp32 device table, in place of DDIM's own sigma
    (Analytic-DPM; include/afd.h: afd_ddim_step_var).  The mean is `ddim_step`'s at that eta.  `out` may be x (in place)."""
    return _step("analytic DDIM step", x, eps, noise, (alpha_hat, sig), (t, t_prev), out, eta=eta, var=True)


def ddim_step_var_dev(x, eps, noise, alpha_hat, sig, t_dev, t_prev_dev, eta, out):
    """ddim_step_var with t = t_dev[0] and t_prev = t_prev_dev[0] read on the device (graph-replayable)."""
    return _step("analytic DDIM step", x, eps, noise, (alpha_hat, sig), (t_dev, t_prev_dev), out, eta=eta, dev=True, var=True)


def ddim_step_var_cfg(x, eps2, noise, alpha_hat, sig, t, t_prev, eta, cfg_scale, out=None, out2=None):
    """Classifier-free guided form: e = torch.lerp(eps2[n:], eps2[:n], cfg_scale), then exactly `ddim_step_var(x, e, ...)`, in
    one launch.  `out` may be x (in place); `out2` (optional) receives the same values."""
    return _step("guided analytic DDIM step", x, eps2, noise, (alpha_hat, sig), (t, t_prev), out, eta=eta, cfg_scale=cfg_scale,
                 out2=out2, var=True)


def ddim_step_var_cfg_dev(x, eps2, noise, alpha_hat, sig, t_dev, t_prev_dev, eta, cfg_scale, out, out2=None):
    """ddim_step_var_cfg with the step indices read on the device (graph-replayable)."""
    return _step("guided analytic DDIM step", x, eps2, noise, (alpha_hat, sig), (t_dev, t_prev_dev), out, eta=eta, cfg_scale=cfg_scale,
                 out2=out2, dev=True, var=True)


def _ddim_invert(what, x, eps, alpha_hat, s, u, out, cfg_scale=None, out2=None, dev=False):
    """One ascending DDIM step s -> u: checks the arguments and calls afd_ddim_invert_step[_cfg][_dev], whose arguments run
    x, eps, alpha_hat, s, u, [cfg_scale], x_out, [x_out2], n, stream.  dev: s and u are int64 device tensors."""
    guided = cfg_scale is not None
    out = torch.empty_like(x) if out is None else out
    n = _step_args(what, x, eps, None, alpha_hat, out, out2, guided)
    if dev:
        for v in (s, u):
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.long or v.numel() < 1:
                raise AfdError(f"afdm: {what}: s_dev / u_dev must be int64 device tensors (element 0 is read)")
        index = [_p(s), _p(u)]
    else:
        s, u = int(s), int(u)
        if not 0 <= s < u < alpha_hat.numel():
            raise AfdError(f"afdm: {what} needs 0 <= s < u < {alpha_hat.numel()} (got s = {s}, u = {u})")
        index = [s, u]
    name = "afd_ddim_invert_step" + "_cfg" * guided + "_dev" * dev
    args = [_p(x), _p(eps), _p(alpha_hat)] + index + ([float(cfg_scale)] if guided else []) + [_p(out)] + ([_p(out2)] if guided else [])
    getattr(lib(), name)(*args, n, _stream())
    return out


def ddim_invert_step(x, eps, alpha_hat, s, u, out=None):
    """The ascending DDIM step s -> u, 0 <= s < u (include/afd.h: afd_ddim_invert_step gives the exact expression): the inverse of
    `ddim_step(., eps, None, alpha_hat, u, s, 0.0)` for the same eps.  `out` defaults to a new tensor (the refinement of
    `Diffusion.invert` re-reads x) and may be x (in place); it must not overlap eps."""
    return _ddim_invert("DDIM invert step", x, eps, alpha_hat, s, u, out)


def ddim_invert_step_dev(x, eps, alpha_hat, s_dev, u_dev, out):
    """ddim_invert_step with s = s_dev[0] and u = u_dev[0] read on the device (graph-replayable)."""
    return _ddim_invert("DDIM invert step", x, eps, alpha_hat, s_dev, u_dev, out, dev=True)


def ddim_invert_step_cfg(x, eps2, alpha_hat, s, u, cfg_scale, out=None, out2=None):
    """Classifier-free guided ascending step: e = torch.lerp(eps2[n:], eps2[:n], cfg_scale), then exactly
    `ddim_invert_step(x, e, ...)`, in one launch.  `out2` (optional) receives the same values as `out`."""
    return _ddim_invert("guided DDIM invert step", x, eps2, alpha_hat, s, u, out, cfg_scale=cfg_scale, out2=out2)


def ddim_invert_step_cfg_dev(x, eps2, alpha_hat, s_dev, u_dev, cfg_scale, out, out2=None):
    """ddim_invert_step_cfg with the levels read on the device (graph-replayable)."""
    return _ddim_invert("guided DDIM invert step", x, eps2, alpha_hat, s_dev, u_dev, out, cfg_scale=cfg_scale, out2=out2, dev=True)


SLERP_MAX_ROW = 3 * 64 * 64


def slerp(a, b, weights):
    """Spherical interpolation of the rows of a towards those of b (include/afd.h: afd_slerp_rows gives the exact expression; rows
    that are parallel, antiparallel or zero are interpolated linearly).  a, b: contiguous fp32 (n, ...) device tensors of one
    shape, at most 3 * 64 * 64 values per row; weights: a 1-D sequence or tensor of W finite numbers (0 gives a, 1 gives b, bit
    for bit).  One launch for all rows and weights.  Returns (n, W, ...): row (i, k) is pair i at weights[k]."""
    for v in (a, b):
        if not isinstance(v, torch.Tensor):
            raise AfdError("afdm: slerp: a and b must be tensors")
    _chk(a, b)
    if a.dim() < 2 or a.shape != b.shape or a.shape[0] < 1:
        raise AfdError(f"afdm: slerp: a and b must be (n, ...) tensors of one shape, n >= 1 (got {tuple(a.shape)} and {tuple(b.shape)})")
    if not a.is_contiguous() or not b.is_contiguous():
        raise AfdError("afdm: slerp: a and b must be contiguous")
    n, row = a.shape[0], a.numel() // a.shape[0]
    if not 1 <= row <= SLERP_MAX_ROW:
        raise AfdError(f"afdm: slerp: a row must hold between 1 and {SLERP_MAX_ROW} values (got {row})")
    if isinstance(weights, torch.Tensor) and (weights.dtype.is_complex or weights.dtype == torch.bool):
        raise AfdError(f"afdm: slerp: weights must be real numbers (got {weights.dtype})")
    try:
        w = torch.as_tensor(weights).detach().to(device="cpu", dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise AfdError("afdm: slerp: weights must be a 1-D sequence or tensor of numbers") from None
    if w.dim() != 1 or w.numel() < 1 or not bool(torch.isfinite(w).all()):
        raise AfdError(f"afdm: slerp: weights must be a non-empty 1-D sequence of finite numbers (got shape {tuple(w.shape)})")
    w = w.to(device=a.device, dtype=torch.float32)
    out = torch.empty((n, w.numel()) + tuple(a.shape[1:]), device=a.device, dtype=torch.float32)
    lib().afd_slerp_rows(_p(a), _p(b), _p(w), _p(out), n, w.numel(), row, _stream())
    return out


def _dpmpp_args(what, x, eps, x0_prev, coef, out, x0_out, out2=None, guided=False):
    n = _step_args(what, x, eps, x0_prev, coef, out, out2, guided)
    _chk(x0_out)
    if coef.numel() != 5:
        raise AfdError(f"afdm: {what} needs coef of 5 values [alpha_t, sigma_t, A, B0, B1] (got {coef.numel()})")
    if not x0_out.is_contiguous() or x0_out.numel() != n:
        raise AfdError(f"afdm: {what}: x0_out must be contiguous and hold {n} elements")
    return n


def dpmpp_step(x, eps, x0_prev, coef, out=None, x0_out=None):
    """DPM-Solver++(2M) update t -> t_prev (include/afd.h: afd_dpmpp_step gives the exact expression).  coef: the step's row of
    `Diffusion.dpmpp_coefficients`, 5 fp32 values on the device (read there: graph-replayable).  x0_prev: None on a first-order
    step, else the previous step's x0.  `out` may be x; `x0_out` may be x0_prev (in place).  Returns (out, x0_out)."""
    out = torch.empty_like(x) if out is None else out
    x0_out = torch.empty_like(x) if x0_out is None else x0_out
    n = _dpmpp_args("DPM++ step", x, eps, x0_prev, coef, out, x0_out)
    lib().afd_dpmpp_step(_p(x), _p(eps), _p(x0_prev), _p(coef), _p(out), _p(x0_out), n, _stream())
    return out, x0_out


def dpmpp_step_cfg(x, eps2, x0_prev, coef, cfg_scale, out=None, out2=None, x0_out=None):
    """Classifier-free guided DPM++ update: e = torch.lerp(eps2[n:], eps2[:n], cfg_scale), then exactly `dpmpp_step(x, e, ...)`,
    in one launch.  `out2` (optional) receives the same values as `out`.  Returns (out, x0_out)."""
    out = torch.empty_like(x) if out is None else out
    x0_out = torch.empty_like(x) if x0_out is None else x0_out
    n = _dpmpp_args("guided DPM++ step", x, eps2, x0_prev, coef, out, x0_out, out2, guided=True)
    lib().afd_dpmpp_step_cfg(_p(x), _p(eps2), _p(x0_prev), _p(coef), float(cfg_scale), _p(out), _p(out2), _p(x0_out), n, _stream())
    return out, x0_out


def _unipc_args(what, x, eps, xc, hist, coef, out, out2=None, guided=False):
    n = _step_args(what, x, eps, xc, coef, out, out2, guided)
    _chk(hist)
    if coef.numel() != 12:
        raise AfdError(f"afdm: {what} needs coef of 12 values [alpha, sigma, Ac, c0..c3, Ap, p0..p2, slot] (got {coef.numel()})")
    if not hist.is_contiguous() or hist.numel() != 3 * n:
        raise AfdError(f"afdm: {what}: hist must be contiguous and hold 3 x {n} elements")
    return n


def unipc_step(x, eps, xc, hist, coef, out=None):
    """One UniPC evaluation: the corrector of the last move and the predictor of the next (include/afd.h: afd_unipc_step gives the
    exact expression).  coef: the evaluation's row of `Diffusion.unipc_coefficients`, 12 fp32 values on the device (read there:
    graph-replayable).  xc (the corrected state, n elements) and hist (the ring of the last three m, 3n elements) are the
    solver's state, updated in place.  `out` may be x.  Returns out, the predicted state of the next level."""
    out = torch.empty_like(x) if out is None else out
    n = _unipc_args("UniPC step", x, eps, xc, hist, coef, out)
    lib().afd_unipc_step(_p(x), _p(eps), _p(xc), _p(hist), _p(coef), _p(out), n, _stream())
    return out


def unipc_step_cfg(x, eps2, xc, hist, coef, cfg_scale, out=None, out2=None):
    """Classifier-free guided UniPC evaluation: e = torch.lerp(eps2[n:], eps2[:n], cfg_scale), then exactly
    `unipc_step(x, e, ...)`, in one launch.  `out2` (optional) receives the same values as `out`.  Returns out."""
    out = torch.empty_like(x) if out is None else out
    n = _unipc_args("guided UniPC step", x, eps2, xc, hist, coef, out, out2, guided=True)
    lib().afd_unipc_step_cfg(_p(x), _p(eps2), _p(xc), _p(hist), _p(coef), float(cfg_scale), _p(out), _p(out2), n, _stream())
    return out


# ---- likelihood: gathered noising, the bound's per-row terms, the prior (include/afd.h gives the exact expressions) ---------
def _rows_args(what, x0, img, t, rows_like, check_range, T=None):
    """Common checks of the row-wise entry points -> (n_img, rows, per).  img / t: int64 device vectors of one value per row;
    check_range: verify on the host (one device sync) that img lies in [0, n_img) and t in [1, T); callers that built them on
    the host and checked them there pass False."""
    _chk(x0, rows_like)
    if x0.dim() < 2 or not x0.is_contiguous() or not rows_like.is_contiguous():
        raise AfdError(f"afdm: {what}: x0 (n_img, ...) and the row tensors must be contiguous")
    n_img, per = x0.shape[0], x0.numel() // max(x0.shape[0], 1)
    rows = rows_like.shape[0]
    if rows_like.numel() != rows * per:
        raise AfdError(f"afdm: {what}: the row tensors must hold {per} values per row like x0 (got shape {tuple(rows_like.shape)})")
    for name, v in (("img", img), ("t", t)):
        if not v.is_cuda or v.dtype != torch.long or v.dim() != 1 or v.numel() != rows or not v.is_contiguous():
            raise AfdError(f"afdm: {what}: {name} must be a contiguous int64 device vector of {rows} values")
    if check_range and rows > 0:
        lo_i, hi_i, lo_t, hi_t = (int(v) for v in torch.stack([img.min(), img.max(), t.min(), t.max()]).cpu())
        if lo_i < 0 or hi_i >= n_img:
            raise AfdError(f"afdm: {what}: img must lie in [0, {n_img}) (got {lo_i} .. {hi_i})")
        if lo_t < 1 or hi_t >= (T if T is not None else 1 << 62):
            raise AfdError(f"afdm: {what}: t must lie in [1, {T}) (got {lo_t} .. {hi_t})")
    return n_img, rows, per


def noise_images_gather(x0, img, eps, t, alpha_hat, out=None, check_range=True):
    """x_t of the rows (img[r], t[r]): `noise_images(x0[img], eps, t, alpha_hat)` bit for bit, without the gather.
    x0: (n_img, C, H, W); img, t: (rows,) int64 device; eps: (rows, C, H, W)."""
    out = torch.empty_like(eps) if out is None else out
    n_img, rows, per = _rows_args("gathered noising", x0, img, t, eps, check_range, alpha_hat.numel())
    _chk(alpha_hat, out)
    if out.shape != eps.shape or not out.is_contiguous():
        raise AfdError("afdm: gathered noising: out must be contiguous and shaped like eps")
    lib().afd_noise_images_gather(_p(x0), n_img, _p(img), _p(eps), _p(t), _p(alpha_hat), _p(out), rows, per, _stream())
    return out


def vlb_terms(x0, img, x_t, eps, eps_hat, t, coef, alpha, alpha_hat, beta, term=None, sq=None, check_range=True):
    """The bound's term of each row, in nats, and sum_j (eps_hat - eps)^2, both fp64 (rows,) device tensors (include/afd.h:
    afd_vlb_terms).  coef: the (T, 4) fp64 table of `Diffusion.vlb_coefficients` on the device.  Returns (term, sq)."""
    n_img, rows, per = _rows_args("bound terms", x0, img, t, eps, check_range, alpha_hat.numel())
    _chk(x_t, eps_hat, alpha, alpha_hat, beta)
    for v in (x_t, eps_hat):
        if v.shape != eps.shape or not v.is_contiguous():
            raise AfdError("afdm: bound terms: x_t and eps_hat must be contiguous and shaped like eps")
    T = alpha_hat.numel()
    if not coef.is_cuda or coef.dtype != torch.float64 or tuple(coef.shape) != (T, 4) or not coef.is_contiguous():
        raise AfdError(f"afdm: bound terms: coef must be the contiguous ({T}, 4) fp64 device table (Diffusion.vlb_coefficients)")
    term = torch.empty(rows, device=eps.device, dtype=torch.float64) if term is None else term
    sq = torch.empty(rows, device=eps.device, dtype=torch.float64) if sq is None else sq
    for v in (term, sq):
        if not v.is_cuda or v.dtype != torch.float64 or v.numel() != rows or not v.is_contiguous():
            raise AfdError(f"afdm: bound terms: term and sq must be contiguous fp64 device tensors of {rows} values")
    lib().afd_vlb_terms(_p(x0), n_img, _p(img), _p(x_t), _p(eps), _p(eps_hat), _p(t), _p(coef), T, _p(alpha), _p(alpha_hat),
                        _p(beta), _p(term), _p(sq), rows, per, _stream())
    return term, sq


def vlb_prior(x0, half_ah, out=None):
    """half_ah * sum_j x0[i, j]^2 per image in fp64 (the prior's data-dependent part), an (n_img,) fp64 device tensor."""
    _chk(x0)
    if x0.dim() < 2 or not x0.is_contiguous():
        raise AfdError("afdm: prior: x0 must be a contiguous (n_img, ...) tensor")
    n_img, per = x0.shape[0], x0.numel() // max(x0.shape[0], 1)
    out = torch.empty(n_img, device=x0.device, dtype=torch.float64) if out is None else out
    if not out.is_cuda or out.dtype != torch.float64 or out.numel() != n_img or not out.is_contiguous():
        raise AfdError(f"afdm: prior: out must be a contiguous fp64 device tensor of {n_img} values")
    lib().afd_vlb_prior(_p(x0), float(half_ah), _p(out), n_img, per, _stream())
    return out


# ---- inpainting: masked steps and the renoise up-move (include/afd.h gives the exact expressions) --------------------------
def denoise_step_masked(x, eps, noise, x0, mask, alpha, alpha_hat, beta, i, out=None):
    """Masked DDPM update i -> i - 1: where mask is 0, `denoise_step`; where it is 1, x0 noised to i - 1 with the same noise
    (x0 itself at i == 1, where noise may be None).  `out` may be x (in place)."""
    return _step("masked denoise step", x, eps, noise, (alpha, alpha_hat, beta), (i,), out, x0=x0, mask=mask, masked=True)


def denoise_step_masked_dev(x, eps, noise, x0, mask, alpha, alpha_hat, beta, t_dev, out):
    """denoise_step_masked with the step index t_dev[0] read on the device (graph-replayable); noise is required."""
    return _step("masked denoise step", x, eps, noise, (alpha, alpha_hat, beta), (t_dev,), out, x0=x0, mask=mask, masked=True, dev=True)


def denoise_step_masked_cfg(x, eps2, noise, x0, mask, alpha, alpha_hat, beta, i, cfg_scale, out=None, out2=None):
    """The guided form of denoise_step_masked (eps2 as for denoise_step_cfg); `out2` (optional) receives the same values."""
    return _step("guided masked denoise step", x, eps2, noise, (alpha, alpha_hat, beta), (i,), out, cfg_scale=cfg_scale, out2=out2,
                 x0=x0, mask=mask, masked=True)


def denoise_step_masked_cfg_dev(x, eps2, noise, x0, mask, alpha, alpha_hat, beta, t_dev, cfg_scale, out, out2=None):
    return _step("guided masked denoise step", x, eps2, noise, (alpha, alpha_hat, beta), (t_dev,), out, cfg_scale=cfg_scale, out2=out2,
                 x0=x0, mask=mask, masked=True, dev=True)


def ddim_step_masked(x, eps, noise, x0, mask, alpha_hat, t, t_prev, eta, out=None):
    """Masked DDIM update t -> t_prev: where mask is 0, `ddim_step` (no noise term when eta == 0); where it is 1, x0 noised to
    t_prev with the same noise (x0 itself at t_prev == 0, where noise may be None).  `out` may be x (in place)."""
    return _step("masked DDIM step", x, eps, noise, (alpha_hat,), (t, t_prev), out, eta=eta, x0=x0, mask=mask, masked=True)


def ddim_step_masked_dev(x, eps, noise, x0, mask, alpha_hat, t_dev, t_prev_dev, eta, out):
    return _step("masked DDIM step", x, eps, noise, (alpha_hat,), (t_dev, t_prev_dev), out, eta=eta, x0=x0, mask=mask, masked=True,
                 dev=True)


def ddim_step_masked_cfg(x, eps2, noise, x0, mask, alpha_hat, t, t_prev, eta, cfg_scale, out=None, out2=None):
    return _step("guided masked DDIM step", x, eps2, noise, (alpha_hat,), (t, t_prev), out, eta=eta, cfg_scale=cfg_scale, out2=out2,
                 x0=x0, mask=mask, masked=True)


def ddim_step_masked_cfg_dev(x, eps2, noise, x0, mask, alpha_hat, t_dev, t_prev_dev, eta, cfg_scale, out, out2=None):
    return _step("guided masked DDIM step", x, eps2, noise, (alpha_hat,), (t_dev, t_prev_dev), out, eta=eta, cfg_scale=cfg_scale,
                 out2=out2, x0=x0, mask=mask, masked=True, dev=True)


def renoise(x, noise, alpha_hat, t_from, t_to, out=None):
    """q(x_{t_to} | x_{t_from}) in one jump: sqrt(a) * x + sqrt(1 - a) * noise, a = alpha_hat[t_to] / alpha_hat[t_from].
    `out` may be x (in place)."""
    out = torch.empty_like(x) if out is None else out
    n = _step_args("renoise", x, noise, None, alpha_hat, out)
    t_from, t_to = int(t_from), int(t_to)
    if not 0 <= t_from < t_to < alpha_hat.numel():
        raise AfdError(f"afdm: renoise needs 0 <= t_from < t_to < {alpha_hat.numel()} (got {t_from}, {t_to})")
    lib().afd_renoise(_p(x), _p(noise), _p(alpha_hat), t_from, t_to, _p(out), n, _stream())
    return out


# ---- reference-guided sampling (ILVR): the fused low-pass refinement (include/afd.h gives the exact expressions) -------------
REFINE_SIDES = (4, 8, 16, 32, 64)


def _refine_args(what, x, ref, noise, alpha_hat, taps, levels, out, out2):
    """The argument check of the refine wrappers -> (taps, levels, planes, S).  x: (..., S, S), S a power of two in [4, 64];
    ref, noise (or None), out and out2 (or None) hold as many elements; taps: an N x N filter, N odd and at most 15."""
    _step_args(what, x, ref, noise, alpha_hat, out, out2)
    if x.dim() < 2 or x.shape[-1] != x.shape[-2] or x.shape[-1] not in REFINE_SIDES:
        raise AfdError(f"afdm: {what} needs square planes (..., S, S) with S a power of two in [4, 64] (got shape {tuple(x.shape)})")
    S = int(x.shape[-1])
    taps = Taps.of(taps)
    if taps.N % 2 == 0 or taps.N > 15:
        raise AfdError(f"afdm: {what} needs an N x N filter with N odd and at most 15 (got N = {taps.N}): an even N shifts the image")
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1 or (S >> int(levels)) < 2:
        raise AfdError(f"afdm: {what} needs an int levels >= 1 with S / 2^levels >= 2 (got levels = {levels!r}, S = {S})")
    return taps, int(levels), x.numel() // (S * S), S


def lowpass_refine(x, ref, noise, alpha_hat, t_prev, taps, levels, out=None, out2=None):
    """ILVR's refinement x + phi(known - x) in one launch: phi = 4^levels up2^levels(down2^levels(.)) with `taps` (an N x N array,
    tensor or ops.Taps), known = ref noised to t_prev with `noise` (ref itself at t_prev == 0, where noise may be None).
    x: (..., S, S).  `out` may be x (in place); `out2` (optional) receives the same values."""
    out = torch.empty_like(x) if out is None else out
    taps, levels, planes, S = _refine_args("low-pass refine", x, ref, noise, alpha_hat, taps, levels, out, out2)
    t_prev = int(t_prev)
    if not 0 <= t_prev < alpha_hat.numel():
        raise AfdError(f"afdm: low-pass refine needs 0 <= t_prev < {alpha_hat.numel()} (got {t_prev})")
    lib().afd_lowpass_refine(_p(x), _p(ref), _p(noise), _p(alpha_hat), t_prev, taps.ptr, taps.N, levels, _p(out), _p(out2), planes, S,
                             _stream())
    return out


def lowpass_refine_dev(x, ref, noise, alpha_hat, t_prev_dev, taps, levels, out, out2=None):
    """lowpass_refine with t_prev = t_prev_dev[0] read on the device (graph-replayable); noise is required (ignored at 0)."""
    taps, levels, planes, S = _refine_args("low-pass refine", x, ref, noise, alpha_hat, taps, levels, out, out2)
    if not t_prev_dev.is_cuda or t_prev_dev.dtype != torch.long or t_prev_dev.numel() < 1:
        raise AfdError("afdm: low-pass refine: t_prev_dev must be an int64 device tensor (element 0 is read)")
    lib().afd_lowpass_refine_dev(_p(x), _p(ref), _p(noise), _p(alpha_hat), _p(t_prev_dev), taps.ptr, taps.N, levels, _p(out), _p(out2),
                                 planes, S, _stream())
    return out


def lowpass_project(v, taps, levels):
    """phi(v) = 4^levels up2^levels(down2^levels(v)) with `taps`: the refine launch with x = 0, t_prev = 0 and ref = v."""
    _chk(v)
    zero = torch.zeros_like(v, memory_format=torch.contiguous_format)
    # (t_prev = 0 reads no schedule: the first zero stands in for the table, whose pointer must not be NULL)
    return lowpass_refine(zero, _c(v), None, zero.view(-1)[:1], 0, taps, levels, out=zero)


def quantize_u8(x):
    _chk(x)
    x = _c(x)
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    lib().afd_quantize_u8(_p(x), _p(out), x.numel(), _stream())
    return out


def rotate_affine(degrees, H, W):
    """The (matrix, offset) scipy.ndimage.rotate builds for an (H, W) plane: in = matrix @ out + offset, fp64 host arrays."""
    import math
    a = np.deg2rad(degrees)
    cs, sn = math.cos(a), math.sin(a)
    m = np.array([[cs, sn], [-sn, cs]], dtype=np.float64)                  # scipy.ndimage.rotate's rot_matrix
    plane = np.array([H, W], dtype=np.float64)
    off = (plane - 1) / 2 - m @ ((plane - 1) / 2)                           # in_center - rot @ out_center
    return np.ascontiguousarray(m), np.ascontiguousarray(off)


def rotate_spline3_wrap(x, degrees):
    """scipy.ndimage.rotate(x, degrees, axes=(2,3), reshape=False, order=3, mode='grid-wrap') on the device."""
    _chk(x)
    x = _c(x)
    n, c, H, W = x.shape
    m, off = rotate_affine(degrees, H, W)
    y = torch.empty_like(x)
    ws = torch.empty(n * c * H * W, device=x.device, dtype=torch.float64)
    lib().afd_affine_spline3_wrap(_p(x), _p(y), n * c, H, W, m.ctypes.data, off.ctypes.data, _p(ws), _stream())
    return y


def affine_spline3_wrap(x, matrix, offset):
    """scipy.ndimage.affine_transform(plane, matrix, offset, order=3, mode='grid-wrap') of every (H, W) plane of x (n, C, H, W)
    on the device: in = matrix @ out + offset in (row, col) order, matrix 2 x 2 and offset 2 host values."""
    _chk(x)
    x = _c(x)
    n, c, H, W = x.shape
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64).reshape(2, 2))
    off = np.ascontiguousarray(np.asarray(offset, dtype=np.float64).reshape(2))
    y = torch.empty_like(x)
    ws = torch.empty(n * c * H * W, device=x.device, dtype=torch.float64)
    lib().afd_affine_spline3_wrap(_p(x), _p(y), n * c, H, W, m.ctypes.data, off.ctypes.data, _p(ws), _stream())
    return y


# ---- equivariance scores: prefilter once, resample / compare row-wise (include/afd.h gives the exact expressions) -----------
def spline3_prefilter_wrap(x, out=None):
    """fp64 cubic B-spline coefficients (periodic) of every (H, W) plane of x (n, C, H, W) fp32: the prefilter of
    `rotate_spline3_wrap`, done once for any number of `affine_spline3_wrap_rows` / `eq_terms` calls."""
    _chk(x)
    if x.dim() != 4 or not x.is_contiguous():
        raise AfdError("afdm: spline prefilter: x must be a contiguous (n, C, H, W) tensor")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float64) if out is None else out
    if not out.is_cuda or out.dtype != torch.float64 or out.shape != x.shape or not out.is_contiguous():
        raise AfdError("afdm: spline prefilter: out must be a contiguous fp64 device tensor shaped like x")
    n, c, H, W = x.shape
    lib().afd_spline3_prefilter_wrap(_p(x), _p(out), n * c, H, W, _stream())
    return out


def _affine_rows_args(what, coef, img, affine, k, check_range):
    """Common checks of the row-wise spline entry points -> (n_src, K, rows, C, H, W)."""
    if not coef.is_cuda or coef.dtype != torch.float64 or coef.dim() != 4 or not coef.is_contiguous():
        raise AfdError(f"afdm: {what}: coef must be a contiguous (n_src, C, H, W) fp64 device tensor (spline3_prefilter_wrap)")
    if not affine.is_cuda or affine.dtype != torch.float64 or affine.dim() != 2 or affine.shape[1] != 6 or affine.shape[0] < 1 \
            or not affine.is_contiguous():
        raise AfdError(f"afdm: {what}: affine must be a contiguous (K, 6) fp64 device table (Diffusion.equivariance_transforms)")
    rows = img.numel() if isinstance(img, torch.Tensor) else -1
    for name, v in (("img", img), ("k", k)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.long or v.dim() != 1 or v.numel() != rows \
                or not v.is_contiguous():
            raise AfdError(f"afdm: {what}: {name} must be a contiguous int64 device vector, one value per row")
    n_src, K = coef.shape[0], affine.shape[0]
    if check_range and rows > 0:
        lo_i, hi_i, lo_k, hi_k = (int(v) for v in torch.stack([img.min(), img.max(), k.min(), k.max()]).cpu())
        if lo_i < 0 or hi_i >= n_src:
            raise AfdError(f"afdm: {what}: img must lie in [0, {n_src}) (got {lo_i} .. {hi_i})")
        if lo_k < 0 or hi_k >= K:
            raise AfdError(f"afdm: {what}: k must lie in [0, {K}) (got {lo_k} .. {hi_k})")
    return (n_src, K, rows) + tuple(coef.shape[1:])


def affine_spline3_wrap_rows(coef, img, affine, k, out=None, check_range=True):
    """Row r = source field img[r] of `coef` (n_src, C, H, W; `spline3_prefilter_wrap`) resampled by transform k[r] of the (K, 6)
    fp64 device table `affine`, rounded once to fp32: (rows, C, H, W).  Bit for bit what `rotate_spline3_wrap` /
    `affine_spline3_wrap` return for that field and that transform.  img, k: (rows,) int64 device."""
    n_src, K, rows, C, H, W = _affine_rows_args("row-wise resampling", coef, img, affine, k, check_range)
    out = torch.empty((rows, C, H, W), device=coef.device, dtype=torch.float32) if out is None else out
    if not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (rows, C, H, W) or not out.is_contiguous():
        raise AfdError(f"afdm: row-wise resampling: out must be a contiguous fp32 device tensor of shape {(rows, C, H, W)}")
    lib().afd_affine_spline3_wrap_rows(_p(coef), n_src, _p(img), _p(affine), K, _p(k), _p(out), rows, C, H, W, _stream())
    return out


def eq_terms(coef_ref, img, affine, k, g, margin, out=None, check_range=True):
    """The equivariance sums of each row, a (rows, 3) fp64 device tensor [sum d^2, sum ref^2, masked pixels * C] with
    ref = field img[r] of `coef_ref` under transform k[r], evaluated in fp64 and never stored, d = double(g[r]) - ref, over the
    transform's validity mask for `margin` (include/afd.h: afd_eq_terms).  g: (rows, C, H, W) fp32."""
    n_src, K, rows, C, H, W = _affine_rows_args("equivariance terms", coef_ref, img, affine, k, check_range)
    _chk(g)
    if tuple(g.shape) != (rows, C, H, W) or not g.is_contiguous():
        raise AfdError(f"afdm: equivariance terms: g must be a contiguous fp32 tensor of shape {(rows, C, H, W)}")
    margin = float(margin)
    if not (0.0 <= margin < float("inf")):
        raise AfdError(f"afdm: equivariance terms: margin must be finite and >= 0 (got {margin})")
    out = torch.empty((rows, 3), device=g.device, dtype=torch.float64) if out is None else out
    if not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (rows, 3) or not out.is_contiguous():
        raise AfdError(f"afdm: equivariance terms: out must be a contiguous fp64 device tensor of shape {(rows, 3)}")
    lib().afd_eq_terms(_p(coef_ref), n_src, _p(img), _p(affine), K, _p(k), _p(g), margin, _p(out), rows, C, H, W, _stream())
    return out


class MseLoss(_Fn):
    """nn.MSELoss() (mean reduction), deterministic two-stage sum  (ddpm_utils.py:490,503)."""

    @staticmethod
    def forward(ctx, target, pred):
        _chk(target, pred)
        target, pred = _c(target), _c(pred)
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        ws = torch.empty(4096, device=pred.device, dtype=torch.float32)
        lib().afd_mse_fwd(_p(pred), _p(target), _p(loss), _p(ws), pred.numel(), _stream())
        ctx.save_for_backward(target, pred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        target, pred = ctx.saved_tensors
        dloss = dloss.reshape(1).contiguous()
        dpred = torch.empty_like(pred)
        lib().afd_mse_bwd(_p(pred), _p(target), _p(dloss), _p(dpred), pred.numel(), _stream())
        return None, dpred


def mse_loss(target, pred):
    return MseLoss.apply(target, pred)


PRED_KINDS = {"eps": 0, "v": 1, "x0": 2}          # AFD_PRED_EPS / AFD_PRED_V / AFD_PRED_X0 of afd.h


def _pred_tensors(what, kind, tables, tensors, min_dim, shape):
    """_objective_args' and _lvar_args' first checks: kind; fp32 device tensors; `tensors` contiguous, of one shape -> the first"""
    if not isinstance(kind, str) or kind not in PRED_KINDS:
        raise AfdError(f"afdm: {what}: unknown prediction {kind!r} ('eps', 'v' or 'x0')")
    if any(not isinstance(o, torch.Tensor) for o in tables + tensors):
        raise AfdError(f"afdm: {what}: every argument but kind must be a tensor")
    _chk(*tables, *tensors)
    first = tensors[0]
    if first.dim() < min_dim or first.numel() == 0:
        raise AfdError(f"afdm: {what}: needs tensors of shape {shape} with at least one element")
    for o in tensors:
        if tuple(o.shape) != tuple(first.shape) or not o.is_contiguous():
            raise AfdError(f"afdm: {what}: every tensor must be contiguous and of shape {tuple(first.shape)}")
    return first


def _row_t_and_table(what, t, alpha_hat, B, t_optional=False):
    """and their last: t a (B,) int64 device tensor (its values are read unchecked; t_optional: or None), alpha_hat a (T,) table"""
    if not (t is None and t_optional) and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.long
                                           or tuple(t.shape) != (B,) or not t.is_contiguous()):
        raise AfdError(f"afdm: {what}: t must be a contiguous int64 device tensor of shape ({B},)")
    if alpha_hat.dim() != 1 or not alpha_hat.is_contiguous():
        raise AfdError(f"afdm: {what}: alpha_hat must be a contiguous (T,) table")


def _objective_args(what, kind, t, alpha_hat, *tensors):
    """-> (AFD_PRED_* code, B, chw) after checking the tensors of one of the objective kernels: `tensors` (B, ...) fp32 device
    tensors of one shape, contiguous; t (B,) int64 on the device; alpha_hat (T,) fp32."""
    first = _pred_tensors(what, kind, (alpha_hat,), tensors, 1, "(B, ...)")
    B = first.shape[0]
    _row_t_and_table(what, t, alpha_hat, B)
    return PRED_KINDS[kind], B, first.numel() // B


class ObjectiveLoss(_Fn):
    """(1 / (B chw)) sum_b w[t_b] sum_i (pred - target)^2 with the target of `kind` formed inside the kernels from x0, eps and
    alpha_hat[t_b] (afd.h: afd_objective_loss_fwd / _bwd): two launches forward and one backward, like MseLoss."""

    @staticmethod
    def forward(ctx, pred, x0, eps, t, alpha_hat, w, kind):
        pred, x0, eps = _c(pred), _c(x0), _c(eps)
        code, B, chw = _objective_args("objective loss", kind, t, alpha_hat, pred, x0, eps)
        if w is not None:
            _chk(w)
            if tuple(w.shape) != tuple(alpha_hat.shape) or not w.is_contiguous():
                raise AfdError(f"afdm: objective loss: w must be a contiguous table of alpha_hat's shape {tuple(alpha_hat.shape)}")
        loss = torch.empty(1, device=pred.device, dtype=torch.float32)
        ws = torch.empty(4096, device=pred.device, dtype=torch.float32)
        lib().afd_objective_loss_fwd(_p(pred), _p(x0), _p(eps), _p(t), _p(alpha_hat), _p(w), code, _p(loss), _p(ws), B, chw, _stream())
        ctx.save_for_backward(pred, x0, eps, t, alpha_hat, w)
        ctx.code = code
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        pred, x0, eps, t, alpha_hat, w = ctx.saved_tensors
        dloss = dloss.reshape(1).contiguous()
        dpred = torch.empty_like(pred)
        B = pred.shape[0]
        lib().afd_objective_loss_bwd(_p(pred), _p(x0), _p(eps), _p(t), _p(alpha_hat), _p(w), ctx.code, _p(dloss), _p(dpred), B,
                                     pred.numel() // B, _stream())
        return dpred, None, None, None, None, None, None


def objective_loss(pred, x0, eps, t, alpha_hat, w=None, kind="eps"):
    """The training loss of a network whose output `pred` means `kind` ("eps", "v" or "x0"), per-row weights w[t] (a (T,) fp32
    device table, None = 1), normalised by the element count.  Differentiable in pred only."""
    return ObjectiveLoss.apply(pred, x0, eps, t, alpha_hat, w, kind)


def pred_to_eps(out, x_t, t, alpha_hat, kind, eps_out=None):
    """The network's output `out` at x_t with per-row timesteps t (int64, on the device) -> eps, one launch (afd.h:
    afd_pred_to_eps).  kind: "v" or "x0" ("eps" needs no conversion and is an error).  eps_out may be `out` (in place)."""
    eps_out = torch.empty_like(out) if eps_out is None else eps_out
    code, B, chw = _objective_args("pred_to_eps", kind, t, alpha_hat, out, x_t, eps_out)
    lib().afd_pred_to_eps(_p(out), _p(x_t), _p(t), _p(alpha_hat), code, _p(eps_out), B, chw, _stream())
    return eps_out


# ---- progressive distillation: the teacher's two DDIM steps per row (include/afd.h gives the exact expressions) ---------------
def distill_mid(out1, z_t, t, t_mid, alpha_hat, kind, out=None):
    """The teacher's raw output `out1` at (z_t, t) -> z_mid, its deterministic DDIM step t -> t_mid with per-row timesteps (int64,
    on the device), evaluated in fp64 and rounded once; one launch (afd.h: afd_distill_mid).  kind: "eps", "v" or "x0".  out may
    be out1 or z_t (in place)."""
    out = torch.empty_like(out1) if out is None else out
    code, B, chw = _objective_args("distill_mid", kind, t, alpha_hat, out1, z_t, out)
    _row_t_and_table("distill_mid", t_mid, alpha_hat, B)
    lib().afd_distill_mid(_p(out1), _p(z_t), _p(t), _p(t_mid), _p(alpha_hat), code, _p(out), B, chw, _stream())
    return out


def distill_target(out2, z_mid, z_t, t, t_mid, t_prev, alpha_hat, kind, x_out=None, eps_out=None):
    """The teacher's raw output `out2` at (z_mid, t_mid) -> (x_tilde, eps_tilde): its DDIM step t_mid -> t_prev (t_prev = 0: the
    chain's last level, alpha_hat[0] as in `ddim_step`) folded with z_t into the (x0, eps) pair whose ONE DDIM step from z_t lands where the teacher's two did; fp64 per
    element, rounded once; one launch (afd.h: afd_distill_target).  x_out / eps_out may each be one of out2, z_mid, z_t."""
    x_out = torch.empty_like(out2) if x_out is None else x_out
    eps_out = torch.empty_like(out2) if eps_out is None else eps_out
    code, B, chw = _objective_args("distill_target", kind, t, alpha_hat, out2, z_mid, z_t, x_out, eps_out)
    _row_t_and_table("distill_target", t_mid, alpha_hat, B)
    _row_t_and_table("distill_target", t_prev, alpha_hat, B)
    lib().afd_distill_target(_p(out2), _p(z_mid), _p(z_t), _p(t), _p(t_mid), _p(t_prev), _p(alpha_hat), code, _p(x_out), _p(eps_out),
                             B, chw, _stream())
    return x_out, eps_out


# ---- consistency distillation: the consistency function, its target and the sampler's step (include/afd.h has the expressions) ----
def _consistency_coef(what, coef, alpha_hat):
    """coef: the (T, 2) fp64 device table [c_skip, c_out] of `Diffusion.consistency_coefficients`"""
    T = alpha_hat.numel()
    if (not isinstance(coef, torch.Tensor) or not coef.is_cuda or coef.dtype != torch.float64 or tuple(coef.shape) != (T, 2)
            or not coef.is_contiguous()):
        raise AfdError(f"afdm: {what}: coef must be the contiguous ({T}, 2) float64 device table of Diffusion.consistency_coefficients")


def consistency_fn(out, z, t, alpha_hat, coef, kind, f_out=None):
    """The raw output `out` at (z, t) with per-row timesteps t (int64, on the device) -> f = c_skip[t] z + c_out[t] x_hat, fp64 per
    element and rounded once; z's bits where c_out[t] == 0 (t = 0), whatever `out` holds there; one launch (afd.h:
    afd_consistency_fn).  f_out may be out or z (in place)."""
    f_out = torch.empty_like(out) if f_out is None else f_out
    code, B, chw = _objective_args("consistency_fn", kind, t, alpha_hat, out, z, f_out)
    _consistency_coef("consistency_fn", coef, alpha_hat)
    lib().afd_consistency_fn(_p(out), _p(z), _p(t), _p(alpha_hat), _p(coef), code, _p(f_out), B, chw, _stream())
    return f_out


def consistency_target(out_tgt, z_prev, z_t, t, t_prev, alpha_hat, coef, kind, x_out=None, eps_out=None):
    """The target network's raw output `out_tgt` at (z_prev, t_prev) -> (x_tilde, eps_tilde): the x0 a student must predict at
    (z_t, t) for its consistency function to equal the target's f(z_prev, t_prev), and the eps that re-forms z_t with it; fp64 per
    element, rounded once; one launch (afd.h: afd_consistency_target).  Needs t >= 1 and t_prev < t per row (read on the device,
    unchecked); at t_prev == 0 the target is z_prev itself and out_tgt is not used.  x_out / eps_out may each be one of out_tgt,
    z_prev, z_t."""
    x_out = torch.empty_like(out_tgt) if x_out is None else x_out
    eps_out = torch.empty_like(out_tgt) if eps_out is None else eps_out
    code, B, chw = _objective_args("consistency_target", kind, t, alpha_hat, out_tgt, z_prev, z_t, x_out, eps_out)
    _row_t_and_table("consistency_target", t_prev, alpha_hat, B)
    _consistency_coef("consistency_target", coef, alpha_hat)
    lib().afd_consistency_target(_p(out_tgt), _p(z_prev), _p(z_t), _p(t), _p(t_prev), _p(alpha_hat), _p(coef), code, _p(x_out),
                                 _p(eps_out), B, chw, _stream())
    return x_out, eps_out


def _consistency_step_args(what, out, z, noise, alpha_hat, coef, kind, x_out):
    tensors = tuple(o for o in (out, z, noise, x_out) if o is not None)
    first = _pred_tensors(what, kind, (alpha_hat,), tensors, 1, "(n, ...)")
    if alpha_hat.dim() != 1 or not alpha_hat.is_contiguous():
        raise AfdError(f"afdm: {what}: alpha_hat must be a contiguous (T,) table")
    _consistency_coef(what, coef, alpha_hat)
    n = first.shape[0]
    return PRED_KINDS[kind], n, first.numel() // n


def consistency_step(out, z, noise, alpha_hat, coef, kind, t, t_next, x_out=None):
    """The consistency sampler's move at level t for every row: f = consistency_fn(out, z, t), then x_out = f at t_next == 0 (noise
    may be None) and noise_images(f, noise, t_next) otherwise, with the bits of those two calls, in one launch (afd.h:
    afd_consistency_step).  x_out may be z or out (in place)."""
    x_out = torch.empty_like(z) if x_out is None else x_out
    code, n, chw = _consistency_step_args("consistency_step", out, z, noise, alpha_hat, coef, kind, x_out)
    t, t_next = int(t), int(t_next)
    if not 0 <= t_next < t < alpha_hat.numel():
        raise AfdError(f"afdm: consistency_step needs 0 <= t_next < t < {alpha_hat.numel()} (got t = {t}, t_next = {t_next})")
    if noise is None and t_next > 0:
        raise AfdError("afdm: consistency_step needs noise unless t_next == 0")
    lib().afd_consistency_step(_p(out), _p(z), _p(noise), _p(alpha_hat), _p(coef), code, t, t_next, _p(x_out), n, chw, _stream())
    return x_out


def consistency_step_dev(out, z, noise, alpha_hat, coef, kind, t_dev, t_next_dev, x_out):
    """consistency_step with t = t_dev[0] and t_next = t_next_dev[0] read on the device (graph-replayable)."""
    code, n, chw = _consistency_step_args("consistency_step", out, z, noise, alpha_hat, coef, kind, x_out)
    _ddim_dev_t("consistency_step", t_dev, t_next_dev)
    lib().afd_consistency_step_dev(_p(out), _p(z), _p(noise), _p(alpha_hat), _p(coef), code, _p(t_dev), _p(t_next_dev), _p(x_out), n,
                                   chw, _stream())
    return x_out


# ---- learned reverse-process variances and the hybrid loss (include/afd.h gives the exact expressions) ----------------------
def _lvar_args(what, kind, out2, t, alpha_hat, lv_coef, *tensors, rows2=1):
    """-> (AFD_PRED_* code, B, chw): out2 is the contiguous (rows2 * B, 2C, ...) output of a learned-variance network, `tensors`
    are contiguous (B, C, ...) fp32 device tensors of one shape (None entries are skipped), t None or (B,) int64 on the device,
    lv_coef the (T, 3) fp64 device table of `Diffusion.lvar_coefficients`."""
    first = _pred_tensors(what, kind, (out2, alpha_hat), tuple(o for o in tensors if o is not None), 2, "(B, C, ...)")
    B, C = first.shape[0], first.shape[1]
    want = (rows2 * B, 2 * C) + tuple(first.shape[2:])
    if tuple(out2.shape) != want or not out2.is_contiguous():
        raise AfdError(f"afdm: {what}: the network's output must be contiguous and of shape {want}: {2 * C} channels, the "
                       f"prediction's {C} and the variance coefficient's {C} (got {tuple(out2.shape)})")
    _row_t_and_table(what, t, alpha_hat, B, t_optional=True)
    T = alpha_hat.numel()
    if lv_coef is not None and (not isinstance(lv_coef, torch.Tensor) or not lv_coef.is_cuda or lv_coef.dtype != torch.float64
                                or tuple(lv_coef.shape) != (T, 3) or not lv_coef.is_contiguous()):
        raise AfdError(f"afdm: {what}: lv_coef must be the contiguous ({T}, 3) fp64 device table (Diffusion.lvar_coefficients)")
    return PRED_KINDS[kind], B, first.numel() // B


def _lvar_tables(what, alpha, alpha_hat, beta, w=None, w_name="w"):
    _chk(alpha, beta, w)
    for name, v in (("alpha", alpha), ("beta", beta), (w_name, w)):
        if v is not None and (tuple(v.shape) != tuple(alpha_hat.shape) or not v.is_contiguous()):
            raise AfdError(f"afdm: {what}: {name} must be a contiguous table of alpha_hat's shape {tuple(alpha_hat.shape)}")


def _vlb_scale(what, vlb_scale):
    if isinstance(vlb_scale, bool) or not isinstance(vlb_scale, (int, float, np.integer, np.floating)) \
            or not np.isfinite(vlb_scale) or vlb_scale < 0:
        raise AfdError(f"afdm: {what}: vlb_scale must be a finite number >= 0 (got {vlb_scale!r})")
    return float(vlb_scale)


class LvarLoss(_Fn):
    """L = L_simple + vlb_scale * L_vlb of a learned-variance output (afd.h: afd_lvar_loss_fwd / _bwd): two launches forward and
    one backward, like ObjectiveLoss.  Returns (L, L_vlb, sums): two 0-d fp32 tensors and the (2,) fp64 tensor [L, L_vlb]; only L
    is differentiable."""

    @staticmethod
    def forward(ctx, out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, kind, vlb_scale, vw=None):
        out2, x0, eps = _c(out2), _c(x0), _c(eps)
        code, B, chw = _lvar_args("learned-variance loss", kind, out2, t, alpha_hat, lv_coef, x0, eps)
        _lvar_tables("learned-variance loss", alpha, alpha_hat, beta, w)
        _lvar_tables("learned-variance loss", alpha, alpha_hat, beta, vw, w_name="vw")
        scale = _vlb_scale("learned-variance loss", vlb_scale)
        aux = torch.empty(2, device=out2.device, dtype=torch.float32)
        aux64 = torch.empty(2, device=out2.device, dtype=torch.float64)
        ws = torch.empty(4096, device=out2.device, dtype=torch.float32)
        if vw is None:
            lib().afd_lvar_loss_fwd(_p(out2), _p(x0), _p(eps), _p(t), _p(alpha), _p(alpha_hat), _p(beta), _p(lv_coef), _p(w), code,
                                    scale, _p(aux), _p(aux64), _p(ws), B, chw, _stream())
        else:
            lib().afd_lvar_loss_fwd_tw(_p(out2), _p(x0), _p(eps), _p(t), _p(alpha), _p(alpha_hat), _p(beta), _p(lv_coef), _p(w), _p(vw),
                                       code, scale, _p(aux), _p(aux64), _p(ws), B, chw, _stream())
        ctx.save_for_backward(out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, vw)
        ctx.code, ctx.scale = code, scale
        loss, vlb = aux[0], aux[1]
        ctx.mark_non_differentiable(vlb, aux64)
        ctx.set_materialize_grads(False)          # (no zero-filled gradients for the two logging outputs: a launch each)
        return loss, vlb, aux64

    @staticmethod
    def backward(ctx, dloss, _daux=None, _daux64=None):
        out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, vw = ctx.saved_tensors
        dloss = dloss.reshape(1).contiguous()
        dout2 = torch.empty_like(out2)
        B = x0.shape[0]
        if vw is None:
            lib().afd_lvar_loss_bwd(_p(out2), _p(x0), _p(eps), _p(t), _p(alpha), _p(alpha_hat), _p(beta), _p(lv_coef), _p(w), ctx.code,
                                    ctx.scale, _p(dloss), _p(dout2), B, x0.numel() // B, _stream())
        else:
            lib().afd_lvar_loss_bwd_tw(_p(out2), _p(x0), _p(eps), _p(t), _p(alpha), _p(alpha_hat), _p(beta), _p(lv_coef), _p(w), _p(vw),
                                       ctx.code, ctx.scale, _p(dloss), _p(dout2), B, x0.numel() // B, _stream())
        return (dout2,) + (None,) * 11


def lvar_loss(out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w=None, kind="eps", vlb_scale=0.0, return_sums=False, vw=None):
    """The hybrid loss L_simple + vlb_scale * L_vlb (Nichol & Dhariwal 2021) of a network whose (B, 2C, ...) output holds the
    prediction (`kind`) and the variance coefficient.  L_simple is `objective_loss` on the prediction (weights w[t] included);
    L_vlb is the variational bound's term of each row in bits per dimension, averaged over the batch, with the mean stopped: the
    prediction's gradient is L_simple's, bit for bit, the coefficient's comes from L_vlb alone.  Returns (loss, L_vlb), two 0-d
    fp32 device tensors (L_vlb detached, unscaled); return_sums: also the (2,) fp64 device tensor [L, L_vlb].
    vw (a (T,) fp32 device table, None = 1): vw[t] multiplies each row's bound terms, and with them that row's gradient of the
    coefficient half -- the timestep sampler's importance weight (afd.h: afd_lvar_loss_fwd_tw / _bwd_tw); vw of ones gives the
    bits of vw=None."""
    loss, vlb, sums = LvarLoss.apply(out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, kind, vlb_scale, vw)
    if return_sums:
        return loss, vlb, sums
    return loss, vlb


# ---- loss-aware timestep sampling (include/afd.h and DESIGN.md section 6m give the semantics) ------------------------------------
def _rows_out(what, rows, B, device):
    if rows is None:
        return torch.empty(B, device=device, dtype=torch.float64)
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.float64 or tuple(rows.shape) != (B,) \
            or not rows.is_contiguous():
        raise AfdError(f"afdm: {what}: out must be a contiguous fp64 device tensor of shape ({B},)")
    return rows


def loss_rows(pred, x0, eps, t, alpha_hat, w=None, kind="eps", out=None):
    """Row b's share of `objective_loss`, times B: (1 / chw) w[t_b] sum_i (pred - target)^2 with the difference formed as the
    loss kernels form it and summed in fp64 -> (B,) fp64 device tensor; one launch (afd.h: afd_loss_rows).  No gradient."""
    pred, x0, eps = _c(pred), _c(x0), _c(eps)
    code, B, chw = _objective_args("loss_rows", kind, t, alpha_hat, pred, x0, eps)
    if w is not None:
        _chk(w)
        if tuple(w.shape) != tuple(alpha_hat.shape) or not w.is_contiguous():
            raise AfdError(f"afdm: loss_rows: w must be a contiguous table of alpha_hat's shape {tuple(alpha_hat.shape)}")
    out = _rows_out("loss_rows", out, B, pred.device)
    lib().afd_loss_rows(_p(pred), _p(x0), _p(eps), _p(t), _p(alpha_hat), _p(w), code, _p(out), B, chw, _stream())
    return out


def lvar_loss_rows(out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w=None, kind="eps", vlb_scale=0.0, out=None):
    """Row b's share of `lvar_loss`, times B: `loss_rows` on the prediction half plus (vlb_scale / (chw ln 2)) sum_i term_i
    -> (B,) fp64 device tensor; one launch (afd.h: afd_lvar_loss_rows).  No gradient."""
    out2, x0, eps = _c(out2), _c(x0), _c(eps)
    code, B, chw = _lvar_args("lvar_loss_rows", kind, out2, t, alpha_hat, lv_coef, x0, eps)
    if t is None or lv_coef is None:
        raise AfdError("afdm: lvar_loss_rows: t and lv_coef must be given")
    _lvar_tables("lvar_loss_rows", alpha, alpha_hat, beta, w)
    scale = _vlb_scale("lvar_loss_rows", vlb_scale)
    out = _rows_out("lvar_loss_rows", out, B, out2.device)
    lib().afd_lvar_loss_rows(_p(out2), _p(x0), _p(eps), _p(t), _p(alpha), _p(alpha_hat), _p(beta), _p(lv_coef), _p(w), code, scale,
                             _p(out), B, chw, _stream())
    return out


def eps_sqnorm_rows(eps, cfg_scale=None, out=None):
    """rows[b] = sum_i (double)e_i^2 over row b of the contiguous fp32 (B, ...) batch eps -> (B,) fp64 device tensor; one launch,
    a fixed summation tree (afd.h: afd_eps_sqnorm_rows).  cfg_scale given: eps holds the 2B-row guided forward and e =
    torch.lerp(eps[B:], eps[:B], cfg_scale), formed as the sampler steps form it.  No gradient."""
    _chk(eps)
    eps = _c(eps.detach())
    guided = cfg_scale is not None
    if eps.dim() < 2 or eps.shape[0] < 1 or eps.numel() == 0 or (guided and eps.shape[0] % 2):
        raise AfdError(f"afdm: eps_sqnorm_rows: eps must be a non-empty (B, ...) batch{', of 2B rows when guided' if guided else ''} "
                       f"(got {tuple(eps.shape)})")
    B = eps.shape[0] // 2 if guided else eps.shape[0]
    chw = eps.numel() // eps.shape[0]
    out = _rows_out("eps_sqnorm_rows", out, B, eps.device)
    if guided:
        lib().afd_eps_sqnorm_rows_cfg(_p(eps), float(cfg_scale), _p(out), B, chw, _stream())
    else:
        lib().afd_eps_sqnorm_rows(_p(eps), _p(out), B, chw, _stream())
    return out


def _dev_table(what, name, v, dtype, shape):
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != dtype or tuple(v.shape) != shape or not v.is_contiguous():
        raise AfdError(f"afdm: {what}: {name} must be a contiguous {dtype} device tensor of shape {shape}")


def tsampler_tick(t, rows, hist, count, lo, uniform_prob, w_base, prob, cdf, wtab, vwtab, warm):
    """The timestep sampler's update + refresh, one launch of one workgroup (afd.h: afd_tsampler_tick): folds the batch (t (B,)
    int64, rows (B,) fp64) into hist (T, H) fp64 / count (T,) int32 in batch order and rebuilds prob (T,) fp64, cdf (T - lo,)
    fp64, wtab (T,) fp32 = w_base * iw (w_base None: 1), vwtab (T,) fp32 = iw (may be None) and warm (1,) int32, all in place."""
    what = "tsampler_tick"
    if not isinstance(hist, torch.Tensor) or hist.dim() != 2:
        raise AfdError(f"afdm: {what}: hist must be a (T, H) tensor")
    T, H = hist.shape
    if isinstance(lo, bool) or not isinstance(lo, int) or not 0 <= lo < T:
        raise AfdError(f"afdm: {what}: lo must be an integer in [0, {T}) (got {lo!r})")
    if isinstance(uniform_prob, bool) or not isinstance(uniform_prob, (int, float)) or not 0.0 <= uniform_prob < 1.0:
        raise AfdError(f"afdm: {what}: uniform_prob must lie in [0, 1) (got {uniform_prob!r})")
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.numel() == 0:
        raise AfdError(f"afdm: {what}: rows must be a (B,) tensor with at least one element")
    B = rows.numel()
    _dev_table(what, "rows", rows, torch.float64, (B,))
    _dev_table(what, "t", t, torch.long, (B,))
    _dev_table(what, "hist", hist, torch.float64, (T, H))
    _dev_table(what, "count", count, torch.int32, (T,))
    _dev_table(what, "prob", prob, torch.float64, (T,))
    _dev_table(what, "cdf", cdf, torch.float64, (T - lo,))
    _dev_table(what, "wtab", wtab, torch.float32, (T,))
    _dev_table(what, "warm", warm, torch.int32, (1,))
    if w_base is not None:
        _dev_table(what, "w_base", w_base, torch.float32, (T,))
    if vwtab is not None:
        _dev_table(what, "vwtab", vwtab, torch.float32, (T,))
    lib().afd_tsampler_tick(_p(t), _p(rows), B, _p(hist), _p(count), T, H, lo, float(uniform_prob), _p(w_base), _p(prob), _p(cdf),
                            _p(wtab), _p(vwtab), _p(warm), _stream())


def tsampler_draw(cdf, u, lo, out=None):
    """t = lo + searchsorted(cdf, u, side="right"), clamped to the last timestep: cdf (n,) fp64 as `tsampler_tick` writes it, u (B,)
    fp64 in [0, 1), both on the device -> (B,) int64 device tensor; one launch (afd.h: afd_tsampler_draw)."""
    what = "tsampler_draw"
    if not isinstance(cdf, torch.Tensor) or cdf.dim() != 1 or cdf.numel() == 0 or not isinstance(u, torch.Tensor) or u.dim() != 1 \
            or u.numel() == 0:
        raise AfdError(f"afdm: {what}: cdf and u must be 1-d tensors with at least one element")
    if isinstance(lo, bool) or not isinstance(lo, int) or lo < 0:
        raise AfdError(f"afdm: {what}: lo must be an integer >= 0 (got {lo!r})")
    n, B = cdf.numel(), u.numel()
    _dev_table(what, "cdf", cdf, torch.float64, (n,))
    _dev_table(what, "u", u, torch.float64, (B,))
    if out is None:
        out = torch.empty(B, device=u.device, dtype=torch.long)
    _dev_table(what, "out", out, torch.long, (B,))
    lib().afd_tsampler_draw(_p(cdf), _p(u), lo, lo + n, _p(out), B, _stream())
    return out


def split_pred(out2, x_t, t, alpha_hat, kind, eps_out=None, want_v=False):
    """A learned-variance output (B, 2C, ...) -> the contiguous eps (B, C, ...): the prediction half, converted as `pred_to_eps`
    does for "v" / "x0" (a copy for "eps"), in one launch; want_v: also the contiguous coefficient half.  Returns eps or (eps, v)."""
    if not isinstance(x_t, torch.Tensor):
        raise AfdError("afdm: split_pred: x_t must be a tensor (it gives the shape of eps)")
    eps_out = torch.empty_like(x_t) if eps_out is None else eps_out
    out2, x_t = _c(out2), _c(x_t)
    code, B, chw = _lvar_args("split_pred", kind, out2, t, alpha_hat, None, x_t, eps_out)
    v_out = torch.empty_like(x_t) if want_v else None
    lib().afd_split_pred(_p(out2), _p(x_t), _p(t), _p(alpha_hat), code, _p(eps_out), _p(v_out), B, chw, _stream())
    return (eps_out, v_out) if want_v else eps_out


def _lvar_step(name, x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, step, cfg_scale, out, out2_x, guided):
    what = "guided learned-variance step" if guided else "learned-variance step"
    code, B, chw = _lvar_args(what, kind, out2, None, alpha_hat, lv_coef, x, noise, out, out2_x, rows2=2 if guided else 1)
    _lvar_tables(what, alpha, alpha_hat, beta)
    if isinstance(step, torch.Tensor):
        if not step.is_cuda or step.dtype != torch.long or step.numel() < 1:
            raise AfdError(f"afdm: {what}: t_dev must be an int64 device tensor (element 0 is read)")
        step = _p(step)
    else:
        step = int(step)
        if not 1 <= step < alpha_hat.numel():
            raise AfdError(f"afdm: {what} needs 1 <= i < {alpha_hat.numel()} (got {step})")
    args = (_p(x), _p(out2), _p(noise), _p(alpha), _p(alpha_hat), _p(beta), _p(lv_coef), code, step)
    if guided:
        getattr(lib(), name)(*args, float(cfg_scale), _p(out), _p(out2_x), B, chw, _stream())
    else:
        getattr(lib(), name)(*args, _p(out), B, chw, _stream())
    return out


def denoise_step_lvar(x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, out=None):
    """The ancestral step i -> i - 1 with the learned variance: mean as `denoise_step` from the output's prediction half (read
    as `kind`), plus exp(logvar / 2) * noise from its coefficient half; noise is ignored at i = 1 and may be None.  out may be x."""
    out = torch.empty_like(x) if out is None else out
    return _lvar_step("afd_denoise_step_lvar", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, 0.0, out, None, False)


def denoise_step_lvar_dev(x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, t_dev, out):
    """denoise_step_lvar with the step index t_dev[0] read on the device (graph-replayable)."""
    return _lvar_step("afd_denoise_step_lvar_dev", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, t_dev, 0.0, out, None, False)


def denoise_step_lvar_cfg(x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, cfg_scale, out=None, out_x2=None):
    """Classifier-free guided `denoise_step_lvar`: out2 is the forward over [conditional rows ; unconditional rows]; the two eps
    are combined as `denoise_step_cfg` combines them, the variance is the conditional row's.  out may be x; out_x2 (optional)
    receives the same values."""
    out = torch.empty_like(x) if out is None else out
    return _lvar_step("afd_denoise_step_lvar_cfg", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, cfg_scale, out, out_x2, True)


def denoise_step_lvar_cfg_dev(x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, t_dev, cfg_scale, out, out_x2=None):
    """denoise_step_lvar_cfg with the step index t_dev[0] read on the device (graph-replayable)."""
    return _lvar_step("afd_denoise_step_lvar_cfg_dev", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, t_dev, cfg_scale, out,
                      out_x2, True)


def vlb_terms_lvar(x0, img, x_t, eps, out2, t, lv_coef, alpha, alpha_hat, beta, kind, term=None, sq=None, check_range=True):
    """`vlb_terms` for a learned-variance output out2 (rows, 2C, ...): the bound's term of each row, in nats, with the
    per-element variance, and sum_j (eps_hat - eps)^2, both fp64 (rows,) device tensors (afd.h: afd_vlb_terms_lvar).
    lv_coef: the (T, 3) fp64 table of `Diffusion.lvar_coefficients` on the device.  Returns (term, sq)."""
    n_img, rows, per = _rows_args("learned-variance bound terms", x0, img, t, eps, check_range, alpha_hat.numel())
    code, _, _ = _lvar_args("learned-variance bound terms", kind, out2, None, alpha_hat, lv_coef, eps, x_t)
    _lvar_tables("learned-variance bound terms", alpha, alpha_hat, beta)
    term = torch.empty(rows, device=eps.device, dtype=torch.float64) if term is None else term
    sq = torch.empty(rows, device=eps.device, dtype=torch.float64) if sq is None else sq
    for v in (term, sq):
        if not v.is_cuda or v.dtype != torch.float64 or v.numel() != rows or not v.is_contiguous():
            raise AfdError(f"afdm: learned-variance bound terms: term and sq must be contiguous fp64 device tensors of {rows} values")
    lib().afd_vlb_terms_lvar(_p(x0), n_img, _p(img), _p(x_t), _p(eps), _p(out2), _p(t), _p(lv_coef), alpha_hat.numel(), _p(alpha),
                             _p(alpha_hat), _p(beta), code, _p(term), _p(sq), rows, per, _stream())
    return term, sq


def batch_gather(data, idx, flip=None, table=None, labels=None, x=None):
    """One batch out of a device-resident store, one launch (afd.h: afd_batch_gather_u8 / _f32): data (N, C, H, W) uint8 (with
    table (C, 256) fp32) or fp32, idx (B,) int64 (a view is fine), flip None or (B,) uint8, labels None or (N,) int64, all on the
    device -> (x (B, C, H, W) fp32, y (B,) int64 or None).  x: where to write (a contiguous fp32 tensor of that shape, or a view
    that is); a fresh tensor by default."""
    what = "batch_gather"
    if not isinstance(data, torch.Tensor) or not data.is_cuda or data.dim() != 4 or not data.is_contiguous() \
            or data.dtype not in (torch.uint8, torch.float32):
        raise AfdError(f"afdm: {what}: data must be a contiguous (N, C, H, W) uint8 or fp32 device tensor")
    N, C, H, W = data.shape
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.long or idx.dim() != 1 or idx.numel() == 0 \
            or not idx.is_contiguous():
        raise AfdError(f"afdm: {what}: idx must be a contiguous (B,) int64 device tensor with at least one element")
    B = idx.numel()
    u8 = data.dtype == torch.uint8
    if u8:
        _dev_table(what, "table", table, torch.float32, (C, 256))
    if flip is not None:
        _dev_table(what, "flip", flip, torch.uint8, (B,))
    y = None
    if labels is not None:
        _dev_table(what, "labels", labels, torch.long, (N,))
        y = torch.empty(B, device=data.device, dtype=torch.long)
    if x is None:
        x = torch.empty(B, C, H, W, device=data.device, dtype=torch.float32)
    _dev_table(what, "x", x, torch.float32, (B, C, H, W))
    if u8:
        lib().afd_batch_gather_u8(_p(data), N, C, H, W, _p(idx), _p(flip), _p(table), _p(x), _p(labels), _p(y), B, _stream())
    else:
        lib().afd_batch_gather_f32(_p(data), N, C, H, W, _p(idx), _p(flip), _p(x), _p(labels), _p(y), B, _stream())
    return x, y


NN_MAX_K = 16
NN_MAX_D_U8 = 32768
NN_WORKSPACE_LIMIT = 64 << 20


def nn_group(N, D, n, k, f32):
    """How many queries one afd_nn_search_* launch takes so that its workspace stays within NN_WORKSPACE_LIMIT: the workspace is
    linear in the number of queries, so this is the limit over the bytes one query needs (at least 1, at most n)."""
    per = int(lib().afd_nn_search_workspace_bytes(N, D, 1, k, int(f32)))
    if per <= 0:
        raise AfdError(f"afdm: nn_search: sizes out of range (N = {N}, D = {D}, n = {n}, k = {k})")
    return max(1, min(n, NN_WORKSPACE_LIMIT // per))


def nn_search(data, queries, k=1, exclude=None):
    """For each query row the k rows of `data` of smallest squared L2 distance, ascending, ties to the lower index (afd.h:
    afd_nn_search_u8 / _f32).  data (N, D) or (N, C, H, W), queries (n, D) or (n, C, H, W) of the same row size and dtype, uint8
    (exact int64 distances, D <= 32768) or fp32 (fp64 sums rounded once to fp32), contiguous, on the device; exclude None or (n,)
    int64 on the device: query q skips row exclude[q] (negative: nothing).  -> (dist (n, k) int64 / fp32, idx (n, k) int64); a
    slot with no candidate left holds idx -1 and dist -1 / +inf.  The queries go through in groups that share one workspace of
    at most NN_WORKSPACE_LIMIT bytes."""
    what = "nn_search"
    for name, v in (("data", data), ("queries", queries)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dim() not in (2, 4) or not v.is_contiguous() or v.numel() == 0 \
                or v.dtype not in (torch.uint8, torch.float32):
            raise AfdError(f"afdm: {what}: {name} must be a non-empty contiguous 2-D or 4-D uint8 or fp32 device tensor")
    N, n = data.shape[0], queries.shape[0]
    D = data.numel() // N
    if queries.dtype != data.dtype or queries.numel() // n != D:
        raise AfdError(f"afdm: {what}: queries must have data's dtype and row size ({data.dtype}, {D})")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= NN_MAX_K:
        raise AfdError(f"afdm: {what}: k must be an int in [1, {NN_MAX_K}] (got {k!r})")
    f32 = data.dtype == torch.float32
    if not f32 and D > NN_MAX_D_U8:
        raise AfdError(f"afdm: {what}: a uint8 row holds at most {NN_MAX_D_U8} elements (got D = {D})")
    if exclude is not None:
        _dev_table(what, "exclude", exclude, torch.long, (n,))
    idx = torch.empty(n, k, device=data.device, dtype=torch.long)
    dist = torch.empty(n, k, device=data.device, dtype=torch.float32 if f32 else torch.long)
    group = nn_group(N, D, n, k, f32)
    nbytes = int(lib().afd_nn_search_workspace_bytes(N, D, group, k, int(f32)))
    ws = torch.empty(nbytes // 8, device=data.device, dtype=torch.long)
    fn = lib().afd_nn_search_f32 if f32 else lib().afd_nn_search_u8
    qflat = queries.view(n, D)
    for a in range(0, n, group):
        b = min(n, a + group)
        fn(_p(data), N, D, _p(qflat[a:b]), b - a, None if exclude is None else _p(exclude[a:b]), k, _p(idx[a:b]), _p(dist[a:b]), _p(ws),
           nbytes, _stream())
    return dist, idx


def _workspace(what, nbytes, sizes, device):
    """-> (the fp64 workspace of an evaluation call, its bytes); nbytes: what the call's afd_*_workspace_bytes gave (0: sizes, the
    text that names them, are out of range)."""
    nbytes = int(nbytes)
    if nbytes <= 0:
        raise AfdError(f"afdm: {what}: sizes out of range ({sizes})")
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64), nbytes


SPECTRUM_MAX_SIDE = 64


def power_spectrum(images, table=None, win_h=None, win_w=None, remove_mean=True, bins=None, R=None, want_power=True):
    """Mean power spectrum of a set of images in fp64 (afd.h: afd_power_spectrum_u8 / _f32).  images (n, C, H, W) uint8 (read
    through table (C, 256) fp32) or fp32, contiguous, on the device, H and W at most 64; win_h (H,) / win_w (W,) fp64 or None (1);
    remove_mean: subtract each plane's own mean first; bins (H, W // 2 + 1) int32 with values in [-1, R) and R: the radial sums are
    wanted; want_power: the (C, H, W // 2 + 1) spectrum is wanted.  -> (power or None, radial (C, R) or None), fresh fp64 tensors:
    radial[c][r] is the SUM of m(v) power[c][u][v] over bins == r, for the caller to divide by its counts."""
    what = "power_spectrum"
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dim() != 4 or not images.is_contiguous() or images.numel() == 0 \
            or images.dtype not in (torch.uint8, torch.float32):
        raise AfdError(f"afdm: {what}: images must be a non-empty contiguous (n, C, H, W) uint8 or fp32 device tensor")
    n, C, H, W = images.shape
    if not (1 <= H <= SPECTRUM_MAX_SIDE and 1 <= W <= SPECTRUM_MAX_SIDE):
        raise AfdError(f"afdm: {what}: H and W must lie in [1, {SPECTRUM_MAX_SIDE}] (got {H}, {W})")
    u8 = images.dtype == torch.uint8
    if u8:
        _dev_table(what, "table", table, torch.float32, (C, 256))
    elif table is not None:
        raise AfdError(f"afdm: {what}: table goes with uint8 images only")
    if win_h is not None:
        _dev_table(what, "win_h", win_h, torch.float64, (H,))
    if win_w is not None:
        _dev_table(what, "win_w", win_w, torch.float64, (W,))
    Wh = W // 2 + 1
    if (bins is None) != (R is None):
        raise AfdError(f"afdm: {what}: bins and R go together")
    if bins is None and not want_power:
        raise AfdError(f"afdm: {what}: nothing to compute (want_power is False and no bins are given)")
    if bins is not None:
        _dev_table(what, "bins", bins, torch.int32, (H, Wh))
        if isinstance(R, bool) or not isinstance(R, int) or R < 1:
            raise AfdError(f"afdm: {what}: R must be an int >= 1 (got {R!r})")
    ws, nbytes = _workspace(what, lib().afd_spectrum_workspace_bytes(n, C, H, W), f"n = {n}, C = {C}, H = {H}, W = {W}", images.device)
    power = torch.empty(C, H, Wh, device=images.device, dtype=torch.float64) if want_power else None
    radial = torch.empty(C, R, device=images.device, dtype=torch.float64) if bins is not None else None
    tail = (n, C, H, W, _p(win_h), _p(win_w), int(bool(remove_mean)), _p(bins), R or 0, _p(power), _p(radial), _p(ws), nbytes, _stream())
    if u8:
        lib().afd_power_spectrum_u8(_p(images), _p(table), *tail)
    else:
        lib().afd_power_spectrum_f32(_p(images), *tail)
    return power, radial


def _feature_set(what, name, v, D=None):
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dim() != 2 or v.numel() == 0 or v.dtype != torch.float32:
        raise AfdError(f"afdm: {what}: {name} must be a non-empty (n, D) fp32 device tensor")
    if D is not None and v.shape[1] != D:
        raise AfdError(f"afdm: {what}: {name} must have the row size {D} (got {v.shape[1]})")
    return _c(v.detach())


MMD_MAX_DEGREE = 8
MMD_MAX_M = 1 << 16


def feature_moments(features, sum=None, outer=None):
    """Sum and sum of outer products of a feature set in fp64 (afd.h: afd_feature_moments_f32).  features (n, D) fp32 on the device
    (made contiguous if it is not); sum (D,) and outer (D, D): contiguous fp64 device tensors to ADD to, given together, or None
    for fresh ones.  -> (sum, outer): sum[c] = sum_r x[r][c], outer[i][j] = sum_r x[r][i] x[r][j], outer symmetric bit for bit."""
    what = "feature_moments"
    features = _feature_set(what, "features", features)
    n, D = features.shape
    if (sum is None) != (outer is None):
        raise AfdError(f"afdm: {what}: sum and outer go together")
    accumulate = sum is not None
    if accumulate:
        _dev_table(what, "sum", sum, torch.float64, (D,))
        _dev_table(what, "outer", outer, torch.float64, (D, D))
    else:
        sum = torch.empty(D, device=features.device, dtype=torch.float64)
        outer = torch.empty(D, D, device=features.device, dtype=torch.float64)
    ws, nbytes = _workspace(what, lib().afd_feature_moments_workspace_bytes(n, D), f"n = {n}, D = {D}", features.device)
    lib().afd_feature_moments_f32(_p(features), n, D, _p(sum), _p(outer), int(accumulate), _p(ws), nbytes, _stream())
    return sum, outer


def poly_mmd_sums(a, b, ia, ib, degree, gamma, coef0, check_range=True):
    """The three kernel sums of a polynomial-kernel MMD per subset, in fp64 (afd.h: afd_poly_mmd_sums_f32).  a (na, D) and b (nb, D)
    fp32 on the device (made contiguous if they are not), ia and ib (S, m) int64 row indices into a and b on the device, m >= 2;
    k(x, y) = (gamma x.y + coef0)^degree, degree an int in [1, 8].  -> sums (S, 3) fp64: the sum of k over i != j within a's rows,
    the same within b's, and over all (i, j) between them.  check_range: the indices are checked against na and nb first (one
    synchronising read); without it an index out of range makes its row NaN."""
    what = "poly_mmd_sums"
    a, b = _feature_set(what, "a", a), _feature_set(what, "b", b)
    if a.shape[1] != b.shape[1]:
        raise AfdError(f"afdm: {what}: a and b must have one row size (got {a.shape[1]} and {b.shape[1]})")
    (na, D), nb = a.shape, b.shape[0]
    for name, v in (("ia", ia), ("ib", ib)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.long or v.dim() != 2 or not v.is_contiguous():
            raise AfdError(f"afdm: {what}: {name} must be a contiguous (S, m) int64 device tensor")
    S, m = ia.shape
    if tuple(ib.shape) != (S, m) or S < 1 or not 2 <= m <= MMD_MAX_M:
        raise AfdError(f"afdm: {what}: ia and ib must have one shape (S, m) with S >= 1 and m in [2, {MMD_MAX_M}] (got {tuple(ia.shape)} "
                       f"and {tuple(ib.shape)})")
    if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or not 1 <= degree <= MMD_MAX_DEGREE:
        raise AfdError(f"afdm: {what}: degree must be an int in [1, {MMD_MAX_DEGREE}] (got {degree!r})")
    if check_range:
        lo, hi = torch.stack([ia.amin(), ib.amin()]).tolist(), torch.stack([ia.amax(), ib.amax()]).tolist()
        if lo[0] < 0 or hi[0] >= na or lo[1] < 0 or hi[1] >= nb:
            raise AfdError(f"afdm: {what}: an index lies outside its array (ia in [{lo[0]}, {hi[0]}] for {na} rows, ib in [{lo[1]}, {hi[1]}] "
                           f"for {nb} rows)")
    ws, nbytes = _workspace(what, lib().afd_poly_mmd_workspace_bytes(S, m, D), f"S = {S}, m = {m}, D = {D}", a.device)
    sums = torch.empty(S, 3, device=a.device, dtype=torch.float64)
    lib().afd_poly_mmd_sums_f32(_p(a), na, _p(b), nb, D, _p(ia), _p(ib), S, m, int(degree), float(gamma), float(coef0), _p(sums), _p(ws),
                                nbytes, _stream())
    return sums


MANIFOLD_MAX_K = 16


def kth_neighbour(features, k):
    """Per row of a feature set the k-th smallest squared L2 distance to another row, in fp64 (afd.h: afd_kth_neighbour_f32).
    features (n, D) fp32 on the device (made contiguous if it is not), k an int in [1, 16].  -> radius2 (n,) fp64; rows are left
    out by index, a NaN distance is no candidate, and a row with fewer than k candidates gets +inf."""
    what = "kth_neighbour"
    features = _feature_set(what, "features", features)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MANIFOLD_MAX_K:
        raise AfdError(f"afdm: {what}: k must be an int in [1, {MANIFOLD_MAX_K}] (got {k!r})")
    n, D = features.shape
    ws, nbytes = _workspace(what, lib().afd_kth_neighbour_workspace_bytes(n, D, int(k)), f"n = {n}, D = {D}", features.device)
    radius2 = torch.empty(n, device=features.device, dtype=torch.float64)
    lib().afd_kth_neighbour_f32(_p(features), n, D, int(k), _p(radius2), _p(ws), nbytes, _stream())
    return radius2


def ball_membership(queries, store, radius2, exclude=None, want_count=True, want_nearest=True):
    """For each query row the number of store rows whose ball holds it and its nearest store row, in fp64 (afd.h:
    afd_ball_membership_f32).  queries (nq, D) and store (nr, D) fp32 on the device (made contiguous if they are not), radius2
    (nr,) fp64: the squared radius of each store row's ball; exclude None or (nq,) int64 on the device: query q skips store row
    exclude[q] (negative: nothing).  -> (count (nq,) int32, nearest (nq,) int64, nearest_d2 (nq,) fp64), None for what was not
    asked for: count[q] is the number of j with d2(q, j) <= radius2[j], nearest[q] the j of smallest d2 (ties to the lower j; -1
    and +inf with no candidate)."""
    what = "ball_membership"
    queries = _feature_set(what, "queries", queries)
    store = _feature_set(what, "store", store, queries.shape[1])
    (nq, D), nr = queries.shape, store.shape[0]
    _dev_table(what, "radius2", radius2, torch.float64, (nr,))
    if exclude is not None:
        _dev_table(what, "exclude", exclude, torch.long, (nq,))
    if not want_count and not want_nearest:
        raise AfdError(f"afdm: {what}: nothing to compute (want_count and want_nearest are both False)")
    dev = queries.device
    ws, nbytes = _workspace(what, lib().afd_ball_membership_workspace_bytes(nq, nr, D), f"nq = {nq}, nr = {nr}, D = {D}", dev)
    count = torch.empty(nq, device=dev, dtype=torch.int32) if want_count else None
    nearest = torch.empty(nq, device=dev, dtype=torch.long) if want_nearest else None
    nearest_d2 = torch.empty(nq, device=dev, dtype=torch.float64) if want_nearest else None
    lib().afd_ball_membership_f32(_p(queries), nq, _p(store), nr, D, _p(radius2), _p(exclude), _p(count), _p(nearest), _p(nearest_d2),
                                  _p(ws), nbytes, _stream())
    return count, nearest, nearest_d2


QUALITY_MAX_SIDE = 64
QUALITY_MAX_WINDOW = 15


def pair_quality(a, b, win, c1, c2, region=None, want_map=False):
    """PSNR and SSIM sums of image pairs in fp64, one launch (afd.h: afd_pair_quality_u8 / _f32).  a and b (n, C, H, W) uint8 or
    fp32 on one device, of one shape and dtype (made contiguous if they are not), H and W at most 64; win: the K window weights,
    a 1-D fp64 cpu tensor or a sequence of numbers, K odd, at most 15 and at most min(H, W); c1, c2: SSIM's two constants; region
    None or a contiguous (1 | n, H, W) uint8 device tensor, non-zero = counted.  -> (out (n, C, 5) fp64: the sum of squared and
    of absolute differences over the region, its pixels, the sum of SSIM over the windows centred in it, those windows; ssim_map
    (n, C, H - K + 1, W - K + 1) fp64 with want_map, else None)."""
    what = "pair_quality"
    for name, v in (("a", a), ("b", b)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dim() != 4 or v.numel() == 0 or v.dtype not in (torch.uint8, torch.float32):
            raise AfdError(f"afdm: {what}: {name} must be a non-empty (n, C, H, W) uint8 or fp32 device tensor")
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        raise AfdError(f"afdm: {what}: a and b must have one shape, dtype and device (got {tuple(a.shape)} {a.dtype} {a.device} and "
                       f"{tuple(b.shape)} {b.dtype} {b.device})")
    a, b = _c(a.detach()), _c(b.detach())
    n, C, H, W = a.shape
    if not (1 <= H <= QUALITY_MAX_SIDE and 1 <= W <= QUALITY_MAX_SIDE):
        raise AfdError(f"afdm: {what}: H and W must lie in [1, {QUALITY_MAX_SIDE}] (got {H}, {W})")
    w = np.ascontiguousarray(win.detach().cpu().numpy() if isinstance(win, torch.Tensor) else np.asarray(win), dtype=np.float64)
    K = int(w.shape[0]) if w.ndim == 1 else 0
    if K < 1 or K % 2 == 0 or K > QUALITY_MAX_WINDOW or K > min(H, W):
        raise AfdError(f"afdm: {what}: win must hold K weights, K odd, at most {QUALITY_MAX_WINDOW} and at most min(H, W) = {min(H, W)} "
                       f"(got shape {tuple(w.shape)})")
    rows = 1
    if region is not None:
        if not isinstance(region, torch.Tensor) or region.device != a.device or region.dtype != torch.uint8 or region.dim() != 3 \
                or tuple(region.shape[1:]) != (H, W) or region.shape[0] not in (1, n) or not region.is_contiguous():
            raise AfdError(f"afdm: {what}: region must be None or a contiguous uint8 tensor of shape (1 | {n}, {H}, {W}) on the images' device")
        rows = int(region.shape[0])
    out = torch.empty(n, C, 5, device=a.device, dtype=torch.float64)
    ssim_map = torch.empty(n, C, H - K + 1, W - K + 1, device=a.device, dtype=torch.float64) if want_map else None
    fn = lib().afd_pair_quality_u8 if a.dtype == torch.uint8 else lib().afd_pair_quality_f32
    fn(_p(a), _p(b), n * C, C, H, W, w.ctypes.data, K, float(c1), float(c2), _p(region), rows, _p(out), _p(ssim_map), _stream())
    return out, ssim_map


# ---- diffusion posterior sampling: the linear operator A x = m . S_s(k * x) and the step's two launches (afd.h) ----
LINOP_MAX_SIDE = 64
LINOP_MAX_KERNEL = 15
LINOP_STRIDES = (1, 2, 4)


def _linop_args(what, kernel, stride, mask, C, h, w, device):
    """-> (the host taps, K, the mask's channels) after checking an operator against a (.., C, h, w) measurement plane.  kernel: a
    (K, K) float32 host array (numpy, or a cpu tensor), K odd and at most 15; stride 1, 2 or 4; mask None or a contiguous
    (1 | C, h, w) fp32 tensor on `device`."""
    taps = np.ascontiguousarray(kernel.detach().cpu().numpy() if isinstance(kernel, torch.Tensor) else np.asarray(kernel), dtype=np.float32)
    K = int(taps.shape[0]) if taps.ndim == 2 and taps.shape[0] == taps.shape[1] else 0
    if K < 1 or K % 2 == 0 or K > LINOP_MAX_KERNEL:
        raise AfdError(f"afdm: {what}: kernel must be (K, K) with K odd and at most {LINOP_MAX_KERNEL} (got shape {tuple(taps.shape)})")
    if stride not in LINOP_STRIDES:
        raise AfdError(f"afdm: {what}: stride must be 1, 2 or 4 (got {stride!r})")
    if not (1 <= h * stride <= LINOP_MAX_SIDE and 1 <= w * stride <= LINOP_MAX_SIDE):
        raise AfdError(f"afdm: {what}: H and W must lie in [1, {LINOP_MAX_SIDE}] (got {h * stride}, {w * stride})")
    mc = 0
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != device or mask.dtype != torch.float32 or mask.dim() != 3 \
                or mask.shape[0] not in (1, C) or tuple(mask.shape[1:]) != (h, w) or not mask.is_contiguous():
            raise AfdError(f"afdm: {what}: mask must be None or a contiguous fp32 tensor of shape (1 | {C}, {h}, {w}) on the images' device")
        mc = int(mask.shape[0])
    return taps, K, mc


def _linop_images(what, name, v):
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() != 4 or v.numel() == 0:
        raise AfdError(f"afdm: {what}: {name} must be a non-empty (n, C, H, W) fp32 device tensor")
    return _c(v.detach())


def linop_apply(x, kernel, stride=1, mask=None):
    """y (n, C, H / s, W / s) = m . S_s(k * x), one launch (afd.h: afd_linop_apply)."""
    what = "linop_apply"
    x = _linop_images(what, "x", x)
    B, C, H, W = x.shape
    if H % stride or W % stride:
        raise AfdError(f"afdm: {what}: H and W must be multiples of the stride {stride} (got {H}, {W})")
    h, w = H // stride, W // stride
    taps, K, mc = _linop_args(what, kernel, stride, mask, C, h, w, x.device)
    y = torch.empty(B, C, h, w, device=x.device, dtype=torch.float32)
    lib().afd_linop_apply(_p(x), _p(y), taps.ctypes.data, K, stride, _p(mask), mc, B, C, H, W, _stream())
    return y


def linop_adjoint(r, kernel, stride=1, mask=None):
    """g (n, C, h s, w s) = A^T r, the transposed strided correlation of m . r, one launch (afd.h: afd_linop_adjoint)."""
    what = "linop_adjoint"
    r = _linop_images(what, "r", r)
    B, C, h, w = r.shape
    taps, K, mc = _linop_args(what, kernel, stride, mask, C, h, w, r.device)
    g = torch.empty(B, C, h * stride, w * stride, device=r.device, dtype=torch.float32)
    lib().afd_linop_adjoint(_p(r), _p(g), taps.ctypes.data, K, stride, _p(mask), mc, B, C, h * stride, w * stride, _stream())
    return g


def dps_residual(x_t, out, t, alpha_hat, kind, y, kernel, stride=1, mask=None, g=None, sums=None):
    """The step side of diffusion posterior sampling in one launch (afd.h: afd_dps_residual): x0_hat = a_t x_t + b_t out with
    (a_t, b_t) of `kind` at alpha_hat[t[row]], r = A x0_hat - y, sums[row, c] = the plane's sum of r^2 in fp64, g = A^T r.
    x_t, out (n, C, H, W) and y (n, C, H / s, W / s) fp32 on one device, contiguous; t (n,) int64 on the device.
    -> (g (n, C, H, W) fp32, sums (n, C) fp64)."""
    what = "dps_residual"
    code, B, _ = _objective_args(what, kind, t, alpha_hat, x_t, out)
    if x_t.dim() != 4:
        raise AfdError(f"afdm: {what}: x_t and out must be (n, C, H, W)")
    _, C, H, W = x_t.shape
    if H % stride or W % stride:
        raise AfdError(f"afdm: {what}: H and W must be multiples of the stride {stride} (got {H}, {W})")
    h, w = H // stride, W // stride
    taps, K, mc = _linop_args(what, kernel, stride, mask, C, h, w, x_t.device)
    _chk(y)
    if tuple(y.shape) != (B, C, h, w) or not y.is_contiguous() or y.device != x_t.device:
        raise AfdError(f"afdm: {what}: y must be a contiguous ({B}, {C}, {h}, {w}) tensor on the images' device (got {tuple(y.shape)})")
    g = torch.empty_like(x_t) if g is None else g
    sums = torch.empty(B, C, device=x_t.device, dtype=torch.float64) if sums is None else sums
    if g.dtype != torch.float32 or tuple(g.shape) != tuple(x_t.shape) or not g.is_contiguous() or g.device != x_t.device \
            or sums.dtype != torch.float64 or tuple(sums.shape) != (B, C) or not sums.is_contiguous() or sums.device != x_t.device:
        raise AfdError(f"afdm: {what}: g must be a contiguous fp32 tensor of x_t's shape and sums a contiguous ({B}, {C}) fp64 one")
    lib().afd_dps_residual(_p(x_t), _p(out), _p(t), _p(alpha_hat), code, _p(y), taps.ctypes.data, K, stride, _p(mask), mc, _p(g),
                           _p(sums), B, C, H, W, _stream())
    return g, sums


def dps_correct(x, g, v, sums, t, alpha_hat, kind, zeta):
    """x[row] -= c_row (a_t g + b_t v) in place, c_row = zeta / sqrt(sum_c sums[row, c]) decided on the device (0 where that sum
    is 0: the row is not touched), one launch (afd.h: afd_dps_correct).  x, g, v: contiguous (n, C, ...) fp32; sums (n, C) fp64;
    t (n,) int64 on the device.  -> x."""
    what = "dps_correct"
    code, B, chw = _objective_args(what, kind, t, alpha_hat, x, g, v)
    if x.dim() < 2 or not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.device != x.device \
            or tuple(sums.shape) != (B, x.shape[1]) or not sums.is_contiguous():
        raise AfdError(f"afdm: {what}: sums must be a contiguous (n, C) fp64 tensor on x's device")
    zeta = float(zeta)
    if not (zeta >= 0 and np.isfinite(zeta)):
        raise AfdError(f"afdm: {what}: zeta must be finite and >= 0 (got {zeta})")
    C = int(x.shape[1])
    lib().afd_dps_correct(_p(x), _p(g), _p(v), _p(sums), _p(t), _p(alpha_hat), code, zeta, B, C, chw // C, _stream())
    return x


# ---- likelihoods from the probability-flow ODE: the trace reduction and Heun's corrector (afd.h) ----
def ode_trace_rows(v, w, cvv, cvw, acc):
    """acc[r] += cvv * sum_j v[r, j]^2 + cvw * sum_j v[r, j] w[r, j] in fp64, one launch, the same bits from call to call (afd.h:
    afd_ode_trace_rows gives the order).  v, w: contiguous fp32 (rows, ...) device tensors of one shape, w None when cvw == 0;
    acc: a contiguous fp64 (rows,) tensor on the same device, updated in place.  -> acc."""
    what = "ode_trace_rows"
    _chk(v, w)
    if not isinstance(v, torch.Tensor) or v.dim() < 1 or v.numel() == 0 or not v.is_contiguous():
        raise AfdError(f"afdm: {what}: v must be a non-empty contiguous (rows, ...) tensor")
    if w is not None and (tuple(w.shape) != tuple(v.shape) or not w.is_contiguous() or w.device != v.device):
        raise AfdError(f"afdm: {what}: w must be None or a contiguous tensor of v's shape {tuple(v.shape)} on v's device")
    rows = int(v.shape[0])
    if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float64 or acc.device != v.device or tuple(acc.shape) != (rows,) \
            or not acc.is_contiguous():
        raise AfdError(f"afdm: {what}: acc must be a contiguous ({rows},) fp64 tensor on v's device")
    cvv, cvw = float(cvv), float(cvw)
    if not (np.isfinite(cvv) and np.isfinite(cvw)):
        raise AfdError(f"afdm: {what}: cvv and cvw must be finite (got {cvv}, {cvw})")
    if w is None and cvw != 0.0:
        raise AfdError(f"afdm: {what}: w may be None only when cvw == 0 (got {cvw})")
    lib().afd_ode_trace_rows(_p(v), _p(w), cvv, cvw, _p(acc), rows, v.numel() // rows, _stream())
    return acc


def ode_heun_step(x, eps_s, eps_u, alpha_hat, s, u, out=None):
    """The corrector of Heun's rule for the move s -> u, 1 <= s < u, of the probability-flow ODE (afd.h: afd_ode_heun_step gives the
    exact expression): x_u = sqrt(a_u) (x / sqrt(a_s) + h (eps_s + eps_u) / 2).  `out` defaults to a new tensor and may be x (in
    place); it must not overlap eps_s or eps_u."""
    what = "ODE Heun step"
    out = torch.empty_like(x) if out is None else out
    n = _step_args(what, x, eps_s, eps_u, alpha_hat, out)
    s, u = int(s), int(u)
    if not 1 <= s < u < alpha_hat.numel():
        raise AfdError(f"afdm: {what} needs 1 <= s < u < {alpha_hat.numel()} (got s = {s}, u = {u})")
    if len({t.device for t in (x, eps_s, eps_u, alpha_hat, out)}) != 1:
        raise AfdError(f"afdm: {what}: every tensor must be on one device")
    lib().afd_ode_heun_step(_p(x), _p(eps_s), _p(eps_u), _p(alpha_hat), s, u, _p(out), n, _stream())
    return out
