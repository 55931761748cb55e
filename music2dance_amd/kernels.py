"""Tensor-level wrappers over the C-ABI (include/m2d.h): raw kernels, no autograd.

PyTorch is plumbing here: it owns device memory (outputs and scratch come from the
caching allocator, so the calls are hipGraph-capture safe) and the current HIP stream.
Every method enqueues hand-written gfx950 kernels and nothing else; inputs must be
contiguous fp32 tensors on a HIP device, otherwise the call raises (no fallback).

A method checks its arguments, allocates outputs (and `_workspace`), and hands pointers and sizes to `_launch` under
the entry point's name; the weight images the GEMMs read are kept by `HipKernels._image`.
"""
import contextlib
import ctypes
import math
import weakref

import numpy as np
import torch

from . import _lib, levers

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _chk(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.M2dError("m2d kernels need HIP device tensors (got %s); there is no CPU path" % t.device)
        if t.dtype != torch.float32:
            raise _lib.M2dError("m2d kernels are fp32 only (got %s)" % t.dtype)
        if not t.is_contiguous():
            raise _lib.M2dError("m2d kernels need contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.M2dError("tensors on different devices")
    return dev


def _chk_track(track, dev, T, hop, window):
    """(B, >= (T-1)*hop + window) fp32 rows on `dev`, unit stride inside a row; -> (B, row stride)."""
    if not track.is_cuda or track.device != dev or track.dtype != torch.float32 or track.dim() != 2:
        raise _lib.M2dError("window view: the track must be a 2-D fp32 tensor on %s" % dev)
    if track.stride(1) != 1 or track.size(1) < (T - 1) * hop + window:
        raise _lib.M2dError("window view: rows must be dense and hold (T-1)*hop + window samples")
    B = track.size(0)
    S = track.stride(0) if B > 1 else track.size(1)
    if S < (T - 1) * hop + window:
        raise _lib.M2dError("window view: overlapping tracks")
    return B, S


def _chk_labels(labels, dev, n, what):
    """class indices handed to a kernel: a contiguous int64 tensor of n entries on the kernels' device"""
    if not labels.is_cuda or labels.device != dev or labels.dtype != torch.int64 or not labels.is_contiguous():
        raise _lib.M2dError("%s: labels must be a contiguous int64 tensor on %s" % (what, dev))
    if labels.numel() != n:
        raise _lib.M2dError("%s: %d labels for %d rows" % (what, labels.numel(), n))


def _bcl(x):
    """(B, C, L) of an activation shaped (B, C, L) or (B, C)"""
    return x.shape[0], x.shape[1], x.shape[2] if x.dim() == 3 else 1


_STREAM_SCRATCH = {}
_FUSED_SPLITK = levers.on("M2D_FUSED_SPLITK")
_TICKET_WORDS = 16384   # 4 bytes per output tile of a split-K launch (include/m2d.h: 64 KB covers every shape)
_BN_MAX_C = 4096        # widest channel / feature count a reducing call may have (the reference's widest: 1024)


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _register_tickets(raw, t):
    """Tell the library which zero-kept ticket scratch raw stream `raw` has (None: none, two-launch split-K)."""
    rc = _lib.lib().m2d_stream_scratch_set(raw, _ptr(t), 0 if t is None else t.numel() * 4)
    _lib.check(rc, "m2d_stream_scratch_set")


def _stream(dev):
    # raw hipStream_t of the current stream without building a torch.cuda.Stream object
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    s = torch._C._cuda_getCurrentRawStream(idx)
    if _PRIVATE is not None:
        _PRIVATE.adopt((idx, s))
    elif _FUSED_SPLITK and (idx, s) not in _STREAM_SCRATCH and not _capturing():
        # first launch on this stream: its zero-kept ticket scratch (include/m2d.h: m2d_stream_scratch_set) - split-K
        # launches then finish without the second (reduction) launch. Never created inside a capture (it would live in
        # that graph's private pool behind a captured memset): a capture without `private_scratch` keeps the
        # two-launch split-K, which needs no state.
        t = torch.zeros(_TICKET_WORDS, dtype=torch.int32, device=dev)
        _STREAM_SCRATCH[(idx, s)] = t
        _register_tickets(s, t)
    return s


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(dev):
    """Device guard for a launch: a no-op when `dev` is already current (the common case)."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(dev)


def _launch(name, dev, *args):
    """THE launch: entry point `name` of the library with `args` and, behind them, the raw current stream of `dev`
    (every launching entry point takes its stream last), under the device guard; a non-zero return raises, naming
    `name`. Callers pass device pointers (`_ptr`) and plain numbers. The stream is looked up here, i.e. after the
    caller has allocated its outputs and workspace: the first look-up on a stream creates its ticket scratch, and
    `private_scratch.adopt` runs from it."""
    with _on(dev):
        rc = getattr(_lib.lib(), name)(*args, _stream(dev))
    if rc != 0:  # (tested here: this is on the host path of every launch, and the check is one more call)
        _lib.check(rc, name)


_WS_BYTES = {}


def _ws_bytes(name, *args):
    """Workspace size queries are pure functions of the shape: ask the library once per shape."""
    if levers.is_set("M2D_PLAN"):  # tuning builds: the plan (and its workspace) follows the environment
        return getattr(_lib.lib(), name)(*args)
    key = (name,) + args
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = getattr(_lib.lib(), name)(*args)
    return n


def _workspace(dev, query, *shape):
    """The workspace the library's size query `query` asks for at `shape` -> (tensor or None, its size in bytes)."""
    nbytes = _ws_bytes(query, *shape)
    if nbytes <= 0:
        return None, 0
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    return ws, ws.numel() * 4


_BN_SCRATCH = {}


def _bn_scratch(dev, C):
    """The zero-kept accumulator scratch of the reducing BatchNorm / channel-sum calls (include/m2d.h:
    m2d_bn_scratch_bytes): one per (device, stream), of FIXED size (captured graphs keep its address: it is never
    re-allocated), zeroed once here and left zeroed by every call. None inside a capture that has not been given one
    (`private_scratch`): the call then takes the stateless three-launch form."""
    if C > _BN_MAX_C:
        return None  # wider than the fixed scratch (a GRU with hidden size > _BN_MAX_C / 3): the stateless three-launch form
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), _stream(dev))
    t = _BN_SCRATCH.get(key)
    if t is None:
        if _capturing() or _PRIVATE is not None:
            return None
        t = _BN_SCRATCH[key] = torch.zeros((2 * _BN_MAX_C + 8,), dtype=torch.float64, device=dev)
    return t


_PRIVATE = None   # the private_scratch scope being captured under, if any


class private_scratch:
    """Scope for CAPTURING a graph: launches made inside it - on the capture stream and on every stream forked from it -
    take their zero-kept scratch (split-K tickets, BatchNorm / channel-sum accumulators) from buffers owned by this
    object instead of the streams' own. A captured launch bakes the scratch ADDRESS in; two graphs captured on one
    stream (torch captures every graph on the same class-level stream by default) would otherwise share it, and
    replaying them concurrently - the phase-2 generator-forward graph runs on the generator stream under the critic
    graph of the previous body - has both sets of kernels counting arrivals in the same words. Keep the object alive
    as long as the graph. Everything is allocated in __init__, i.e. outside the capture: `nstreams` sets (the capture
    stream + the side streams the modules fork); a further stream gets none and its calls take the stateless forms."""

    def __init__(self, dev, nstreams=4):
        self.dev = dev
        self.free = [(torch.zeros(_TICKET_WORDS, dtype=torch.int32, device=dev) if _FUSED_SPLITK else None,
                      torch.zeros((2 * _BN_MAX_C + 8,), dtype=torch.float64, device=dev)) for _ in range(nstreams)]
        self.by_stream = {}
        self.saved = {}

    @staticmethod
    def _install(key, tickets, sums):
        """Make (tickets, sums) the scratch of stream `key` in the module's tables and in the library (None: none)."""
        for table, t in ((_STREAM_SCRATCH, tickets), (_BN_SCRATCH, sums)):
            if t is None:
                table.pop(key, None)
            else:
                table[key] = t
        if _FUSED_SPLITK:
            _register_tickets(key[1], tickets)

    def adopt(self, key):
        """First launch on stream `key` = (device index, raw stream) inside the scope: give it one of the sets."""
        if key in self.by_stream:
            return
        pair = self.free.pop() if self.free else (None, None)
        self.by_stream[key] = pair
        self.saved[key] = (_STREAM_SCRATCH.get(key), _BN_SCRATCH.get(key))
        self._install(key, *pair)

    def __enter__(self):
        global _PRIVATE
        self._outer, _PRIVATE = _PRIVATE, self
        return self

    def __exit__(self, *exc):
        global _PRIVATE
        _PRIVATE = self._outer
        for key, old in self.saved.items():
            self._install(key, *old)
        self.saved = {}
        return False


def set_plan_model(model):
    """Which cost model ranks the GEMM engine's launch plans (include/m2d.h: m2d_plan_model_set): 4 where the streams of
    a loop body overlap (two-branch phase-3 critic), 5 where launches run one after the other (phase 2, pose-only critic).
    PROCESS-WIDE, and plans decide summation orders: a program sets it once, before its first launch (bench.py does for
    its c2 / c5 presets, the phase-2 train script does) - the engines do not touch it (round 5: an engine that switched it
    in its constructor changed the arithmetic of whatever ran next in the process). An explicit M2D_PLAN_MODEL in the
    environment wins. Cached workspace sizes follow the plans: dropped."""
    if levers.is_set("M2D_PLAN_MODEL") or not hasattr(_lib.lib(), "m2d_plan_model_set"):
        return
    if _lib.lib().m2d_plan_model_get() != int(model):
        _lib.check(_lib.lib().m2d_plan_model_set(int(model)), "m2d_plan_model_set")
        _WS_BYTES.clear()


def reset_scratch():
    """Re-zero every zero-kept scratch buffer of the streams' own (not the graphs' private ones). A launch that was
    aborted mid-way (device fault, a persistent kernel's timeout) can leave arrival counters or accumulators non-zero,
    which would silently corrupt every later reducing / split-K call on that stream: callers that detect such an
    error call this AFTER synchronising the device."""
    for t in list(_STREAM_SCRATCH.values()) + list(_BN_SCRATCH.values()):
        t.zero_()


def conv_out_len(L, ks, stride, pad):
    return (L + 2 * pad - ks) // stride + 1


def _gemm_shape(mode, a, b):
    """mode 0: a(M,K) b(N,K)^T; 1: a(M,K) b(K,N); 2: a(K,M)^T b(K,N) -> (M, N, K)"""
    if mode == 0:
        M, K = a.shape
        N, K2 = b.shape
    elif mode == 1:
        M, K = a.shape
        K2, N = b.shape
    else:
        K, M = a.shape
        K2, N = b.shape
    assert K == K2, "gemm: inner dimension mismatch"
    return M, N, K


class HipKernels:
    """The product implementation: every method is one or a few HIP kernel launches."""

    name = "hip"

    # ---------------------------------------------------------------- weight images
    def __init__(self):
        # images of live weight tensors (packed conv weights, include/m2d.h: m2d_conv1d_pack_weights; W^T of the GRUs):
        # (id(w), kind) -> (weakref to w, w._version, raw stream or None, image). Only kept inside a weight_cache()
        # scope, i.e. while the caller guarantees the weights are constant
        self._packed = {}
        self._cache_depth = 0
        self.pack_launches = 0
        self._adam_kept = set()   # keys of the images adam_multi has rewritten since the last invalidate_packed()

    @contextlib.contextmanager
    def weight_cache(self, keep=False):
        """Scope in which conv weights are promised constant except where invalidate_packed() is
        called (right after an optimizer step): the packed images the forward / backward-data
        GEMMs read are built once per weight tensor instead of once per call. Outside a scope every
        call packs afresh - a tensor's version counter is no proof of constancy (fused optimizers
        update parameters without moving it).
        keep: leave the images in place when the scope closes, for the next scope of the same owner (the
        training engine: the generator's weights do not change during the critic iterations of a cycle).
        The owner then vouches that between its scopes parameters only change through operations that move
        the version counter (copy_, load_state_dict, in-place math) or are announced with invalidate_packed()."""
        self._cache_depth += 1
        try:
            yield self
        finally:
            self._cache_depth -= 1
            if self._cache_depth == 0 and not keep:
                self._packed.clear()

    def invalidate_packed(self, tensors=None):
        """Drop the images of `tensors` (the parameters an optimizer step just changed), or all of them."""
        if tensors is None:
            self._packed.clear()
        else:
            ids = {id(w) for w in tensors}
            # the (w_fwd, w_bwd) images adam_multi has just rewritten stay
            for key in [k for k in self._packed if k[0] in ids and k not in self._adam_kept]:
                del self._packed[key]
            self._adam_kept = set()

    def _image(self, w, kind, build):
        """The image `build()` makes of weight tensor `w` on the current stream, one per (tensor, kind). Inside a
        weight_cache() scope it is kept and handed out again while it is of this very tensor (not another one at
        the same address), the tensor's version counter has not moved, and the asking stream is the one it was
        written on (or it is marked valid on every stream: None, see adam_multi); it goes when the tensor dies."""
        stream = _stream(w.device)
        key = (id(w), kind)
        if self._cache_depth > 0:
            ent = self._packed.get(key)
            if ent is not None and ent[0]() is w and ent[1] == w._version and (ent[2] is None or ent[2] == stream):
                return ent[3]
        image = build()
        if self._cache_depth > 0:
            packed = self._packed

            def _drop(_ref, key=key):
                packed.pop(key, None)

            packed[key] = (weakref.ref(w, _drop), w._version, stream, image)
        return image

    def packed_weights(self, w):
        """(w_fwd (Cin, ks, Cout), w_bwd (Cout, ks, Cin)): the K-major images of a conv weight the forward / backward-data
        GEMMs read (written on the current stream)."""
        def build():
            Cout, Cin, ks = w.shape
            wf = torch.empty((Cin, ks, Cout), dtype=torch.float32, device=w.device)
            wb = torch.empty((Cout, ks, Cin), dtype=torch.float32, device=w.device)
            _launch("m2d_conv1d_pack_weights", w.device, _ptr(w), _ptr(wf), _ptr(wb), Cout, Cin, ks)
            self.pack_launches += 1
            return wf, wb

        return self._image(w, "conv", build)

    def packed_k4(self, w, pad):
        """Wk4[(ci, tap group)][Cout][4]: the image the tap-vectorised stride-4 forward reads (cached like the others)."""
        def build():
            Cout, Cin, ks = w.shape
            elems = _lib.lib().m2d_conv1d_k4_packed_elems(Cout, Cin, ks, pad)
            out = torch.empty((elems,), dtype=torch.float32, device=w.device)
            _launch("m2d_conv1d_pack_weights_k4", w.device, _ptr(w), _ptr(out), Cout, Cin, ks, pad)
            self.pack_launches += 1
            return out

        return self._image(w, ("k4", pad), build)

    def transposed(self, w):
        """w.t().contiguous() of a 2-D weight (the GRU kernels read W^T), kept like the packed conv images: built
        once per weight tensor inside a weight_cache() scope, dropped by invalidate_packed()."""
        return self._image(w, "T", lambda: w.t().contiguous())

    # ---------------------------------------------------------------- conv1d
    _SEPARATE_BIAS = levers.on("M2D_SEPARATE_BIAS")
    _K4 = levers.on("M2D_K4")  # A/B lever: 0 = stride-4 forwards through the generic engine
    _K4_OK = {}

    def _k4(self, Cin, L, Cout, ks, stride, pad):
        if not self._K4 or stride != 4:
            return False
        key = (Cin, L, Cout, ks, stride, pad)
        ok = self._K4_OK.get(key)
        if ok is None:
            ok = self._K4_OK[key] = bool(_lib.lib().m2d_conv1d_k4_applicable(Cin, L, Cout, ks, stride, pad))
        return ok

    @staticmethod
    def _thin(Cin, Cout, ks, stride):
        """the library's thin_ok (csrc/conv1d_thin.hip): the single-channel k25 / s4 kernels take 32 output channels only"""
        return Cin == 1 and Cout == 32 and ks == 25 and stride == 4

    def conv1d_fwd(self, x, w, bias, stride, pad, act=0, slope=0.0, residual=None, out_mask=None,
                   out_mask_slope=0.0, with_stats=False, out=None, sum_out=None):
        """y = out_mask * act(conv(x) + bias) + residual  (mask BEFORE the residual)
        -> y, or (y, sums) with `with_stats`: sums (2*Cout,) float64 = per-channel sum / sum of squares of y
        from the conv's own epilogue (what a following BatchNorm needs: bn_fwd_sums).
        out: write y there (may alias out_mask: in-place masking). sum_out (needs residual): second output
        sum_out = y + residual while y itself stays without the residual; -> (y, sum_out)."""
        dev = _chk(x, w, bias, residual, out_mask, out, sum_out)
        B, Cin, L = x.shape
        Cout, Cin2, ks = w.shape
        assert Cin == Cin2, "conv1d: channel mismatch"
        Lout = conv_out_len(L, ks, stride, pad)
        y = torch.empty((B, Cout, Lout), dtype=torch.float32, device=dev) if out is None else out
        assert tuple(y.shape) == (B, Cout, Lout)
        full_length = Lout == 1 and pad == 0 and L == ks
        if sum_out is not None:
            assert not with_stats and residual is not None and tuple(sum_out.shape) == tuple(y.shape)
        # tap-vectorised stride-4 forward (audio critic l2..l5 and the penalty's tangent through them), or the engine
        # (the k4 kernel stages x by 16-byte LDS-DMA: an x off 16 bytes - a view into a wider buffer - takes the engine)
        k4 = self._k4(Cin, L, Cout, ks, stride, pad) and x.data_ptr() % 16 == 0
        if k4:
            wk4 = self.packed_k4(w, pad)
        else:
            wp = self.packed_weights(w)[0] if (Cin >= 16 and not full_length) else None
        ws, nws = _workspace(dev, 'm2d_conv1d_workspace_bytes', 0, B, Cin, L, Cout, ks, stride, pad)
        sums = torch.empty((2 * Cout,), dtype=torch.float64, device=dev) if with_stats else None
        if k4:
            _launch("m2d_conv1d_fwd_k4", dev, _ptr(x), _ptr(wk4), _ptr(bias), _ptr(y), _ptr(sum_out), B, Cin, L, Cout,
                    ks, stride, pad, act, slope, _ptr(residual), _ptr(out_mask), out_mask_slope, _ptr(sums), _ptr(ws),
                    nws)
        elif sum_out is not None:
            _launch("m2d_conv1d_fwd_sum", dev, _ptr(x), _ptr(w), _ptr(wp), _ptr(bias), _ptr(y), _ptr(sum_out), B, Cin,
                    L, Cout, ks, stride, pad, act, slope, _ptr(residual), _ptr(out_mask), out_mask_slope, _ptr(ws), nws)
        else:
            _launch("m2d_conv1d_fwd", dev, _ptr(x), _ptr(w), _ptr(wp), _ptr(bias), _ptr(y), B, Cin, L, Cout, ks,
                    stride, pad, act, slope, _ptr(residual), _ptr(out_mask), out_mask_slope, _ptr(sums), _ptr(ws), nws)
        if sum_out is not None:
            return y, sum_out
        return (y, sums) if with_stats else y

    def conv1d_bwd_data(self, dy, w, L, stride, pad, dy_mask=None, dy_mask_slope=0.0, out_mask=None,
                        out_mask_slope=0.0, residual=None, out=None):
        """dx = out_mask * (conv^T(dy * dy_mask, w) + residual); out: write dx there.
        out_mask may hold only the first B / 2 .. B samples: the samples behind them then read the mask from its start
        again (include/m2d.h: m2d_conv1d_bwd_data_shared_mask; no dy_mask / residual in that form)."""
        dev = _chk(dy, w, dy_mask, out_mask, residual, out)
        B, Cout, Lout = dy.shape
        Cout2, Cin, ks = w.shape
        assert Cout == Cout2 and Lout == conv_out_len(L, ks, stride, pad)
        dx = torch.empty((B, Cin, L), dtype=torch.float32, device=dev) if out is None else out
        assert tuple(dx.shape) == (B, Cin, L)
        shared_mask = out_mask is not None and out_mask.shape[0] != B
        if shared_mask:
            mb = out_mask.shape[0]
            assert tuple(out_mask.shape[1:]) == (Cin, L) and 2 * mb >= B and dy_mask is None and residual is None
            wp = self.packed_weights(w)[1]
        else:
            full_length = Lout == 1 and pad == 0 and L == ks
            if (out_mask is not None or residual is not None) and self._thin(Cin, Cout, ks, stride):
                raise _lib.M2dError("conv1d_bwd_data: out_mask / residual are not supported on the thin (Cin = 1, Cout = 32, k25 s4) path")
            wp = None if (full_length or self._thin(Cin, Cout, ks, stride)) else self.packed_weights(w)[1]
        ws, nws = _workspace(dev, 'm2d_conv1d_workspace_bytes', 1, B, Cin, L, Cout, ks, stride, pad)
        if shared_mask:
            _launch("m2d_conv1d_bwd_data_shared_mask", dev, _ptr(dy), _ptr(w), _ptr(wp), _ptr(dx), B, Cin, L, Cout, ks,
                    stride, pad, _ptr(out_mask), out_mask_slope, mb, _ptr(ws), nws)
        elif residual is not None:
            assert tuple(residual.shape) == tuple(dx.shape)
            _launch("m2d_conv1d_bwd_data_res", dev, _ptr(dy), _ptr(w), _ptr(wp), _ptr(dx), B, Cin, L, Cout, ks, stride,
                    pad, _ptr(dy_mask), dy_mask_slope, _ptr(residual), _ptr(out_mask), out_mask_slope, _ptr(ws), nws)
        else:
            _launch("m2d_conv1d_bwd_data", dev, _ptr(dy), _ptr(w), _ptr(wp), _ptr(dx), B, Cin, L, Cout, ks, stride,
                    pad, _ptr(dy_mask), dy_mask_slope, _ptr(out_mask), out_mask_slope, _ptr(ws), nws)
        return dx

    def conv1d_bwd_weight(self, x, dy, ks, stride, pad, dy_mask=None, dy_mask_slope=0.0, with_bias=False,
                          bias_from_sample=0):
        """-> dw, or (dw, dbias) with `with_bias`: dbias = sum over (batch, length) of the masked dy, over the
        samples [bias_from_sample, B) only (rows in front of them pair second-order operands: no bias term)."""
        dev = _chk(x, dy, dy_mask)
        B, Cin, L = x.shape
        B2, Cout, Lout = dy.shape
        assert B == B2 and Lout == conv_out_len(L, ks, stride, pad)
        dw = torch.empty((Cout, Cin, ks), dtype=torch.float32, device=dev)
        # The library takes the bias gradient from the same launch as one all-ones column of the x operand. Where
        # Cin * ks is a multiple of the 128-column tile that column costs a whole extra N tile (the encoder's k4 layers:
        # 129 columns = 2 tiles for 128, 257 = 3 for 256 ...), and for short outputs (K = (l, n) order: both operands
        # row-fast) it also keeps the launch off the LDS-direct kernel (measured in the step: the 128 -> 256 encoder
        # layer's weight gradient 501 us with the column, 190-220 us without). There the bias gradient is one
        # channel-sum pass over dy instead (M2D_SEPARATE_BIAS=0: always the column) - for short outputs and for up to four
        # column tiles; measured not to pay on the critic's layers (profiles/r05_separate_bias_shapes_diff.txt: the pose
        # critic's 896 + 1 columns 95.5 -> 89.2 us + a 22 us pass, the audio critic's 3 200 + 1 columns 567 -> 604 us).
        # (round 6: also for up to eight column tiles when the launch is long - the U-Net's 256 -> 128 k3 blocks at
        # 4 800 x 200 positions: 768 + 1 columns ran 7 tiles for 6.008, 2.46 ms at 77 TFLOP/s; the sum pass costs 0.12 ms)
        sep_bias = (with_bias and self._SEPARATE_BIAS and (Cin * ks) % 128 == 0 and
                    (Lout < 16 or Cin * ks <= 512 or (Cin * ks <= 1024 and B * Lout >= 200000))
                    and not self._thin(Cin, Cout, ks, stride) and _bn_scratch(dev, Cout) is not None)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev) if (with_bias and not sep_bias) else None
        ws, nws = _workspace(dev, 'm2d_conv1d_workspace_bytes', 2, B, Cin, L, Cout, ks, stride, pad)
        if bias_from_sample:
            _launch("m2d_conv1d_bwd_weight_from", dev, _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), B, Cin, L, Cout, ks,
                    stride, pad, _ptr(dy_mask), dy_mask_slope, int(bias_from_sample), _ptr(ws), nws)
        else:
            _launch("m2d_conv1d_bwd_weight", dev, _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), B, Cin, L, Cout, ks, stride,
                    pad, _ptr(dy_mask), dy_mask_slope, _ptr(ws), nws)
        if sep_bias:
            f = int(bias_from_sample)
            db = self.channel_sums(dy[f:] if f else dy, None if dy_mask is None else (dy_mask[f:] if f else dy_mask), dy_mask_slope)
        return (dw, db) if with_bias else dw

    # ---------------------------------------------------------------- conv over the windows of a padded track
    def conv1d_fwd_windows(self, track, T, hop, window, w, bias, stride, pad, act=0, slope=0.0, with_stats=False):
        """track (B, S); logical input (B*T, 1, window), window t of track b = track[b, t*hop : t*hop + window]
        (never materialised). -> y (B*T, Cout, Lout)."""
        dev = _chk(w, bias)
        B, S = _chk_track(track, dev, T, hop, window)
        Cout, Cin, ks = w.shape
        assert Cin == 1, "window views are single-channel"
        Lout = conv_out_len(window, ks, stride, pad)
        y = torch.empty((B * T, Cout, Lout), dtype=torch.float32, device=dev)
        ws, nws = _workspace(dev, 'm2d_conv1d_workspace_bytes', 0, B * T, 1, window, Cout, ks, stride, pad)
        sums = torch.empty((2 * Cout,), dtype=torch.float64, device=dev) if with_stats else None
        _launch("m2d_conv1d_fwd_windows", dev, _ptr(track), B, S, T, hop, window, _ptr(w), _ptr(bias), _ptr(y), Cout,
                ks, stride, pad, act, slope, _ptr(sums), _ptr(ws), nws)
        return (y, sums) if with_stats else y

    def conv1d_bwd_weight_windows(self, track, T, hop, window, dy, ks, stride, pad, dy_mask=None, dy_mask_slope=0.0,
                                  with_bias=False):
        dev = _chk(dy, dy_mask)
        B, S = _chk_track(track, dev, T, hop, window)
        N, Cout, Lout = dy.shape
        assert N == B * T and Lout == conv_out_len(window, ks, stride, pad)
        dw = torch.empty((Cout, 1, ks), dtype=torch.float32, device=dev)
        db = torch.empty((Cout,), dtype=torch.float32, device=dev) if with_bias else None
        ws, nws = _workspace(dev, 'm2d_conv1d_workspace_bytes', 2, B * T, 1, window, Cout, ks, stride, pad)
        _launch("m2d_conv1d_bwd_weight_windows", dev, _ptr(track), B, S, T, hop, window, _ptr(dy), _ptr(dw), _ptr(db),
                Cout, ks, stride, pad, _ptr(dy_mask), dy_mask_slope, _ptr(ws), nws)
        return (dw, db) if with_bias else dw

    # ---------------------------------------------------------------- gemm
    def gemm(self, mode, a, b, bias=None, act=0, slope=0.0, a_mask=None, a_mask_slope=0.0, out_mask=None,
             out_mask_slope=0.0, out=None):
        """mode 0: a(M,K) b(N,K)^T (+bias[N]); 1: a(M,K) b(K,N); 2: a(K,M)^T b(K,N). out: write there (may alias
        out_mask: in-place masking)."""
        dev = _chk(a, b, bias, a_mask, out_mask, out)
        M, N, K = _gemm_shape(mode, a, b)
        c = torch.empty((M, N), dtype=torch.float32, device=dev) if out is None else out
        assert tuple(c.shape) == (M, N)
        ws, nws = _workspace(dev, 'm2d_gemm_workspace_bytes', mode, M, N, K)
        _launch("m2d_gemm", dev, mode, _ptr(a), _ptr(b), _ptr(bias), _ptr(c), M, N, K, act, slope, _ptr(a_mask),
                a_mask_slope, _ptr(out_mask), out_mask_slope, _ptr(ws), nws)
        return c

    @staticmethod
    def _chk_rows(*tensors):
        """2-D fp32 device tensors whose rows are dense (stride(1) == 1) but may be a column block of a wider
        buffer (any stride(0) >= the row length) -> device."""
        dev = None
        for t in tensors:
            if t is None:
                continue
            if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
                raise _lib.M2dError("gemm_ld: 2-D fp32 HIP tensors only")
            if t.size(1) > 1 and t.stride(1) != 1 or (t.size(0) > 1 and t.stride(0) < t.size(1)):
                raise _lib.M2dError("gemm_ld: rows must be dense")
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise _lib.M2dError("tensors on different devices")
        return dev

    @staticmethod
    def _ld(t):
        return t.stride(0) if t.size(0) > 1 else t.size(1)

    def gemm_ld(self, mode, a, b, bias=None, act=0, slope=0.0, a_mask=None, a_mask_slope=0.0, out_mask=None,
                out_mask_slope=0.0, out=None):
        """gemm() on row-strided 2-D views (column blocks of wider buffers): a_mask must share a's layout,
        out_mask the output's (it may BE the output: in-place masking). out: a view to write into."""
        dev = self._chk_rows(a, b, a_mask, out_mask, out)
        _chk(bias)
        M, N, K = _gemm_shape(mode, a, b)
        c = torch.empty((M, N), dtype=torch.float32, device=dev) if out is None else out
        assert tuple(c.shape) == (M, N)
        if a_mask is not None:
            assert a_mask.shape == a.shape and self._ld(a_mask) == self._ld(a)
        if out_mask is not None:
            assert out_mask.shape == c.shape and self._ld(out_mask) == self._ld(c)
        ws, nws = _workspace(dev, 'm2d_gemm_workspace_bytes', mode, M, N, K)
        _launch("m2d_gemm_ld", dev, mode, _ptr(a), self._ld(a), _ptr(b), self._ld(b), _ptr(bias), _ptr(c), self._ld(c),
                M, N, K, act, slope, _ptr(a_mask), a_mask_slope, _ptr(out_mask), out_mask_slope, _ptr(ws), nws)
        return c

    # ---------------------------------------------------------------- tanh heads
    def tanh_fwd(self, x):
        dev = _chk(x)
        y = torch.empty_like(x)
        _launch("m2d_tanh_fwd", dev, _ptr(x), _ptr(y), x.numel())
        return y

    def tanh_bwd(self, gy, y):
        """gy * (1 - y^2)"""
        dev = _chk(gy, y)
        gx = torch.empty_like(gy)
        _launch("m2d_tanh_bwd", dev, _ptr(gy), _ptr(y), _ptr(gx), gy.numel())
        return gx

    def tanh_bwd_bwd(self, g, gy, y):
        """-2 * y * g * gy: the gradient of tanh_bwd(gy, y) w.r.t. y for cotangent g"""
        dev = _chk(g, gy, y)
        out = torch.empty_like(y)
        _launch("m2d_tanh_bwd_bwd", dev, _ptr(g), _ptr(gy), _ptr(y), _ptr(out), y.numel())
        return out

    def adam_multi(self, params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, step, skip=None, repack=True,
                   ema=None, ema_decay=None):
        """One torch.optim.Adam step (defaults: no weight decay, no amsgrad) over the listed tensors in one launch per 48
        (include/m2d.h: m2d_adam_multi). repack: conv weights (3-D, >= 16 input channels) that have live packed images in
        the weight cache get those images rewritten in the same pass - the cache entries stay valid across the step
        (the engines call invalidate_packed() for everything else). skip: optional device float (non-zero = no-op).
        ema: a list parallel to `params` of shadow tensors (or None per tensor) that the same launch moves towards the
        fresh parameters, e += (1 - ema_decay) * (p - e) (m2d_adam_multi_ema, one launch per 40); their cached images
        are NOT rewritten - the caller drops them with invalidate_packed(). ema=None: m2d_adam_multi."""
        if not params:
            return
        shadows = () if ema is None else [e for e in ema if e is not None]
        dev = _chk(*params, *grads, *exp_avgs, *exp_avg_sqs, *shadows, skip if torch.is_tensor(skip) else None)
        items = (_lib.AdamItem * len(params))()
        keep = []
        for it, p, g, m, v in zip(items, params, grads, exp_avgs, exp_avg_sqs):
            assert p.numel() == g.numel() == m.numel() == v.numel()
            it.param, it.grad, it.exp_avg, it.exp_avg_sq, it.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            key = (id(p), "conv")
            ent = self._packed.get(key) if (repack and p.dim() == 3) else None
            if ent is not None and ent[0]() is p:
                # written on THIS stream; consumers on other streams fork behind it (side.wait_stream(main) in the
                # modules), so the refreshed entry is marked valid for every stream (None)
                wf, wb = ent[3]
                it.pack_fwd, it.pack_bwd = wf.data_ptr(), wb.data_ptr()
                it.cout, it.cin, it.ks = p.shape
                keep.append((key, (ent[0], p._version, None, ent[3])))
        bc1 = 1.0 - beta1 ** step
        bc2s = (1.0 - beta2 ** step) ** 0.5
        skip_word = (skip if isinstance(skip, int) else _ptr(skip)) or 0
        if ema is None:
            _launch("m2d_adam_multi", dev, ctypes.addressof(items), len(params), lr, beta1, beta2, eps, bc1, bc2s,
                    skip_word)
        else:
            if ema_decay is None or len(ema) != len(params):
                raise _lib.M2dError("adam_multi: ema needs ema_decay and one entry (tensor or None) per parameter")
            for p, e in zip(params, ema):
                if e is not None and (e.numel() != p.numel() or e.data_ptr() == p.data_ptr()):
                    raise _lib.M2dError("adam_multi: a shadow has its parameter's element count and storage of its own")
            shadow_ptrs = (ctypes.c_void_p * len(params))(*[None if e is None else e.data_ptr() for e in ema])
            omd = 1.0 - float(ema_decay)   # (rounded to fp32 once, by the call)
            _launch("m2d_adam_multi_ema", dev, ctypes.addressof(items), ctypes.addressof(shadow_ptrs), len(params), lr,
                    beta1, beta2, eps, bc1, bc2s, omd, skip_word)
        for key, ent in keep:
            self._packed[key] = ent
        # (accumulated over the launches of one optimizer step - several step groups / 48-tensor batches - and consumed
        # by the invalidate_packed() that follows the step)
        self._adam_kept.update(k for k, _ in keep)

    # ---------------------------------------------------------------- critic iteration: pack + loss
    def pose_pack3(self, real, fake_rows, alpha, out=None):
        """real (B, T, C), fake_rows (B*T, C), alpha (B,) -> (3B, C, T) = [interpolated | real | fake] channels-first."""
        dev = _chk(real, fake_rows, alpha, out)
        B, T, C = real.shape
        assert fake_rows.numel() == real.numel() and alpha.numel() == B
        o = torch.empty((3 * B, C, T), dtype=torch.float32, device=dev) if out is None else out
        _launch("m2d_pose_pack3", dev, _ptr(real), _ptr(fake_rows), _ptr(alpha), _ptr(o), B, T, C)
        return o

    def wgan_critic_loss(self, scores, B, pen0, pen1, gamma):
        """scores (3B,) = [interpolated | real | fake] -> (3,) = (loss_critic, gp, w_dist)."""
        dev = _chk(scores, pen0, pen1)
        assert scores.numel() == 3 * B
        out = torch.empty((3,), dtype=torch.float32, device=dev)
        _launch("m2d_wgan_critic_loss", dev, _ptr(scores), B, _ptr(pen0), _ptr(pen1), float(gamma), _ptr(out))
        return out

    # ---------------------------------------------------------------- batch norm
    def channel_sums(self, x, mask=None, slope=0.0):
        """x: (B, C, L) or (B, C) -> (C,) sums over batch and length (optionally masked)."""
        dev = _chk(x, mask)
        B, C, L = _bcl(x)
        out = torch.empty((C,), dtype=torch.float32, device=dev)
        scratch = _bn_scratch(dev, C)
        # no zero-kept scratch (C wider than the fixed one, or a capture that was not given one): the stateless
        # three-launch form needs its workspace (passing none made the call fail with "workspace too small")
        ws, nws = (None, 0) if scratch is not None else _workspace(dev, 'm2d_bn_workspace_bytes', C)
        _launch("m2d_channel_sums", dev, _ptr(x), _ptr(mask), slope, _ptr(out), B, C, L, _ptr(ws), nws, _ptr(scratch))
        return out

    @staticmethod
    def _out_block(out, shape, dev):
        """`out`: where a result of `shape` = (B, C, L) goes when it is a channel block of a wider buffer - a view
        shaped like the result whose samples are out.stride(0) elements apart, dense inside a sample; None: a fresh
        dense tensor. -> (tensor, batch stride; 0 = dense)"""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=dev), 0
        assert out.shape == shape and out.dtype == torch.float32 and out.device == dev
        assert out.dim() == 3 and out.stride(2) == 1 and out.stride(1) == out.shape[2] and out.stride(0) >= out.shape[1] * out.shape[2]
        return out, out.stride(0)

    def _bn_fwd_begin(self, x, gamma, beta, running_mean, running_var, residual=None, sums=None, out=None, up=1):
        """What the BatchNorm forwards share: the tensor checks, the result ((B, C, up * L), placed by `_out_block`) and the
        two (C,) rows kept for the backward. -> dev, (B, C, L), y, its batch stride, save_mean, save_invstd"""
        dev = _chk(x, gamma, beta, running_mean, running_var, residual)
        B, C, L = _bcl(x)
        if sums is not None:
            self._sums_ok(sums, C, dev)
        y, ypitch = self._out_block(out, x.shape if up == 1 else (B, C, up * L), dev)
        save_mean = torch.empty((C,), dtype=torch.float32, device=dev)
        save_invstd = torch.empty((C,), dtype=torch.float32, device=dev)
        return dev, (B, C, L), y, ypitch, save_mean, save_invstd

    def bn_fwd(self, x, gamma, beta, running_mean, running_var, training, eps, momentum, act=0, slope=0.0,
               residual=None, out=None):
        dev, (B, C, L), y, ypitch, save_mean, save_invstd = self._bn_fwd_begin(x, gamma, beta, running_mean, running_var,
                                                                              residual, None, out)
        ws, nws = _workspace(dev, 'm2d_bn_workspace_bytes', C)
        _launch("m2d_bn_fwd_to", dev, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(y),
                _ptr(save_mean), _ptr(save_invstd), B, C, L, eps, momentum, 1 if training else 0, act, slope,
                _ptr(residual), _ptr(ws), nws, _ptr(_bn_scratch(dev, C)) if training else 0, ypitch)
        return y, save_mean, save_invstd

    @staticmethod
    def _sums_ok(sums, C, dev):
        if sums.dtype != torch.float64 or sums.numel() != 2 * C or not sums.is_contiguous() or sums.device != dev:
            raise _lib.M2dError("BatchNorm sums must be a contiguous float64 tensor of 2*C elements on the device")

    def bn_stats(self, x):
        """(2C,) float64: per-channel sum and sum of squares of x (B, C[, L]) over batch and length."""
        dev = _chk(x)
        B, C, L = _bcl(x)
        sums = torch.empty((2 * C,), dtype=torch.float64, device=dev)
        _launch("m2d_bn_stats", dev, _ptr(x), _ptr(sums), B, C, L, _ptr(_bn_scratch(dev, C)))
        return sums

    def bn_fwd_sums(self, x, sums, count, gamma, beta, running_mean, running_var, eps, momentum, act=0, slope=0.0,
                    residual=None, out=None):
        """Training forward from batch sums over `count` elements per channel (bn_stats, a conv's epilogue, or
        their all-reduce across data-parallel ranks). -> y, save_mean, save_invstd."""
        dev, (B, C, L), y, ypitch, save_mean, save_invstd = self._bn_fwd_begin(x, gamma, beta, running_mean, running_var,
                                                                              residual, sums, out)
        _launch("m2d_bn_fwd_sums_to", dev, _ptr(x), _ptr(sums), float(count), _ptr(gamma), _ptr(beta),
                _ptr(running_mean), _ptr(running_var), _ptr(y), _ptr(save_mean), _ptr(save_invstd), B, C, L, eps,
                momentum, act, slope, _ptr(residual), ypitch)
        return y, save_mean, save_invstd

    def bn_update_running(self, sums, count, running_mean, running_var, eps, momentum):
        """running buffers advanced once more with batch sums they were already advanced with (include/m2d.h)"""
        dev = _chk(running_mean, running_var)
        C = running_mean.numel()
        self._sums_ok(sums, C, dev)
        tmp = torch.empty((2 * C,), dtype=torch.float32, device=dev)
        _launch("m2d_bn_update_running", dev, _ptr(sums), float(count), _ptr(running_mean), _ptr(running_var),
                _ptr(tmp), C, eps, momentum)

    def bn_fwd_sums_pool(self, x, sums, count, gamma, beta, running_mean, running_var, eps, momentum, act=0, slope=0.0,
                         out=None):
        """bn_fwd_sums with MaxPool1d(2, 2) of the result made in the same pass. -> (y, pooled, save_mean, save_invstd);
        out: where y goes (a channel block of a wider buffer, as bn_fwd_sums)."""
        dev, (B, C, L), y, ypitch, save_mean, save_invstd = self._bn_fwd_begin(x, gamma, beta, running_mean, running_var,
                                                                              None, sums, out)
        pooled = torch.empty((B, C, L // 2), dtype=torch.float32, device=dev)
        _launch("m2d_bn_fwd_sums_pool_to", dev, _ptr(x), _ptr(sums), float(count), _ptr(gamma), _ptr(beta),
                _ptr(running_mean), _ptr(running_var), _ptr(y), _ptr(pooled), _ptr(save_mean), _ptr(save_invstd), B, C,
                L, eps, momentum, act, slope, ypitch)
        return y, pooled, save_mean, save_invstd

    def bn_fwd_sums_upsample2(self, x, sums, count, gamma, beta, running_mean, running_var, eps, momentum, act=0, slope=0.0,
                              out=None):
        """upsample2_linear(bn_fwd_sums(x)) in one pass (the normalised tensor itself is not written).
        -> (up (B, C, 2L), save_mean, save_invstd); out: a (B, C, 2L) channel block of a wider buffer."""
        dev, (B, C, L), up, pitch, save_mean, save_invstd = self._bn_fwd_begin(x, gamma, beta, running_mean, running_var,
                                                                              None, sums, out, up=2)
        _launch("m2d_bn_fwd_sums_upsample2_to", dev, _ptr(x), _ptr(sums), float(count), _ptr(gamma), _ptr(beta),
                _ptr(running_mean), _ptr(running_var), _ptr(up), _ptr(save_mean), _ptr(save_invstd), B, C, L, eps,
                momentum, act, slope, pitch)
        return up, save_mean, save_invstd

    def bn_bwd_stats(self, dy, x, gamma, beta, save_mean, save_invstd, act=0, slope=0.0):
        """(2C,) float64: sum dz and sum dz * xhat, dz = dy * act'(bn(x))."""
        dev = _chk(dy, x, gamma, beta, save_mean, save_invstd)
        B, C, L = _bcl(x)
        sums = torch.empty((2 * C,), dtype=torch.float64, device=dev)
        _launch("m2d_bn_bwd_stats", dev, _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(save_mean),
                _ptr(save_invstd), _ptr(sums), B, C, L, act, slope, _ptr(_bn_scratch(dev, C)))
        return sums

    def _bn_bwd_begin(self, dy, x, gamma, beta, save_mean, save_invstd, *sums):
        """What the two backwards share: the checks, the three results and the workspace."""
        dev = _chk(dy, x, gamma, beta, save_mean, save_invstd)
        B, C, L = _bcl(x)
        for s in sums:
            self._sums_ok(s, C, dev)
        dx = torch.empty_like(x)
        dgamma = torch.empty((C,), dtype=torch.float32, device=dev)
        dbeta = torch.empty((C,), dtype=torch.float32, device=dev)
        return (dev, (B, C, L), dx, dgamma, dbeta) + _workspace(dev, 'm2d_bn_workspace_bytes', C)

    def bn_bwd_sums(self, dy, x, gamma, beta, save_mean, save_invstd, sums_local, sums_global, count, act=0, slope=0.0):
        dev, (B, C, L), dx, dgamma, dbeta, ws, nws = self._bn_bwd_begin(dy, x, gamma, beta, save_mean, save_invstd,
                                                                       sums_local, sums_global)
        _launch("m2d_bn_bwd_sums", dev, _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(save_mean), _ptr(save_invstd),
                _ptr(sums_local), _ptr(sums_global), float(count), _ptr(dx), _ptr(dgamma), _ptr(dbeta), B, C, L, act,
                slope, _ptr(ws), nws)
        return dx, dgamma, dbeta

    def bn_bwd(self, dy, x, gamma, beta, save_mean, save_invstd, act=0, slope=0.0):
        dev, (B, C, L), dx, dgamma, dbeta, ws, nws = self._bn_bwd_begin(dy, x, gamma, beta, save_mean, save_invstd)
        _launch("m2d_bn_bwd", dev, _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(save_mean), _ptr(save_invstd),
                _ptr(dx), _ptr(dgamma), _ptr(dbeta), B, C, L, act, slope, _ptr(ws), nws, _ptr(_bn_scratch(dev, C)))
        return dx, dgamma, dbeta

    # ---------------------------------------------------------------- GRU
    @staticmethod
    def _chk_lengths(lengths, dev, B):
        """per-sequence lengths handed to a kernel: a contiguous int32 tensor of B entries on the kernels' device"""
        if lengths is None:
            return
        if not lengths.is_cuda or lengths.device != dev or lengths.dtype != torch.int32 or not lengths.is_contiguous():
            raise _lib.M2dError("GRU lengths must be a contiguous int32 tensor on %s (got %s %s)"
                                % (dev, lengths.dtype, lengths.device))
        if lengths.numel() != B:
            raise _lib.M2dError("GRU lengths: %d entries for a batch of %d" % (lengths.numel(), B))

    def gru_layer_fwd(self, gi, w_hh_t, b_hh, lengths=None, save=True):
        """gi: (B, T, 3H) with b_ih added; w_hh_t: (H, 3H). Returns out (B,T,H), saved gates or None."""
        dev = _chk(gi, w_hh_t, b_hh)
        B, T, H3 = gi.shape
        H = H3 // 3
        self._chk_lengths(lengths, dev, B)
        out = torch.empty((B, T, H), dtype=torch.float32, device=dev)
        saved = torch.empty((4, B, T, H), dtype=torch.float32, device=dev) if save else None
        _launch("m2d_gru_layer_fwd", dev, _ptr(gi), _ptr(w_hh_t), _ptr(b_hh), _ptr(lengths), _ptr(out),
                *([_ptr(g) for g in saved] if save else [0] * 4), B, T, H)
        return out, saved

    def gru_layer_bwd(self, dout, out, saved, w_hh, lengths=None):
        dev = _chk(dout, out, saved, w_hh)
        B, T, H = out.shape
        self._chk_lengths(lengths, dev, B)
        dgi = torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev)
        dgh = torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev)
        dh_buf = torch.empty((2, B, H), dtype=torch.float32, device=dev)
        _launch("m2d_gru_layer_bwd", dev, _ptr(dout), _ptr(out), *[_ptr(g) for g in saved], _ptr(w_hh), _ptr(lengths),
                _ptr(dgi), _ptr(dgh), _ptr(dh_buf), B, T, H)
        return dgi, dgh

    def gru_small_fwd(self, gi, w_hh, b_hh, lengths=None, save=True, with_out=True):
        """One GRU layer with 1 <= H <= 16 in one launch. gi: (B, T, 3H) with b_ih added; w_hh: (3H, H).
        Returns (out (B,T,H) or None, h_n (B,H), saved (4,B,T,H) or None); save implies out (the backward reads it)."""
        dev = _chk(gi, w_hh, b_hh)
        B, T, H3 = gi.shape
        H = H3 // 3
        self._chk_lengths(lengths, dev, B)
        out = torch.empty((B, T, H), dtype=torch.float32, device=dev) if (with_out or save) else None
        h_n = torch.empty((B, H), dtype=torch.float32, device=dev)
        saved = torch.empty((4, B, T, H), dtype=torch.float32, device=dev) if save else None
        _launch("m2d_gru_small_fwd", dev, _ptr(gi), _ptr(w_hh), _ptr(b_hh), _ptr(lengths), _ptr(out), _ptr(h_n),
                _ptr(saved), B, T, H)
        return out, h_n, saved

    def gru_small_bwd(self, dout, dh_n, out, saved, w_hh, lengths=None):
        """BPTT of gru_small_fwd (dout and / or dh_n may be None) -> (dgi, dgh), each (B, T, 3H)."""
        dev = _chk(dout, dh_n, out, saved, w_hh)
        B, T, H = out.shape
        self._chk_lengths(lengths, dev, B)
        dgi = torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev)
        dgh = torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev)
        _launch("m2d_gru_small_bwd", dev, _ptr(dout), _ptr(dh_n), _ptr(out), _ptr(saved), _ptr(w_hh), _ptr(lengths),
                _ptr(dgi), _ptr(dgh), B, T, H)
        return dgi, dgh

    @staticmethod
    def _ptr_array(tensors):
        if tensors is None:
            return None, None
        arr = (ctypes.c_void_p * len(tensors))(*[_ptr(t) for t in tensors])
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    def _gru_counters(self, dev, B, L, persistent):
        """the scratch that requests the persistent form (one launch for the whole recurrence; the library decides),
        or None: step launches, by the caller's wish or after a recovered time-out (recover_async_fault)"""
        return (torch.empty((_lib.lib().m2d_gru_stack_counters(B, L),), dtype=torch.int32, device=dev)
                if (persistent and self.persistent_gru) else None)

    def gru_stack_fwd(self, gi0, w_ih_t, b_ih, w_hh_t, b_hh, lengths=None, save=True, persistent=True, h0=None,
                      want_state=False):
        """L-layer GRU on the (layer, t) diagonal. Lists have L entries (entry 0 of w_ih_t / b_ih may
        be None). Returns ([out_l (B,T,H)], [saved_l (4,B,T,H)] or None).
        h0: the initial state, (L, B, H) or a list of L (B, H) tensors (None: zeros); want_state: also return h_n
        (L, B, H), the state after step lengths[b] - 1 (T - 1 without lengths) -> (outs, saved, h_n)."""
        L = len(w_hh_t)
        dev = _chk(gi0, *[t for t in list(w_ih_t) + list(b_ih) + list(w_hh_t) + list(b_hh) if t is not None])
        B, T, H3 = gi0.shape
        H = H3 // 3
        self._chk_lengths(lengths, dev, B)
        if h0 is not None:
            h0 = list(h0)
            if len(h0) != L or any(tuple(t.shape) != (B, H) for t in h0) or _chk(*h0) != dev:
                raise _lib.M2dError("GRU h0: %d layers of (%d, %d) on %s expected" % (L, B, H, dev))
        # (one allocation: the persistent launch pre-fills every layer's output with its hand-off sentinel in one memset)
        outs = list(torch.empty((L, B, T, H), dtype=torch.float32, device=dev).unbind(0))
        saved = [torch.empty((4, B, T, H), dtype=torch.float32, device=dev) for _ in range(L)] if save else None
        h_n = torch.empty((L, B, H), dtype=torch.float32, device=dev) if want_state else None
        keep = [self._ptr_array(v) for v in (w_ih_t, b_ih, w_hh_t, b_hh, outs, saved, h0,
                                             h_n.unbind(0) if want_state else None)]
        counters = self._gru_counters(dev, B, L, persistent)
        state = h0 is not None or want_state  # (without one, the entry point without: its name is in the error texts)
        _launch("m2d_gru_stack_fwd_state" if state else "m2d_gru_stack_fwd", dev, _ptr(gi0), *[k[1] for k in keep[:6]],
                _ptr(lengths), *([keep[6][1], keep[7][1]] if state else []), B, T, H, L, _ptr(counters))
        return (outs, saved, h_n) if want_state else (outs, saved)

    @staticmethod
    def check_async_errors():
        """Raise if a persistent GRU launch timed out (another process holding the CUs it waits for).
        Call after a stream synchronisation; cheap (reads one pinned host word)."""
        if _lib.lib().m2d_gru_persist_error():
            raise _lib.M2dError("persistent GRU launch timed out: outputs of that call are invalid "
                                "(several processes on one GPU? set M2D_PERSISTENT_GRU=0)")

    # -- recovery from such a timeout inside the process (engine.WganGpEngine._check_async)
    persistent_gru = True        # False: every recurrence from now on runs as per-step launches
    async_faults = 0             # timeouts recovered from

    @staticmethod
    def fault_word():
        """Device-visible address of the word a persistent recurrence raises when it gives up (or None): the `skip`
        argument of adam_multi - an optimizer step queued behind the failed launch then voids itself on the device."""
        return _lib.lib().m2d_async_fault_word() or None

    @staticmethod
    def fault_fetch(dst):
        """dst[0] (device float) = 1.0 when that word is raised, else 0.0, on the current stream (dp.GradExchange)"""
        _launch("m2d_fault_fetch", _chk(dst), _ptr(dst))

    @staticmethod
    def raise_async_fault():
        """test hook: raise the word as a timed-out recurrence would"""
        _lib.check(_lib.lib().m2d_gru_persist_raise(), "m2d_gru_persist_raise")

    @classmethod
    def recover_async_fault(cls):
        """-> True when a persistent recurrence had timed out. The word is still raised at this point, so after the
        device synchronisation made here EVERY optimizer step queued behind the failed launch has skipped itself (no
        garbage reached the parameters); then the word is cleared, the scratch re-zeroed, and recurrences run as
        per-step launches from now on (fresh launches - nothing is re-executed, the affected iterations are lost)."""
        if not _lib.lib().m2d_gru_persist_peek():
            return False
        torch.cuda.synchronize()
        _lib.lib().m2d_gru_persist_error()
        reset_scratch()
        cls.persistent_gru = False
        cls.async_faults += 1
        return True

    def gru_stack_bwd(self, dout, outs, saved, w_hh, w_ih, lengths=None, persistent=True):
        """BPTT of the stack; returns ([dgi_l (B,T,3H)], [dgh_l (B,T,3H)]). persistent: one launch for the whole
        recurrence when the library finds room for it (bit-identical to the step launches)."""
        L = len(outs)
        dev = _chk(dout, *outs, *saved, *w_hh, *[t for t in w_ih if t is not None])
        B, T, H = outs[0].shape
        self._chk_lengths(lengths, dev, B)
        dgi = [torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev) for _ in range(L)]
        dgh = [torch.empty((B, T, 3 * H), dtype=torch.float32, device=dev) for _ in range(L)]
        dhb = [torch.empty((2, B, H), dtype=torch.float32, device=dev) for _ in range(L)]
        keep = [self._ptr_array(v) for v in (outs, saved, w_hh, w_ih, dgi, dgh, dhb)]
        counters = self._gru_counters(dev, B, L, persistent)
        _launch("m2d_gru_stack_bwd", dev, _ptr(dout), *[k[1] for k in keep], _ptr(lengths), B, T, H, L, _ptr(counters))
        return dgi, dgh

    # ---------------------------------------------------------------- gradient penalty
    def gp_interpolate(self, real, fake, alpha):
        """real, fake: (B, n); alpha: (B,) -> alpha*real + (1-alpha)*fake."""
        dev = _chk(real, fake, alpha)
        B, n = real.shape
        out = torch.empty_like(real)
        _launch("m2d_gp_interpolate", dev, _ptr(real), _ptr(fake), _ptr(alpha), _ptr(out), B, n)
        return out

    def gp_penalty_fwd(self, g, lp):
        dev = _chk(g)
        B, n = g.shape
        norms = torch.empty((B,), dtype=torch.float32, device=dev)
        pen = torch.empty((), dtype=torch.float32, device=dev)
        ws, nws = _workspace(dev, 'm2d_gp_penalty_workspace_bytes', B)
        _launch("m2d_gp_penalty_fwd", dev, _ptr(g), _ptr(norms), _ptr(pen), B, n, 1 if lp else 0, _ptr(ws), nws)
        return pen, norms

    def gp_penalty_bwd(self, g, norms, gout, lp, out=None):
        dev = _chk(g, norms, gout, out)
        B, n = g.shape
        dg = torch.empty_like(g) if out is None else out
        assert dg.numel() == g.numel()
        _launch("m2d_gp_penalty_bwd", dev, _ptr(g), _ptr(norms), _ptr(gout), _ptr(dg), B, n, 1 if lp else 0)
        return dg

    # ---------------------------------------------------------------- losses
    def l1_mean_fwd(self, a, b):
        dev = _chk(a, b)
        out = torch.empty((), dtype=torch.float32, device=dev)
        ws, nws = _workspace(dev, 'm2d_reduce_workspace_bytes')
        _launch("m2d_l1_mean_fwd", dev, _ptr(a), _ptr(b), _ptr(out), a.numel(), _ptr(ws), nws)
        return out

    def l1_mean_bwd(self, a, b, gout):
        dev = _chk(a, b, gout)
        da = torch.empty_like(a)
        _launch("m2d_l1_mean_bwd", dev, _ptr(a), _ptr(b), _ptr(gout), _ptr(da), a.numel())
        return da

    def cross_entropy_fwd(self, logits, labels, with_pred=False):
        """mean softmax cross-entropy of (B, C) logits against int64 labels -> (0-dim loss, int64 argmax or None)"""
        dev = _chk(logits)
        B, C = logits.shape
        _chk_labels(labels, dev, B, "cross entropy")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        pred = torch.empty((B,), dtype=torch.int64, device=dev) if with_pred else None
        ws, nws = _workspace(dev, 'm2d_cross_entropy_workspace_bytes', B, C)
        _launch("m2d_cross_entropy_fwd", dev, _ptr(logits), _ptr(labels), _ptr(loss), _ptr(pred), B, C, _ptr(ws), nws)
        return loss, pred

    def cross_entropy_bwd(self, logits, labels, gout):
        dev = _chk(logits, gout)
        B, C = logits.shape
        _chk_labels(labels, dev, B, "cross entropy")
        dlogits = torch.empty_like(logits)
        _launch("m2d_cross_entropy_bwd", dev, _ptr(logits), _ptr(labels), _ptr(gout), _ptr(dlogits), B, C)
        return dlogits

    @staticmethod
    def _chk_bce(x, n0, n1):
        if not x.is_contiguous() or x.numel() != n0 + n1:
            raise _lib.M2dError("bce on logits: %d contiguous logits expected for segments of %d + %d"
                                % (x.numel(), n0, n1))

    def bce_logits_fwd(self, x, n0, t0, n1=0, t1=0.0, with_dx=False):
        """BCEWithLogitsLoss(mean) of logits[:n0] against t0 plus that of logits[n0:n0 + n1] against t1 ->
        (out (3,) = (sum of the two means, mean_0, mean_1), dx = d out[0] / d logits (shape of x) or None)"""
        dev = _chk(x)
        self._chk_bce(x, n0, n1)
        out = torch.empty((3,), dtype=torch.float32, device=dev)
        dx = torch.empty_like(x) if with_dx else None
        _launch("m2d_bce_logits_fwd", dev, _ptr(x), int(n0), float(t0), int(n1), float(t1), _ptr(out), _ptr(dx))
        return out, dx

    def bce_logits_bwd(self, x, n0, t0, n1, t1, gout):
        """dx = gout[0] * (sigmoid(x) - t) / n_segment; gout a device scalar"""
        dev = _chk(x, gout)
        self._chk_bce(x, n0, n1)
        dx = torch.empty_like(x)
        _launch("m2d_bce_logits_bwd", dev, _ptr(x), int(n0), float(t0), int(n1), float(t1), _ptr(gout), _ptr(dx))
        return dx

    # ---------------------------------------------------------------- label conditioning and dropout (cond.hip)
    def label_concat(self, x, E, labels, layout, out=None):
        """[x | E[labels[b]]]: layout 0 x (B, T, C) -> (B, T, C + D); layout 1 x (B, C, T) -> (B, C + D, T)"""
        dev = _chk(x, E, out)
        B = x.shape[0]
        _chk_labels(labels, dev, B, "label_concat")
        L, D = E.shape
        if layout == 0:
            T, C = x.shape[1], x.shape[2]
            shape = (B, T, C + D)
        else:
            C, T = x.shape[1], x.shape[2]
            shape = (B, C + D, T)
        o = torch.empty(shape, dtype=torch.float32, device=dev) if out is None else out
        assert tuple(o.shape) == shape
        _launch("m2d_label_concat", dev, _ptr(x), _ptr(E), _ptr(labels), _ptr(o), B, T, C, L, D, int(layout))
        return o

    def pose_pack3_label(self, real, fake_rows, alpha, E, real_lbl, fake_lbl, out=None):
        """real (B, T, C), fake_rows (B*T, C), alpha (B,), E (L, D) -> (3B, C + D, T) = [interpolated | real | fake]
        channels-first with the label channels (real labels on the first two blocks, fake labels on the last)."""
        dev = _chk(real, fake_rows, alpha, E, out)
        B, T, C = real.shape
        L, D = E.shape
        assert fake_rows.numel() == real.numel() and alpha.numel() == B
        _chk_labels(real_lbl, dev, B, "pose_pack3_label")
        _chk_labels(fake_lbl, dev, B, "pose_pack3_label")
        o = torch.empty((3 * B, C + D, T), dtype=torch.float32, device=dev) if out is None else out
        assert tuple(o.shape) == (3 * B, C + D, T)
        _launch("m2d_pose_pack3_label", dev, _ptr(real), _ptr(fake_rows), _ptr(alpha), _ptr(E), _ptr(real_lbl),
                _ptr(fake_lbl), _ptr(o), B, T, C, L, D)
        return o

    def label_embed_bwd(self, dx, labels, r0, r1, c0, L, D, layout, out=None):
        """dE (L, D) = per class, the sum over rows [r0, r1) carrying it (labels: one per row of the range) of
        dx[row, c0:c0 + D, :] summed over time; layout 0: dx (R, T, Ctot), layout 1: dx (R, Ctot, T)"""
        dev = _chk(dx, out)
        _chk_labels(labels, dev, r1 - r0, "label_embed_bwd")
        assert 0 <= r0 < r1 <= dx.shape[0]
        T, Ctot = (dx.shape[1], dx.shape[2]) if layout == 0 else (dx.shape[2], dx.shape[1])
        o = torch.empty((L, D), dtype=torch.float32, device=dev) if out is None else out
        _launch("m2d_label_embed_bwd", dev, _ptr(dx), _ptr(labels), _ptr(o), int(r0), int(r1), T, Ctot, int(c0),
                int(L), int(D), int(layout))
        return o

    def randn_frames(self, seed, frame0, B, n, C, device, out=None):
        """(B, n, C) standard normals; entry (b, i, c) is a pure function of (seed, b, frame0 + i, c) (m2d_randn_frames)"""
        o = torch.empty((B, n, C), dtype=torch.float32, device=device) if out is None else out
        dev = _chk(o)
        if tuple(o.shape) != (B, n, C) or o.dtype != torch.float32 or not o.is_contiguous():
            raise _lib.M2dError("randn_frames: out must be a contiguous float32 (%d, %d, %d) tensor" % (B, n, C))
        _launch("m2d_randn_frames", dev, _ptr(o), int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame0), int(B), int(n), int(C))
        return o

    def render_sticks(self, poses, height, width, out=None):
        """poses (n, 69) or (n, 23, 3) fp32 -> (n, height, width, 3) uint8 RGB stick figures (m2d_render_sticks)"""
        dev = _chk(poses)
        if poses.dim() not in (2, 3) or tuple(poses.shape[1:]) not in ((69,), (23, 3)):
            raise _lib.M2dError("render_sticks: poses must be (n, 69) or (n, 23, 3), got %s" % (tuple(poses.shape),))
        if not (1 <= int(height) <= 4096 and 1 <= int(width) <= 4096):
            raise _lib.M2dError("render_sticks: height and width must lie in [1, 4096], got %d x %d" % (height, width))
        n = poses.shape[0]
        shape = (n, int(height), int(width), 3)
        o = torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else out
        if (not o.is_cuda or o.device != dev or o.dtype != torch.uint8 or tuple(o.shape) != shape
                or not o.is_contiguous()):
            raise _lib.M2dError("render_sticks: out must be a contiguous uint8 %s tensor on %s" % (shape, dev))
        _launch("m2d_render_sticks", dev, _ptr(poses), n, int(height), int(width), _ptr(o))
        return o

    def jpeg_encode(self, frames, qtabs, capacity=None):
        """frames (n, H, W, 3) uint8 RGB on a HIP device (contiguous, any byte alignment), qtabs two quantisation
        tables of 64 entries in 1..255 (row-major) -> (out, offsets): the frames' JPEG streams back to back in the
        uint8 device buffer `out` of `capacity` bytes (default: the raw frame bytes) and the int64 device tensor
        offsets (n + 1). When offsets[n] exceeds the capacity nothing was written: call again with that capacity
        (m2d_jpeg_encode; no host synchronisation here)"""
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise _lib.M2dError("jpeg_encode: frames must be a tensor on a HIP device; there is no CPU path")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise _lib.M2dError("jpeg_encode: frames must be uint8 (n, H, W, 3), got %s %s"
                                % (frames.dtype, tuple(frames.shape)))
        if not frames.is_contiguous():
            raise _lib.M2dError("jpeg_encode: frames must be contiguous")
        n, H, W = (int(s) for s in frames.shape[:3])
        if not (1 <= H <= 4096 and 1 <= W <= 4096):
            raise _lib.M2dError("jpeg_encode: height and width must lie in [1, 4096], got %d x %d" % (H, W))
        q = [int(v) for t in qtabs for v in t]
        if len(q) != 128 or not all(1 <= v <= 255 for v in q):
            raise _lib.M2dError("jpeg_encode: qtabs must be two tables of 64 entries in 1..255")
        dev = frames.device
        cap = n * H * W * 3 if capacity is None else int(capacity)
        if cap < 0:
            raise _lib.M2dError("jpeg_encode: capacity < 0")
        out = torch.empty((cap,), dtype=torch.uint8, device=dev)
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        ws, nws = _workspace(dev, "m2d_jpeg_workspace_bytes", n, H, W)
        _launch("m2d_jpeg_encode", dev, _ptr(frames), n, H, W, bytes(q), _ptr(out), cap, _ptr(offsets), _ptr(ws), nws)
        return out, offsets

    @staticmethod
    def _chk_audio_rows(t, what):
        """fp32 rows on a HIP device, unit stride inside a row (a column slice of a wider buffer is fine) -> leading
        dimension"""
        if not t.is_cuda:
            raise _lib.M2dError("m2d kernels need HIP device tensors (got %s); there is no CPU path" % t.device)
        if t.dtype != torch.float32 or t.dim() != 2:
            raise _lib.M2dError("resample_poly: %s must be a 2-D float32 tensor" % what)
        B, n = t.shape
        if n > 1 and t.stride(1) != 1:
            raise _lib.M2dError("resample_poly: the rows of %s must be dense" % what)
        ld = t.stride(0) if B > 1 and n > 0 else n
        if ld < n:
            raise _lib.M2dError("resample_poly: overlapping rows in %s" % what)
        return ld

    def resample_poly(self, x, x0, taps, up, down, n0, ny, out=None):
        """Outputs [n0, n0 + ny) of the polyphase resampling by up / down of rows x (B, nx) that hold the samples with
        absolute indices [x0, x0 + nx) (zeros elsewhere) -> (B, ny); taps: odd-length fp32 filter (m2d_resample_poly:
        y[n] = sum_m taps[n down + half - m up] x[m], bit-identical however a track is cut into calls)"""
        ldx = self._chk_audio_rows(x, "x")
        dev = _chk(taps)
        if taps.dim() != 1 or taps.device != x.device:
            raise _lib.M2dError("resample_poly: taps must be a 1-D tensor on %s" % x.device)
        B, nx = x.shape
        ny = int(ny)
        if ny < 0:
            raise _lib.M2dError("resample_poly: ny < 0")
        o = torch.empty((B, ny), dtype=torch.float32, device=dev) if out is None else out
        ldy = self._chk_audio_rows(o, "out")
        if o.device != dev or tuple(o.shape) != (B, ny):
            raise _lib.M2dError("resample_poly: out must be a (%d, %d) tensor on %s" % (B, ny, dev))
        _launch("m2d_resample_poly", dev, _ptr(x), int(x0), nx, ldx, _ptr(taps), taps.numel(), int(up), int(down),
                _ptr(o), int(n0), ny, ldy, B)
        return o

    # ---------------------------------------------------------------- beat alignment (metrics.py)
    def stft_pack_basis(self, table):
        """table (2, n_fft / 2 + 1, n_fft) fp32, the windowed DFT basis made on the host -> the image m2d_stft_bands
        reads (m2d_stft_pack_basis); kept like the weight images inside a weight_cache() scope (metrics.stft_basis
        keeps one per (n_fft, device) besides)"""
        dev = _chk(table)
        n_fft = table.shape[-1] if table.dim() == 3 else 0
        elems = _lib.lib().m2d_stft_image_elems(int(n_fft))
        if elems == 0 or tuple(table.shape) != (2, n_fft // 2 + 1, n_fft):
            raise _lib.M2dError("stft_pack_basis: a (2, n_fft / 2 + 1, n_fft) table with n_fft a power of two in "
                                "[256, 2048] expected, got %s" % (tuple(table.shape),))

        def build():
            image = torch.empty((elems,), dtype=torch.float32, device=dev)
            _launch("m2d_stft_pack_basis", dev, _ptr(table), int(n_fft), _ptr(image))
            return image

        return self._image(table, "stft", build)

    def stft_bands(self, x, n_frames, hop, n_fft, image, bands, frame0=0):
        """Band energies E (B, n_frames, nb) of STFT frames frame0 .. of audio rows x (B, S) (rows may be cut from a
        wider buffer); image: stft_pack_basis's of this n_fft; bands (nb, n_fft / 2 + 1) fp32 (m2d_stft_bands)"""
        ldx = self._chk_audio_rows(x, "x")
        dev = _chk(image, bands)
        if dev != x.device:
            raise _lib.M2dError("stft_bands: the basis image and the bands must be on %s" % x.device)
        B, S = x.shape
        T, hop, n_fft = int(n_frames), int(hop), int(n_fft)
        if bands.dim() != 2 or n_fft < 2 or bands.shape[1] != n_fft // 2 + 1:
            raise _lib.M2dError("stft_bands: bands must be (nb, n_fft / 2 + 1), got %s" % (tuple(bands.shape),))
        if image.numel() != _lib.lib().m2d_stft_image_elems(n_fft):
            raise _lib.M2dError("stft_bands: n_fft must be a power of two in [256, 2048] and the image packed for it "
                                "(got n_fft = %d, an image of %d floats)" % (n_fft, image.numel()))
        nb = bands.shape[0]
        if T < 0 or B == 0:
            raise _lib.M2dError("stft_bands: n_frames < 0 or no rows")
        E = torch.empty((B, T, nb), dtype=torch.float32, device=dev)
        _launch("m2d_stft_bands", dev, _ptr(x), ldx, S, B, int(frame0), T, hop, n_fft, _ptr(image), _ptr(bands), nb,
                _ptr(E))
        return E

    def onset_flux(self, E, gamma=1.0):
        """E (B, T, nb) -> onset strength (B, T) (m2d_onset_flux)"""
        dev = _chk(E)
        if E.dim() != 3 or E.shape[0] == 0 or E.shape[2] == 0:
            raise _lib.M2dError("onset_flux: band energies (B, T, nb) expected, got %s" % (tuple(E.shape),))
        B, T, nb = E.shape
        o = torch.empty((B, T), dtype=torch.float32, device=dev)
        _launch("m2d_onset_flux", dev, _ptr(E), B, T, nb, float(gamma), _ptr(o))
        return o

    def motion_speed(self, poses):
        """poses (B, T, J, 3), T >= 2 -> mean joint speed (B, T) (m2d_motion_speed)"""
        dev = _chk(poses)
        if poses.dim() != 4 or poses.shape[3] != 3:
            raise _lib.M2dError("motion_speed: poses (B, T, J, 3) expected, got %s" % (tuple(poses.shape),))
        B, T, J, _ = poses.shape
        v = torch.empty((B, T), dtype=torch.float32, device=dev)
        _launch("m2d_motion_speed", dev, _ptr(poses), B, T, J, _ptr(v))
        return v

    def beat_align(self, onset, speed, sigma_onset=1.0, sigma_speed=2.0, sigma_align=2.0, return_events=False):
        """onset, speed (B, T) -> scores (B, 4) = [beat_align, beat_cover, |K|, |M|] (m2d_beat_align); with
        return_events also (motion events, music events (B, T) uint8, smoothed onset, smoothed speed (B, T))"""
        dev = _chk(onset, speed)
        if onset.dim() != 2 or onset.shape != speed.shape or onset.shape[0] == 0:
            raise _lib.M2dError("beat_align: onset and speed must both be (B, T), got %s and %s"
                                % (tuple(onset.shape), tuple(speed.shape)))
        B, T = onset.shape
        limit = _lib.lib().m2d_beat_align_max_frames()
        if T > limit:
            raise _lib.M2dError("beat_align: %d frames a row, the kernel takes at most %d (score the track in "
                                "sections)" % (T, limit))
        scores = torch.empty((B, 4), dtype=torch.float32, device=dev)
        extra = (None,) * 4
        if return_events:
            extra = (torch.empty((B, T), dtype=torch.uint8, device=dev), torch.empty((B, T), dtype=torch.uint8, device=dev),
                     torch.empty((B, T), dtype=torch.float32, device=dev),
                     torch.empty((B, T), dtype=torch.float32, device=dev))
        _launch("m2d_beat_align", dev, _ptr(onset), _ptr(speed), B, T, float(sigma_onset), float(sigma_speed),
                float(sigma_align), _ptr(scores), *[_ptr(t) for t in extra])
        return (scores,) + extra if return_events else scores

    def gauss_smooth(self, c, sigma):
        """c (B, T) -> g(c, sigma) (B, T): the smoothing of beat_align, bit-equal to its smoothed curves, for rows of
        any length (m2d_gauss_smooth)"""
        dev = _chk(c)
        if c.dim() != 2 or c.shape[0] == 0:
            raise _lib.M2dError("gauss_smooth: a curve (B, T) expected, got %s" % (tuple(c.shape),))
        B, T = c.shape
        out = torch.empty((B, T), dtype=torch.float32, device=dev)
        _launch("m2d_gauss_smooth", dev, _ptr(c), B, T, float(sigma), _ptr(out))
        return out

    def sync_scan_max_frames(self):
        return _lib.lib().m2d_sync_scan_max_frames()

    def sync_scan(self, a, b, factors, max_lag, min_overlap, na=None, nb=None):
        """a (B, Ta), b (B, Tb) fp32 curves (rows may be cut from wider buffers), na / nb optional int32 (B,) row
        lengths on the device -> (r (B, F, 2 max_lag + 1) fp64, n (same) int32): the Pearson correlation of a[j] with
        b at (j + l) / f for every factor f and lag l in [-max_lag, max_lag], and the number of pairs (m2d_sync_scan)"""
        dev, lda = self._rows2d("sync_scan", a)
        devb, ldb = self._rows2d("sync_scan", b)
        B, Ta = a.shape
        if devb != dev or b.shape[0] != B or B == 0:
            raise _lib.M2dError("sync_scan: a %s on %s and b %s on %s do not go together"
                                % (tuple(a.shape), dev, tuple(b.shape), devb))
        Tb = b.shape[1]
        limit = self.sync_scan_max_frames()
        if max(Ta, Tb) > limit:
            raise _lib.M2dError("sync_scan: %d frames a row, the kernel takes at most %d (scan the take in sections)"
                                % (max(Ta, Tb), limit))
        for name, t in (("na", na), ("nb", nb)):
            if t is not None and (not t.is_cuda or t.device != dev or t.dtype != torch.int32 or not t.is_contiguous()
                                  or tuple(t.shape) != (B,)):
                raise _lib.M2dError("sync_scan: %s must be a contiguous int32 tensor (%d,) on %s" % (name, B, dev))
        fac = [float(f) for f in factors]
        F, L = len(fac), int(max_lag)
        if F == 0 or L < 0:
            raise _lib.M2dError("sync_scan: at least one factor and max_lag >= 0 expected")
        r = torch.empty((B, F, 2 * L + 1), dtype=torch.float64, device=dev)
        n = torch.empty((B, F, 2 * L + 1), dtype=torch.int32, device=dev)
        _launch("m2d_sync_scan", dev, _ptr(a), lda, _ptr(na), _ptr(b), ldb, _ptr(nb), B, Ta, Tb,
                (ctypes.c_double * F)(*fac), F, L, int(min_overlap), _ptr(r), _ptr(n))
        return r, n

    # ---------------------------------------------------------------- distribution scores (metrics.py)
    @staticmethod
    def _chk64(what, *tensors):
        """contiguous fp64 tensors on one HIP device (the moments, matrices and scores of the distribution kernels)"""
        dev = None
        for t in tensors:
            if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise _lib.M2dError("%s: contiguous float64 tensors on a HIP device expected (got %s on %s)"
                                    % (what, t.dtype, t.device))
            if dev is not None and t.device != dev:
                raise _lib.M2dError("%s: tensors on different devices" % what)
            dev = t.device
        return dev

    @staticmethod
    def _rows2d(what, X):
        """X (N, D) fp32 on a HIP device, unit stride inside a row (a column block of a wider buffer is taken as it
        is) -> (device, row stride)"""
        if not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
            raise _lib.M2dError("%s: a 2-D fp32 tensor on a HIP device expected (got %s %s on %s)"
                                % (what, tuple(X.shape), X.dtype, X.device))
        if X.shape[1] > 0 and X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
            raise _lib.M2dError("%s: rows must be dense" % what)
        return X.device, (X.stride(0) if X.shape[0] > 1 else max(X.shape[1], 1))

    def sym_eig_max_dim(self):
        return _lib.lib().m2d_sym_eig_max_dim()

    def kinetic_features(self, poses, fps=25.0, up_axis=1):
        """poses (B, T, J, 3), T >= 3 -> F (B, 3 J): per joint the mean squared horizontal speed, the mean squared
        vertical speed and the mean absolute acceleration (m2d_kinetic_features)"""
        dev = _chk(poses)
        if poses.dim() != 4 or poses.shape[3] != 3 or poses.shape[0] == 0 or poses.shape[2] == 0:
            raise _lib.M2dError("kinetic_features: poses (B, T, J, 3) expected, got %s" % (tuple(poses.shape),))
        B, T, J, _ = poses.shape
        F = torch.empty((B, 3 * J), dtype=torch.float32, device=dev)
        _launch("m2d_kinetic_features", dev, _ptr(poses), B, T, J, float(fps), int(up_axis), _ptr(F))
        return F

    def feature_moments(self, X):
        """X (N, D) fp32, N >= 2, D <= sym_eig_max_dim() -> (mean (D), cov (D, D)) fp64, unbiased (m2d_feature_moments)"""
        dev, ldx = self._rows2d("feature_moments", X)
        N, D = X.shape
        mean = torch.empty((D,), dtype=torch.float64, device=dev)
        cov = torch.empty((D, D), dtype=torch.float64, device=dev)
        _launch("m2d_feature_moments", dev, _ptr(X), ldx, N, D, _ptr(mean), _ptr(cov))
        return mean, cov

    def sym_eig(self, A, vectors=False):
        """A (P, D, D) fp64 symmetric -> (w (P, D) ascending, V (P, D, D) with the eigenvectors as columns or None,
        info (P, 2) = [sweeps, converged]) (m2d_sym_eig)"""
        dev = self._chk64("sym_eig", A)
        if A.dim() != 3 or A.shape[1] != A.shape[2] or A.shape[0] == 0:
            raise _lib.M2dError("sym_eig: matrices (P, D, D) expected, got %s" % (tuple(A.shape),))
        P, D, _ = A.shape
        w = torch.empty((P, D), dtype=torch.float64, device=dev)
        V = torch.empty((P, D, D), dtype=torch.float64, device=dev) if vectors else None
        info = torch.empty((P, 2), dtype=torch.float64, device=dev)
        ws, nws = _workspace(dev, "m2d_sym_eig_workspace_bytes", P, D, int(bool(vectors)))
        _launch("m2d_sym_eig", dev, _ptr(A), P, D, _ptr(w), _ptr(V), _ptr(info), _ptr(ws), nws)
        return w, V, info

    def frechet(self, mean1, cov1, mean2, cov2):
        """P pairs of moments, mean (P, D) and cov (P, D, D) fp64 -> (P, 6) fp64 = [fd, |mean1 - mean2|^2,
        tr cov1 + tr cov2, tr (cov1 cov2)^1/2, sweeps, converged] (m2d_frechet)"""
        dev = self._chk64("frechet", mean1, cov1, mean2, cov2)
        if (mean1.dim() != 2 or mean1.shape[0] == 0 or mean2.shape != mean1.shape
                or tuple(cov1.shape) != tuple(mean1.shape) + (mean1.shape[1],) or cov2.shape != cov1.shape):
            raise _lib.M2dError("frechet: means (P, D) and covariances (P, D, D) expected, got %s %s %s %s"
                                % tuple(tuple(t.shape) for t in (mean1, cov1, mean2, cov2)))
        P, D = mean1.shape
        out = torch.empty((P, 6), dtype=torch.float64, device=dev)
        ws, nws = _workspace(dev, "m2d_frechet_workspace_bytes", P, min(D, self.sym_eig_max_dim()))
        _launch("m2d_frechet", dev, _ptr(mean1), _ptr(cov1), _ptr(mean2), _ptr(cov2), P, D, _ptr(out), _ptr(ws), nws)
        return out

    def pairwise_mean_dist(self, X, groups=1):
        """X (G K, D) fp32, G groups of K consecutive rows -> (G,) fp64: the mean Euclidean distance over the pairs of
        each group, NaN for K = 1 (m2d_pairwise_mean_dist)"""
        dev, ldx = self._rows2d("pairwise_mean_dist", X)
        G = int(groups)
        if G <= 0 or X.shape[0] == 0 or X.shape[0] % G:
            raise _lib.M2dError("pairwise_mean_dist: %d rows do not make %d groups" % (X.shape[0], G))
        K, D = X.shape[0] // G, X.shape[1]
        out = torch.empty((G,), dtype=torch.float64, device=dev)
        ws, nws = _workspace(dev, "m2d_pairwise_mean_dist_workspace_bytes", G, K)
        _launch("m2d_pairwise_mean_dist", dev, _ptr(X), ldx, G, K, D, _ptr(out), _ptr(ws), nws)
        return out

    # ---------------------------------------------------------------- nearest-neighbour queries (metrics.py)
    def knn_max_k(self):
        return _lib.lib().m2d_knn_max_k()

    def knn_radii(self, X, k):
        """X (N, D) fp32, N >= k + 1, 1 <= k <= knn_max_k() -> r2 (N,) fp32: the k-th smallest squared distance of
        each row to the other rows, the row itself excluded by index (m2d_knn_radii)"""
        dev, ldx = self._rows2d("knn_radii", X)
        N, D = X.shape
        r2 = torch.empty((N,), dtype=torch.float32, device=dev)
        ws, nws = _workspace(dev, "m2d_knn_radii_workspace_bytes", N, int(k))
        _launch("m2d_knn_radii", dev, _ptr(X), ldx, N, D, int(k), _ptr(r2), _ptr(ws), nws)
        return r2

    def ball_query(self, Q, P, r2=None):
        """Q (M, D), P (N, D) fp32, r2 (N,) fp32 or None -> (count (M,) int32 = #{i : d2(Q_j, P_i) <= r2[i]} or None,
        nn_d2 (M,) fp32 = min_i d2(Q_j, P_i), nn_idx (M,) int32 = the smallest index attaining it) (m2d_ball_query)"""
        dev, ldq = self._rows2d("ball_query", Q)
        devp, ldp = self._rows2d("ball_query", P)
        if devp != dev or Q.shape[1] != P.shape[1]:
            raise _lib.M2dError("ball_query: Q %s on %s and P %s on %s do not go together"
                                % (tuple(Q.shape), dev, tuple(P.shape), devp))
        M, D = Q.shape
        N = P.shape[0]
        if r2 is not None and (_chk(r2) != dev or tuple(r2.shape) != (N,)):
            raise _lib.M2dError("ball_query: r2 (%d,) on %s expected, got %s on %s" % (N, dev, tuple(r2.shape), r2.device))
        count = None if r2 is None else torch.empty((M,), dtype=torch.int32, device=dev)
        nn_d2 = torch.empty((M,), dtype=torch.float32, device=dev)
        nn_idx = torch.empty((M,), dtype=torch.int32, device=dev)
        ws, nws = _workspace(dev, "m2d_ball_query_workspace_bytes", M, N)
        _launch("m2d_ball_query", dev, _ptr(Q), ldq, M, _ptr(P), ldp, N, D, _ptr(r2), _ptr(count), _ptr(nn_d2),
                _ptr(nn_idx), _ptr(ws), nws)
        return count, nn_d2, nn_idx

    def dropout(self, x, mask, p_keep=0.5, scale=2.0, seed=None, offset=0, out=None):
        """y = x * keep * scale. seed None: keep from the uint8 `mask` (the caller's); else Philox4x32-10 bits of
        (seed, offset, index), written into `mask` when given. x None: the mask only. -> y (or mask)."""
        gen = seed is not None
        dev = _chk(x, out)
        if mask is not None:
            if mask.dtype != torch.uint8 or not mask.is_contiguous():
                raise _lib.M2dError("dropout: a contiguous uint8 mask expected")
            dev = dev or mask.device
            if x is not None and mask.numel() != x.numel():
                raise _lib.M2dError("dropout: mask and input differ in size")
        if not gen and mask is None:
            raise _lib.M2dError("dropout: a mask or a seed is needed")
        n = x.numel() if x is not None else mask.numel()
        y = (torch.empty_like(x) if out is None else out) if x is not None else None
        _launch("m2d_dropout", dev, _ptr(x), _ptr(y), _ptr(mask), n, float(p_keep), float(scale),
                int(seed or 0) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, int(gen))
        return y if x is not None else mask

    @staticmethod
    def _strided_mean(name, x, B, C, T, sb, sc, st):
        """A 0-dim mean over the (B, C, T) view, with element strides (sb, sc, st), of storage `x` (entry point `name`)"""
        dev = _chk(x)
        out = torch.empty((), dtype=torch.float32, device=dev)
        ws, nws = _workspace(dev, 'm2d_reduce_workspace_bytes')
        _launch(name, dev, _ptr(x), _ptr(out), B, C, T, sb, sc, st, _ptr(ws), nws)
        return out

    def tv_mean_fwd(self, x, B, C, T, sb, sc, st):
        """x: storage holding a (B, C, T) view with element strides (sb, sc, st)."""
        return self._strided_mean("m2d_tv_mean_fwd", x, B, C, T, sb, sc, st)

    def tv_mean_bwd(self, x, gout, B, C, T, sb, sc, st):
        dev = _chk(x, gout)
        dx = torch.empty_like(x)
        _launch("m2d_tv_mean_bwd", dev, _ptr(x), _ptr(gout), _ptr(dx), B, C, T, sb, sc, st)
        return dx

    # ---------------------------------------------------------------- evaluation metric, dataset scaling
    def jerk_mean_fwd(self, x, B, C, T, sb, sc, st):
        """jerkiness of the (B, C, T) view (element strides sb, sc, st) of storage `x` -> 0-dim."""
        return self._strided_mean("m2d_jerk_mean_fwd", x, B, C, T, sb, sc, st)

    def affine_cols(self, x, scale, shift, out=None):
        """x (..., cols) * scale[cols] + shift[cols] (MinMaxScaler transform / inverse); out may be x."""
        dev = _chk(x, scale, shift, out)
        cols = x.shape[-1]
        assert scale.numel() == cols and shift.numel() == cols
        y = torch.empty_like(x) if out is None else out
        _launch("m2d_affine_cols", dev, _ptr(x), _ptr(scale), _ptr(shift), _ptr(y), x.numel() // max(cols, 1), cols)
        return y

    # ---------------------------------------------------------------- U-Net resampling
    def maxpool2_fwd(self, x):
        """x: (B, C, L) dense, or a channel block of a wider buffer (samples x.stride(0) apart, dense inside)"""
        B, C, L = x.shape
        block = (not x.is_contiguous() and x.stride(2) == 1 and x.stride(1) == L and x.stride(0) > C * L and x.is_cuda
                 and x.dtype == torch.float32 and L % 2 == 0 and (C * L) % 8 == 0 and x.stride(0) % 4 == 0
                 and x.data_ptr() % 16 == 0)
        if block:
            dev = x.device
        else:
            x = x if x.is_contiguous() else x.contiguous()
            dev = _chk(x)
        y = torch.empty((B, C, L // 2), dtype=torch.float32, device=dev)
        if block:
            _launch("m2d_maxpool2_fwd_from", dev, _ptr(x), _ptr(y), B, C, L, x.stride(0))
        else:
            _launch("m2d_maxpool2_fwd", dev, _ptr(x), _ptr(y), B * C, L)
        return y

    def maxpool2_bwd(self, x, dy):
        dev = _chk(x, dy)
        B, C, L = x.shape
        dx = torch.empty_like(x)
        _launch("m2d_maxpool2_bwd", dev, _ptr(x), _ptr(dy), _ptr(dx), B * C, L)
        return dx

    def upsample2_fwd(self, x, out=None):
        dev = _chk(x)
        B, C, L = x.shape
        y, ypitch = self._out_block(out, (B, C, 2 * L), dev)
        _launch("m2d_upsample2_fwd_to", dev, _ptr(x), _ptr(y), B, C, L, ypitch)
        return y

    def upsample2_bwd(self, dy):
        dev = _chk(dy)
        B, C, Lo = dy.shape
        dx = torch.empty((B, C, Lo // 2), dtype=torch.float32, device=dev)
        _launch("m2d_upsample2_bwd", dev, _ptr(dy), _ptr(dx), B * C, Lo // 2)
        return dx

    # ---------------------------------------------------------------- profiler
    def prof_begin(self):
        _lib.check(_lib.lib().m2d_prof_begin(), "m2d_prof_begin")

    def prof_dump(self):
        """[(family, tag, d0, d1, d2, ms, flops, bytes)] per launch of the current profiling session."""
        cap = 1 << 22
        buf = ctypes.create_string_buffer(cap)
        n = _lib.lib().m2d_prof_dump(buf, cap)
        rows = []
        for line in buf.raw[:n].decode().splitlines():
            f = line.split(",")
            rows.append((int(f[0]), f[1], int(f[2]), int(f[3]), int(f[4]), float(f[5]), float(f[6]),
                         float(f[7]) if len(f) > 7 else 0.0))
        return rows

    def prof_end(self):
        buf = (ctypes.c_double * 20)()
        _lib.check(_lib.lib().m2d_prof_end(buf, 20), "m2d_prof_end")
        fams = ["gemm", "bn", "gru", "pointwise", "reduce"]
        return {f: {"ms": buf[4 * i], "launches": int(buf[4 * i + 1]), "flops": buf[4 * i + 2],
                    "bytes": buf[4 * i + 3]} for i, f in enumerate(fams)}


_impl = HipKernels()


def impl():
    return _impl


def set_impl(obj):
    """Test hook (tests/fake_backend.py installs a CPU stand-in to exercise host logic)."""
    global _impl
    prev = _impl
    _impl = obj
    return prev


# ---------------------------------------------------------------- the loaders' crop + augment gather (data.py)
# struct M2dAugmentRow of include/m2d.h, as the numpy record the host fills: one row of the batch
AUGMENT_ROW = np.dtype([("pose_start", "<i8"), ("pose_first", "<i8"), ("pose_last", "<i8"), ("audio_start", "<i8"),
                        ("audio_first", "<i8"), ("audio_last", "<i8"), ("a", "<i4"), ("b", "<i4"),
                        ("tap_offset", "<i4"), ("ntaps", "<i4"), ("mirror", "<i4"), ("cos_yaw", "<f4"),
                        ("sin_yaw", "<f4"), ("gain", "<f4")])
assert AUGMENT_ROW.itemsize == 80
AUGMENT_MAX_RATIO, AUGMENT_MAX_TAPS = 64, 1281


def crop_augment(poses, track, table, scale, shift, taps, T, S):
    """m2d_crop_augment: poses (frames, C) fp32 store, track (samples,) fp32 store or None (then S == 0), table: HOST
    numpy array of B AUGMENT_ROW records, scale / shift (C,), taps: the concatenated tap buffer (1-D; None without audio)
    -> (out_poses (B, T, C), out_audio (B, S) or None). The table's contents are checked HERE, before anything is
    uploaded or launched (the library sees only a device pointer): a reduced speed with terms in [1, 64], a window that
    lies inside its own take and a take that lies inside the store, odd tap counts inside the tap buffer, finite factors.
    A module function, not a HipKernels method: the loaders' host path never comes here (it runs data.augment_window), so
    the CPU stand-ins of the kernel layer have no counterpart of it."""
    name = "crop_augment"
    dev = _chk(poses, track, scale, shift, taps)
    T, S = int(T), int(S)
    if poses.dim() != 2 or poses.shape[0] < 1:
        raise _lib.M2dError("%s: the pose store must be a non-empty (frames, C) tensor" % name)
    frames, C = poses.shape
    if scale.numel() != C or shift.numel() != C:
        raise _lib.M2dError("%s: scale and shift must hold C = %d values" % (name, C))
    if not isinstance(table, np.ndarray) or table.dtype != AUGMENT_ROW or table.ndim != 1:
        raise _lib.M2dError("%s: the table must be a 1-D numpy array of kernels.AUGMENT_ROW records" % name)
    if S > 0 and (track is None or taps is None or track.dim() != 1 or taps.dim() != 1 or track.numel() < 1):
        raise _lib.M2dError("%s: S > 0 needs a 1-D track store and a 1-D tap buffer" % name)
    if S == 0:
        track = taps = None
    B = len(table)
    if B > 0 and T > 0:   # (B, T <= 0: the library refuses)
        a, b = table["a"].astype(np.int64), table["b"].astype(np.int64)
        if ((a < 1) | (b < 1) | (a > AUGMENT_MAX_RATIO) | (b > AUGMENT_MAX_RATIO)).any():
            raise _lib.M2dError("%s: a speed a / b needs 1 <= a, b <= %d" % (name, AUGMENT_MAX_RATIO))
        if any(math.gcd(int(x), int(y)) != 1 for x, y in zip(a, b)):
            raise _lib.M2dError("%s: a speed a / b must be reduced by its gcd" % name)
        need = -(-(T - 1) * a // b) + 1
        first, last, start = table["pose_first"], table["pose_last"], table["pose_start"]
        if ((first < 0) | (last >= frames) | (start < first) | (start + need - 1 > last)).any():
            raise _lib.M2dError("%s: a pose window leaves its take, or a take leaves the store of %d frames"
                                % (name, frames))
        if not (np.isfinite(table["cos_yaw"]) & np.isfinite(table["sin_yaw"]) & np.isfinite(table["gain"])).all():
            raise _lib.M2dError("%s: cos, sin and gain must be finite" % name)
        if S > 0:
            first, last, start = table["audio_first"], table["audio_last"], table["audio_start"]
            if ((first < 0) | (last >= track.numel()) | (start < first) | (start > last)).any():
                raise _lib.M2dError("%s: an audio window starts outside its take, or a take leaves the store of %d "
                                    "samples" % (name, track.numel()))
            off, nt = table["tap_offset"].astype(np.int64), table["ntaps"].astype(np.int64)
            resampled = a != b
            if (resampled & ((nt < 1) | (nt % 2 == 0) | (nt > AUGMENT_MAX_TAPS) | (off < 0)
                             | (off + nt > taps.numel()))).any():
                raise _lib.M2dError("%s: a row's taps must be an odd number <= %d inside the tap buffer of %d"
                                    % (name, AUGMENT_MAX_TAPS, taps.numel()))
    rows = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8)).to(dev) if B > 0 else None
    out = torch.empty((max(B, 0), max(T, 0), C), dtype=torch.float32, device=dev)
    audio = torch.empty((B, S), dtype=torch.float32, device=dev) if S > 0 else None
    _launch("m2d_crop_augment", dev, _ptr(poses), frames, C, _ptr(track), 0 if track is None else track.numel(),
            _ptr(rows), _ptr(scale), _ptr(shift), _ptr(taps), 0 if taps is None else taps.numel(), _ptr(out),
            _ptr(audio), B, T, S)
    return out, audio
