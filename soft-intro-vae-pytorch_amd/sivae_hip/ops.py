"""Tensor-level wrappers over the libsivae_hip C ABI (no autograd here — see `functional.py`).

Every function takes contiguous fp32 ROCm-device tensors, allocates the outputs, launches on torch's
current HIP stream and returns immediately (stream-async). CPU tensors are rejected loudly: the
product path has no CPU fallback.
"""
import collections
import ctypes
import functools
import os
import sys

import numpy as np
import torch

from . import lib as _lib

LRELU_SLOPE = 0.2
LOSS_TYPES = {"mse": 0, "l1": 1, "bce": 2}

_workspaces = {}


class KernelTimer:
    """Optional per-launch HIP-event timing of the MFMA conv kernels (used by bench.py for the roofline
    object).  Events are recorded on torch's current stream — the stream the kernels are launched on —
    and only read back after the timed region, so the instrumented run stays asynchronous."""

    def __init__(self):
        self.records = []  # (kernel_key, flops, start_event, end_event)

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, key, flops, start, executed=None):
        """flops: algorithmic FLOPs of the reference op; executed: FLOPs the kernel actually issues to the matrix
        pipe when that differs (Winograd)."""
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.append((key, flops, start, ev, flops if executed is None else executed))

    def summary(self):
        """-> {kernel_key: dict(launches, total_ms, avg_ms, flops)} (call after torch.cuda.synchronize())"""
        out = {}
        for key, flops, s, e, ex in self.records:
            d = out.setdefault(key, dict(launches=0, total_ms=0.0, flops=0.0, executed_flops=0.0))
            d["launches"] += 1
            d["total_ms"] += s.elapsed_time(e)
            d["flops"] += flops
            d["executed_flops"] += ex
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / max(d["launches"], 1)
        return out


TIMER = None  # set to a KernelTimer() to instrument conv2d_fwd / conv2d_wgrad launches


def timer_begin():
    """start event of an instrumented launch, or None (no timer installed: the only cost of an untimed launch)"""
    return TIMER.begin() if TIMER is not None else None


def timer_end(t0, key, flops, ratio=None):
    """close the record `timer_begin` opened (call it under `if t0 is not None`); ratio = (numerator, denominator) of
    executed over algorithmic FLOPs where they differ"""
    TIMER.end(key, flops, t0, executed=None if ratio is None else flops * ratio[0] / ratio[1])


def u8_to_f32(src, flip=None, nhwc=False, scale=1.0 / 255.0):
    """uint8 image batch (NCHW, or NHWC with nhwc=True) -> fp32 NCHW * scale; flip: int32 [B], nonzero = mirror."""
    if not src.is_cuda or src.dtype != torch.uint8 or not src.is_contiguous() or src.dim() != 4:
        raise TypeError("sivae_hip.u8_to_f32: expected a contiguous 4-D uint8 ROCm tensor")
    if nhwc:
        B, H, W, C = src.shape
    else:
        B, C, H, W = src.shape
    if flip is not None and (not flip.is_cuda or flip.dtype != torch.int32 or flip.numel() != B):
        raise TypeError("sivae_hip.u8_to_f32: flip must be an int32 ROCm tensor with one entry per sample")
    dst = torch.empty((B, C, H, W), dtype=torch.float32, device=src.device)
    _lib.call("sivae_u8_to_f32", _p(src), _p(dst), _p(flip), B, C, H, W, int(bool(nhwc)), float(scale), _s())
    return dst


def f32_to_u8(src, scale=255.0):
    """fp32 images -> uint8 the way the reference quantises generated batches (clip(x*255, 0, 255) truncated)"""
    if not src.is_cuda or src.dtype != torch.float32 or not src.is_contiguous():
        raise TypeError("sivae_hip.f32_to_u8: expected a contiguous float32 ROCm tensor")
    dst = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    _lib.call("sivae_f32_to_u8", _p(src), _p(dst), src.numel(), float(scale), _s())
    return dst


def _require(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("sivae_hip: tensor is on %s — the Soft-IntroVAE HIP kernels need a ROCm device "
                               "tensor and have no CPU fallback" % t.device)
        if t.dtype != torch.float32 and t.dtype != torch.int64:
            raise TypeError("sivae_hip: expected float32, got %s" % t.dtype)
        if not t.is_contiguous():
            raise ValueError("sivae_hip: tensor must be contiguous")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s(t=None):
    """HIP stream the launch goes to: torch's current stream of the TENSOR's device (the drop-in entry points also
    make that device current, so legacy `_s()` calls agree with it)"""
    return ctypes.c_void_p(torch.cuda.current_stream(None if t is None else t.device).cuda_stream)


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream); kernels on one stream are ordered, so sharing is safe."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


_counters = {}
# SIVAE_BN_FUSED_FINALIZE=1: the per-channel finalize of the BatchNorm backward runs in the last block of the reduction
# kernel (agent-scope fence + counter) instead of as its own ~5 us launch.  Measured a LOSS (round 3, one call, 256x256):
# 16-image shard 213.9 vs 227.3 img/s, bootstrap 8-image shard 196.4 vs 215.0 — the release fence every block needs
# (buffer_wbl2 + buffer_inv at agent scope: the 8 XCD L2s are not coherent inside a kernel) costs far more than the
# ~110 launches it removes -> off by default.
BN_FUSED_FINALIZE = os.environ.get("SIVAE_BN_FUSED_FINALIZE", "0") == "1"


def counters(device):
    """8192 zero-initialised unsigned ints per (device, stream) for kernels that finish a reduction in their last block
    (each such kernel leaves them zero)"""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _counters.get(key)
    if buf is None:
        buf = torch.zeros(8192, dtype=torch.int32, device=device)
        _counters[key] = buf
    return buf


# SIVAE_BN_FUSED=0: the three-launch BatchNorm backward (reduce / finalize / dx: two reads of dy and x) instead of the
# one-pass persistent kernel of bn_fused.hip (one read, activations held in registers across a grid barrier).  The
# persistent kernel needs its whole grid resident — two PROCESSES sharing one GPU (the 2-rank same-device tests) must
# switch it off; one process per GPU (the deployment) is fine.
BN_FUSED = os.environ.get("SIVAE_BN_FUSED", "1") != "0"
_bn_states = {}


def bn_fused_state(device):
    """barrier / counter state of sivae_bn_bwd_fused per (device, stream): zeroed once, left consistent by every call"""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _bn_states.get(key)
    if buf is None:
        buf = torch.zeros(_lib.load().sivae_bn_bwd_fused_state_uints(), dtype=torch.int32, device=device)
        _bn_states[key] = buf
    return buf


BN_FUSED_POISON_MSG = ("sivae_hip: a one-pass BatchNorm backward (sivae_bn_bwd_fused) gave up at its grid barrier on "
                       "device/stream %s: its grid was not fully resident (another persistent kernel or process on "
                       "the GPU, or a CU mask).  The iteration's gradients are invalid.  Set SIVAE_BN_FUSED=0 (the "
                       "three-launch form) or SIVAE_BN_FUSED_PERSISTENT=0 for this deployment.")


def bn_fused_poisoned():
    """The non-raising form of `bn_fused_check`: None, or the message to raise with.  Data-parallel callers fold the
    answer into a collective flag first (sivae_hip.dp.any_rank) so that every rank raises together — a rank raising alone
    leaves the others waiting in the next all-reduce."""
    if not _bn_states:
        return None
    w = _lib.load().sivae_bn_bwd_fused_poison_word()
    bad = [k for k, buf in _bn_states.items() if int(buf[w].item()) != 0]
    if not bad:
        return None
    for k in bad:
        _bn_states[k].zero_()
    return BN_FUSED_POISON_MSG % (bad,)


def bn_fused_check():
    """Was a persistent BatchNorm-backward launch abandoned (its grid barrier timed out because the grid was not fully
    resident — another persistent kernel, a CU mask the runtime does not report)?  Reads one word per barrier state (a
    device->host copy: call it where results are read back anyway — the training loops do, once per logging interval);
    if set: zeroes the state (the counters of an abandoned launch are inconsistent) and raises.  The outputs of the
    abandoned launch and of everything after it are garbage."""
    msg = bn_fused_poisoned()
    if msg is not None:
        raise RuntimeError(msg)


def _out(out, shape, device):
    """a caller-provided destination (a contiguous fp32 device tensor of exactly `shape`: the parameter-gradient slab
    views of optim.FlatAdam) or a fresh tensor"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if (tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous()
            or out.device != device):
        raise ValueError("sivae_hip: out must be a contiguous float32 tensor of shape %s on %s" % (tuple(shape), device))
    return out


def _pg(pg_out, C, device, want):
    """(dgamma, dbeta) destinations of a BatchNorm backward"""
    if not want:
        return None, None
    if pg_out is not None:
        return _out(pg_out[0], (C,), device), _out(pg_out[1], (C,), device)
    return (torch.empty(C, dtype=torch.float32, device=device), torch.empty(C, dtype=torch.float32, device=device))


# ------------------------------------------------------------------------------------------------ conv
def pack_weight(w, mode):
    """w [Co, Ci, k, k] (or [out, in] for Linear) -> packed GEMM operand. mode 0 fwd, 1 dgrad."""
    _require(w)
    if w.dim() == 2:
        Co, Ci, ks = w.shape[0], w.shape[1], 1
    else:
        Co, Ci, ks = w.shape[0], w.shape[1], w.shape[2]
    L = _lib.load()
    nbytes = L.sivae_pack_conv_weight_bytes(Co, Ci, ks, mode)
    if nbytes == 0:
        raise _lib.SivaeError("sivae_pack_conv_weight_bytes", -3)
    wp = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _lib.call("sivae_pack_conv_weight", _p(w), _p(wp), Co, Ci, ks, mode, _s())
    return wp


def pack_wino(w, mode):
    """w [Co, Ci, 3, 3] -> Winograd F(2x2,3x3) filter transform U = G g G^T, packed [j][ci][co][i]."""
    _require(w)
    Co, Ci = w.shape[0], w.shape[1]
    assert w.dim() == 4 and w.shape[2] == 3 and w.shape[3] == 3
    nbytes = _lib.load().sivae_pack_wino_weight_bytes(Co, Ci, mode)
    if nbytes == 0:
        raise _lib.SivaeError("sivae_pack_wino_weight_bytes", -3)
    up = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _lib.call("sivae_pack_wino_weight", _p(w), _p(up), Co, Ci, mode, _s())
    return up


# SIVAE_WINO=0 keeps every 3x3 conv on the direct implicit-GEMM kernel (A/B measurements, debugging)
WINO = os.environ.get("SIVAE_WINO", "1") != "0"
WINO_UP = os.environ.get("SIVAE_WINO_UP", "1") != "0"  # phase-decomposed F(2x2,2x2) kernel for conv-after-upsample
WINO_WGRAD = os.environ.get("SIVAE_WINO_WGRAD", os.environ.get("SIVAE_WINO", "1")) != "0"
# Winograd F(4x4,3x3) for the large-map 3x3 convs without a fused prologue (SIVAE_WINO4=0: F(2x2,3x3) everywhere);
# SIVAE_WINO4_MAXC: largest channel count it takes (its U slab per 64-channel tile is 2.25x the F(2x2,3x3) one)
WINO4 = os.environ.get("SIVAE_WINO4", "1") != "0"
WINO4_MAXC = int(os.environ.get("SIVAE_WINO4_MAXC", "512"))
# SIVAE_WINO4_B6: the F(4x4,3x3) forward / data gradient on the bf16 matrix pipe with fp32-exact products (six bf16 MFMAs
# per fp32 product, conv_wino4_b6.hip) for layers with at least SIVAE_WINO4_B6_MINC input channels; 0: the fp32-MFMA kernel
WINO4_B6 = os.environ.get("SIVAE_WINO4_B6", "0") != "0"
WINO4_B6_MINC = int(os.environ.get("SIVAE_WINO4_B6_MINC", "16"))
WINO4_B6_PRO = os.environ.get("SIVAE_WINO4_B6_PRO", "1") != "0"
# F(4x4,3x3) weight gradient (conv_wino4_wgrad.hip); SIVAE_WINO4_WGRAD=0: the F(2x2,3x3) one everywhere
WINO4_WGRAD = WINO4 and os.environ.get("SIVAE_WINO4_WGRAD", "1") != "0"
# SIVAE_WINO4_FORCE=1: take the F(4x4,3x3) kernels wherever they are SUPPORTED, not only where they pay (tests: the
# oracle comparisons run at batch 2-4, below the work-item thresholds)
WINO4_FORCE = os.environ.get("SIVAE_WINO4_FORCE", "0") == "1"
# SIVAE_WINO4_SPLITK=0: no split-K form of the F(4x4,3x3) kernel (launches below one work item per CU stay on F(2x2,3x3))
WINO4_SPLITK = os.environ.get("SIVAE_WINO4_SPLITK", "1") != "0"
# SIVAE_WINO4_SMALL=0: 8x8 / 4x4 maps stay on F(2x2,3x3) (the F(4x4,3x3) kernel runs them as grids of 8 / 32 images per item)
WINO4_SMALL = os.environ.get("SIVAE_WINO4_SMALL", "1") != "0"
WINO4_SMALL_FORCE = os.environ.get("SIVAE_WINO4_SMALL_FORCE", "0") == "1"  # (tests / tools: wherever it is supported)
# SIVAE_WINO4_UP_SMALL=0: convs of an upsampled input on 16x16 / 8x8 output maps stay on F(2x2,3x3) with upsample addressing
WINO4_UP_SMALL = os.environ.get("SIVAE_WINO4_UP_SMALL", "1") != "0"
# SIVAE_WINO4_DGRAD_POOL=0: the data gradient of an upsample-conv with <= 64 input channels stays on conv_wino_up_dgrad.hip
WINO4_DGRAD_POOL = os.environ.get("SIVAE_WINO4_DGRAD_POOL", "1") != "0"
WINO4_PRO = os.environ.get("SIVAE_WINO4_PRO", "1") != "0"  # ... also with a fused BatchNorm prologue (conv2 forward)
# SIVAE_FUSE_BN_BWD=1: reduce BatchNorm-1's backward sums in the epilogue of conv2's data gradient.  Measured a LOSS at
# 256x256 bs128 (593 vs 585 ms per iteration: the extra tensor read sits on the kernel's critical path and disables its
# next-item prefetch, which costs more than the 14 ms reduction pass it removes) -> off by default.
FUSE_BN_BWD = os.environ.get("SIVAE_FUSE_BN_BWD", "0") == "1"
# streaming kernel for the 1x1 convs (SIVAE_CONV1_STREAM=0: the LDS-tiled direct kernel)
CONV1_STREAM = os.environ.get("SIVAE_CONV1_STREAM", "1") != "0"
# merged-contraction kernel for the 5x5 convs from <= 3 into <= 64 channels (SIVAE_CONV5_K75=0: the direct kernel)
CONV5_K75 = os.environ.get("SIVAE_CONV5_K75", "1") != "0"
# 1-bit LeakyReLU sign mask written by the block's last BatchNorm pass and read by its backward instead of the saved
# output (SIVAE_SIGNMASK=0: the backward reads the output tensor again)
SIGNMASK = os.environ.get("SIVAE_SIGNMASK", "1") != "0"


class PackedW:
    """Both GEMM-operand forms of one weight tensor (direct pack; Winograd transform for 3x3), built lazily.
    conv2d_fwd picks the kernel per call from the feature-map size."""

    def __init__(self, w, mode):
        self.w, self.mode = w, mode
        self._direct = self._wino = None

    def direct(self):
        if self._direct is None:
            self._direct = pack_weight(self.w, self.mode)
        return self._direct

    # operand forms sivae_pack_batch rebuilds in place: (form id of include/sivae_hip.h, attribute holding the buffer)
    _BATCH_FORMS = ((0, "_direct"), (1, "_wino"), (2, "_wino4"), (3, "_wino_up"), (4, "_wino_up_dgrad"),
                    (5, "_wino4_b6"))

    def batch_forms(self):
        """[(form id, buffer)] of the operand forms built so far that the batched repack can rebuild in place"""
        return [(f, getattr(self, a)) for f, a in self._BATCH_FORMS if getattr(self, a, None) is not None]

    def refreshed(self):
        """the weight changed and the batched repack rebuilt the forms of batch_forms() in place: drop the others (they
        are rebuilt on demand)"""
        self._k75 = None

    def wino(self):
        if self._wino is None:
            self._wino = pack_wino(self.w, self.mode)
        return self._wino

    def wino4(self):
        """F(4x4,3x3) filter transform [6][Ci_pad][Co_pad][6] (conv_wino4.hip)"""
        if getattr(self, "_wino4", None) is None:
            w = self.w
            Co, Ci = w.shape[0], w.shape[1]
            nbytes = _lib.load().sivae_pack_wino4_weight_bytes(Co, Ci, self.mode)
            up = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            _lib.call("sivae_pack_wino4_weight", _p(w), _p(up), Co, Ci, self.mode, _s(w))
            self._wino4 = up
        return self._wino4

    def wino4_b6(self):
        """the F(4x4,3x3) filter transform pre-split into three bf16 pieces, MFMA-ready (conv_wino4_b6.hip)"""
        if getattr(self, "_wino4_b6", None) is None:
            w = self.w
            Co, Ci = w.shape[0], w.shape[1]
            nbytes = _lib.load().sivae_pack_wino4_b6_weight_bytes(Co, Ci, self.mode)
            up = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            _lib.call("sivae_pack_wino4_b6_weight", _p(w), _p(up), Co, Ci, self.mode, _s(w))
            self._wino4_b6 = up
        return self._wino4_b6

    def wino_up_dgrad(self):
        if getattr(self, "_wino_up_dgrad", None) is None:
            assert self.mode == 0
            w = self.w
            Co, Ci = w.shape[0], w.shape[1]
            nbytes = _lib.load().sivae_pack_wino_up_dgrad_weight_bytes(Co, Ci)
            ud = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            _lib.call("sivae_pack_wino_up_dgrad_weight", _p(w), _p(ud), Co, Ci, _s())
            self._wino_up_dgrad = ud
        return self._wino_up_dgrad

    def k75(self):
        """merged-contraction operand [76][64] of a 5x5 conv from <= 3 into <= 64 channels (conv5_k75.hip); mode 0:
        forward of w [Cb][Cs][5][5], mode 1: data gradient of w [Cs][Cb][5][5]"""
        if getattr(self, "_k75", None) is None:
            w = self.w
            n_big, n_small = (w.shape[0], w.shape[1]) if self.mode == 0 else (w.shape[1], w.shape[0])
            wq = torch.empty(_lib.load().sivae_pack_conv5_k75_bytes() // 4, dtype=torch.float32, device=w.device)
            _lib.call("sivae_pack_conv5_k75", _p(w), _p(wq), n_small, n_big, self.mode, _s(w))
            self._k75 = wq
        return self._k75

    def wino_up(self):
        """phase-decomposed F(2x2,2x2) transform for the conv-after-upsample forward kernel (mode 0 only)"""
        if getattr(self, "_wino_up", None) is None:
            assert self.mode == 0
            w = self.w
            Co, Ci = w.shape[0], w.shape[1]
            nbytes = _lib.load().sivae_pack_wino_up_weight_bytes(Co, Ci)
            up = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            _lib.call("sivae_pack_wino_up_weight", _p(w), _p(up), Co, Ci, _s())
            self._wino_up = up
        return self._wino_up


def space_to_depth2(x):
    """[B, C, 2Hs, 2Ws] -> parity planes [B, 4, C, Hs, Ws] (plane 2p+q = x[..., p::2, q::2])"""
    _require(x)
    B, C, H, W = x.shape
    out = torch.empty((B, 4, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    _lib.call("sivae_space_to_depth2", _p(x), _p(out), B, C, H // 2, W // 2, _s())
    return out


# ------------------------------------------------------------------------------------------------ routes
# WHICH kernel a convolution or BatchNorm backward gets is decided here, from integers and flags alone: the module
# switches above (read at call time) and library predicates, which need no device.  The launch functions below only
# allocate and marshal what the route names.  tests/test_conv_routes_host.py holds the routes of the benchmarked
# networks to a recording of the previous dispatch; a new kernel path is a new Route value here and nothing else.
#   family       kernel family (k75 / stream1x1 / wino4 / wino4_splitk / wino4_b6 / wino_up / wino / wino_splitk / direct ...)
#   entry        the C entry point
#   operand      the PackedW method that builds the weight operand (None: the caller's direct pack, or no weight)
#   args         which optional arguments `entry` takes (_conv_call)
#   materialise  the upsampled input (BatchNorm: the pooled dy) is expanded by a launch of its own first
#   split        split-K factor
#   stats_rows   rows of the BatchNorm statistics partials the epilogue writes (asked for with want_stats only)
#   ws_bytes     scratch the entry point needs
#   key, ratio   KernelTimer key (the kernel rocprofv3 names) and executed / algorithmic FLOPs as (numerator, denominator)
#   error        (exception type, message) of a combination that is refused
Route = collections.namedtuple("Route", "family entry operand args materialise split stats_rows ws_bytes key ratio error",
                               defaults=(None, "", False, 1, 0, 0, None, None, None))
_F44, _F22, _F22_UP = (36.0, 144.0), (16.0, 36.0), (9.0, 36.0)  # multiplies per output: F(4x4,3x3), F(2x2,3x3), F(2x2,2x2)
_routes = {}


def _memo(route_fn):
    """A conv route depends on its arguments, the module switches and library predicates that are fixed for the process:
    computed once per layer shape (four predicate calls and a key string, about 4 us, on every launch otherwise — the
    small-batch iterations are bound by host time per launch).  `_SwitchWatch` below empties the memo whenever an
    attribute of this module is assigned, which is how tests and tools flip switches."""
    @functools.wraps(route_fn)
    def cached(*sizes, **flags):
        k = (route_fn, sizes, tuple(flags.items()))
        r = _routes.get(k)
        if r is None:
            r = _routes[k] = route_fn(*sizes, **flags)
        return r
    return cached


def _tf(flag):
    return "true" if flag else "false"


def conv_fwd_kernel_key(ks, Co, pro):
    """name of the template instantiation sivae_conv2d_fwd dispatches to (mirrors conv_fwd.hip)"""
    tile = {3: ("1,2,1,4,8,3", "2,2,1,4,2,3", "2,2,2,2,2,2"), 1: ("1,2,1,4,32,1", "2,2,1,4,16,1", "2,2,2,2,16,1"),
            5: ("1,2,1,4,4,4", "2,2,1,4,4,4", "2,2,2,2,4,3")}[ks][0 if Co <= 32 else (1 if Co <= 64 else 2)]
    return "conv_fwd_kernel<%d,%s,%s>" % (ks, tile, _tf(pro))


def conv_wgrad_kernel_key(ks, Co, pro):
    tile = {3: "3,1,1,2,2,3", 1: "1,2,2,2,2,1",
            5: ("1,1,1,1,2,2" if Co <= 32 else "1,1,1,2,1,2")}[ks]
    return "conv_wgrad_kernel<%d,%s,%s>" % (ks, tile, _tf(pro))


def _wino_key(W, pro):
    return "conv_wino_kernel<%s,%s>" % ("1,4" if W >= 32 else ("2,3" if W >= 16 else ("2,2" if W == 8 else "1,1")), _tf(pro))


def _w4_key(b6, pro, sup):
    """conv_wino4_kernel<PRO>, or conv_wino4_grid_kernel<PRO> on 8x8 / 4x4 maps"""
    return ("conv_wino4_b6_kernel<%s>" if b6 else
            ("conv_wino4_grid_kernel<%s>" if sup >= 3 else "conv_wino4_kernel<%s>")) % _tf(pro)


def wino4_b6_takes(Ci, pro):
    return WINO4_B6 and Ci >= WINO4_B6_MINC and (not pro or WINO4_B6_PRO)


@_memo
def conv2d_fwd_route(B, Ci, Co, H, W, ks, *, packed=True, mode=0, bias=False, pro=False, upsample=False,
                     want_stats=False, has_out=False, accumulate=False, nseg=1):
    """route of conv2d_fwd for a [B, Ci] input and a [B, Co, H, W] OUTPUT map (packed: wp is a PackedW of that mode)"""
    L = _lib.load()
    if (CONV5_K75 and ks == 5 and packed and not pro and not upsample and not accumulate and not has_out
            and L.sivae_conv5_k75_supported(Ci, Co) == 1):
        # the encoder stem / the data gradient of Decoder.predict: whole contraction (K = 75) merged; 64 output rows x 76
        # contraction columns are issued
        return Route("k75", "sivae_conv5_k75_fwd", "k75", "bS", key="conv5_k75_kernel", ratio=(64.0 * 76, Co * Ci * 25.0),
                     stats_rows=L.sivae_conv5_k75_num_px_tiles(B, H, W) if want_stats else 0)
    if (CONV1_STREAM and ks == 1 and not bias and not pro and not upsample and not want_stats
            and L.sivae_conv1x1_stream_supported(B, Ci, Co, H * W) == 1):
        # ResidualBlock.conv_expand (forward / data gradient): x streamed straight into the MFMA operand
        return Route("stream1x1", "sivae_conv1x1_stream", "direct" if packed else None, "fa", key="conv1x1_stream_kernel")
    sup = L.sivae_conv2d_wino4_supported(H, W) if (WINO and WINO4) else 0
    if sup > 2 and not (WINO4_SMALL and (WINO4_SMALL_FORCE or L.sivae_conv2d_wino4_small_pays(B, Ci, Co, H, W) == 1)):
        sup = 0  # (8x8 / 4x4 maps: only where the image-grid launch beats F(2x2,3x3) — few items or short K slices do not)
    # an upsampled input: the phase-form kernels (conv_wino_up.hip) cover the maps from 32x32 up; on the 16x16 / 8x8 outputs
    # of the deep decoder blocks (Decoder res_in_16 / res_in_8, train_soft_intro_vae.py:153-158) the upsampled tensor is a
    # few MB — materialise it (one small launch) and take the F(4x4,3x3) image-grid kernel instead of F(2x2,3x3)
    if (sup and ks == 3 and not bias and packed and 16 <= Ci and max(Ci, Co) <= WINO4_MAXC
            and (not upsample or (sup >= 2 and WINO4_UP_SMALL and not pro))
            # (maps up to 16x16: whole image grids per work item, inside one segment)
            and (B // nseg) % L.sivae_conv2d_wino4_images_per_item(H, W) == 0
            and (not pro or (WINO4_PRO and nseg * ((Ci + 31) // 32) * 32 <= 1024))):
        pays = L.sivae_conv2d_wino4_pays(B, Ci, Co, H, W) == 1
        # fewer work items than CUs (the deep layers of a per-GPU shard): split over K when that fills the chip
        S = L.sivae_conv2d_wino4_splitk(B, Ci, Co, H, W) if (WINO4_SPLITK and not pays) else 1
        b6 = wino4_b6_takes(Ci, pro) and sup <= 2
        if S > 1:
            return Route("wino4_splitk", "sivae_conv2d_wino4_b6_fwd_splitk" if b6 else "sivae_conv2d_wino4_fwd_splitk",
                         "wino4_b6" if b6 else "wino4", "PSagw", upsample, S, B if want_stats else 0,  # (rows per image)
                         L.sivae_conv2d_wino4_splitk_workspace_bytes(B, Ci, Co, H, W), _w4_key(b6, pro, sup), _F44)
        if pays or WINO4_FORCE:
            # large maps: F(4x4,3x3) — 2.25 multiplies per output pixel instead of 4
            entry, args = (("sivae_conv2d_wino4_b6_fwd", "PSag") if b6 else
                           (("sivae_conv2d_wino4_fwd_pro", "PSag") if pro else ("sivae_conv2d_wino4_fwd", "Sa")))
            return Route("wino4_b6" if b6 else "wino4", entry, "wino4_b6" if b6 else "wino4", args, upsample,
                         stats_rows=L.sivae_conv2d_wino4_num_px_tiles(B, H, W) if want_stats else 0,
                         key=_w4_key(b6, pro, sup), ratio=_F44)
    wino = WINO and ks == 3 and not bias and packed and L.sivae_conv2d_wino_supported(H, W) == 1
    if nseg > 1 and (pro or want_stats) and not wino:
        return Route("direct", "sivae_conv2d_fwd", error=(
            ValueError, "sivae_hip: a segmented batch needs the Winograd 3x3 kernels for fused BatchNorm work"))
    if wino and WINO_UP and upsample and not accumulate and mode == 0 and L.sivae_conv2d_wino_up_supported(H, W) == 1:
        if nseg > 1 and pro:
            return Route("wino_up", "sivae_conv2d_wino_up_fwd", error=(
                ValueError, "sivae_hip: no segmented prologue in the upsample-phase kernel"))
        return Route("wino_up", "sivae_conv2d_wino_up_fwd", "wino_up", "PS", ratio=_F22_UP,
                     key="conv_wino_up_kernel<%s,%s>" % ("1,4" if W >= 64 else "2,3", _tf(pro)),
                     stats_rows=L.sivae_conv2d_wino_up_num_px_tiles(B, H, W) if want_stats else 0)
    if wino:
        # split-K for launches that would leave most of the chip idle (deep small maps at small batch)
        S = L.sivae_conv2d_wino_splitk(B, Ci, Co, H, W)
        seg = "_seg" if nseg > 1 else ""
        if S > 1:
            return Route("wino_splitk", "sivae_conv2d_wino_fwd_splitk" + seg, "wino", "PSuagw" if seg else "PSuaw", split=S,
                         stats_rows=L.sivae_conv2d_wino_splitk_stats_rows(B, Ci, Co, H, W) if want_stats else 0,
                         ws_bytes=L.sivae_conv2d_wino_splitk_workspace_bytes(B, Ci, Co, H, W), key=_wino_key(W, pro),
                         ratio=_F22)
        return Route("wino", "sivae_conv2d_wino_fwd" + seg, "wino", "PSuag" if seg else "bPSua", key=_wino_key(W, pro),
                     ratio=_F22, stats_rows=L.sivae_conv2d_wino_num_px_tiles(B, H, W) if want_stats else 0)
    return Route("direct", "sivae_conv2d_fwd", "direct" if packed else None, "bPSkua", key=conv_fwd_kernel_key(ks, Co, pro),
                 stats_rows=L.sivae_conv2d_fwd_num_px_tiles(B, Co, H, W) if want_stats else 0)


@_memo
def conv2d_wgrad_route(B, Ci, Co, H, W, ks, *, pro=False, upsample=False, nseg=1):
    """route of conv2d_wgrad for dy [B, Co, H, W] (x at half resolution with upsample)"""
    L = _lib.load()
    if (WINO_WGRAD and WINO_UP and upsample and ks == 3 and not pro
            and L.sivae_conv2d_wino_up_wgrad_supported(H // 2, W // 2) == 1):
        # conv after nearest-2x upsample: phase-form F(2x2,2x2) weight gradient on the low-resolution x
        return Route("wino_up_wgrad", "sivae_conv2d_wino_up_wgrad", None, "hw", key="wino_up_wgrad_kernel", ratio=_F22_UP,
                     ws_bytes=L.sivae_conv2d_wino_up_wgrad_workspace_bytes(B, Ci, Co, H // 2, W // 2))
    ips = L.sivae_conv2d_wino4_wgrad_images_per_stage(H, W) if ks == 3 else 0  # (8x8 / 4x4 maps: 2 / 4 images per strip)
    # (an upsampled x on the 16x16 / 8x8 maps, which the phase-form weight gradient above does not take: materialised, as
    # in conv2d_fwd_route)
    if (WINO4_WGRAD and WINO_WGRAD and ks == 3 and (not pro or nseg <= 2)
            and (not upsample or (WINO4_UP_SMALL and not pro and H <= 16 and W <= 16))
            and max(Ci, Co) <= WINO4_MAXC and ips > 0 and (B // nseg) % ips == 0 and (ips == 1 or WINO4_SMALL)
            and (L.sivae_conv2d_wino4_wgrad_pays(B, Ci, Co, H, W) == 1 or (WINO4_FORCE and min(Ci, Co) >= 16))):
        # Winograd F(4x4,3x3) weight gradient (conv_wino4_wgrad.hip): 36 instead of 64 multiplies per tile, co, ci
        return Route("wino4_wgrad", "sivae_conv2d_wino4_wgrad", None, "Pgw", upsample, ratio=_F44,
                     ws_bytes=L.sivae_conv2d_wino4_wgrad_workspace_bytes(B, Ci, Co, H, W),
                     key="wino4_wgrad_kernel<%s,%s>" % (_tf(pro), _tf(ips > 1)))
    if WINO_WGRAD and ks == 3 and L.sivae_conv2d_wino_wgrad_supported(H, W) == 1:
        seg = nseg > 1 and pro
        return Route("wino_wgrad", "sivae_conv2d_wino_wgrad_seg" if seg else "sivae_conv2d_wino_wgrad", None,
                     "Pugw" if seg else "Puw", ws_bytes=L.sivae_conv2d_wino_wgrad_workspace_bytes(B, Ci, Co, H, W),
                     key="wino_wgrad_kernel<%s,1>" % _tf(pro), ratio=_F22)
    if nseg > 1 and pro:
        return Route("direct_wgrad", "sivae_conv2d_wgrad", error=(
            ValueError, "sivae_hip: a segmented batch needs the Winograd weight-gradient kernel for a fused prologue"))
    return Route("direct_wgrad", "sivae_conv2d_wgrad", None, "Pkuw", key=conv_wgrad_kernel_key(ks, Co, pro),
                 ws_bytes=L.sivae_conv2d_wgrad_workspace_bytes(B, Ci, Co, H, W, ks))


@_memo
def conv2d_up_dgrad_route(B, C, N, H, W, *, has_wp1=False, dx_al8=True):
    """route of conv2d_up_dgrad for dy [B, C, H, W] -> dx [B, N, H/2, W/2]; the operand of the wino4_pool family is built
    from the mode-1 PackedW (wp1), the others from the mode-0 one.  dx_al8: the destination is 8-byte aligned (every
    tensor of its own is; a view at an odd element offset is not) — the wino4_pool kernel stores pixel pairs and takes
    only such destinations, the phase-form kernels take any float32 destination"""
    L = _lib.load()
    if (WINO4_DGRAD_POOL and WINO4 and has_wp1 and dx_al8 and max(C, N) <= WINO4_MAXC
            and L.sivae_conv2d_wino4_dgrad_pool_pays(B, C, N, H, W) == 1):
        return Route("wino4_pool", "sivae_conv2d_wino4_dgrad_pool", "wino4", "a", key="conv_wino4_pool_kernel<false>",
                     ratio=_F44)
    key = "conv_wino_up_dgrad_kernel<%s>" % ("1,4" if W // 2 >= 32 else "2,3")
    S = L.sivae_conv2d_wino_up_dgrad_splitk(B, C, N, H // 2, W // 2)
    if S > 1:  # small shards: split the 4C input planes
        return Route("wino_up_dgrad_splitk", "sivae_conv2d_wino_up_dgrad_splitk_run", "wino_up_dgrad", "haw", split=S,
                     ws_bytes=L.sivae_conv2d_wino_up_dgrad_splitk_workspace_bytes(B, C, N, H // 2, W // 2), key=key,
                     ratio=_F22_UP)
    return Route("wino_up_dgrad", "sivae_conv2d_wino_up_dgrad", "wino_up_dgrad", "ha", key=key, ratio=_F22_UP)


ScaleConvRoutes = collections.namedtuple("ScaleConvRoutes", "forward dgrad wgrad refused")


@_memo
def scale_conv_routes(kind, B, Ci, Co, H, W):
    """routes of a fused_scale convolution of the style variant (functional.conv_upscale / conv_downscale) on an input
    [B, Ci, H, W]: kind "up" -> [B, Co, 2H, 2W], "down" -> [B, Co, H/2, W/2].  Both are the 3x3 convolution of a
    nearest-2x upsampled input with Cl low-resolution and Cf full-resolution channels, run one way or the other:
        up:    forward conv2d_fwd(upsample)    data gradient conv2d_up_dgrad         weight gradient conv2d_wgrad(upsample)
        down:  forward conv2d_up_dgrad         data gradient conv2d_fwd(upsample)    weight gradient conv2d_wgrad(upsample)
    -> (forward, dgrad, wgrad, refused): the three Routes of the layer, and why it stays on torch's convolutions (None:
    it runs on the kernels)."""
    if kind not in ("up", "down"):
        raise ValueError("sivae_hip: scale_conv_routes kind must be 'up' or 'down', got %r" % (kind,))
    if kind == "down" and (H % 2 or W % 2):
        return ScaleConvRoutes(None, None, None, "odd full-resolution side %dx%d" % (H, W))
    (Cl, Cf, h, w) = (Ci, Co, H, W) if kind == "up" else (Co, Ci, H // 2, W // 2)
    if min(B, Cl, Cf, h, w) <= 0:
        return ScaleConvRoutes(None, None, None, "empty tensor")
    conv = conv2d_fwd_route(B, Cl, Cf, 2 * h, 2 * w, 3, upsample=True)
    # (the destination of the phase data gradient is a tensor of its own here, never a slab view: dx_al8)
    adj = conv2d_up_dgrad_route(B, Cf, Cl, 2 * h, 2 * w, has_wp1=True)
    wgrad = conv2d_wgrad_route(B, Cl, Cf, 2 * h, 2 * w, 3, upsample=True)
    fwd, dgrad = (conv, adj) if kind == "up" else (adj, conv)
    refused = None
    for r in (conv, adj, wgrad):
        if r.error:
            refused = r.error[1]
    if refused is None and not conv2d_up_dgrad_supported(h, w):
        refused = "no phase-form data gradient on %dx%d maps" % (h, w)
    return ScaleConvRoutes(fwd, dgrad, wgrad, refused)


def bn_bwd_route(B, C, H, W, *, op="bn_bwd", four_d=True, dy_pooled=False, nseg=1):
    """route of bn_bwd / bn_bwd_signmask / bn_bwd_dzsum (op: "bn_bwd", "signmask", "dzsum") for x [B, C, H, W] (four_d
    False: x is [B, C] or flat, H * W elements per channel and image): the one-launch persistent kernel, the
    synchronised pair, or the three-launch form that takes every variant (nseg = 1: seg_images == B, the plain op)."""
    L = _lib.load()
    sync = SYNC_BN is not None
    # (shapes / modes the fused read of a pooled dy does not cover: the pool's adjoint runs first)
    expand = op == "bn_bwd" and dy_pooled and (sync or bool(H & 1) or bool(W & 3))
    if (BN_FUSED and not sync and four_d
            # several ranks share this GPU (tests only): their persistent grids could starve each other
            and os.environ.get("SIVAE_DP_SAME_DEVICE", "0") != "1"
            and L.sivae_bn_bwd_fused_supported(B, C, H, W, B // nseg) == 1):
        return Route("bn_fused", "sivae_bn_bwd_fused", materialise=expand,
                     ws_bytes=L.sivae_bn_bwd_fused_workspace_bytes(B, C, H, W, B // nseg))
    if sync and nseg > 1:
        return Route("bn_seg", "sivae_bn_bwd_seg", materialise=expand, error=(
            RuntimeError, "sivae_hip: segmented batches and synchronised BatchNorm do not combine"))
    ws = L.sivae_bn_workspace_bytes(B // nseg, nseg * C, H * W)
    # (the sync pair has no mask / block-sum argument: bn_signmask_supported / bn_bwd_dzsum_supported keep those ops
    # away under SYNC_BN, and a direct call of them gets the local statistics of the three-launch form)
    if sync and op == "bn_bwd":
        return Route("bn_sync", "sivae_bn_bwd_reduce", materialise=expand, ws_bytes=ws)
    return Route("bn_seg", "sivae_bn_bwd_seg", materialise=expand, ws_bytes=ws)


def _prologue(pro):
    """pro = (mean, invstd, gamma, beta, slope) of a fused producer BatchNorm + LeakyReLU, or None -> the five C arguments"""
    if pro is None:
        return None, None, None, None, 1.0
    pm, pi, pg, pb, slope = pro
    _require(pm, pi, pg, pb)
    return _p(pm), _p(pi), _p(pg), _p(pb), float(slope)


def _conv_call(r, a, b, c, dims, ks=0, bias=None, pro=None, stats=None, upsample=False, accumulate=False, seg=0,
               out_f32=False):
    """the one launch of a conv route.  Every conv entry point takes a subset of the same arguments in the same order —
    three tensors, [b]ias, [P]rologue + slope, [S]tatistics, the five sizes ([h]: the map halved, [f]: H * W as one),
    [k]ernel size, [u]psample flag, [a]ccumulate flag, fp32 NCHW [o]utput flag (bf16 mode), se[g]ment images,
    [w]orkspace + its size, stream — and r.args names the subset."""
    s = r.args
    args = [_p(a), _p(b), _p(c)]
    if "b" in s:
        args.append(_p(bias))
    if "P" in s:
        args.extend(_prologue(pro))
    if "S" in s:
        args.append(_p(stats))
    B, Ci, Co, H, W = dims
    args.extend((B, Ci, Co, H // 2, W // 2) if "h" in s else ((B, Ci, Co, H * W) if "f" in s else dims))
    if "k" in s:
        args.append(ks)
    if "u" in s:
        args.append(int(bool(upsample)))
    if "a" in s:
        args.append(int(bool(accumulate)))
    if "o" in s:
        args.append(int(bool(out_f32)))
    if "g" in s:
        args.append(seg)
    if "w" in s:
        ws = workspace(r.ws_bytes, a.device)
        args.extend((_p(ws), ws.numel()))
    _lib.call(r.entry, *args, _s(a))


def conv2d_dgrad_bnbwd_supported(H, W):
    return WINO and FUSE_BN_BWD and SYNC_BN is None and _lib.load().sivae_conv2d_wino_supported(H, W) == 1


def conv2d_dgrad_bnbwd(dy, wp, Cm, bn_x, mean, invstd, gamma, beta, slope=LRELU_SLOPE):
    """3x3 data gradient dh = dgrad(dy) whose epilogue also reduces the BatchNorm-backward sums of
    h = LeakyReLU(BN(bn_x)): -> (dh, partials [n_tiles, Cm, 2])"""
    _require(dy, bn_x, mean, invstd, gamma, beta)
    B, Ci, H, W = dy.shape
    dh = torch.empty((B, Cm, H, W), dtype=torch.float32, device=dy.device)
    part = torch.empty((_lib.load().sivae_conv2d_wino_num_px_tiles(B, H, W), Cm, 2), dtype=torch.float32,
                       device=dy.device)
    t0 = timer_begin()
    _lib.call("sivae_conv2d_wino_dgrad_bnbwd", _p(dy), _p(wp.wino()), _p(dh), _p(bn_x), _p(mean), _p(invstd), _p(gamma),
              _p(beta), float(slope), _p(part), B, Ci, Cm, H, W, _s())
    if t0 is not None:
        timer_end(t0, _wino_key(W, False), 2.0 * B * H * W * Cm * Ci * 9, _F22)
    return dh, part


def bn_bwd_from_partials(dy, x, mean, invstd, gamma, beta, partials, slope=LRELU_SLOPE, want_param_grads=True,
                         pg_out=None):
    """BatchNorm(+LeakyReLU, sign recomputed from x) backward whose reduction pass was done by the producer of dy"""
    _require(dy, x, mean, invstd, gamma, beta, partials)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    ws = workspace(_lib.load().sivae_bn_workspace_bytes(B, C, HW), x.device)
    dx = torch.empty_like(x)
    dgamma, dbeta = _pg(pg_out, C, x.device, want_param_grads)
    _lib.call("sivae_bn_bwd_from_partials", _p(dy), _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), float(slope),
              _p(partials), partials.shape[0], _p(dx), _p(dgamma), _p(dbeta), B, C, HW, _p(ws), ws.numel(), _s())
    return dx, dgamma, dbeta


def conv2d_up_dgrad_supported(Hs, Ws):
    return WINO_UP and _lib.load().sivae_conv2d_wino_up_dgrad_supported(Hs, Ws) == 1


def conv2d_up_dgrad(dy, wp, N, out=None, accumulate=False, wp1=None):
    """gradient of conv3x3(Upsample2(x)) with respect to the LOW-resolution x: dy [B, C, 2Hs, 2Ws] -> [B, N, Hs, Ws]
    (wp: PackedW of the conv's weight [C, N, 3, 3], mode 0; wp1: the mode-1 PackedW of the same weight — with it the
    launches with N <= 64 take the F(4x4,3x3) kernel with the 2x2 block sum folded into its output transform)."""
    _require(dy, out)
    B, C, H, W = dy.shape
    r = conv2d_up_dgrad_route(B, C, N, H, W, has_wp1=wp1 is not None, dx_al8=out is None or not (out.data_ptr() & 7))
    dx = _out(out, (B, N, H // 2, W // 2), dy.device)
    t0 = timer_begin()
    _conv_call(r, dy, getattr(wp1 if r.family == "wino4_pool" else wp, r.operand)(), dx, (B, C, N, H, W),
               accumulate=accumulate)
    if t0 is not None:
        timer_end(t0, r.key, 2.0 * B * H * W * C * N * 9, r.ratio)
    return dx


def seg_prologue_supported(H, W):
    """maps on which a SEGMENTED batch (nseg > 1) can keep the BatchNorm prologue fused into conv2 and into conv2's
    weight gradient (the Winograd kernels carry per-segment parameter tables); elsewhere the block stores h"""
    L = _lib.load()
    return (WINO and WINO_WGRAD and L.sivae_conv2d_wino_supported(H, W) == 1
            and L.sivae_conv2d_wino_wgrad_supported(H, W) == 1)


def conv2d_fwd(x, wp, Co, ks, bias=None, pro=None, upsample=False, want_stats=False, out=None,
               accumulate=False, nseg=1):
    """x [B, Ci, H, W] (or [B, Ci, H/2, W/2] with upsample) -> y [B, Co, H, W] (+ stats partials).

    wp: a direct pack (tensor from pack_weight) or a PackedW; with a PackedW the kernel is chosen per call from the
    layer's sizes (conv2d_fwd_route).
    pro = (mean, invstd, gamma, beta, slope): fused producer BatchNorm + LeakyReLU on load."""
    B, Ci, Hs, Ws = x.shape
    H, W = (2 * Hs, 2 * Ws) if upsample else (Hs, Ws)
    packed = isinstance(wp, PackedW)
    r = conv2d_fwd_route(B, Ci, Co, H, W, ks, packed=packed, mode=wp.mode if packed else 0, bias=bias is not None,
                         pro=pro is not None, upsample=bool(upsample), want_stats=want_stats, has_out=out is not None,
                         accumulate=bool(accumulate), nseg=nseg)
    _require(x, bias, out, None if packed else wp)
    if r.error is not None:
        raise r.error[0](r.error[1])
    if r.materialise:
        x, upsample = upsample2_fwd(x), False
    w = getattr(wp, r.operand)() if packed else wp
    y = _out(out, (B, Co, H, W), x.device)
    stats = torch.empty((r.stats_rows, Co, 2), dtype=torch.float32, device=x.device) if want_stats else None
    t0 = timer_begin()
    _conv_call(r, x, w, y, (B, Ci, Co, H, W), ks, bias, pro, stats, upsample, accumulate, (B // nseg) if nseg > 1 else 0)
    if t0 is not None:
        timer_end(t0, r.key, 2.0 * B * H * W * Co * Ci * ks * ks, r.ratio)  # (algorithmic: the reference nn.Conv2d's FLOPs)
    return (y, stats) if want_stats else y


def conv2d_wgrad(x, dy, ks, pro=None, upsample=False, out=None, nseg=1):
    """-> dW [Co, Ci, ks, ks]  (written into `out` when given)"""
    _require(x, dy)
    B, Ci = x.shape[0], x.shape[1]
    _, Co, H, W = dy.shape
    r = conv2d_wgrad_route(B, Ci, Co, H, W, ks, pro=pro is not None, upsample=bool(upsample), nseg=nseg)
    if r.error is not None:
        raise r.error[0](r.error[1])
    if r.materialise:
        x, upsample = upsample2_fwd(x), False
    dw = _out(out, (Co, Ci, ks, ks), x.device)
    t0 = timer_begin()
    _conv_call(r, x, dy, dw, (B, Ci, Co, H, W), ks, None, pro, None, upsample, False,
               (B // nseg) if (nseg > 1 and pro is not None) else 0)
    if t0 is not None:  # (includes the tiny slice-reduce launch that follows the MFMA kernel)
        timer_end(t0, r.key, 2.0 * B * H * W * Co * Ci * ks * ks, r.ratio)
    return dw


def conv3x3_flip_transpose(w, scale=1.0, out=None):
    """w [R, S, 3, 3] -> scale * w.transpose(0, 1).flip(2, 3), [S, R, 3, 3] (written into `out` when given: any contiguous
    float32 view, a parameter-gradient slab among them).  The weight transform of the style variant's fused_scale
    convolutions and, the other way round, of their weight gradients (scale_conv.hip)."""
    _require(w, out)
    if w.dtype != torch.float32:
        raise TypeError("sivae_hip: expected float32, got %s" % w.dtype)
    if w.dim() != 4 or w.shape[2] != 3 or w.shape[3] != 3:
        raise ValueError("sivae_hip: conv3x3_flip_transpose takes a [R, S, 3, 3] weight, got %s" % (tuple(w.shape),))
    R, S = w.shape[0], w.shape[1]
    dst = _out(out, (S, R, 3, 3), w.device)
    _lib.call("sivae_conv3x3_flip_transpose", _p(w), _p(dst), R, S, float(scale), _s(w))
    return dst


# ------------------------------------------------------------------------------------------------ linear
def linear_supported(B, K, N):
    return _lib.load().sivae_linear_supported(B, K, N) == 1


def linear_fwd(x, w, bias=None, relu=False):
    """y = x W^T + b (optionally ReLU) for a small batch: x [B, K], w [N, K] -> [B, N]"""
    _require(x, w, bias)
    B, K = x.shape
    N = w.shape[0]
    ws = workspace(_lib.load().sivae_linear_workspace_bytes(B, K, N), x.device)
    y = torch.empty((B, N), dtype=torch.float32, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_linear_fwd", _p(x), _p(w), _p(bias), _p(y), int(bool(relu)), B, K, N, _p(ws), ws.numel(), _s(x))
    if t0 is not None:
        timer_end(t0, "linear_fwd_kernel", 2.0 * B * K * N)
    return y


def linear_dgrad(dy, w):
    _require(dy, w)
    B, N = dy.shape
    K = w.shape[1]
    ws = workspace(_lib.load().sivae_linear_workspace_bytes(B, K, N), dy.device)
    dx = torch.empty((B, K), dtype=torch.float32, device=dy.device)
    t0 = timer_begin()
    _lib.call("sivae_linear_dgrad", _p(dy), _p(w), _p(dx), B, K, N, _p(ws), ws.numel(), _s(dy))
    if t0 is not None:
        timer_end(t0, "linear_dgrad_kernel", 2.0 * B * K * N)
    return dx


def linear_wgrad(dy, x, out=None):
    _require(dy, x)
    B, N = dy.shape
    K = x.shape[1]
    dw = _out(out, (N, K), dy.device)
    t0 = timer_begin()
    _lib.call("sivae_linear_wgrad", _p(dy), _p(x), _p(dw), B, K, N, _s(dy))
    if t0 is not None:
        timer_end(t0, "linear_wgrad_kernel", 2.0 * B * K * N)
    return dw


# ------------------------------------------------------------------------------------------------ 5x5 edges
def pack5_smallco(w, mode):
    """mode 0: w [Cs<=3, Cb, 5, 5] (predict) ; mode 1: w [Cb, Cs<=3, 5, 5] (stem, data-gradient operand)"""
    _require(w)
    n_small, n_big = (w.shape[0], w.shape[1]) if mode == 0 else (w.shape[1], w.shape[0])
    nbytes = _lib.load().sivae_pack_conv5_smallco_bytes(n_small, n_big)
    if nbytes == 0:
        raise _lib.SivaeError("sivae_pack_conv5_smallco_bytes", -2)
    wq = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _lib.call("sivae_pack_conv5_smallco", _p(w), _p(wq), n_small, n_big, mode, _s())
    return wq


def conv5_smallco_fwd(x, wq, Co, bias=None):
    _require(x, wq, bias)
    B, Ci, H, W = x.shape
    y = torch.empty((B, Co, H, W), dtype=torch.float32, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_conv5_smallco_fwd", _p(x), _p(wq), _p(y), _p(bias), B, Ci, Co, H, W, _s())
    if t0 is not None:
        timer_end(t0, "conv5_smallco_fwd_kernel<9>", 2.0 * B * H * W * Co * Ci * 25)
    return y


def conv5_edge_wgrad(x, dy, out=None):
    _require(x, dy)
    B, Ci, H, W = x.shape
    Co = dy.shape[1]
    ws = workspace(_lib.load().sivae_conv5_edge_wgrad_workspace_bytes(B, Ci, Co, H, W), x.device)
    dw = _out(out, (Co, Ci, 5, 5), x.device)
    t0 = timer_begin()
    _lib.call("sivae_conv5_edge_wgrad", _p(x), _p(dy), _p(dw), B, Ci, Co, H, W, _p(ws), ws.numel(), _s())
    if t0 is not None:
        timer_end(t0, "conv5_edge_wgrad_kernel<%s>" % ("true" if Co <= 3 else "false"), 2.0 * B * H * W * Co * Ci * 25)
    return dw


# ------------------------------------------------------------------------------------------------ BN
def bn_stats(x, running_mean=None, running_var=None, num_batches_tracked=None, eps=1e-5, momentum=0.1):
    _require(x, running_mean, running_var, num_batches_tracked)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    L = _lib.load()
    ws = workspace(L.sivae_bn_workspace_bytes(B, C, HW), x.device)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    _lib.call("sivae_bn_stats", _p(x), B, C, HW, float(eps), float(momentum), _p(running_mean), _p(running_var),
              _p(num_batches_tracked), _p(mean), _p(invstd), _p(ws), ws.numel(), _s())
    return mean, invstd


# Synchronised BatchNorm (opt-in for data-parallel runs): SYNC_BN = None, or a callable
# `sync(sums_fp64[C, 2]) -> world_size` that all-reduces (SUM) the per-channel sums in place.  With it, the batch
# statistics (forward) and the two gradient means (backward) are those of the GLOBAL batch, so N shards of B/N
# reproduce the single-process batch-B numbers; the default (None) is local BatchNorm, what DDP does to this model.
SYNC_BN = None


def stats_rows_fit_segments(rows, B, nseg):
    """can `rows` conv-epilogue statistics rows of B images (image order: a row is a pixel tile of one image, or a whole
    number of images) be cut into nseg segments of B / nseg images without a row straddling two of them?"""
    per_row = B // rows if rows < B else 1
    return not (rows % nseg or (rows < B and B % rows) or (rows >= B and rows % B) or (B // nseg) % per_row)


def bn_stats_from_conv(partials, B, C, HW, running_mean=None, running_var=None, num_batches_tracked=None,
                       eps=1e-5, momentum=0.1, nseg=1, seg_rev=False):
    """nseg > 1: B = nseg * B_seg images, rows of `partials` in image order; -> mean, invstd of nseg * C entries
    ([nseg][C]); the running buffers get one update per segment (seg_rev: last segment first)"""
    _require(partials, running_mean, running_var, num_batches_tracked)
    mean = torch.empty(nseg * C, dtype=torch.float32, device=partials.device)
    invstd = torch.empty(nseg * C, dtype=torch.float32, device=partials.device)
    if nseg > 1:
        # a partial row covers a pixel tile of ONE image, or — image pairs on 16 x 16 maps, several images per tile on the
        # 8 x 8 / 4 x 4 maps — a whole number of images: it must never straddle two segments (their statistics would mix)
        rows = partials.shape[0]
        if not stats_rows_fit_segments(rows, B, nseg):
            raise ValueError("sivae_hip: %d statistics rows of %d images cannot be cut into %d segments" % (rows, B, nseg))
    if nseg > 1 and SYNC_BN is not None:
        raise RuntimeError("sivae_hip: segmented batches and synchronised BatchNorm do not combine")
    if SYNC_BN is None:
        # (thousands of partial rows — the large-map layers at batch 128 — are folded in two coalesced stages through a
        # scratch buffer; the call is the one-stage form below that)
        nws = _lib.load().sivae_bn_stats_from_conv_workspace_bytes(partials.shape[0], nseg, C)
        ws = workspace(nws, partials.device) if nws else None
        _lib.call("sivae_bn_stats_from_conv_ws", _p(partials), partials.shape[0], nseg, int(bool(seg_rev)), B // nseg,
                  C, HW, float(eps), float(momentum), _p(running_mean), _p(running_var), _p(num_batches_tracked),
                  _p(mean), _p(invstd), _p(ws), ws.numel() if ws is not None else 0, _s())
        return mean, invstd
    sums = torch.empty((C, 2), dtype=torch.float64, device=partials.device)
    _lib.call("sivae_bn_sums_from_conv", _p(partials), partials.shape[0], C, _p(sums), _s())
    world = SYNC_BN(sums)
    _lib.call("sivae_bn_finalize_sums", _p(sums), C, float(B) * HW * world, float(eps), float(momentum),
              _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(mean), _p(invstd), _s())
    return mean, invstd


def bn_update_running(mean, invstd, count, running_mean, running_var, num_batches_tracked, eps=1e-5, momentum=0.1,
                      nseg=1, seg_rev=False):
    _require(mean, invstd, running_mean, running_var, num_batches_tracked)
    _lib.call("sivae_bn_update_running_seg", _p(mean), _p(invstd), nseg, int(bool(seg_rev)), mean.numel() // nseg,
              float(count), float(eps), float(momentum), _p(running_mean), _p(running_var), _p(num_batches_tracked),
              _s())


def bn_apply_act(x, res, mean, invstd, gamma, beta, slope=LRELU_SLOPE, out=None, res_up=False, nseg=1):
    """res_up: res is [B, C, H/2, W/2] and is added through nearest-2x upsample addressing"""
    _require(x, res, mean, invstd, gamma, beta, out)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = out if out is not None else torch.empty_like(x)
    H, W = (x.shape[2], x.shape[3]) if x.dim() == 4 else (1, HW)
    if res_up:
        assert res.shape == (B, C, H // 2, W // 2)
    _lib.call("sivae_bn_apply_act_seg", _p(x), _p(res), int(bool(res_up)), _p(mean), _p(invstd), _p(gamma), _p(beta),
              float(slope), _p(y), None, B, C, H, W, B // nseg, _s())
    return y


def bn_apply_act_pool(x, res, mean, invstd, gamma, beta, slope=LRELU_SLOPE, want_full=True, nseg=1):
    """-> (y, AvgPool2d(2)(y)) in one pass (y is None with want_full=False); None when the shape is not covered
    (odd H or W % 4 != 0)"""
    B, C, H, W = x.shape
    if (H & 1) or (W & 3):
        return None
    _require(x, res, mean, invstd, gamma, beta)
    y = torch.empty_like(x) if want_full else None
    yp = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    _lib.call("sivae_bn_apply_act_seg", _p(x), _p(res), 0, _p(mean), _p(invstd), _p(gamma), _p(beta), float(slope),
              _p(y), _p(yp), B, C, H, W, B // nseg, _s())
    return y, yp


def bn_signmask_supported(x):
    """the 1-bit LeakyReLU sign mask path: local BatchNorm, H even, W % 8 == 0"""
    return SIGNMASK and SYNC_BN is None and x.dim() == 4 and not (x.shape[2] & 1) and not (x.shape[3] & 7)


def bn_apply_act_signmask(x, res, mean, invstd, gamma, beta, slope=LRELU_SLOPE, res_up=False, pool=False,
                          want_full=True, nseg=1):
    """LeakyReLU(BN(x) + res) -> (y, y_pooled, mask): y is None with want_full=False (pool only), y_pooled is None
    without pool; mask = the activation's sign bits (uint8, 1 bit per element) for bn_bwd_signmask"""
    _require(x, res, mean, invstd, gamma, beta)
    B, C, H, W = x.shape
    assert pool or want_full
    y = torch.empty_like(x) if want_full else None
    yp = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device) if pool else None
    mask = torch.empty(_lib.load().sivae_bn_signmask_bytes(B, C, H * W), dtype=torch.uint8, device=x.device)
    _lib.call("sivae_bn_apply_act_signmask_seg", _p(x), _p(res), int(bool(res_up)), _p(mean), _p(invstd), _p(gamma),
              _p(beta), float(slope), _p(y), _p(yp), _p(mask), B, C, H, W, B // nseg, _s())
    return y, yp, mask


def _bn_bwd_run(op, dy, y, mask, x, mean, invstd, gamma, beta, act_mode, slope, want_dz, dz_sum, dy_pooled,
                want_param_grads, pg_out, nseg):
    """the body of bn_bwd / bn_bwd_signmask / bn_bwd_dzsum: route -> allocate -> launch.  -> dx, dz (full resolution, its
    2x2 block sums with dz_sum, or None), dgamma, dbeta (mean / invstd are [nseg][C])"""
    B, C = x.shape[0], x.shape[1]
    H, W = (x.shape[2], x.shape[3]) if x.dim() == 4 else (1, x.numel() // (B * C))
    r = bn_bwd_route(B, C, H, W, op=op, four_d=x.dim() == 4, dy_pooled=bool(dy_pooled), nseg=nseg)
    if r.materialise:
        dy, dy_pooled = avgpool2_bwd(dy, H, W), False
    _require(dy, y, x, mean, invstd, gamma, beta)
    if r.error is not None:
        raise r.error[0](r.error[1])
    dx = torch.empty_like(x)
    dz = None
    if dz_sum:
        dz = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    elif want_dz:
        dz = torch.empty_like(x)
    dgamma, dbeta = _pg(pg_out, C, x.device, want_param_grads)
    ws = workspace(r.ws_bytes, x.device)
    if r.family == "bn_sync":
        local = torch.empty((C, 2), dtype=torch.float64, device=x.device)
        _lib.call(r.entry, _p(dy), _p(y), _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), int(act_mode), float(slope),
                  _p(local), B, C, H * W, _p(ws), ws.numel(), _s())
        glob = local.clone()
        world = SYNC_BN(glob)
        _lib.call("sivae_bn_bwd_apply", _p(dy), _p(y), _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta),
                  int(act_mode), float(slope), _p(local), _p(glob), float(B) * H * W * world, _p(dx), _p(dz),
                  _p(dgamma), _p(dbeta), B, C, H * W, _p(ws), ws.numel(), _s())
        return dx, dz, dgamma, dbeta
    # (every variant, segmented or not, that the two general entry points take)
    general = (_p(dy), _p(y), _p(mask), _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), int(act_mode), float(slope),
               _p(dx), _p(dz), _p(dgamma), _p(dbeta), B, C, H, W, int(bool(dy_pooled)), int(bool(dz_sum)), B // nseg)
    if r.family == "bn_fused":
        try:
            _lib.call(r.entry, *general, _p(bn_fused_state(x.device)), _p(ws), ws.numel(), _s(x))
            return dx, dz, dgamma, dbeta
        except _lib.SivaeError as e:
            if e.code != -2:
                raise
            # a shape the plan of this variant does not take after all (the query and the launch plan with the same
            # register budget since round 5, so this is a safety net): the three-launch form takes every shape
            ws = workspace(_lib.load().sivae_bn_workspace_bytes(B // nseg, nseg * C, H * W), x.device)
    # SIVAE_BN_FUSED_FINALIZE: the per-channel finalize runs inside the reduction kernel (a dead end kept behind its
    # switch: local statistics only, and a flat or [B, C] input only when it is segmented)
    fin = BN_FUSED_FINALIZE and C <= 8192 and SYNC_BN is None and (nseg > 1 or x.dim() == 4)
    _lib.call("sivae_bn_bwd_seg", *general, _p(counters(x.device) if fin else None), _p(ws), ws.numel(), _s())
    return dx, dz, dgamma, dbeta


def bn_bwd_signmask(dy, mask, x, mean, invstd, gamma, slope=LRELU_SLOPE, dy_pooled=False, dz_sum=False,
                    want_dz=True, want_param_grads=True, pg_out=None, nseg=1):
    """backward of bn_apply_act_signmask -> dx, dz (full resolution, or its 2x2 block sums with dz_sum), dgamma,
    dbeta.  dy_pooled: dy is the gradient of the pooled output."""
    B, C, H, W = x.shape
    if mask.dtype != torch.uint8 or not mask.is_cuda or mask.numel() < _lib.load().sivae_bn_signmask_bytes(B, C, H * W):
        raise TypeError("sivae_hip: bn_bwd_signmask needs the uint8 device mask bn_apply_act_signmask returned")
    return _bn_bwd_run("signmask", dy, None, mask, x, mean, invstd, gamma, None, 3, slope, want_dz, dz_sum, dy_pooled,
                       want_param_grads, pg_out, nseg)


def bn_bwd_dzsum_supported(x):
    return SYNC_BN is None and not (x.shape[2] & 1) and not (x.shape[3] & 3)


def bn_bwd_dzsum(dy, y, x, mean, invstd, gamma, slope=LRELU_SLOPE, want_param_grads=True, pg_out=None, nseg=1):
    """act_mode-1 BatchNorm(+residual+LeakyReLU) backward -> dx, dz_half (2x2 block sums of the residual-branch
    gradient, [B, C, H/2, W/2]), dgamma, dbeta"""
    return _bn_bwd_run("dzsum", dy, y, None, x, mean, invstd, gamma, None, 1, slope, False, True, False,
                       want_param_grads, pg_out, nseg)


def bn_bwd(dy, y, x, mean, invstd, gamma, slope=LRELU_SLOPE, want_dz=False, want_param_grads=True, beta=None,
           act_mode=None, dy_pooled=False, pg_out=None, nseg=1):
    """-> dx, dz (or None), dgamma, dbeta (or None, None).
    act_mode: 0 none, 1 LeakyReLU sign from the saved output y, 2 sign recomputed from x (needs beta).
    dy_pooled: dy is the gradient of AvgPool2d(2)(output) at half resolution; the pool's adjoint is applied on load."""
    if act_mode is None:
        act_mode = 1 if y is not None else 0
    return _bn_bwd_run("bn_bwd", dy, y, None, x, mean, invstd, gamma, beta, act_mode, slope, want_dz, False, dy_pooled,
                       want_param_grads, pg_out, nseg)


def channel_sum(x, out=None):
    _require(x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    L = _lib.load()
    ws = workspace(L.sivae_bn_workspace_bytes(B, C, HW), x.device)
    out = _out(out, (C,), x.device)
    _lib.call("sivae_channel_sum", _p(x), _p(out), B, C, HW, _p(ws), ws.numel(), _s())
    return out


# ------------------------------------------------------------------------------------------------ eltwise
def avgpool2_fwd(x):
    _require(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    _lib.call("sivae_avgpool2_fwd", _p(x), _p(y), B * C, H, W, _s())
    return y


def avgpool2_bwd(dy, H, W):
    _require(dy)
    B, C = dy.shape[0], dy.shape[1]
    dx = torch.empty((B, C, H, W), dtype=torch.float32, device=dy.device)
    _lib.call("sivae_avgpool2_bwd", _p(dy), _p(dx), B * C, H, W, _s())
    return dx


def upsample2_fwd(x):
    _require(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    _lib.call("sivae_upsample2_fwd", _p(x), _p(y), B * C, H, W, _s())
    return y


def upsample2_bwd(dy):
    _require(dy)
    B, C, H2, W2 = dy.shape
    dx = torch.empty((B, C, H2 // 2, W2 // 2), dtype=torch.float32, device=dy.device)
    _lib.call("sivae_upsample2_bwd", _p(dy), _p(dx), B * C, H2 // 2, W2 // 2, _s())
    return dx


def relu_fwd(x, inplace=False):
    _require(x)
    y = x if inplace else torch.empty_like(x)
    _lib.call("sivae_relu_fwd", _p(x), _p(y), x.numel(), _s())
    return y


def relu_bwd(dy, y):
    _require(dy, y)
    dx = torch.empty_like(dy)
    _lib.call("sivae_relu_bwd", _p(dy), _p(y), _p(dx), dy.numel(), _s())
    return dx


def add_(y, x):
    _require(y, x)
    assert y.numel() == x.numel()
    _lib.call("sivae_add_inplace", _p(y), _p(x), y.numel(), _s())
    return y


# ------------------------------------------------------------------------------------------------ losses
def _ld(t):
    """[B, Z] view with unit inner stride -> leading dimension"""
    assert t.dim() == 2 and t.stride(1) == 1, "mu/logvar must be [B, Z] with unit inner stride"
    if not t.is_cuda:
        raise RuntimeError("sivae_hip: tensor is on %s — no CPU fallback" % t.device)
    return t.stride(0)


def reparam_fwd(mu, logvar, eps):
    _require(eps)
    B, Z = mu.shape
    ld = _ld(mu)
    assert _ld(logvar) == ld
    z = torch.empty((B, Z), dtype=torch.float32, device=mu.device)
    _lib.call("sivae_reparam_fwd", _p(mu), _p(logvar), ld, _p(eps), _p(z), B, Z, _s())
    return z


def reparam_bwd(dz, logvar, eps):
    _require(dz, eps)
    B, Z = dz.shape
    dmu = torch.empty_like(dz)
    dlv = torch.empty_like(dz)
    _lib.call("sivae_reparam_bwd", _p(dz), _p(logvar), _ld(logvar), _p(eps), _p(dmu), _p(dlv), Z, B, Z, _s())
    return dmu, dlv


def kl_fwd(logvar, mu, mu_o=0.0, logvar_o=0.0):
    B, Z = mu.shape
    ld = _ld(mu)
    assert _ld(logvar) == ld
    out = torch.empty(B, dtype=torch.float32, device=mu.device)
    _lib.call("sivae_kl_fwd", _p(logvar), _p(mu), ld, float(mu_o), float(logvar_o), _p(out), B, Z, _s())
    return out


def kl_bwd(g, per_sample, g_scale, logvar, mu, mu_o=0.0, logvar_o=0.0):
    _require(g)
    B, Z = mu.shape
    ld = _ld(mu)
    dlv = torch.empty((B, Z), dtype=torch.float32, device=mu.device)
    dmu = torch.empty((B, Z), dtype=torch.float32, device=mu.device)
    _lib.call("sivae_kl_bwd", _p(g), int(bool(per_sample)), float(g_scale), _p(logvar), _p(mu), ld, float(mu_o),
              float(logvar_o), _p(dlv), _p(dmu), Z, B, Z, _s())
    return dlv, dmu


def _prior(t, B, Z, like):
    """calc_kl prior as (fp32 device tensor, row stride, column stride) broadcastable to [B, Z]"""
    t = t.detach().to(device=like.device, dtype=torch.float32)
    if t.dim() > 2:
        raise ValueError("calc_kl: prior of shape %s does not broadcast to [B, Z]" % (tuple(t.shape),))
    while t.dim() < 2:
        t = t.unsqueeze(0)
    r, c = t.shape
    if r not in (1, B) or c not in (1, Z):
        raise ValueError("calc_kl: prior of shape %s does not broadcast to [%d, %d]" % (tuple(t.shape), B, Z))
    t = t.contiguous()
    return t, (c if r == B else 0), (1 if c == Z else 0)


def kl_fwd_t(logvar, mu, mu_o, logvar_o):
    B, Z = mu.shape
    ld = _ld(mu)
    assert _ld(logvar) == ld
    mo, mo_rs, mo_cs = _prior(mu_o, B, Z, mu)
    lo, lo_rs, lo_cs = _prior(logvar_o, B, Z, mu)
    out = torch.empty(B, dtype=torch.float32, device=mu.device)
    _lib.call("sivae_kl_fwd_t", _p(logvar), _p(mu), ld, _p(mo), mo_rs, mo_cs, _p(lo), lo_rs, lo_cs, _p(out), B, Z,
              _s(mu))
    return out


def kl_bwd_t(g, per_sample, g_scale, logvar, mu, mu_o, logvar_o):
    _require(g)
    B, Z = mu.shape
    ld = _ld(mu)
    mo, mo_rs, mo_cs = _prior(mu_o, B, Z, mu)
    lo, lo_rs, lo_cs = _prior(logvar_o, B, Z, mu)
    dlv = torch.empty((B, Z), dtype=torch.float32, device=mu.device)
    dmu = torch.empty((B, Z), dtype=torch.float32, device=mu.device)
    _lib.call("sivae_kl_bwd_t", _p(g), int(bool(per_sample)), float(g_scale), _p(logvar), _p(mu), ld, _p(mo), mo_rs,
              mo_cs, _p(lo), lo_rs, lo_cs, _p(dlv), _p(dmu), Z, B, Z, _s(mu))
    return dlv, dmu


def recon_rowsum_fwd(x, recon, loss_type):
    _require(x, recon)
    B = x.shape[0]
    D = x.numel() // B
    L = _lib.load()
    ws = workspace(L.sivae_recon_workspace_bytes(B, D), x.device)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.call("sivae_recon_rowsum_fwd", _p(x), _p(recon), LOSS_TYPES[loss_type], _p(out), B, D, _p(ws), ws.numel(),
              _s())
    return out


def recon_bwd(x, recon, loss_type, g, g_mode, g_scale, want_drecon=True, want_dx=False):
    _require(x, recon, g)
    B = x.shape[0]
    D = x.numel() // B
    d_r = torch.empty_like(recon) if want_drecon else None
    d_x = torch.empty_like(x) if want_dx else None
    _lib.call("sivae_recon_bwd", _p(x), _p(recon), LOSS_TYPES[loss_type], _p(g), int(g_mode), float(g_scale),
              _p(d_r), _p(d_x), B, D, _s())
    return d_r, d_x


def recon_elem_fwd(x, recon, loss_type):
    _require(x, recon)
    out = torch.empty_like(x)
    _lib.call("sivae_recon_elem_fwd", _p(x), _p(recon), LOSS_TYPES[loss_type], _p(out), x.numel(), _s())
    return out


def vec_sum(v, scale=1.0):
    _require(v)
    out = torch.empty((), dtype=torch.float32, device=v.device)
    _lib.call("sivae_vec_sum", _p(v), v.numel(), float(scale), _p(out), _s())
    return out


def expelbo_fwd(L_, KL, scale, beta_rec, beta_neg):
    _require(L_, KL)
    B = L_.numel()
    e = torch.empty(B, dtype=torch.float32, device=L_.device)
    out = torch.empty((), dtype=torch.float32, device=L_.device)
    _lib.call("sivae_expelbo_fwd", _p(L_), _p(KL), float(scale), float(beta_rec), float(beta_neg), B, _p(e), _p(out),
              _s())
    return out, e


def expelbo_bwd(gout, e, scale, beta_rec, beta_neg):
    _require(gout, e)
    B = e.numel()
    dL = torch.empty_like(e)
    dKL = torch.empty_like(e)
    _lib.call("sivae_expelbo_bwd", _p(gout), _p(e), float(scale), float(beta_rec), float(beta_neg), B, _p(dL),
              _p(dKL), _s())
    return dL, dKL


def lincomb(ts, ws):
    """sum_i ws[i] * ts[i] of up to six device scalars, one launch (lossE / lossD)"""
    n = len(ts)
    _require(*ts)
    out = torch.empty((), dtype=torch.float32, device=ts[0].device)
    ps = [_p(t) for t in ts] + [None] * (6 - n)
    w = [float(v) for v in ws] + [0.0] * (6 - n)
    _lib.call("sivae_lincomb", *ps, *w, n, _p(out), _s())
    return out


def lincomb_bwd(g, ws):
    n = len(ws)
    _require(g)
    out = torch.empty(n, dtype=torch.float32, device=g.device)
    w = [float(v) for v in ws] + [0.0] * (6 - n)
    _lib.call("sivae_lincomb_bwd", _p(g), *w, n, _p(out), _s())
    return out


def randn(shape, seed, offset, device):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _require(out)
    _lib.call("sivae_randn", _p(out), out.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
              _s())
    return out


def randn_dev(shape, seed, offset_dev, device):
    """normals from the Philox stream whose position is the device scalar offset_dev (uint64 stored in an int64
    tensor); the position is advanced on the device"""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _lib.call("sivae_randn_dev", _p(out), out.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(offset_dev), _s())
    return out


# ------------------------------------------------------------------------------------------------ optimizer
def adam_step_dev(param, grad, exp_avg, exp_avg_sq, state, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """state: float64 device tensor [4] = {t, lr, step_size, sqrt(bias_correction2)} (t and the factors are advanced
    on the device)"""
    _require(param, grad, exp_avg, exp_avg_sq)
    _lib.call("sivae_adam_step_dev", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(state),
              float(beta1), float(beta2), float(eps), float(grad_scale), _s())


def sum_slabs(flat_grad, slabs):
    """flat_grad += slabs[0] + slabs[1] + ... (<= 4 slabs; the per-use parameter-gradient slabs of optim.FlatAdam)"""
    _require(flat_grad, *slabs)
    n = flat_grad.numel()
    assert 1 <= len(slabs) <= 4 and all(t.numel() == n for t in slabs)
    ptrs = [_p(t) for t in slabs] + [None] * (4 - len(slabs))
    _lib.call("sivae_sum_slabs", _p(flat_grad), ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, _s(flat_grad))


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _require(param, grad, exp_avg, exp_avg_sq)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _lib.call("sivae_adam_step", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(lr / bc1),
              float(beta1), float(beta2), float(eps), float(bc2 ** 0.5), float(grad_scale), _s())


# ------------------------------------------------------------------------------------------------ FID (fid.hip)
FID_MAX_DIMS = 8192


def _require_device(who, kernels, *tensors, need="a ROCm device tensor", on=None):
    """the FID and feature wrappers' one refusal of anything that is not on the device (`on`: said instead of where the
    offending tensor is)"""
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("sivae_hip.%s: tensor is on %s — the %s kernels need %s and have no CPU fallback"
                               % (who, on or getattr(t, "device", type(t).__name__), kernels, need))


def _require_f64(who, *tensors):
    for t in tensors:
        _require_device(who, "FID", t)
        if t.dtype != torch.float64:
            raise TypeError("sivae_hip.%s: expected float64, got %s" % (who, t.dtype))


def _require_f32(who, kernels, *tensors, dtype_first=False, skip_none=True):
    """what the wrappers of the 4-element-chunk kernels (style.hip, rgb.hip, mapping.hip, multi_tensor.hip) demand of
    every tensor: on a ROCm device, float32, contiguous.  dtype_first: a wrong dtype is named before a wrong device"""
    for t in tensors:
        if t is None and skip_none:
            continue
        if not dtype_first:
            _require_device(who, kernels, t)
        if t.dtype != torch.float32:
            raise TypeError("sivae_hip.%s: expected float32, got %s" % (who, t.dtype))
        if dtype_first:
            _require_device(who, kernels, t)
        if not t.is_contiguous():
            raise ValueError("sivae_hip.%s: tensor must be contiguous" % who)


def fid_state(d, device):
    """-> (G [d, d], s [d]): a zeroed fp64 moment state (sivae_hip.fid.ActivationStatistics holds one)"""
    if not 1 <= int(d) <= FID_MAX_DIMS:
        raise ValueError("sivae_hip.fid_state: dims must be in 1 .. %d, got %d" % (FID_MAX_DIMS, d))
    return (torch.zeros((int(d), int(d)), dtype=torch.float64, device=device),
            torch.zeros(int(d), dtype=torch.float64, device=device))


def fid_state_copy(G, s):
    """-> copies of a moment state"""
    _require_f64("fid_state_copy", G, s)
    G2, s2 = torch.empty_like(G), torch.empty_like(s)
    G2.copy_(G)
    s2.copy_(s)
    return G2, s2


def fid_staging(rows, d, device):
    """-> a [rows, d] fp32 staging buffer for activation rows"""
    return torch.empty((int(rows), int(d)), dtype=torch.float32, device=device)


def fid_moments(a, n, G, s):
    """G += a[:n]^T a[:n] on the 64 x 64 block tiles on and above the diagonal, s += the column sums of a[:n]; a: fp32
    [rows >= n, d] with unit column stride (any row stride), converted to fp64 on load.  In place, returns nothing."""
    if not a.is_cuda or a.dtype != torch.float32 or a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise TypeError("sivae_hip.fid_moments: expected a 2-D float32 ROCm tensor with unit column stride")
    _require_f64("fid_moments", G, s)
    d = a.shape[1]
    if not 0 <= int(n) <= a.shape[0] or tuple(G.shape) != (d, d) or tuple(s.shape) != (d,) or \
            not (G.is_contiguous() and s.is_contiguous()):
        raise ValueError("sivae_hip.fid_moments: n rows of a [rows, d] go into contiguous G [d, d] and s [d]")
    t0 = timer_begin()
    _lib.call("sivae_fid_moments", _p(a), int(a.stride(0)) if a.shape[0] > 1 else d, int(n), d, _p(G), _p(s),
              _s(a))
    if t0 is not None:
        timer_end(t0, "fid_moments", float(n) * d * (d + 1))


def fid_finalize(G, s, n):
    """-> (mu [d], sigma [d, d]) fp64: mu = s / n, sigma = (G - s s^T / n) / (n - 1), exactly symmetric"""
    _require_f64("fid_finalize", G, s)
    d = s.shape[0]
    if tuple(G.shape) != (d, d) or not (G.is_contiguous() and s.is_contiguous()) or int(n) < 1:
        raise ValueError("sivae_hip.fid_finalize: contiguous G [d, d], s [d] and n >= 1 rows")
    mu = torch.empty(d, dtype=torch.float64, device=G.device)
    sigma = torch.empty((d, d), dtype=torch.float64, device=G.device)
    _lib.call("sivae_fid_finalize", _p(G), _p(s), int(n), d, _p(mu), _p(sigma), _s(G))
    return mu, sigma


def fid_xty(x, y, symmetric=False):
    """-> x^T y [M, N] fp64 for x [K, M], y [K, N] (unit column stride); symmetric=True (M == N, a product symmetric by
    construction) computes the tiles on and above the diagonal and mirrors them: the result is exactly symmetric"""
    _require_f64("fid_xty", x, y)
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0] or \
            (x.shape[1] > 1 and x.stride(1) != 1) or (y.shape[1] > 1 and y.stride(1) != 1):
        raise ValueError("sivae_hip.fid_xty: x [K, M] and y [K, N] with unit column stride")
    K, M = x.shape
    N = y.shape[1]
    out = torch.empty((M, N), dtype=torch.float64, device=x.device)
    t0 = timer_begin()
    ldx, ldy = (int(x.stride(0)), int(y.stride(0))) if K > 1 else (M, N)
    _lib.call("sivae_fid_xty_f64", _p(x), ldx, _p(y), ldy, _p(out), N, K, M, N, int(bool(symmetric)), _s(x))
    if t0 is not None:
        timer_end(t0, "fid_xty_sym" if symmetric else "fid_xty", (1.0 if symmetric else 2.0) * K * M * N)
    return out


# ------------------------------------------------------------------- pairwise figures on the features (feat_pairs.hip)
FEAT_MAX_K = 8


def _feat_rows(who, *xs):
    """each x: a 2-D float32 ROCm tensor [n >= 1, 1 <= d <= FID_MAX_DIMS] with unit column stride, all of one d
    -> (pointer, row stride, n) per tensor, then d"""
    out = []
    for x in xs:
        _require_device(who, "feature", x)
        if x.dtype != torch.float32:
            raise TypeError("sivae_hip.%s: expected float32 feature rows, got %s" % (who, x.dtype))
        if x.dim() != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= FID_MAX_DIMS or (x.shape[1] > 1 and x.stride(1) != 1) \
                or x.shape[1] != xs[0].shape[1] or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            raise ValueError("sivae_hip.%s: feature rows [n >= 1, 1 <= d <= %d] of one d with unit column stride, got %s "
                             "with strides %s" % (who, FID_MAX_DIMS, tuple(x.shape), tuple(x.stride())))
        out.append((_p(x), int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1]), int(x.shape[0])))
    return out + [int(xs[0].shape[1])]


def _feat_vec(who, t, n, dtype=torch.float64):
    _require_device(who, "feature", t)
    if t.dtype != dtype or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError("sivae_hip.%s: expected a contiguous %s vector of %d elements, got %s %s"
                         % (who, dtype, n, t.dtype, tuple(t.shape)))
    return _p(t)


def _feat_range(who, c0, c1, n):
    c0, c1 = int(c0), int(n if c1 is None else c1)
    if not 0 <= c0 <= c1 <= n:
        raise ValueError("sivae_hip.%s: columns [%d, %d) of %d" % (who, c0, c1, n))
    return c0, c1


def feat_row_sqnorm(x):
    """-> [n] fp64: the squared norm of every row of x (fp32 [n, d], unit column stride), summed in fp64, k ascending"""
    (px, ldx, n), d = _feat_rows("feat_row_sqnorm", x)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    _lib.call("sivae_feat_row_sqnorm", px, ldx, n, d, _p(out), _s(x))
    return out


def feat_sqdist(x, nrmx, y, nrmy):
    """-> D [nx, ny] fp64, D[i][j] = max(0, |x_i|^2 + |y_j|^2 - 2 x_i . y_j) with the norms of feat_row_sqnorm"""
    (px, ldx, nx), (py, ldy, ny), d = _feat_rows("feat_sqdist", x, y)
    pnx, pny = _feat_vec("feat_sqdist", nrmx, nx), _feat_vec("feat_sqdist", nrmy, ny)
    out = torch.empty((nx, ny), dtype=torch.float64, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_feat_sqdist", px, ldx, nx, pnx, py, ldy, ny, pny, d, _p(out), ny, _s(x))
    if t0 is not None:
        timer_end(t0, "feat_sqdist", 2.0 * nx * ny * d)
    return out


def feat_knn_state(n, k, device):
    """-> best [n, k] fp64, every entry +inf: the running state of feat_knn_update"""
    if not 1 <= int(k) <= FEAT_MAX_K:
        raise ValueError("sivae_hip.feat_knn_state: k must be in 1 .. %d, got %d" % (FEAT_MAX_K, k))
    best = torch.empty((int(n), int(k)), dtype=torch.float64, device=device)
    best.fill_(float("inf"))
    return best


def feat_knn_update(x, nrmx, y, nrmy, best, c0=0, c1=None, self_pairs=False):
    """best [nx, k] (ascending) <- per row the k smallest of its values and the squared distances to the rows
    y[c0:c1]; self_pairs: the pair j == i is left out by index (x and y are the same set).  In place."""
    (px, ldx, nx), (py, ldy, ny), d = _feat_rows("feat_knn_update", x, y)
    pnx, pny = _feat_vec("feat_knn_update", nrmx, nx), _feat_vec("feat_knn_update", nrmy, ny)
    _require_f64("feat_knn_update", best)
    if best.dim() != 2 or best.shape[0] != nx or not 1 <= best.shape[1] <= FEAT_MAX_K or not best.is_contiguous():
        raise ValueError("sivae_hip.feat_knn_update: best must be contiguous [%d, 1 .. %d], got %s"
                         % (nx, FEAT_MAX_K, tuple(best.shape)))
    c0, c1 = _feat_range("feat_knn_update", c0, c1, ny)
    t0 = timer_begin()
    _lib.call("sivae_feat_knn_update", px, ldx, nx, pnx, py, ldy, ny, pny, c0, c1, d, int(best.shape[1]),
              int(bool(self_pairs)), _p(best), _s(x))
    if t0 is not None:
        timer_end(t0, "feat_knn_update", 2.0 * nx * (c1 - c0) * d)


def feat_within_state(n, device):
    """-> count [n] int32, zero: the running state of feat_within_update"""
    return torch.zeros(int(n), dtype=torch.int32, device=device)


def feat_within_update(q, nrmq, x, nrmx, radius, count, c0=0, c1=None):
    """count[j] += the number of rows i in [c0, c1) of x with sqdist(q_j, x_i) <= radius[i].  In place."""
    (pq, ldq, nq), (px, ldx, nx), d = _feat_rows("feat_within_update", q, x)
    pnq, pnx = _feat_vec("feat_within_update", nrmq, nq), _feat_vec("feat_within_update", nrmx, nx)
    prad = _feat_vec("feat_within_update", radius, nx)
    pcount = _feat_vec("feat_within_update", count, nq, torch.int32)
    c0, c1 = _feat_range("feat_within_update", c0, c1, nx)
    t0 = timer_begin()
    _lib.call("sivae_feat_within_update", pq, ldq, nq, pnq, px, ldx, nx, pnx, prad, c0, c1, d, pcount, _s(q))
    if t0 is not None:
        timer_end(t0, "feat_within_update", 2.0 * nq * (c1 - c0) * d)


def feat_poly_sums(x, y, gamma, coef0=1.0, degree=3, skip_diag=False):
    """-> [S] fp64: per subset s the sum over i, j (i != j with skip_diag) of (gamma x[s, i] . y[s, j] + coef0)^degree;
    x [S, m, d], y [S, n, d] fp32 with unit column stride"""
    for t in (x, y):
        _require_device("feat_poly_sums", "feature", t)
        if t.dtype != torch.float32:
            raise TypeError("sivae_hip.feat_poly_sums: expected float32 feature rows, got %s" % t.dtype)
        if t.dim() != 3 or min(t.shape) < 1 or not t.shape[2] <= FID_MAX_DIMS or (t.shape[2] > 1 and t.stride(2) != 1) \
                or (t.shape[1] > 1 and t.stride(1) < t.shape[2]) or t.stride(0) < 0:
            raise ValueError("sivae_hip.feat_poly_sums: subsets [S, rows, 1 <= d <= %d] with unit column stride, got %s "
                             "with strides %s" % (FID_MAX_DIMS, tuple(t.shape), tuple(t.stride())))
    if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
        raise ValueError("sivae_hip.feat_poly_sums: x %s and y %s differ in subsets or d" % (tuple(x.shape), tuple(y.shape)))
    if int(degree) not in (1, 2, 3, 4):
        raise ValueError("sivae_hip.feat_poly_sums: degree must be 1 .. 4, got %r" % (degree,))
    S, m, d = x.shape
    n = y.shape[1]
    ldx, ldy = int(x.stride(1)) if m > 1 else d, int(y.stride(1)) if n > 1 else d
    out = torch.empty(S, dtype=torch.float64, device=x.device)
    nbytes = _lib.load().sivae_feat_poly_workspace_bytes(S, m)
    ws = workspace(nbytes, x.device)
    t0 = timer_begin()
    _lib.call("sivae_feat_poly_sums", _p(x), int(x.stride(0)) if S > 1 else 0, ldx, _p(y), int(y.stride(0)) if S > 1 else 0,
              ldy, S, m, n, d, float(gamma), float(coef0), int(degree), int(bool(skip_diag)), _p(out), _p(ws), ws.numel(),
              _s(x))
    if t0 is not None:
        timer_end(t0, "feat_poly_sums", 2.0 * S * m * n * d)
    return out


def feat_gather(rows, index):
    """-> [S, m, d] fp32: rows[index] for index int64 [S, m] on the device (plumbing: torch's gather into a buffer of this
    module)"""
    _require_device("feat_gather", "feature", rows, index, need="ROCm device tensors", on="the CPU")
    if rows.dtype != torch.float32 or rows.dim() != 2 or index.dtype != torch.int64 or index.dim() != 2:
        raise TypeError("sivae_hip.feat_gather: float32 rows [n, d] and int64 index [S, m]")
    out = torch.empty((index.shape[0], index.shape[1], rows.shape[1]), dtype=torch.float32, device=rows.device)
    torch.index_select(rows, 0, index.reshape(-1), out=out.view(-1, rows.shape[1]))
    return out


def feat_bank(capacity, d, device):
    """-> a [capacity, d] fp32 buffer for feature rows (sivae_hip.fidelity.FeatureBank holds one)"""
    if not 1 <= int(d) <= FID_MAX_DIMS:
        raise ValueError("sivae_hip.feat_bank: dims must be in 1 .. %d, got %d" % (FID_MAX_DIMS, d))
    return torch.empty((int(capacity), int(d)), dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------------ style variant (style.hip)
STYLE_NOISE_NONE, STYLE_NOISE_PER_SAMPLE, STYLE_NOISE_BATCH_CONSTANT = 0, 1, 2


def _style_f32(who, *tensors):
    _require_f32(who, "style", *tensors)


def _style_dims(who, x, bias, style=None, noise=None, noise_weight=None, mode=0):
    if x.dim() != 4 or x.shape[2] * x.shape[3] < 2:
        raise ValueError("sivae_hip.%s: expected x [B, C, H, W] with H W >= 2, got %s" % (who, tuple(x.shape)))
    B, C, H, W = x.shape
    if bias.numel() != C:
        raise ValueError("sivae_hip.%s: bias must have C = %d elements, got %s" % (who, C, tuple(bias.shape)))
    if style is not None and tuple(style.shape) != (B, 2 * C):
        raise ValueError("sivae_hip.%s: style must be [B, 2 C] = (%d, %d), got %s" % (who, B, 2 * C, tuple(style.shape)))
    if mode not in (STYLE_NOISE_NONE, STYLE_NOISE_PER_SAMPLE, STYLE_NOISE_BATCH_CONSTANT):
        raise ValueError("sivae_hip.%s: noise mode must be 0, 1 or 2, got %r" % (who, mode))
    if mode != STYLE_NOISE_NONE:
        want = (B if mode == STYLE_NOISE_PER_SAMPLE else 1, 1, H, W)
        if noise is None or noise_weight is None or tuple(noise.shape) != want or noise_weight.numel() != C:
            raise ValueError("sivae_hip.%s: noise mode %d needs noise %s and noise_weight with C = %d elements"
                             % (who, mode, want, C))
    return B, C, H, W


def style_dec_fwd(x, noise, noise_weight, bias, style, mode, layer=0, eps=1e-8, blur=False):
    """-> (y, mean [B, C], rstd [B, C]): noise injection (mode 1: noise [B, 1, H, W]; 2: [1, 1, H, W]; 0: none, the
    layer's fixed bump) -> bias -> LeakyReLU(0.2) -> InstanceNorm -> y = xh (style[:, :C] + 1) + style[:, C:].
    blur=True: the same of style_blur(x), bit for bit, taken from x by 9 taps (the blurred tensor is never stored)"""
    if mode == STYLE_NOISE_NONE:
        noise = noise_weight = None
    _style_f32("style_dec_fwd", x, noise, noise_weight, bias, style)
    B, C, H, W = _style_dims("style_dec_fwd", x, bias, style, noise, noise_weight, mode)
    y = torch.empty_like(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, C), dtype=torch.float32, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_style_dec_blur_fwd" if blur else "sivae_style_dec_fwd", _p(x), _p(noise), _p(noise_weight), _p(bias),
              _p(style), _p(y), _p(mean), _p(rstd), B, C, H, W, int(mode), int(layer), float(eps), _s(x))
    if t0 is not None:
        timer_end(t0, "style_dec_blur_fwd_kernel" if blur else "style_dec_fwd_kernel", 12.0 * x.numel())
    return y, mean, rstd


def style_dec_bwd(dy, x, noise, noise_weight, bias, style, mean, rstd, mode, layer=0, want_dx=True, want_dnw=True,
                  want_dbias=True, want_dstyle=True, blur=False):
    """-> (dx, dnoise_weight [C], dbias [C], dstyle [B, 2 C]), None for what is not wanted (and for dnoise_weight in mode
    0); the activation is recomputed from x.  blur=True: the backward of style_dec_fwd(..., blur=True) from the UNBLURRED
    x, dx = style_blur of the gradient with respect to style_blur(x): inside the kernel where style_dec_blur_bwd_fused(H, W)
    says so, by a style_blur call here otherwise"""
    if mode == STYLE_NOISE_NONE:
        noise = noise_weight = None
        want_dnw = False
    _style_f32("style_dec_bwd", dy, x, noise, noise_weight, bias, style, mean, rstd)
    B, C, H, W = _style_dims("style_dec_bwd", x, bias, style, noise, noise_weight, mode)
    if dy.shape != x.shape or tuple(mean.shape) != (B, C) or tuple(rstd.shape) != (B, C):
        raise ValueError("sivae_hip.style_dec_bwd: dy like x and mean, rstd [B, C] expected")
    dx = torch.empty_like(x) if want_dx else None
    dnw = torch.empty(C, dtype=torch.float32, device=x.device) if want_dnw else None
    dbias = torch.empty(C, dtype=torch.float32, device=x.device) if want_dbias else None
    dstyle = torch.empty((B, 2 * C), dtype=torch.float32, device=x.device) if want_dstyle else None
    L = _lib.load()
    ws_bytes = (L.sivae_style_dec_blur_bwd_workspace_bytes if blur else L.sivae_style_dec_bwd_workspace_bytes)(B, C)
    ws = workspace(ws_bytes, x.device) if (want_dnw or want_dbias) else None
    t0 = timer_begin()
    _lib.call("sivae_style_dec_blur_bwd" if blur else "sivae_style_dec_bwd", _p(dy), _p(x), _p(noise), _p(noise_weight),
              _p(bias), _p(style), _p(mean), _p(rstd), _p(dx), _p(dnw), _p(dbias), _p(dstyle), B, C, H, W, int(mode),
              int(layer), _p(ws), 0 if ws is None else ws.numel(), _s(x))
    if t0 is not None:
        timer_end(t0, "style_dec_blur_bwd_kernel" if blur else "style_dec_bwd_kernel", 30.0 * x.numel())
    if blur and want_dx and not style_dec_blur_bwd_fused(H, W):
        dx = style_blur(dx)  # (a plane beyond the LDS bound: the kernel left the gradient with respect to blur(x))
    return dx, dnw, dbias, dstyle


def style_dec_blur_bwd_fused(H, W):
    """does style_dec_bwd(..., blur=True) finish in one launch at this plane size (the plane staged in LDS)"""
    return bool(_lib.load().sivae_style_dec_blur_bwd_fused(int(H), int(W)))


def style_enc_fwd(x, bias, eps=1e-5, blur=False):
    """-> (xn, mean [B, C], std [B, C]) of t = lrelu_0.2(x + bias): xn = (t - mean) / sqrt(var + eps), std = sqrt(var).
    blur=True: style_blur(xn) in the place of xn, bit for bit (xn itself is not written)"""
    _style_f32("style_enc_fwd", x, bias)
    B, C, H, W = _style_dims("style_enc_fwd", x, bias)
    xn = torch.empty_like(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    std = torch.empty((B, C), dtype=torch.float32, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_style_enc_blur_fwd" if blur else "sivae_style_enc_fwd", _p(x), _p(bias), _p(xn), _p(mean), _p(std),
              B, C, H, W, float(eps), _s(x))
    if t0 is not None:
        timer_end(t0, "style_enc_blur_fwd_kernel" if blur else "style_enc_fwd_kernel", 8.0 * x.numel())
    return xn, mean, std


def style_enc_bwd(dxn, dmean, dstd, x, bias, mean, std, eps=1e-5, want_dx=True, want_dbias=True, blur=False):
    """-> (dx, dbias [C]) from the three upstream gradients (each may be None: zero); where std == 0 the dstd term is
    dropped (the reference's gradient is NaN there).  blur=True: dxn is the gradient of style_blur(xn); the kernel reads
    its blur by 9 taps"""
    _style_f32("style_enc_bwd", dxn, dmean, dstd, x, bias, mean, std)
    B, C, H, W = _style_dims("style_enc_bwd", x, bias)
    if (dxn is not None and dxn.shape != x.shape) or any(t is not None and tuple(t.shape) != (B, C)
                                                         for t in (dmean, dstd, mean, std)):
        raise ValueError("sivae_hip.style_enc_bwd: dxn like x and dmean, dstd, mean, std [B, C] expected")
    dx = torch.empty_like(x) if want_dx else None
    dbias = torch.empty(C, dtype=torch.float32, device=x.device) if want_dbias else None
    L = _lib.load()
    ws_bytes = (L.sivae_style_enc_blur_bwd_workspace_bytes if blur else L.sivae_style_enc_bwd_workspace_bytes)(B, C)
    ws = workspace(ws_bytes, x.device) if want_dbias else None
    t0 = timer_begin()
    _lib.call("sivae_style_enc_blur_bwd" if blur else "sivae_style_enc_bwd", _p(dxn), _p(dmean), _p(dstd), _p(x), _p(bias),
              _p(mean), _p(std), _p(dx), _p(dbias), B, C, H, W, float(eps), _p(ws), 0 if ws is None else ws.numel(), _s(x))
    if t0 is not None:
        timer_end(t0, "style_enc_blur_bwd_kernel" if blur else "style_enc_bwd_kernel", 20.0 * x.numel())
    return dx, dbias


def style_blur(x):
    """the depthwise [1, 2, 1] x [1, 2, 1] / 16 filter with zero padding; its own adjoint (the backward is the same call)"""
    _style_f32("style_blur", x)
    if x.dim() != 4:
        raise ValueError("sivae_hip.style_blur: expected x [B, C, H, W], got %s" % (tuple(x.shape),))
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    _lib.call("sivae_style_blur", _p(x), _p(y), B, C, H, W, _s(x))
    return y


STYLE_RGB_MAX_K = 4  # image channels the RGB-layer kernels of rgb.hip are built for


def _style_rgb_f32(who, *tensors):
    """dtypes first, so that a wrong one is named as such wherever the tensor is"""
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError("sivae_hip.%s: expected float32, got %s" % (who, t.dtype))


def _style_rgb_dims(who, feat, img, weight, bias, to_rgb, pool=False):
    """feat [B, C, Ho, Wo] (or its shape), img [B, K, H, W] (or its shape), weight with K C elements ([K, C] for to_rgb,
    [C, K] for from_rgb; the reference's [., ., 1, 1] is the same memory), bias [K] / [C] -> (B, C, H, W, K), H, W the
    image's"""
    fs, ims = tuple(getattr(feat, "shape", feat)), tuple(getattr(img, "shape", img))
    if len(fs) != 4 or len(ims) != 4 or fs[0] != ims[0] or min(fs) < 1 or min(ims) < 1:
        raise ValueError("sivae_hip.%s: expected features [B, C, H, W] and an image [B, K, H, W], got %s and %s"
                         % (who, fs, ims))
    B, C, K, H, W = fs[0], fs[1], ims[1], ims[2], ims[3]
    if not 1 <= K <= STYLE_RGB_MAX_K:
        raise ValueError("sivae_hip.%s: 1 <= K <= %d image channels, got %d" % (who, STYLE_RGB_MAX_K, K))
    if pool and (H % 2 or W % 2):
        raise ValueError("sivae_hip.%s: pooling needs an even H and W, got %d x %d" % (who, H, W))
    if fs[2:] != ((H // 2, W // 2) if pool else (H, W)):
        raise ValueError("sivae_hip.%s: features %s do not belong to the image %s (pool=%s)" % (who, fs, ims, bool(pool)))
    lead = (K, C) if to_rgb else (C, K)
    if weight.numel() != K * C or tuple(weight.shape[:2]) != lead or bias.numel() != lead[0]:
        raise ValueError("sivae_hip.%s: weight %s / bias %s do not fit C = %d, K = %d"
                         % (who, tuple(weight.shape), tuple(bias.shape), C, K))
    return B, C, H, W, K


def style_to_rgb_fwd(x, weight, bias, prev=None, blend=1.0):
    """-> y [B, K, H, W] = bias + the 1x1 convolution of x [B, C, H, W] with weight [K, C]; with prev [B, K, H/2, W/2]:
    torch.lerp(prev upsampled 2x (nearest), that, blend)"""
    _style_rgb_f32("style_to_rgb_fwd", x, weight, bias, prev)
    if x.dim() != 4 or weight.dim() < 2:
        raise ValueError("sivae_hip.style_to_rgb_fwd: expected x [B, C, H, W] and weight [K, C]")
    K = weight.shape[0]
    B, C, H, W, K = _style_rgb_dims("style_to_rgb_fwd", x, (x.shape[0], K, x.shape[2], x.shape[3]), weight, bias, True)
    _style_f32("style_to_rgb_fwd", x, weight, bias, prev)
    if prev is not None and (H % 2 or W % 2 or tuple(prev.shape) != (B, K, H // 2, W // 2)):
        raise ValueError("sivae_hip.style_to_rgb_fwd: prev must be [B, K, H/2, W/2] of an even H, W, got %s"
                         % (tuple(prev.shape),))
    y = torch.empty((B, K, H, W), dtype=torch.float32, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_to_rgb_fwd", _p(x), _p(weight), _p(bias), _p(prev), float(blend), _p(y), B, C, H, W, K, _s(x))
    if t0 is not None:
        timer_end(t0, "rgb_to_fwd_kernel", 2.0 * K * x.numel())
    return y


def style_to_rgb_bwd(dy, x, weight, has_prev=False, blend=1.0, want_dx=True, want_dw=True, want_dbias=True,
                     want_dprev=True):
    """-> (dx, dw [K, C], dbias [K], dprev [B, K, H/2, W/2]), None for what is not wanted (and for dprev of a forward
    without prev)"""
    _style_rgb_f32("style_to_rgb_bwd", dy, x, weight)
    if x.dim() != 4 or dy.dim() != 4 or weight.dim() < 2:
        raise ValueError("sivae_hip.style_to_rgb_bwd: expected dy [B, K, H, W], x [B, C, H, W] and weight [K, C]")
    B, C, H, W, K = _style_rgb_dims("style_to_rgb_bwd", x, dy, weight, weight[:, 0], True)
    _style_f32("style_to_rgb_bwd", dy, x, weight)
    has_prev = bool(has_prev)
    want_dprev = bool(want_dprev) and has_prev
    if has_prev and (H % 2 or W % 2):
        raise ValueError("sivae_hip.style_to_rgb_bwd: a blended forward has an even H and W, got %d x %d" % (H, W))
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty((K, C), dtype=torch.float32, device=x.device) if want_dw else None
    dbias = torch.empty(K, dtype=torch.float32, device=x.device) if want_dbias else None
    dprev = torch.empty((B, K, H // 2, W // 2), dtype=torch.float32, device=x.device) if want_dprev else None
    ws = workspace(_lib.load().sivae_to_rgb_bwd_workspace_bytes(B, C, H, W, K), x.device) if (want_dw or want_dbias) else None
    t0 = timer_begin()
    _lib.call("sivae_to_rgb_bwd", _p(dy), _p(x), _p(weight), int(has_prev), float(blend), _p(dx), _p(dw), _p(dbias),
              _p(dprev), B, C, H, W, K, _p(ws), 0 if ws is None else ws.numel(), _s(x))
    if t0 is not None:
        timer_end(t0, "rgb_to_bwd_kernel", 4.0 * K * x.numel())
    return dx, dw, dbias, dprev


def style_from_rgb_fwd(img, weight, bias, pool=False, other=None, blend=1.0):
    """-> y [B, C, Ho, Wo] = lrelu_0.2(lrelu_0.2(bias + the 1x1 convolution of img [B, K, H, W] with weight [C, K])), on the
    2 x 2 average of img with pool (Ho, Wo = H/2, W/2); with other [B, C, Ho, Wo]: torch.lerp(that, other, blend)"""
    _style_rgb_f32("style_from_rgb_fwd", img, weight, bias, other)
    if img.dim() != 4 or weight.dim() < 2:
        raise ValueError("sivae_hip.style_from_rgb_fwd: expected img [B, K, H, W] and weight [C, K]")
    pool = bool(pool)
    Bi, _, Hi, Wi = img.shape
    fshape = (Bi, weight.shape[0], Hi // 2, Wi // 2) if pool else (Bi, weight.shape[0], Hi, Wi)
    B, C, H, W, K = _style_rgb_dims("style_from_rgb_fwd", fshape, img, weight, bias, False, pool)
    _style_f32("style_from_rgb_fwd", img, weight, bias, other)
    if other is not None and tuple(other.shape) != fshape:
        raise ValueError("sivae_hip.style_from_rgb_fwd: other must be %s, got %s" % (fshape, tuple(other.shape)))
    y = torch.empty(fshape, dtype=torch.float32, device=img.device)
    t0 = timer_begin()
    _lib.call("sivae_from_rgb_fwd", _p(img), _p(weight), _p(bias), int(pool), _p(other), float(blend), _p(y), B, C, H, W,
              K, _s(img))
    if t0 is not None:
        timer_end(t0, "rgb_from_fwd_kernel", 2.0 * K * y.numel())
    return y


def style_from_rgb_bwd(dy, img, weight, bias, pool=False, has_other=False, blend=1.0, want_dimg=True, want_dw=True,
                       want_dbias=True, want_dother=True):
    """-> (dimg like img, dw [C, K], dbias [C], dother like dy), None for what is not wanted (and for dother of a forward
    without other); the pre-activation is recomputed from img"""
    _style_rgb_f32("style_from_rgb_bwd", dy, img, weight, bias)
    if img.dim() != 4 or dy.dim() != 4 or weight.dim() < 2:
        raise ValueError("sivae_hip.style_from_rgb_bwd: expected dy [B, C, Ho, Wo], img [B, K, H, W] and weight [C, K]")
    pool, has_other = bool(pool), bool(has_other)
    B, C, H, W, K = _style_rgb_dims("style_from_rgb_bwd", dy, img, weight, bias, False, pool)
    _style_f32("style_from_rgb_bwd", dy, img, weight, bias)
    want_dother = bool(want_dother) and has_other
    dimg = torch.empty_like(img) if want_dimg else None
    dw = torch.empty((C, K), dtype=torch.float32, device=img.device) if want_dw else None
    dbias = torch.empty(C, dtype=torch.float32, device=img.device) if want_dbias else None
    dother = torch.empty_like(dy) if want_dother else None
    ws = workspace(_lib.load().sivae_from_rgb_bwd_workspace_bytes(B, C, H, W, K, int(pool)), img.device) \
        if (want_dw or want_dbias) else None
    t0 = timer_begin()
    _lib.call("sivae_from_rgb_bwd", _p(dy), _p(img), _p(weight), _p(bias), int(pool), int(has_other), float(blend),
              _p(dimg), _p(dw), _p(dbias), _p(dother), B, C, H, W, K, _p(ws), 0 if ws is None else ws.numel(), _s(img))
    if t0 is not None:
        timer_end(t0, "rgb_from_bwd_kernel", 6.0 * K * dy.numel())
    return dimg, dw, dbias, dother


# ------------------------------------------------------------------------------------------------ mapping networks, style assembly (mapping.hip)
def _map_f32(who, *tensors):
    _require_f32(who, "mapping", *tensors, dtype_first=True)  # (so that a wrong dtype is named as such wherever the tensor is)


def _map_rows(who, x, *same):
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("sivae_hip.%s: expected rows [B, Z] with B, Z >= 1, got %s" % (who, tuple(x.shape)))
    for t in same:
        if t is not None and t.shape != x.shape:
            raise ValueError("sivae_hip.%s: %s does not match %s" % (who, tuple(t.shape), tuple(x.shape)))
    return x.shape


def pixel_norm_fwd(x, eps=1e-8):
    """-> (y, r [B]): y = x r with r = 1 / sqrt(mean_z x^2 + eps) per row of x [B, Z]"""
    _map_f32("pixel_norm_fwd", x)
    B, Z = _map_rows("pixel_norm_fwd", x)
    y = torch.empty_like(x)
    r = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.call("sivae_pixel_norm_fwd", _p(x), _p(y), _p(r), B, Z, float(eps), _s(x))
    return y, r


def pixel_norm_bwd(dy, x, r):
    """-> dx = r dy - x r^3 mean_z(dy x)"""
    _map_f32("pixel_norm_bwd", dy, x, r)
    B, Z = _map_rows("pixel_norm_bwd", x, dy)
    if tuple(r.shape) != (B,):
        raise ValueError("sivae_hip.pixel_norm_bwd: r must be [B] = (%d,), got %s" % (B, tuple(r.shape)))
    dx = torch.empty_like(x)
    _lib.call("sivae_pixel_norm_bwd", _p(dy), _p(x), _p(r), _p(dx), B, Z, _s(x))
    return dx


def _slope(who, slope):
    slope = float(slope)
    if not 0.0 <= slope <= 1.0:
        raise ValueError("sivae_hip.%s: the LeakyReLU slope must be in [0, 1], got %r" % (who, slope))
    return slope


def linear_lrelu_fwd(x, w, bias=None, slope=0.2):
    """linear_fwd with LeakyReLU(slope) as the epilogue: y = v > 0 ? v : v slope, v = x W^T + b"""
    _require(x, w, bias)
    slope = _slope("linear_lrelu_fwd", slope)
    B, K = x.shape
    N = w.shape[0]
    ws = workspace(_lib.load().sivae_linear_workspace_bytes(B, K, N), x.device)
    y = torch.empty((B, N), dtype=torch.float32, device=x.device)
    t0 = timer_begin()
    _lib.call("sivae_linear_lrelu_fwd", _p(x), _p(w), _p(bias), _p(y), slope, B, K, N, _p(ws), ws.numel(), _s(x))
    if t0 is not None:
        timer_end(t0, "linear_fwd_kernel", 2.0 * B * K * N)
    return y


def lrelu_bias_bwd(dy, y=None, slope=0.2, want_dz=True, want_dbias=True, out=None):
    """-> (dz, dbias [N]): dz = dy (y > 0 ? 1 : slope) from the saved output y (None: no activation, dz is dy itself and
    nothing is copied) and dbias = sum_b dz (out: its destination); None for what is not wanted"""
    _map_f32("lrelu_bias_bwd", dy, y)
    slope = _slope("lrelu_bias_bwd", slope)
    B, N = _map_rows("lrelu_bias_bwd", dy, y)
    dz = torch.empty_like(dy) if (want_dz and y is not None) else None
    dbias = _out(out, (N,), dy.device) if want_dbias else None
    if dz is not None or dbias is not None:
        _lib.call("sivae_lrelu_bias_bwd", _p(dy), _p(y), slope, _p(dz), _p(dbias), B, N, _s(dy))
    if want_dz and y is None:
        dz = dy
    return dz, dbias


def _styles_cfg(who, L, has_s2, cutoff, psi, trunc_cutoff):
    L = int(L)
    if L < 1:
        raise ValueError("sivae_hip.%s: num_layers must be >= 1, got %d" % (who, L))
    cutoff = L if not has_s2 else int(cutoff)
    if not 0 <= cutoff <= L:
        raise ValueError("sivae_hip.%s: the mixing cutoff must be in [0, %d], got %d" % (who, L, cutoff))
    truncate = psi is not None
    trunc_cutoff = int(trunc_cutoff) if truncate else 0
    if not 0 <= trunc_cutoff <= L:
        raise ValueError("sivae_hip.%s: the truncation cutoff must be in [0, %d], got %d" % (who, L, trunc_cutoff))
    return L, cutoff, truncate, float(psi) if truncate else 1.0, trunc_cutoff


def styles_fwd(s, num_layers, s2=None, cutoff=None, avg=None, beta=None, psi=None, trunc_cutoff=None):
    """-> styles [B, L, Z] from s [B, Z] (model.py:176-200): with beta, avg [L, Z] <- lerp(avg, mean_b s, 1 - beta) IN
    PLACE first; with s2, the layers l >= cutoff take s2; with psi, styles[:, l] = lerp(avg[l], styles[:, l], psi) for
    l < trunc_cutoff"""
    _map_f32("styles_fwd", s, s2, avg)
    B, Z = _map_rows("styles_fwd", s, s2)
    if s2 is not None and cutoff is None:
        raise ValueError("sivae_hip.styles_fwd: s2 needs the mixing cutoff")
    if psi is not None and trunc_cutoff is None:
        raise ValueError("sivae_hip.styles_fwd: psi needs the truncation cutoff")
    L, cutoff, truncate, psi, trunc_cutoff = _styles_cfg("styles_fwd", num_layers, s2 is not None, cutoff, psi, trunc_cutoff)
    update = beta is not None
    if (update or truncate) and avg is None:
        raise ValueError("sivae_hip.styles_fwd: beta and psi need the running average avg [L, Z]")
    if avg is not None and tuple(avg.shape) != (L, Z):
        raise ValueError("sivae_hip.styles_fwd: avg must be [L, Z] = (%d, %d), got %s" % (L, Z, tuple(avg.shape)))
    weight = 1.0 - float(beta) if update else 0.0  # (formed in double, as the reference's 1.0 - dlatent_avg_beta)
    if not 0.0 <= weight <= 1.0:
        raise ValueError("sivae_hip.styles_fwd: beta must be in [0, 1], got %r" % (beta,))
    out = torch.empty((B, L, Z), dtype=torch.float32, device=s.device)
    _lib.call("sivae_styles_fwd", _p(s), _p(s2), cutoff, _p(avg), int(update), weight, int(truncate), psi, trunc_cutoff,
              _p(out), B, L, Z, _s(s))
    return out


def styles_bwd(dstyles, has_s2=False, cutoff=None, psi=None, trunc_cutoff=None, want_ds=True, want_ds2=True):
    """-> (ds, ds2): the coefficient-weighted sums of dstyles [B, L, Z] over each source's layers; None for what is not
    wanted (and for ds2 of a forward without s2)"""
    _map_f32("styles_bwd", dstyles)
    if dstyles.dim() != 3 or min(dstyles.shape) < 1:
        raise ValueError("sivae_hip.styles_bwd: expected dstyles [B, L, Z], got %s" % (tuple(dstyles.shape),))
    B, L, Z = dstyles.shape
    has_s2 = bool(has_s2)
    L, cutoff, truncate, psi, trunc_cutoff = _styles_cfg("styles_bwd", L, has_s2, cutoff, psi, trunc_cutoff)
    ds = torch.empty((B, Z), dtype=torch.float32, device=dstyles.device) if want_ds else None
    ds2 = torch.empty((B, Z), dtype=torch.float32, device=dstyles.device) if (want_ds2 and has_s2) else None
    if ds is not None or ds2 is not None:
        _lib.call("sivae_styles_bwd", _p(dstyles), int(has_s2), cutoff, int(truncate), psi, trunc_cutoff, _p(ds), _p(ds2),
                  B, L, Z, _s(dstyles))
    return ds, ds2


# ------------------------------------------------------------------------------------------------ multi-tensor launches (multi_tensor.hip)
def _mt_f32(who, lists):
    """the tensor lists of a multi-tensor call: same length, and per index float32, contiguous, on ONE ROCm device and
    of one element count -> (device, element counts)"""
    if len({len(l) for l in lists}) > 1:
        raise ValueError("sivae_hip.%s: the tensor lists differ in length: %s" % (who, [len(l) for l in lists]))
    dev = None
    for ts in zip(*lists):
        for t in ts:
            _require_f32(who, "multi-tensor", t, skip_none=False)
            if t.numel() != ts[0].numel():
                raise ValueError("sivae_hip.%s: element counts differ: %s against %s"
                                 % (who, tuple(t.shape), tuple(ts[0].shape)))
            dev = dev or t.device
            if t.device != dev:
                raise ValueError("sivae_hip.%s: tensors on %s and on %s" % (who, dev, t.device))
    return dev, np.array([t.numel() for t in lists[0]], dtype=np.uintp)


def _mt_addresses(tensors):
    return np.array([t.data_ptr() for t in tensors], dtype=np.uint64)


def _np(a):
    return ctypes.c_void_p(a.ctypes.data)


def mt_launches(numel):
    """launches a multi-tensor call makes for these element counts (host only)"""
    n = np.ascontiguousarray(numel, dtype=np.uintp)
    rc = _lib.load().sivae_mt_launches(_np(n), len(n))
    if rc < 0:
        raise _lib.SivaeError("sivae_mt_launches", rc)
    return rc


def mt_lreq_adam(params, grads, states, step_sizes, beta2, eps):
    """One LREQAdam step of every listed tensor in place (params and states = exp_avg_sq are written, grads are read):
    v <- beta2 v + (1 - beta2) g g;  p <- p - step_sizes[t] g / (sqrt(v) + eps).  step_sizes: one Python float per tensor
    (lr sqrt(1 - beta2^step) coef, formed in double).  On the current stream of the tensors' device; nothing is
    allocated on the device, copied or synchronised.  -> the number of launches"""
    if len(step_sizes) != len(params):
        raise ValueError("sivae_hip.mt_lreq_adam: %d step sizes for %d tensors" % (len(step_sizes), len(params)))
    dev, n = _mt_f32("mt_lreq_adam", (params, grads, states))
    if dev is None:
        return 0
    p, g, v = _mt_addresses(params), _mt_addresses(grads), _mt_addresses(states)
    s = np.array(step_sizes, dtype=np.float64).astype(np.float32)
    _lib.call("sivae_mt_lreq_adam", _np(p), _np(g), _np(v), _np(n), _np(s), len(n), float(beta2), float(1.0 - beta2),
              float(eps), _s(params[0]))
    return mt_launches(n)


def mt_lerp_(dst, src, weight):
    """dst[t].lerp_(src[t], weight) for every listed pair in place, torch's formula.  -> the number of launches"""
    dev, n = _mt_f32("mt_lerp_", (dst, src))
    if dev is None:
        return 0
    d, q = _mt_addresses(dst), _mt_addresses(src)
    _lib.call("sivae_mt_lerp", _np(d), _np(q), _np(n), len(n), float(weight), _s(dst[0]))
    return mt_launches(n)


class _SwitchWatch(type(sys)):
    """this module's type: assigning any of its attributes (ops.WINO4 = False, monkeypatch.setattr(ops, ...), dp's
    ops.SYNC_BN = sync) forgets the memoised routes"""

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        _routes.clear()


sys.modules[__name__].__class__ = _SwitchWatch
