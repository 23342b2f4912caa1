"""Thin torch-tensor wrappers over the C ABI (include/tfc_gan.h). torch is used for device memory and streams only.

Activations are torch tensors of physical shape [N, H, W, pitch] (NHWC); a `View` names a channel window
[coff, coff + C) of such a buffer, which is how skip connections share one concat buffer without copies.
"""
import ctypes
import os
from dataclasses import dataclass

import torch

from . import _lib, parallel
from ._lib import (DT_BF16, DT_BF16X3, DT_F32, EP_ACCUM, EP_BIAS, EP_LEAKY, EP_RELU, EP_STATS, EP_TANH_NCHW, OP_CONV, OP_CONV2, OP_CONV3, OP_CONV3R, OP_CONVT, OP_PADCONV,
                   OP_UPCONV, check)


def lib():
    return _lib.load()


class batch_invariant_scope:
    """`with batch_invariant_scope(x)`: x = None leaves the process's batch-invariant setting (_lib.set_batch_invariant) alone, True / False
    overrides it inside the block -- for every thread and stream that launches kernels meanwhile"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = _lib.get_batch_invariant()
        if self.on is not None:
            _lib.set_batch_invariant(self.on)

    def __exit__(self, *exc):
        if self.on is not None:
            _lib.set_batch_invariant(self.prev)
        return False


def torch_dtype(dt):
    return torch.bfloat16 if dt == DT_BF16 else torch.float32


BF16X3 = "bf16x3"                   # the third compute mode: fp32 storage, convolutions split into bf16 hi / lo on the bf16 matrix cores


def dt_of(dtype):
    if isinstance(dtype, str):
        if dtype == BF16X3:
            return DT_BF16X3
    elif dtype == torch.bfloat16:
        return DT_BF16
    elif dtype == torch.float32:
        return DT_F32
    raise ValueError(f"compute dtype must be torch.bfloat16, torch.float32 or \"bf16x3\", got {dtype!r}")


def pad8(c):
    return (c + 7) // 8 * 8


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.TfcError("libtfcgan_hip kernels need CUDA/HIP tensors; got a CPU tensor "
                                "(there is no CPU fallback in this package)")


@dataclass
class View:
    """Channel window of an NHWC buffer."""
    t: torch.Tensor      # [N, H, W, pitch]
    C: int               # logical channels
    coff: int = 0

    @property
    def N(self):
        return self.t.shape[0]

    @property
    def H(self):
        return self.t.shape[1]

    @property
    def W(self):
        return self.t.shape[2]

    @property
    def pitch(self):
        return self.t.shape[3]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.coff * self.t.element_size())

    def sub(self, coff, C):
        return View(self.t, C, self.coff + coff)


class ZeroArena:
    """Small zero-initialised fp32 scratch (InstanceNorm statistics, bias-gradient partials, loss scalars) for one training step:
    ONE fill per step instead of one torch.zeros launch per buffer (~33 per step). `begin()` re-zeroes the part handed out since
    the previous begin(); views stay valid until the next begin() -- i.e. for the rest of the step that took them."""

    def __init__(self, device, nfloats=1 << 20):
        self.buf = torch.zeros(nfloats, dtype=torch.float32, device=device)
        self.used = 0
        self.active = False

    def begin(self):
        if self.used:
            self.buf[:self.used].zero_()
        self.used = 0
        self.active = True

    def take(self, shape):
        n = 1
        for d in shape:
            n *= int(d)
        n4 = (n + 63) // 64 * 64                                  # 256-byte granules: every view stays 16-byte aligned
        if self.used + n4 > self.buf.numel():
            return torch.zeros(shape, dtype=torch.float32, device=self.buf.device)
        v = self.buf[self.used:self.used + n].view(shape)
        self.used += n4
        return v


_ARENA = {}


def arena_begin(device):
    """start a step: from now on zeros_f32() on this device is served from the step arena"""
    dev = torch.device(device)
    a = _ARENA.get(dev)
    if a is None:
        a = _ARENA[dev] = ZeroArena(dev)
    a.begin()
    return a


def arena_end(device):
    """end of the step: later zeros_f32() calls (module-level forward / backward outside TrainStep) get buffers of their own"""
    a = _ARENA.get(torch.device(device))
    if a is not None:
        a.active = False


def zeros_f32(shape, device):
    a = _ARENA.get(torch.device(device))
    return a.take(tuple(shape)) if a is not None and a.active else torch.zeros(shape, dtype=torch.float32, device=device)


def new_act(N, H, W, C, dt, device, zero=False):
    f = torch.zeros if zero else torch.empty
    return View(f((N, H, W, C), dtype=torch_dtype(dt), device=device), C)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# Partial-sum scratch of the reducing entry points (include/tfc_gan.h, "DETERMINISM"): sums that cross workgroups leave each workgroup as a partial
# in a fixed slot of this buffer and are added in a fixed order behind the kernel -- no float atomics anywhere on the training path. One buffer per
# (device, stream): launches on one stream are ordered, and a kernel's partials are consumed by the reduction queued right behind it.
_PART_WS = {}


def part_ws(device):
    key = (torch.device(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _PART_WS.get(key)
    if ws is None:
        ws = _PART_WS[key] = torch.empty(lib().tfc_part_ws_floats(), dtype=torch.float32, device=device)
    return ctypes.c_void_p(ws.data_ptr())


OUT_HW = {OP_CONV: lambda h: h - 1, OP_PADCONV: lambda h: h, OP_CONVT: lambda h: 2 * h, OP_UPCONV: lambda h: 2 * h, OP_CONV3: lambda h: h,
          OP_CONV2: lambda h: h // 2, OP_CONV3R: lambda h: h}


# ---- convolution family ---------------------------------------------------------------------------------------
def packed_bytes(dt, op, pas, Cin, Cout):
    return lib().tfc_conv_packed_bytes(dt, op, pas, Cin, Cout)


def pack_weight(dt, op, pas, w, Cin, Cout, scale=None, out=None):
    """w: torch-layout fp32 weight on the GPU; returns a uint8 tensor holding the MFMA operand stream."""
    require_gpu(w)
    assert w.dtype == torch.float32 and w.is_contiguous()
    nbytes = packed_bytes(dt, op, pas, Cin, Cout)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    assert out.numel() >= nbytes
    check(lib().tfc_conv_pack(stream_ptr(), dt, op, pas, _p(w), _p(scale), _p(out), Cin, Cout), "tfc_conv_pack")
    return out


class PackPlan:
    """All operand streams of one network packed by a single launch. jobs: list of (op, pass, weight fp32 tensor, Cin, Cout);
    the weight tensors and the returned stream buffers must stay where they are (flat parameter buffer, persistent streams)."""

    def __init__(self, dt, jobs):
        self.dt = dt
        dev = jobs[0][2].device
        n = len(jobs)
        self.streams = [torch.empty(packed_bytes(dt, op, pas, cin, cout), dtype=torch.uint8, device=dev) for op, pas, w, cin, cout in jobs]
        self.keep = [w for _, _, w, _, _ in jobs]
        host = (ctypes.c_uint8 * lib().tfc_pack_plan_bytes(n))()
        nblk = ctypes.c_int(0)
        ci = lambda xs: (ctypes.c_int * n)(*xs)  # noqa: E731
        cp = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        nj = lib().tfc_pack_plan_build(dt, n, ci([j[0] for j in jobs]), ci([j[1] for j in jobs]), cp(self.keep), cp(self.streams),
                                       ci([j[3] for j in jobs]), ci([j[4] for j in jobs]), ctypes.cast(host, ctypes.c_void_p), ctypes.byref(nblk))
        if nj < 0:
            check(nj, "tfc_pack_plan_build")
        self.njobs, self.nblocks = nj, nblk.value
        self.plan = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)

    def run(self):
        check(lib().tfc_conv_pack_planned(stream_ptr(), self.dt, _p(self.plan), self.njobs, self.nblocks), "tfc_conv_pack_planned")


def conv_fwd(dt, op, x: View, Cin, Cout, packed, y: View = None, bias=None, stats=None, out_nchw=None, flags=0, oscale=None):
    if bias is not None:
        flags |= EP_BIAS
    if stats is not None:
        flags |= EP_STATS
    if out_nchw is not None:
        flags |= EP_TANH_NCHW
    check(lib().tfc_conv_fwd(stream_ptr(), dt, op, x.ptr, x.pitch, x.N, x.H, x.W, Cin, Cout, _p(packed),
                             None if y is None else y.ptr, 0 if y is None else y.pitch, _p(bias), _p(stats), _p(out_nchw), _p(oscale), flags,
                             part_ws(x.t.device) if stats is not None else None), "tfc_conv_fwd")


def first_block_bwd_supported(dt, Cin, Cout):
    if os.environ.get("TFC_NO_FUSED_FIRST_BWD"):                  # A/B knob for profiling
        return False
    return bool(lib().tfc_first_block_bwd_supported(dt, Cin, Cout))


def first_block_fwd_supported():
    return not os.environ.get("TFC_NO_FUSED_FIRST_FWD")           # A/B knob for profiling (read per call)


def conv_first_fwd(dt, x: View, Cin, Cout, packed, y: View, bias=None, oscale=None, flags=0, sign_mask=None):
    """first convolution of a network (8 padded input channels -> 64) on the weights-stationary kernel; sign_mask: uint8 [N, H-1, W-1, 8] that receives
    one bit per stored value (> 0) for the fused backward of the block"""
    if bias is not None:
        flags |= EP_BIAS
    check(lib().tfc_conv_first_fwd(stream_ptr(), dt, x.ptr, x.pitch, x.N, x.H, x.W, Cin, Cout, _p(packed), y.ptr, y.pitch, _p(bias), _p(oscale), flags,
                                   _p(sign_mask)), "tfc_conv_first_fwd")


def first_block_fwd(dt, x: View, Cin, Cout, packed, out: View, bias=None, oscale=None, slope=0.2, act_after_rounding=False, sign_mask=None):
    """conv -> [+bias, x 1/sigma] -> LeakyReLU -> BlurPool(stride 2) of a first block in one kernel (the conv output is never written); `out` may be a
    channel window of a wider buffer"""
    check(lib().tfc_first_block_fwd(stream_ptr(), dt, x.ptr, x.pitch, x.N, x.H, x.W, Cin, Cout, _p(packed), _p(bias), _p(oscale), slope,
                                    1 if act_after_rounding else 0, out.ptr, out.pitch, _p(sign_mask)), "tfc_first_block_fwd")


def first_block_bwd_wgrad(dt, x: View, y: View, dy_pooled: View, Cin, Cout, dw, slope=0.2, accumulate=False, ws=None, bias_sums=None, sign_mask=None):
    """[BlurPool]^T -> LeakyReLU' -> weight (+ bias) gradient of the first block in one kernel: the gradient of the conv output is never written.
    sign_mask (from conv_first_fwd): read instead of the stored activation y (8 bytes per pixel instead of 128)"""
    nbytes = lib().tfc_conv_wgrad_ws_bytes(OP_CONV, Cin, Cout)
    if ws is None or ws.numel() * ws.element_size() < nbytes:
        nbig = lib().tfc_conv_wgrad_ws_bytes(OP_CONV, 1024, 512)
        ws = torch.zeros(max(nbytes, nbig), dtype=torch.uint8, device=x.t.device)
    assert dw.dtype == torch.float32 and dw.is_contiguous()
    check(lib().tfc_first_block_bwd_wgrad(stream_ptr(), dt, x.ptr, x.pitch, None if y is None else y.ptr, 0 if y is None else y.pitch, dy_pooled.ptr,
                                          dy_pooled.pitch, x.N, x.H, x.W, Cin, Cout, slope, _p(ws), _p(dw), 1 if accumulate else 0, _p(bias_sums),
                                          part_ws(x.t.device) if bias_sums is not None else None, _p(sign_mask)), "tfc_first_block_bwd_wgrad")
    return ws


def conv_dgrad_image(dt, dy: View, N, H, W, Cin, w, oscale, nch):
    """first discriminator conv, gradient w.r.t. its first `nch` input channels as fp32 NCHW [N,nch,H,W] (bf16 path)"""
    out = torch.empty((N, nch, H, W), dtype=torch.float32, device=dy.t.device)
    check(lib().tfc_conv_dgrad_image(stream_ptr(), dt, dy.ptr, dy.pitch, N, H, W, Cin, w.shape[0], _p(w), _p(oscale), nch, _p(out)),
          "tfc_conv_dgrad_image")
    return out


def upconv_head_fwd(dt, x: View, w, bias, out_nchw):
    """generator head (upsample + pad + conv(128 -> C<=4) + tanh), bf16: x NHWC View with 128 channels, w torch-layout fp32"""
    Cout = w.shape[0]
    check(lib().tfc_upconv_head_fwd(stream_ptr(), dt, x.ptr, x.pitch, x.N, x.H, x.W, 128, Cout, _p(w), _p(bias), _p(out_nchw)),
          "tfc_upconv_head_fwd")


def upconv_head_dgrad(dt, dy: View, N, H, W, w, dx: View):
    """input gradient of the generator head (bf16, 128 input channels, <= 8 output channels): dy NHWC8 at 2H x 2W -> dx [N,H,W,128]"""
    check(lib().tfc_upconv_head_dgrad(stream_ptr(), dt, dy.ptr, dy.pitch, N, H, W, 128, w.shape[0], _p(w), dx.ptr, dx.pitch), "tfc_upconv_head_dgrad")


def patchgan_head_fwd(dt, x: View, w, y: View):
    check(lib().tfc_patchgan_head_fwd(stream_ptr(), dt, x.ptr, x.pitch, x.N, x.H, x.W, x.C, _p(w), y.ptr, y.pitch), "tfc_patchgan_head_fwd")


# Scratch of the reflect-padded convolution's input gradient (the padded gradient that its fold pass reads; include/tfc_gan.h): one buffer per
# (device, stream), as for part_ws, grown to the largest call so far and handed to the library for the calling thread in front of each call.
_DGRAD_WS = {}


def _dgrad_ws(dt, op, N, H, W, Cin, Cout, device):
    need = lib().tfc_conv_dgrad_ws_bytes(dt, op, N, H, W, Cin, Cout)
    if not need:
        return
    key = (torch.device(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _DGRAD_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _DGRAD_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    check(lib().tfc_conv_dgrad_set_ws(_p(ws), ws.numel()), "tfc_conv_dgrad_set_ws")


def conv_dgrad(dt, op, dy: View, N, H, W, Cin, Cout, packed, dx: View, accumulate=False, oscale=None):
    if op == OP_CONV3R:
        _dgrad_ws(dt, op, N, H, W, Cin, Cout, dy.t.device)
    check(lib().tfc_conv_dgrad(stream_ptr(), dt, op, dy.ptr, dy.pitch, N, H, W, Cin, Cout, _p(packed), dx.ptr, dx.pitch,
                               _p(oscale), EP_ACCUM if accumulate else 0), "tfc_conv_dgrad")


def conv_wgrad(dt, op, x: View, dy: View, Cin, Cout, dw, accumulate=False, ws=None):
    nbytes = lib().tfc_conv_wgrad_ws_bytes(op, Cin, Cout)
    if ws is None or ws.numel() * ws.element_size() < nbytes:
        nbig = lib().tfc_conv_wgrad_ws_bytes(op, 1024, 512)       # the largest layer of the path, so one buffer serves every call
        ws = torch.zeros(max(nbytes, nbig), dtype=torch.uint8, device=x.t.device)   # zero ONCE: the kernels re-zero the accumulator
    assert dw.dtype == torch.float32 and dw.is_contiguous()
    check(lib().tfc_conv_wgrad(stream_ptr(), dt, op, x.ptr, x.pitch, dy.ptr, dy.pitch, x.N, x.H, x.W, Cin, Cout, _p(ws), _p(dw),
                               1 if accumulate else 0), "tfc_conv_wgrad")
    return ws


# ---- fused norm / activation / blur-pool ----------------------------------------------------------------------
def act_fwd(dt, x: View, y: View, stats=None, slope=0.2, pool=0, drop_p=0.0, seed=0, stats_out=None):
    check(lib().tfc_act_fwd(stream_ptr(), dt, x.ptr, x.pitch, x.N, x.H, x.W, x.C, _p(stats), 0 if stats is None else 1, slope, pool,
                            drop_p, seed & 0xFFFFFFFF, y.ptr, y.pitch, _p(stats_out), part_ws(x.t.device) if stats_out is not None else None), "tfc_act_fwd")


def norm_add_fwd(dt, x: View, res: View, stats, y: View):
    """y = res + InstanceNorm(x; stats): the second half of a residual block in one pass (y may be x or res)"""
    check(lib().tfc_norm_add_fwd(stream_ptr(), dt, x.ptr, x.pitch, res.ptr, res.pitch, x.N, x.H, x.W, x.C, _p(stats), y.ptr, y.pitch), "tfc_norm_add_fwd")


def act_bwd(dt, mode, dy: View, x: View, N, H, W, C, dx: View = None, stats=None, slope=0.2, pool=0, drop_p=0.0, seed=0, rstats=None):
    check(lib().tfc_act_bwd(stream_ptr(), dt, mode, dy.ptr, dy.pitch, None if x is None else x.ptr, 0 if x is None else x.pitch,
                            N, H, W, C, _p(stats), 0 if stats is None else 1, slope, pool, drop_p, seed & 0xFFFFFFFF, _p(rstats),
                            None if dx is None else dx.ptr, 0 if dx is None else dx.pitch, part_ws(dy.t.device) if rstats is not None else None),
          "tfc_act_bwd")


def act_bwd_signs(dt, dy: View, sign_mask, N, H, W, C, dx: View, slope=0.2, rstats=None):
    """act_bwd(mode 0, pool 2) of a first block whose conv output was never stored: LeakyReLU' from the sign words of first_block_fwd / conv_first_fwd"""
    check(lib().tfc_act_bwd_signs(stream_ptr(), dt, dy.ptr, dy.pitch, _p(sign_mask), N, H, W, C, slope, _p(rstats), dx.ptr, dx.pitch,
                                  part_ws(dy.t.device) if rstats is not None else None), "tfc_act_bwd_signs")


def dropout_mask(n, drop_p, seed, device):
    out = torch.empty(n, dtype=torch.uint8, device=device)
    check(lib().tfc_dropout_mask(stream_ptr(), _p(out), n, drop_p, seed & 0xFFFFFFFF), "tfc_dropout_mask")
    return out


# ---- layout plumbing ------------------------------------------------------------------------------------------
def pack_nhwc8(dt, a, b=None):
    """NCHW fp32 a [N,Ca,H,W] (and b) -> NHWC with 8 channels."""
    require_gpu(a, b)
    a = a.contiguous().float()
    N, Ca, H, W = a.shape
    Cb = 0
    if b is not None:
        b = b.contiguous().float()
        Cb = b.shape[1]
    out = new_act(N, H, W, 8, dt, a.device)
    check(lib().tfc_pack_nhwc8(stream_ptr(), dt, _p(a), Ca, _p(b), Cb, out.ptr, N, H, W), "tfc_pack_nhwc8")
    return out


def unpack_nchw(dt, v: View, C, out=None, alpha=1.0, beta=0.0, c0=0):
    N, H, W = v.N, v.H, v.W
    if out is None:
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=v.t.device)
    check(lib().tfc_unpack_nchw(stream_ptr(), dt, v.ptr, v.pitch, c0, C, _p(out), N, H, W, alpha, beta), "tfc_unpack_nchw")
    return out


def tanh_bwd_pack(dt, g, y, dbias=None):
    N, C, H, W = g.shape
    out = new_act(N, H, W, 8, dt, g.device)
    check(lib().tfc_tanh_bwd_pack(stream_ptr(), dt, _p(g), _p(y), out.ptr, _p(dbias), N, C, H, W, part_ws(g.device) if dbias is not None else None),
          "tfc_tanh_bwd_pack")
    return out


def colsum(dt, v: View, out):
    rows = v.N * v.H * v.W
    check(lib().tfc_colsum(stream_ptr(), dt, v.ptr, rows, v.pitch, v.C, _p(out), part_ws(v.t.device) if rows >= 4096 else None), "tfc_colsum")


def cast_from_f32(dt, x):
    y = torch.empty(x.shape, dtype=torch_dtype(dt), device=x.device)
    check(lib().tfc_cast(stream_ptr(), dt, 0, _p(x.contiguous()), _p(y), x.numel()), "tfc_cast")
    return y


def cast_to_f32(dt, x):
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().tfc_cast(stream_ptr(), dt, 1, _p(x.contiguous()), _p(y), x.numel()), "tfc_cast")
    return y


def axpby(out, x, y, a, b):
    check(lib().tfc_axpby(stream_ptr(), _p(out), _p(x), _p(y), out.numel(), a, b), "tfc_axpby")
    return out


# ---- spectral norm --------------------------------------------------------------------------------------------
def spectral_norm_step(W, u, v, sigma2, power_iter=True, ws=None):
    R = W.shape[0]
    K = W.numel() // R
    need = lib().tfc_spectral_norm_batched_ws_floats(1, (ctypes.c_int * 1)(R), (ctypes.c_int * 1)(K))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=W.device)
    check(lib().tfc_spectral_norm_step(stream_ptr(), _p(W), _p(u), _p(v), _p(sigma2), _p(ws), R, K, 1 if power_iter else 0),
          "tfc_spectral_norm_step")


def spectral_norm_step_batched(Ws, us, vs, sigma2s, power_iter=True, u_snaps=None, v_snaps=None, ws=None):
    """one power iteration (u <- norm(W v), v <- norm(W^T u), sigma = u.W v) for up to 4 layers in 3 launches"""
    n = len(Ws)
    R = [int(W.shape[0]) for W in Ws]
    K = [int(W.numel() // W.shape[0]) for W in Ws]
    Ra, Ka = (ctypes.c_int * n)(*R), (ctypes.c_int * n)(*K)
    need = lib().tfc_spectral_norm_batched_ws_floats(n, Ra, Ka)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=Ws[0].device)

    def arr(ts):
        return None if ts is None else (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    check(lib().tfc_spectral_norm_step_batched(stream_ptr(), n, arr(Ws), arr(us), arr(vs), arr(sigma2s), arr(u_snaps), arr(v_snaps),
                                               Ra, Ka, _p(ws), 1 if power_iter else 0), "tfc_spectral_norm_step_batched")
    return ws


def spectral_norm_bwd(G, W, u, v, sigma2, gout, accumulate=False):
    R = W.shape[0]
    K = W.numel() // R
    ws = torch.empty(256, dtype=torch.float32, device=W.device)    # per-workgroup partials of <G, W> (doubles), added in a fixed order
    check(lib().tfc_spectral_norm_bwd(stream_ptr(), _p(G), _p(W), _p(u), _p(v), _p(sigma2), _p(ws), _p(gout), R, K,
                                      1 if accumulate else 0), "tfc_spectral_norm_bwd")


# ---- loss heads -----------------------------------------------------------------------------------------------
def patch16_triplet(fake, real, neg_idx, want_grad=True, gscale=1.0):
    """fake/real: fp32 NCHW [N,C,256,256]; neg_idx: 16 ints. Returns (loss[1], dfake or None). The 4x4 grid of patch_triplet."""
    assert len(neg_idx) == 16, "make_16_patches: 16 negative indices (reference :233-251)"
    return patch_triplet(fake, real, neg_idx, want_grad, gscale)


def patch_triplet(fake, real, neg_idx, want_grad=True, gscale=1.0):
    """The triplet head on a 2x2 or 4x4 patch grid, inferred from len(neg_idx) (4: PATCH-4 / GLO-4, reference TFCGAN_multigpu_patchFFT.py:468-481;
    16: PATCH-16, reference TFCGAN_multigpu_patchFFT_16P.py:558-583). fake/real: fp32 NCHW [N,C,256,256]. Returns (loss[1], dfake or None)."""
    n = len(neg_idx)
    if n not in (4, 16):
        raise _lib.TfcError(f"patch_triplet: {n} negative indices (the patch grid has 4 or 16 patches)")
    require_gpu(fake, real)
    assert fake.shape == real.shape and fake.shape[2:] == (256, 256), "the reference hard-codes the patch offsets of 256x256 images"
    fake = fake.contiguous().float()
    real = real.contiguous().float()
    N, C = fake.shape[:2]
    loss = torch.empty(1, dtype=torch.float32, device=fake.device)
    dfake = torch.empty_like(fake) if want_grad else None
    idx = (ctypes.c_int * n)(*[int(i) for i in neg_idx])
    check(lib().tfc_patch_triplet(stream_ptr(), _p(fake), _p(real), idx, 2 if n == 4 else 4, N, C, _p(loss), _p(dfake), gscale), "tfc_patch_triplet")
    return loss, dfake


_FFT_WS = {}


def _image_f32(img):
    """the image as the spectrum / temperature kernels read it: fp32, unit stride on W (any strides on N/C/H)"""
    require_gpu(img)
    if img.dtype != torch.float32:
        img = img.float()
    if img.stride(3) != 1:
        img = img.contiguous()
    return img


def _fft_scratch(device, need):
    """at least `need` bytes of row-pass scratch, one buffer per (device, stream): calls on a stream are ordered"""
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _FFT_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _FFT_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def fft_spectrum(img, S, wins_x, wins_y, shift=True, direct=False):
    """img: fp32 [N,C,H,W] (any strides on N/C/H, unit stride on W). Returns amp, pha [N*wins_x*wins_y, S, S//2+1].
    direct=True: the direct-DFT kernel (no scratch) instead of the LDS radix-4 FFT -- the tests cross-check the two."""
    img = _image_f32(img)
    N, C = img.shape[:2]
    assert img.shape[2] >= wins_y * S and img.shape[3] >= wins_x * S
    nwin = N * wins_x * wins_y
    amp = torch.empty((nwin, S, S // 2 + 1), dtype=torch.float32, device=img.device)
    pha = torch.empty_like(amp)
    ws = None if direct else _fft_scratch(img.device, lib().tfc_fft_spectrum_ws_bytes(S, nwin))
    check(lib().tfc_fft_spectrum(stream_ptr(), _p(img), img.stride(0), img.stride(1), img.stride(2), C, S, wins_x, wins_y, N,
                                 _p(amp), _p(pha), 1 if shift else 0, _p(ws)), "tfc_fft_spectrum")
    return amp, pha


def fft_spectrum_rect(img, H, row0=0, row_step=0, wins=1, shift=True):
    """Spectra of `wins` windows of H rows x 256 columns per image, window k starting at image row row0 + k * row_step (H in 2 .. 256; the regional
    FFT loss uses H = 100, rows 0 and 100). img: fp32 [N,C,h,w >= 256] (any strides on N/C/H, unit stride on W). Returns amp, pha [N*wins, H, 129]."""
    img = _image_f32(img)
    N, C, h, w = img.shape
    nwin = N * wins
    amp = torch.empty((nwin, max(H, 0), 129), dtype=torch.float32, device=img.device)
    pha = torch.empty_like(amp)
    ws = _fft_scratch(img.device, max(lib().tfc_fft_spectrum_rect_ws_bytes(H, nwin), 16))    # 0 bytes for a refused H: the call below says why
    check(lib().tfc_fft_spectrum_rect(stream_ptr(), _p(img), img.stride(0), img.stride(1), img.stride(2), C, h, w, H, row0, row_step, wins, N,
                                      _p(amp), _p(pha), 1 if shift else 0, _p(ws)), "tfc_fft_spectrum_rect")
    return amp, pha


BATCH_SCOPES = ("global", "shard")


def phased_scope(batch_scope, what):
    """does a batch-coupled operator run in phases with an exchange between them? batch_scope "global" (the default): the batch is the gathered batch
    of all ranks, so with active collectives (parallel.collectives_active) yes; "shard": each rank's own samples, as before the phases existed.
    Without active collectives both values take the unsplit entry point: same launches, same bits."""
    if batch_scope not in BATCH_SCOPES:
        raise _lib.TfcError(f"{what}: batch_scope={batch_scope!r} ('global': the batch of all ranks, 'shard': this rank's samples)")
    return batch_scope == "global" and parallel.collectives_active()


def batch_kl_sum(af, pf, ar, scale, out, batch_scope="global", group=None):
    """out[0] += scale * sum exp(t)(t - xa), out[1] += scale * sum exp(t)(t - xp) with t / xa / xp = log_softmax over dim 0 of ar / af / pf
    (contiguous fp32 [N, ...] of one shape; ar is the target of both terms, as in the reference's KL regional loss). batch_scope "global" on several
    ranks: the softmax runs over the entries of all ranks and the sums over this rank's terms (phased_scope)."""
    phased = phased_scope(batch_scope, "batch_kl_sum")
    require_gpu(af, pf, ar, out)
    for name, v in (("af", af), ("pf", pf), ("ar", ar)):
        if v.dtype != torch.float32 or not v.is_contiguous() or v.shape != af.shape or v.dim() < 1 or v.shape[0] < 1:
            raise _lib.TfcError(f"batch_kl_sum: {name} is {v.dtype} {tuple(v.shape)}, contiguous={v.is_contiguous()} "
                                f"(three contiguous fp32 tensors of one shape [N >= 1, ...])")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < 2:
        raise _lib.TfcError(f"batch_kl_sum: out is {out.dtype} with {out.numel()} elements (contiguous fp32, at least 2)")
    N = af.shape[0]
    M = af.numel() // N
    if not phased:
        check(lib().tfc_batch_kl_sum(stream_ptr(), _p(af), _p(pf), _p(ar), N, M, scale, _p(out)), "tfc_batch_kl_sum")
        return
    # the softmax over the batch of ALL ranks: first walk, exchange of the (max, sum) pairs, merge in rank order, second walk
    rec = torch.empty((3, M, 2), dtype=torch.float32, device=af.device)
    check(lib().tfc_batch_kl_stats(stream_ptr(), _p(af), _p(pf), _p(ar), N, M, _p(rec)), "tfc_batch_kl_stats")
    recs = parallel.all_gather_records(rec, group)
    check(lib().tfc_batch_kl_merge(stream_ptr(), _p(recs), recs.shape[0], M, _p(rec)), "tfc_batch_kl_merge")      # rec is free again: the global pairs
    check(lib().tfc_batch_kl_terms(stream_ptr(), _p(af), _p(pf), _p(ar), N, M, _p(rec), scale, _p(out)), "tfc_batch_kl_terms")


def logmag_mse(amp_a, amp_b, absolute=False):
    """per window mean squared (or absolute) difference of the log-magnitude spectra over the FULL S x S spectrum"""
    nwin, S = amp_a.shape[0], amp_a.shape[1]
    out = torch.empty(nwin, dtype=torch.float32, device=amp_a.device)
    fn = lib().tfc_logmag_mae if absolute else lib().tfc_logmag_mse
    check(fn(stream_ptr(), _p(amp_a), _p(amp_b), S, nwin, _p(out)), "tfc_logmag_mae" if absolute else "tfc_logmag_mse")
    return out


def vectorize_temps(img, lut):
    """img: fp32 [N,C,H,W] (unit stride on W); lut: fp32 [256] on the device. Returns [N,H,W] fp32 (channel 0 -> uint8 -> lut)."""
    img = _image_f32(img)
    N, _, H, W = img.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=img.device)
    check(lib().tfc_vectorize_temps(stream_ptr(), _p(img), img.stride(0), img.stride(2), N, H, W, _p(lut), _p(out)), "tfc_vectorize_temps")
    return out


def row_triplet(anchor, positive, negative, margin=1.0):
    """nn.TripletMarginLoss(margin, p=2) over the last dim of three equal-shape contiguous fp32 tensors -> scalar [1]."""
    require_gpu(anchor)
    assert anchor.shape == positive.shape == negative.shape
    a, p_, n = (t.float().contiguous() for t in (anchor, positive, negative))
    W = a.shape[-1]
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    check(lib().tfc_row_triplet(stream_ptr(), _p(a), _p(p_), _p(n), a.numel() // W, W, float(margin), _p(out)), "tfc_row_triplet")
    return out


def l1_sum(a, b, scale, out, zero_first=False):
    check(lib().tfc_l1_sum(stream_ptr(), _p(a), _p(b), a.numel(), scale, _p(out), 1 if zero_first else 0), "tfc_l1_sum")


def bce_relativistic(dt, a: View, b: View, mode, t1, t2=0.0, da: View = None, db: View = None, gscale=1.0):
    n = a.N * a.H * a.W
    loss = torch.empty(1, dtype=torch.float32, device=a.t.device)
    check(lib().tfc_bce_relativistic(stream_ptr(), dt, a.ptr, b.ptr, n, a.pitch, t1, t2, mode, _p(loss),
                                     None if da is None else da.ptr, None if db is None else db.ptr, gscale), "tfc_bce_relativistic")
    return loss


def adam_step(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0):
    check(lib().tfc_adam_step(stream_ptr(), _p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, step, gscale), "tfc_adam_step")


# ---- label plane + auxiliary classifier heads (csrc/debias.hip; the label-conditioned 4-patch scripts) ---------------------------------------------
AUX_CLASSES = (2, 4, 3)             # gender, ethnicity, age: reference TFCGAN_multigpu_patchFFT_debiased.py:218-220


def _ptr3(ts):
    return (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])


def _int3(v):
    return (ctypes.c_int * 3)(*[int(i) for i in v])


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.TfcError(f"{what} must be a contiguous fp32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    return t


def pack_nhwc8_labels(dt, img, labels, fc_w, fc_b):
    """torch.cat((img, fc(labels).view(N,1,H,W)), 1) as the NHWC8 activation of the compute dtype: channels 0..2 img, 3 the label plane, 4..7 zero"""
    require_gpu(img, labels, fc_w, fc_b)
    img = img.contiguous().float()
    labels = labels.contiguous().float()
    N, C, H, W = img.shape
    if C != 3 or tuple(labels.shape) != (N, 3) or tuple(fc_w.shape) != (H * W, 3) or tuple(fc_b.shape) != (H * W,):
        raise _lib.TfcError(f"pack_nhwc8_labels: img {tuple(img.shape)}, labels {tuple(labels.shape)}, fc.weight {tuple(fc_w.shape)}, fc.bias "
                            f"{tuple(fc_b.shape)} (expected [N,3,H,W], [N,3], [H*W,3], [H*W])")
    out = new_act(N, H, W, 8, dt, img.device)
    check(lib().tfc_pack_nhwc8_labels(stream_ptr(), dt, _p(img), _p(labels), _p(_f32c(fc_w, "fc.weight")), _p(_f32c(fc_b, "fc.bias")), out.ptr, N, H, W),
          "tfc_pack_nhwc8_labels")
    return out


def label_plane_bwd(g, labels, d_fc_w, d_fc_b, ch=3, accumulate=False):
    """g: fp32 NCHW input gradient [N,C,H,W] whose channel `ch` is the label plane's -> d fc.weight [H*W,3], d fc.bias [H*W] (written or accumulated)"""
    require_gpu(g, labels, d_fc_w, d_fc_b)
    N, C, H, W = g.shape
    labels = labels.contiguous().float()
    check(lib().tfc_label_plane_bwd(stream_ptr(), _p(_f32c(g, "g")), C, ch, _p(labels), _p(_f32c(d_fc_w, "d fc.weight")), _p(_f32c(d_fc_b, "d fc.bias")),
                                    N, H, W, 1 if accumulate else 0), "tfc_label_plane_bwd")


def aux_heads_fwd(dt, x: View, ws, bs, classes=AUX_CLASSES):
    """x: the packed discriminator input [N,H,W,8]; ws / bs: the three heads' weights [C_h, 6*H*W] and biases [C_h] (fp32) -> logits [N, sum C_h]"""
    require_gpu(x.t, *ws, *bs)
    logits = torch.empty((x.N, sum(classes)), dtype=torch.float32, device=x.t.device)
    check(lib().tfc_aux_heads_fwd(stream_ptr(), dt, x.ptr, x.pitch, x.N, x.H, x.W, _ptr3([_f32c(w, "head weight") for w in ws]),
                                  _ptr3([_f32c(b, "head bias") for b in bs]), _int3(classes), _p(logits), part_ws(x.t.device)), "tfc_aux_heads_fwd")
    return logits


def check_targets(targets, classes=AUX_CLASSES):
    """targets: anything that np.asarray turns into [N,3] whole numbers (host values) -> int32 numpy [N,3]; refuses values outside [0, C_h)"""
    import numpy as np
    a = np.asarray(targets.detach().cpu() if isinstance(targets, torch.Tensor) else targets)
    if a.ndim != 2 or a.shape[1] != 3:
        raise _lib.TfcError(f"labels: shape {a.shape} (expected [N,3]: gender, ethnicity, age)")
    r = np.rint(a.astype(np.float64))
    if not np.array_equal(r, a.astype(np.float64)):
        raise _lib.TfcError("labels: class indices must be whole numbers")
    for h, c in enumerate(classes):
        if r.shape[0] and (r[:, h].min() < 0 or r[:, h].max() >= c):
            raise _lib.TfcError(f"labels: column {h} has a class outside [0, {c}) (values {r[:, h].min():g} .. {r[:, h].max():g})")
    return np.ascontiguousarray(r.astype(np.int32))


def softmax_ce_heads(logits, targets, weights=(1.0, 1.0, 1.0), scale=1.0, want_grad=True, classes=AUX_CLASSES, targets_host=None):
    """logits [N, sum C_h] fp32, targets int32 [N,3] on the device (targets_host: the same as int32 numpy, validated by the library when given).
    Returns (probs [N, sum C_h], losses [4] = three head losses + scale * weighted sum, dlogits or None)."""
    require_gpu(logits, targets)
    N = logits.shape[0]
    assert targets.dtype == torch.int32 and targets.is_contiguous() and tuple(targets.shape) == (N, 3)
    probs = torch.empty_like(logits)
    losses = torch.empty(4, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    th = None
    if targets_host is not None:
        assert targets_host.dtype.name == "int32" and targets_host.shape == (N, 3) and targets_host.flags["C_CONTIGUOUS"]
        th = targets_host.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    check(lib().tfc_softmax_ce_heads(stream_ptr(), _p(_f32c(logits, "logits")), _p(targets), th, _int3(classes),
                                     (ctypes.c_float * 3)(*[float(w) for w in weights]), float(scale), N, _p(probs), _p(losses), _p(dl)),
          "tfc_softmax_ce_heads")
    return probs, losses, dl


def aux_heads_dgrad(g, ws, dlogits, classes=AUX_CLASSES):
    """g [N,C>=3,H,W] fp32 (in place): g[:, :3] += the heads' gradient w.r.t. the img_A half of their input"""
    require_gpu(g, dlogits, *ws)
    N, C, H, W = g.shape
    check(lib().tfc_aux_heads_dgrad(stream_ptr(), _p(_f32c(g, "g")), C, N, H, W, _ptr3([_f32c(w, "head weight") for w in ws]), _int3(classes),
                                    _p(_f32c(dlogits, "dlogits"))), "tfc_aux_heads_dgrad")
    return g


def aux_heads_wgrad(dt, x_r: View, dl_r, x_f: View, dl_f, dws, dbs, accumulate=False, classes=AUX_CLASSES):
    """weight / bias gradients of the three heads from the real pair (x_r, dl_r) and, when given, the fake pair, into the torch-layout gradients"""
    require_gpu(x_r.t, dl_r, *dws, *dbs)
    assert x_f is None or (x_f.t.shape == x_r.t.shape and x_f.pitch == x_r.pitch)
    check(lib().tfc_aux_heads_wgrad(stream_ptr(), dt, x_r.ptr, _p(_f32c(dl_r, "dlogits")), None if x_f is None else x_f.ptr,
                                    None if dl_f is None else _p(_f32c(dl_f, "dlogits")), x_r.pitch, x_r.N, x_r.H, x_r.W,
                                    _ptr3([_f32c(w, "head weight gradient") for w in dws]), _ptr3([_f32c(b, "head bias gradient") for b in dbs]),
                                    _int3(classes), 1 if accumulate else 0), "tfc_aux_heads_wgrad")


# ---- edge mask of the MASK-4 script (csrc/mask.hip; TFCGAN_multigpu_patchFFT_experiment.py:385-390) ---------------------------------------------------
MASK_STATS = 16                     # floats at the head of a mask workspace: mn, mx, ties, ties, M, ties(M), dM, L1 loss, dmx, dmn (include/tfc_gan.h)


class MaskCtx:
    """what one forward of the mask operator leaves on the device: the signed Laplacian, the blurred plane Bl (mask = Bl / M) and the workspace that
    holds the extrema, their tie counts and (after a backward) the global sums. Nothing of it is read by the host. phased: the extrema are those of
    all ranks' samples (mask_fwd ran in phases); the backward then runs in phases too, over `group`."""
    __slots__ = ("N", "H", "W", "lap", "bl", "ws", "phased", "group")

    @property
    def M(self):                    # device float: max of Bl over the batch
        return self.ws[4:5]


MASK_RECORD_WORDS = 4               # TFC_MASK_RECORD_BYTES / 8: what a rank leaves between two phases (include/tfc_gan.h)
MASK_TIE_LIMIT = 1 << 24            # tie counts are kept as floats in the workspace: exact up to 2^24


def _mask_dims(img, what):
    if img.dim() != 4 or img.shape[1] != 3:
        raise _lib.TfcError(f"{what}: image {tuple(img.shape)} (expected [N,3,H,W])")
    N, _, H, W = img.shape
    if H < 8 or W < 8:
        raise _lib.TfcError(f"{what}: H={H}, W={W} (both filters reflect once: H, W >= 8)")
    return N, H, W


def check_mask_tie_range(world, N, H, W, what="mask_fwd"):
    """a tie count of the gathered batch can reach world * N * H * W and is kept as a float: refuse what a float cannot count"""
    if world * N * H * W > MASK_TIE_LIMIT:
        raise _lib.TfcError(f"{what}: world * N * H * W = {world} * {N} * {H} * {W} = {world * N * H * W} > 2^24: the tie counts of the batch extrema "
                            f"are kept as fp32 and would no longer be exact (use batch_scope='shard' or a smaller global batch)")


def _mask_exchange(c, rec, which):
    """gather this rank's record, merge the records of all ranks into the stats floats of c.ws"""
    recs = parallel.all_gather_records(rec, c.group)
    check(lib().tfc_mask_merge(stream_ptr(), _p(c.ws), _p(recs), recs.shape[0], which), "tfc_mask_merge")


def mask_fwd(img, batch_scope="global", group=None):
    """img fp32 [N,3,H,W] -> MaskCtx (lap, Bl, extrema on the device). fp32 in every compute mode. batch_scope "global" on several ranks: the extrema
    are those of the gathered batch (two phases, two small exchanges: phased_scope)."""
    phased = phased_scope(batch_scope, "mask_fwd")
    require_gpu(img)
    N, H, W = _mask_dims(img, "mask_fwd")
    if phased:
        check_mask_tie_range(parallel.dist.get_world_size(group), N, H, W)
    img = img.detach().contiguous().float()
    c = MaskCtx()
    c.N, c.H, c.W, c.phased, c.group = N, H, W, phased, group
    c.lap = torch.empty((N, 1, H, W), dtype=torch.float32, device=img.device)
    c.bl = torch.empty_like(c.lap)
    c.ws = torch.empty(lib().tfc_mask_ws_bytes(N, H, W) // 4, dtype=torch.float32, device=img.device)
    if not phased:
        check(lib().tfc_mask_fwd(stream_ptr(), _p(img), _p(c.lap), _p(c.bl), _p(c.ws), N, H, W), "tfc_mask_fwd")
        return c
    rec = torch.empty(MASK_RECORD_WORDS, dtype=torch.int64, device=img.device)
    check(lib().tfc_mask_fwd_lap(stream_ptr(), _p(img), _p(c.lap), _p(c.ws), _p(rec), N, H, W), "tfc_mask_fwd_lap")
    _mask_exchange(c, rec, 0)
    rec = torch.empty_like(rec)                                   # a fresh record: the gather of the first may still be reading it
    check(lib().tfc_mask_fwd_blur(stream_ptr(), _p(c.lap), _p(c.bl), _p(c.ws), _p(rec), N, H, W), "tfc_mask_fwd_blur")
    _mask_exchange(c, rec, 1)
    return c


def mask_scale(c: MaskCtx):
    """the mask itself [N,1,H,W] = Bl / M"""
    out = torch.empty_like(c.bl)
    check(lib().tfc_mask_scale(stream_ptr(), _p(c.bl), _p(c.ws), _p(out), c.N, c.H, c.W), "tfc_mask_scale")
    return out


def mask_bwd(c: MaskCtx, dout=None, ref=None, scale=1.0, want_grad=True, batch_scope="global"):
    """exact backward of the mask operator through the context of its forward. dout [N,1,H,W]: an upstream gradient -> dimg [N,3,H,W]. ref [N,1,H,W]:
    the L1 loss scale * mean|mask - ref| -> (loss [1], dimg or None). Through a context whose forward ran in phases (batch_scope "global" on several
    ranks) the loss is this rank's share, scale * mean over ITS samples -- the mean over ranks is the loss of the gathered batch --, and dimg is the
    gradient of the SUM of the ranks' shares (of the ranks' sum dout * mask) w.r.t. this rank's images: after the 1/world of the gradient exchange the
    parameters receive the gradient of the gathered-batch loss."""
    if (dout is None) == (ref is None):
        raise _lib.TfcError("mask_bwd: exactly one of dout (an upstream gradient) and ref (the L1 loss against it)")
    if phased_scope(batch_scope, "mask_bwd") != c.phased:
        raise _lib.TfcError(f"mask_bwd: batch_scope={batch_scope!r} through a context whose forward ran with the other scope")
    u = dout if ref is None else ref
    require_gpu(u, c.bl)
    if tuple(u.shape) != tuple(c.bl.shape):
        raise _lib.TfcError(f"mask_bwd: {tuple(u.shape)} against a mask of {tuple(c.bl.shape)}")
    u = _f32c(u.detach().contiguous(), "dout / ref")
    dev = c.bl.device
    dimg = torch.empty((c.N, 3, c.H, c.W), dtype=torch.float32, device=dev) if (want_grad or ref is None) else None
    dmn = torch.empty_like(c.bl) if dimg is not None else None
    dbuf = torch.empty_like(c.bl) if ref is not None else None
    if not c.phased:
        check(lib().tfc_mask_bwd(stream_ptr(), _p(c.lap), _p(c.bl), _p(c.ws), _p(u if ref is None else None), _p(u if ref is not None else None),
                                 float(scale), _p(dbuf), _p(dmn), _p(dimg), c.N, c.H, c.W), "tfc_mask_bwd")
    else:
        rec = torch.empty(MASK_RECORD_WORDS, dtype=torch.int64, device=dev)
        check(lib().tfc_mask_bwd_dot(stream_ptr(), _p(c.bl), _p(c.ws), _p(u if ref is None else None), _p(u if ref is not None else None),
                                     float(scale), _p(dbuf), _p(rec), c.N, c.H, c.W), "tfc_mask_bwd_dot")
        if dimg is not None:                                      # the loss alone needs no exchange: it is this rank's own
            _mask_exchange(c, rec, 2)
            rec = torch.empty_like(rec)
            check(lib().tfc_mask_bwd_blur(stream_ptr(), _p(c.lap), _p(c.bl), _p(c.ws), _p(u if ref is None else dbuf), _p(dmn), _p(rec), c.N, c.H, c.W),
                  "tfc_mask_bwd_blur")
            _mask_exchange(c, rec, 3)
            check(lib().tfc_mask_bwd_lap(stream_ptr(), _p(c.lap), _p(c.ws), _p(dmn), _p(dimg), c.N, c.H, c.W), "tfc_mask_bwd_lap")
    if ref is None:
        return dimg
    return c.ws[7:8].clone(), dimg


def pack_nhwc8_plane(dt, x, plane, plane_div=None):
    """torch.cat((x, plane), 1) as the NHWC8 activation of the compute dtype: channels 0..2 x, 3 the plane [N,1,H,W] (divided by the device float
    plane_div when given: Bl of a MaskCtx with its M), 4..7 zero. The plane is data: it gets no gradient."""
    require_gpu(x, plane)
    x = x.contiguous().float()
    N, C, H, W = x.shape
    if C != 3 or tuple(plane.shape) != (N, 1, H, W):
        raise _lib.TfcError(f"pack_nhwc8_plane: x {tuple(x.shape)}, plane {tuple(plane.shape)} (expected [N,3,H,W] and [N,1,H,W])")
    out = new_act(N, H, W, 8, dt, x.device)
    check(lib().tfc_pack_nhwc8_plane(stream_ptr(), dt, _p(x), _p(_f32c(plane, "plane")), _p(plane_div), out.ptr, N, H, W), "tfc_pack_nhwc8_plane")
    return out


# ---- STN21 localiser (vit.hip) ---------------------------------------------------------------------------------
globals().update({k: v for k, v in _lib.CONSTANTS.items() if k.startswith("VIT_")})      # VIT_A_ROWS, VIT_B_WEIGHT, VIT_C_ROWS, VIT_ACT_NONE, ...


class VitGemm(ctypes.Structure):
    """TfcVitGemm, fields as include/tfc_gan.h declares them"""
    _fields_ = _lib.STRUCTS["TfcVitGemm"]


def _fp(t):
    return None if t is None else t.data_ptr()


def vit_gemm(dt, M, N, K, a, b, c, a_mode=VIT_A_ROWS, lda=None, a2=None, a_rg=0, a_rso=0, b_mode=VIT_B_WEIGHT, ldb=None, b2=None,
             c_mode=VIT_C_ROWS, ldc=None, c2=None, c_rg=0, c_rso=0, bias=None, res=None, act=VIT_ACT_NONE, aux=None, ldaux=None, unfold=(0, 0, 0, 0)):
    """C(m, n) = epilogue(sum_k A(m, k) B(k, n)) on fp32 CUDA tensors (tfc_vit_gemm: modes and epilogue in include/tfc_gan.h). Defaults: A [M][K]
    rows, B = an nn.Linear weight [N][K], C [M][N] rows. a / b / c may be views: their data_ptr() is the base the strides count from."""
    require_gpu(a, a2, b, b2, c, c2, bias, res, aux)
    for t in (a, a2, b, b2, c, c2, bias, res, aux):
        assert t is None or t.dtype == torch.float32, t.dtype
    if lda is None:
        lda = K if a_mode == VIT_A_ROWS else M
    if ldb is None:
        ldb = K if b_mode == VIT_B_WEIGHT else N
    g = VitGemm(M, N, K, a_mode, a_rg, _fp(a), _fp(a2), lda, a_rso, b_mode, c_mode, _fp(b), _fp(b2), ldb, _fp(c), _fp(c2), N if ldc is None else ldc,
                c_rso, c_rg, act, _fp(bias), _fp(res), _fp(aux), N if ldaux is None else ldaux, *unfold)
    dev = (c if c is not None else c2).device
    check(lib().tfc_vit_gemm(stream_ptr(), dt, ctypes.byref(g), part_ws(dev)), "tfc_vit_gemm")


def vit_layernorm_fwd(x, gamma, beta, eps=1e-6):
    """rows of x [.., D] -> (y, mean, rstd)"""
    require_gpu(x, gamma, beta)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    check(lib().tfc_vit_layernorm_fwd(stream_ptr(), _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D, eps), "tfc_vit_layernorm_fwd")
    return y, mean, rstd


def vit_layernorm_bwd(dy, x, mean, rstd, gamma, dres=None, want_gb=True):
    """-> (dx = dres + d LN / d x, dgb [2][D] = (d gamma, d beta) or None)"""
    require_gpu(dy, x, mean, rstd, gamma, dres)
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty_like(x)
    dgb = torch.empty((2, D), dtype=torch.float32, device=x.device) if want_gb else None
    check(lib().tfc_vit_layernorm_bwd(stream_ptr(), _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx), _p(dgb), rows, D, part_ws(x.device)),
          "tfc_vit_layernorm_bwd")
    return dx, dgb


def vit_colsum(v, rows, L, ld=None):
    """out[L] = sum over `rows` rows (ld apart) of v, in a fixed order"""
    require_gpu(v)
    out = torch.empty(L, dtype=torch.float32, device=v.device)
    check(lib().tfc_vit_colsum(stream_ptr(), _p(v), L if ld is None else ld, rows, L, _p(out), part_ws(v.device)), "tfc_vit_colsum")
    return out


def vit_attention_fwd(dt, qkv, N, T, H, scale):
    """qkv [N*T, 3*H*64] -> (out [N*T, H*64], probs [N, H, T, T])"""
    require_gpu(qkv)
    out = torch.empty((N * T, H * 64), dtype=torch.float32, device=qkv.device)
    probs = torch.empty((N, H, T, T), dtype=torch.float32, device=qkv.device)
    check(lib().tfc_vit_attention_fwd(stream_ptr(), dt, _p(qkv), _p(out), _p(probs), N, T, H, scale), "tfc_vit_attention_fwd")
    return out, probs


def vit_attention_bwd(dt, dout, qkv, probs, N, T, H, scale):
    require_gpu(dout, qkv, probs)
    dqkv = torch.empty_like(qkv)
    check(lib().tfc_vit_attention_bwd(stream_ptr(), dt, _p(dout), _p(qkv), _p(probs), _p(dqkv), N, T, H, scale), "tfc_vit_attention_bwd")
    return dqkv


VIT_ATTN_TQ = VIT_ATTN_TK = 64      # query-tile / key-tile heights of the tiled attention kernels (TQ, TK of csrc/vit.hip)
VIT_ATTN_MAX_T = 1025               # 512 x 512 at patch 16


def vit_attention_tiled_fwd(dt, qkv, N, T, H, scale):
    """qkv [N*T, 3*H*64] -> (out [N*T, H*64], stats [N, H, 3, T]: per query row the maximum of the signed logits as hi + lo and the sum of
    exp((logit - max) |scale|)). Any 1 <= T <= 1025; no [T, T] tensor is written."""
    require_gpu(qkv)
    out = torch.empty((N * T, H * 64), dtype=torch.float32, device=qkv.device)
    stats = torch.empty((N, H, 3, T), dtype=torch.float32, device=qkv.device)
    check(lib().tfc_vit_attention_tiled_fwd(stream_ptr(), dt, _p(qkv), _p(out), _p(stats), N, T, H, scale), "tfc_vit_attention_tiled_fwd")
    return out, stats


def vit_attention_tiled_bwd(dt, dout, qkv, out, stats, N, T, H, scale):
    """-> dqkv like qkv. `out` (the forward's output) is accepted for the call's symmetry and not read: delta is rowsum(P dP) on the recomputed
    fp32 P, as in the kernels for T <= 64 (rowsum(dO o O) would carry the bf16 rounding of P into every dS)."""
    require_gpu(dout, qkv, out, stats)
    dqkv = torch.empty_like(qkv)
    ws = torch.empty((N, H, T), dtype=torch.float32, device=qkv.device)
    check(lib().tfc_vit_attention_tiled_bwd(stream_ptr(), dt, _p(dout), _p(qkv), _p(stats), _p(dqkv), N, T, H, scale, _p(ws)),
          "tfc_vit_attention_tiled_bwd")
    return dqkv


def vit_tokens_fwd(x, cls, pos):
    """x [N, T, D] with the patch tokens in rows 1..T-1: row 0 = cls, every row += pos (in place)"""
    require_gpu(x, cls, pos)
    N, T, D = x.shape
    check(lib().tfc_vit_tokens_fwd(stream_ptr(), _p(x), _p(cls), _p(pos), N, T, D), "tfc_vit_tokens_fwd")


# ---- measurement ----------------------------------------------------------------------------------------------
def prof_enable(on):
    check(lib().tfc_prof_enable(1 if on else 0), "tfc_prof_enable")


def prof_records(max_records=4096):
    """per-call records since the last collect: list of dicts {kclass, ms, flop, op, pass, N, H, W, Cin, Cout} (synchronise first)"""
    kc = (ctypes.c_int * max_records)()
    ms = (ctypes.c_double * max_records)()
    fl = (ctypes.c_double * max_records)()
    meta = (ctypes.c_int * (7 * max_records))()
    n = lib().tfc_prof_records(max_records, kc, ms, fl, meta)
    if n < 0:
        check(n, "tfc_prof_records")
    keys = ("op", "pass", "N", "H", "W", "Cin", "Cout")
    return [dict(kclass=kc[i], ms=ms[i], flop=fl[i], **{k: meta[7 * i + j] for j, k in enumerate(keys)}) for i in range(n)]


def prof_collect(kclass):
    ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
    check(lib().tfc_prof_collect(kclass, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n)), "tfc_prof_collect")
    return ms.value, fl.value, n.value


# ---- evaluation metrics (include/tfc_gan.h, "evaluation metrics"; csrc/metrics.hip) ------------------------------------------------------------
# Operands: uint8 device tensors [N, ...] whose images are contiguous blocks (stride(0) may be anything >= the image). Scratch is a fresh torch
# allocation per call (the caching allocator: no synchronisation), so calls on different streams never share it.
def _flat_u8(t):
    """[N, ...] uint8 on the device with every image contiguous -> (tensor, bytes per image)"""
    require_gpu(t)
    assert t.dtype == torch.uint8 and t.dim() >= 2, "uint8 [N, ...] images expected"
    if not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < t[0].numel()):
        t = t.contiguous()
    return t, t[0].numel()


def _img_stride(t, count):
    """bytes between images; a batch of one has none, and says "aligned" so that its single image may take the 128-bit loads"""
    return t.stride(0) if t.shape[0] > 1 else (count + 15) // 16 * 16


def pair_moments(a, b, want_psnr=True, want_ncc=True):
    """Exact integer moments of N image pairs: int64 [N,10] = sum a, sum b, sum a^2, sum b^2, sum ab, sum (a-b)^2, min a, max a, min b, max b;
    plus PSNR and NCC (fp64 [N], or None when not wanted)."""
    a, count = _flat_u8(a)
    b, cb = _flat_u8(b)
    assert a.shape[0] == b.shape[0] and count == cb, "a and b must hold the same number of images of the same size"
    N = a.shape[0]
    ws = torch.empty(max(lib().tfc_pair_moments_ws_bytes(N, count), 8) // 8, dtype=torch.int64, device=a.device)
    mom = torch.empty((N, 10), dtype=torch.int64, device=a.device)
    psnr = torch.empty(N, dtype=torch.float64, device=a.device) if want_psnr else None
    ncc = torch.empty(N, dtype=torch.float64, device=a.device) if want_ncc else None
    check(lib().tfc_pair_moments_u8(stream_ptr(), _p(a), _img_stride(a, count), _p(b), _img_stride(b, count), count, N, _p(ws),
                                    _p(mom), _p(psnr), _p(ncc)), "tfc_pair_moments_u8")
    return mom, psnr, ncc


def ssim_u8(a, b, wy=7, wx=7, data_range=255.0):
    """a, b: uint8 [N,H,W] gray on the device (unit stride along W; row and image strides are passed through). fp64 [N]."""
    require_gpu(a, b)
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.dim() == 3 and a.shape == b.shape, "uint8 [N,H,W] pairs of one shape expected"
    if a.stride(2) != 1:
        a = a.contiguous()
    if b.stride(2) != 1:
        b = b.contiguous()
    N, H, W = a.shape
    ws = torch.empty(max(lib().tfc_ssim_ws_bytes(N, H, W, wy, wx), 8) // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(N, dtype=torch.float64, device=a.device)
    span = (H - 1) * max(a.stride(1), b.stride(1)) + W
    check(lib().tfc_ssim_u8(stream_ptr(), _p(a), a.stride(0) if N > 1 else span, a.stride(1), _p(b), b.stride(0) if N > 1 else span, b.stride(1),
                            N, H, W, wy, wx, float(data_range), _p(ws), _p(out)), "tfc_ssim_u8")
    return out


def hist_color(img, layout):
    """8 x 8 x 8 colour histogram, uint32 [N,512]. layout: "hwc" [N,H,W,3], "chw" [N,3,H,W], "gray" [N,H,W] (read as R = G = B)."""
    img, count = _flat_u8(img)
    N = img.shape[0]
    npix = count if layout == "gray" else count // 3
    pix, chan = {"hwc": (3, 1), "chw": (1, npix), "gray": (1, 0)}[layout]
    hist = torch.empty((N, 512), dtype=torch.int32, device=img.device)
    check(lib().tfc_hist_u8_color(stream_ptr(), _p(img), _img_stride(img, count), pix, chan, npix, N, _p(hist)), "tfc_hist_u8_color")
    return hist


def bhattacharyya(h1, h2):
    """h1, h2: int32 [N,nbins] counts -> fp64 [N]"""
    out = torch.empty(h1.shape[0], dtype=torch.float64, device=h1.device)
    check(lib().tfc_bhattacharyya(stream_ptr(), _p(h1), _p(h2), h1.shape[0], h1.shape[1], _p(out)), "tfc_bhattacharyya")
    return out


def joint_hist(a, b, moments, nb, edge_f32=False):
    """[N,nb,nb] int32 joint histogram of np.histogram2d(a / 255, b / 255, bins = nb) on float32 pixels; moments: pair_moments(a, b)[0]"""
    a, count = _flat_u8(a)
    b, cb = _flat_u8(b)
    assert a.shape[0] == b.shape[0] and count == cb
    N = a.shape[0]
    luts = torch.empty((2, N, 256), dtype=torch.uint8, device=a.device)
    check(lib().tfc_mi_bin_lut(stream_ptr(), _p(moments), N, nb, 1 if edge_f32 else 0, _p(luts[0]), _p(luts[1])), "tfc_mi_bin_lut")
    hist = torch.empty((N, nb, nb), dtype=torch.int32, device=a.device)
    check(lib().tfc_hist_u8_joint(stream_ptr(), _p(a), _img_stride(a, count), _p(b), _img_stride(b, count), count, N,
                                  _p(luts[0]), _p(luts[1]), nb, _p(hist)), "tfc_hist_u8_joint")
    return hist


def mutual_information(hist):
    """hist: int32 [N,nb,nb] counts -> fp64 [N]"""
    out = torch.empty(hist.shape[0], dtype=torch.float64, device=hist.device)
    check(lib().tfc_mutual_information(stream_ptr(), _p(hist), hist.shape[0], hist.shape[1], _p(out)), "tfc_mutual_information")
    return out
