"""Shared shapes and arithmetic of the bf16x3 compute mode tests (tests/test_bf16x3_host.py on the CPU, tests/test_gpu_36_bf16x3.py on the GPU).

bf16x3: every fp32 operand value a is split as a_hi = bf16_rn(a), a_lo = bf16_rn(a - a_hi) and a product as a_hi b_hi + a_hi b_lo + a_lo b_hi,
accumulated in fp32. Per product the error is at most u^2 (3 + 2u) |a b| with u = 2^-8; the normwise bound B below adds 2^-20 for the fp32
accumulation (independent zero-mean data: the per-product errors add like the products themselves)."""
from collections import namedtuple

import torch

from tfc_gan_amd.ops import OP_CONV, OP_CONV3, OP_CONVT, OP_PADCONV, OP_UPCONV

B = 3 * 2.0 ** -16 + 2.0 ** -20                    # ~4.67e-5: normwise relative error bound of one bf16x3 convolution vs exact arithmetic

# passes: "f" forward, "d" dgrad, "w" wgrad. flags: "bias", "tanh" (bias + tanh, NCHW store), "stats" (InstanceNorm sums), "accum" (TFC_EP_ACCUM)
Case = namedtuple("Case", "name op Cin Cout H N passes flags")
CASES = [
    Case("first_layer_c3", OP_CONV, 3, 64, 20, 2, "fdw", ""),             # the 8-padded 3-channel first layer
    Case("conv_stats", OP_CONV, 64, 128, 16, 2, "fdw", "stats"),          # InstanceNorm statistics epilogue
    Case("conv_multitile", OP_CONV, 32, 64, 41, 2, "fdw", "accum"),       # 5 x 3 tiles per image; accumulating forward / dgrad
    Case("padconv", OP_PADCONV, 64, 32, 9, 2, "fdw", "bias"),
    Case("convt", OP_CONVT, 128, 64, 8, 2, "fdw", "accum"),
    Case("upconv", OP_UPCONV, 64, 32, 8, 2, "fdw", ""),
    Case("upconv_head", OP_UPCONV, 128, 3, 8, 2, "fdw", "tanh"),          # the generator head: bias + tanh, NCHW store
    Case("conv3", OP_CONV3, 64, 64, 12, 2, "fd", "bias"),                 # LPIPS 3 x 3 (no weight-gradient pass)
    Case("wgrad_over_slab_budget", OP_CONV, 1024, 2048, 5, 1, "w", ""),   # 32 x 32 (n-block, c-block) pairs: more than the 512 slabs
]


def weight_shape(c):
    return (c.Cin, c.Cout, 4, 4) if c.op == OP_CONVT else (c.Cout, c.Cin, 4, 4)


def split(a):
    """fp32 tensor -> (hi, lo) as float64 tensors holding exact bf16 values"""
    a = a.to(torch.float32)
    hi = a.to(torch.bfloat16).to(torch.float32)
    lo = (a - hi).to(torch.bfloat16).to(torch.float32)   # a - hi is exact in fp32
    return hi.double(), lo.double()


def three_term(f, a, b, terms=("hh", "hl", "lh")):
    """f(a, b) bilinear (a convolution) evaluated on the split operands in float64: the sum of the chosen hi / lo products"""
    ah, al = split(a)
    bh, bl = split(b)
    pick = {"h": (ah, bh), "l": (al, bl)}
    out = 0
    for t in terms:
        out = out + f(pick[t[0]][0], pick[t[1]][1])
    return out


def rel(got, want):
    got, want = got.double(), want.double()
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()
