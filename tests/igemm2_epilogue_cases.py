"""Cases of the gather GEMM's epilogue tests (test_gpu_52_igemm2_epilogue.py on the GPU, test_igemm2_epilogue_host.py on the host): inputs and the
float64 expectations of both are built HERE, once, so that the host test proves on the CPU exactly what the GPU test asks of the kernel.

Method: tests/conv_exact.py (integer operands, every partial sum exact in fp32, torch.equal against float64).

The persistent kernel compiles its epilogue once per flag set of the training step and once with the flags read at run time. FLAG_SETS names the six
specialised sets plus one combination that takes the run-time copy; GEOMETRIES are the smallest shapes at which the batched store pass can go wrong:
  * conv output 9 x 9 and 17 x 17 (tile 8 x 16): a second tile row with one live row, a second tile column with one live column;
  * transposed convolution of a 5 x 5 input: four phases storing at stride 2 into a 10 x 10 plane;
  * an n-block with fewer live channels than the tile is wide (the n0 < Nout guard). The plan gives a 128-channel tile only to layers with at least
    128 output channels (tfc_plan_igemm: nb >= 4), so Cout = 96 meets the guard on the 64-channel tile (second n-block: 32 of 64) and Cout = 160
    meets it on the 128-channel tiles (second n-block: 32 of 128); the 32-channel tile has no partial n-block and takes Cout = 96 as three whole ones.
Every destination is the skip window of a concat buffer (pitch 2 C, channel offset C) inside a larger allocation with sentinels around it.
"""
import zlib
from collections import namedtuple

import torch

from tests import conv_exact as X
from tfc_gan_amd import _lib, ops
from tfc_gan_amd.ops import OP_CONV, OP_CONV3, OP_CONVT

OSCALE = X.OSCALE                            # 1/2: with half-integer biases every pre-activation is a multiple of 1/2
LEAKY = 0.2                                  # the fixed slope of TFC_EP_LEAKY: one fp32 multiply and a maximum (conv_exact.leaky_f32)
GUARD = 64                                   # sentinel elements in front of and behind the concat buffer (128 bytes: keeps 16-byte alignment)

FlagSet = namedtuple("FlagSet", "name flags bias oscale stats accum ops")
FLAG_SETS = [
    FlagSet("none", 0, False, False, False, False, (OP_CONV, OP_CONVT)),
    FlagSet("stats", _lib.EP_STATS, False, False, True, False, (OP_CONV, OP_CONVT)),
    FlagSet("bias_oscale_leaky", _lib.EP_BIAS | _lib.EP_LEAKY, True, True, False, False, (OP_CONV, OP_CONVT)),
    FlagSet("oscale", 0, False, True, False, False, (OP_CONV, OP_CONVT)),
    FlagSet("accum", _lib.EP_ACCUM, False, False, False, True, (OP_CONV, OP_CONVT)),
    FlagSet("bias_relu", _lib.EP_BIAS | _lib.EP_RELU, True, False, False, False, (OP_CONV3,)),
    FlagSet("bias_only_runtime_flags", _lib.EP_BIAS, True, False, False, False, (OP_CONV, OP_CONVT, OP_CONV3)),
]

Geom = namedtuple("Geom", "name op N H Cin")
GEOMETRIES = [
    Geom("conv9x9", OP_CONV, 2, 10, 32),
    Geom("conv17x17", OP_CONV, 3, 18, 64),
    Geom("convT5to10", OP_CONVT, 2, 5, 64),
    Geom("conv3_9x9", OP_CONV3, 2, 9, 32),
    Geom("conv3_17x17", OP_CONV3, 2, 17, 64),
]
# workgroup tile (tfc_debug_set_igemm_config) -> (channels of the tile, Cout of its cases)
TILES = {0: (128, 160), 1: (64, 96), 2: (32, 96), 3: (128, 160)}
GRID_COUT = 128                              # the grid-hook cases: 4 / 4 / 8 / 16 work items on the 9 x 9 shape, none a multiple of 3


def seed(*key):
    return zlib.crc32(".".join(str(k) for k in key).encode())


def out_hw(g):
    return ops.OUT_HW[g.op](g.H)


def weight_shape(g, Cout):
    return (g.Cin, Cout, 4, 4) if g.op == OP_CONVT else (Cout, g.Cin, 4, 4)


def inputs(g, Cout):
    """float64 CPU tensors: x, w (torch layout; CONV3: only the 3 x 3 corner of the slot is nonzero, as lpips.py packs it), bias (multiples of 1/2),
    base (what an accumulating call adds to)"""
    x = X.ints((g.N, g.Cin, g.H, g.H), seed(g.name, Cout, "x"))
    w = X.ints(weight_shape(g, Cout), seed(g.name, Cout, "w"))
    if g.op == OP_CONV3:
        w[:, :, 3, :] = 0
        w[:, :, :, 3] = 0
    b = X.ints((Cout,), seed(g.name, Cout, "b")) / 2
    base = X.ints((g.N, Cout, out_hw(g), out_hw(g)), seed(g.name, Cout, "base"))
    return x, w, b, base


def worst_partial_sum(g, fs):
    """an upper bound of every |partial sum| in quanta (1/2 with a bias or oscale): all taps of all padded input channels at amplitude 1, + the bias"""
    quantum = 2 if (fs.bias or fs.oscale) else 1
    return (ops.pad8(g.Cin) * X.TAPS[g.op] + (1 if fs.bias else 0)) * quantum


def expected(g, fs, z, b, base):
    """what the kernel stores (bf16), from the float64 convolution z: acc * oscale + bias in fp32 (exact), the activation in fp32, one rounding to bf16;
    accumulation adds the stored bf16 value to the destination's in fp32 (exact) and rounds again"""
    quantum = 2 if (fs.bias or fs.oscale) else 1
    v = z * (OSCALE if fs.oscale else 1.0) + (b.view(1, -1, 1, 1) if fs.bias else 0.0)
    X.assert_dyadic(v, quantum, f"{g.name} {fs.name} reference")
    v32 = X.store(v, ops.DT_F32)
    if fs.flags & _lib.EP_LEAKY:
        v32 = X.leaky_f32(v32, LEAKY)
    if fs.flags & _lib.EP_RELU:
        v32 = torch.clamp_min(v32, 0.0)
    want = v32.to(torch.bfloat16)
    if fs.accum:
        want = X.store(want.double() + base, ops.DT_BF16)
    return want
