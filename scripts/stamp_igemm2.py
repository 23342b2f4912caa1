"""Diagnostic: phase shares of the persistent gather GEMM (tfc_igemm2_kernel) from s_memtime stamps; needs a -DTFC_STAMP build (TFC_SO_OVERRIDE).
Read the SHARES, never the run time of this build.

    python scripts/stamp_igemm2.py [FLAGSET ...]        default: all six

FLAGSET names the epilogue the launches take -- the kernel compiles one copy of its epilogue per set:
    none      no flags (generator convolutions without a norm)
    stats     TFC_EP_STATS (convolutions in front of an InstanceNorm)
    dfwd      TFC_EP_BIAS | TFC_EP_LEAKY with an oscale (discriminator forward)
    oscale    no flags, with an oscale (discriminator input gradients)
    accum     TFC_EP_ACCUM into the skip window of a concat buffer (generator down-path input gradients)
    vgg       TFC_EP_BIAS | TFC_EP_RELU on TFC_OP_CONV3 (LPIPS feature stack)
The input-gradient entry point carries no stamp buffer, so the gradient sets run through tfc_conv_fwd with the same flags; the shape (64, 64, 256, convT)
stands for a Cin = 64 stride-2 input gradient: the same 2 x 2-tap gather with a 64-channel K loop."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import tfc_gan_amd as T
from tfc_gan_amd import ops, _lib
DEV = "cuda:0"
dt = ops.DT_BF16
N = 32
lib = _lib.load()
#           name: (flags, bias, oscale, stats, window, op)
FLAGSETS = {"none": (0, False, False, False, False, ops.OP_CONV),
            "stats": (ops.EP_STATS, False, False, True, False, ops.OP_CONV),
            "dfwd": (ops.EP_BIAS | ops.EP_LEAKY, True, True, False, False, ops.OP_CONV),
            "oscale": (0, False, True, False, False, ops.OP_CONV),
            "accum": (ops.EP_ACCUM, False, False, False, True, ops.OP_CONV),
            "vgg": (ops.EP_BIAS | ops.EP_RELU, True, False, False, False, ops.OP_CONV3)}
shapes = [(128, 64, 128, None), (64, 128, 256, None), (32, 256, 512, None), (16, 512, 512, None), (8, 512, 512, None), (64, 64, 256, ops.OP_CONVT)]
names = sys.argv[1:] or list(FLAGSETS)
for name in names:
    flags, has_bias, has_osc, has_stats, win, set_op = FLAGSETS[name]
    for H, Cin, Cout, shape_op in shapes:
        op = shape_op if shape_op is not None and set_op == ops.OP_CONV else set_op
        OH = ops.OUT_HW[op](H)
        x = ops.View(torch.randn(N, H, H, Cin, device=DEV).to(torch.bfloat16), Cin)
        w = torch.randn(*((Cin, Cout) if op == ops.OP_CONVT else (Cout, Cin)), 4, 4, device=DEV) * 0.03
        y = ops.View(torch.zeros(N, OH, OH, 2 * Cout, dtype=torch.bfloat16, device=DEV), Cout, Cout) if win else ops.new_act(N, OH, OH, Cout, dt, DEV)
        pk = ops.pack_weight(dt, op, 0, w, Cin, Cout)
        bias = torch.randn(Cout, device=DEV) if has_bias else None
        osc = torch.full((1,), 0.7, device=DEV) if has_osc else None
        stats = torch.zeros(N, Cout, 2, device=DEV) if has_stats else None
        stamps = torch.zeros(1 << 20, dtype=torch.int64, device=DEV)
        for _ in range(3):
            ops.check(lib.tfc_conv_fwd(ops.stream_ptr(), dt, op, x.ptr, x.pitch, N, H, H, Cin, Cout, ops._p(pk), y.ptr, y.pitch, ops._p(bias), ops._p(stats),
                                       ops._p(stamps), ops._p(osc), flags, ops.part_ws(DEV) if has_stats else None), "conv")
        torch.cuda.synchronize()
        s = stamps.cpu().numpy().reshape(-1, 16)
        s = s[s[:, 0] != 0].astype(np.int64)
        life = s[:, 0]
        pro = s[:, 1] * 0
        print(f"   shader clock during the kernel: {100e6 * (s[:, 0] / s[:, 6]).mean() / 1e9:.3f} GHz")
        print(f"[{name}] op {op} H={H} {Cin}->{Cout}: {len(s)} waves, tiles/wave {s[:, 7].mean():.2f}, lifetime mean {life.mean():.0f} cycles, ")
        print(f"   prologue(first tile) {pro.mean():8.0f}  {pro.sum() / life.sum():6.1%}")
        for i, n in ((2, "mainloop"), (1, " of which stage sync"), (8, " of which halo issue"), (9, " of which first A read"), (3, "ep:acc->lds"), (4, "ep:barrier"), (5, "ep:stores")):
            print(f"   {n:20s} {s[:, i].mean():8.0f}  {s[:, i].sum() / life.sum():6.1%}   per tile {(s[:, i] / s[:, 7]).mean():8.0f}")
