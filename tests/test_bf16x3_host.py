"""bf16x3 compute mode, CPU side: the public constants, and the arithmetic the GPU tests rely on (tests/test_gpu_36_bf16x3.py).

The bound B of tests/bf16x3_cases.py is checked here on the split arithmetic itself, emulated in float64 from exact bf16 hi / lo values, before
any kernel is involved: every convolution shape of the GPU test stays within B, while plain bf16 operands and the variants that drop one cross term
miss it by 10x or more (so B separates a correct kernel from one that silently runs plain bf16 or drops a term). The network test shows that the
generator bar (L1 <= 1e-4 against the fp32 oracle) is reachable by this arithmetic."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import bf16x3_cases as C
from tests.conv_exact import ref_fwd
from tfc_gan_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtype_constants():
    assert ops.dt_of("bf16x3") == _lib.DT_BF16X3 == 2
    assert _lib.CONSTANTS["DT_BF16X3"] == _lib.DT_BF16X3          # the header's value
    # the kernels' shared header takes the value from the public header and does not restate it
    desc = open(os.path.join(ROOT, "tfc-gan_amd", "csrc", "tfc_desc.h")).read()
    assert '#include "../../include/tfc_gan.h"' in desc and "#define TFC_DT_" not in desc and "#define TFC_EP_" not in desc
    assert ops.torch_dtype(_lib.DT_BF16X3) == torch.float32
    assert ops.dt_of(torch.bfloat16) == _lib.DT_BF16 and ops.dt_of(torch.float32) == _lib.DT_F32
    for bad in ("bf16", "fp32", "BF16X3", "bf16x2", torch.float16, None):
        with pytest.raises(ValueError):
            ops.dt_of(bad)


def test_set_compute_dtype_accepts_bf16x3():
    prev = T.get_compute_dtype()
    try:
        T.set_compute_dtype("bf16x3")
        assert T.get_compute_dtype() == "bf16x3"
        with pytest.raises(ValueError):
            T.set_compute_dtype("tf32")
        assert T.get_compute_dtype() == "bf16x3"
    finally:
        T.set_compute_dtype(prev)


def test_split_is_exact_and_keeps_non_finite():
    g = torch.Generator().manual_seed(1)
    a = torch.randn(4096, generator=g) * torch.exp(torch.randn(4096, generator=g) * 4)
    hi, lo = C.split(a)
    assert torch.equal(hi.to(torch.bfloat16).double(), hi) and torch.equal(lo.to(torch.bfloat16).double(), lo)
    err = (hi + lo - a.double()).abs() / a.double().abs()
    assert err.max().item() <= 2.0 ** -16                      # |a - hi - lo| <= u |a - hi| <= u^2 |a|
    hi, lo = C.split(torch.tensor([float("inf"), float("-inf"), float("nan")]))
    assert not torch.isfinite(hi + lo).any()


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_bound_holds_for_the_split_arithmetic(case):
    g = torch.Generator().manual_seed(7)
    x = torch.randn((1, case.Cin, case.H, case.H), generator=g)
    w = torch.randn(C.weight_shape(case), generator=g)
    if case.op == ops.OP_CONV3:
        w[:, :, 3, :] = 0
        w[:, :, :, 3] = 0
    f = lambda a, b: ref_fwd(case.op, a, b)  # noqa: E731
    exact = f(x.double(), w.double())
    errs = {t: C.rel(C.three_term(f, x, w, t), exact) for t in (("hh", "hl", "lh"), ("hh",), ("hh", "hl"), ("hh", "lh"))}
    print(case.name, {"+".join(k): f"{v:.3e}" for k, v in errs.items()}, f"B {C.B:.3e}")
    assert errs[("hh", "hl", "lh")] <= C.B
    for t in (("hh",), ("hh", "hl"), ("hh", "lh")):
        assert errs[t] >= 10 * C.B, (t, errs[t])


class _SplitConvs:
    """replaces every non-depthwise conv2d / conv_transpose2d by the three-term split on fp32 storage (products exact, fp32 sums)"""

    def __enter__(self):
        self.c2, self.ct = F.conv2d, F.conv_transpose2d
        c2, ct = self.c2, self.ct

        def three(fn, x, w, b, **kw):
            xh, xl = C.split(x)
            wh, wl = C.split(w)
            f = lambda a, bb: fn(a.float(), bb.float(), None, **kw)  # noqa: E731
            y = f(xl, wh) + f(xh, wl) + f(xh, wh)
            return y if b is None else y + b.view(1, -1, 1, 1)

        def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
            if groups != 1:
                return c2(x, w, b, stride, padding, dilation, groups)     # BlurPool: stays fp32, as in the engine
            return three(c2, x, w, b, stride=stride, padding=padding, dilation=dilation)

        def conv_transpose2d(x, w, b=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
            return three(ct, x, w, b, stride=stride, padding=padding, output_padding=output_padding, dilation=dilation)

        F.conv2d, F.conv_transpose2d = conv2d, conv_transpose2d
        return self

    def __exit__(self, *a):
        F.conv2d, F.conv_transpose2d = self.c2, self.ct


def test_generator_bar_is_reachable_by_the_split_arithmetic(golden):
    """the oracle generator (init_weights_portable(seed=3), synthetic_pairs(1, seed=11): the inputs of generator_fwd.npz) with every convolution
    replaced by the three-term split: L1 vs the fp32 oracle <= 1e-4 (BASELINE north_star)"""
    torch.set_num_threads(8)
    A, _ = O.synthetic_pairs(1, seed=11)
    G = O.init_weights_portable(O.GeneratorUNet((3, 256, 256)), seed=3).eval()
    with torch.no_grad():
        want = G(A)
        with _SplitConvs():
            got = G(A)
    l1 = (got - want).abs().mean().item()
    l1_golden = (got[:, :, ::8, ::8] - torch.from_numpy(np.asarray(golden("generator_fwd")["fake_sub"]))).abs().mean().item()
    print(f"bf16x3 emulation: generator L1 vs fp32 oracle {l1:.3e}, vs golden subsample {l1_golden:.3e}")
    assert l1 <= 1e-4, l1
