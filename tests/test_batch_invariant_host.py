"""Batch-invariant mode, host side: the launch plans, asked through tfc_conv_plan_query -- the launchers' own decision functions,
no GPU needed -- for every convolution the step issues, in the three compute modes and all passes.

  * mode on: the record (kernel, tile form, partial slots per image, split count, workgroups per image, ...) is the same for every batch size and
    does not move with the chip's compute-unit count;
  * mode off: at least one layer's record differs between N = 1 and N = 32 -- the test can see what it guards;
  * mode on at N = 32 equals mode off at N = 32 on 256 compute units: the reference batch keeps its tuned forms.
"""
import ctypes
import os
import subprocess
import sys
import threading

import pytest

import tfc_gan_amd as T
from tfc_gan_amd import _lib

from tests import conv_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 5, 13, 32, 64)
NCU = 256
FLAG_BITS = {"bias": _lib.EP_BIAS, "stats": _lib.EP_STATS, "accum": _lib.EP_ACCUM, "tanh": _lib.EP_TANH_NCHW, "leaky": _lib.EP_LEAKY, "relu": _lib.EP_RELU}
PLAN_FIRST_BLOCK = 0x10000
GEMM_ENTRIES = ("conv_fwd", "conv_dgrad", "conv_wgrad")
FIRST_BLOCK_ENTRIES = ("first_block_fwd", "first_block_bwd_wgrad")
# upconv_head_fwd / upconv_head_dgrad / patchgan_head_fwd / conv_dgrad_image are single-form bf16 kernels (one output pixel's sum per thread or wave,
# no launch choice): they have no plan to query. In fp32 / bf16x3 the same layers run through the gather GEMM and ARE in the table below.


def plan_cases():
    """(id, dt, op, pass, H, W, Cin, Cout, flags) of every plan-carrying convolution call of the three compute modes"""
    out = []
    for c in X.CASES:
        bits = 0
        for f in c.flags:
            bits |= FLAG_BITS.get(f, 0)
        if c.entry in GEMM_ENTRIES:
            out.append((f"bf16-{X.case_id(c)}", _lib.DT_BF16, c.op, c.pas, c.H, c.W, c.Cin, c.Cout, bits))
        elif c.entry in FIRST_BLOCK_ENTRIES:
            out.append((f"bf16-{X.case_id(c)}", _lib.DT_BF16, c.op, c.pas, c.H, c.W, c.Cin, c.Cout, PLAN_FIRST_BLOCK))
    for name, dt in (("fp32", _lib.DT_F32), ("bf16x3", _lib.DT_BF16X3)):
        for pas in (0, 1, 2):
            for c in X.fp32_cases(pas):
                layer = next(k for k in X.CASES if k.net == c.net and k.layer == c.layer and k.pas == 0)
                bits = _lib.EP_STATS if (pas == 0 and "stats" in layer.flags) else 0
                out.append((f"{name}-{X.case_id(c)}-p{pas}", dt, c.op, pas, c.H, c.W, c.Cin, c.Cout, bits))
    return out


PLAN_CASES = plan_cases()


def query(lib, case, N, ncu=NCU):
    _, dt, op, pas, H, W, Cin, Cout, flags = case
    rec = (ctypes.c_int * 8)()
    rc = lib.tfc_conv_plan_query(dt, op, pas, N, H, W, Cin, Cout, flags, ncu, rec, 8)
    assert rc == 8, (case, lib.tfc_last_error())
    return tuple(rec)


@pytest.fixture()
def lib():
    lib = _lib.load()
    prev = T.get_batch_invariant()
    yield lib
    T.set_batch_invariant(prev)
    _lib.load()


def test_table_covers_the_three_modes_and_all_passes():
    dts = {c[1] for c in PLAN_CASES}
    assert dts == {_lib.DT_BF16, _lib.DT_F32, _lib.DT_BF16X3}
    for dt in dts:
        assert {c[3] for c in PLAN_CASES if c[1] == dt} == {0, 1, 2}
    assert len(PLAN_CASES) > 150


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_plan_does_not_depend_on_batch_or_chip_when_on(lib, case):
    T.set_batch_invariant(True)
    lib = _lib.load()
    assert lib.tfc_get_batch_invariant() == 1
    want = query(lib, case, 32)
    for N in BATCHES:
        for ncu in (NCU, 64, 304):
            assert query(lib, case, N, ncu) == want, (N, ncu)


def test_plans_do_depend_on_batch_when_off(lib):
    """sensitivity: with the mode off the deep layers change tile form (and with it their InstanceNorm slot count) between N = 1 and N = 32"""
    T.set_batch_invariant(False)
    lib = _lib.load()
    assert lib.tfc_get_batch_invariant() == 0
    differ = [c[0] for c in PLAN_CASES if query(lib, c, 1) != query(lib, c, 32)]
    fwd_or_dgrad = [c[0] for c in PLAN_CASES if c[3] != 2 and query(lib, c, 1)[:3] != query(lib, c, 32)[:3]]
    print("plans that differ between N = 1 and N = 32:", len(differ), "of", len(PLAN_CASES), "; kernel / tile form / slots of a forward or dgrad pass:", fwd_or_dgrad)
    assert differ
    assert fwd_or_dgrad                                            # not only split counts of weight gradients: the per-sample arithmetic moves


@pytest.mark.parametrize("dt,kernel", [(_lib.DT_BF16, 10), (_lib.DT_F32, 10), (_lib.DT_BF16X3, 13)], ids=["bf16", "fp32", "bf16x3"])
def test_weight_gradient_above_the_slab_budget_plans_rounds_not_atomics(lib, dt, kernel):
    """1056 -> 1024 channels are 33 x 16 = 528 (n-block, c-block) pairs, more than the 512 split-K slabs: the layer runs in rounds of 512 pairs in every
    compute mode. The record is the first round's (512 pairs over the 4 one-tile images of batch 4: split 1), and slot 6, once "flushed with float
    atomics", is 0. The 2 x 2-tap kernel (TFC_K_WGRAD22 = 11; a transposed convolution too wide for the phase-fused kernels) does the same."""
    T.set_batch_invariant(False)
    lib = _lib.load()
    rec = query(lib, ("conv4x4-rounds", dt, _lib.OP_CONV, 2, 8, 8, 1056, 1024, 0), 4)
    assert (rec[0], rec[3], rec[6]) == (kernel, 1, 0), rec
    rec = query(lib, ("convT2x2-rounds", dt, _lib.OP_CONVT, 2, 4, 4, 2112, 1024, 0), 4)
    assert (rec[0], rec[3], rec[6]) == (11 if dt == _lib.DT_BF16 else kernel, 1, 0), rec


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_reference_batch_keeps_its_tuned_plan(lib, case):
    T.set_batch_invariant(False)
    off = query(_lib.load(), case, 32)
    T.set_batch_invariant(True)
    assert query(_lib.load(), case, 32) == off


def test_setting_reaches_every_thread(lib):
    """the library's flag is per thread; the package's setting is process-wide and each thread applies it when it next fetches the library"""
    T.set_batch_invariant(True)
    seen = {}

    def other():
        seen["on"] = _lib.load().tfc_get_batch_invariant()
        seen["raw"] = lib.tfc_set_batch_invariant(0)              # this thread only
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"on": 1, "raw": 0}
    assert _lib.load().tfc_get_batch_invariant() == 1
    T.set_batch_invariant(False)
    assert _lib.load().tfc_get_batch_invariant() == 0 and T.get_batch_invariant() is False


@pytest.mark.parametrize("value,want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_env_knob(value, want):
    env = dict(os.environ)
    env.pop("TFC_BATCH_INVARIANT", None)
    if value is not None:
        env["TFC_BATCH_INVARIANT"] = value
    code = ("import tfc_gan_amd as T; from tfc_gan_amd import _lib; "
            "print(T.get_batch_invariant(), _lib.load().tfc_get_batch_invariant())")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(want), "1" if want else "0"]


def test_step_classes_take_the_argument():
    import inspect
    assert inspect.signature(T.TrainStep.__init__).parameters["batch_invariant"].default is None
    assert inspect.signature(T.STN21Step.__init__).parameters["batch_invariant"].default is None
    T.set_batch_invariant(False)
    with T.ops.batch_invariant_scope(True):
        assert T.get_batch_invariant() is True
    with T.ops.batch_invariant_scope(None):
        assert T.get_batch_invariant() is False
    assert T.get_batch_invariant() is False
