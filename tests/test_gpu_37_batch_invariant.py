"""Batch-invariant mode on the GPU: with tfc_gan_amd.set_batch_invariant(True) everything that belongs to one sample -- the generator's
and the discriminator's outputs, every activation / statistic / sign word their contexts keep, the input gradients of their backward passes -- is
bit-identical (torch.equal) whatever batch the sample is computed in, in the three compute modes. Inputs and weights: the oracle's seeded
`synthetic_pairs` / `init_weights_portable`, as the workers use them; the generator runs in eval() (dropout masks are keyed by the local sample index).
"""
import ctypes
import os
import socket
import subprocess
import sys

import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import conv_exact as X
from tfc_gan_amd import nets, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [torch.bfloat16, torch.float32, "bf16x3"]
MODE_IDS = ["bf16", "fp32", "bf16x3"]
SUBS = {32: [(0, 1), (5, 12), (16, 32)], 13: [(12, 13)]}      # batch -> sub-batches [lo, hi) computed on their own


@pytest.fixture()
def invariant():
    prev, prev_dt = T.get_batch_invariant(), T.get_compute_dtype()
    T.set_batch_invariant(True)
    yield
    T.set_batch_invariant(prev)
    T.set_compute_dtype(prev_dt)


_CORES = {}


def cores(mode):
    """GeneratorCore / DiscriminatorCore of `mode` on the portable weights, with gradient buffers of their own"""
    if mode not in _CORES:
        dev = torch.device("cuda", 0)
        dt = ops.dt_of(mode)
        Gm = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(dev).eval()
        Dm = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(dev)
        G, D = nets.GeneratorCore(dt, 3), nets.DiscriminatorCore(dt, 3)
        gp = {k: v.detach().float().contiguous() for k, v in Gm.named_core_params().items()}
        dp = {k: v.detach().float().contiguous() for k, v in Dm.named_core_params().items()}
        G.set_params(gp)
        D.set_params(dp, Dm.named_core_buffers())
        G.repack()
        D.repack()
        _CORES[mode] = (G, D, {k: torch.zeros_like(v) for k, v in gp.items()})
    return _CORES[mode]


def per_sample(obj, N, path="ctx", out=None, seen=None):
    """every tensor below `obj` whose leading dimension is the batch: {path: tensor (logical channels of a View only)}"""
    out = {} if out is None else out
    seen = set() if seen is None else seen
    if obj is None or isinstance(obj, (int, float, str, bool)) or id(obj) in seen:
        return out
    seen.add(id(obj))
    if isinstance(obj, ops.View):
        if obj.t.shape[0] == N:
            out[path] = obj.t[..., obj.coff:obj.coff + obj.C]
    elif isinstance(obj, torch.Tensor):
        if obj.dim() >= 1 and obj.shape[0] == N:
            out[path] = obj
    elif isinstance(obj, (list, tuple)):
        for i, o in enumerate(obj):
            per_sample(o, N, f"{path}[{i}]", out, seen)
    elif isinstance(obj, dict):
        for k, o in obj.items():
            per_sample(o, N, f"{path}[{k!r}]", out, seen)
    elif hasattr(obj, "__dict__"):
        for k, o in vars(obj).items():
            per_sample(o, N, f"{path}.{k}", out, seen)
    return out


def snapshot(obj, N):
    return {k: v.detach().clone() for k, v in per_sample(obj, N).items()}


def compare(full, part, lo, hi, what):
    assert full.keys() == part.keys(), (what, sorted(full.keys() ^ part.keys()))
    bad = [k for k in full if not torch.equal(full[k][lo:hi], part[k])]
    assert not bad, (what, lo, hi, bad)
    return len(full)


def g_run(G, grads, A, gfake):
    fake, ctx = G.forward(A, seed=0, train=False)
    snap = snapshot(ctx, A.shape[0])
    snap["fake"] = fake.detach().clone()
    gx = G.backward(ctx, gfake, grads, need_input_grad=True)
    snap["dx"] = gx.detach().clone()
    torch.cuda.synchronize()
    return snap


def d_run(D, A, B, glog):
    logits, ctx = D.forward(A, B, power_iter=False, save=True)
    N = A.shape[0]
    snap = snapshot(ctx, N)
    snap["logits"] = logits.t[..., logits.coff:logits.coff + 1].detach().clone()
    g = ops.new_act(N, logits.H, logits.W, 8, D.dt, A.device)
    g.t.zero_()
    g.t[..., 0] = glog.to(g.t.dtype)
    gx = D.backward(ctx, g, grads=None, need_input_grad=True)
    snap["dx"] = gx.detach().clone()
    torch.cuda.synchronize()
    return snap


def inputs(N, dev):
    A, B = O.synthetic_pairs(N, seed=63)
    gen = torch.Generator().manual_seed(7)
    gfake = (torch.randn(N, 3, 256, 256, generator=gen) * 1e-3).to(dev)
    glog = (torch.randn(N, 16, 16, generator=gen) * 1e-2).to(dev)
    return A.to(dev), B.to(dev), gfake, glog


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", [32, 13])
def test_generator_forward_backward_per_sample_bits(invariant, mode, N):
    dev = torch.device("cuda", 0)
    G, _, grads = cores(mode)
    A, _, gfake, _ = inputs(N, dev)
    full = g_run(G, grads, A, gfake)
    for lo, hi in SUBS[N]:
        part = g_run(G, grads, A[lo:hi].contiguous(), gfake[lo:hi].contiguous())
        n = compare(full, part, lo, hi, f"G {mode} N={N}")
    print(f"  generator {mode} N={N}: {n} per-sample tensors bit-equal on {SUBS[N]}")
    assert n >= 10


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", [32, 13])
def test_discriminator_forward_backward_per_sample_bits(invariant, mode, N):
    dev = torch.device("cuda", 0)
    _, D, _ = cores(mode)
    A, B, _, glog = inputs(N, dev)
    full = d_run(D, B, A, glog)
    for lo, hi in SUBS[N]:
        part = d_run(D, B[lo:hi].contiguous(), A[lo:hi].contiguous(), glog[lo:hi].contiguous())
        n = compare(full, part, lo, hi, f"D {mode} N={N}")
    print(f"  discriminator {mode} N={N}: {n} per-sample tensors bit-equal on {SUBS[N]}")
    assert n >= 5


def test_sensitivity_default_fp32_generator_differs_between_batch_2_and_1():
    """SENSITIVITY CHECK: with the mode OFF the fp32 generator forward of a sample is not the same in a batch of 2 and a batch of 1 (up to
    7e-6) -- the comparison above can see what the mode removes"""
    dev = torch.device("cuda", 0)
    prev = T.get_batch_invariant()
    T.set_batch_invariant(False)
    try:
        G, _, _ = cores(torch.float32)
        A = O.synthetic_pairs(2, seed=63)[0].to(dev)
        two, _ = G.forward(A, seed=0, train=False, save=False)
        one, _ = G.forward(A[0:1].contiguous(), seed=0, train=False, save=False)
        torch.cuda.synchronize()
        diff = (two[0:1] - one).abs().max().item()
        print(f"  fp32 generator, mode off, sample 0 in a batch of 2 against a batch of 1: max |diff| = {diff:.3e}")
        assert not torch.equal(two[0:1], one)
        T.set_batch_invariant(True)
        two, _ = G.forward(A, seed=0, train=False, save=False)
        one, _ = G.forward(A[0:1].contiguous(), seed=0, train=False, save=False)
        torch.cuda.synchronize()
        assert torch.equal(two[0:1], one)
    finally:
        T.set_batch_invariant(prev)


@pytest.mark.parametrize("streams", [1, 2])
def test_step_is_bit_reproducible_with_the_mode_on(streams):
    dev = torch.device("cuda", 0)
    prev_side = T.set_wgrad_stream(streams == 2)

    def run():
        G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(dev)
        D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(dev)
        ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, batch_invariant=True)
        A, B = O.synthetic_pairs(2, seed=63)
        for _ in range(2):
            out = ts.step(A.to(dev), B.to(dev))
        torch.cuda.synchronize()
        return {"g": ts.gflat.data.clone(), "d": ts.dflat.data.clone(), "fake": out["fake_B"].clone(),
                "loss": torch.stack([out["loss_G"].float(), out["loss_D"].float()]).clone()}
    try:
        assert T.get_batch_invariant() is False
        a, b = run(), run()
        assert T.get_batch_invariant() is False                   # the argument of TrainStep holds inside step() only
    finally:
        T.set_wgrad_stream(prev_side)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_against_two(worker, tmp_path, extra_env, timeout):
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", TFC_BATCH_INVARIANT="1", **extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    subprocess.run([sys.executable, worker, one], check=True, env=env, timeout=timeout)       # child processes, never an exec of this one
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(_free_port()), worker, two], check=True, env=env, timeout=timeout)
    return torch.load(one, weights_only=True), torch.load(two, weights_only=True)


# Bars on the rel-L2 between one rank with the whole batch and two ranks with half each, for the gradients (gg, dg) and for the weights after the Adam
# step (g, d). With the mode on every per-sample quantity is bit-equal, so what is left is the order in which the samples enter the fp32 weight-gradient
# sums (in-kernel split-K on one rank, all-reduce on two): round-off of an fp32 sum; in g / d it shows where Adam's first step, lr * g / (|g| + eps),
# amplifies a gradient of round-off size. Each bar is twice the value measured on the MI355X with the mode on (profiles/batch_invariant_ab.md, which
# also has the mode-off figures of the same session); every reduction has a fixed order, so the figures reproduce to the bit.
PATCH16_BARS = {"gg": 1.9e-6, "dg": 3.5e-7, "g": 6.8e-7, "d": 2.5e-7}     # measured 9.32e-7, 1.72e-7, 3.40e-7, 1.24e-7 (mode off: 1.1e-3, 4.2e-5, 2.9e-4, 2.9e-5)
STN21_BARS = {"gg": 1.2e-7, "dg": 5.1e-7, "g": 2.6e-7, "d": 1.4e-7}        # measured 5.55e-8, 2.54e-7, 1.29e-7, 7.00e-8 (mode off: 7.2e-3, 4.0e-5, 6.4e-4, 1.4e-5)


def _rel_l2_within(a, b, bars, what):
    figures = {k: ((a[k] - b[k]).norm() / a[k].norm()).item() for k in ("gg", "dg", "g", "d")}
    for k, r in figures.items():
        print(f"  {what} {k} rel-L2 {r:.3e} (bar {bars[k]})")
    for k, r in figures.items():
        assert r <= bars[k], (what, k, r)


def test_patch16_two_ranks_match_one_rank_bit_equal_image(tmp_path):
    a, b = _one_against_two(os.path.join(ROOT, "tests", "batch_invariant_ddp_worker.py"), tmp_path, {}, 300)
    assert torch.equal(a["fake_B"], b["fake_B"])
    assert torch.equal(a["logits"], b["logits"])
    _rel_l2_within(a, b, PATCH16_BARS, "PATCH-16")


def test_stn21_two_ranks_match_one_rank_bit_equal_theta_images_logits(tmp_path):
    """theta is the per-sample quantity whose drift with the batch size DESIGN 3.6 blames for the 7.2e-3 of the default mode"""
    a, b = _one_against_two(os.path.join(ROOT, "tests", "batch_invariant_stn21_worker.py"), tmp_path, {"TFC_LOCALISER": "hip"}, 600)
    for k in ("theta", "fake_B", "warped_B", "fake_A2", "logits_D1", "logits_D2"):
        assert a[k].shape[0] == 2 and torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
    assert torch.allclose(a["losses"], b["losses"], rtol=2e-5, atol=1e-6), (a["losses"], b["losses"])
    _rel_l2_within(a, b, STN21_BARS, "STN21")


# ---- weight gradients at batches that have fewer tiles than the reference batch's split count ----------------------------------------------------------
# With the mode on the split count of a weight gradient is the reference batch's; at N = 1 or 2 the deep layers then have fewer pixel tiles than
# splits: the launchers run a shorter split-major grid and zero-fill the slabs no split owns. Every weight-gradient call of the step, in the three
# compute modes, on the SAME x and dy with the mode on and off, through ONE scratch buffer in the engine's call order (stale slabs of the layer before
# lie in it). The two results add the same fp32 products of the same operands and differ only in how the pixel tiles are grouped into partial sums:
# WGRAD_ORDER_BOUND is the 1e-5 rel-L2 that tests/test_gpu_20_ddp.py grants a weight gradient whose samples enter the sum in another order. A slab
# that is missed, read uninitialised or zeroed wrongly moves the result by O(1).
WGRAD_ORDER_BOUND = 1e-5


def _wgrad_cases(mode):
    if mode == torch.bfloat16:
        return [c for c in X.WGRAD_ENGINE_ORDER]
    return X.fp32_cases(2)


def _wgrad_call(dt, c, x, dy, ws, sign_mask, on):
    T.set_batch_invariant(on)
    dw = torch.full(X.weight_shape(c), float("nan"), dtype=torch.float32, device=x.t.device)
    bias = None
    if c.entry == "first_block_bwd_wgrad":
        bias = torch.zeros(c.Cout, dtype=torch.float32, device=x.t.device)
        ws = ops.first_block_bwd_wgrad(dt, x, None, dy, c.Cin, c.Cout, dw, slope=0.2, ws=ws, bias_sums=bias, sign_mask=sign_mask)
    else:
        ws = ops.conv_wgrad(dt, c.op, x, dy, c.Cin, c.Cout, dw, False, ws)
    torch.cuda.synchronize()
    return dw, bias, ws


# test hook 2 keeps the per-phase launches of the transposed convolutions reachable: the 2 x 2-tap kernel behind them exists in bf16 only
@pytest.mark.parametrize("mode,force_cfg", [(torch.bfloat16, -1), (torch.float32, -1), ("bf16x3", -1), (torch.bfloat16, 2)],
                         ids=["bf16", "fp32", "bf16x3", "bf16-per-phase"])
@pytest.mark.parametrize("N", [1, 2])
def test_weight_gradients_with_fewer_tiles_than_splits(mode, N, force_cfg):
    dev = torch.device("cuda", 0)
    dt = ops.dt_of(mode)
    lib = ops.lib()
    prev = T.get_batch_invariant()
    gen = torch.Generator().manual_seed(11)
    ws, worst, shorter = None, ("", 0.0), 0
    try:
        for c in _wgrad_cases(mode):
            if force_cfg == 2 and c.op != X.OP_CONVT:
                continue
            first = c.entry == "first_block_bwd_wgrad"
            OH = 128 if first else X.out_hw(c)
            x = ops.new_act(N, c.H, c.W, ops.pad8(c.Cin), dt, dev, zero=True)
            dy = ops.new_act(N, OH, OH, ops.pad8(c.Cout), dt, dev, zero=True)
            x.t[..., :c.Cin] = torch.randn(N, c.H, c.W, c.Cin, generator=gen).to(dev).to(x.t.dtype)
            dy.t[..., :c.Cout] = torch.randn(N, OH, OH, c.Cout, generator=gen).to(dev).to(dy.t.dtype)
            sign_mask = torch.randint(0, 256, (N, c.H - 1, c.W - 1, 8), generator=gen, dtype=torch.uint8).to(dev) if first else None
            rec_on, rec_off = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
            flags = 0x10000 if first else 0
            T.set_batch_invariant(True)
            assert ops.lib().tfc_conv_plan_query(dt, c.op, 2, N, c.H, c.W, c.Cin, c.Cout, flags, 256, rec_on, 8) == 8
            T.set_batch_invariant(False)
            assert ops.lib().tfc_conv_plan_query(dt, c.op, 2, N, c.H, c.W, c.Cin, c.Cout, flags, 256, rec_off, 8) == 8
            shorter += rec_on[3] > rec_off[3]
            if force_cfg >= 0:
                ops._lib.check(lib.tfc_debug_set_igemm_config(force_cfg), "set cfg")
            off, boff, ws = _wgrad_call(dt, c, x, dy, ws, sign_mask, False)
            on, bon, ws = _wgrad_call(dt, c, x, dy, ws, sign_mask, True)
            assert torch.isfinite(off).all() and torch.isfinite(on).all(), X.case_id(c)
            r = ((on - off).norm() / off.norm()).item()
            print(f"  {MODE_IDS[MODES.index(mode)]} N={N} {X.case_id(c)}: kernel {rec_on[0]} splits {rec_off[3]} -> {rec_on[3]}  rel-L2 {r:.3e}")
            worst = max(worst, (X.case_id(c), r), key=lambda t: t[1])
            assert r <= WGRAD_ORDER_BOUND, (X.case_id(c), r)
            if first:
                rb = ((bon - boff).norm() / boff.norm()).item()
                assert rb <= WGRAD_ORDER_BOUND, (X.case_id(c), "bias sums", rb)
    finally:
        lib.tfc_debug_set_igemm_config(-1)
        T.set_batch_invariant(prev)
    print(f"  worst: {worst}; layers whose planned split count exceeds the default one at this batch: {shorter}")
    assert force_cfg == 2 or shorter >= 1                         # the case this test exists for does occur at this batch


def test_fft_amplitude_and_phase_per_sample_bits(invariant):
    """contract item 3: the per-window amplitude / phase spectra of the FFT loss are per-sample buffers (one workgroup per window, no launch choice
    depends on the batch): a sample's windows are the same bits in any batch. The triplet and BCE heads keep no per-sample value: their kernels add
    straight into the batch scalar."""
    dev = torch.device("cuda", 0)
    img = O.synthetic_pairs(13, seed=63)[1].to(dev)
    for S, wins in ((64, 4), (256, 1)):
        amp, pha = ops.fft_spectrum(img, S, wins, wins)
        per = wins * wins
        for lo, hi in ((0, 1), (5, 12), (12, 13)):
            a1, p1 = ops.fft_spectrum(img[lo:hi].contiguous(), S, wins, wins)
            assert torch.equal(amp[lo * per:hi * per], a1) and torch.equal(pha[lo * per:hi * per], p1), (S, lo, hi)
