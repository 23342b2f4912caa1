"""GPU tests of the localiser at ViT patch 32 and 16 (65 and 257 tokens): the tiled attention pair of csrc/vit.hip against the fp64 restatement
of tests/stn21_edges_ref.py at the bars of tests/test_gpu_42_stn21_edges.py, its agreement with the whole-sequence kernels where both apply, its
determinism and batch invariance, its refusals; the general ViT kernels at the sizes only these patch sizes reach (65 K-slices, the split-K
weight gradient, the unfold at P = 16, a 197 376-wide column sum) on exact integers; and the whole localiser / the STN21 step at patch 32 / 16
by the methods of tests/test_gpu_34_localiser.py.

The tile heights of the tiled kernels are ops.VIT_ATTN_TQ = ops.VIT_ATTN_TK = 64: the token counts run one under, at and one over one tile and
two tiles, besides T = 1, 17 and 257 (four full tiles and one row)."""
import warnings

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from tests import stn21_edges_ref as R
from tests.test_gpu_34_localiser import _inputs, _run, ints, unfold
from tfc_gan_amd import ops, stn21, vit
from tfc_gan_amd._lib import DT_BF16, DT_BF16X3, DT_F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
rel = R.rel_l2
AN, AH, ASCALE = 2, 3, 0.125
TQ, TK = ops.VIT_ATTN_TQ, ops.VIT_ATTN_TK
assert TQ == TK == 64
TOKEN_COUNTS = sorted({1, 17, 64, 65, 257, TQ - 1, TQ, TQ + 1, 2 * TQ - 1, 2 * TQ, 2 * TQ + 1})


def tiled(dt, qkv, do, N, Tt, H, scale):
    qg, dg = qkv.to(DEV), do.to(DEV)
    o, stats = ops.vit_attention_tiled_fwd(dt, qg, N, Tt, H, scale)
    return o, stats, ops.vit_attention_tiled_bwd(dt, dg, qg, o, stats, N, Tt, H, scale)


# ---- 1 - 3: the pair against the fp64 restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tt", TOKEN_COUNTS)
def test_tiled_attention_fp32_token_counts(Tt):
    """fp32 mode against fp64 at the bars of test_attention_fp32_token_counts; at T = 1 its exact identities (P = 1: out = v, dv = dO, dq = dk = 0;
    the saved sum l is 1)"""
    qkv, do = R.attention_inputs(AN, Tt, AH, seed=Tt)
    od, _, dqd = R.attention_model(qkv, do, AN, Tt, AH, ASCALE)
    o, stats, dqkv = tiled(DT_F32, qkv, do, AN, Tt, AH, ASCALE)
    assert tuple(stats.shape) == (AN, AH, 3, Tt) and torch.isfinite(stats).all()
    print(f"tiled fp32 T={Tt}: out {rel(o, od):.2e}, dqkv {rel(dqkv, dqd) if Tt > 1 else 0.0:.2e}")
    assert rel(o, od) < 1e-6
    if Tt == 1:
        g3 = dqkv.reshape(AN, 3, AH * 64).cpu()
        assert torch.equal(stats[:, :, 2].cpu(), torch.ones(AN, AH, 1))
        assert torch.equal(g3[:, :2], torch.zeros(AN, 2, AH * 64)) and torch.equal(g3[:, 2], do)
        assert torch.equal(o.cpu(), qkv.reshape(AN, 3, AH * 64)[:, 2])
    else:
        assert rel(dqkv, dqd) < 1e-5


@pytest.mark.parametrize("Tt", [65, 257])
def test_tiled_attention_fp32_large_logits(Tt):
    """qkv scaled by 10 (logits of about +-100, rows close to one-hot): finite, and the two fp32 bars hold. Plain fp32 logits miss both on the
    CPU (2.9e-6 on the output, 1.8e-5 on dqkv): this holds the hi + lo logits in place."""
    qkv, do = R.attention_inputs(2, Tt, 3, seed=0, gain=10.0)
    od, pd, dqd = R.attention_model(qkv, do, 2, Tt, 3, ASCALE)
    assert pd.max().item() > 0.999
    o, stats, dqkv = tiled(DT_F32, qkv, do, 2, Tt, 3, ASCALE)
    print(f"tiled large logits T={Tt}: out {rel(o, od):.2e}, dqkv {rel(dqkv, dqd):.2e}")
    assert torch.isfinite(o).all() and torch.isfinite(stats).all() and torch.isfinite(dqkv).all()
    assert rel(o, od) < 1e-6 and rel(dqkv, dqd) < 1e-5


@pytest.mark.parametrize("Tt", [17, 65, 129, 257])
def test_tiled_attention_bf16_rounding_points(Tt):
    """bf16 mode against the fp64 restatement that rounds where the kernels round, at the bar of test_attention_bf16_rounding_points"""
    qkv, do = R.attention_inputs(AN, Tt, AH, seed=0)
    od, _, dqd = R.attention_model(qkv, do, AN, Tt, AH, ASCALE, rounding=R.ROUNDINGS)
    o, _, dqkv = tiled(DT_BF16, qkv, do, AN, Tt, AH, ASCALE)
    print(f"tiled bf16 T={Tt}: out {rel(o, od):.2e}, dqkv {rel(dqkv, dqd):.2e}")
    assert rel(o, od) <= 2e-4 and rel(dqkv, dqd) <= 2e-4


# ---- 4: agreement with the whole-sequence kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tt", [17, 64])
@pytest.mark.parametrize("dt,bar_o,bar_g", [(DT_BF16, 2e-4, 2e-4), (DT_F32, 1e-6, 1e-5)])
def test_tiled_attention_agrees_with_whole_sequence_kernels(Tt, dt, bar_o, bar_g):
    qkv, do = R.attention_inputs(AN, Tt, AH, seed=3)
    o, _, dqkv = tiled(dt, qkv, do, AN, Tt, AH, ASCALE)
    o0, probs = ops.vit_attention_fwd(dt, qkv.to(DEV), AN, Tt, AH, ASCALE)
    dqkv0 = ops.vit_attention_bwd(dt, do.to(DEV), qkv.to(DEV), probs, AN, Tt, AH, ASCALE)
    print(f"tiled vs whole-sequence T={Tt} dt={dt}: out {rel(o, o0):.2e}, dqkv {rel(dqkv, dqkv0):.2e}")
    assert rel(o, o0) <= bar_o and rel(dqkv, dqkv0) <= bar_g


# ---- 5: determinism and batch invariance of the pair -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_tiled_attention_deterministic_and_batch_invariant(dt):
    N, Tt, H = 8, 257, 12
    qkv, do = R.attention_inputs(N, Tt, H, seed=5)
    full = tiled(dt, qkv, do, N, Tt, H, ASCALE)
    again = tiled(dt, qkv, do, N, Tt, H, ASCALE)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    o, stats, dqkv = full
    for lo, hi in ((0, 1), (3, 8)):
        po, ps, pg = tiled(dt, qkv[lo * Tt:hi * Tt], do[lo * Tt:hi * Tt], hi - lo, Tt, H, ASCALE)
        assert torch.equal(po, o[lo * Tt:hi * Tt]) and torch.equal(ps, stats[lo:hi]) and torch.equal(pg, dqkv[lo * Tt:hi * Tt])


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------------
def test_tiled_attention_refusals():
    """T = 0, T = 1026 and dt = TFC_DT_BF16X3 on both entry points, and a null pointer: non-zero, a text that names the entry point, and nothing
    launched (the sentinel-filled outputs are untouched). Every buffer is large enough for the largest T passed."""
    lib = ops.lib()
    Tmax = 1026
    qkv = torch.randn(2 * Tmax, 3 * 64, device=DEV)
    do = torch.randn(2 * Tmax, 64, device=DEV)
    out, dqkv = torch.full((2 * Tmax, 64), 7.0, device=DEV), torch.full((2 * Tmax, 3 * 64), 7.0, device=DEV)
    stats, ws = torch.full((2, 1, 3, Tmax), 7.0, device=DEV), torch.full((2, 1, Tmax), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    fwd, bwd = b"tfc_vit_attention_tiled_fwd", b"tfc_vit_attention_tiled_bwd"
    dt_text = b": dt 2: the ViT kernels run bf16 or fp32 only (TFC_DT_BF16X3 is not supported)"
    for dt, Tt, text in ((DT_F32, 0, b": T = 0 tokens (1 <= T <= 1025)"), (DT_BF16, 1026, b": T = 1026 tokens (1 <= T <= 1025)"), (DT_BF16X3, 17, dt_text)):
        assert lib.tfc_vit_attention_tiled_fwd(ops.stream_ptr(), dt, p(qkv), p(out), p(stats), 2, Tt, 1, 0.125) != 0
        assert lib.tfc_last_error() == fwd + text
        assert lib.tfc_vit_attention_tiled_bwd(ops.stream_ptr(), dt, p(do), p(qkv), p(stats), p(dqkv), 2, Tt, 1, 0.125, p(ws)) != 0
        assert lib.tfc_last_error() == bwd + text
    assert lib.tfc_vit_attention_tiled_fwd(ops.stream_ptr(), DT_F32, p(qkv), None, p(stats), 2, 17, 1, 0.125) != 0
    assert lib.tfc_last_error() == fwd + b": null pointer"
    assert lib.tfc_vit_attention_tiled_bwd(ops.stream_ptr(), DT_F32, p(do), p(qkv), p(stats), p(dqkv), 2, 17, 1, 0.125, None) != 0
    assert lib.tfc_last_error() == bwd + b": null pointer"
    torch.cuda.synchronize()
    for t in (out, dqkv, stats, ws):
        assert torch.equal(t, torch.full_like(t, 7.0))


# ---- 7: the general kernels at the new shapes, exact on integers -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_gemm_and_colsum_at_patch16_shapes_exact(dt):
    """fc_loc[0] at patch 16: K = 197 376 = 65 K-slices (|sums| <= 9 * 197 376 < 2^24: exact in fp32 in any order); a weight gradient over
    4128 rows, the first split-K of the TRANS / ROWS form (4128 > 4096: two slices); the position gradient's column sum of width 257 * 768"""
    M, N, K = 3, 64, 257 * 768
    assert (K + 3071) // 3072 == 65
    X, W, b = ints((M, K), 1), ints((N, K), 2), ints((N,), 3)
    y = torch.empty((M, N), device=DEV)
    ops.vit_gemm(dt, M, N, K, X.to(DEV), W.to(DEV), y, bias=b.to(DEV))
    assert torch.equal(y.cpu(), (X.double() @ W.double().T + b.double()).float())
    rows, n_out, k_in = 4128, 70, 96
    dY, Xr = ints((rows, n_out), 4), ints((rows, k_in), 5)
    dw = torch.empty((n_out, k_in), device=DEV)
    ops.vit_gemm(dt, n_out, k_in, rows, dY.to(DEV), Xr.to(DEV), dw, a_mode=ops.VIT_A_TRANS, b_mode=ops.VIT_B_ROWS)
    assert torch.equal(dw.cpu(), (dY.double().T @ Xr.double()).float())
    v = ints((2, K), 6)
    assert torch.equal(ops.vit_colsum(v.to(DEV), 2, K).cpu(), v.double().sum(0).float())


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_patch16_unfold_forms_exact(dt):
    """the patch embedding's three unfold forms at P = 16 on a pair of 2 x 3 x 64 x 64 images: K = 6 * 256 = 1536, 16 patches, 17 tokens"""
    n, P, D, S = 2, 16, 96, 64
    npch, Kp = (S // P) ** 2, 6 * P * P
    assert (npch, Kp) == (16, 1536)
    A, B = ints((n, 3, S, S), 7, -2, 3), ints((n, 3, S, S), 8, -2, 3)
    Wp, bp = ints((D, Kp), 9, -2, 3), ints((D,), 10)
    U = unfold(torch.cat((A, B), 1), P).double()
    x = torch.zeros((n, npch + 1, D), device=DEV)
    ops.vit_gemm(dt, n * npch, D, Kp, A.to(DEV), Wp.to(DEV), x[:, 1:, :], a_mode=ops.VIT_A_UNFOLD, a2=B.to(DEV), c_rg=npch, c_rso=(npch + 1) * D,
                 ldc=D, bias=bp.to(DEV), unfold=(3, S, S, P))
    assert torch.equal(x[:, 1:].cpu(), (U @ Wp.double().T + bp.double()).float().reshape(n, npch, D))
    assert torch.equal(x[:, 0].cpu(), torch.zeros(n, D))
    dX = ints((n, npch + 1, D), 11).to(DEV)
    dXp = dX[:, 1:].reshape(n * npch, D).double().cpu()
    dA, dB = torch.empty((n, 3, S, S), device=DEV), torch.empty((n, 3, S, S), device=DEV)
    ops.vit_gemm(dt, n * npch, Kp, D, dX[:, 1:, :], Wp.to(DEV), dA, a_rg=npch, a_rso=(npch + 1) * D, lda=D, b_mode=ops.VIT_B_ROWS,
                 c_mode=ops.VIT_C_UNFOLD, c2=dB, unfold=(3, S, S, P))
    assert torch.equal(unfold(torch.cat((dA, dB), 1).cpu(), P), (dXp @ Wp.double()).float())
    dW = torch.empty((D, Kp), device=DEV)
    ops.vit_gemm(dt, D, Kp, n * npch, dX[:, 1:, :], A.to(DEV), dW, a_mode=ops.VIT_A_TRANS, lda=D, a_rg=npch, a_rso=(npch + 1) * D,
                 b_mode=ops.VIT_B_UNFOLD, b2=B.to(DEV), unfold=(3, S, S, P))
    assert torch.equal(dW.cpu(), (dXp.T @ U).float())


# ---- 8: the whole localiser against fp64 -------------------------------------------------------------------------------------------------------
def _randomise(net, vt):
    with torch.no_grad():
        vt.cls_token.normal_(0, 0.5)
        vt.positions.normal_(0, 0.5)
        for m in vt.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
        if net is not None:
            net.fc_loc[6].weight.mul_(4.0)


def _net(patch, seed=0):
    torch.manual_seed(seed)
    net = stn21.Net((3, 256, 256), localiser="torch", patch_size=patch)
    _randomise(net, net.localization.vit[0])
    return net


def _run_tokens(vt, A, B, g, dev, hip=False, autocast=False):
    """tokens, dA, dB and the ViT's parameter gradients of sum(tokens * g)"""
    vt.zero_grad(set_to_none=True)
    a, b = A.to(dev).requires_grad_(True), B.to(dev).requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        tok = vit.vit_tokens(vt, a, b) if hip else vt(torch.cat((a, b), 1))
    (tok.float() * g.to(dev)).sum().backward()
    return {"tokens": tok.detach().float(), "dA": a.grad.detach(), "dB": b.grad.detach(), **{k: p.grad.detach().clone() for k, p in vt.named_parameters()}}


def _compare(ref, base, got, dtype, least):
    factor, floor = (2.0, 1e-6) if dtype == torch.float32 else (1.5, 1e-3)
    assert set(got) == set(ref) and len(got) > least
    worst = []
    for k in ref:
        eh, et = rel(got[k], ref[k]), rel(base[k], ref[k])
        worst.append((eh / (et + 1e-30), k, eh, et))
        assert eh <= factor * et + floor, (k, eh, et)
    worst.sort(reverse=True)
    print("largest hip/torch error ratios:", [(k, f"{eh:.2e}", f"{et:.2e}") for _, k, eh, et in worst[:5]])


@pytest.fixture(scope="module")
def fp64_patch32():
    net = _net(32)
    A, B, g = _inputs(4, 31)
    ref = _run(net.double(), A.double(), B.double(), g.double(), "cpu")
    return net.state_dict(), (A, B, g), ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_whole_localiser_patch32_vs_fp64(fp64_patch32, dtype):
    """Net(patch_size=32) at batch 4 by the method of test_whole_localiser_vs_fp64: theta, tokens, dA, dB and every parameter gradient"""
    sd, (A, B, g), ref = fp64_patch32
    net = _net(32)
    net.load_state_dict(sd)
    net = net.float().to(DEV)
    T.set_compute_dtype(dtype)
    try:
        base = _run(net, A, B, g, DEV, autocast=dtype == torch.bfloat16)
        net.localiser = "hip"
        got = _run(net, A, B, g, DEV)
    finally:
        T.set_compute_dtype(torch.bfloat16)
    _compare(ref, base, got, dtype, 160)


@pytest.fixture(scope="module")
def fp64_patch16_tokens():
    torch.manual_seed(0)
    vt = stn21.VisionTransformer(256, 16, 6)
    _randomise(None, vt)
    A, B, _ = _inputs(2, 33)
    g = torch.from_numpy(np.random.default_rng(33).standard_normal((2, 257, 768)).astype(np.float32))
    ref = _run_tokens(vt.double(), A.double(), B.double(), g.double(), "cpu")
    return vt.state_dict(), (A, B, g), ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_vit_tokens_patch16_vs_fp64(fp64_patch16_tokens, dtype):
    """VisionTransformer(256, 16, 6) at batch 2 (257 tokens; without the head, whose 200 M-parameter fc_loc[0] has no place in an fp64 CPU run):
    tokens, dA, dB and the ViT's parameter gradients"""
    sd, (A, B, g), ref = fp64_patch16_tokens
    vt = stn21.VisionTransformer(256, 16, 6)
    vt.load_state_dict(sd)
    vt = vt.float().to(DEV)
    T.set_compute_dtype(dtype)
    try:
        base = _run_tokens(vt, A, B, g, DEV, autocast=dtype == torch.bfloat16)
        got = _run_tokens(vt, A, B, g, DEV, hip=True)
    finally:
        T.set_compute_dtype(torch.bfloat16)
    _compare(ref, base, got, dtype, 150)


# ---- 9: batch invariance and determinism of the whole localiser at patch 16 --------------------------------------------------------------------
@pytest.fixture(scope="module")
def net_patch16():
    net = _net(16, seed=1).to(DEV)
    net.localiser = "hip"
    return net


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_patch16_localiser_batch_invariant_and_deterministic(net_patch16, dtype):
    """batch 8 against [0:1] and [3:8]: theta, tokens, dA and dB bit-identical; two runs: every gradient bit-identical"""
    A, B, g = _inputs(8, 41)
    T.set_compute_dtype(dtype)
    try:
        full = _run(net_patch16, A, B, g, DEV)
        again = _run(net_patch16, A, B, g, DEV)
        for k in full:
            assert torch.equal(full[k], again[k]), k
        del again
        for sl in (slice(0, 1), slice(3, 8)):
            part = _run(net_patch16, A[sl], B[sl], g[sl], DEV)
            for k in ("theta", "tokens", "dA", "dB"):
                assert torch.equal(part[k], full[k][sl]), (dtype, sl, k, (part[k] - full[k][sl]).abs().max().item())
    finally:
        T.set_compute_dtype(torch.bfloat16)


# ---- 10: the STN21 step at patch 16 -------------------------------------------------------------------------------------------------------------
def test_stn21_step_patch16_hip_localiser():
    """one bf16 step at batch 4 with patch_size=16 on the HIP localiser: finite losses, every localiser parameter group but theta_emb moves, and
    two fresh runs from one seed give torch.equal flat gradients"""
    def run():
        torch.manual_seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            st = stn21.STN21Step((3, 256, 256), lpips=None, device=DEV, seed=3, localiser="hip", patch_size=16)
        before = {k: p.detach().clone() for k, p in st.net.named_parameters()}
        A, B = T.synthetic_pairs(4, seed=21)
        out = st.step(A.to(DEV), B.to(DEV))
        torch.cuda.synchronize()
        return st, out, before
    T.set_compute_dtype(torch.bfloat16)
    st, out, before = run()
    assert st.net.localiser == "hip" and st.net.patch_size == 16 and st.net.fc_loc[0].in_features == 257 * 768
    for k in ("loss_G", "loss_GAN", "recon_loss", "perc_loss", "morph_loss", "loss_D"):
        assert torch.isfinite(out[k]).all(), k
    for k, p in st.net.named_parameters():
        if k.startswith("theta_emb"):
            continue                                                # declared and never used by the reference (STN:178)
        assert not torch.equal(before[k], p.detach()), f"{k} did not move"
    gg, dg = st.gflat.grad.clone(), st.dflat.grad.clone()
    del st, before, out
    st2, _, _ = run()
    assert torch.equal(st2.gflat.grad, gg)
    assert torch.equal(st2.dflat.grad, dg)
