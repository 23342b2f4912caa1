"""GPU tests of the STN21 kernels (csrc/vit.hip, csrc/stn.hip, tfc_row_triplet_kernel of csrc/losses.hip) at the launch and shape edges that
tests/test_gpu_34_localiser.py and tests/test_gpu_30_stn.py do not reach. Every case is the smallest shape that takes its branch, and the
arithmetic that shows it does stands in the test's docstring:

  row-chunked split-K (m0 > 0, ragged last chunk) and K % 32 != 0      test_gemm_chunked_split_k_*, test_gemm_ragged_k_*
  attention at T = 1..3, 42 / 43 and 63 / 64 (the 64 KiB LDS line)     test_attention_fp32_token_counts, test_attention_bf16_rounding_points
  LayerNorm at D = 64 / 1024, ragged rows, zero variance, offset      test_layernorm_*
  column sums with ld > L, the token kernel                          test_colsum_*, test_tokens_*
  row triplets past their grid caps (2048 / 512 workgroups)           test_row_triplet_*
  morphological gradient on ties and one-pixel planes                 test_morph_gradient_on_ties_and_thin_planes
  warp with every tap clipped, H or W = 2, theta-only backward        test_warp_*
  refusals: message texts, and a refused call launches nothing        test_*_refusals

References are fp64 (or exact integers); the shared restatements live in tests/stn21_edges_ref.py and are checked on the CPU by
tests/test_stn21_edges_host.py."""
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from tests import stn21_edges_ref as R
from tests.test_gpu_30_stn import ref_morph_gradient, ref_warp, rnd
from tfc_gan_amd import ops
from tfc_gan_amd._lib import DT_BF16, DT_BF16X3, DT_F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
rel = R.rel_l2


def ints(shape, seed, lo=-3, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).float()


def last_error():
    return ops.lib().tfc_last_error()


# ---- A. GEMM -----------------------------------------------------------------------------------------------------------------------------------
CHUNK_M, CHUNK_N, CHUNK_K = 711, 6144, 4100


@pytest.fixture(scope="module")
def chunked_case():
    """operands in -3..3 and the exact X Wt of (711, 6144, 4100): |sums| <= 9 * 4100 < 2^24, so an fp32 CPU matmul is exact in any order"""
    X, W, b, Rs = ints((CHUNK_M, CHUNK_K), 1), ints((CHUNK_N, CHUNK_K), 2), ints((CHUNK_N,), 3), ints((CHUNK_M, CHUNK_N), 4)
    prod = X @ W.T
    assert prod.abs().max().item() < 2 ** 24
    return {"X": X.to(DEV), "W": W.to(DEV), "b": b, "R": Rs, "prod": prod}


def _assert_chunked(M, N, K):
    """K = 4100 > 4096: 129 K-tiles in 2 slices of 65 tiles = 2080 and 2020 columns, the second ending in a 4-wide tile (4100 = 128 * 32 + 4).
    Rows per launch: floor(part_ws / (2 * 6144) / 64) * 64 = 640 with the 8 388 608-float scratch; M = 711 gives two launches, the second with
    m0 = 640 and 71 rows (one full tile and one of 7 rows). Computed from tfc_part_ws_floats() so that a scratch of another size fails here."""
    assert 4096 < K <= 2 * 3072 and K % 32 == 4
    cap = ops.lib().tfc_part_ws_floats() // (2 * N) // 64 * 64
    assert 64 <= cap < M and 0 < (M - cap) % 64 < 64 and M - cap > 64, (cap, M)
    assert cap == 640


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_gemm_chunked_split_k_exact(chunked_case, dt):
    """gap 1 + 2: Y = X Wt + b + residual through tfc_launch_vit_gemm's row-chunk loop (see _assert_chunked): part[z][row - m0][n], the reduce
    kernel's m0 + idx / N and the ragged last chunk, with a short last K tile in the last slice. torch.equal to the exact integers."""
    M, N, K = CHUNK_M, CHUNK_N, CHUNK_K
    _assert_chunked(M, N, K)
    c = chunked_case
    want = c["prod"] + c["b"] + c["R"]
    y = torch.full((M, N), float("nan"), device=DEV)
    ops.vit_gemm(dt, M, N, K, c["X"], c["W"], y, bias=c["b"].to(DEV), res=c["R"].to(DEV))
    got = y.cpu()
    bad = (got != want).nonzero()
    assert torch.equal(got, want), (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_gemm_chunked_split_k_gelu_epilogue(chunked_case, dt):
    """the same two launches with the GELU epilogue behind the reduce: aux (the pre-activation) is exact for all 711 rows, which pins the
    epilogue's row m0 + idx / N in both C and aux; operands scaled by 1/8 (exact) as in test_gemm_activation_epilogues"""
    M, N, K = CHUNK_M, CHUNK_N, CHUNK_K
    _assert_chunked(M, N, K)
    c = chunked_case
    pre = (c["prod"] + c["b"] + c["R"]) / 8
    aux = torch.full((M, N), float("nan"), device=DEV)
    y = torch.full((M, N), float("nan"), device=DEV)
    ops.vit_gemm(dt, M, N, K, c["X"], c["W"] / 8, y, bias=(c["b"] / 8).to(DEV), res=(c["R"] / 8).to(DEV), act=ops.VIT_ACT_GELU, aux=aux)
    assert torch.equal(aux.cpu(), pre)
    torch.testing.assert_close(y.cpu(), F.gelu(pre.double()).float(), rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
def test_gemm_ragged_k_without_split(dt):
    """gap 2: K % 32 != 0 and K < 32 with one K-slice: the k >= kend -> 0 padding of ld_a / ld_b in the loaders that walk the row index across
    lanes (weight-gradient form: A transposed, B rows) and in the mixed pair of the dgrad form (A rows, B rows). Exact integers."""
    for i, (M, N, K) in enumerate([(5, 70, 37), (64, 64, 1), (65, 33, 31), (17, 6, 100)]):
        A, B = ints((K, M), 20 + 2 * i), ints((K, N), 21 + 2 * i)
        c = torch.full((M, N), float("nan"), device=DEV)
        ops.vit_gemm(dt, M, N, K, A.to(DEV), B.to(DEV), c, a_mode=ops.VIT_A_TRANS, b_mode=ops.VIT_B_ROWS)
        assert torch.equal(c.cpu(), (A.double().T @ B.double()).float()), ("wgrad", M, N, K)
    M, N, K = 17, 100, 70
    A, B = ints((M, K), 30), ints((K, N), 31)
    c = torch.full((M, N), float("nan"), device=DEV)
    ops.vit_gemm(dt, M, N, K, A.to(DEV), B.to(DEV), c, b_mode=ops.VIT_B_ROWS)
    assert torch.equal(c.cpu(), (A.double() @ B.double()).float()), ("dgrad", M, N, K)


def test_gemm_refusals():
    """gap 7: the dt, ldb and aux checks of tfc_vit_gemm with their texts; a refused call launches nothing (C keeps its fill)"""
    M, N, K = 5, 70, 37
    A, B = ints((M, K), 40).to(DEV), ints((N, K), 41).to(DEV)
    c = torch.full((M, N), 7.0, device=DEV)
    for kw, dt, text in (({}, DT_BF16X3, b"tfc_vit_gemm: dt 2 (bf16 or fp32 only; the ViT kernels do not support TFC_DT_BF16X3)"),
                         ({"ldb": K - 1}, DT_F32, b"tfc_vit_gemm: ldb"),
                         ({"act": ops.VIT_DACT_GELU}, DT_F32, b"tfc_vit_gemm: aux")):
        with pytest.raises(T.TfcError):
            ops.vit_gemm(dt, M, N, K, A, B, c, **kw)
        assert last_error() == text
    torch.cuda.synchronize()
    assert torch.equal(c, torch.full_like(c, 7.0))


# ---- B. LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, g, b, dy):
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, g, b))
    yd = F.layer_norm(xd, (x.shape[-1],), gd, bd, 1e-6)
    yd.backward(dy.double())
    return yd.detach(), xd.grad, gd.grad, bd.grad


@pytest.mark.parametrize("rows,D", [(1, 64), (5, 64), (7, 1024), (3, 768)])
def test_layernorm_widths_and_ragged_rows_vs_fp64(rows, D):
    """gap 5: D = 64 (one value per lane, nv = 1), D = 1024 (nv = 16, the whole register array), and row counts that are no multiple of the 4
    rows of a workgroup (1, 5, 7, 3: the last workgroup has idle waves); with and without the residual gradient and the gamma / beta sums"""
    torch.manual_seed(rows * 1000 + D)
    x, g, b, dy, dres = torch.randn(rows, D) * 3 + 1, torch.randn(D), torch.randn(D), torch.randn(rows, D), torch.randn(rows, D)
    yd, dxd, dgd, dbd = _ln_ref(x, g, b, dy)
    y, mean, rstd = ops.vit_layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV))
    assert rel(y, yd) < 1e-6
    assert rel(mean, x.double().mean(-1)) < 1e-6 and rel(rstd, (x.double().var(-1, unbiased=False) + 1e-6).rsqrt()) < 1e-6
    dx, dgb = ops.vit_layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV), dres=dres.to(DEV))
    assert rel(dx, dxd + dres.double()) < 1e-5
    assert rel(dgb[0], dgd) < 1e-5 and rel(dgb[1], dbd) < 1e-5
    dx2, none = ops.vit_layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV), dres=None, want_gb=False)
    assert none is None and rel(dx2, dxd) < 1e-5


def test_layernorm_gamma_beta_sums_over_ten_chunks():
    """301 rows of 768: ten 32-row chunks of tfc_vit_colsum_kernel, the last with 13 rows, more chunks than the eight part-lanes of the
    fixed-order reduce behind it"""
    torch.manual_seed(301)
    rows, D = 301, 768
    x, g, b, dy = torch.randn(rows, D) * 2 - 1, torch.randn(D), torch.randn(D), torch.randn(rows, D)
    _, _, dgd, dbd = _ln_ref(x, g, b, dy)
    _, mean, rstd = ops.vit_layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV))
    _, dgb = ops.vit_layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV))
    assert rel(dgb[0], dgd) < 1e-5 and rel(dgb[1], dbd) < 1e-5


def test_layernorm_zero_variance_row():
    """a row of 0.5s between random rows: mean exactly 0.5, so y = beta exactly, rstd = 1 / sqrt(eps) = 1000, dx finite and right"""
    torch.manual_seed(5)
    rows, D = 5, 768
    x = torch.randn(rows, D)
    x[2] = 0.5
    g, b, dy = torch.randn(D), torch.randn(D), torch.randn(rows, D)
    _, dxd, _, _ = _ln_ref(x, g, b, dy)
    y, mean, rstd = ops.vit_layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV))
    assert torch.equal(y[2].cpu(), b) and mean[2].item() == 0.5
    assert abs(rstd[2].item() - 1000.0) <= 1e-6 * 1000.0
    dx, _ = ops.vit_layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV))
    assert torch.isfinite(dx).all()
    assert rel(dx, dxd) < 1e-5 and rel(dx[2], dxd[2]) < 1e-5


def test_layernorm_large_common_offset():
    """x = 1000 + N(0, 1), D = 1024: fp32 itself limits the result (the mean is rounded to ulp(1000) = 6e-5), so the bar is 4x the error of
    torch's own fp32 CPU F.layer_norm / autograd against fp64 on the same tensors, + 1e-6 (CPU: torch 2.2e-5 forward, so a bar of 9e-5; a
    two-pass fp32 model 2.4e-5; a one-pass variance 3.5e-2 -- tests/test_stn21_edges_host.py). Measured on the MI355X: see the printed line."""
    torch.manual_seed(0)
    rows, D = 7, 1024
    x = 1000 + torch.randn(rows, D)
    g, b, dy = torch.randn(D), torch.randn(D), torch.randn(rows, D)
    yd, dxd, dgd, dbd = _ln_ref(x, g, b, dy)
    xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, g, b))
    yt = F.layer_norm(xt, (D,), gt, bt, 1e-6)
    yt.backward(dy)
    y, mean, rstd = ops.vit_layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV))
    dx, dgb = ops.vit_layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, g.to(DEV))
    for name, got, torch32, want in (("y", y, yt, yd), ("dx", dx, xt.grad, dxd), ("dgamma", dgb[0], gt.grad, dgd), ("dbeta", dgb[1], bt.grad, dbd)):
        e, et = rel(got, want), rel(torch32, want)
        print(f"large-offset LayerNorm {name}: kernel {e:.2e}, torch fp32 {et:.2e}, bar {4 * et + 1e-6:.2e}")
    for name, got, torch32, want in (("y", y, yt, yd), ("dx", dx, xt.grad, dxd), ("dgamma", dgb[0], gt.grad, dgd), ("dbeta", dgb[1], bt.grad, dbd)):
        assert rel(got, want) <= 4 * rel(torch32, want) + 1e-6, name


def test_layernorm_refusals():
    """gap 7: D > 1024, D % 64 != 0 and rows = 0 are refused with `bad args`, forward and backward, and nothing is launched"""
    lib = ops.lib()
    buf = torch.randn(4, 1088, device=DEV)
    g = torch.ones(1088, device=DEV)
    y, dx = torch.full((4, 1088), 7.0, device=DEV), torch.full((4, 1088), 7.0, device=DEV)
    mean, rstd = torch.full((4,), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    for rows, D in ((4, 1088), (4, 96), (0, 768)):
        assert lib.tfc_vit_layernorm_fwd(ops.stream_ptr(), p(buf), p(g), p(g), p(y), p(mean), p(rstd), rows, D, 1e-6) != 0
        assert last_error() == b"bad args"
        assert lib.tfc_vit_layernorm_bwd(ops.stream_ptr(), p(buf), p(buf), p(mean), p(rstd), p(g), None, p(dx), None, rows, D, ops.part_ws(torch.device(DEV))) != 0
        assert last_error() == b"bad args"
    torch.cuda.synchronize()
    for t in (y, dx, mean, rstd):
        assert torch.equal(t, torch.full_like(t, 7.0))


# ---- C. attention ------------------------------------------------------------------------------------------------------------------------------
AN, AH, ASCALE = 2, 3, 0.125


@pytest.mark.parametrize("Tt", [1, 2, 3, 42, 43, 63, 64])
def test_attention_fp32_token_counts(Tt):
    """gap 3: dynamic LDS is 4 T 65 4 B forward and 6 T 65 4 B backward. T = 42: 43 680 / 65 520 B, T = 43: 44 720 / 67 080 B (the backward's
    first launch above 64 KiB = 65 536 B, through hipFuncSetAttribute); T = 63: 65 520 / 98 280 B, T = 64: 66 560 / 99 840 B (the forward's first,
    and every lane of the softmax row live). T < 4 leaves whole waves without a row in the `i = w; i < T; i += 4` loops."""
    qkv, do = R.attention_inputs(AN, Tt, AH, seed=Tt)
    od, pd, dqd = R.attention_model(qkv, do, AN, Tt, AH, ASCALE)
    o, probs = ops.vit_attention_fwd(DT_F32, qkv.to(DEV), AN, Tt, AH, ASCALE)
    dqkv = ops.vit_attention_bwd(DT_F32, do.to(DEV), qkv.to(DEV), probs, AN, Tt, AH, ASCALE)
    assert rel(o, od) < 1e-6 and rel(probs, pd) < 1e-6
    assert (probs.double().sum(-1) - 1).abs().max().item() <= 4 * 2.0 ** -23
    if Tt == 1:
        g3 = dqkv.reshape(AN, 3, AH * 64).cpu()
        assert torch.equal(probs.cpu(), torch.ones(AN, AH, 1, 1))
        assert torch.equal(g3[:, :2], torch.zeros(AN, 2, AH * 64)) and torch.equal(g3[:, 2], do)
        assert torch.equal(o.cpu(), qkv.reshape(AN, 3, AH * 64)[:, 2])
    else:
        assert rel(dqkv, dqd) < 1e-5


def test_attention_fp32_large_logits():
    """qkv scaled by 10: logits of about +-100, softmax rows close to one-hot; finite, and at the same bars against fp64 on the fp32 inputs.
    This test found the forward keeping each logit in one fp32: at |logit| = 100 that is 4e-6 absolute, which is the relative error of every
    small probability, and dq / dk of a nearly one-hot row consist of those. Measured on the MI355X with the 64-term fmaf chain: output 1.01e-6,
    probabilities 1.02e-6 (bar 1e-6), dqkv 6.6e-6; with four partial sums 6.4e-7 / 6.6e-7 but dqkv 1.08e-5 (bar 1e-5); other seeds reach 3e-5 on
    the CPU in any fp32 order. The kernel now carries q.k as hi + lo (compensated dot product) until the row maximum is subtracted: 2.7e-8 on
    the output, 2.2e-8 on the probabilities and 3.3e-7 on dqkv on the MI355X."""
    Tt = 17
    qkv, do = R.attention_inputs(AN, Tt, AH, seed=0, gain=10.0)
    od, pd, dqd = R.attention_model(qkv, do, AN, Tt, AH, ASCALE)
    assert (qkv.double().reshape(AN, Tt, 3, AH, 64)[:, :, 0].abs().max() > 30) and pd.max().item() > 0.999
    o, probs = ops.vit_attention_fwd(DT_F32, qkv.to(DEV), AN, Tt, AH, ASCALE)
    dqkv = ops.vit_attention_bwd(DT_F32, do.to(DEV), qkv.to(DEV), probs, AN, Tt, AH, ASCALE)
    print(f"large logits: out {rel(o, od):.2e}, probs {rel(probs, pd):.2e}, dqkv {rel(dqkv, dqd):.2e}")
    assert torch.isfinite(o).all() and torch.isfinite(probs).all() and torch.isfinite(dqkv).all()
    assert rel(o, od) < 1e-6 and rel(probs, pd) < 1e-6 and rel(dqkv, dqd) < 1e-5


@pytest.mark.parametrize("Tt", [2, 17, 43, 64])
def test_attention_bf16_rounding_points(Tt):
    """gap 4: the bf16 kernels against the fp64 restatement that rounds where they round (q, k, v, dO on load; P before P v and Pt dO, the saved
    probabilities staying fp32; dS before its products). Bar: rel-L2 2e-4 on the output and on dqkv. On the CPU an fp32 emulation of the same
    roundings is within 5e-5 (6e-8 apart from a handful of bf16 tie flips of dS, each worth about 1.5e-5 at T = 64), and every single omitted
    rounding moves one of the two by more than 1.2e-3 (tests/test_stn21_edges_host.py). Measured on the MI355X: see the printed line."""
    qkv, do = R.attention_inputs(AN, Tt, AH, seed=0)
    od, pd, dqd = R.attention_model(qkv, do, AN, Tt, AH, ASCALE, rounding=R.ROUNDINGS)
    o, probs = ops.vit_attention_fwd(DT_BF16, qkv.to(DEV), AN, Tt, AH, ASCALE)
    dqkv = ops.vit_attention_bwd(DT_BF16, do.to(DEV), qkv.to(DEV), probs, AN, Tt, AH, ASCALE)
    print(f"bf16 attention T={Tt}: out {rel(o, od):.2e}, probs {rel(probs, pd):.2e}, dqkv {rel(dqkv, dqd):.2e}")
    assert rel(o, od) <= 2e-4 and rel(dqkv, dqd) <= 2e-4
    assert rel(probs, pd) < 1e-6                                   # the saved probabilities are fp32 softmax values of the rounded q, k


def test_attention_refusals():
    """gap 7: T = 65, T = 0 and dt = TFC_DT_BF16X3, forward and backward, with their texts; nothing is launched"""
    lib = ops.lib()
    qkv = torch.randn(2 * 65, 3 * 64, device=DEV)
    do = torch.randn(2 * 65, 64, device=DEV)
    out, probs, dqkv = torch.full((2 * 65, 64), 7.0, device=DEV), torch.full((2, 1, 65, 65), 7.0, device=DEV), torch.full((2 * 65, 3 * 64), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    dt_text = b"dt 2: the ViT kernels run bf16 or fp32 only (TFC_DT_BF16X3 is not supported)"
    for dt, Tt, text in ((DT_F32, 65, b"bad args"), (DT_BF16, 0, b"bad args"), (DT_BF16X3, 17, dt_text)):
        assert lib.tfc_vit_attention_fwd(ops.stream_ptr(), dt, p(qkv), p(out), p(probs), 2, Tt, 1, 0.125) != 0
        assert last_error() == text
        assert lib.tfc_vit_attention_bwd(ops.stream_ptr(), dt, p(do), p(qkv), p(probs), p(dqkv), 2, Tt, 1, 0.125) != 0
        assert last_error() == text
    torch.cuda.synchronize()
    for t in (out, probs, dqkv):
        assert torch.equal(t, torch.full_like(t, 7.0))


# ---- D. column sums and tokens -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,L,ld", [(1, 1, 1), (33, 257, 257), (300, 768, 768), (45, 5, 2304)])
def test_colsum_exact_at_ragged_sizes_and_row_pitch(rows, L, ld):
    """gap 6: one element; a second, one-row chunk and a second, one-column workgroup (33 = 32 + 1, 257 = 256 + 1); ten chunks (300 = 9 * 32 + 12);
    and ld > L: five columns out of rows 2304 apart, read from the middle of a wider tensor. Integers: exact in any order."""
    base = ints((rows, ld), rows + L).to(DEV)
    c0 = 100 if ld > L else 0
    view = base[:, c0:c0 + L]
    assert view.data_ptr() == base.data_ptr() + 4 * c0
    got = ops.vit_colsum(view, rows, L, ld=ld)
    assert torch.equal(got.cpu(), base.cpu()[:, c0:c0 + L].double().sum(0).float())


@pytest.mark.parametrize("N,Tt,D", [(3, 17, 768), (2, 1, 64)])
def test_tokens_fwd_exact(N, Tt, D):
    """gap 6: x[n][0] = cls + pos[0] whatever x held there (NaN here); x[n][t] += pos[t]: one fp32 add per element, so torch.equal"""
    torch.manual_seed(N + Tt)
    x, cls, pos = torch.randn(N, Tt, D), torch.randn(D), torch.randn(Tt, D)
    want = x.clone()
    want[:, 0] = cls
    want = want + pos
    x[:, 0] = float("nan")
    xg = x.to(DEV)
    ops.vit_tokens_fwd(xg, cls.to(DEV), pos.to(DEV))
    assert torch.equal(xg.cpu(), want)


# ---- E. row triplets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", R.TRIPLET_WIDTHS)
def test_row_triplet_grad_second_ragged_trip(W):
    """gap 8: tfc_row_triplet_grad_kernel runs at most 2048 workgroups x 4 waves = 8192 rows per trip of its grid-stride loop; 8200 rows give a
    second trip that carries 8 rows (two workgroups). W = 3 and 20 leave lanes idle, 64 fills the wave, 65 and 130 take a second and third pass
    of the lane loop with 1 and 2 live lanes. Active and inactive hinges alternate row by row; no row is within 0.05 of the knife edge
    (asserted on the fp64 reference, nothing excluded). Against nn.TripletMarginLoss in fp64 on the same fp32 values, at the existing bars."""
    rows = R.TRIPLET_ROWS
    assert rows > 2048 * 4 and (rows - 2048 * 4) == 8
    a, p, n = R.triplet_rows(rows, W, seed=W)
    want, ga, hinge = R.triplet_ref(a, p, n)
    assert hinge.abs().min().item() >= R.TRIPLET_MARGIN
    active = hinge > 0
    assert active.any() and (~active).any()
    a2 = a.to(DEV).requires_grad_(True)
    got = T.triplet_margin_rows(a2, p.to(DEV), n.to(DEV))
    assert abs(got.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item())), (got.item(), want.item())
    (g2,) = torch.autograd.grad(got, a2)
    g2 = g2.cpu()
    assert (g2.double() - ga).abs().max().item() <= 1e-7 + 1e-5 * ga.abs().max().item()
    assert torch.equal(g2[~active], torch.zeros_like(g2[~active]))
    assert torch.equal(g2[-8:] != 0, ga[-8:] != 0) and active[-8:].any()   # the ragged trip wrote its rows
    nograd = T.triplet_margin_rows(a.to(DEV), p.to(DEV), n.to(DEV))   # da == nullptr: the same loss bits
    assert torch.equal(nograd, got.detach())


@pytest.mark.parametrize("rows,W", [(2050, 5), (8192, 256)])
def test_row_triplet_temperature_head_past_its_grid_cap(rows, W):
    """gap 8: tfc_row_triplet_kernel runs at most 512 workgroups = 2048 rows per trip. 2050 rows: a second trip of 2 rows; 8192 x 256 is the
    batch-32 shape of the temperature head: four full trips. Against fp64, at the existing bar of 1e-5."""
    a, p, n = rnd((rows, W), 1), rnd((rows, W), 2), rnd((rows, W), 3)
    want = F.triplet_margin_loss(a.double(), p.double(), n.double(), margin=1.0, p=2).item()
    got = ops.row_triplet(a.to(DEV), p.to(DEV), n.to(DEV)).item()
    assert abs(got - want) < 1e-5, (got, want)


# ---- F. morphological gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed,pad_rows", R.MORPH_CASES)
def test_morph_gradient_on_ties_and_thin_planes(shape, seed, pad_rows):
    """gap 9: values in {0, 1/4, .., 1}, so maxima and minima tie everywhere, and three equal leading rows as the warp's border padding leaves
    them. The kernel takes the first maximum / minimum in the order centre, up, down, left, right; ref_morph_gradient under torch autograd
    follows the same rule (checked on the CPU in tests/test_stn21_edges_host.py). Forward and backward are exact (integer upstream gradient),
    and every plane's dx sums to exactly 0. Planes of one row, one column and one pixel have no neighbour on one or both axes."""
    x, go = R.morph_case(shape, seed, pad_rows)
    xr = x.clone().requires_grad_(True)
    want = ref_morph_gradient(xr)
    (gx,) = torch.autograd.grad(want, xr, go)
    if pad_rows:
        assert (want == 0).any()                                    # whole plateaus: the data really has ties
    x2 = x.to(DEV).requires_grad_(True)
    got = T.morph_gradient(x2)
    assert torch.equal(got.detach().cpu(), want.detach())
    (g2,) = torch.autograd.grad(got, x2, go.to(DEV))
    assert torch.equal(g2.cpu(), gx)
    assert torch.equal(g2.sum((-2, -1)).cpu(), torch.zeros(shape[:-2]))


# ---- G. warp -----------------------------------------------------------------------------------------------------------------------------------
IDENT = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]])


def _warp_both(src, theta, go_seed=3):
    """torch's affine_grid + grid_sample with autograd on the CPU, and the kernels; asserts the three existing bars"""
    src, theta = src.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    want = ref_warp(src, theta)
    go = rnd(tuple(want.shape), go_seed)
    gsrc, gth = torch.autograd.grad(want, (src, theta), go)
    s2, t2 = src.detach().to(DEV).requires_grad_(True), theta.detach().to(DEV).requires_grad_(True)
    got = T.affine_warp(s2, t2)
    g2s, g2t = torch.autograd.grad(got, (s2, t2), go.to(DEV))
    assert (got.cpu() - want.detach()).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item())
    assert (g2s.cpu() - gsrc).abs().max().item() <= 1e-4 * max(1.0, gsrc.abs().max().item())
    assert (g2t.cpu() - gth).abs().max().item() <= 2e-3 * max(1.0, gth.abs().max().item()), (g2t.cpu(), gth)
    return got.detach().cpu(), g2s.cpu(), g2t.cpu(), go


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 2, 2), (1, 1, 2, 5), (2, 3, 5, 2), (1, 3, 17, 300)])
def test_warp_minimal_and_ragged_sizes_vs_torch(N, C, H, W):
    """gap 10: H = 2 or W = 2, where every sample's four taps clip to the two rows / columns there are; and 17 x 300 = 5100 pixels = 19 * 256 +
    236: a partly filled last workgroup and 20 partial-sum slots per image behind the theta gradient"""
    _warp_both(rnd((N, C, H, W), 1), IDENT[None] + rnd((N, 2, 3), 2, 0.2))


def test_warp_whole_grid_right_of_the_source():
    """gap 10: a translation by +3 in normalised x puts every sample at x >= 1.5 (W - 1), so all 16 taps clip to the last column: the output is
    that column broadcast (H - 1 = 32 makes the base grid's y exact), the source gradient has mass in that column only, and d theta agrees
    with torch's"""
    N, C, H, W = 2, 3, 33, 70
    src = torch.rand((N, C, H, W), generator=torch.Generator().manual_seed(1))   # image values in [0, 1): the 1e-6 below is absolute
    theta = IDENT[None].repeat(N, 1, 1)
    theta[:, 0, 2] = 3.0
    out, gs, _, go = _warp_both(src, theta)
    print(f"clipped warp: max |out - last column| {(out - src[..., -1:].expand_as(src)).abs().max().item():.2e}")
    assert (out - src[..., -1:].expand_as(src)).abs().max().item() <= 1e-6
    assert torch.equal(gs[..., :-1], torch.zeros_like(gs[..., :-1])) and gs[..., -1].abs().min().item() > 0
    assert (gs[..., -1] - go.sum(-1)).abs().max().item() <= 1e-4 * max(1.0, go.sum(-1).abs().max().item())


def test_warp_quarter_turn_on_a_non_square_source():
    """a 90 degree rotation [[0, -1, 0], [1, 0, 0]] of a 33 x 70 source: x walks with the output's rows and y with its columns"""
    N = 2
    theta = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0]])[None].repeat(N, 1, 1)
    _warp_both(rnd((N, 3, 33, 70), 4), theta)


def test_warp_theta_only_backward_gives_the_same_bits():
    """gap 10: a source that does not require grad takes the dsrc == nullptr path of tfc_affine_warp_bwd_kernel; d theta is bit-equal to the
    call that also scatters the source gradient"""
    N, C, H, W = 2, 3, 17, 300
    src, theta = rnd((N, C, H, W), 1).to(DEV), (IDENT[None] + rnd((N, 2, 3), 2, 0.2)).to(DEV)
    go = rnd((N, C, H, W), 3).to(DEV)
    s2, t2 = src.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    _, g_both = torch.autograd.grad(T.affine_warp(s2, t2), (s2, t2), go)
    t3 = theta.clone().requires_grad_(True)
    (g_theta,) = torch.autograd.grad(T.affine_warp(src, t3), t3, go)
    assert torch.equal(g_theta, g_both) and g_theta.abs().min().item() > 0


def test_warp_refusals():
    """gap 11: H = 1 (and W = 1) are refused with `bad args`, forward and backward, and nothing is launched"""
    lib = ops.lib()
    src, theta = torch.randn(1, 1, 1, 8, device=DEV), IDENT.reshape(1, 6).to(DEV)
    out, dth, dsrc = torch.full((1, 1, 1, 8), 7.0, device=DEV), torch.full((1, 6), 7.0, device=DEV), torch.full((1, 1, 1, 8), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    for H, W in ((1, 8), (8, 1)):
        assert lib.tfc_affine_warp_fwd(ops.stream_ptr(), p(src), p(theta), p(out), 1, 1, H, W) != 0
        assert last_error() == b"bad args"
        assert lib.tfc_affine_warp_bwd(ops.stream_ptr(), p(src), p(theta), p(src), p(dth), p(dsrc), 1, 1, H, W, ops.part_ws(torch.device(DEV))) != 0
        assert last_error() == b"bad args"
    torch.cuda.synchronize()
    for t in (out, dth, dsrc):
        assert torch.equal(t, torch.full_like(t, 7.0))
