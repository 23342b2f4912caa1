"""CPU checks of tests/stream_edges_ref.py, the restatements and input builders that tests/test_gpu_51_stream_edges.py holds the streaming kernels
against, and of the conditions those GPU tests rely on: that every size list straddles the cap its launcher states, that the integer data stays
exact (below 2^24), that torch's own bf16 conversion is the round-to-nearest-even of the bit model on every special value, that the closed forms
are the autograd of the losses, and that plain fp32 arithmetic meets the bounds the kernels are held to (with room: a bound that fp32 itself
misses would say nothing about a kernel)."""
import re
import os

import numpy as np
import pytest
import torch

from oracle import tfcgan_oracle as O
from tests import stream_edges_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tfc-gan_amd", "csrc")


def _launcher(name, path="elementwise.hip"):
    with open(os.path.join(CSRC, path)) as f:
        text = f.read()
    m = re.search(r"hipError_t " + name + r"\(.*?\n}\n", text, re.S)
    assert m, name
    return m.group(0)


def test_caps_are_the_launchers():
    """the caps of stream_edges_ref are the numbers in the launchers' text, and each size list has a case just on either side"""
    for name in ("tfc_launch_adam", "tfc_launch_axpby", "tfc_launch_dropout_mask", "tfc_launch_cast"):
        assert "if (nb > 4096) nb = 4096;" in _launcher(name), name
    assert "if (nb > 512) nb = 512;" in _launcher("tfc_launch_l1_sum", "losses.hip")
    assert "if (nb > 256) nb = 256;" in _launcher("tfc_launch_bce_rel")
    assert "if (nbk > 1024) nbk = 1024;" in _launcher("tfc_launch_tanh_bwd_pack")
    sn = _launcher("tfc_launch_sn_bwd")
    assert "(n + 1023) / 1024" in sn and "if (nb > TFC_SN_BWD_PARTS) nb = TFC_SN_BWD_PARTS;" in sn
    with open(os.path.join(CSRC, "tfc_desc.h")) as f:
        assert re.search(r"#define\s+TFC_SN_BWD_PARTS\s+128\b", f.read())
    head = _launcher("tfc_launch_head_fwd")
    assert "(npix + 3) / 4" in head and "(C / ue <= 64) ? 0" in head
    with open(os.path.join(CSRC, "elementwise.hip")) as f:
        assert re.search(r"#define\s+TFC_HEAD_NB\s+512\b", f.read())
    cs = _launcher("tfc_launch_colsum")
    assert "rows >= 4096" in cs and "(rows + 1023) / 1024" in cs and "2048 / nbx" in cs
    for sizes, cap in ((R.FLAT_SIZES, R.FLAT_CAP), (R.L1_SIZES, R.L1_CAP), (R.BCE_SIZES, R.BCE_CAP)):
        assert cap in sizes and cap + 1 in sizes and min(sizes) == 1 and max(sizes) > 2 * cap and max(sizes) % 256 != 0
    assert R.flat_grid(R.FLAT_SIZES[-1]) == (4096, 3) and R.flat_grid(R.FLAT_CAP) == (4096, 1) and R.flat_grid(R.FLAT_CAP + 1) == (4096, 2)
    pix = [n * h * w for n, h, w in R.TANH_SHAPES]
    assert pix[-1] == 262656 > R.TANH_CAP and all(p < R.TANH_CAP for p in pix[:-1])
    elems = [r * k for r, k in R.SN_SHAPES]
    assert R.SN_PARTS * R.SN_PER_PART in elems and sum(e > R.SN_PARTS * R.SN_PER_PART for e in elems) == 2
    assert (130 * 1031) % 4 != 0 and (64 * 8193) % 4 == 0                                   # the scalar loop past the cap, and the float4 loop
    hp = [n * h * w for n, h, w in R.HEAD_SHAPES]
    assert hp[-1] == 2187 > R.HEAD_CAP_PIXELS and hp[1] % 4 != 0


def test_colsum_routes_and_exactness():
    """ny of the row-split route is 4, 5, 6, 9 (below, at and above the reducer's 8 lanes) for every C of the test; without part_ws, or below
    4096 rows, it is 1; C / ue = 3 and 9 leave idle lanes in the last workgroup of 8 vectors; the sums stay far below 2^24"""
    part = 8388608
    for dtype, Cs in R.COLSUM_C.items():
        ue = R.ue_of(dtype)
        assert sorted(c // ue for c in Cs)[:3] == [1, 3, 9] and all(c % ue == 0 for c in Cs)
        for C in Cs:
            assert [R.colsum_ny(r, C, dtype, part) for r in R.COLSUM_ROWS_SPLIT] == [4, 5, 6, 9]
            assert all(R.colsum_ny(r, C, dtype, part) == 1 for r in R.COLSUM_ROWS_ONE)
            assert R.colsum_ny(8225, C, dtype, part, with_part=False) == 1
    data = R.ternary((64, 24), 3)
    buf, coff, pitch = R.colsum_buffer(data, 33, 24, torch.bfloat16, wide=True)
    assert (coff, pitch) == (8, 40) and torch.equal(buf[:, 8:32].double(), data[:33]) and (buf[:, :8] == R.COLSUM_SENTINEL).all()
    assert (buf[:, 32:] == R.COLSUM_SENTINEL).all() and R.COLSUM_SENTINEL > max(R.COLSUM_ROWS_SPLIT) + 20
    assert colsum_max() < 2 ** 24 and (R.colsum_prefill(512) != 0).all()


def colsum_max():
    return max(R.COLSUM_ROWS_SPLIT) + float(R.colsum_prefill(512).abs().max())


def test_cast_reference_is_round_to_nearest_even():
    """x.to(torch.bfloat16), the reference of the cast test, is RNE on the bits for every special (ties both ways, signed zeros, infinities, the
    NaN, overflow to inf, denormals) and on random data; widening is exact on all 65 536 bf16 patterns"""
    x = R.cast_f32_data(5000)
    s = R.bits_f32(R.CAST_SPECIALS)
    assert torch.equal(R.bits32(x[:len(s)]), R.bits32(s)) and torch.equal(R.bits32(x[-len(s):]), R.bits32(s))
    model = R.bf16_rne_bits(x).to(torch.int16).view(torch.bfloat16)
    assert torch.isnan(x).sum() == 2 and R.same_floats(x.to(torch.bfloat16), model) and not R.same_floats(-model, model)
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0xBF808000: 0xBF80, 0xBF818000: 0xBF82, 0x80000000: 0x8000, 0x7F7FFFFF: 0x7F80,
            0xFF7FFFFF: 0xFF80, 0x7FC00000: 0x7FC0, 0x00000001: 0x0000, 0x00008000: 0x0000, 0x00018000: 0x0002, 0x007FFFFF: 0x0080,
            0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81}
    got = dict(zip(R.CAST_SPECIALS, R.bf16_rne_bits(s).tolist()))
    assert {k: got[k] for k in want} == want
    assert R.bits_f32([0x7F7FFFFF]).item() == np.finfo(np.float32).max and torch.isnan(R.bits_f32([0x7FC00000])).all()
    b = R.cast_bf16_data(70000)
    assert len(set(R.bits16(b).tolist())) == 65536
    assert torch.equal(R.bits32(b.float()), R.bits16(b) << 16) and torch.isnan(b).any()
    assert R.cast_f32_data(1).item() == R.bits_f32(R.CAST_SPECIALS[:1]).item()


def test_axpby_bound_holds_for_both_fp32_evaluations():
    """2^-23 (|a x| + |b y|) covers the unfused fp32 evaluation (two products, one sum) and the contracted one (one product, one fma); with
    power-of-two coefficients on integer data both are exact"""
    n = 200001
    for a, b in R.AXPBY_AB:
        x, y = R.axpby_data(n)
        a32, b32 = np.float32(a), np.float32(b)
        for yy in (y, None):
            ref, bound = R.axpby_ref(x, yy, a, b)
            plain = a32 * x.numpy() + (b32 * yy.numpy() if yy is not None else np.float32(0))
            fused = (float(a32) * x.double().numpy() + (b32 * yy.numpy()).astype(np.float64)).astype(np.float32) if yy is not None else plain
            for ev in (plain, fused):
                assert ev.dtype == np.float32 and (np.abs(ev.astype(np.float64) - ref.numpy()) <= bound.numpy()).all()
    for a, b in R.AXPBY_AB_EXACT:
        x, y = R.axpby_data(n, exact=True)
        ref, _ = R.axpby_ref(x, y, a, b)
        assert torch.equal((a * x + b * y).double(), ref) and torch.equal(ref, ref.round()) and ref.abs().max() < 2 ** 24


def test_keep_mask_edges():
    """O.hip_keep_mask, the reference of the dropout-mask test: p = 0 keeps everything; the thresholds of the four p are 0, 1, 2^23, 2^24 - 1 in
    float32 as in float64 (the entry point gets a float and uses lrintf); a mask of n is a prefix of a longer one (the index is the only input);
    a seed >= 2^31 is taken modulo 2^32; the vector form equals a scalar restatement of tfc_hash32"""
    for p, t in zip(R.DROP_P, (0, 1, 1 << 23, (1 << 24) - 1)):
        assert float(np.float32(p)) == p and int(np.rint(np.float32(p) * np.float32(16777216.0))) == t == int(round(p * 16777216.0))
    assert max(R.DROP_SEEDS) >= 2 ** 31
    n = 300000
    for seed in R.DROP_SEEDS:
        assert O.hip_keep_mask(seed, n, 0.0).all()
        rates = [O.hip_keep_mask(seed, n, p).mean() for p in R.DROP_P]
        assert rates[0] == 1.0 and rates[1] > 0.9999 and 0.49 < rates[2] < 0.51 and rates[3] < 1e-4
        assert np.array_equal(O.hip_keep_mask(seed, n, 0.5)[:777], O.hip_keep_mask(seed, 777, 0.5))
        assert np.array_equal(O.hip_keep_mask(seed, 64, 0.5), O.hip_keep_mask(seed + 2 ** 32, 64, 0.5))

        def h(i, s=seed):
            M = 0xFFFFFFFF
            x = (i * 0x9E3779B1 + s) & M
            x ^= x >> 16; x = (x * 0x85EBCA6B) & M; x ^= x >> 13; x = (x * 0xC2B2AE35) & M; x ^= x >> 16
            x = (x + s * 0x27D4EB2F) & M; x ^= x >> 15; x = (x * 0x2C1B3C6D) & M; x ^= x >> 12
            return x
        idx = [0, 1, 255, 256, R.FLAT_CAP - 1, R.FLAT_CAP, 2 * R.FLAT_CAP + 2]
        full = O.hip_keep_mask(seed, R.FLAT_SIZES[-1], 0.5)
        assert [bool(full[i]) for i in idx] == [(h(i) >> 8) >= (1 << 23) for i in idx]


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("gscale", R.ADAM_GSCALES)
def test_adam_fp32_restatement_meets_the_bounds(step, gscale):
    """On the whole draw (2 x 4096 x 256 + 3 elements): a plain fp32 numpy Adam step meets the m and v bounds 2^-22 (|b x| + |(1 - b) y|), and c, 8 x
    its largest relative error in the update (fp32 powf-style bias corrections included), is below 1e-4; with c the fp32 step meets the p
    bound 2^-24 |p| + c |delta| as well. 1 - b is exact in fp32 for both betas, so the fp64 reference and the kernel use the same weights."""
    hp = R.ADAM_HP
    for b in (hp["b1"], hp["b2"]):
        b32 = np.float32(b)
        assert float(np.float32(1) - b32) == 1.0 - float(b32)
    n = R.FLAT_SIZES[-1]
    st = R.adam_state(n)
    ref, f32 = R.adam_ref(*st, step, gscale, **hp), R.adam_f32(*st, step, gscale, **hp)
    c = R.adam_c(ref, f32)
    print(f"step {step} gscale {gscale}: c = {c:.3e}; fp32 m / v errors in units of their bounds: "
          f"{np.max(np.abs(f32['m'] - ref['m']) / np.maximum(ref['m_bound'], 1e-300)):.3f} / "
          f"{np.max(np.abs(f32['v'] - ref['v']) / np.maximum(ref['v_bound'], 1e-300)):.3f}")
    assert c < 1e-4
    assert (np.abs(f32["m"] - ref["m"]) <= ref["m_bound"]).all() and (np.abs(f32["v"] - ref["v"]) <= ref["v_bound"]).all()
    assert (np.abs(f32["p"] - ref["p"]) <= R.adam_p_bound(ref, c)).all()


def test_adam_state_blocks_and_trips():
    """the state of n is the first n of one draw plus its two zero blocks (denominator = eps in the second); the blocks stay inside the first trip
    of the large sizes, and there every element of the second and third trip is moved by far more than the bounds (so `differs from its input`
    is a statement about the loop, not about luck): p, m and v each change in more than 99.9 % of those elements and in all of the last three"""
    hp = R.ADAM_HP
    p, m, v, g = R.adam_state(255)
    g0, v0 = R.adam_blocks(255)
    assert g0.stop - g0.start == 15 and (g[g0] == 0).all() and (v[g0] != 0).all() and (v[v0] == 0).all() and (g[v0] == 0).all()
    ref = R.adam_ref(p, m, v, g, 1, 1.0, **hp)
    assert np.allclose(ref["delta"][v0], float(np.float32(hp["lr"])) / 0.5 * (0.5 * m[v0].astype(np.float64)) / float(np.float32(hp["eps"])), rtol=1e-12)
    assert R.adam_state(1)[3].shape == (1,) and R.adam_state(1)[3][0] != 0
    big = R.adam_state(R.FLAT_SIZES[-1])
    assert all(np.array_equal(a[:255][~_in(255, g0, v0)], b[~_in(255, g0, v0)]) for a, b in zip(big, (p, m, v, g)))
    for n in R.FLAT_SIZES[-2:]:
        g0, v0 = R.adam_blocks(n)
        assert v0.stop <= R.FLAT_CAP
        st = R.adam_state(n)
        ref = R.adam_ref(*st, 1000, 0.5, **hp)
        for name, old in (("p", st[0]), ("m", st[1]), ("v", st[2])):
            moved = np.abs(ref[name][R.FLAT_CAP:] - old[R.FLAT_CAP:]) > 4 * R.EPS24 * np.abs(old[R.FLAT_CAP:])
            assert moved.mean() > 0.999 and (n < 2 * R.FLAT_CAP or moved[-3:].all()), (n, name, moved.mean())


def _in(n, *slices):
    mask = np.zeros(n, dtype=bool)
    for s in slices:
        mask[s] = True
    return mask


def test_integer_cases_are_exact():
    """tanh backward: g (1 - y^2) is an integer in -8..8 and the largest bias sum stays below 2^24; L1: 2 n x scale stays below 2^24 for both
    scales of the GPU test, with the pre-set value added"""
    g, y, want = R.tanh_case(2, 4, 16, 24, 5)
    assert torch.equal(want, want.round()) and want.abs().max() == 8 and set(y.unique().tolist()) == {-0.5, 0.0, 0.5}
    assert torch.equal((g * (1 - y * y)).double(), want)
    assert 8 * max(n * h * w for n, h, w in R.TANH_SHAPES) < 2 ** 24
    a, b, tot = R.l1_case(1000)
    assert tot == (a - b).abs().sum().item() and 2 * R.L1_SIZES[-1] * 4 + 1000 < 2 ** 24
    x, w, want = R.head_case(1, 3, 5, 64, 9)
    assert want.shape == (1, 1, 3, 5) and torch.equal(want, want.round()) and 16 * 1024 < 2 ** 24


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bce_reference_is_the_autograd_of_the_losses(dtype):
    """bce_ref's closed-form gradient and loss are the oracle's relativistic losses under fp64 autograd (label 0.9 as the float the entry point
    gets); the logits cover [-30, 30], an exact 0 and +-90 inside the first 257, where expf(-|x|) = 8.2e-40 lies below the smallest normal float (a flush to zero or a denormal: log1pf and the sigmoid must not care) and the reference stays finite"""
    a, b = R.bce_logits(dtype)
    x = a.double() - b.double()
    assert x.min() == -90 and x.max() == 90 and (x[:257] == 0).any() and (x[:257] == 90).any() and (x[:257] == -90).any()
    inner = x[x.abs() < 80]
    assert inner.min() < -29 and inner.max() > 29 and 0 < np.exp(np.float32(-90.0)) < np.finfo(np.float32).tiny
    t1 = float(np.float32(R.BCE_T1))
    for n in (257, R.BCE_SIZES[-1]):
        ad, bd = a[:n].double().requires_grad_(True), b[:n].double().requires_grad_(True)
        for mode, loss in ((0, O.loss_gan_generator(ad, bd, valid=t1)), (1, O.loss_discriminator(ad, bd, valid=t1))):
            ga, gb = torch.autograd.grad(loss, (ad, bd), allow_unused=True)
            ref = R.bce_ref(a, b, n, mode, 0.25)
            assert abs(ref["loss"] - loss.item()) <= 1e-13 * abs(loss.item())
            assert torch.allclose(ref["da"], 0.25 * ga, rtol=1e-12, atol=1e-20)
            if mode == 1:
                assert torch.allclose(-ref["da"], 0.25 * gb, rtol=1e-12, atol=1e-20)
            assert np.isfinite(ref["loss"]) and 0 < ref["grad_err"] < 1e-6 / n and 0 < ref["loss_err"] < 1e-5


def test_spectral_norm_backward_closed_form():
    """the expression tfc_sn_bwd_apply_kernel evaluates is the fp64 autograd of ((W / (u W v)) G).sum(); at R = K = 1 the gradient is zero and the
    dyadic case evaluates to exactly 0 in fp32 as in fp64"""
    for i, (Rr, K) in enumerate(R.SN_SHAPES[:4]):
        W, G, u, v = R.sn_case(Rr, K, 50 + i)
        assert abs(u.norm().item() - 1) < 1e-6 and abs(v.norm().item() - 1) < 1e-6
        want = R.sn_grad(W, G, u, v, torch.float64)
        assert (R.sn_closed_form(W, G, u, v) - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
    W, G, u, v = R.sn_case(1, 1, 0)
    assert torch.equal(R.sn_grad(W, G, u, v, torch.float64), torch.zeros(1, 1, dtype=torch.float64))
    assert torch.equal(R.sn_grad(W, G, u, v, torch.float32), torch.zeros(1, 1))


def test_head_weight_paths():
    """which tests reach which weight path of tfc_head_fwd_kernel (filter in LDS when C / ue > 64): test_patchgan_head_kernel_matches_padconv runs
    C = 512 in both dtypes and test_exact_patchgan_head_fwd C = 512 in bf16, i.e. LDS in fp32 only and registers in bf16 only. HEAD_CASES adds the
    other two: registers in fp32 (C = 64) and LDS in bf16 (C = 1024)"""
    assert R.head_uses_lds(torch.float32, 512) and not R.head_uses_lds(torch.bfloat16, 512)
    assert [R.head_uses_lds(dt, C) for dt, C in R.HEAD_CASES] == [False, True, False, False, True]
    assert 16 * 1024 * 4 <= 65536                                  # the bf16 LDS case fits the 64 KiB a launch gets without an attribute
