"""CPU checks of tests/stn21_edges_ref.py, the restatements the STN21 edge tests (tests/test_gpu_42_stn21_edges.py) hold the kernels against:
the attention restatement against torch's fp64 autograd, the separation of the bf16 rounding model from every single omitted rounding, the
two-pass LayerNorm against the one-pass form at a large offset, the tie rule of the morphological gradient against the torch restatement, and the
hinge margins of the row-triplet data."""
import pytest
import torch
import torch.nn.functional as F

from tests import stn21_edges_ref as R
from tests.test_gpu_30_stn import ref_morph_gradient

N, H, SCALE = 2, 3, 0.125


@pytest.mark.parametrize("T", [1, 2, 3, 17, 43, 64])
def test_attention_restatement_matches_autograd_fp64(T):
    """the hand-written backward of attention_model with no rounding is torch's autograd, to 1e-12, and the dqkv packing is the qkv layout"""
    qkv, do = R.attention_inputs(N, T, H, seed=T)
    got, want = R.attention_model(qkv, do, N, T, H, SCALE), R.attention_autograd(qkv, do, N, T, H, SCALE)
    for g, w, name in zip(got, want, ("out", "probs", "dqkv")):
        if T == 1 and name == "dqkv":                              # dq = dk = 0 exactly: compare dv, and the zeros as zeros
            g3, w3 = g.reshape(N, 3, H * 64), w.reshape(N, 3, H * 64)
            assert torch.equal(g3[:, :2], torch.zeros_like(g3[:, :2])) and w3[:, :2].abs().max().item() <= 1e-15
            g, w = g3[:, 2], w3[:, 2]
        assert R.rel_l2(g, w) <= 1e-12, (T, name, R.rel_l2(g, w))


@pytest.mark.parametrize("T", [2, 17, 43, 64])
def test_attention_rounding_model_separates_single_omissions(T):
    """The bf16 bar of the GPU test (rel-L2 2e-4 on the output and on dqkv against the fp64 restatement with all six roundings) stands between two
    facts, both reproduced here on the GPU test's data (seed 0, N(0, 1)):
    (a) an fp32 emulation with the same roundings stays within 2e-5 of the restatement, once its bf16 tie flips of dS are set aside: where fp32
        and fp64 round dS[i][j] to different bf16 neighbours the element moves by one bf16 ulp, and ONE flip of a typical element among the
        2 * 3 * 64 * 64 of T = 64 is already 1.5e-5 of dqkv (measured: 3 flips, 3.5e-5 at T = 64; 2.7e-5 at T = 43; none at T = 2, 17). The flips
        are counted (at most one element in a thousand), their exact contribution delta k / deltat q is taken out, and what remains meets
        2e-5; with the flips left in, the emulation is still under a quarter of the bar (5e-5);
    (b) leaving out any single rounding (q, k, v, dO, P, dS) moves the output or dqkv by more than 5e-4 (measured: 1.25e-3 at the least)."""
    qkv, do = R.attention_inputs(N, T, H, seed=0)
    p64, p32 = {}, {}
    full = R.attention_model(qkv, do, N, T, H, SCALE, rounding=R.ROUNDINGS, parts=p64)
    emu = R.attention_model(qkv, do, N, T, H, SCALE, dtype=torch.float32, rounding=R.ROUNDINGS, parts=p32)
    delta = R.bf16r(p64["dS"]) - R.bf16r(p32["dS"]).double()       # exactly 0 wherever both round to the same bf16 value
    flips = int((delta != 0).sum())
    fixed = emu[2].double() + R.pack_dqkv(delta @ p64["k"], delta.transpose(-2, -1) @ p64["q"], torch.zeros_like(p64["q"]))
    e_out, e_raw, e_fix = R.rel_l2(emu[0], full[0]), R.rel_l2(emu[2], full[2]), R.rel_l2(fixed, full[2])
    print(f"T={T}: fp32 emulation vs restatement: out {e_out:.2e}, dqkv {e_raw:.2e} ({flips} dS tie flips of {delta.numel()}), without them {e_fix:.2e}")
    assert e_out <= 2e-5 and e_fix <= 2e-5 and e_raw <= 5e-5
    assert flips <= delta.numel() // 1000
    for name in R.ROUNDINGS:
        o = R.attention_model(qkv, do, N, T, H, SCALE, rounding=tuple(x for x in R.ROUNDINGS if x != name))
        moved = max(R.rel_l2(o[0], full[0]), R.rel_l2(o[2], full[2]))
        print(f"T={T}: without the rounding of {name}: {moved:.2e}")
        assert moved > 5e-4, (name, moved)


def test_layernorm_two_pass_meets_the_offset_bar_and_one_pass_does_not():
    """x = 1000 + N(0, 1), D = 1024: the GPU test's bar is 4x the error of torch's own fp32 F.layer_norm against fp64, + 1e-6 (fp32 itself limits
    the result: the mean is rounded to ulp(1000)). A two-pass fp32 model of the kernel meets it; the one-pass variance E[x^2] - mean^2 misses it
    a hundredfold."""
    torch.manual_seed(0)
    D = 1024
    x = 1000 + torch.randn(7, D)
    g, b = torch.randn(D), torch.randn(D)
    want = F.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-6)
    bar = 4 * R.rel_l2(F.layer_norm(x, (D,), g, b, 1e-6), want) + 1e-6
    two, one = R.rel_l2(R.layernorm_fp32(x, g, b, 1e-6), want), R.rel_l2(R.layernorm_fp32(x, g, b, 1e-6, two_pass=False), want)
    print(f"bar {bar:.2e}, two-pass {two:.2e}, one-pass {one:.2e}")
    assert two <= bar and one > 100 * bar


@pytest.mark.parametrize("shape,seed,pad_rows", R.MORPH_CASES)
def test_morph_tie_rule_scalar_model_agrees_with_torch_restatement(shape, seed, pad_rows):
    """On tied data the kernel's rule (first maximum / minimum in the order centre, up, down, left, right; the scalar model restates the kernel's
    loop) and ref_morph_gradient under torch's autograd agree exactly: max(dim) / min(dim) return the first index, and the restatement stacks in
    that order. A torch that changes the tie order of max fails here, on the CPU, before the GPU test is blamed."""
    x, go = R.morph_case(shape, seed, pad_rows)
    xr = x.clone().requires_grad_(True)
    want = ref_morph_gradient(xr)
    (gx,) = torch.autograd.grad(want, xr, go)
    Hh, Ww = shape[-2:]
    out, dx = R.morph_model(x.reshape(-1, Hh, Ww).numpy(), go.reshape(-1, Hh, Ww).numpy())
    assert torch.equal(torch.from_numpy(out).reshape(shape), want.detach())
    assert torch.equal(torch.from_numpy(dx).reshape(shape), gx)
    assert torch.equal(gx.sum((-2, -1)), torch.zeros(shape[:-2]))  # +g and -g per output pixel: every plane sums to 0 exactly
    if Hh * Ww > 1 and pad_rows:
        assert (want == 0).any()                                    # the data really has ties: whole plateaus


@pytest.mark.parametrize("W", R.TRIPLET_WIDTHS)
def test_triplet_rows_keep_their_hinge_margin(W):
    """the construction of triplet_rows: no row within 0.05 of the hinge's knife edge (0.3 for W >= 20, where exactly the even rows are active),
    active and inactive rows alternate, and every 97th row has p = a exactly"""
    a, p, n = R.triplet_rows(R.TRIPLET_ROWS, W, seed=W)
    _, ga, hinge = R.triplet_ref(a, p, n)
    assert hinge.abs().min().item() >= R.TRIPLET_MARGIN
    active = hinge > 0
    even = torch.arange(R.TRIPLET_ROWS) % 2 == 0
    assert active[even].all() and (~active[~even]).any()
    if W >= 20:
        assert torch.equal(active, even) and hinge.abs().min().item() >= 0.3
    assert torch.equal(p[::97], a[::97]) and not torch.equal(p[1::97], a[1::97])
    assert torch.equal(ga[~active], torch.zeros_like(ga[~active])) and torch.isfinite(ga).all()
