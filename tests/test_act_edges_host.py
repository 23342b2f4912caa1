"""CPU checks of tests/act_edges_ref.py, which tests/test_gpu_55_act_edges.py holds the activation, blur-pool and norm-add kernels against:
that the float64 restatements are torch autograd of reflect pad + depthwise convolution + normalisation at given statistics, on non-square
planes down to 3 x 3; that the launch caps restated there are the launchers' text; that the case tables name every route the route function
can return, stay under 64 MB a case and keep every normalised element away from the activation's knife edge; and that the comparison the
GPU test uses rejects each of a list of one-line mutants of the restatement at one table entry or more -- the shapes and bounds can fail."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import act_edges_ref as R
from tests import conv_exact as X

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tfc-gan_amd", "csrc")
PLANES = ((3, 3), (3, 7), (4, 5), (7, 4), (5, 9), (16, 33))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def torch_fwd(x, stats, slope, pool, keep, drop_p):
    """pad (reflect) + conv2d(groups = C) + normalisation at the given sums, all torch float64"""
    N, C, H, W = x.shape
    if stats is not None:
        s = T(stats).double()
        m = s[..., 0] / (H * W)
        var = (s[..., 1] / (H * W) - m * m).clamp_min(0.0)
        x = (x - m[:, :, None, None]) * torch.rsqrt(var + R.EPS)[:, :, None, None]
    a = torch.where(x > 0, x, x * slope)
    if pool:
        k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64) / 8.0
        a = F.conv2d(F.pad(a, (1, 2, 1, 2), mode="reflect"), torch.outer(k, k)[None, None].repeat(C, 1, 1, 1), stride=pool, groups=C)
    if keep is not None:
        a = a * T(keep) / (1.0 - drop_p)
    return a


@pytest.mark.parametrize("H,W", PLANES)
def test_blur_matrices_are_conv_exact(H, W):
    """blur_fwd / blur_bwd equal conv_exact.blur / blur_t (reflect pad (1, 2), taps / 8, stride 1 and 2) on non-square planes, exactly: integer
    data, dyadic taps"""
    x = R.ternary((2, 3, H, W), 5)
    for pool in (1, 2):
        y = R.blur_fwd(x, pool)
        assert y.shape[2:] == (R.out_len(H, pool), R.out_len(W, pool))
        assert np.array_equal(y, X.blur(T(x), pool).numpy())
        g = R.ternary(y.shape, 6)
        assert np.array_equal(R.blur_bwd(g, H, W, pool), X.blur_t(T(g), x.shape, pool).numpy())


@pytest.mark.parametrize("H,W", PLANES)
@pytest.mark.parametrize("pool,slope,drop", [(2, 0.2, 0.0), (2, 0.25, 0.5), (1, 0.2, 0.0), (0, 0.0, 0.5), (1, 1.0, 0.0)])
@pytest.mark.parametrize("norm", [False, True])
def test_restatements_are_autograd(H, W, pool, slope, drop, norm):
    """forward, mode 0 (with its bias sums), modes 1 and 2 (chained: mode 2 reads mode 1's sums unrounded) and norm-add against autograd"""
    N, C = 2, 3
    x = R.knife_free((N, C, H, W), 3, R.FP32, zero_plane=False)
    stats = None
    if norm:
        stats = np.stack((x.sum((2, 3)), (x * x).sum((2, 3))), -1)          # float64 here: the derivation, not the rounding, is under test
    Ho, Wo = R.out_len(H, pool), R.out_len(W, pool)
    keep = R.keep_mask(9, N, Ho, Wo, C, drop) if drop else None
    xt = T(x).requires_grad_(True)
    y = torch_fwd(xt, stats, slope, pool, keep, drop)
    got = R.act_fwd_ref(x, stats, slope, pool, keep, drop)
    assert got.shape == tuple(y.shape)
    assert np.abs(got - y.detach().numpy()).max() <= 1e-13 * max(1.0, np.abs(got).max())
    dy = R.gauss(got.shape, 4, R.FP32)
    if norm:
        # autograd through the statistics too: the sums are functions of x in nn.InstanceNorm2d, which is what modes 1 + 2 restate
        xn = T(x).requires_grad_(True)
        mu = xn.mean((2, 3), keepdim=True)
        var = (xn * xn).mean((2, 3), keepdim=True) - mu * mu
        xh = (xn - mu) * torch.rsqrt(var + R.EPS)
        a = torch.where(xh > 0, xh, xh * slope)
        yy = X.blur(a, pool) if pool else a
        if keep is not None:
            yy = yy * T(keep) / (1.0 - drop)
        (gx,) = torch.autograd.grad(yy, xn, T(dy))
        rs = R.act_bwd_ref(1, dy, x, stats, slope, pool, (H, W), keep, drop)
        dx = R.act_bwd_ref(2, dy, x, stats, slope, pool, (H, W), keep, drop, rstats=rs)
        assert np.abs(dx - gx.numpy()).max() <= 1e-10 * max(1.0, np.abs(dx).max())
        res = R.gauss(x.shape, 8, R.FP32)
        assert np.abs(R.norm_add_ref(x, res, stats) - (T(res) + xh).detach().numpy()).max() <= 1e-12
    else:
        (gx,) = torch.autograd.grad(y, xt, T(dy))
        dx, bias = R.act_bwd_ref(0, dy, x, None, slope, pool, (H, W), keep, drop)
        assert np.abs(dx - gx.numpy()).max() <= 1e-13 * max(1.0, np.abs(dx).max())
        assert np.abs(bias - gx.sum((2, 3)).numpy()).max() <= 1e-12 * H * W
        if slope == 1.0:                                           # the pure blur's transpose needs no x
            dx0, _ = R.act_bwd_ref(0, dy, None, None, slope, pool, (H, W), keep, drop)
            assert np.array_equal(dx0, dx)


def test_mode1_sums_are_the_gradient_moments():
    """mode 1 = (sum g', sum g' xhat) with g' the gradient at xhat, and act'(0) = slope (the kernels' convention) on an all-zero plane"""
    N, C, H, W = 2, 2, 4, 5
    x = R.knife_free((N, C, H, W), 1, R.FP32)
    assert not x[0, 0].any()
    stats = R.stats_of(x)
    dy = R.gauss((N, C, H, W), 2, R.FP32)
    rs = R.act_bwd_ref(1, dy, x, stats, 0.2, 0, (H, W))
    xh, _ = R.xhat_of(x, stats, R.F64)
    g = dy * np.where(xh > 0, 1.0, 0.2)
    assert not xh[0, 0].any() and np.allclose(rs[0, 0, 0], 0.2 * dy[0, 0].sum(), rtol=1e-12) and rs[0, 0, 1] == 0.0
    assert np.allclose(rs[..., 0], g.sum((2, 3)), rtol=1e-12, atol=1e-12) and np.allclose(rs[..., 1], (g * xh).sum((2, 3)), rtol=1e-12, atol=1e-12)


def test_caps_are_the_launchers():
    """ACT_CAP, the reference batch, the partial-sum scratch and the launchers' conditions are the text of the sources route() restates"""
    with open(os.path.join(CSRC, "elementwise.hip")) as f:
        ew = f.read()
    with open(os.path.join(CSRC, "tfc_desc.h")) as f:
        desc = f.read()
    with open(os.path.join(CSRC, "api.hip")) as f:
        api = f.read()
    assert re.search(r"#define TFC_ACT_CAP (\d+)", ew).group(1) == str(R.ACT_CAP)
    assert re.search(r"#define TFC_REF_BATCH (\d+)", desc).group(1) == str(R.REF_BATCH)
    assert "#define TFC_PART_WS_FLOATS (8 << 20)" in desc and R.PART_WS_FLOATS == 8 << 20
    for text in ("if (inv) N = TFC_REF_BATCH;", "const int cap = TFC_ACT_CAP / (N > 0 ? N : 1);", "const int ppb = 256 / cv;", "if (nb > cap) nb = cap;",
                 "if (p.pool == 2 && !stats_out) {", "act_grid(((p.Ho + 1) / 2) * ((p.Wo + 1) / 2), p.C",
                 "if (p.pool == 1 && !p.norm && p.slope == 1.f && !p.drop_thresh24 &&", "if (p.C % (8 * UE) != 0 || p.H < 4 || p.W < 4) return false;",
                 "const int tiles_x = (p.W + 31) / 32, tiles_y = (p.H + 7) / 8;", "if (p.pool == 2 && use_x) {", "const int cslice = p.C < 64 ? p.C : 64;",
                 "const int tiles_x = (p.W + 31) / 32, tiles_y = (p.H + 15) / 16;", "if (p.pool == 1 && mode == 0 && !use_x && !rstats && !p.drop_thresh24 &&",
                 "const dim3 grid = act_grid(p.H * p.W, p.C, dt == TFC_DT_BF16 ? 8 : 4, p.N);"):
        assert text in ew, text
    for text in ("p.Ho = pool == 2 ? (H - 1) / 2 + 1 : H;", "REQUIRE(cv <= 256 && (256 % cv) == 0", "p.eps = 1e-5f;"):
        assert text in api, text
    assert R.act_grid_cap(2, False) == 2048 and R.act_grid_cap(64, False) == 64 and R.act_grid_cap(2, True) == 128 and R.act_grid_cap(8192, False) == 1
    assert R.legal_widths(R.BF16) == (8, 16, 32, 64, 128, 256, 512, 1024, 2048) and R.legal_widths(R.FP32)[-1] == 1024


@pytest.fixture(scope="module")
def cases():
    return R.all_cases()


def test_tables_name_every_route(cases):
    """every route route() can return is named by a table entry, in both dtypes where the route exists in both; every geometry of the issue's
    sweep is there at the cheap width; the cap cases are capped, multi-trip and ragged by route()'s own account; every case is under 64 MB"""
    for dtype in R.DTYPES:
        named = {c.kernel for c in cases if c.dtype == dtype}
        want = set(R.ROUTES) - ({"pool2_bwd<signs>"} if dtype == R.FP32 else set())
        assert named == want, (dtype, sorted(want ^ named))
    assert all(c.kernel == R.route_of(c).kernel for c in cases)
    assert max(R.case_bytes(c) for c in cases) < 64 << 20
    geo = {(c.H, c.W) for c in cases if c.why.startswith("geometry") and c.C == R.cheap_c(c.dtype)}
    assert geo == {(h, w) for h in list(range(3, 21)) + [31, 32, 33] for w in (3, 4, 5, 6, 7, 8, 31, 32, 33, 34, 35, 63, 64, 65)}
    tiled = {(c.H, c.W) for c in cases if c.why.startswith("geometry") and c.C == R.tiled_c(c.dtype)}
    assert {(h, w) for h in (3, 4, 5) for w in (3, 4, 5)} <= tiled
    for edge in (7, 8, 9, 15, 16, 17, 31, 32, 33):
        assert any(h == edge for h, _ in tiled) and any(w == edge for _, w in tiled), edge
    # section 3: tiled pool-2 backward below its 64-channel slice and beyond one slice, the generic kernels at one pixel per workgroup, and the
    # partial-sum reduction at L = 2 C = 4096
    r = R.route("bwd", R.FP32, 2, 17, 33, 4, pool=2)
    assert r.kernel == "pool2_bwd<0>" and r.grid == (4, 2, 1)
    assert R.route("bwd", R.BF16, 2, 17, 33, 128, pool=2).grid[2] == 2
    assert R.act_grid(35, 2048, R.BF16, 2, False)[0] == 35 and any(c.C == 2048 and c.stats_out for c in cases)
    assert not any(c.kernel == R.REFUSED for c in cases) and R.route("fwd", R.BF16, 64, 5, 13, 2048, stats_out=True).kernel == R.REFUSED
    assert R.route("fwd", R.FP32, 64, 5, 13, 1024, stats_out=True).kernel == "act_fwd<stats>"      # 64 x 64 x 2048 floats: exactly the scratch
    caps = [c for c in cases if c.why == "grid cap"]
    for kernel in ("act_fwd<stats>", "act_fwd", "pool2_fwd<act>", "act_bwd<0,0>", "act_bwd<1,0>", "norm_add"):
        for dtype in R.DTYPES:
            mine = [c for c in caps if c.kernel == kernel and c.dtype == dtype]
            assert {(c.inv, c.N) for c in mine} >= {(True, 1), (True, 2)} and (kernel == "pool2_fwd<act>" or any(not c.inv for c in mine)), kernel
            for c in mine:
                r = R.route_of(c)
                assert r.grid[0] == R.act_grid_cap(c.N, c.inv) and r.trips > 1 and r.ragged, c


def test_normalised_cases_are_knife_free(cases):
    """|xhat| >= 0.1 on every element of every normalised case but the all-zero plane (where it is exactly 0, in any precision): nothing is
    masked, so there is no share of cases to cap"""
    seen = set()
    for c in cases:
        key = (c.dtype, c.N, c.C, c.H, c.W)
        if not c.norm or key in seen:
            continue
        seen.add(key)
        d = R.case_inputs(c._replace(entry="nadd", mode=0, drop=0.0, pool=0))
        for wd in (R.F64, R.F32):
            xh, _ = R.xhat_of(d["x"], d["stats"], wd)
            assert not xh[0, 0].any(), key
            xh[0, 0] = 1.0
            assert np.abs(xh).min() >= 0.1, (key, float(np.abs(xh).min()))
    assert len(seen) >= 2 * 3 * 4


def test_exact_cases_are_exact(cases):
    """the exact tier's references are multiples of their quantum below 2^24 quanta, statistics of squares included (checked on the CPU for the
    pitch / width shapes and the largest plane of the sweep; the GPU test asserts it again for every case it runs)"""
    n = 0
    for c in cases:
        if R.is_exact(c) and c.dtype == R.BF16 and ((c.H, c.W) in ((17, 33), (33, 65)) and c.C <= 64):
            R.exact_want(c, R.case_reference(c, R.case_inputs(c)))
            n += 1
    assert n > 50


# which table entries to try per mutant: a filter on the case (the first few that match are tried until one rejects)
MUTANT_CASES = {
    "no_alias_n2": lambda c: c.pool and (c.H, c.W) in ((4, 5), (5, 7)),
    "no_alias_n3": lambda c: c.pool and (c.H, c.W) in ((4, 5), (5, 7)),
    "no_alias_m1": lambda c: c.pool and (c.H, c.W) in ((4, 5), (5, 7)),
    "swap_taps_last_row": lambda c: c.pool and (c.H, c.W) in ((4, 5), (5, 7)),
    "ho_half": lambda c: c.pool == 2 and (c.H, c.W) == (5, 7),
    "drop_npix_in": lambda c: c.pool == 2 and c.drop and c.C <= 64,
    "drop_no_slice_offset": lambda c: c.drop and c.C == 128,
    "slot_left_out": lambda c: (c.stats_out or c.rstats) and R.is_exact(c) and (c.H, c.W) == (5, 7),
    "swap_s1_s2": lambda c: c.mode == 1 and (c.H, c.W) == (4, 5),
    "act0_is_1": lambda c: c.entry == "bwd" and c.use_x and R.is_exact(c) and c.slope != 1.0 and (c.H, c.W) == (5, 7),
    "mg_is_sum": lambda c: c.mode == 2 and (c.H, c.W) == (4, 5),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_comparison_rejects_mutant(mutant, cases):
    """R.rejects() compares with the function and the bound of the GPU test; the unmutated restatement passes the same comparison"""
    tried = [c for c in cases if MUTANT_CASES[mutant](c)][:40]
    assert tried
    hit = None
    for c in tried:
        d = R.case_inputs(c)
        if R.rejects(c, d, mutant):
            hit = c
            break
    assert hit is not None, f"{mutant}: passed at all {len(tried)} entries tried"
    assert not R.rejects(hit, R.case_inputs(hit), None)
    if mutant in ("no_alias_n2", "no_alias_n3", "no_alias_m1", "swap_taps_last_row", "ho_half"):
        # the geometry mutants fall at forward AND backward entries, of both pools where the alias exists
        for entry in ("fwd", "bwd"):
            assert any(R.rejects(c, R.case_inputs(c), mutant) for c in tried if c.entry == entry), (mutant, entry)
