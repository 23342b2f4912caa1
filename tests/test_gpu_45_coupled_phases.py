"""GPU tests of the phase entry points behind batch_scope="global" (DESIGN.md 3.4): the edge mask's forward / backward and the batch-softmax KL loss
run in phases on SHARDS of one batch, in one process, with the records of the emulated ranks concatenated in rank order where the real path gathers
them (parallel.all_gather_records). What the merged phases compute must be what the unsplit entry points compute on the whole batch.

The mask inputs are built from tests/test_gpu_44_mask.py's case n3_19x37: x = img[0], y = img[1], batch [x, y, x, y]. Every extremum is then attained
exactly twice -- the minimum of |lap| in the copies of x, both maxima in the copies of y (asserted on the fp64 restatement) -- so split (2, 2) makes
"equal values add their counts" decide every merge, and split (1, 3), whose rank 0 holds only x, makes "the winner's count" decide the maxima.
Tolerances are those of test_gpu_44_mask.py: 8x the error the fp32-CPU restatement shows against fp64 on the same input.
"""
import functools

import pytest
import torch

import tfc_gan_amd as T
from tests import mask_ref as R
from tfc_gan_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REC = ops.MASK_RECORD_WORDS


def rel_l2(got, want):
    want = want.double()
    return ((got.double() - want).norm() / want.norm()).item()


def p(t):
    return None if t is None else t.data_ptr()


def last_error():
    return ops.lib().tfc_last_error().decode("utf-8", "replace")


def ok(rc, what):
    assert rc == 0, (what, last_error())


# ---- the emulated ranks ---------------------------------------------------------------------------------------------------------------------------
class Rank:
    """one shard's buffers, as ops.mask_fwd / ops.mask_bwd allocate them"""

    def __init__(self, img):
        self.img = img.to(DEV).contiguous()
        self.N, _, self.H, self.W = img.shape
        self.lap = torch.empty((self.N, 1, self.H, self.W), device=DEV)
        self.bl = torch.empty_like(self.lap)
        self.ws = torch.zeros(ops.lib().tfc_mask_ws_bytes(self.N, self.H, self.W) // 4, device=DEV)
        self.dims = (self.N, self.H, self.W)


def merge(ranks, recs, which):
    allrec = torch.stack(recs)                                     # rank order, as the all-gather leaves them
    for r in ranks:
        ok(ops.lib().tfc_mask_merge(ops.stream_ptr(), p(r.ws), p(allrec), len(ranks), which), "tfc_mask_merge")
    return allrec


def phased_forward(shards):
    lib, s = ops.lib(), ops.stream_ptr()
    ranks = [Rank(x) for x in shards]
    recs = [torch.empty(REC, dtype=torch.int64, device=DEV) for _ in ranks]
    for r, rec in zip(ranks, recs):
        ok(lib.tfc_mask_fwd_lap(s, p(r.img), p(r.lap), p(r.ws), p(rec), *r.dims), "tfc_mask_fwd_lap")
    rec_f1 = merge(ranks, recs, 0)
    for r, rec in zip(ranks, recs):
        ok(lib.tfc_mask_fwd_blur(s, p(r.lap), p(r.bl), p(r.ws), p(rec), *r.dims), "tfc_mask_fwd_blur")
    rec_f2 = merge(ranks, recs, 1)
    return ranks, rec_f1.cpu(), rec_f2.cpu()


def phased_backward(ranks, douts=None, refs=None, scale=1.0):
    """-> (dimg per rank, loss per rank or None)"""
    lib, s = ops.lib(), ops.stream_ptr()
    recs = [torch.empty(REC, dtype=torch.int64, device=DEV) for _ in ranks]
    us = [u.to(DEV).contiguous() for u in (douts if refs is None else refs)]
    dbufs = [torch.empty_like(r.bl) if refs is not None else None for r in ranks]
    dmns = [torch.empty_like(r.bl) for r in ranks]
    dimgs = [torch.empty((r.N, 3, r.H, r.W), device=DEV) for r in ranks]
    for r, rec, u, db in zip(ranks, recs, us, dbufs):
        ok(lib.tfc_mask_bwd_dot(s, p(r.bl), p(r.ws), p(u) if refs is None else None, p(u) if refs is not None else None, scale, p(db), p(rec), *r.dims),
           "tfc_mask_bwd_dot")
    merge(ranks, recs, 2)
    for r, rec, u, db, dmn in zip(ranks, recs, us, dbufs, dmns):
        ok(lib.tfc_mask_bwd_blur(s, p(r.lap), p(r.bl), p(r.ws), p(u if refs is None else db), p(dmn), p(rec), *r.dims), "tfc_mask_bwd_blur")
    merge(ranks, recs, 3)
    for r, dmn, dimg in zip(ranks, dmns, dimgs):
        ok(lib.tfc_mask_bwd_lap(s, p(r.lap), p(r.ws), p(dmn), p(dimg), *r.dims), "tfc_mask_bwd_lap")
    return dimgs, ([r.ws[7:8].clone() for r in ranks] if refs is not None else None)


def split(t, sizes):
    return list(torch.split(t, list(sizes)))


# ---- inputs and references, computed once ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_case():
    g = torch.Generator().manual_seed(2)                           # test_gpu_44_mask.py: CASES["n3_19x37"]
    img3 = torch.tanh(torch.randn(3, 3, 19, 37, generator=g))
    x, y = img3[0], img3[1]
    img = torch.stack([x, y, x, y])
    dout = torch.randn(4, 1, 19, 37, generator=torch.Generator().manual_seed(1202))       # different on the two copies
    parts = R.mask_parts(img.double())
    g64 = R.mask_vjp(img.double(), dout.double())
    return {"img": img, "dout": dout, "parts": parts, "grad64": g64, "err_bwd": rel_l2(R.mask_vjp(img, dout), g64),
            "err_fwd": (R.mask_maker(img).double() - parts["mask"]).abs().max().item()}


def assert_tie_conditions(c):
    """the minimum of L twice, in the copies of x; the maxima of L and of Bl twice, in the copies of y; each separated from its runner-up"""
    L, Bl = c["parts"]["L"], c["parts"]["Bl"]
    Ls, Bs = L.flatten().sort().values, Bl.flatten().sort().values
    assert Ls[0] == Ls[1] and Ls[2] - Ls[1] > 1e-5 and Ls[0] > 1e-5
    assert Ls[-1] == Ls[-2] and (Ls[-2] - Ls[-3]) / Ls[-1] > 1e-4
    assert Bs[-1] == Bs[-2] and (Bs[-2] - Bs[-3]) / Bs[-1] > 1e-4
    per = lambda t, f: f(t.flatten(1), 1).values                   # noqa: E731  per-sample extremum
    assert per(L, torch.min)[0] == Ls[0] and per(L, torch.min)[2] == Ls[0] and per(L, torch.min)[1] > Ls[0]
    assert per(L, torch.max)[1] == Ls[-1] and per(L, torch.max)[3] == Ls[-1] and per(L, torch.max)[0] < Ls[-1]
    assert per(Bl, torch.max)[1] == Bs[-1] and per(Bl, torch.max)[3] == Bs[-1] and per(Bl, torch.max)[0] < Bs[-1]


@functools.lru_cache(maxsize=None)
def ragged_case():
    """two samples of 70 x 130: several tiles with remainders both ways per sample"""
    g = torch.Generator().manual_seed(3)                           # chosen so that the separation asserted in the test holds
    img = torch.tanh(torch.randn(2, 3, 70, 130, generator=g))
    dout = torch.randn(2, 1, 70, 130, generator=g)
    parts = R.mask_parts(img.double())
    g64 = R.mask_vjp(img.double(), dout.double())
    return {"img": img, "dout": dout, "parts": parts, "grad64": g64, "err_bwd": rel_l2(R.mask_vjp(img, dout), g64)}


def assert_forward_equals_whole(img, ranks):
    whole = ops.mask_fwd(img.to(DEV), batch_scope="shard")
    assert torch.equal(torch.cat([r.lap for r in ranks]), whole.lap)
    assert torch.equal(torch.cat([r.bl for r in ranks]), whole.bl)
    for r in ranks:
        assert torch.equal(r.ws[:6], whole.ws[:6]), (r.ws[:6].tolist(), whole.ws[:6].tolist())
        mask = torch.empty_like(r.bl)
        ok(ops.lib().tfc_mask_scale(ops.stream_ptr(), p(r.bl), p(r.ws), p(mask), *r.dims), "tfc_mask_scale")
        r.mask = mask
    assert torch.equal(torch.cat([r.mask for r in ranks]), ops.mask_scale(whole))
    return whole


# ---- 1. the mask ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(2, 2), (1, 3)])
def test_mask_phases_on_shards_equal_the_whole_batch(sizes):
    c = tie_case()
    assert_tie_conditions(c)
    ranks, rec_f1, rec_f2 = phased_forward(split(c["img"], sizes))
    whole = assert_forward_equals_whole(c["img"], ranks)
    assert whole.ws[2:4].tolist() == [2.0, 2.0] and whole.ws[5].item() == 2.0        # all three tie counts
    # the records themselves: 64-bit counts; in (1, 3) rank 0 holds one copy of x: it has the minimum once and lower maxima
    counts = [(int(r[1]), int(r[3])) for r in rec_f1], [int(r[1]) for r in rec_f2]
    print(f"  split {sizes}: tie counts per rank (min, max of L) {counts[0]}, (max of Bl) {counts[1]}")
    assert sum(a for a, _ in counts[0]) == 2
    if sizes == (1, 3):
        assert counts[0][1] == (1, 2) and counts[1][1] == 2 and rec_f1[0][2] != rec_f1[1][2] and rec_f2[0][0] != rec_f2[1][0]
    else:
        assert counts[0] == [(1, 1), (1, 1)] and counts[1] == [1, 1]
    dimgs, _ = phased_backward(ranks, douts=split(c["dout"], sizes))
    err = rel_l2(torch.cat(dimgs).cpu(), c["grad64"])
    print(f"  split {sizes}: backward rel-L2 error {err:.3e} (fp32 CPU restatement {c['err_bwd']:.3e}, tol 8x)")
    assert err <= 8 * c["err_bwd"]


def test_mask_l1_phases_on_two_shards():
    """each rank's loss is its own share (the mean of the two is the loss of the batch); its dfake is the gradient of the SUM of the shares, i.e. twice
    the gradient of the batch loss"""
    c = tie_case()
    assert_tie_conditions(c)
    scale = 0.5
    real = torch.tanh(torch.randn(4, 3, 19, 37, generator=torch.Generator().manual_seed(109)))    # chosen so that the assertion below holds
    m_f, m_r = c["parts"]["mask"], R.mask_maker(real.double())
    assert (m_f - m_r).abs().min().item() > 1e-5
    err_r = (R.mask_maker(real).double() - m_r).abs().max().item()
    loss64, grad64 = R.mask_l1_grad(c["img"].double(), real.double(), scale)
    err32 = rel_l2(R.mask_l1_grad(c["img"], real, scale)[1], grad64)
    r_ranks, _, _ = phased_forward(split(real, (2, 2)))
    assert_forward_equals_whole(real, r_ranks)
    ranks, _, _ = phased_forward(split(c["img"], (2, 2)))
    dimgs, losses = phased_backward(ranks, refs=[r.mask for r in r_ranks], scale=scale)
    loss = 0.5 * (losses[0].item() + losses[1].item())
    tol_loss = scale * 8 * (c["err_fwd"] + err_r) + 2.0 ** -22 * loss64.item()
    err = rel_l2(torch.cat(dimgs).cpu(), 2.0 * grad64)
    print(f"  loss {loss:.8g} = mean of {losses[0].item():.8g}, {losses[1].item():.8g} (fp64 {loss64.item():.8g}, tol {tol_loss:.2e}); "
          f"gradient rel-L2 error {err:.3e} (fp32 CPU {err32:.3e}, tol 8x)")
    assert abs(loss - loss64.item()) <= tol_loss
    assert err <= 8 * err32


def test_mask_phases_on_ragged_tiles():
    c = ragged_case()
    L, Bl = c["parts"]["L"].flatten().sort().values, c["parts"]["Bl"].flatten().sort().values
    assert (L[-1] - L[-2]) / L[-1] > 1e-4 and (Bl[-1] - Bl[-2]) / Bl[-1] > 1e-4 and L[0] > 1e-5 and L[1] - L[0] > 1e-5      # test_gpu_44_mask.assert_separated
    ranks, _, _ = phased_forward(split(c["img"], (1, 1)))
    assert_forward_equals_whole(c["img"], ranks)
    dimgs, _ = phased_backward(ranks, douts=split(c["dout"], (1, 1)))
    err = rel_l2(torch.cat(dimgs).cpu(), c["grad64"])
    print(f"  2 x 70 x 130, split (1, 1): backward rel-L2 error {err:.3e} (fp32 CPU restatement {c['err_bwd']:.3e}, tol 8x)")
    assert err <= 8 * c["err_bwd"]


@pytest.mark.parametrize("which", ["tie", "ragged"])
def test_mask_phases_with_one_record_leave_the_bits_of_the_unsplit_entry_points(which):
    c = tie_case() if which == "tie" else ragged_case()
    img, dout = c["img"].to(DEV), c["dout"].to(DEV)
    ref = ops.mask_scale(ops.mask_fwd(img.flip(0), batch_scope="shard"))
    whole = ops.mask_fwd(img, batch_scope="shard")
    (rank,), _, _ = phased_forward([c["img"]])
    assert torch.equal(rank.lap, whole.lap) and torch.equal(rank.bl, whole.bl) and torch.equal(rank.ws[:6], whole.ws[:6])
    want = ops.mask_bwd(whole, dout=dout, batch_scope="shard")
    (got,), _ = phased_backward([rank], douts=[dout])
    assert torch.equal(got, want) and torch.equal(rank.ws[:10], whole.ws[:10])
    want_loss, want = ops.mask_bwd(whole, ref=ref, scale=0.5, batch_scope="shard")
    (got,), (loss,) = phased_backward([rank], refs=[ref], scale=0.5)
    assert torch.equal(got, want) and torch.equal(loss, want_loss) and torch.equal(rank.ws[:10], whole.ws[:10])


def test_phase_argument_checks_return_errors_without_launching():
    lib, s = ops.lib(), ops.stream_ptr()
    img = torch.zeros(1, 3, 8, 8, device=DEV)
    lap, bl, dmn, ws = (torch.full((64,), 5.0, device=DEV) for _ in range(4))
    rec = torch.full((4 * REC,), 7, dtype=torch.int64, device=DEV)
    a = dict(img=p(img), lap=p(lap), bl=p(bl), dmn=p(dmn), ws=p(ws), rec=p(rec))
    assert lib.tfc_mask_fwd_lap(s, None, a["lap"], a["ws"], a["rec"], 1, 8, 8) != 0
    assert lib.tfc_mask_fwd_lap(s, a["img"], a["lap"], a["ws"], None, 1, 8, 8) != 0
    assert lib.tfc_mask_fwd_lap(s, a["img"], a["lap"], a["ws"], a["rec"] + 4, 1, 8, 8) != 0             # misaligned record
    assert lib.tfc_mask_fwd_lap(s, a["img"], a["lap"], a["ws"], a["rec"], 1, 7, 8) != 0
    assert lib.tfc_mask_fwd_blur(s, a["lap"], None, a["ws"], a["rec"], 1, 8, 8) != 0
    assert lib.tfc_mask_fwd_blur(s, a["lap"], a["bl"], a["ws"], a["rec"], 0, 8, 8) != 0
    for world, which in ((0, 0), (-1, 1), (65, 0), (1, -1), (1, 4)):
        assert lib.tfc_mask_merge(s, a["ws"], a["rec"], world, which) != 0, (world, which)
        assert "world" in last_error() or "which" in last_error()
    assert lib.tfc_mask_merge(s, None, a["rec"], 1, 0) != 0 and lib.tfc_mask_merge(s, a["ws"], None, 1, 0) != 0
    assert lib.tfc_mask_bwd_dot(s, a["bl"], a["ws"], None, None, 1.0, None, a["rec"], 1, 8, 8) != 0     # neither dout nor ref
    assert lib.tfc_mask_bwd_dot(s, a["bl"], a["ws"], a["lap"], a["lap"], 1.0, a["dmn"], a["rec"], 1, 8, 8) != 0    # both
    assert lib.tfc_mask_bwd_dot(s, a["bl"], a["ws"], None, a["lap"], 1.0, None, a["rec"], 1, 8, 8) != 0  # ref without dout_buf
    assert lib.tfc_mask_bwd_dot(s, a["bl"], a["ws"], a["lap"], None, 1.0, None, None, 1, 8, 8) != 0
    assert lib.tfc_mask_bwd_blur(s, a["lap"], a["bl"], a["ws"], None, a["dmn"], a["rec"], 1, 8, 8) != 0
    assert lib.tfc_mask_bwd_blur(s, a["lap"], a["bl"], a["ws"], a["lap"], a["dmn"], None, 1, 8, 8) != 0
    assert lib.tfc_mask_bwd_lap(s, a["lap"], a["ws"], a["dmn"], None, 1, 8, 8) != 0
    assert lib.tfc_mask_bwd_lap(s, a["lap"], a["ws"], a["dmn"], a["img"], 1, 8, 1 << 21) != 0
    x = torch.full((2, 8), 3.0, device=DEV)
    krec, out = torch.full((3, 8, 2), 9.0, device=DEV), torch.zeros(2, device=DEV)
    assert lib.tfc_batch_kl_stats(s, p(x), p(x), None, 2, 8, p(krec)) != 0
    assert lib.tfc_batch_kl_stats(s, p(x), p(x), p(x), 2, 0, p(krec)) != 0 and "M" in last_error()
    assert lib.tfc_batch_kl_stats(s, p(x), p(x), p(x), 2, 8, None) != 0
    for world, M in ((0, 8), (65, 8), (1, 0)):
        assert lib.tfc_batch_kl_merge(s, p(krec), world, M, p(krec)) != 0, (world, M)
    assert lib.tfc_batch_kl_merge(s, None, 1, 8, p(krec)) != 0 and lib.tfc_batch_kl_merge(s, p(krec), 1, 8, None) != 0
    assert lib.tfc_batch_kl_terms(s, p(x), p(x), p(x), 2, 8, None, 1.0, p(out)) != 0
    assert lib.tfc_batch_kl_terms(s, p(x), p(x), p(x), 2, 8, p(krec), 1.0, None) != 0
    assert lib.tfc_batch_kl_terms(s, p(x), p(x), p(x), 0, 8, p(krec), 1.0, p(out)) != 0
    torch.cuda.synchronize()
    for t in (lap, bl, dmn, ws):
        assert bool((t == 5.0).all())
    assert bool((rec == 7).all()) and bool((krec == 9.0).all()) and not out.any() and not img.any()     # nothing ran
    assert lib.tfc_abi_version() == 3


# ---- 2. the KL loss -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kl_case(name):
    if name == "n5_m1000":                                         # test_gpu_41_region.py::test_regional_loss_properties: exp(t) underflows, ragged M
        gen, N, M = torch.Generator().manual_seed(5), 5, 1000
    else:                                                          # more than one pass of the 512 x 256 grid, and ragged
        gen, N, M = torch.Generator().manual_seed(6), 4, 131331
    af, pf, ar = (torch.randn(N, M, generator=gen) * s for s in (3e5, 2.0, 3e5))
    tt = torch.log_softmax(ar.double(), 0)
    want = [(tt.exp() * (tt - torch.log_softmax(v.double(), 0))).mean().item() for v in (af, pf)]
    return af, pf, ar, want


def kl_phases(shards, M, scale):
    """shards: per emulated rank (af, pf, ar) on the device -> out[2], the sum of every rank's scale * terms"""
    lib, s = ops.lib(), ops.stream_ptr()
    recs = torch.empty((len(shards), 3, M, 2), device=DEV)
    for r, (a, b, c) in enumerate(shards):
        ok(lib.tfc_batch_kl_stats(s, p(a), p(b), p(c), a.shape[0], M, p(recs[r])), "tfc_batch_kl_stats")
    glob = torch.empty((3, M, 2), device=DEV)
    ok(lib.tfc_batch_kl_merge(s, p(recs), len(shards), M, p(glob)), "tfc_batch_kl_merge")
    out = torch.zeros(2, device=DEV)
    for a, b, c in shards:
        ok(lib.tfc_batch_kl_terms(s, p(a), p(b), p(c), a.shape[0], M, p(glob), scale, p(out)), "tfc_batch_kl_terms")
    return out


@pytest.mark.parametrize("name,sizes", [("n5_m1000", (1, 4)), ("n5_m1000", (2, 3)), ("n4_m131331", (2, 2))])
def test_kl_phases_on_shards_vs_fp64_log_softmax_of_the_whole_batch(name, sizes):
    af, pf, ar, want = kl_case(name)
    shards = list(zip(*[[t.contiguous().to(DEV) for t in split(v, sizes)] for v in (af, pf, ar)]))
    out = kl_phases(shards, af.shape[1], 1.0 / af.numel())
    print(f"  {name} split {sizes}: amplitude term {out[0].item():.9g} (fp64 {want[0]:.9g}), phase term {out[1].item():.9g} (fp64 {want[1]:.9g})")
    assert abs(out[0].item() - want[0]) <= 1e-5 * abs(want[0])
    assert abs(out[1].item() - want[1]) <= 1e-5 * abs(want[1]) + 1e-6


@pytest.mark.parametrize("name", ["n5_m1000", "n4_m131331"])
def test_kl_phases_with_one_record_leave_the_bits_of_the_unsplit_kernel(name):
    af, pf, ar, _ = kl_case(name)
    af, pf, ar = af.to(DEV), pf.to(DEV), ar.to(DEV)
    want = torch.zeros(2, device=DEV)
    ops.batch_kl_sum(af, pf, ar, 1.0 / af.numel(), want, batch_scope="shard")
    got = kl_phases([(af, pf, ar)], af.shape[1], 1.0 / af.numel())
    assert torch.equal(got, want), (got.tolist(), want.tolist())


# ---- the Python surface without a process group: both scopes are the unsplit path ------------------------------------------------------------------
def test_both_scopes_are_the_same_launches_without_collectives():
    c = tie_case()
    img, dout = c["img"].to(DEV), c["dout"].to(DEV)
    a, b = ops.mask_fwd(img), ops.mask_fwd(img, batch_scope="shard")
    assert not a.phased and not b.phased and torch.equal(a.bl, b.bl) and torch.equal(a.ws[:6], b.ws[:6])
    assert torch.equal(ops.mask_bwd(a, dout=dout), ops.mask_bwd(b, dout=dout, batch_scope="shard"))
    assert torch.equal(T.mask_maker(img, batch_scope="global"), T.mask_maker(img, batch_scope="shard"))
    for bad in (lambda: ops.mask_fwd(img, batch_scope="rank"), lambda: ops.mask_bwd(a, dout=dout, batch_scope=None),
                lambda: T.mask_maker(img, batch_scope="all"), lambda: T.mask_l1_loss(img, img, batch_scope="x"),
                lambda: T.regional_fft_loss(img, img, "kl", batch_scope="x")):
        with pytest.raises(T.TfcError, match="batch_scope"):
            bad()
