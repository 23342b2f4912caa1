"""GPU tests of the label-conditioned ("debiased") 4-patch step: the kernels of csrc/debias.hip against tests/debias_ref.py (fp64, fed the same
dtype-rounded inputs), the full step against the fixtures lifted from the reference scripts, bit-level determinism and the unchanged defaults."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import debias_ref as R
from tfc_gan_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(20, 1), (20, 3), (20, 5), (256, 2)]          # (H = W, N): 400 pixels are a multiple of no chunk (1.56 chunks of 256); 256 x 256 is the product's
DTS = [(ops.DT_F32, "fp32"), (ops.DT_BF16, "bf16")]
OTHER = (3, 5, 4)                                       # 12 rows: the kernels' second instantiation (not the reference's 2 + 4 + 3)


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def close(got, want, what=""):
    """the project's bound for fp32 gradient heads: 1e-9 + 1e-5 * max|want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, bound = np.abs(got - want).max(), 1e-9 + 1e-5 * np.abs(want).max()
    print(f"{what}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


@functools.lru_cache(maxsize=None)
def case(S, N, classes=R.CLASSES):
    """host inputs of one shape, made once: images in [-1,1], labels, fc and head parameters at the fixture's scale, logit gradients"""
    rng = np.random.default_rng(1000 * S + N + sum(classes))
    HW = S * S
    c = {"a": rng.uniform(-1, 1, (N, 3, S, S)).astype(np.float32), "b": rng.uniform(-1, 1, (N, 3, S, S)).astype(np.float32),
         "a2": rng.uniform(-1, 1, (N, 3, S, S)).astype(np.float32),
         "labels": np.stack([rng.integers(0, k, N) for k in R.CLASSES], 1).astype(np.float32),
         "fc_w": rng.normal(0, 0.02, (HW, 3)).astype(np.float32), "fc_b": rng.normal(0, 0.02, HW).astype(np.float32),
         "ws": [rng.normal(0, 0.002 * (65536 / HW) ** 0.5, (k, 6 * HW)).astype(np.float32) for k in classes],
         "bs": [rng.normal(0, 0.1, k).astype(np.float32) for k in classes],
         "dl": rng.normal(0, 0.3, (N, sum(classes))).astype(np.float32), "dl2": rng.normal(0, 0.3, (N, sum(classes))).astype(np.float32),
         "g4": rng.normal(0, 1e-3, (N, 4, S, S)).astype(np.float32), "g3": rng.normal(0, 1e-3, (N, 3, S, S)).astype(np.float32),
         "y": np.stack([rng.integers(0, k, N) for k in classes], 1).astype(np.int32)}
    return c


def packed(dt, a, b):
    """the discriminator input as the step packs it, and its values as fp64 [N,H,W,8]"""
    x8 = ops.pack_nhwc8(dt, t(a), t(b))
    return x8, x8.t.float().cpu().numpy().astype(np.float64)


# ---- (a) / (b): the label plane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N", SHAPES)
def test_pack_labels_vs_ref(S, N):
    c = case(S, N)
    want = R.pack_labels(c["a"], c["labels"], c["fc_w"], c["fc_b"])
    x32 = ops.pack_nhwc8_labels(ops.DT_F32, t(c["a"]), t(c["labels"]), t(c["fc_w"]), t(c["fc_b"]))
    assert x32.t.dtype == torch.float32 and tuple(x32.t.shape) == (N, S, S, 8)
    close(x32.t.cpu().numpy(), want, f"pack_labels fp32 S={S} N={N}")
    assert torch.equal(x32.t[..., :3], t(c["a"]).permute(0, 2, 3, 1)) and not x32.t[..., 4:].any()
    # bf16: the same fp32 arithmetic rounded once (to nearest even) -- exactly the fp32 result cast
    x16 = ops.pack_nhwc8_labels(ops.DT_BF16, t(c["a"]), t(c["labels"]), t(c["fc_w"]), t(c["fc_b"]))
    assert x16.t.dtype == torch.bfloat16 and torch.equal(x16.t, x32.t.to(torch.bfloat16))


@pytest.mark.parametrize("S,N", SHAPES)
def test_label_plane_bwd_vs_ref(S, N):
    c = case(S, N)
    dw_want, db_want = R.plane_bwd(c["g4"][:, 3].reshape(N, -1), c["labels"])
    dw, db = torch.full((S * S, 3), 7.0, device=DEV), torch.full((S * S,), 7.0, device=DEV)
    ops.label_plane_bwd(t(c["g4"]), t(c["labels"]), dw, db)
    close(dw.cpu().numpy(), dw_want, f"d fc.weight S={S} N={N}")
    close(db.cpu().numpy(), db_want, f"d fc.bias S={S} N={N}")
    dw2, db2 = dw.clone(), db.clone()
    ops.label_plane_bwd(t(c["g4"]), t(c["labels"]), dw2, db2, accumulate=True)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


# ---- (c): the heads' logits -------------------------------------------------------------------------------------------------------------------
def linear_gap(X, ws, bs):
    """max |torch-CPU fp32 F.linear - fp64| on these very inputs: what one fp32 summation order costs against another"""
    W, b = np.concatenate(ws, 0), np.concatenate(bs, 0)
    f32 = F.linear(torch.from_numpy(X.astype(np.float32)), torch.from_numpy(W), torch.from_numpy(b)).numpy().astype(np.float64)
    return np.abs(f32 - (X @ W.astype(np.float64).T + b.astype(np.float64)[None])).max()


@pytest.mark.parametrize("dt,name", DTS)
@pytest.mark.parametrize("S,N", SHAPES)
def test_aux_heads_fwd_vs_ref(S, N, dt, name):
    """Bound: 4 x the gap between torch-CPU fp32 F.linear and fp64 on the same inputs, measured in the test (both are fp32 sums of the same products
    in different orders). Measured on the build machine's CPU: 256 x 256, N = 2 (393,216 terms, |z| <= 1.57): gap 5.0e-6 on fp32 inputs, 4.8e-6 on
    bf16-rounded ones; 20 x 20 (2,400 terms, |z| <= 1.78): gap 3.0e-7 .. 4.6e-7."""
    c = case(S, N)
    x8, xv = packed(dt, c["a"], c["b"])
    want = R.heads_fwd(xv, c["ws"], c["bs"])
    gap = linear_gap(R.flat_input(xv), c["ws"], c["bs"])
    ws, bs = [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]
    got = ops.aux_heads_fwd(dt, x8, ws, bs)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"aux_heads_fwd {name} S={S} N={N}: max err {err:.3e}, F.linear gap {gap:.3e}, max|z| {np.abs(want).max():.3f}")
    assert gap > 0 and err <= 4 * gap, (err, gap)
    assert torch.equal(got, ops.aux_heads_fwd(dt, x8, ws, bs))              # fixed slots, fixed order: the same bits every time


def test_aux_heads_other_class_counts():
    """12 rows in all: the kernels' general instantiation (weights and sums by 4-byte accesses)"""
    S, N = 20, 3
    c = case(S, N, OTHER)
    for dt, name in DTS:
        x8, xv = packed(dt, c["a"], c["b"])
        ws, bs = [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]
        got = ops.aux_heads_fwd(dt, x8, ws, bs, classes=OTHER)
        gap = linear_gap(R.flat_input(xv), c["ws"], c["bs"])
        assert np.abs(got.cpu().numpy() - R.heads_fwd(xv, c["ws"], c["bs"])).max() <= 4 * gap
        dws, dbs = [torch.full_like(w, 3.0) for w in ws], [torch.full_like(b, 3.0) for b in bs]
        ops.aux_heads_wgrad(dt, x8, t(c["dl"]), None, None, dws, dbs, classes=OTHER)
        dW, db = R.heads_wgrad([(xv, c["dl"])], OTHER)
        for h in range(3):
            close(dws[h].cpu().numpy(), dW[h], f"other wgrad {name} head {h}")
            close(dbs[h].cpu().numpy(), db[h], f"other bgrad {name} head {h}")
    g = t(c["g3"])
    ops.aux_heads_dgrad(g, ws, t(c["dl"]), classes=OTHER)
    close(g.cpu().numpy(), c["g3"].astype(np.float64) + R.heads_dgrad(c["dl"], c["ws"], S * S).reshape(N, 3, S, S), "other dgrad")
    probs, losses, dl = ops.softmax_ce_heads(t(c["dl"]), t(c["y"], torch.int32), (1.0, 2.0, 0.5), 0.25, classes=OTHER, targets_host=c["y"])
    p_want, l_want, dl_want = R.softmax_ce_heads(c["dl"], c["y"], (1.0, 2.0, 0.5), 0.25, OTHER)
    assert np.abs(losses.cpu().numpy() - l_want).max() <= 2e-6
    close(probs.cpu().numpy(), p_want, "other probs")
    close(dl.cpu().numpy(), dl_want, "other dlogits")


# ---- (d): softmax + cross entropy on the softmax output ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 5, 300])           # 300: more samples than the workgroup has threads
@pytest.mark.parametrize("weights,scale", [((1.0, 1.0, 1.0), 1.0), ((1.0, 10.0, 1.0), 1.0 / 3.0)])
def test_softmax_ce_heads_vs_ref(N, weights, scale):
    rng = np.random.default_rng(77 + N)
    z = rng.normal(0, 1.5, (N, 9)).astype(np.float32)
    y = np.stack([rng.integers(0, k, N) for k in R.CLASSES], 1).astype(np.int32)
    probs, losses, dl = ops.softmax_ce_heads(t(z), t(y, torch.int32), weights, scale, targets_host=y)
    p_want, l_want, dl_want = R.softmax_ce_heads(z, y, weights, scale)
    err = np.abs(losses.cpu().numpy().astype(np.float64) - l_want).max()
    print(f"softmax_ce N={N}: losses {losses.cpu().numpy()}, max err {err:.3e}")
    assert err <= 2e-6                                                      # the triplet head's bound (absolute)
    close(probs.cpu().numpy(), p_want, "probs")
    close(dl.cpu().numpy(), dl_want, "dlogits")
    p2, l2, none = ops.softmax_ce_heads(t(z), t(y, torch.int32), weights, scale, want_grad=False)
    assert none is None and torch.equal(p2, probs) and torch.equal(l2, losses)


# ---- (e) / (f): the heads' backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N", SHAPES)
def test_aux_heads_dgrad_vs_ref(S, N):
    c = case(S, N)
    g = t(c["g3"])
    ops.aux_heads_dgrad(g, [t(w) for w in c["ws"]], t(c["dl"]))
    close(g.cpu().numpy(), c["g3"].astype(np.float64) + R.heads_dgrad(c["dl"], c["ws"], S * S).reshape(N, 3, S, S), f"aux dgrad S={S} N={N}")


@pytest.mark.parametrize("dt,name", DTS)
@pytest.mark.parametrize("S,N", SHAPES)
def test_aux_heads_wgrad_vs_ref(S, N, dt, name):
    c = case(S, N)
    xr, xrv = packed(dt, c["a"], c["b"])
    xf, xfv = packed(dt, c["a2"], c["b"])
    dW, db = R.heads_wgrad([(xrv, c["dl"]), (xfv, c["dl2"])])
    shapes = [(k, 6 * S * S) for k in R.CLASSES]
    dws, dbs = [torch.full(s, 5.0, device=DEV) for s in shapes], [torch.full((k,), 5.0, device=DEV) for k in R.CLASSES]
    ops.aux_heads_wgrad(dt, xr, t(c["dl"]), xf, t(c["dl2"]), dws, dbs)
    for h in range(3):
        close(dws[h].cpu().numpy(), dW[h], f"aux wgrad {name} S={S} N={N} head {h}")
        close(dbs[h].cpu().numpy(), db[h], f"aux bgrad {name} S={S} N={N} head {h}")
    again_w, again_b = [torch.empty(s, device=DEV) for s in shapes], [torch.empty(k, device=DEV) for k in R.CLASSES]
    ops.aux_heads_wgrad(dt, xr, t(c["dl"]), xf, t(c["dl2"]), again_w, again_b)
    assert all(torch.equal(a, b) for a, b in zip(again_w + again_b, dws + dbs))
    # one launch per pair with the accumulate flag: real, then fake on top
    two_w, two_b = [torch.empty(s, device=DEV) for s in shapes], [torch.empty(k, device=DEV) for k in R.CLASSES]
    ops.aux_heads_wgrad(dt, xr, t(c["dl"]), None, None, two_w, two_b)
    ops.aux_heads_wgrad(dt, xf, t(c["dl2"]), None, None, two_w, two_b, accumulate=True)
    for h in range(3):
        close(two_w[h].cpu().numpy(), dW[h], f"aux wgrad in two launches {name} head {h}")
        close(two_b[h].cpu().numpy(), db[h], f"aux bgrad in two launches {name} head {h}")


# ---- bit-level and sanity checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,name", DTS)
def test_sample0_bits_do_not_depend_on_the_batch(dt, name):
    S = 20
    c = case(S, 3)
    ws, bs = [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]
    out = {}
    for N in (1, 3):
        a, b, lab = t(c["a"][:N]), t(c["b"][:N]), t(c["labels"][:N])
        x = ops.pack_nhwc8_labels(dt, a, lab, t(c["fc_w"]), t(c["fc_b"]))
        logits = ops.aux_heads_fwd(dt, ops.pack_nhwc8(dt, a, b), ws, bs)
        probs, _, _ = ops.softmax_ce_heads(logits, t(c["y"][:N], torch.int32))
        out[N] = (x.t[0].clone(), logits[0].clone(), probs[0].clone())
    for one, three in zip(out[1], out[3]):
        assert torch.equal(one, three)


def test_zero_head_weights_give_uniform_probabilities():
    S, N = 20, 3
    c = case(S, N)
    x8, _ = packed(ops.DT_BF16, c["a"], c["b"])
    ws = [torch.zeros(k, 6 * S * S, device=DEV) for k in R.CLASSES]
    bs = [torch.zeros(k, device=DEV) for k in R.CLASSES]
    logits = ops.aux_heads_fwd(ops.DT_BF16, x8, ws, bs)
    assert not logits.any()
    probs, losses, dl = ops.softmax_ce_heads(logits, t(c["y"], torch.int32))
    for C, off in zip(R.CLASSES, R.offsets()):
        assert torch.equal(probs[:, off:off + C], torch.full((N, C), 1 / C, dtype=torch.float32, device=DEV))
    # CrossEntropyLoss of the uniform vector u = 1/C: logsumexp(u) - u = log C
    assert np.abs(losses[:3].cpu().numpy() - np.log(np.array(R.CLASSES, np.float64))).max() <= 2e-6
    assert abs(float(losses[3]) - float(np.log(24.0))) <= 2e-6


def test_argument_checks_return_errors_without_launching():
    S, N = 20, 2
    c = case(S, 3)
    L = ops.lib()
    st, i3 = ops.stream_ptr(), (ctypes.c_int * 3)
    x8, _ = packed(ops.DT_BF16, c["a"][:N], c["b"][:N])
    ws, bs = [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]
    w3, b3 = ops._ptr3(ws), ops._ptr3(bs)
    logits = torch.full((N, 9), 3.0, device=DEV)
    pw = ops.part_ws(DEV)
    ok = i3(2, 4, 3)

    def refused(rc, word):
        assert rc != 0 and word in L.tfc_last_error().decode(), (rc, L.tfc_last_error())
    refused(L.tfc_aux_heads_fwd(st, ops.DT_BF16, None, 8, N, S, S, w3, b3, ok, ops._p(logits), pw), "null")
    refused(L.tfc_aux_heads_fwd(st, ops.DT_BF16, x8.ptr, 16, N, S, S, w3, b3, ok, ops._p(logits), pw), "pitch")
    refused(L.tfc_aux_heads_fwd(st, ops.DT_BF16, x8.ptr, 8, N, S, S, w3, b3, i3(8, 8, 1), ops._p(logits), pw), "16 rows")
    refused(L.tfc_aux_heads_fwd(st, ops.DT_BF16, x8.ptr, 8, N, S, S, w3, b3, ok, ops._p(logits), None), "null")
    refused(L.tfc_aux_heads_fwd(st, ops.DT_BF16, x8.ptr, 8, N, 3, 3, w3, b3, ok, ops._p(logits), pw), "multiple of 4")
    dws, dbs = [torch.full_like(w, 3.0) for w in ws], [torch.full_like(b, 3.0) for b in bs]
    refused(L.tfc_aux_heads_wgrad(st, ops.DT_BF16, x8.ptr, ops._p(logits), None, None, 12, N, S, S, ops._ptr3(dws), ops._ptr3(dbs), ok, 0), "pitch")
    refused(L.tfc_aux_heads_wgrad(st, ops.DT_BF16, x8.ptr, None, None, None, 8, N, S, S, ops._ptr3(dws), ops._ptr3(dbs), ok, 0), "null")
    g = torch.full((N, 3, S, S), 3.0, device=DEV)
    refused(L.tfc_aux_heads_dgrad(st, None, 3, N, S, S, w3, ok, ops._p(logits)), "null")
    refused(L.tfc_aux_heads_dgrad(st, ops._p(g), 3, N, S, S, w3, i3(9, 9, 9), ops._p(logits)), "16 rows")
    refused(L.tfc_pack_nhwc8_labels(st, ops.DT_BF16, ops._p(g), None, ops._p(g), ops._p(g), x8.ptr, N, S, S), "null")
    refused(L.tfc_label_plane_bwd(st, ops._p(g), 3, 3, ops._p(logits), ops._p(g), ops._p(g), N, S, S, 0), "channel")
    y_bad = np.array([[0, 4, 0], [1, 0, 2]], np.int32)                      # ethnicity has 4 classes
    with pytest.raises(T.TfcError, match="outside"):
        ops.softmax_ce_heads(logits, t(y_bad, torch.int32), targets_host=y_bad)
    with pytest.raises(T.TfcError, match="outside"):
        ops.check_targets(y_bad)
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it held
    assert all(bool((v == 3.0).all()) for v in [logits, g] + dws + dbs)


# ---- the full step ----------------------------------------------------------------------------------------------------------------------------
HEAD_KEYS = ["aux_gender.0.weight", "aux_ethn.0.weight", "aux_age.0.weight"]
LOSS_KEYS = ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_D", "loss_label", "real_loss_label", "fake_loss_label")


def debias_nets(seed_g=61, seed_d=62):
    """the fixtures' networks: portable initialiser, the three head weights multiplied by 0.1 (tests/golden/make_golden_debias.py says why)"""
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256), labels=3), seed=seed_g)
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256), aux_classes=(2, 4, 3)), seed=seed_d)
    with torch.no_grad():
        for k in ("aux_gender", "aux_ethn", "aux_age"):
            getattr(D, k)[0].weight.mul_(0.1)
    return G.to(DEV).eval(), D.to(DEV).train()


@pytest.mark.parametrize("kind", ["v1", "v3"])
def test_debias_train_step_fp32_vs_reference_golden(golden, kind):
    """TrainStep(**debias_weights(kind), patches=4) at N = 2 in fp32 compute mode against one step of the networks lifted from the label-conditioned
    scripts: the checks and tolerances of test_patch4_train_step_fp32_vs_reference_golden (losses 2e-4, gradient tensors 1e-2 relative L2, Adam
    deltas 2e-6 mean), the new losses, gradients and deltas in the same classes; the heads' probabilities at 1e-5"""
    g = golden(f"train_step_debias_{kind}")
    T.set_compute_dtype(torch.float32)
    try:
        G, D = debias_nets()
        gb = {k: v.clone() for k, v in G.state_dict().items()}
        db = {k: v.clone() for k, v in D.state_dict().items()}
        A, B = O.synthetic_pairs(2, seed=465)
        ts = T.TrainStep(G, D, compute_dtype=torch.float32, patches=4, **T.debias_weights(kind))
        out = ts.step(A.to(DEV), B.to(DEV), neg_idx=g["neg_idx"].tolist(), labels=torch.tensor(g["labels"], dtype=torch.float32),
                      gen_labels=g["gen_labels"])
        torch.cuda.synchronize()
    finally:
        T.set_compute_dtype(torch.bfloat16)
    assert set(out) == {"loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D", "fake_B", "loss_label",
                        "real_loss_label", "fake_loss_label", "fake_probs", "d_real_probs", "d_fake_probs"}
    for k in LOSS_KEYS:
        want = float(g[k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 2e-4 * max(1.0, abs(want)), (k, float(out[k]), want)
    assert (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["fake_sub"]).cpu()).abs().mean().item() <= 1e-4
    for k in ("fake_probs", "d_real_probs", "d_fake_probs"):
        err = np.abs(out[k].cpu().numpy() - g[k]).max()
        print(f"  {k}: max err {err:.3e}")
        assert err <= 1e-5, (k, err)

    def rel(got, want, tol=1e-2):
        want = torch.as_tensor(want).double()
        r = ((got.cpu().double() - want).norm() / want.norm()).item()
        print(f"  grad rel-L2 error {r:.3e} (tol {tol})")
        return r <= tol

    assert rel(ts.gflat.grad_views["down1.model.0.weight"], g["g_grad_down1"])                     # all 4 input channels
    assert rel(ts.gflat.grad_views["up3.model.0.weight"][::16, ::16], g["g_grad_up3"])
    assert rel(ts.gflat.grad_views["fc.weight"][::61], g["g_grad_fc_w"])
    assert rel(ts.gflat.grad_views["fc.bias"][::61], g["g_grad_fc_b"])
    assert rel(ts.dflat.grad_views["model.13.weight"], g["d_grad_head"])
    assert rel(ts.dflat.grad_views["model.0.bias"], g["d_grad_b0"])
    assert rel(ts.dflat.grad_views["model.3.parametrizations.weight.original"][::8, ::8], g["d_grad_w3"])
    assert rel(ts.dflat.grad_views["aux_ethn.0.weight"][:, ::997], g["d_grad_ethn_w"])
    assert rel(torch.cat([ts.dflat.grad_views[k.replace("weight", "bias")] for k in HEAD_KEYS]), g["d_grad_aux_b"])
    for key, ref, sub in (("final.2.weight", g["g_delta_final_w"], None), ("down1.model.0.weight", g["g_delta_down1"], None),
                          ("fc.bias", g["g_delta_fc_b"], slice(None, None, 61))):
        got = (G.state_dict()[key] - gb[key]).cpu()
        got = got if sub is None else got[sub]
        assert (got - torch.as_tensor(ref)).abs().mean().item() <= 2e-6, key
    got = (D.state_dict()["model.13.weight"] - db["model.13.weight"]).cpu()
    assert (got - torch.as_tensor(g["d_delta_head"])).abs().mean().item() <= 2e-6
    got = (D.state_dict()["aux_gender.0.weight"] - db["aux_gender.0.weight"]).cpu()[:, ::997]
    assert (got - torch.as_tensor(g["d_delta_gender_w"])).abs().mean().item() <= 2e-6
    assert torch.allclose(D.state_dict()["model.3.parametrizations.weight.0._u"].cpu(), torch.as_tensor(g["d_u3"]), atol=1e-4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, "bf16x3"])
def test_debias_train_step_bf16_losses(golden, dtype):
    """the bf16 step at N = 2 against the v1 fixture: losses within the project's bf16 step bound (3e-2 relative, test_train_step_bf16_vs_reference_golden;
    tests/test_gpu_39_patch4.py holds no bf16 bound of its own). The bf16x3 mode (fp32 storage, three-term bf16 products: at least bf16's precision
    everywhere) takes the same step through the non-fused branches and is held to the same bound."""
    g = golden("train_step_debias_v1")
    T.set_compute_dtype(dtype)
    try:
        G, D = debias_nets()
        A, B = O.synthetic_pairs(2, seed=465)
        ts = T.TrainStep(G, D, compute_dtype=dtype, patches=4, **T.debias_weights("v1"))
        out = ts.step(A.to(DEV), B.to(DEV), neg_idx=g["neg_idx"].tolist(), labels=g["labels"], gen_labels=g["gen_labels"])
        torch.cuda.synchronize()
    finally:
        T.set_compute_dtype(torch.bfloat16)
    for k in LOSS_KEYS:
        want = float(g[k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 3e-2 * max(1.0, abs(want)), (k, float(out[k]), want)
    for k in ("fc.weight", "fc.bias", "aux_age.0.weight", "aux_age.0.bias"):
        grad = (ts.gflat if k.startswith("fc") else ts.dflat).grad_views[k]
        assert torch.isfinite(grad).all() and grad.abs().max().item() > 0, k


def test_debias_step_is_bit_deterministic_on_one_and_two_streams():
    """two labelled steps from the same state (bf16, N = 2, labels drawn by the step): the same bits run to run on two streams and against the
    one-stream schedule, in every parameter, gradient and loss"""
    runs = []
    prev = T.set_wgrad_stream(True)
    try:
        for on in (True, True, False):
            T.set_wgrad_stream(on)
            G, D = debias_nets(71, 72)
            A, B = O.synthetic_pairs(2, seed=73)
            A, B = A.to(DEV), B.to(DEV)
            ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, patches=4, **T.debias_weights("v1"))
            lab = np.array([[1, 3, 2], [0, 1, 0]])
            ts.step(A, B, labels=lab)
            out2 = ts.step(A, B, labels=lab)
            torch.cuda.synchronize()
            runs.append({"g_w": ts.gflat.data.clone(), "d_w": ts.dflat.data.clone(), "g_grad": ts.gflat.grad.clone(), "d_grad": ts.dflat.grad.clone(),
                         "fake": out2["fake_B"].clone(), "probs": torch.cat([out2[k] for k in ("fake_probs", "d_real_probs", "d_fake_probs")]).clone(),
                         "losses": torch.stack([out2[k].reshape(()).float() for k in sorted(out2) if out2[k].numel() == 1]).clone()})
    finally:
        T.set_wgrad_stream(prev)
    ref = runs[0]
    assert torch.isfinite(ref["losses"]).all() and ref["g_grad"].abs().max().item() > 0
    for what, other in (("two streams, run to run", runs[1]), ("two streams vs one stream", runs[2])):
        for k in ref:
            assert torch.equal(ref[k], other[k]), (what, k)


# ---- the modules and the defaults -------------------------------------------------------------------------------------------------------------
def test_modules_forward_with_labels_under_no_grad_and_refusal_under_autograd(golden):
    g = golden("debias_heads")
    T.set_compute_dtype(torch.float32)
    try:
        G, D = debias_nets()
        assert list(G.state_dict().keys()) == list(g["g_keys"]) and list(D.state_dict().keys()) == list(g["d_keys"])
        A, B = O.synthetic_pairs(2, seed=465)
        lab = torch.tensor(g["labels"], dtype=torch.float32)
        with torch.no_grad():
            fake = G(A.to(DEV), lab.to(DEV))
            logits, gh, eh, ah = D(B.to(DEV), A.to(DEV))
        assert tuple(fake.shape) == (2, 3, 256, 256) and tuple(logits.shape) == (2, 1, 16, 16) and torch.isfinite(fake).all()
        for got, key in ((gh, "gender_hat"), (eh, "ethn_hat"), (ah, "age_hat")):
            assert np.abs(got.cpu().numpy() - g[key]).max() <= 1e-5, key
        with pytest.raises(T.TfcError, match="TrainStep"):
            G(A.to(DEV), lab.to(DEV))
        with pytest.raises(T.TfcError, match="TrainStep"):
            D(B.to(DEV), A.to(DEV))
        with pytest.raises(T.TfcError, match="patches=4"):
            T.TrainStep(G, D, patches=16, labels="real")
        with pytest.raises(T.TfcError, match="labels"):
            T.TrainStep(G, D, patches=4)
        ts = T.TrainStep(G, D, compute_dtype=torch.float32, patches=4, **T.debias_weights("v2"))
        with pytest.raises(T.TfcError, match="needs labels"):
            ts.step(A.to(DEV), B.to(DEV))
        with pytest.raises(T.TfcError, match="outside"):
            ts.step(A.to(DEV), B.to(DEV), labels=[[0, 4, 0], [1, 0, 0]])
    finally:
        T.set_compute_dtype(torch.bfloat16)


def test_defaults_keep_keys_and_the_unlabelled_step_bits():
    """GeneratorUNet(shape) / Discriminator1(shape) keep the oracle's key lists, and a PATCH-4 step without labels gives the same bits whether or not
    a labelled step (every new code path) ran in the process before it"""
    assert list(T.GeneratorUNet((3, 256, 256)).state_dict().keys()) == list(O.GeneratorUNet((3, 256, 256)).state_dict().keys())
    assert list(T.Discriminator1((3, 256, 256)).state_dict().keys()) == list(O.Discriminator1((3, 256, 256)).state_dict().keys())

    def plain_step():
        G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=81).to(DEV)
        D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=82).to(DEV)
        A, B = O.synthetic_pairs(2, seed=83)
        ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, patches=4, seed=5)
        out = ts.step(A.to(DEV), B.to(DEV))
        torch.cuda.synchronize()
        assert set(out) == {"loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D", "fake_B"}
        return [ts.gflat.data.clone(), ts.dflat.data.clone(), ts.gflat.grad.clone(), ts.dflat.grad.clone(), out["fake_B"].clone(),
                torch.stack([out[k].reshape(()).float() for k in sorted(out) if k != "fake_B"])]
    before = plain_step()
    G, D = debias_nets()
    A, B = O.synthetic_pairs(2, seed=465)
    T.TrainStep(G, D, patches=4, **T.debias_weights("v3")).step(A.to(DEV), B.to(DEV), labels=[[1, 3, 2], [0, 1, 0]])
    after = plain_step()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
