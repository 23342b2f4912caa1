"""Host-side tests of the label-conditioned ("debiased") 4-patch step: the fp64 restatement tests/debias_ref.py against the fixtures lifted from the
reference scripts (1e-6 relative), the script weights, the key lists, the drawn labels, the annotated dataset and the refusals. No GPU."""
import csv

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import debias_ref as R
from tfc_gan_amd import ops
from tfc_gan_amd.engine import draw_gen_labels

HEADS = ("aux_gender", "aux_ethn", "aux_age")


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.fixture(scope="module")
def nets():
    """the fixtures' networks on the CPU (parameters only: nothing here runs a kernel)"""
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256), labels=3), seed=61)
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256), aux_classes=(2, 4, 3)), seed=62)
    with torch.no_grad():
        for k in HEADS:
            getattr(D, k)[0].weight.mul_(0.1)
    return G, D


def heads_case(nets):
    G, D = nets
    A, B = O.synthetic_pairs(2, seed=465)
    x8 = np.zeros((2, 256, 256, 8))
    x8[..., :3], x8[..., 3:6] = B.numpy().transpose(0, 2, 3, 1), A.numpy().transpose(0, 2, 3, 1)      # D(real_B, real_A): img_A = B
    ws = [getattr(D, k)[0].weight.detach().numpy() for k in HEADS]
    bs = [getattr(D, k)[0].bias.detach().numpy() for k in HEADS]
    return A, x8, ws, bs


def test_ref_matches_the_reference_heads_fixture(golden, nets):
    """fp64 logits, probabilities, the double-softmax cross entropy, its gradient through both softmaxes, the heads' input / weight / bias gradients
    and the label plane against the reference's modules (evaluated in double by make_golden_debias.py) at 1e-6 relative"""
    g = golden("debias_heads")
    G, _ = nets
    A, x8, ws, bs = heads_case(nets)
    probs, losses, dl = R.softmax_ce_heads(R.heads_fwd(x8, ws, bs), g["labels"])
    assert rel(probs, np.concatenate([g["gender_hat"], g["ethn_hat"], g["age_hat"]], 1)) <= 1e-6
    assert rel(losses[:3], g["ce_terms"]) <= 1e-6 and abs(losses[3] - g["ce_terms"].astype(np.float64).sum()) <= 1e-6 * losses[3]
    assert rel(R.heads_dgrad(dl, ws, 65536).reshape(2, 3, 256, 256)[:, :, ::8, ::8], g["g_input_sub"]) <= 1e-6
    dW, db = R.heads_wgrad([(x8, dl)])
    assert rel(dW[1][:, ::997], g["g_ethn_w_sub"]) <= 1e-6
    for h, key in enumerate(("g_gender_b", "g_ethn_b", "g_age_b")):
        assert rel(db[h], g[key]) <= 1e-6
    plane = R.plane(g["labels"], G.fc.weight.detach().numpy(), G.fc.bias.detach().numpy()).reshape(2, 256, 256)
    assert rel(plane[:, ::8, ::8], g["plane_sub"]) <= 1e-6
    packed = R.pack_labels(A.numpy(), g["labels"], G.fc.weight.detach().numpy(), G.fc.bias.detach().numpy())
    assert np.array_equal(packed[..., 3], plane) and not packed[..., 4:].any()


def test_ref_gradients_agree_with_autograd():
    """the hand-written double-softmax backward and the plane / head gradients against torch autograd in fp64"""
    rng = np.random.default_rng(3)
    N, HW = 4, 16
    z = torch.tensor(rng.normal(0, 1.5, (N, 9)), requires_grad=True)
    y = np.stack([rng.integers(0, k, N) for k in R.CLASSES], 1)
    w, s = (1.0, 10.0, 1.0), 1.0 / 3.0
    total = 0.0
    for h, (C, off) in enumerate(zip(R.CLASSES, R.offsets())):
        total = total + w[h] * torch.nn.functional.cross_entropy(torch.softmax(z[:, off:off + C], 1), torch.tensor(y[:, h]))
    (s * total).backward()
    probs, losses, dl = R.softmax_ce_heads(z.detach().numpy(), y, w, s)
    assert abs(losses[3] - float((s * total).detach())) <= 1e-12 and rel(dl, z.grad.numpy()) <= 1e-12
    x8 = rng.normal(0, 1, (N, 4, 4, 8))
    ws = [rng.normal(0, 1, (k, 6 * HW)) for k in R.CLASSES]
    X = torch.tensor(R.flat_input(x8), requires_grad=True)
    Wt = [torch.tensor(v, requires_grad=True) for v in ws]
    (torch.cat([X @ v.T for v in Wt], 1) * torch.tensor(dl)).sum().backward()
    assert rel(R.heads_dgrad(dl, ws, HW).reshape(N, -1), X.grad.numpy()[:, :3 * HW]) <= 1e-12
    dW, db = R.heads_wgrad([(x8, dl)])
    assert all(rel(a, b.grad.numpy()) <= 1e-12 for a, b in zip(dW, Wt)) and rel(np.concatenate(db), dl.sum(0)) <= 1e-12
    labels, g = rng.integers(0, 3, (N, 3)).astype(float), rng.normal(0, 1, (N, HW))
    dw, dbias = R.plane_bwd(g, labels)
    assert rel(dw, np.einsum("np,nk->pk", g, labels)) <= 1e-12 and rel(dbias, g.sum(0)) <= 1e-12


@pytest.mark.parametrize("kind", ["v1", "v3"])
def test_loss_composition_matches_the_step_fixtures(golden, kind):
    g = golden(f"train_step_debias_{kind}")
    f = {k: float(g[k]) for k in g.files if g[k].ndim == 0}
    assert abs(R.loss_G(kind, f["loss_GAN_g"], f["loss_triplet_patch"], f["loss_label"], f["loss_FFT"]) - f["loss_G"]) <= 1e-6 * f["loss_G"]
    kw = T.debias_weights(kind)
    mine = kw["lambda_gan"] * f["loss_GAN_g"] + kw["lambda_trip"] * f["loss_triplet_patch"] + kw["lambda_fft"] * f["loss_FFT"] + f["loss_label"]
    assert abs(mine - f["loss_G"]) <= 1e-6 * f["loss_G"]
    # the three label terms from the stored probabilities: the generator's against the labels it was fed, the discriminator's real pair against the
    # real labels and its fake pair against the drawn ones (DB1:522, :603-606; DB3:531, :612-618)
    fed = g["gen_labels"] if kw["labels"] == "generated" else g["labels"]
    for probs, targets, weights, scale, key in ((g["fake_probs"], fed, kw["label_weights"], 1.0, "loss_label"),
                                                (g["d_real_probs"], g["labels"], (1, 1, 1), kw["d_label_scale"], "real_loss_label"),
                                                (g["d_fake_probs"], g["gen_labels"], (1, 1, 1), kw["d_label_scale"], "fake_loss_label")):
        _, losses, _ = R.softmax_ce_heads(np.log(probs.astype(np.float64)), targets, weights, scale)       # softmax(log p) = p
        assert abs(losses[3] - f[key]) <= 1e-6 * max(1.0, f[key]), (key, losses[3], f[key])
    bce = 2.0 * f["loss_D"] - f["real_loss_label"] - f["fake_loss_label"]                                   # loss_real_g + loss_fake_g
    assert abs(R.loss_D(bce, 0.0, f["real_loss_label"], f["fake_loss_label"]) - f["loss_D"]) <= 1e-6 * f["loss_D"]


def test_debias_weights_table():
    assert T.debias_weights("v1") == {"lambda_gan": 1.0, "lambda_fft": 0.001, "lambda_trip": 1.0, "labels": "generated",
                                      "label_weights": (1.0, 1.0, 1.0), "d_label_scale": 1.0}
    assert T.debias_weights("v2") == {"lambda_gan": 1.0, "lambda_fft": 0.001, "lambda_trip": 0.0, "labels": "real",
                                      "label_weights": (1.0, 1.0, 1.0), "d_label_scale": 1.0 / 3.0}
    assert T.debias_weights("v3") == {"lambda_gan": 1.0, "lambda_fft": 0.001, "lambda_trip": 0.0, "labels": "real",
                                      "label_weights": (1.0, 10.0, 1.0), "d_label_scale": 1.0 / 3.0}
    with pytest.raises(T.TfcError):
        T.debias_weights("v4")


def test_state_dict_keys_and_parameter_orders(golden, nets):
    g = golden("debias_heads")
    G, D = nets
    assert list(G.state_dict().keys()) == list(g["g_keys"]) and list(D.state_dict().keys()) == list(g["d_keys"])
    assert tuple(G.fc.weight.shape) == (65536, 3) and tuple(G.down1.model[0].weight.shape) == (64, 4, 4, 4)
    assert tuple(D.aux_ethn[0].weight.shape) == (4, 393216) and isinstance(D.aux_age[1], torch.nn.Softmax)
    # defaults: today's modules and keys
    assert list(T.GeneratorUNet((3, 256, 256)).state_dict().keys()) == list(O.GeneratorUNet((3, 256, 256)).state_dict().keys())
    assert list(T.Discriminator1((3, 256, 256)).state_dict().keys()) == list(O.Discriminator1((3, 256, 256)).state_dict().keys())
    assert "fc.weight" not in T.nets.g_param_names() and not any(k.startswith("aux") for k in T.nets.d_param_names())
    # bucket order: fc.* last in G, the heads first in D; every trainable parameter has a place
    assert T.nets.g_backward_order()[-2:] == ["fc.weight", "fc.bias"] and T.nets.d_backward_order()[:6] == T.nets.d_aux_names()
    assert set(G.named_core_params()) == {k for k, _ in G.named_parameters()} and set(D.named_core_params()) == {k for k, _ in D.named_parameters()}
    flat = T.parallel.FlatParams(D.named_core_params(), T.nets.d_backward_order(), torch.device("cpu"))
    assert flat.order[:6] == T.nets.d_aux_names() and all(flat.offsets[k] % 4 == 0 for k in flat.order)
    assert T.nets.GeneratorCore(ops.DT_BF16, 3, 3).down[0][:3] == ("down1", 4, 64) and T.nets.GeneratorCore(ops.DT_BF16, 3).down == T.nets.G_DOWN


def test_gen_labels_draw():
    a = draw_gen_labels(64, seed=7, step=3, rank=0)
    assert a.shape == (64, 3) and a.dtype.kind == "i"
    for h, c in enumerate((2, 4, 3)):
        assert a[:, h].min() == 0 and a[:, h].max() == c - 1                 # 64 draws reach both ends of every range
    assert np.array_equal(a, draw_gen_labels(64, seed=7, step=3, rank=0))
    assert not np.array_equal(a, draw_gen_labels(64, seed=7, step=3, rank=1))
    assert not np.array_equal(a, draw_gen_labels(64, seed=7, step=4, rank=0))
    assert not np.array_equal(a, draw_gen_labels(64, seed=8, step=3, rank=0))
    assert np.array_equal(ops.check_targets(a), a.astype(np.int32))


def test_labelled_dataset_reads_the_annotations(tmp_path):
    from PIL import Image
    (tmp_path / "train").mkdir()
    rng = np.random.default_rng(5)
    names = ["c.png", "a.png", "b.png"]                                      # the CSV's order, not the directory's
    rows = [[n, "x", g, e, a] for n, (g, e, a) in zip(names, [(1, 3, 2), (0, 0, 0), (1, 2, 1)])]
    pix = {}
    for n in names:
        pix[n] = rng.integers(0, 256, (12, 32, 3), dtype=np.uint8)
        Image.fromarray(pix[n], "RGB").save(tmp_path / "train" / n)
    with open(tmp_path / "annots.csv", "w", newline="") as f:
        csv.writer(f).writerows([["file", "subject", "gender", "ethn", "age"]] + rows)
    ds = T.LabelledImageDataset(str(tmp_path / "annots.csv"), str(tmp_path))
    assert len(ds) == 3 and [p.rsplit("/", 1)[1] for p in ds.files] == names
    assert ds.labels.dtype == np.float32 and ds.labels.tolist() == [[1, 3, 2], [0, 0, 0], [1, 2, 1]]
    assert all(np.array_equal(ds[i], pix[n]) for i, n in enumerate(names))
    assert np.array_equal(ops.check_targets(torch.from_numpy(ds.labels)), ds.labels.astype(np.int32))
    with open(tmp_path / "bad.csv", "w", newline="") as f:
        csv.writer(f).writerows([["file", "gender"], ["a.png", 1]])
    with pytest.raises(T.TfcError):
        T.LabelledImageDataset(str(tmp_path / "bad.csv"), str(tmp_path))


def test_refusals(nets):
    G, D = nets
    with pytest.raises(T.TfcError, match="patches=4"):                       # before anything touches a device
        T.TrainStep(G, D, patches=16, labels="real")
    with pytest.raises(T.TfcError, match="labels="):
        T.TrainStep(G, D, patches=4, labels="fake")
    with pytest.raises(T.TfcError, match="labels=3"):
        T.TrainStep(T.GeneratorUNet((3, 256, 256)), D, patches=4, labels="real")
    with pytest.raises(T.TfcError, match="needs labels="):
        T.TrainStep(G, D, patches=4)
    with pytest.raises(T.TfcError):
        T.GeneratorUNet((3, 256, 256), labels=2)
    with pytest.raises(T.TfcError):
        T.Discriminator1((3, 256, 256), aux_classes=(2, 2, 2))
    with pytest.raises(T.TfcError, match="outside"):
        ops.check_targets([[0, 4, 0]])                                       # ethnicity has 4 classes
    with pytest.raises(T.TfcError, match="outside"):
        ops.check_targets(torch.tensor([[-1.0, 0.0, 0.0]]))
    with pytest.raises(T.TfcError, match="whole"):
        ops.check_targets([[0.5, 0, 0]])
    with pytest.raises(T.TfcError, match=r"\[N,3\]"):
        ops.check_targets([0, 1, 2])
    step = T.TrainStep.__new__(T.TrainStep)                                  # the step's own label check, without a device
    step.seed, step.dev, step.D = 0, torch.device("cpu"), T.nets.DiscriminatorCore(ops.DT_BF16, 3, (2, 4, 3))
    with pytest.raises(T.TfcError, match="needs labels="):
        step._label_tensors(None, None, 2, 1)
    with pytest.raises(T.TfcError, match="label rows"):
        step._label_tensors([[0, 0, 0]], None, 2, 1)
    real, gen = step._label_tensors([[1, 3, 2], [0, 1, 0]], None, 2, 1)
    assert real[1].dtype == torch.int32 and real[0].tolist() == [[1.0, 3.0, 2.0], [0.0, 1.0, 0.0]] and np.array_equal(gen[2], draw_gen_labels(2, 0, 1, 0))
    with pytest.raises(T.TfcError, match="forward\\(x, labels\\)"):
        G(torch.zeros(1, 3, 256, 256))
