"""fp64 restatement of the label-conditioned ("debiased") pieces, for the tests (numpy; nothing here is imported by the package).

Reference TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_debiased.py ("DB1"): the label plane fc(labels).view(N,1,H,W) (DB1:173), the three Linear + Softmax
heads on torch.cat((img_A, img_B), 1).view(N, -1) (DB1:224-231) and nn.CrossEntropyLoss applied to the softmax OUTPUT (DB1:522, :603-606), i.e.
loss_h = mean_n( logsumexp(p_h[n]) - p_h[n, y] ) with p_h = softmax(z_h): a second log-softmax on top of the first, kept as the reference has it.
Held to tests/golden/debias_heads.npz and the step fixtures at 1e-6 relative (tests/test_debias_host.py).
"""
import numpy as np

CLASSES = (2, 4, 3)                 # gender, ethnicity, age (DB1:218-220)


def offsets(classes=CLASSES):
    return [int(sum(classes[:h])) for h in range(len(classes))]


def plane(labels, fc_w, fc_b):
    """labels [N,3], fc_w [HW,3], fc_b [HW] -> [N,HW]"""
    return np.asarray(labels, np.float64) @ np.asarray(fc_w, np.float64).T + np.asarray(fc_b, np.float64)[None]


def plane_bwd(g, labels):
    """g [N,HW]: gradient of the plane -> (d fc.weight [HW,3], d fc.bias [HW])"""
    g = np.asarray(g, np.float64)
    return g.T @ np.asarray(labels, np.float64), g.sum(0)


def pack_labels(img, labels, fc_w, fc_b):
    """img [N,3,H,W] -> [N,H,W,8]: channels 0..2 the image, 3 the plane, 4..7 zero"""
    N, _, H, W = img.shape
    out = np.zeros((N, H, W, 8), np.float64)
    out[..., :3] = np.asarray(img, np.float64).transpose(0, 2, 3, 1)
    out[..., 3] = plane(labels, fc_w, fc_b).reshape(N, H, W)
    return out


def flat_input(x8):
    """the packed discriminator input [N,H,W,8] (channels 0..5) -> torch.cat((img_A, img_B), 1).view(N, -1): column c*H*W + p"""
    N = x8.shape[0]
    return np.asarray(x8, np.float64)[..., :6].transpose(0, 3, 1, 2).reshape(N, -1)


def heads_fwd(x8, ws, bs):
    """ws: three [C_h, 6*H*W], bs: three [C_h] -> logits [N, sum C_h]"""
    X = flat_input(x8)
    return np.concatenate([X @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)[None] for w, b in zip(ws, bs)], 1)


def softmax(z):
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def softmax_ce_heads(logits, targets, weights=(1.0, 1.0, 1.0), scale=1.0, classes=CLASSES):
    """-> probs [N, sum C], losses [4] (three head terms, scale * weighted sum), dlogits [N, sum C] = d losses[3] / d logits"""
    z = np.asarray(logits, np.float64)
    y = np.asarray(targets).astype(np.int64)
    N = z.shape[0]
    probs, dl, losses = np.zeros_like(z), np.zeros_like(z), np.zeros(4)
    for h, (C, off) in enumerate(zip(classes, offsets(classes))):
        p = softmax(z[:, off:off + C])
        probs[:, off:off + C] = p
        m = p.max(1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(p - m).sum(1))
        losses[h] = np.mean(lse - p[np.arange(N), y[:, h]])
        dp = np.exp(p - lse[:, None])                            # softmax(p): the loss's own softmax
        dp[np.arange(N), y[:, h]] -= 1.0
        dp *= scale * weights[h] / N
        dl[:, off:off + C] = p * (dp - (dp * p).sum(1, keepdims=True))      # back through the module's softmax
    losses[3] = scale * sum(w * l for w, l in zip(weights, losses[:3]))
    return probs, losses, dl


def heads_dgrad(dlogits, ws, HW):
    """-> gradient w.r.t. the img_A half of the input, [N,3,HW]"""
    Wc = np.concatenate([np.asarray(w, np.float64) for w in ws], 0)          # [sum C, 6*HW]
    return (np.asarray(dlogits, np.float64) @ Wc)[:, :3 * HW].reshape(-1, 3, HW)


def heads_wgrad(pairs, classes=CLASSES):
    """pairs: [(x8, dlogits), ...] -> (three dW [C_h, 6*HW], three db [C_h])"""
    dW = sum(np.asarray(dl, np.float64).T @ flat_input(x8) for x8, dl in pairs)
    db = sum(np.asarray(dl, np.float64).sum(0) for _, dl in pairs)
    offs = offsets(classes)
    return [dW[o:o + c] for o, c in zip(offs, classes)], [db[o:o + c] for o, c in zip(offs, classes)]


def loss_G(kind, l_gan, l_trip, l_label, l_fft):
    """DB1:572 / DB2:582 / DB3:583 without the LPIPS and temperature terms"""
    return l_gan + l_trip + l_label + 0.001 * l_fft if kind == "v1" else l_gan + l_label + 0.001 * l_fft


def loss_D(l_real, l_fake, real_ll, fake_ll):
    """DB1:609 (real_ll / fake_ll already carry the script's 1 or 1/3)"""
    return 0.5 * ((l_real + real_ll) + (l_fake + fake_ll))
