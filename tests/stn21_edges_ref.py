"""Plain restatements shared by tests/test_gpu_42_stn21_edges.py (against the kernels) and tests/test_stn21_edges_host.py (against torch, on the
CPU): attention forward / backward with the bf16 rounding points of csrc/vit.hip as switches, LayerNorm in one-pass and two-pass fp32, a scalar
model of the morphological gradient with the kernel's tie rule, and the row-triplet data whose hinge margins the tests assert. No import side
effects, no GPU."""
import numpy as np
import torch
import torch.nn as nn

# ---- attention ---------------------------------------------------------------------------------------------------------------------------------
# tfc_vit_attn_fwd / _bwd in bf16 mode round: q, k, v and dO when they are loaded; P before P v and before Pt dO (the SAVED probabilities stay
# fp32, and dS is formed from the fp32 P); dS before dS k, dSt q. Everything else (logits, softmax, sums) is fp32 there, fp64 here.
ROUNDINGS = ("q", "k", "v", "do", "p", "ds")


def bf16r(x):
    """x rounded to bf16 (through fp32, as the kernel's operands are fp32 when it rounds them), in x's dtype"""
    return x.float().bfloat16().to(x.dtype)


def pack_dqkv(dq, dk, dv):
    """[N, H, T, 64] x 3 -> [N*T, 3*H*64] in the qkv layout"""
    N, H, T, _ = dq.shape
    return torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(N * T, 3 * H * 64)


def attention_model(qkv, dout, N, T, H, scale, dtype=torch.float64, rounding=(), parts=None):
    """qkv [N*T, 3*H*64] in the reshape(n, t, 3, heads, 64) layout, dout [N*T, H*64] or None -> (out [N*T, H*64], probs [N, H, T, T], dqkv or
    None), computed in `dtype` with the operands named in `rounding` rounded to bf16 where the kernel rounds them. The backward is written out
    (dS = P (dP - rowsum(P dP)) scale), not taken from autograd, so that the rounding of P and dS has a place to stand. `parts` (a dict)
    receives q, k as used and dS before its rounding."""
    assert set(rounding) <= set(ROUNDINGS), rounding

    def r(name, x):
        return bf16r(x) if name in rounding else x
    D = H * 64
    x = qkv.to(dtype).reshape(N, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = r("q", x[0]), r("k", x[1]), r("v", x[2])
    P = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
    out = (r("p", P) @ v).transpose(1, 2).reshape(N * T, D)
    if dout is None:
        return out, P, None
    go = r("do", dout.to(dtype).reshape(N, T, H, 64).permute(0, 2, 1, 3))
    dP = go @ v.transpose(-2, -1)
    dS_raw = P * (dP - (P * dP).sum(-1, keepdim=True)) * scale
    if parts is not None:
        parts.update(q=q, k=k, dS=dS_raw)
    dS = r("ds", dS_raw)
    return out, P, pack_dqkv(dS @ k, dS.transpose(-2, -1) @ q, r("p", P).transpose(-2, -1) @ go)


def attention_autograd(qkv, dout, N, T, H, scale):
    """the same attention through torch autograd in fp64 (the form of the existing GPU test)"""
    D = H * 64
    qd = qkv.double().requires_grad_(True)
    q, k, v = qd.reshape(N, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    P = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
    out = (P @ v).transpose(1, 2).reshape(N * T, D)
    out.backward(dout.double())
    return out.detach(), P.detach(), qd.grad


def attention_inputs(N, T, H, seed=0, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N * T, 3 * H * 64, generator=g) * gain, torch.randn(N * T, H * 64, generator=g)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------
def layernorm_fp32(x, gamma, beta, eps, two_pass=True):
    """fp32 LayerNorm rows the way tfc_vit_ln_fwd_kernel orders them (two_pass: mean, then the variance of the centred values) or the way it
    must NOT (one pass: E[x^2] - mean^2, which cancels when the rows carry a large common offset)"""
    x = x.float()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True) if two_pass else (x * x).mean(-1, keepdim=True) - mu * mu
    return (x - mu) * torch.rsqrt(var + eps) * gamma.float() + beta.float()


# ---- morphological gradient --------------------------------------------------------------------------------------------------------------------
def morph_model(x, gout=None):
    """scalar model of tfc_morph_grad_fwd / _bwd_kernel on x [planes, H, W] (numpy fp32): max - min over the in-image pixels of the 3 x 3 cross,
    the FIRST maximum / minimum in the order centre, up, down, left, right (strict compares), and the backward that sends +g to the arg-max and
    -g to the arg-min pixel. Returns (out, dx or None)."""
    x = np.asarray(x, dtype=np.float32)
    P, H, W = x.shape
    out = np.zeros_like(x)
    dx = None if gout is None else np.zeros_like(x)
    offs = ((-1, 0), (1, 0), (0, -1), (0, 1))
    for p in range(P):
        for i in range(H):
            for j in range(W):
                mx = mn = x[p, i, j]
                amx = amn = (i, j)
                for di, dj in offs:
                    ii, jj = i + di, j + dj
                    if ii < 0 or ii >= H or jj < 0 or jj >= W:
                        continue
                    v = x[p, ii, jj]
                    if v > mx:
                        mx, amx = v, (ii, jj)
                    if v < mn:
                        mn, amn = v, (ii, jj)
                out[p, i, j] = mx - mn
                if dx is not None:
                    dx[p, amx[0], amx[1]] += gout[p, i, j]
                    dx[p, amn[0], amn[1]] -= gout[p, i, j]
    return out, dx


def tied_planes(planes, H, W, seed, pad_rows=0):
    """values in {0, 1/4, .., 1} (plateaus and ties everywhere); the first pad_rows rows equal, as the warp's border padding leaves them"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 5, (planes, H, W), generator=g).float() / 4
    if pad_rows > 1:
        x[:, 1:pad_rows, :] = x[:, :1, :]
    return x


# (shape, seed, leading rows set equal): the tied (1, 3, 13, 9) case with its padded border; rows and columns of one pixel; a single pixel; a shape
# that does not fill its last workgroup (2 * 3 * 17 * 31 = 3162 = 12 * 256 + 90)
MORPH_CASES = (((1, 3, 13, 9), 1, 3), ((2, 1, 1, 7), 2, 0), ((2, 1, 7, 1), 3, 0), ((1, 1, 1, 1), 4, 0), ((2, 3, 17, 31), 5, 0))


def morph_case(shape, seed, pad_rows):
    """-> (x, gout) of `shape`: tied data and an integer-valued upstream gradient (every dx is then a short signed sum of small integers: exact)"""
    H, W = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    return tied_planes(planes, H, W, seed, pad_rows).reshape(shape), int_grad(shape, seed + 100)


def int_grad(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float()


# ---- row triplets ------------------------------------------------------------------------------------------------------------------------------
TRIPLET_ROWS = 8200                                                # 8192 row slots (2048 workgroups x 4 waves) + one ragged trip of 8 rows
TRIPLET_WIDTHS = (3, 20, 64, 65, 130)
TRIPLET_MARGIN = 0.05                                              # no row's hinge argument is nearer to 0 than this (asserted on the fp64 reference)


def triplet_rows(rows, W, seed):
    """a ~ N(0, 1); p = a + 0.3 noise; n = a + noise * (0.05 on even rows, 3.0 on odd rows); every 97th row has p = a exactly.
    For W >= 20 the hinge is active on exactly the even rows and no row comes nearer than 0.3 to the knife edge. At W = 3 the odd rows' hinge
    argument 1 + |a - p| - |a - n|, |a - n| = 3 chi(3), has density around 0: of 4100 odd rows about a dozen fall within 0.05 of it, and no
    seed avoids that (the best of 96 599 seeds scanned reached 0.026; the tail extrapolates to one seed in 10^9). So the draw itself keeps the
    margin: a row whose hinge argument lies within 0.06 of 0 gets a fresh noise vector for its negative from the same generator, until none is
    left. The tests then assert the margin over ALL rows and mask nothing."""
    g = torch.Generator().manual_seed(seed)
    a, e1, e2 = (torch.randn(rows, W, generator=g) for _ in range(3))
    p = a + 0.3 * e1
    p[::97] = a[::97]
    s = torch.where(torch.arange(rows) % 2 == 0, 0.05, 3.0)[:, None]
    while True:
        n = a + e2 * s
        near = triplet_ref(a, p, n)[2].abs() < TRIPLET_MARGIN + 0.01
        if not near.any():
            return a, p, n
        e2[near] = torch.randn(int(near.sum()), W, generator=g)


def triplet_ref(a, p, n, margin=1.0):
    """nn.TripletMarginLoss(margin, p=2) in fp64 on the given (fp32) values -> (loss, d loss / d a, the per-row hinge argument)"""
    ad = a.double().requires_grad_(True)
    pd, nd = p.double(), n.double()
    loss = nn.TripletMarginLoss(margin=margin, p=2)(ad, pd, nd)
    (ga,) = torch.autograd.grad(loss, ad)
    with torch.no_grad():
        hinge = margin + nn.functional.pairwise_distance(ad, pd) - nn.functional.pairwise_distance(ad, nd)
    return loss.detach(), ga, hinge
