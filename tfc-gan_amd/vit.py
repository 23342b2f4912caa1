"""The STN21 localiser (reference STN:150-201: `Net.stn_phi` = kornia VisionTransformer(256, patch 64, 6 channels) + the fc_loc MLP) on the
package's own HIP kernels (csrc/vit.hip), forward and backward, as ONE autograd Function. The patch size comes from the patch weight's shape:
patch 64 (17 tokens) runs the whole-sequence attention kernels, patch 32 / 16 (65 / 257 tokens) the tiled pair, which saves per-row softmax
statistics instead of the probabilities.

Numerics: the compute dtype follows `set_compute_dtype` -- bf16 rounds every GEMM and attention-matmul operand to bf16 with
fp32 accumulation (what `torch.autocast` does around the reference's ViT, STN:162), fp32 keeps the operands exact (f32-input MFMA); LayerNorm
statistics, softmax, GELU, the residual stream, stored activations and all gradients are fp32 in both. The result of a sample does not depend on the
batch it is computed in (bit for bit: tokens, theta, input gradient), and parameter gradients are sums in a fixed order (no float atomics).

The parameters are the modules' own `nn.Parameter`s, read as fp32 on every call (no cached bf16 copies: the optimizer moves them in place);
autograd accumulates the returned gradients into their `.grad` as it does for the torch layers.
"""
import torch

from . import ops
from .models import get_compute_dtype

EPS = 1e-6
_PER_BLOCK = 12       # norm1 w/b, qkv w/b, proj w/b, norm2 w/b, fc1 w/b, fc2 w/b


def vit_params(vit):
    """the VisionTransformer's parameters in the order the Function takes them"""
    ps = [vit.patch.weight, vit.patch.bias, vit.cls_token, vit.positions]
    for b in vit.blocks:
        ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight, b.attn.proj.bias, b.norm2.weight, b.norm2.bias,
               b.mlp[0].weight, b.mlp[0].bias, b.mlp[2].weight, b.mlp[2].bias]
    return ps + [vit.norm.weight, vit.norm.bias]


def head_params(fc_loc):
    return [t for i in (0, 2, 4, 6) for t in (fc_loc[i].weight, fc_loc[i].bias)]


def _f(t):
    return t.detach().contiguous().float()


class _LocaliserFn(torch.autograd.Function):
    """apply(meta, img_a, img_b, *params): meta = (dt, heads, with_head). img_b None: img_a carries every input channel (the concatenated pair).
    params = vit_params(...) [+ head_params(...) when with_head]. Returns theta delta [N, 6] (with_head) or the tokens [N, T, D]."""

    @staticmethod
    def forward(ctx, meta, img_a, img_b, *params):
        dt, heads, with_head = meta
        ops.require_gpu(img_a, img_b, *params)
        a = _f(img_a)
        b = _f(img_b) if img_b is not None else None
        ps = [_f(p) for p in params]
        N, uc, H, W = a.shape                                     # channels per image (with b: the same count in each)
        assert b is None or b.shape == a.shape, "the two images must have one shape"
        wp, bp, cls, pos = ps[:4]
        D, P = wp.shape[0], wp.shape[-1]
        Kp = wp[0].numel()
        assert Kp == (uc if b is None else 2 * uc) * P * P, "patch weight / input channels"
        npch = (H // P) * (W // P)
        T = npch + 1
        M = N * T
        depth = (len(ps) - 6 - (8 if with_head else 0)) // _PER_BLOCK
        unfold = (uc, H, W, P)
        x = torch.empty((N, T, D), dtype=torch.float32, device=a.device)
        ops.vit_gemm(dt, N * npch, D, Kp, a, wp.reshape(D, Kp), x[:, 1:, :], a_mode=ops.VIT_A_UNFOLD, a2=a if b is None else b, c_rg=npch,
                     c_rso=T * D, ldc=D, bias=bp, unfold=unfold)
        ops.vit_tokens_fwd(x, cls, pos)
        x = x.reshape(M, D)
        scale = float((D // heads) ** -0.5)
        saved = []
        for i in range(depth):
            g1, be1, wqkv, bqkv, wpr, bpr, g2, be2, w1, b1, w2, b2 = ps[4 + _PER_BLOCK * i: 4 + _PER_BLOCK * (i + 1)]
            h1, m1, r1 = ops.vit_layernorm_fwd(x, g1, be1, EPS)
            qkv = torch.empty((M, 3 * D), dtype=torch.float32, device=a.device)
            ops.vit_gemm(dt, M, 3 * D, D, h1, wqkv, qkv, bias=bqkv)
            if T <= 64:                                           # the whole-sequence kernels (patch 64: the bits every existing test pins)
                o, probs = ops.vit_attention_fwd(dt, qkv, N, T, heads, scale)
            else:                                                 # tiled kernels: `probs` holds the row statistics [N, H, 3, T], not [N, H, T, T]
                o, probs = ops.vit_attention_tiled_fwd(dt, qkv, N, T, heads, scale)
            xm = torch.empty_like(x)
            ops.vit_gemm(dt, M, D, D, o, wpr, xm, bias=bpr, res=x)
            h2, m2, r2 = ops.vit_layernorm_fwd(xm, g2, be2, EPS)
            hid = w1.shape[0]
            pre = torch.empty((M, hid), dtype=torch.float32, device=a.device)
            gl = torch.empty_like(pre)
            ops.vit_gemm(dt, M, hid, D, h2, w1, gl, bias=b1, act=ops.VIT_ACT_GELU, aux=pre)
            xn = torch.empty_like(x)
            ops.vit_gemm(dt, M, D, hid, gl, w2, xn, bias=b2, res=xm)
            saved.append((x, m1, r1, h1, qkv, probs, o, xm, m2, r2, h2, pre, gl))
            x = xn
        gf, bf = ps[4 + _PER_BLOCK * depth: 6 + _PER_BLOCK * depth]
        tok, mf, rf = ops.vit_layernorm_fwd(x, gf, bf, EPS)
        ctx.meta = (dt, heads, with_head, N, T, D, P, npch, Kp, depth, unfold, scale)
        ctx.imgs = (a, b)
        ctx.ps = ps
        ctx.saved = saved
        ctx.final = (x, mf, rf, tok)
        if not with_head:
            return tok.reshape(N, T, D)
        hw = ps[6 + _PER_BLOCK * depth:]
        z, acts = tok.reshape(N, T * D), []
        for j, act in enumerate((ops.VIT_ACT_RELU, ops.VIT_ACT_RELU, ops.VIT_ACT_SIGMOID, ops.VIT_ACT_NONE)):
            w, bb = hw[2 * j], hw[2 * j + 1]
            out = torch.empty((N, w.shape[0]), dtype=torch.float32, device=a.device)
            ops.vit_gemm(dt, N, w.shape[0], w.shape[1], z, w, out, bias=bb, act=act)
            acts.append(z)
            z = out
        ctx.head = (acts, z)
        return z

    @staticmethod
    def backward(ctx, grad):
        dt, heads, with_head, N, T, D, P, npch, Kp, depth, unfold, scale = ctx.meta
        a, b = ctx.imgs
        ps = ctx.ps
        need = ctx.needs_input_grad
        M = N * T
        dev = a.device
        grads = [None] * len(ps)
        g = _f(grad)

        def wgrad(dy, x, rows, n_out, k_in, lda=None, ldb=None):          # dW[n_out][k_in] = dyT x over `rows` rows
            dw = torch.empty((n_out, k_in), dtype=torch.float32, device=dev)
            ops.vit_gemm(dt, n_out, k_in, rows, dy, x, dw, a_mode=ops.VIT_A_TRANS, lda=n_out if lda is None else lda, b_mode=ops.VIT_B_ROWS,
                         ldb=k_in if ldb is None else ldb)
            return dw

        def dgrad(dy, w, rows, act=ops.VIT_ACT_NONE, aux=None, res=None):   # dX = dy W (times the derivative factor of the layer below)
            n_out, k_in = w.shape
            dx = torch.empty((rows, k_in), dtype=torch.float32, device=dev)
            ops.vit_gemm(dt, rows, k_in, n_out, dy, w, dx, b_mode=ops.VIT_B_ROWS, act=act, aux=aux, res=res)
            return dx

        base = 6 + _PER_BLOCK * depth
        if with_head:
            acts, _ = ctx.head
            hw = ps[base:]
            dacts = (ops.VIT_DACT_RELU, ops.VIT_DACT_RELU, ops.VIT_DACT_SIGMOID)
            dz = g.reshape(N, -1)
            for j in (3, 2, 1, 0):
                w = hw[2 * j]
                grads[base + 2 * j] = wgrad(dz, acts[j], N, w.shape[0], w.shape[1])
                grads[base + 2 * j + 1] = ops.vit_colsum(dz, N, w.shape[0])
                if j > 0:
                    dz = dgrad(dz, w, N, act=dacts[j - 1], aux=acts[j])
                else:
                    dz = dgrad(dz, w, N)
            dtok = dz.reshape(M, D)
        else:
            dtok = g.reshape(M, D)
        xl, mf, rf, _ = ctx.final
        dx, dgb = ops.vit_layernorm_bwd(dtok, xl, mf, rf, ps[base - 2])
        grads[base - 2], grads[base - 1] = dgb[0], dgb[1]
        for i in reversed(range(depth)):
            x, m1, r1, h1, qkv, probs, o, xm, m2, r2, h2, pre, gl = ctx.saved[i]
            o0 = 4 + _PER_BLOCK * i
            g1, _, wqkv, _, wpr, _, g2, _, w1, _, w2, _ = ps[o0:o0 + _PER_BLOCK]
            hid = w1.shape[0]
            grads[o0 + 10] = wgrad(dx, gl, M, D, hid)
            grads[o0 + 11] = ops.vit_colsum(dx, M, D)
            dpre = dgrad(dx, w2, M, act=ops.VIT_DACT_GELU, aux=pre)
            grads[o0 + 8] = wgrad(dpre, h2, M, hid, D)
            grads[o0 + 9] = ops.vit_colsum(dpre, M, hid)
            dh2 = dgrad(dpre, w1, M)
            dxm, dgb = ops.vit_layernorm_bwd(dh2, xm, m2, r2, g2, dres=dx)
            grads[o0 + 6], grads[o0 + 7] = dgb[0], dgb[1]
            grads[o0 + 4] = wgrad(dxm, o, M, D, D)
            grads[o0 + 5] = ops.vit_colsum(dxm, M, D)
            do = dgrad(dxm, wpr, M)
            if T <= 64:
                dqkv = ops.vit_attention_bwd(dt, do, qkv, probs, N, T, heads, scale)
            else:
                dqkv = ops.vit_attention_tiled_bwd(dt, do, qkv, o, probs, N, T, heads, scale)
            grads[o0 + 2] = wgrad(dqkv, h1, M, 3 * D, D)
            grads[o0 + 3] = ops.vit_colsum(dqkv, M, 3 * D)
            dh1 = dgrad(dqkv, wqkv, M)
            dx, dgb = ops.vit_layernorm_bwd(dh1, x, m1, r1, g1, dres=dxm)
            grads[o0], grads[o0 + 1] = dgb[0], dgb[1]
        # dx: gradient of the assembled tokens [N][T][D]
        dpos = ops.vit_colsum(dx, N, T * D).reshape(T, D)
        grads[3] = dpos
        grads[2] = dpos[0].clone().reshape(ps[2].shape)
        grads[1] = ops.vit_colsum(dpos[1:], T - 1, D)
        wp = ps[0]
        dxp = dx.reshape(N, T, D)[:, 1:, :]                                 # patch rows: row r at (r / npch) * T * D + (r % npch) * D
        img2 = a if b is None else b
        dwp = torch.empty((D, Kp), dtype=torch.float32, device=dev)
        ops.vit_gemm(dt, D, Kp, N * npch, dxp, a, dwp, a_mode=ops.VIT_A_TRANS, lda=D, a_rg=npch, a_rso=T * D, b_mode=ops.VIT_B_UNFOLD, ldb=Kp, b2=img2,
                     unfold=unfold)
        grads[0] = dwp.reshape(wp.shape)
        da = torch.empty_like(a) if need[1] else None
        db = torch.empty_like(b) if (b is not None and need[2]) else None
        if da is not None or db is not None:
            ops.vit_gemm(dt, N * npch, Kp, D, dxp, wp.reshape(D, Kp), da, a_rg=npch, a_rso=T * D, lda=D, b_mode=ops.VIT_B_ROWS, ldb=Kp,
                         c_mode=ops.VIT_C_UNFOLD, c2=db, unfold=unfold)
        ctx.saved = ctx.final = ctx.head = ctx.ps = ctx.imgs = None
        out = [None, da, db]
        for k, gr in enumerate(grads):
            out.append(gr if need[3 + k] else None)
        return tuple(out)


def _dt():
    dt = ops.dt_of(get_compute_dtype())
    if dt == ops.DT_BF16X3:
        raise ValueError('the HIP ViT localiser does not support the "bf16x3" compute mode (bf16 or fp32 only)')
    return dt


def vit_tokens(vit, img_a, img_b=None):
    """VisionTransformer forward on the HIP kernels: tokens [N, T, 768]; img_b None: img_a holds all input channels"""
    return _LocaliserFn.apply((_dt(), vit.blocks[0].attn.heads, False), img_a, img_b, *vit_params(vit))


def stn_phi(net, img_a, img_b=None):
    """Net.stn_phi on the HIP kernels: theta delta [N, 2, 3] of fc_loc(ViT(cat(img_a, img_b)))"""
    vit = net.localization.vit[0]
    th = _LocaliserFn.apply((_dt(), vit.blocks[0].attn.heads, True), img_a, img_b, *vit_params(vit), *head_params(net.fc_loc))
    return th.view(-1, 2, 3)
