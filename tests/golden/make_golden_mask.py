"""Generate the fixtures of the edge-mask 4-patch script, tests/golden/{mask_maker,train_step_mask4}.npz, from the REFERENCE'S OWN definitions (runs only
in the build container, like make_golden_patch4.py, whose helpers it shares).

Lifted by `ast`, executed on the CPU, from TFCGAN_multigpu_patchFFT_experiment.py ("4X"): mask_maker (4X:385-390), UNetDown, UNetUp, GeneratorUNet
(4-channel down1, forward(img_A, mask), 4X:141-181), Discriminator1, FFT_Components / fft_components, fft_loss (4X:317-339) and triplet_patches
(4X:343-367, its four np.random.randint draws handed in). kornia is not installed: the lifted mask_maker runs on the stand-in `K` of
tests/mask_ref.py (kornia's three functions restated from their definitions; parity with kornia itself is not pinned). The training loop is INLINE
in the script and therefore restated here line for line with the reference's own criteria (cited below). LPIPS (needs VGG weights) and the
temperature head (zero gradient) are left out, as in every other step fixture.

Conditions: N = 2, G.eval() / D.train(), init_weights_portable(G, 61) / (D, 62), CPU fp32 for the step, fp64 for the operator alone.
The step fixture holds TWO runs from the same state:
  (a) the weight of loss_mask in loss_G set to 0: everything train_step_patch4.npz holds. The mask still feeds the generator, so this pins the
      4-channel generator end to end, and only the VALUES of the batch extrema reach it;
  (b) the script's 0.5 * loss_mask: losses, fake and the discriminator-side results only. The generator's gradients of this run carry a
      single-pixel spike at the argmin of |laplacian|, whose position two correct implementations need not agree on.

No reference source text is written anywhere: only outputs are stored; inputs are regenerated from seeds.
Usage:  python tests/golden/make_golden_mask.py        (writes next to this file)
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import O, cuda_is_identity, lift, save  # noqa: E402  (sets MKL_CBWR before torch starts MKL)
from make_golden_patch4 import four  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import mask_ref  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REF = "/root/reference/TFC-GAN-FFT"
X4 = os.path.join(REF, "TFCGAN_multigpu_patchFFT_experiment.py")
NETS = ["UNetDown", "UNetUp", "GeneratorUNet", "Discriminator1"]
OP_CASES = [("n1_8x8", (1, 8, 8), 0), ("n3_19x37", (3, 19, 37), 2)]     # (tag, (N, H, W), seed): tanh(randn), as tests/test_gpu_44_mask.py draws them


class _Draws:
    """np.random for the lifted triplet_patches: randint hands out the given negatives in order (4X:354-357)"""

    def __init__(self, seq):
        self.seq = list(seq)

    def randint(self, n, size=1):
        return np.array([self.seq.pop(0)])


def op_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    N, H, W = shape
    return torch.tanh(torch.randn(N, 3, H, W, generator=g)), torch.randn(N, 1, H, W, generator=g)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    L = lift(X4, NETS + ["FFT_Components", "fft_components", "fft_loss", "mask_maker"], extra={"K": mask_ref.K})
    L["opt"].patch_height = L["opt"].patch_width = 128
    L["opt"].batch_size = 2
    trip = nn.TripletMarginLoss(margin=1.0, p=2)                             # 4X:77 triplet_loss
    bce = nn.BCEWithLogitsLoss()                                             # 4X:70 criterion_GAN
    l1 = nn.L1Loss()                                                         # 4X:85-86, :89 criterion_amp / criterion_phase / criterion_mask

    # (a) the operator alone, in double: the lifted mask_maker and autograd's gradient of sum(dout * mask)
    arrays = {}
    for tag, shape, seed in OP_CASES:
        img, dout = op_input(shape, seed)
        x = img.double().requires_grad_(True)
        m = L["mask_maker"](x)
        assert m.dtype == torch.float64 and tuple(m.shape) == (shape[0], 1) + shape[1:]
        (m * dout.double()).sum().backward()
        arrays[f"mask_{tag}"], arrays[f"grad_{tag}"] = m, x.grad
    A, B = O.synthetic_pairs(2, seed=465)
    arrays["mask_A_sub"] = L["mask_maker"](A.double())[:, :, ::4, ::4]
    arrays["mask_B_sub"] = L["mask_maker"](B.double())[:, :, ::4, ::4]
    save("mask_maker", g_keys=np.array(list(L["GeneratorUNet"]((3, 256, 256)).state_dict().keys())), **arrays)

    # (b) one training step, N = 2, twice from the same state
    def step(weight_mask):
        G3 = L["GeneratorUNet"]((3, 256, 256))
        D3 = L["Discriminator1"]((3, 256, 256))
        O.init_weights_portable(G3, seed=61)
        O.init_weights_portable(D3, seed=62)
        G3.eval()          # no dropout; InstanceNorm has no running stats so eval == train otherwise
        D3.train()         # spectral-norm power iteration on, as in training
        oG = torch.optim.Adam(G3.parameters(), lr=2e-4, betas=(0.5, 0.999))   # 4X:478
        oD = torch.optim.Adam(D3.parameters(), lr=2e-4, betas=(0.5, 0.999))   # 4X:479
        A3, B3 = O.synthetic_pairs(2, seed=465)
        B1, B2, B3_, B4 = four(B3)                                           # batch["B1"] .. ["B4"], 4X:543-546
        g_before = {k: v.clone() for k, v in G3.state_dict().items()}
        d_before = {k: v.clone() for k, v in D3.state_dict().items()}
        nidx = [3, 0, 2, 1]
        tp = lift(X4, ["triplet_patches"], extra={"np": types.SimpleNamespace(random=_Draws(nidx)), "triplet_loss": trip})
        tp["opt"].batch_size = 2
        mask_A = L["mask_maker"](A3)                                         # 4X:548
        oG.zero_grad()
        fake3 = G3(A3, mask_A)                                               # 4X:563
        pf = D3(fake3, A3)                                                   # 4X:567
        pr = D3(B3, A3)                                                      # 4X:568
        l_gan = bce(pf - pr.detach(), torch.full_like(pf, 0.9))              # 4X:569
        with cuda_is_identity():
            l_fft_script = L["fft_loss"](fake3.detach(), B1, B2, B3_, B4)    # 4X:572 (tensor -> PIL -> numpy: no gradient)
            cs = [(L["fft_components"](a.detach()), L["fft_components"](b)) for a, b in zip(four(fake3), four(B3))]
        l_amp = 0.25 * sum(l1(cf[0], cr[0]) for cf, cr in cs)                # the four-patch MEAN the package logs; 4X:335-336 sums
        l_pha = 0.25 * sum(l1(cf[1], cr[1]) for cf, cr in cs)
        l_fft = 1 / 2 * (l_amp + l_pha)
        assert abs(float(l_fft_script) - 4 * float(l_fft)) <= 1e-5 * float(l_fft_script)
        l_trip = tp["triplet_patches"](fake3, B1, B2, B3_, B4)               # 4X:575
        l_mask = l1(L["mask_maker"](fake3), L["mask_maker"](B3))             # 4X:584
        l_G = 0.5 * l_gan + 0.5 * l_trip + 0.001 * l_fft_script + weight_mask * l_mask     # 4X:587 without pix_g / temp_g
        l_G.backward()
        g_grad_down1 = G3.down1.model[0].weight.grad.clone()
        g_grad_up3 = G3.up3.model[0].weight.grad[::16, ::16].clone()
        oG.step()
        oD.zero_grad()
        pr2 = D3(B3, A3)                                                     # 4X:602
        pf2 = D3(fake3.detach(), A3)                                         # 4X:604
        l_D = 0.5 * (bce(pr2 - pf2, torch.full_like(pr2, 0.9)) + bce(pf2 - pr2, torch.zeros_like(pr2)))     # 4X:607-609
        l_D.backward()
        out = dict(neg_idx=np.array(nidx), loss_G=l_G, loss_GAN_g=l_gan, loss_triplet_patch=l_trip, loss_FFT=l_fft, loss_Amp=l_amp, loss_Pha=l_pha,
                   loss_FFT_script=l_fft_script, loss_mask=l_mask, loss_D=l_D, fake_sub=fake3[:, :, ::8, ::8],
                   d_grad_head=D3.model[13].weight.grad.clone(), d_grad_b0=D3.model[0].bias.grad.clone(),
                   d_grad_w3=D3.model[3].parametrizations.weight.original.grad[::8, ::8].clone())
        oD.step()
        out.update(d_delta_head=D3.state_dict()["model.13.weight"] - d_before["model.13.weight"],
                   d_u3=D3.state_dict()["model.3.parametrizations.weight.0._u"])
        if weight_mask == 0:
            out.update(g_grad_down1=g_grad_down1, g_grad_up3=g_grad_up3,
                       g_delta_final_w=G3.state_dict()["final.2.weight"] - g_before["final.2.weight"],
                       g_delta_down1=G3.state_dict()["down1.model.0.weight"] - g_before["down1.model.0.weight"])
        return out

    a, b = step(0.0), step(0.5)
    merged = dict(a)
    merged.update({"b_" + k: v for k, v in b.items() if k != "neg_idx"})
    save("train_step_mask4", **merged)


if __name__ == "__main__":
    main()
