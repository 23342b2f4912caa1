"""Generate the 4-patch fixtures tests/golden/{triplet4,fft_patch128,train_step_patch4,train_step_glo4}.npz from the REFERENCE'S OWN definitions
(runs only in the build container, like make_golden.py, whose `lift` / `cuda_is_identity` / `save` and stand-ins it uses).

Lifted by `ast`, executed on CPU fp32:
    TFCGAN_multigpu_patchFFT.py  ("4P", PATCH-4): FFT_Components, fft_components, sample_spectra, UNetDown, UNetUp, GeneratorUNet, Discriminator1
    TFCGAN_multigpu_globalFFT.py ("4G", GLO-4)  : FFT_Components, fft_components (whole image) and the same network classes
The 2x2 patch slicing, the four triplet terms and the step are INLINE in the reference's training loop (4P:458-541, 4G:454-530), so they are
restated here line for line with nn.TripletMarginLoss(margin=1.0, p=2) on torch CPU (cited below), as section (ix) of make_golden.py does for P16.

No reference source text is written anywhere: only outputs (and the negative indices) are stored; inputs are regenerated from seeds.
Usage:  python tests/golden/make_golden_patch4.py        (writes next to this file)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import O, cuda_is_identity, lift, save  # noqa: E402  (sets MKL_CBWR before torch starts MKL)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REF = "/root/reference/TFC-GAN-FFT"
P4 = os.path.join(REF, "TFCGAN_multigpu_patchFFT.py")
G4 = os.path.join(REF, "TFCGAN_multigpu_globalFFT.py")
NETS = ["UNetDown", "UNetUp", "GeneratorUNet", "Discriminator1"]


def four(x):
    """4P:468-471 (fake_B1..4; the dataset cuts B1..B4 the same way, datasets_temp_Patches.py)"""
    return (x[:, :, 0:0 + 256 // 2, 0:0 + 256 // 2], x[:, :, 0:0 + 256 // 2, 128:128 + 256 // 2],
            x[:, :, 128:128 + 256 // 2, 0:0 + 256 // 2], x[:, :, 128:128 + 256 // 2, 128:128 + 256 // 2])


def triplet4(trip, fake_B, real_B, neg):
    """4P:474-481 with the four np.random.randint(4) draws given as `neg`"""
    f, b = four(fake_B), four(real_B)
    random_patches = torch.stack(list(b))                                   # 4P:474
    terms = [trip(f[k], b[k], random_patches[neg[k]]) for k in range(4)]      # 4P:477-480
    return 0.25 * (terms[0] + terms[1] + terms[2] + terms[3]), terms          # 4P:481


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    R = lift(P4, NETS + ["FFT_Components", "fft_components", "sample_spectra"])
    R["opt"].patch_height = R["opt"].patch_width = 128                       # 4P: --patch_height 128
    RG = lift(G4, NETS + ["FFT_Components", "fft_components"])
    trip = nn.TripletMarginLoss(margin=1.0, p=2)                             # 4P:74 triplet_loss
    bce = nn.BCEWithLogitsLoss()                                             # 4P:67 criterion_GAN
    l1 = nn.L1Loss()                                                         # 4P:82-83 criterion_amp / criterion_phase

    # (a) triplet head at N = 3 (and on sample 0 alone): r_k == k at k = 1
    fk, rl = O.synthetic_pairs(3, seed=431)
    fk = torch.tanh(fk * 1.5)
    neg = [2, 1, 0, 2]
    f3 = fk.clone().requires_grad_(True)
    total3, per3 = triplet4(trip, f3, rl, neg)
    total3.backward()
    f1 = fk[:1].clone().requires_grad_(True)
    total1, _ = triplet4(trip, f1, rl[:1], neg)
    total1.backward()
    save("triplet4", neg_idx=np.array(neg), loss_n3=total3, per_patch_n3=torch.stack(per3), gfake_sub_n3=f3.grad[:, :, ::4, ::4],
         gfake_absmean_n3=f3.grad.abs().mean(), loss_n1=total1, gfake_sub_n1=f1.grad[:, :, ::4, ::4])

    # (b) FFT head: lifted fft_components on a 128 x 128 patch (values incl. negatives: uint8 wrap-around), the 4-patch loss composed as
    # 4P:499-511, and the lifted sample_spectra on 128 x 128 tensors
    ff, rr = O.synthetic_pairs(1, seed=441)
    ff = torch.tanh(ff * 2.0) * 0.999
    with cuda_is_identity():
        amp, pha = R["fft_components"](four(ff)[2])
        comps = [(R["fft_components"](a), R["fft_components"](b)) for a, b in zip(four(ff), four(rr))]
    loss_amp = 0.25 * sum(l1(cf[0], cr[0]) for cf, cr in comps)              # 4P:509
    loss_pha = 0.25 * sum(l1(cf[1], cr[1]) for cf, cr in comps)              # 4P:510
    loss_fft = 1 / 2 * (loss_amp + loss_pha)                                 # 4P:511
    sp_in, _ = O.synthetic_pairs(2, seed=481)
    sp_in = (torch.tanh(sp_in * 1.2) * 0.999 + 1e-3)[:, :, 128:, :128]       # patch 2 of two images; no all-zero spectrum bins
    R["opt"].img_height = R["opt"].img_width = 128                           # sample_spectra reshapes to (N, 1, img_height, img_width), 4P:300
    with cuda_is_identity():
        spec = R["sample_spectra"](sp_in)
    R["opt"].img_height = R["opt"].img_width = 256
    save("fft_patch128", amp2=amp, pha2=pha, loss_fft=loss_fft, loss_amp=loss_amp, loss_pha=loss_pha, spec_sub=spec[:, :, ::4, ::4],
         spec_mean=spec.mean(), spec_row7=spec[1, 0, 7, :])

    # (c) one training step of each script (4P:455-541 / 4G:454-530 minus LPIPS and the temperature head), N = 1, eval-mode dropout
    def step(L, tag, seed, global_fft):
        G3 = L["GeneratorUNet"]((3, 256, 256))
        D3 = L["Discriminator1"]((3, 256, 256))
        O.init_weights_portable(G3, seed=61)
        O.init_weights_portable(D3, seed=62)
        G3.eval()          # no dropout; InstanceNorm has no running stats so eval == train otherwise
        D3.train()         # spectral-norm power iteration on, as in training
        oG = torch.optim.Adam(G3.parameters(), lr=2e-4, betas=(0.5, 0.999))
        oD = torch.optim.Adam(D3.parameters(), lr=2e-4, betas=(0.5, 0.999))
        A3, B3 = O.synthetic_pairs(1, seed=seed)
        g_before = {k: v.clone() for k, v in G3.state_dict().items()}
        d_before = {k: v.clone() for k, v in D3.state_dict().items()}
        nidx = [3, 0, 2, 1]                                                  # r_k == k at k = 2
        oG.zero_grad()
        fake3 = G3(A3)                                                       # 4P:458
        pf = D3(fake3, A3)                                                   # 4P:462
        pr = D3(B3, A3)                                                      # 4P:463
        l_gan = bce(pf - pr.detach(), torch.full_like(pf, 0.9))              # 4P:464
        l_trip, _ = triplet4(trip, fake3, B3, nidx)                          # 4P:468-481
        with cuda_is_identity():
            if global_fft:                                                   # 4G:495-499
                af, phf = L["fft_components"](fake3.detach())
                ar, phr = L["fft_components"](B3)
                l_amp, l_pha = l1(af, ar), l1(phf, phr)
            else:                                                            # 4P:499-510
                cs = [(L["fft_components"](a.detach()), L["fft_components"](b)) for a, b in zip(four(fake3), four(B3))]
                l_amp = 0.25 * sum(l1(cf[0], cr[0]) for cf, cr in cs)
                l_pha = 0.25 * sum(l1(cf[1], cr[1]) for cf, cr in cs)
        l_fft = 1 / 2 * (l_amp + l_pha)                                      # 4P:511
        l_G = 0.5 * l_gan + l_trip + 1 / 100 * l_fft                         # 4P:515 without pix_g / temp_g
        l_G.backward()
        g_grad_down1 = G3.down1.model[0].weight.grad.clone()
        g_grad_up3 = G3.up3.model[0].weight.grad[::16, ::16].clone()
        oG.step()
        oD.zero_grad()
        pr2 = D3(B3, A3)                                                     # 4P:530
        pf2 = D3(fake3.detach(), A3)                                         # 4P:532
        l_D = 0.5 * (bce(pr2 - pf2, torch.full_like(pr2, 0.9)) + bce(pf2 - pr2, torch.zeros_like(pr2)))     # 4P:535-537
        l_D.backward()
        d_grad_head = D3.model[13].weight.grad.clone()
        d_grad_b0 = D3.model[0].bias.grad.clone()
        d_grad_w3 = D3.model[3].parametrizations.weight.original.grad[::8, ::8].clone()
        oD.step()
        save(tag, neg_idx=np.array(nidx), loss_G=l_G, loss_GAN_g=l_gan, loss_triplet_patch=l_trip, loss_FFT=l_fft, loss_Amp=l_amp,
             loss_Pha=l_pha, loss_D=l_D, fake_sub=fake3[:, :, ::8, ::8], g_grad_down1=g_grad_down1, g_grad_up3=g_grad_up3,
             d_grad_head=d_grad_head, d_grad_b0=d_grad_b0, d_grad_w3=d_grad_w3,
             g_delta_final_w=G3.state_dict()["final.2.weight"] - g_before["final.2.weight"],
             g_delta_down1=G3.state_dict()["down1.model.0.weight"] - g_before["down1.model.0.weight"],
             d_delta_head=D3.state_dict()["model.13.weight"] - d_before["model.13.weight"],
             d_u3=D3.state_dict()["model.3.parametrizations.weight.0._u"])

    R["opt"].batch_size = RG["opt"].batch_size = 1
    step(R, "train_step_patch4", 465, False)
    step(RG, "train_step_glo4", 466, True)


if __name__ == "__main__":
    main()
