"""Generate tests/golden/train_step_darkvisible.npz from the REFERENCE'S OWN definitions (runs only in the build container; helpers shared with
make_golden.py, which section (xiii) of it does the same for the STN21 script).

Lifted by `ast` from TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py ("DV") and executed on the CPU in fp32: the LIVE top-level definitions of UNetDown,
UNetUp, GeneratorUNet1 / 2, Discriminator1 / 2 (DV:370-423, the plain pix2pix PatchGAN; the spectral-norm pair at DV:427-486 sits inside a string
literal and is not a definition), LocalizerVIT, Net (DV:132-209: affine_grid(align_corners=True) + grid_sample(bicubic, border,
align_corners=False)), global_pixel_loss, global_gen_loss, global_disc_loss (DV:493-526), FFT_Components and fft_components (DV:529-569).
The batch-loop body DV:677-735 is INLINE in the script and is restated here line for line with those definitions.

Conditions, as for the STN21 fixture: N = 1, eval-mode dropout, oracle.init_weights_portable seeds 101..105 in the order G1, G2, D1, D2, Net, the last
localiser layer scaled up so that the warp is visible, lr 1e-4 (the script's default), perc_loss = 0 on both sides (lpips_pytorch and its weights are
absent). Stand-ins (make_golden.py header): antialiased_cnns.BlurPool -> oracle.BlurPool, K.VisionTransformer -> tfc_gan_amd.stn21.VisionTransformer.
The 257-token localiser's first Linear is 197 376 x 1024: about 5 GB of host memory with its gradient and Adam state.

No reference source text is written anywhere: only outputs are stored; inputs are regenerated from seeds.
Usage:  python tests/golden/make_golden_darkvisible.py        (writes next to this file)
"""
import itertools
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import O, cuda_is_identity, lift, save  # noqa: E402  (sets MKL_CBWR before torch starts MKL)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

DV = "/root/reference/TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py"
NAMES = ["UNetDown", "UNetUp", "GeneratorUNet1", "GeneratorUNet2", "Discriminator1", "Discriminator2", "LocalizerVIT", "Net", "global_pixel_loss",
         "global_gen_loss", "global_disc_loss", "FFT_Components", "fft_components"]
LR = 1e-4                                    # DV's --lr default


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    import tfc_gan_amd.stn21 as P21
    L = lift(DV, NAMES, extra={"K": types.SimpleNamespace(VisionTransformer=P21.VisionTransformer), "print": lambda *a, **k: None,
                               "criterion_GAN": nn.BCEWithLogitsLoss(), "criterion_L1": nn.L1Loss()})
    shp = (3, 256, 256)
    nets5 = {"G1": L["GeneratorUNet1"](shp), "G2": L["GeneratorUNet2"](shp), "D1": L["Discriminator1"](shp), "D2": L["Discriminator2"](shp),
             "net": L["Net"]()}
    for i, m in enumerate(nets5.values()):
        O.init_weights_portable(m, seed=101 + i)
    with torch.no_grad():                                          # a visible (still small) warp: scale the last localiser layer up
        nets5["net"].fc_loc[6].weight.mul_(4.0)
        nets5["net"].fc_loc[6].bias.copy_(torch.tensor([0.03, -0.02, 0.04, 0.02, -0.03, -0.05]))
    keep = {"G2.final": nets5["G2"].final[2].weight.detach().clone(), "net.fc6": nets5["net"].fc_loc[6].weight.detach().clone(),
            "D1.head": nets5["D1"].model[12].weight.detach().clone()}
    d_keys = list(nets5["D1"].state_dict().keys())
    assert d_keys == list(nets5["D2"].state_dict().keys())
    net_keys = list(nets5["net"].state_dict().keys())
    nets5["G1"].eval(); nets5["G2"].eval(); nets5["net"].eval(); nets5["D1"].train(); nets5["D2"].train()
    L["discriminator1"], L["discriminator2"] = nets5["D1"], nets5["D2"]
    L["valid"] = torch.full((1, 1, 16, 16), 0.9)                   # DV:670-672
    L["fake"] = torch.zeros((1, 1, 16, 16))
    A, B = O.synthetic_pairs(1, seed=105)
    oG = torch.optim.Adam(itertools.chain(nets5["G1"].parameters(), nets5["G2"].parameters(), nets5["net"].parameters()), lr=LR, betas=(0.5, 0.999))
    oD = torch.optim.Adam(itertools.chain(nets5["D1"].parameters(), nets5["D2"].parameters()), lr=LR, betas=(0.5, 0.999))
    # ---- DV:677-718 ----
    oG.zero_grad()
    with cuda_is_identity():
        fake_B = nets5["G1"](A)
        warped_B = nets5["net"](img_A=A, img_B=fake_B, src=B)
        fake_A = nets5["G2"](warped_B)
        recon = L["global_pixel_loss"](warped_B, fake_B)
        perc = torch.zeros(())                                     # LPIPS off on both sides
        amp_f, pha_f = L["fft_components"](fake_A)
        amp_r, pha_r = L["fft_components"](A)
        loss_fft = (L["criterion_amp"](amp_f, amp_r) + L["criterion_phase"](pha_f, pha_r)).mean()
        assert not loss_fft.requires_grad                          # through PIL and numpy: a value only
        gan1 = L["global_gen_loss"](A, B, fake_B, mode="B")
        gan2 = L["global_gen_loss"](A, B, fake_A, mode="A")
    gan = (gan1 + gan2).mean()
    loss_G = (gan + recon + perc + loss_fft).mean()
    loss_G.backward()
    net = nets5["net"]
    grads = {"g_G1_down1": nets5["G1"].down1.model[0].weight.grad.clone(), "g_G2_down1": nets5["G2"].down1.model[0].weight.grad.clone(),
             "g_fc6": net.fc_loc[6].weight.grad.clone(), "g_fc6_bias": net.fc_loc[6].bias.grad.clone(),
             "g_fc0": net.fc_loc[0].weight.grad[::64, ::256].clone()}
    oG.step()
    # ---- DV:725-734 ----
    oD.zero_grad()
    lD1 = L["global_disc_loss"](A, B, fake_img=fake_B, mode="B")
    lD2 = L["global_disc_loss"](A, B, fake_img=fake_A, mode="A")
    lD = 0.5 * (lD1 + lD2)
    lD.backward()
    D1, D2 = nets5["D1"], nets5["D2"]
    grads.update({"g_D1_head": D1.model[12].weight.grad.clone(), "g_D2_b0": D2.model[0].bias.grad.clone(),
                  "g_D2_w8": D2.model[8].weight.grad[::16, ::16].clone(),
                  "g_D2_b8": D2.model[8].bias.grad.clone(),             # a bias in front of InstanceNorm: rounding noise around zero
                  "g_D2_w8_absmax": D2.model[8].weight.grad.abs().max()})
    oD.step()
    save("train_step_darkvisible", loss_G=loss_G, loss_GAN=gan, recon_loss=recon, perc_loss=perc, loss_FFT=loss_fft, loss_D=lD, loss_D1=lD1, loss_D2=lD2,
         warped_sub=warped_B[:, :, ::8, ::8], fake_A_sub=fake_A[:, :, ::8, ::8], fake_B_sub=fake_B[:, :, ::8, ::8],
         d_G2_final=nets5["G2"].final[2].weight.detach() - keep["G2.final"], d_fc6=net.fc_loc[6].weight.detach() - keep["net.fc6"],
         d_D1_head=D1.model[12].weight.detach() - keep["D1.head"],
         d_keys=np.array(d_keys), net_keys=np.array(net_keys), **grads)


if __name__ == "__main__":
    main()
