"""Generate the regional-FFT fixtures tests/golden/{fft_region,train_step_region_l1,train_step_region_kl}.npz from the REFERENCE'S OWN definitions
(runs only in the build container, like make_golden.py, whose `lift` / `cuda_is_identity` / `save` and stand-ins it uses).

Lifted by `ast`, executed on CPU fp32:
    TFCGAN_multigpu_patchFFT_withregion_FFT.py    ("4R"): FFT_Components, fft_components, fft_loss, regional_fft_loss and the network classes
    TFCGAN_multigpu_patchFFT_withregion_FFT_KL.py ("4K"): the same names; its criterion_amp_R / criterion_phase_R (nn.KLDivLoss(reduction="mean",
                                                          log_target=True), 4K:84-85) and criterion_amp_P / criterion_phase_P (nn.L1Loss, 4K:86-87)
                                                          are handed to `lift` through extra=
The lifted regional_fft_loss returns the total only, so its parts are composed here, per window, from the function's own nested reg_fft (lifted out
of its body) and the lifted criteria, and the composed total is checked against the lifted function's. The step is inline in the training loop
(4R:594-642, 4K:611-658) and restated statement by statement under this file's own names, as make_golden_patch4.py does for 4P.

No reference source text is written anywhere: only outputs (and the negative indices) are stored; inputs are regenerated from seeds.
Usage:  python tests/golden/make_golden_region.py        (writes next to this file)
"""
import ast
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, O, cuda_is_identity, lift, save  # noqa: E402  (sets MKL_CBWR before torch starts MKL)
from make_golden_patch4 import four, triplet4  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

R4 = os.path.join(REF, "TFCGAN_multigpu_patchFFT_withregion_FFT.py")
K4 = os.path.join(REF, "TFCGAN_multigpu_patchFFT_withregion_FFT_KL.py")
NETS = ["UNetDown", "UNetUp", "GeneratorUNet", "Discriminator1"]
HEADS = ["FFT_Components", "fft_components", "regional_fft_loss", "fft_loss"]


def lift_reg_fft(path, ns):
    """the nested reg_fft of regional_fft_loss (4R:358-371, 4K:362-375), compiled into the namespace the lifted module-level names live in"""
    tree = ast.parse(open(path).read())
    outer = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "regional_fft_loss"]
    inner = [n for n in outer[0].body if isinstance(n, ast.FunctionDef) and n.name == "reg_fft"]
    assert len(outer) == 1 and len(inner) == 1
    exec(compile(ast.Module(body=inner, type_ignores=[]), path, "exec"), ns)
    return ns["reg_fft"]


ROWS = {"hair": (0, 100), "eyes": (100, 100)}          # (first row, row count) of the two windows: 4R:375-376 / 4K:379-380, all 256 columns


def window(x, name):
    """the rows of one named window of x [N,3,256,256], as a view"""
    row0, h = ROWS[name]
    return x.narrow(2, row0, h)


def parts(L, reg_fft, kl, fake_B, real_B):
    """(loss_FFT_reg, loss_Amp_reg, loss_Pha_reg): the parts the reference adds up in 4R:384-399 (kl False) / 4K:388-418 (kl True), composed per
    window from the lifted reg_fft and the lifted criteria. Each part is the hair term plus the eyes term, in that order, so the total has the bits of
    the lifted function's (main() asserts it).
    kl: every spectrum goes through log_softmax over dim 0, the batch; the target of the PHASE term is the log-softmaxed real AMPLITUDE, because the
    reference takes both targets from the real amplitudes (4K:401, :404). The real phases are computed and unused."""
    crit_amp, crit_pha = (L["criterion_amp_R"], L["criterion_phase_R"]) if kl else (L["criterion_amp"], L["criterion_phase"])
    loss_amp = loss_pha = None
    for name in ("hair", "eyes"):
        amp_fake, pha_fake = reg_fft(window(fake_B, name))
        amp_real, pha_real = reg_fft(window(real_B, name))
        if kl:
            amp_fake, pha_fake = F.log_softmax(amp_fake, dim=0), F.log_softmax(pha_fake, dim=0)
            amp_real = pha_real = F.log_softmax(amp_real, dim=0)
        term_amp, term_pha = crit_amp(amp_fake, amp_real), crit_pha(pha_fake, pha_real)
        loss_amp = term_amp if loss_amp is None else loss_amp + term_amp
        loss_pha = term_pha if loss_pha is None else loss_pha + term_pha
    return 0.5 * (loss_amp + loss_pha), loss_amp, loss_pha


def head_inputs(n):
    x, real = O.synthetic_pairs(n, seed=501)
    return torch.tanh(x * 1.5) * 0.999, real


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    kl_extra = {"criterion_amp_R": nn.KLDivLoss(reduction="mean", log_target=True),           # 4K:84
                "criterion_phase_R": nn.KLDivLoss(reduction="mean", log_target=True),         # 4K:85
                "criterion_amp_P": nn.L1Loss(), "criterion_phase_P": nn.L1Loss()}             # 4K:86-87
    LR = lift(R4, NETS + HEADS)
    LK = lift(K4, NETS + HEADS, extra=kl_extra)
    for L in (LR, LK):
        L["opt"].patch_height = L["opt"].patch_width = 128
    reg_r, reg_k = lift_reg_fft(R4, LR), lift_reg_fft(K4, LK)

    # (a) the head: spectra of the "eyes" region of sample 0, the L1 form at N = 1, 3 and the KL form at N = 1, 2, 3
    rec = {}
    for n in (1, 2, 3):
        fake, real = head_inputs(n)
        LR["opt"].batch_size = LK["opt"].batch_size = n
        with cuda_is_identity():
            if n == 1:
                amp, pha = reg_r(window(fake, "eyes"))
                rec.update(amp_eyes0=amp[0, 0], pha_eyes0=pha[0, 0])
            for tag, L, reg, kl in (("l1", LR, reg_r, False), ("kl", LK, reg_k, True)):
                if tag == "l1" and n == 2:
                    continue
                total = L["regional_fft_loss"](fake, real)
                got = parts(L, reg, kl, fake, real)
                assert torch.equal(total, got[0]), (tag, n, total, got[0])
                rec[f"{tag}_n{n}"] = torch.stack(got)
                print(f"  {tag} N={n}: lifted {float(total):.7g}  amp {float(got[1]):.7g}  pha {float(got[2]):.7g}")
    save("fft_region", **rec)

    # (b) one training step of each script at N = 2 (the KL term vanishes at N = 1), minus LPIPS and the temperature head, eval-mode dropout
    trip = nn.TripletMarginLoss(margin=1.0, p=2)                             # 4R:74 triplet_loss
    bce = nn.BCEWithLogitsLoss()                                             # 4R:67 criterion_GAN

    def step(L, reg, tag, seed, kl):
        L["opt"].batch_size = 2
        G3 = L["GeneratorUNet"]((3, 256, 256))
        D3 = L["Discriminator1"]((3, 256, 256))
        O.init_weights_portable(G3, seed=61)
        O.init_weights_portable(D3, seed=62)
        G3.eval()          # no dropout; InstanceNorm has no running stats so eval == train otherwise
        D3.train()         # spectral-norm power iteration on, as in training
        oG = torch.optim.Adam(G3.parameters(), lr=2e-4, betas=(0.5, 0.999))
        oD = torch.optim.Adam(D3.parameters(), lr=2e-4, betas=(0.5, 0.999))
        A3, B3 = O.synthetic_pairs(2, seed=seed)
        g_before = {k: v.clone() for k, v in G3.state_dict().items()}
        d_before = {k: v.clone() for k, v in D3.state_dict().items()}
        nidx = [1, 3, 2, 0]                                                  # r_k == k at k = 2
        oG.zero_grad()
        fake3 = G3(A3)                                                       # 4R:595
        pf = D3(fake3, A3)                                                   # 4R:598
        pr = D3(B3, A3)                                                      # 4R:599
        l_gan = bce(pf - pr.detach(), torch.full_like(pf, 0.9))              # 4R:600
        with cuda_is_identity():
            fft_sum = L["fft_loss"](fake3.detach(), *four(B3))               # 4R:603 / 4K:620: the SUM over the four patches (4R:315-317)
            l_reg, l_amp_reg, l_pha_reg = parts(L, reg, kl, fake3.detach(), B3)
            assert torch.equal(l_reg, L["regional_fft_loss"](fake3.detach(), B3))
        l_trip, _ = triplet4(trip, fake3, B3, nidx)                          # 4R:609 triplet_patches with the four draws given
        if kl:
            loss_FFT_reg = 0.01 * l_reg                                      # 4K:623
            l_G = 1 / 2 * (l_gan + 0.0001 * loss_FFT_reg + l_trip)           # 4K:636 without temp_g / pix_g (loss_FFT = 0.001 * fft_loss is logged only)
        else:
            loss_FFT = 0.0001 * fft_sum                                      # 4R:603
            loss_FFT_reg = 0.0001 * l_reg                                    # 4R:606
            l_G = 1 / 2 * (l_gan + loss_FFT + loss_FFT_reg + l_trip)         # 4R:620 without temp_g / pix_g
        l_G.backward()
        g_grad_down1 = G3.down1.model[0].weight.grad.clone()
        g_grad_up3 = G3.up3.model[0].weight.grad[::16, ::16].clone()
        oG.step()
        oD.zero_grad()
        pr2 = D3(B3, A3)                                                     # 4R:635
        pf2 = D3(fake3.detach(), A3)                                         # 4R:637
        l_D = 0.5 * (bce(pr2 - pf2, torch.full_like(pr2, 0.9)) + bce(pf2 - pr2, torch.zeros_like(pr2)))     # 4R:640-642
        l_D.backward()
        d_grad_head = D3.model[13].weight.grad.clone()
        d_grad_b0 = D3.model[0].bias.grad.clone()
        d_grad_w3 = D3.model[3].parametrizations.weight.original.grad[::8, ::8].clone()
        oD.step()
        # loss_FFT: the MEAN over the four patches (what patch_fft_loss / TrainStep log); fft_loss_sum: the script's own value
        save(tag, neg_idx=np.array(nidx), loss_G=l_G, loss_GAN_g=l_gan, loss_triplet_patch=l_trip, loss_FFT=fft_sum / 4, fft_loss_sum=fft_sum,
             loss_FFT_reg=l_reg, loss_Amp_reg=l_amp_reg, loss_Pha_reg=l_pha_reg, loss_D=l_D, fake_sub=fake3[:, :, ::8, ::8],
             g_grad_down1=g_grad_down1, g_grad_up3=g_grad_up3, d_grad_head=d_grad_head, d_grad_b0=d_grad_b0, d_grad_w3=d_grad_w3,
             g_delta_final_w=G3.state_dict()["final.2.weight"] - g_before["final.2.weight"],
             g_delta_down1=G3.state_dict()["down1.model.0.weight"] - g_before["down1.model.0.weight"],
             d_delta_head=D3.state_dict()["model.13.weight"] - d_before["model.13.weight"],
             d_u3=D3.state_dict()["model.3.parametrizations.weight.0._u"])

    step(LR, reg_r, "train_step_region_l1", 511, False)
    step(LK, reg_k, "train_step_region_kl", 512, True)


if __name__ == "__main__":
    main()
