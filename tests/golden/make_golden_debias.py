"""Generate the fixtures of the label-conditioned ("debiased") 4-patch scripts, tests/golden/{debias_heads,train_step_debias_v1,train_step_debias_v3}.npz,
from the REFERENCE'S OWN definitions (runs only in the build container, like make_golden_patch4.py, whose helpers it shares).

Lifted by `ast`, executed on the CPU (the steps in fp32, the heads-only fixture in fp64), from TFCGAN_multigpu_patchFFT_debiased.py ("DB1"): UNetDown, UNetUp, GeneratorUNet (fc + 4-channel down1,
DB1:142-186), Discriminator1 (three Linear + Softmax heads, DB1:194-233) and fft_components / FFT_Components. ..._debiased_V2.py ("DB2") and
..._debiased_V3.py ("DB3") define the same classes; what differs is the training loop, which is INLINE in all three scripts and therefore restated
here line for line with the reference's own criteria (cited below): v1 = DB1:498-613, v3 = DB3:498-629 (DB2 is DB3 with unit label weights).
LPIPS (needs VGG weights) and the temperature head (zero gradient) are left out, as in every other step fixture.

Conditions: N = 2 (label_formatter takes its squeeze_() branch, DB1:251-254), G.eval() / D.train(), init_weights_portable(G, 61) / (D, 62) with
the three head weights multiplied by 0.1: at the initialiser's std 0.02 the 393,216-term logits spread by ~6, the first softmax saturates and the
gradient through it underflows -- a fixture that would test nothing. With the factor every probability lies in (0.02, 0.98) (asserted below).

No reference source text is written anywhere: only outputs are stored; inputs are regenerated from seeds.
Usage:  python tests/golden/make_golden_debias.py        (writes next to this file)
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import O, cuda_is_identity, lift, save  # noqa: E402  (sets MKL_CBWR before torch starts MKL)
from make_golden_patch4 import four, triplet4  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REF = "/root/reference/TFC-GAN-FFT"
DB1 = os.path.join(REF, "TFCGAN_multigpu_patchFFT_debiased.py")
NETS = ["UNetDown", "UNetUp", "GeneratorUNet", "Discriminator1"]
LABELS = [[1, 3, 2], [0, 1, 0]]          # real labels: gender, ethnicity, age
GEN_LABELS = [[0, 2, 1], [1, 0, 2]]      # the step's np.random.randint draws (DB1:504-506), fixed
HEADS = ("aux_gender", "aux_ethn", "aux_age")


def label_formatter(labels):
    """DB1:249-261 at opt.batch_size > 1 (the .to(device='cuda') is a no-op here)"""
    return labels.type(torch.LongTensor).squeeze_()


def build(L):
    G = L["GeneratorUNet"]((3, 256, 256))
    D = L["Discriminator1"]((3, 256, 256))
    O.init_weights_portable(G, seed=61)
    O.init_weights_portable(D, seed=62)
    with torch.no_grad():
        for h in HEADS:
            getattr(D, h)[0].weight.mul_(0.1)
    G.eval()           # no dropout; InstanceNorm has no running stats so eval == train otherwise
    D.train()          # spectral-norm power iteration on, as in training
    return G, D


def check_probs(*ps):
    for p in ps:
        p = p.detach()
        assert float(p.min()) > 0.02 and float(p.max()) < 0.98, (float(p.min()), float(p.max()))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    warnings.filterwarnings("ignore", message="Implicit dimension choice for softmax")     # nn.Softmax() without dim, DB1:218-220
    L = lift(DB1, NETS + ["FFT_Components", "fft_components"])
    L["opt"].patch_height = L["opt"].patch_width = 128
    L["opt"].batch_size = 2
    trip = nn.TripletMarginLoss(margin=1.0, p=2)                             # DB1:81 triplet_loss
    bce = nn.BCEWithLogitsLoss()                                             # DB1:68 criterion_GAN
    ce = nn.CrossEntropyLoss()                                               # DB1:71 criterion_label
    l1 = nn.L1Loss()                                                         # DB1:88-89 criterion_amp / criterion_phase
    labels = torch.tensor(LABELS, dtype=torch.float32)                       # batch["LAB"], DB1:482
    gen_labels = torch.tensor(GEN_LABELS, dtype=torch.float32)               # DB1:504-507

    # (a) the heads and the label plane alone: D's heads on (B, A), the double-softmax cross entropy and its gradients; fc of the labels.
    # The lifted modules are evaluated in DOUBLE here (module.double(), double inputs): an fp32 sum of 393,216 products leaves ~5e-6 on a logit and
    # ~2.6e-6 (relative) on a probability, above the 1e-6 the fp64 restatement tests/debias_ref.py is held to. Same definitions, exact arithmetic.
    G, D = build(L)
    G, D = G.double(), D.double()
    A, B = (v.double() for v in O.synthetic_pairs(2, seed=465))
    Bq = B.clone().requires_grad_(True)
    _, gh, eh, ah = D(Bq, A)                                                 # DB1:588
    check_probs(gh, eh, ah)
    assert gh.dtype == torch.float64
    tg, te, ta = (label_formatter(labels[:, k]) for k in range(3))           # DB1:599-601
    terms = [ce(gh, tg), ce(eh, te), ce(ah, ta)]                             # DB1:603
    (terms[0] + terms[1] + terms[2]).backward()
    plane = G.fc(labels.double()).view(2, 1, 256, 256)                       # DB1:173
    save("debias_heads", g_keys=np.array(list(G.state_dict().keys())), d_keys=np.array(list(D.state_dict().keys())),
         labels=np.array(LABELS), gender_hat=gh, ethn_hat=eh, age_hat=ah, ce_terms=torch.stack(terms),
         g_input_sub=Bq.grad[:, :, ::8, ::8], g_ethn_w_sub=D.aux_ethn[0].weight.grad[:, ::997], g_gender_b=D.aux_gender[0].bias.grad,
         g_ethn_b=D.aux_ethn[0].bias.grad, g_age_b=D.aux_age[0].bias.grad, plane_sub=plane[:, 0, ::8, ::8])

    # (b) one training step of v1 (DB1) and v3 (DB3), N = 2
    def step(tag, kind):
        G3, D3 = build(L)
        oG = torch.optim.Adam(G3.parameters(), lr=2e-4, betas=(0.5, 0.999))   # DB1:414
        oD = torch.optim.Adam(D3.parameters(), lr=2e-4, betas=(0.5, 0.999))   # DB1:415
        A3, B3 = O.synthetic_pairs(2, seed=465)
        g_before = {k: v.clone() for k, v in G3.state_dict().items()}
        d_before = {k: v.clone() for k, v in D3.state_dict().items()}
        nidx = [3, 0, 2, 1]
        gen_gender, gen_ethn, gen_age = (gen_labels[:, k:k + 1] for k in range(3))      # DB1:504-506
        gender, ethn, age = (label_formatter(labels[:, k]) for k in range(3))           # DB3:519-521 / DB1:599-601
        oG.zero_grad()
        if kind == "v1":
            fake3 = G3(A3, gen_labels)                                       # DB1:508
        else:
            fake3 = G3(A3, labels)                                           # DB3:512
        pf, gen_f, eth_f, age_f = D3(fake3, A3)                              # DB1:512
        pr, _, _, _ = D3(B3, A3)                                             # DB1:513
        check_probs(gen_f, eth_f, age_f)
        l_gan = bce(pf - pr.detach(), torch.full_like(pf, 0.9))              # DB1:514
        gg, ge, ga = label_formatter(gen_gender.clone()), label_formatter(gen_ethn.clone()), label_formatter(gen_age.clone())   # DB1:518-521
        if kind == "v1":
            l_label = ce(gen_f, gg) + ce(eth_f, ge) + ce(age_f, ga)          # DB1:522
        else:
            l_label = ce(gen_f, gender) + 10 * ce(eth_f, ethn) + ce(age_f, age)          # DB3:531
        l_trip, _ = triplet4(trip, fake3, B3, nidx)                          # DB1:526-539
        with cuda_is_identity():
            cs = [(L["fft_components"](a.detach()), L["fft_components"](b)) for a, b in zip(four(fake3), four(B3))]      # DB1:556-564
        l_amp = 0.25 * sum(l1(cf[0], cr[0]) for cf, cr in cs)                # DB1:566
        l_pha = 0.25 * sum(l1(cf[1], cr[1]) for cf, cr in cs)                # DB1:567
        l_fft = 1 / 2 * (l_amp + l_pha)                                      # DB1:568
        if kind == "v1":
            l_G = l_gan + l_trip + l_label + 0.001 * l_fft                   # DB1:572 without pix_g / temp_g
        else:
            l_G = l_gan + l_label + 0.001 * l_fft                            # DB3:583 without pix_g / temp_g
        l_G.backward()
        g_grad_down1 = G3.down1.model[0].weight.grad.clone()
        g_grad_up3 = G3.up3.model[0].weight.grad[::16, ::16].clone()
        g_grad_fc_w = G3.fc.weight.grad[::61].clone()
        g_grad_fc_b = G3.fc.bias.grad[::61].clone()
        oG.step()
        oD.zero_grad()
        pr2, prg, pre, pra = D3(B3, A3)                                      # DB1:588
        pf2, pfg, pfe, pfa = D3(fake3.detach(), A3)                          # DB1:591
        check_probs(prg, pre, pra, pfg, pfe, pfa)
        l_real = bce(pr2 - pf2, torch.full_like(pr2, 0.9))                   # DB1:594
        l_fake = bce(pf2 - pr2, torch.zeros_like(pr2))                       # DB1:595
        if kind == "v1":
            real_ll = ce(prg, gender) + ce(pre, ethn) + ce(pra, age)         # DB1:603
            fake_ll = ce(pfg, gg) + ce(pfe, ge) + ce(pfa, ga)                # DB1:606
        else:
            real_ll = 1 / 3 * (ce(prg, gender) + ce(pre, ethn) + ce(pra, age))            # DB3:612
            fake_ll = 1 / 3 * (ce(pfg, gg) + ce(pfe, ge) + ce(pfa, ga))      # DB3:618
        l_D = 1 / 2 * ((l_real + real_ll) + (l_fake + fake_ll))              # DB1:609
        l_D.backward()
        d_grad_head = D3.model[13].weight.grad.clone()
        d_grad_b0 = D3.model[0].bias.grad.clone()
        d_grad_w3 = D3.model[3].parametrizations.weight.original.grad[::8, ::8].clone()
        d_grad_ethn_w = D3.aux_ethn[0].weight.grad[:, ::997].clone()
        d_grad_aux_b = torch.cat([getattr(D3, h)[0].bias.grad for h in HEADS])
        oD.step()
        save(tag, neg_idx=np.array(nidx), labels=np.array(LABELS), gen_labels=np.array(GEN_LABELS),
             loss_G=l_G, loss_GAN_g=l_gan, loss_triplet_patch=l_trip, loss_FFT=l_fft, loss_Amp=l_amp, loss_Pha=l_pha, loss_label=l_label,
             loss_D=l_D, real_loss_label=real_ll, fake_loss_label=fake_ll, fake_probs=torch.cat([gen_f, eth_f, age_f], 1),
             d_real_probs=torch.cat([prg, pre, pra], 1), d_fake_probs=torch.cat([pfg, pfe, pfa], 1),
             fake_sub=fake3[:, :, ::8, ::8], g_grad_down1=g_grad_down1, g_grad_up3=g_grad_up3, g_grad_fc_w=g_grad_fc_w, g_grad_fc_b=g_grad_fc_b,
             d_grad_head=d_grad_head, d_grad_b0=d_grad_b0, d_grad_w3=d_grad_w3, d_grad_ethn_w=d_grad_ethn_w, d_grad_aux_b=d_grad_aux_b,
             g_delta_final_w=G3.state_dict()["final.2.weight"] - g_before["final.2.weight"],
             g_delta_down1=G3.state_dict()["down1.model.0.weight"] - g_before["down1.model.0.weight"],
             g_delta_fc_b=(G3.state_dict()["fc.bias"] - g_before["fc.bias"])[::61],
             d_delta_head=D3.state_dict()["model.13.weight"] - d_before["model.13.weight"],
             d_delta_gender_w=(D3.state_dict()["aux_gender.0.weight"] - d_before["aux_gender.0.weight"])[:, ::997],
             d_u3=D3.state_dict()["model.3.parametrizations.weight.0._u"])

    step("train_step_debias_v1", "v1")
    step("train_step_debias_v3", "v3")


if __name__ == "__main__":
    main()
