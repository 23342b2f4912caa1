"""Torch restatements for the DarkVisible tests (host and GPU): the plain pix2pix PatchGAN from torch ops, its bf16-storage variant in the style of
the oracle's (a round-to-bf16 at exactly the points where nets.Pix2PixCore stores a bf16 tensor, fp32 arithmetic in between), and the mixed-mode warp,
which is literally torch's two calls."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import tfcgan_oracle as O

BLOCKS = ((0, False), (2, True), (5, True), (8, True))     # (index in nn.Sequential, InstanceNorm2d)
HEAD = 12


class Pix2PixRef(nn.Module):
    """four blocks Conv2d(k4, s2, p1, bias) -> [InstanceNorm2d, not the first] -> LeakyReLU(0.2); ZeroPad2d((1, 0, 1, 0)) + Conv2d(512, 1, 4, p1, no bias).
    The convolutions live in `model` at the indices of the usual nn.Sequential layout, so the state_dict keys are model.{0,2,5,8}.{weight,bias} and
    model.12.weight; forward() is written out with functional ops."""

    def __init__(self, channels=3):
        super().__init__()
        layers = [nn.Identity() for _ in range(HEAD + 1)]
        cin = 2 * channels
        for (i, _), cout in zip(BLOCKS, (64, 128, 256, 512)):
            layers[i] = nn.Conv2d(cin, cout, 4, stride=2, padding=1)
            cin = cout
        layers[HEAD] = nn.Conv2d(512, 1, 4, padding=1, bias=False)
        self.model = nn.Sequential(*layers)

    def forward(self, img_A, img_B):
        h = torch.cat((img_A, img_B), 1)
        for i, norm in BLOCKS:
            m = self.model[i]
            h = F.conv2d(h, m.weight, m.bias, stride=2, padding=1)
            if norm:
                h = F.instance_norm(h, eps=1e-5)
            h = F.leaky_relu(h, 0.2)
        return F.conv2d(F.pad(h, (1, 0, 1, 0)), self.model[HEAD].weight, padding=1)


def forward_bf16(D, img_A, img_B):
    """Pix2PixRef.forward with the engine's bf16 storage points: the packed input (value and gradient), the packed weights, block 1's ACTIVATED output
    (its pre-activation is never stored, the gradient of it is), the raw convolution outputs of blocks 2-4 and their normalised + activated outputs
    (values and gradients), the logits; the head kernel reads fp32 weights"""
    rb, rw, rg = O._RoundBoth.apply, O._RoundFwd.apply, O._RoundBwd.apply
    h = torch.cat((rb(img_A), O._bf(img_B)), 1)
    for i, norm in BLOCKS:
        m = D.model[i]
        z = F.conv2d(h, rw(m.weight), m.bias, stride=2, padding=1)
        if norm:
            h = rb(F.leaky_relu(F.instance_norm(rb(z), eps=1e-5), 0.2))
        else:
            h = rb(F.leaky_relu(rg(z), 0.2))
    return rb(F.conv2d(F.pad(h, (1, 0, 1, 0)), D.model[HEAD].weight, padding=1))


def mixed_warp(src, theta, sample_align_corners=False):
    """per sample F.affine_grid(align_corners=True) + F.grid_sample(bicubic, border, align_corners=sample_align_corners)"""
    outs = []
    for i in range(src.shape[0]):
        grid = F.affine_grid(theta[i:i + 1], src[i:i + 1].size(), align_corners=True)
        outs.append(F.grid_sample(src[i:i + 1], grid, mode="bicubic", padding_mode="border", align_corners=sample_align_corners))
    return torch.cat(outs)
