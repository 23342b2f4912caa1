"""Host tests of the STN21 localiser switch (Net(localiser=...), TFC_LOCALISER): the knob's values, its default, the refusal of CPU tensors by the
HIP path, and the "torch" path staying the plain torch-layer composition it was (tests/golden/make_golden.py uses it as kornia's stand-in)."""
import pytest
import torch

import tfc_gan_amd as T
from tfc_gan_amd import stn21


def test_localiser_knob_values(monkeypatch):
    monkeypatch.delenv("TFC_LOCALISER", raising=False)
    assert stn21.Net((3, 128, 128)).localiser == "torch"                  # the default stays the torch layers
    assert stn21.Net((3, 128, 128), localiser="hip").localiser == "hip"
    monkeypatch.setenv("TFC_LOCALISER", "hip")
    net = stn21.Net((3, 128, 128))
    assert net.localiser == "hip"
    assert stn21.Net((3, 128, 128), localiser="torch").localiser == "torch"  # an explicit argument wins over the environment
    net.localiser = "torch"
    assert net.localiser == "torch"
    with pytest.raises(ValueError):
        net.localiser = "cuda"
    assert net.localiser == "torch"
    monkeypatch.setenv("TFC_LOCALISER", "bogus")
    with pytest.raises(ValueError):
        stn21.Net((3, 128, 128))
    with pytest.raises(ValueError):
        stn21.Net((3, 128, 128), localiser="HIP")


def test_localiser_state_dict_unchanged_by_the_knob():
    torch.manual_seed(0)
    a = stn21.Net((3, 128, 128), localiser="torch")
    b = stn21.Net((3, 128, 128), localiser="hip")
    assert list(a.state_dict()) == list(b.state_dict())
    assert "localiser" not in " ".join(a.state_dict())


def test_hip_localiser_refuses_cpu_tensors():
    torch.manual_seed(1)
    net = stn21.Net((3, 128, 128), localiser="hip")
    A, B = torch.randn(1, 3, 128, 128), torch.randn(1, 3, 128, 128)
    with pytest.raises(T.TfcError):
        net.stn_phi(torch.cat((A, B), 1))
    with pytest.raises(T.TfcError):
        net(A, B, B)


def test_torch_localiser_is_the_plain_layer_composition(monkeypatch):
    """the default path computes exactly localization -> flatten -> fc_loc (what it computed before the knob existed), forward and backward"""
    monkeypatch.delenv("TFC_LOCALISER", raising=False)
    torch.manual_seed(2)
    net = stn21.Net((3, 128, 128))
    x = torch.randn(2, 6, 128, 128, requires_grad=True)
    got = net.stn_phi(x)
    (got * torch.arange(12.0).reshape(2, 2, 3)).sum().backward()
    gx, gw = x.grad.clone(), net.localization.vit[0].patch.weight.grad.clone()
    x.grad = None
    net.zero_grad()
    xs = net.localization(x)
    want = net.fc_loc(xs.reshape(xs.shape[0], -1)).view(-1, 2, 3)
    (want * torch.arange(12.0).reshape(2, 2, 3)).sum().backward()
    assert torch.equal(got, want)
    assert torch.equal(gx, x.grad) and torch.equal(gw, net.localization.vit[0].patch.weight.grad)
