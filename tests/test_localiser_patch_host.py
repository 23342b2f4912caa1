"""Host-side checks of the localiser's `patch_size` option and of the tiled attention entry points' declarations (no GPU): the header,
`_lib.PROTOTYPES` and the built library carry the two symbols; `stn21.Net` sizes `positions` and `fc_loc[0]` from the patch size, keeps its
state_dict key list, runs on the CPU at patch 32, and refuses a patch size that does not divide the image or passes 1025 tokens."""
import ctypes

import pytest
import torch

from tfc_gan_amd import _lib, stn21

NEW = ("tfc_vit_attention_tiled_fwd", "tfc_vit_attention_tiled_bwd")


def test_tiled_attention_symbols_declared_and_exported():
    so = ctypes.CDLL(_lib.build())
    for name in NEW:
        assert name in _lib.PROTOTYPES                               # = declared in the header
        assert hasattr(so, name)
    # the argument counts of the header's declarations
    assert [len(_lib.PROTOTYPES[name][1]) for name in NEW] == [9, 11]
    assert any(g.startswith("tfc_vit_attn_tiled") for g in _lib.GUARDED_KERNELS)        # the no-spill gate covers the new kernels


@pytest.fixture(scope="module")
def nets():
    out = {}
    for p in (16, 32, 64):
        torch.manual_seed(0)
        out[p] = stn21.Net((3, 256, 256), localiser="torch", patch_size=p)
    return out


@pytest.mark.parametrize("p,tokens,features", [(16, 257, 197376), (32, 65, 49920), (64, 17, 13056)])
def test_net_shapes_follow_patch_size(nets, p, tokens, features):
    net = nets[p]
    assert net.patch_size == p
    assert net.fc_loc[0].in_features == features == tokens * 768
    vit = net.localization.vit[0]
    assert tuple(vit.positions.shape) == (tokens, 768)
    assert tuple(vit.patch.weight.shape) == (768, 6, p, p)


def test_state_dict_keys_do_not_depend_on_patch_size(nets):
    keys = {p: list(n.state_dict()) for p, n in nets.items()}
    assert keys[16] == keys[32] == keys[64] and len(keys[64]) == 160       # 150 of the ViT, 2 of theta_emb, 8 of fc_loc
    assert list(stn21.Net((3, 256, 256), localiser="torch").state_dict()) == keys[64]       # the default is patch 64
    assert stn21.Net((3, 256, 256), localiser="torch").patch_size == 64


def test_cpu_forward_at_patch_32(nets):
    x = torch.randn(1, 6, 256, 256, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        theta = nets[32].stn_phi(x)
    assert tuple(theta.shape) == (1, 2, 3) and torch.isfinite(theta).all()


@pytest.mark.parametrize("p,word", [(48, "divisor"), (4, "4097")])
def test_bad_patch_size_raises(p, word):
    """48 does not divide 256; 4 gives 64 * 64 + 1 = 4097 tokens, above the kernels' 1025"""
    for make in (lambda: stn21.Net((3, 256, 256), localiser="torch", patch_size=p), lambda: stn21.LocalizerVIT((3, 256, 256), patch_size=p)):
        with pytest.raises(ValueError) as e:
            make()
        assert word in str(e.value) and (p == 48 or "1025" in str(e.value))
