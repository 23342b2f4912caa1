"""Host-side tests of the CycleGAN generator (no GPU): the reflect-padded 3 x 3 convolution op is declared on every layer of the binding and exported by
the built library; its gather descriptors -- the reflect rule of the forward and weight-gradient halo, the padded-grid input gradient and its fold --
reproduce torch in the library's host emulator; GeneratorResNet carries the reference's state_dict keys (fixture: names and shapes only); the module's
torch path equals the float64 restatement tests/cyclegan_ref.py, which pins that restatement against torch's own layers; the HIP path refuses a
replica and a CPU tensor."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import cyclegan_ref as R
from tfc_gan_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = {"tfc_norm_add_fwd": 13, "tfc_conv_dgrad_ws_bytes": 7, "tfc_conv_dgrad_set_ws": 2}       # name -> number of arguments


def test_op_conv3r_comes_out_of_the_header_parse():
    assert _lib.CONSTANTS["OP_CONV3R"] == 6                       # the next free op number of the header
    assert _lib.OP_CONV3R == 6 and ops.OP_CONV3R == 6
    assert sorted(v for k, v in _lib.CONSTANTS.items() if k.startswith("OP_")) == list(range(7))
    f = ops.OUT_HW[_lib.OP_CONV3R]
    assert [f(h) for h in (2, 9, 64)] == [2, 9, 64]
    assert set(ops.OUT_HW) == {v for k, v in _lib.CONSTANTS.items() if k.startswith("OP_")}


def test_new_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.PROTOTYPES, name                      # = declared in the header
        assert len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert hasattr(lib, name), name                           # = exported by the built library
    assert lib.tfc_abi_version() == 3                             # symbols are only added
    for pas in (0, 1):
        assert lib.tfc_conv_packed_bytes(ops.DT_BF16, _lib.OP_CONV3R, pas, 256, 256) == lib.tfc_conv_packed_bytes(ops.DT_BF16, _lib.OP_CONV3, pas, 256, 256) > 0
    # the scratch of the input gradient: the padded gradient in the storage type; nothing for any other op
    assert lib.tfc_conv_dgrad_ws_bytes(ops.DT_BF16, _lib.OP_CONV3R, 2, 9, 17, 32, 64) == 2 * 11 * 19 * 32 * 2
    assert lib.tfc_conv_dgrad_ws_bytes(ops.DT_F32, _lib.OP_CONV3R, 2, 9, 17, 32, 64) == 2 * 11 * 19 * 32 * 4
    assert lib.tfc_conv_dgrad_ws_bytes(ops.DT_BF16, _lib.OP_CONV3, 2, 9, 17, 32, 64) == 0


def _nhwc8(x):
    n, c, h, w = x.shape
    out = np.zeros((n, h, w, (c + 7) // 8 * 8), dtype=np.float32)
    out[..., :c] = x.detach().numpy().transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out)


def _emulate(pas, es, a, b, out_shape, N, H, W, Cin, Cout):
    y = np.zeros(out_shape, dtype=np.float32)
    rc = _lib.load().tfc_host_emulate_conv(_lib.OP_CONV3R, pas, es, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
                                           y.ctypes.data_as(ctypes.c_void_p), N, H, W, Cin, Cout)
    _lib.check(rc, "tfc_host_emulate_conv")
    return y


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(3, 2, 2, 32, 32), (2, 8, 16, 32, 32), (2, 9, 17, 32, 64), (2, 3, 20, 64, 32)])
@pytest.mark.parametrize("es", [2, 4])
def test_conv3r_gather_model_matches_torch(N, H, W, Cin, Cout, es):
    """the descriptors of the three passes and the packed operand stream, evaluated by the library's host emulator, against
    F.conv2d(F.pad(x, mode="reflect"), w) and its autograd adjoints (the padding's adjoint included); bounds of test_darkvisible_host.py"""
    rng = np.random.default_rng(900 + Cin + H)
    x = torch.from_numpy(rng.standard_normal((N, Cin, H, W)).astype(np.float32)).requires_grad_(True)
    w4 = np.zeros((Cout, Cin, 4, 4), dtype=np.float32)
    w4[:, :, :3, :3] = (rng.standard_normal((Cout, Cin, 3, 3)) * 0.1).astype(np.float32)
    w = torch.from_numpy(w4).requires_grad_(True)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w[:, :, :3, :3])
    go = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    gx, gw = torch.autograd.grad(y, (x, w), go)
    c8 = lambda c: (c + 7) // 8 * 8  # noqa: E731
    got = _emulate(0, es, _nhwc8(x), w4, (N, H, W, c8(Cout)), N, H, W, Cin, Cout)
    np.testing.assert_allclose(got[..., :Cout], y.detach().numpy().transpose(0, 2, 3, 1), atol=2e-4)
    got = _emulate(1, es, _nhwc8(go), w4, (N, H, W, c8(Cin)), N, H, W, Cin, Cout)
    np.testing.assert_allclose(got[..., :Cin], gx.numpy().transpose(0, 2, 3, 1), atol=2e-4)
    got = _emulate(2, es, _nhwc8(x), _nhwc8(go), (Cout, Cin, 4, 4), N, H, W, Cin, Cout)
    np.testing.assert_allclose(got, gw.numpy(), atol=2e-3, rtol=1e-4)
    assert np.abs(got[:, :, 3, :]).max() == 0 and np.abs(got[:, :, :, 3]).max() == 0      # the seven unused taps of the slot


def test_conv3r_refuses_a_one_pixel_axis_on_the_host():
    q = (ctypes.c_int * 8)()
    lib = _lib.load()
    assert lib.tfc_conv_plan_query(ops.DT_BF16, _lib.OP_CONV3R, 0, 1, 1, 4, 32, 32, 0, 256, q, 8) < 0
    msg = lib.tfc_last_error().decode()
    assert "H=1" in msg and "W=4" in msg, msg
    assert lib.tfc_conv_plan_query(ops.DT_BF16, _lib.OP_CONV3R, 0, 1, 2, 2, 32, 32, 0, 256, q, 8) == 8


def test_generator_resnet_keys_and_shapes_equal_the_reference():
    g = np.load(os.path.join(GOLDEN, "cyclegan_keys.npz"), allow_pickle=False)
    shape, n = tuple(int(v) for v in g["input_shape"]), int(g["num_residual_blocks"])
    assert (shape, n) == ((3, 256, 256), 9)
    sd = T.GeneratorResNet(shape, n).state_dict()
    assert list(sd) == [str(k) for k in g["names"]]
    for k, row in zip(sd, g["shapes"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in row[:sd[k].dim()]), k
    convs = [k[:-len(".weight")] for k in sd if k.endswith(".weight") and "block" not in k]
    assert convs == ["model.1", "model.4", "model.7", "model.20", "model.24", "model.28"]
    assert [k for k in sd if k.startswith("model.10.")] == ["model.10.block.1.weight", "model.10.block.1.bias", "model.10.block.5.weight",
                                                            "model.10.block.5.bias"]
    assert "model.18.block.5.bias" in sd and not any(k.startswith("model.19.") for k in sd)
    assert list(T.ResidualBlock(32).state_dict()) == ["block.1.weight", "block.1.bias", "block.5.weight", "block.5.bias"]


def test_torch_trunk_on_cpu_equals_the_restatement_in_float64():
    """trunk="torch" on the CPU against tests/cyclegan_ref.py at (3, 32, 32), 2 blocks, float64, to 1e-12: pins the restatement against torch's own
    layers (nn.ReflectionPad2d, nn.InstanceNorm2d, nn.Upsample) -- output and input gradient"""
    g = O.init_weights_portable(T.GeneratorResNet((3, 32, 32), 2, trunk="torch"), seed=75, std=0.05).double()
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((2, 3, 32, 32))).requires_grad_(True)
    go = torch.from_numpy(rng.standard_normal((2, 3, 32, 32)))
    y = g(x)
    (gx,) = torch.autograd.grad(y, x, go)
    x2 = x.detach().clone().requires_grad_(True)
    y2 = R.generator_resnet(x2, {k: v.detach() for k, v in g.state_dict().items()}, 2)
    (gx2,) = torch.autograd.grad(y2, x2, go)
    assert y.dtype == torch.float64 and (y - y2).abs().max().item() <= 1e-12
    assert (gx - gx2).abs().max().item() <= 1e-12
    blk = g.model[10]
    xb = torch.from_numpy(rng.standard_normal((2, 256, 5, 6)))
    want = R.residual_block(xb, *R.block_params({k: v.detach() for k, v in blk.state_dict().items()}, ""))["out"]
    assert (blk.forward_torch(xb) - want).abs().max().item() <= 1e-12


def test_hip_path_refuses_a_replica_and_a_cpu_tensor():
    blk = T.ResidualBlock(32)
    with pytest.raises(T.TfcError, match="CPU tensor"):
        blk(torch.zeros(1, 32, 4, 4))
    with pytest.raises(T.TfcError, match="CPU tensor"):
        T.GeneratorResNet((3, 16, 16), 1)(torch.zeros(1, 3, 16, 16))
    for mod in (T.ResidualBlock(32), T.GeneratorResNet((3, 16, 16), 1)):
        mod._is_replica = True
        with pytest.raises(T.TfcError, match="DataParallel"):
            mod(torch.zeros(1, mod.features if isinstance(mod, T.ResidualBlock) else 3, 16, 16))
    with pytest.raises(T.TfcError, match="trunk="):
        T.GeneratorResNet((3, 16, 16), 1, trunk="eager")
    with pytest.raises(T.TfcError, match="multiples of 64"):
        T.nets.ResNetTrunkCore(ops.DT_BF16, 24, 1)
