"""Host half of the batch-32 exact tests (tests/conv_exact.py): the case table agrees with the network definitions, and the chosen value ranges keep
every partial sum of every pass exact in fp32 at both test batches."""
import torch

from oracle import tfcgan_oracle as O
from tests import conv_exact as X
from tfc_gan_amd import nets, ops
from tfc_gan_amd.ops import OP_CONV, OP_CONVT, OP_PADCONV, OP_UPCONV


def _derived(S=256, channels=3):
    """(net, layer, entry, pass, op, H, W, Cin, Cout, view) of the bf16 step, derived from the oracle's block lists, nets.D_BLOCKS and ops.OUT_HW"""
    out = set()
    # generator: down_i reads the pooled output of down_{i-1} (a skip window of a concat buffer for i >= 1)
    h = S
    downs = []
    for i, (name, cin, cout, normalize, drop) in enumerate(O._DOWNS):
        cin = channels if cin is None else cin
        downs.append((name, h, cin, cout))
        if i == 0:
            out.add(("G", name, "first_block_fwd", 0, OP_CONV, h, h, cin, cout, X.WINDOW))
            out.add(("G", name, "first_block_bwd_wgrad", 2, OP_CONV, h, h, cin, cout, X.WINDOW))   # dy_pooled: skip half of a concat gradient
        else:
            out.add(("G", name, "conv_fwd", 0, OP_CONV, h, h, cin, cout, X.WINDOW))
            out.add(("G", name, "conv_wgrad", 2, OP_CONV, h, h, cin, cout, X.WINDOW))
            out.add(("G", name, "conv_dgrad", 1, OP_CONV, h, h, cin, cout, X.WINDOW))
        h = nets.pooled(ops.OUT_HW[OP_CONV](h))
    # up_j reads d6 (j = 0) or the whole concat buffer of up_{j-1}; its output has the size of the skip it is concatenated with
    for j, (name, cin, cout, drop) in enumerate(O._UPS):
        view = X.FRESH if j == 0 else X.WHOLE
        for entry, pas in (("conv_fwd", 0), ("conv_wgrad", 2), ("conv_dgrad", 1)):
            out.add(("G", name, entry, pas, OP_CONVT, h, h, cin, cout, view))
        skip = downs[len(O._DOWNS) - 2 - j]
        assert ops.OUT_HW[OP_CONVT](h) == skip[1] // 2 and cout + skip[3] == (O._UPS[j + 1][1] if j + 1 < len(O._UPS) else 128)
        h = ops.OUT_HW[OP_CONVT](h)
    assert ops.OUT_HW[OP_UPCONV](h) == S
    for entry, pas in (("upconv_head_fwd", 0), ("conv_wgrad", 2), ("upconv_head_dgrad", 1)):
        out.add(("G", "final", entry, pas, OP_UPCONV, h, h, 128, channels, X.WHOLE))
    # discriminator: conv -> BlurPool(2) blocks on the image pair, then the ZeroPad + conv head
    h = S
    for bi, (i, cin, cout) in enumerate(nets.D_BLOCKS):
        name = f"model.{i}"
        if bi == 0:
            cin = 2 * channels
            out.add(("D", name, "first_block_fwd", 0, OP_CONV, h, h, cin, cout, X.FRESH))
            out.add(("D", name, "first_block_bwd_wgrad", 2, OP_CONV, h, h, cin, cout, X.FRESH))
            out.add(("D", name, "conv_dgrad_image", 1, OP_CONV, h, h, cin, cout, X.FRESH))
        else:
            for entry, pas in (("conv_fwd", 0), ("conv_wgrad", 2), ("conv_dgrad", 1)):
                out.add(("D", name, entry, pas, OP_CONV, h, h, cin, cout, X.FRESH))
        h = nets.pooled(ops.OUT_HW[OP_CONV](h))
    last = nets.D_BLOCKS[-1][2]
    for entry, pas in (("patchgan_head_fwd", 0), ("conv_wgrad", 2), ("conv_dgrad", 1)):
        out.add(("D", "model.13", entry, pas, OP_PADCONV, h, h, last, 1, X.FRESH))
    return out


def test_table_matches_the_network_definitions():
    table = {(c.net, c.layer, c.entry, c.pas, c.op, c.H, c.W, c.Cin, c.Cout, c.view) for c in X.CASES if c.net in ("G", "D")}
    want = _derived()
    assert table == want, {"not in the table": sorted(want - table), "not in the networks": sorted(table - want)}
    keys = [X.case_id(c) + f"-{c.pas}" for c in X.CASES]
    assert len(keys) == len(set(keys)), "duplicate table rows"


def test_lpips_rows_match_vgg16():
    from tfc_gan_amd import lpips
    h, cin, rows, first = 256, None, [], True
    for v in lpips.VGG16_CFG:
        if v == "M":
            h //= 2
            continue
        rows.append((h, 32 if first else cin, v))             # bf16: the image padded to one 64-byte channel chunk
        cin, first = v, False
    assert rows == X.LPIPS_LAYERS


def test_engine_order_of_the_weight_gradients():
    """G's weight gradients first (head, up5..up1, down6..down1), then D's (head, block 3..0): the order nets.py threads its workspace in"""
    names = [(c.net, c.layer) for c in X.WGRAD_ENGINE_ORDER]
    g = [("G", "final")] + [("G", n) for n, *_ in reversed(nets.G_UP)] + [("G", n) for n, *_ in reversed(nets.G_DOWN)]
    d = [("D", "model.13")] + [("D", f"model.{i}") for i, _, _ in reversed(nets.D_BLOCKS)]
    assert names == g + d


def test_value_ranges_keep_every_partial_sum_exact():
    for N in X.BATCHES:
        for c in X.CASES + X.fp32_cases(0) + X.fp32_cases(1) + X.fp32_cases(2):
            b = X.worst_partial_sum(c, N)
            assert b < X.EXACT_BOUND, (X.case_id(c), c.pas, N, b)


def test_lattice_density_bound_holds():
    v = X.ints((3, 5, 128, 128), 1, density=X.FIRST_BWD_DY_DENSITY)
    per_plane = (v != 0).sum((2, 3))
    assert per_plane.max().item() <= -(-128 * 128 // X.FIRST_BWD_DY_DENSITY)
    assert v.abs().max().item() == 1


def test_first_block_reference_chain_is_exact_and_bf16_representable():
    """the float64 d_raw of the fused first-block backward at slope 1/4 is a multiple of 1/256 that bf16 holds exactly (host restatement of what the
    GPU test asserts), and the exact compare localises a single bad element"""
    torch.manual_seed(0)
    N, Hc = 2, 33
    Po = (Hc - 1) // 2 + 1
    dy = X.ints((N, 64, Po, Po), 3, density=X.FIRST_BWD_DY_DENSITY)
    y = X.ints((N, 64, Hc, Hc), 4)
    d_raw = X.blur_t(dy, (N, 64, Hc, Hc), 2) * torch.where(y > 0, 1.0, X.SLOPE)
    X.assert_dyadic(d_raw, X.FIRST_BWD_QUANTUM, "d_raw")
    assert torch.equal(X.store(d_raw, ops.DT_BF16).double(), d_raw)
    a = X.store(d_raw, ops.DT_BF16)
    b = a.clone()
    b[1, 17, 9, 20] += 1
    try:
        X.assert_exact(b, a, "probe")
    except AssertionError as e:
        msg = str(e)
        assert "1 of" in msg and "image: 1 of 2" in msg and "(1, 17, 9, 20)" in msg, msg
    else:
        raise AssertionError("assert_exact missed a difference")
