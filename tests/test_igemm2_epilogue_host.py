"""Host half of the gather GEMM's epilogue tests (cases: tests/igemm2_epilogue_cases.py). No GPU: the float64 references the GPU test compares
against are checked here against the library's host model of the gather (tfc_host_emulate_conv), every input stays in the range where fp32 partial sums
are exact, and the case table covers what it says it covers."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_exact as X
from tests import igemm2_epilogue_cases as E
from tfc_gan_amd import _lib, ops

_GEOM_COUT = sorted({(g.name, cout) for g in E.GEOMETRIES for _, cout in E.TILES.values()} | {(E.GEOMETRIES[0].name, E.GRID_COUT)})
_BY_NAME = {g.name: g for g in E.GEOMETRIES}


def _nhwc8(x):
    n, c, h, w = x.shape
    out = np.zeros((n, h, w, ops.pad8(c)), dtype=np.float32)
    out[..., :c] = x.numpy().transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out)


@pytest.mark.parametrize("gname,Cout", _GEOM_COUT)
def test_float64_reference_equals_the_host_gather_model(gname, Cout):
    """ref_fwd in float64 == the library's own model of the gather (bf16 element size) on the same integers, element for element"""
    g = _BY_NAME[gname]
    x, w, b, base = E.inputs(g, Cout)
    z = X.ref_fwd(g.op, x, w)
    X.assert_dyadic(z, 1, f"{gname} reference")
    OH = E.out_hw(g)
    assert tuple(z.shape) == (g.N, Cout, OH, OH)
    y = np.zeros((g.N, OH, OH, ops.pad8(Cout)), dtype=np.float32)
    wn = np.ascontiguousarray(w.numpy().astype(np.float32))
    rc = _lib.load().tfc_host_emulate_conv(g.op, 0, 2, _nhwc8(x).ctypes.data_as(ctypes.c_void_p), wn.ctypes.data_as(ctypes.c_void_p),
                                           y.ctypes.data_as(ctypes.c_void_p), g.N, g.H, g.H, g.Cin, Cout)
    _lib.check(rc, "tfc_host_emulate_conv")
    got = torch.from_numpy(y[..., :Cout]).permute(0, 3, 1, 2).double()
    X.assert_exact(got, z, f"{gname} Cout {Cout}: host gather model against float64")


@pytest.mark.parametrize("gname,Cout", _GEOM_COUT)
def test_inputs_and_expectations_stay_exact(gname, Cout):
    """every partial sum below 2^24 quanta; the expectation of every flag set is built without a rounding that is not the kernel's (conv_exact.store and
    assert_dyadic raise otherwise); statistics of the stored tensor are exact sums in fp32"""
    g = _BY_NAME[gname]
    x, w, b, base = E.inputs(g, Cout)
    for t in (x, w, base, 2 * b):
        assert torch.equal(t, t.round()) and t.abs().max().item() <= 1
    z = X.ref_fwd(g.op, x, w)
    for fs in E.FLAG_SETS:
        if g.op not in fs.ops:
            continue
        assert E.worst_partial_sum(g, fs) < X.EXACT_BOUND
        want = E.expected(g, fs, z, b, base)
        assert want.dtype == torch.bfloat16 and torch.isfinite(want.float()).all()
        if fs.stats:
            v = want.double()
            assert v.abs().sum((2, 3)).max().item() < X.EXACT_BOUND and (v * v).sum((2, 3)).max().item() < X.EXACT_BOUND


def test_case_table_covers_the_edges():
    tiles = {g.name: (-(-E.out_hw(g) // X.TILE_H), -(-E.out_hw(g) // X.TILE_W)) for g in E.GEOMETRIES}
    assert tiles["conv9x9"] == (2, 1) and E.out_hw(_BY_NAME["conv9x9"]) % X.TILE_H == 1         # a second tile row with one live row
    assert tiles["conv17x17"] == (3, 2) and E.out_hw(_BY_NAME["conv17x17"]) % X.TILE_W == 1     # a second tile column with one live column
    assert E.out_hw(_BY_NAME["convT5to10"]) == 10
    for cfg, (bn, cout) in E.TILES.items():
        assert cout % 8 == 0 and (cout % bn != 0 or bn == 32), (cfg, bn, cout)                  # a partial last n-block wherever the tile has one
        assert bn < 128 or cout >= 128                                                          # the plan's own condition for a 128-channel tile
    # the grid-hook cases: with 3 workgroups the last round is partial on every tile form
    g = _BY_NAME["conv9x9"]
    for cfg, (bn, _) in E.TILES.items():
        nwork = g.N * tiles["conv9x9"][0] * tiles["conv9x9"][1] * -(-E.GRID_COUT // bn)
        assert nwork > 3 and nwork % 3 != 0, (cfg, nwork)
    # the six specialised flag sets of the kernel and one that takes the run-time copy
    special = {0, _lib.EP_STATS, _lib.EP_BIAS | _lib.EP_LEAKY, _lib.EP_ACCUM, _lib.EP_BIAS | _lib.EP_RELU}
    assert {fs.flags for fs in E.FLAG_SETS[:6]} == special and E.FLAG_SETS[6].flags not in special
