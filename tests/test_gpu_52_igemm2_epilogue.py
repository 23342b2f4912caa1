"""Bit-exact tests of the persistent gather GEMM's epilogue (tfc_igemm2_kernel): every flag set the kernel compiles its own epilogue for, and one that
takes the run-time copy, on every workgroup tile, at ragged tiles in both directions, a partial n-block, the four strided phases of a transposed
convolution and a windowed destination; and the grid hook (tfc_debug_set_persistent_grid), which must not change a bit.

Cases, inputs and expectations: tests/igemm2_epilogue_cases.py (proven on the host by test_igemm2_epilogue_host.py). Comparison: torch.equal."""
import ctypes

import pytest
import torch

from tests import conv_exact as X
from tests import igemm2_epilogue_cases as E
from tfc_gan_amd import _lib, ops
from tfc_gan_amd.ops import DT_BF16, View

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_IGEMM2 = 1                                 # tfc_conv_plan_query slot 0: the persistent kernel (as test_gpu_49_conv2_exact.py reads it)


@pytest.fixture(autouse=True)
def hooks_off():
    lib = _lib.load()
    yield
    _lib.check(lib.tfc_debug_set_igemm_config(-1), "tfc_debug_set_igemm_config")
    _lib.check(lib.tfc_debug_set_persistent_grid(0), "tfc_debug_set_persistent_grid")


_REF = {}


def reference(g, Cout):
    """inputs and the float64 convolution of a (geometry, Cout), computed once and shared (never modified) by the tests that need them"""
    key = (g.name, Cout)
    if key not in _REF:
        x, w, b, base = E.inputs(g, Cout)
        _REF[key] = dict(x=x, w=w, b=b, base=base, z=X.ref_fwd(g.op, x, w),
                         xv=X.to_view(x.to(DEV), DT_BF16), pk=ops.pack_weight(DT_BF16, g.op, 0, w.to(DEV, torch.float32).contiguous(), g.Cin, Cout),
                         bias=b.to(DEV, torch.float32).contiguous(), osc=torch.tensor([E.OSCALE], dtype=torch.float32, device=DEV))
    return _REF[key]


def window(g, Cout, fill64):
    """(flat, View): the skip window -- channels [C, 2 C) of an [N, OH, OW, 2 C] concat buffer -- in the middle of a flat allocation with GUARD
    sentinel elements on either side; the window holds fill64 (NCHW float64), everything else SENTINEL"""
    OH = E.out_hw(g)
    n = g.N * OH * OH * 2 * Cout
    flat = torch.full((n + 2 * E.GUARD,), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    t = flat[E.GUARD:E.GUARD + n].view(g.N, OH, OH, 2 * Cout)
    t[..., Cout:] = fill64.permute(0, 2, 3, 1).to(DEV, torch.bfloat16)
    return flat, View(t, Cout, Cout)


def run(g, fs, Cout, ref):
    """one launch into a fresh window; returns (flat buffer, View, statistics or None)"""
    OH = E.out_hw(g)
    fill = ref["base"] if fs.accum else torch.full((g.N, Cout, OH, OH), 3.0, dtype=torch.float64)
    flat, yv = window(g, Cout, fill)
    stats = torch.zeros((g.N, Cout, 2), dtype=torch.float32, device=DEV) if fs.stats else None
    ops.conv_fwd(DT_BF16, g.op, ref["xv"], g.Cin, Cout, ref["pk"], yv, bias=ref["bias"] if fs.bias else None, stats=stats, flags=fs.flags,
                 oscale=ref["osc"] if fs.oscale else None)
    torch.cuda.synchronize()
    return flat, yv, stats


def check(g, fs, Cout, ref, flat, yv, stats, what):
    got = X.from_view(yv).cpu()
    X.assert_exact(got, E.expected(g, fs, ref["z"], ref["b"], ref["base"]), what)
    X.assert_untouched(yv, what)                                  # the other half of the concat buffer
    guards = torch.cat([flat[:E.GUARD], flat[-E.GUARD:]]).float()
    assert int((guards != X.SENTINEL).sum()) == 0, f"{what}: elements in front of or behind the buffer changed"
    if stats is not None:                                         # float64 sums of the tensor the kernel stored
        v = got.double()
        assert v.abs().sum((2, 3)).max().item() < X.EXACT_BOUND and (v * v).sum((2, 3)).max().item() < X.EXACT_BOUND
        X.assert_exact(stats[..., 0].cpu().double(), v.sum((2, 3)), f"{what} statistics 0", X.VEC_DIMS)
        X.assert_exact(stats[..., 1].cpu().double(), (v * v).sum((2, 3)), f"{what} statistics 1", X.VEC_DIMS)


def force_tile(cfg, g, Cout, flags):
    """force the workgroup tile and make sure the plan took it: the persistent kernel in form cfg"""
    lib = _lib.load()
    _lib.check(lib.tfc_debug_set_igemm_config(cfg), "tfc_debug_set_igemm_config")
    q = (ctypes.c_int * 8)()
    assert lib.tfc_conv_plan_query(DT_BF16, g.op, 0, g.N, g.H, g.H, g.Cin, Cout, flags, 256, q, 8) == 8
    assert (q[0], q[1]) == (K_IGEMM2, cfg), (cfg, list(q))


@pytest.mark.parametrize("g", E.GEOMETRIES, ids=[g.name for g in E.GEOMETRIES])
@pytest.mark.parametrize("cfg", sorted(E.TILES))
def test_exact_epilogue_flag_sets_on_every_tile(cfg, g):
    """each flag set the geometry's op takes, on workgroup tile cfg, stored into a window: exact values, exact statistics, nothing else touched"""
    Cout = E.TILES[cfg][1]
    ref = reference(g, Cout)
    for fs in E.FLAG_SETS:
        if g.op not in fs.ops:
            continue
        force_tile(cfg, g, Cout, fs.flags)
        flat, yv, stats = run(g, fs, Cout, ref)
        check(g, fs, Cout, ref, flat, yv, stats, f"{g.name} Cout {Cout} tile {cfg} {fs.name}")


@pytest.mark.parametrize("cfg", sorted(E.TILES))
def test_grid_hook_changes_no_bit(cfg):
    """1 workgroup (one walk over every work item), 3 (the work items do not divide: a partial last round, and the one-tile-late statistics flush meets a
    workgroup with no next tile) and the default grid give the same bits in the whole allocation and in the statistics -- and the right ones"""
    lib = _lib.load()
    g, Cout = E.GEOMETRIES[0], E.GRID_COUT
    ref = reference(g, Cout)
    for fs in E.FLAG_SETS:
        if g.op not in fs.ops:
            continue
        force_tile(cfg, g, Cout, fs.flags)
        outs = []
        for workgroups in (1, 3, 0):
            _lib.check(lib.tfc_debug_set_persistent_grid(workgroups), "tfc_debug_set_persistent_grid")
            flat, yv, stats = run(g, fs, Cout, ref)
            what = f"{g.name} Cout {Cout} tile {cfg} {fs.name} grid {workgroups}"
            check(g, fs, Cout, ref, flat, yv, stats, what)
            outs.append((flat, stats))
        _lib.check(lib.tfc_debug_set_persistent_grid(0), "tfc_debug_set_persistent_grid")
        for flat, stats in outs[1:]:
            assert torch.equal(flat.view(torch.int16), outs[0][0].view(torch.int16)), f"{fs.name} tile {cfg}: the destination depends on the grid"
            if stats is not None:
                assert torch.equal(stats.view(torch.int32), outs[0][1].view(torch.int32)), f"{fs.name} tile {cfg}: the statistics depend on the grid"
