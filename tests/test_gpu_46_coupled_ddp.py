"""Data-parallel equivalence of the batch-coupled 4-patch configurations: MASK-4 (the edge mask is normalised by extrema of the whole batch) and the
KL regional loss (softmax over the batch) with batch_scope="global", and the label-conditioned step, on two ranks (sharing the one card, gloo), each
stepping its half of a global batch of 4, against one rank stepping all 4 images -- held to the bounds of
tests/test_gpu_20_ddp.py::test_two_ranks_match_one_rank. With batch_scope="shard" each rank normalises over its own two images: the control runs
must MISS those bounds, which is what shows that the bounds see the coupling."""
import functools
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "coupled_ddp_worker.py")
RCCL_WORKER = os.path.join(ROOT, "tests", "coupled_rccl_world1_worker.py")
COUPLED = {"mask": ("loss_mask",), "kl": ("loss_FFT_reg", "loss_Amp_reg", "loss_Pha_reg"),
           "debias": ("loss_label", "real_loss_label", "fake_loss_label")}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@functools.lru_cache(maxsize=None)
def _tmp():
    return tempfile.TemporaryDirectory(prefix="coupled_ddp_")        # removed when the interpreter ends; shared by the cached runs below


@functools.lru_cache(maxsize=None)
def run(config, ranks, scope="global"):
    """one worker run (a child process, never an exec of this one), loaded; the one-rank run of a configuration is shared by its tests"""
    out = os.path.join(_tmp().name, f"{config}_{ranks}_{scope}.pt")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TFC_FORCE_COLLECTIVES"):
        env.pop(k, None)
    if ranks == 1:
        cmd = [sys.executable, WORKER, out, config, scope]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), WORKER, out, config, scope]
    subprocess.run(cmd, check=True, env=env, timeout=300)
    return torch.load(out, weights_only=True)


def violations(a, b):
    """the bounds of test_two_ranks_match_one_rank that b misses against a, as a list of strings (empty: b matches a)"""
    bad = []
    if not torch.equal(a["u3"], b["u3"]):                          # spectral-norm state depends on the weights only: bit-equal on every rank and run
        bad.append("u3 differs")
    assert a["keys"] == b["keys"]
    for k, x, y in zip(a["keys"], a["losses"], b["losses"]):       # every logged scalar
        if not torch.allclose(x, y, rtol=2e-5, atol=1e-6):
            bad.append(f"{k}: {x.item():.9g} vs {y.item():.9g}")
    for k in ("gg", "dg"):                                          # all-reduced gradient SUM / world == single-process batch-mean gradient
        rel = ((a[k] - b[k]).norm() / a[k].norm()).item()
        print(f"  {k}: rel-L2 difference {rel:.3e}")
        if not rel <= 1e-5:
            bad.append(f"{k}: rel-L2 {rel:.3e}")
    for k in ("g", "d"):                                            # the first Adam step moves every weight by ~lr: only round-off-level gradients may differ
        frac = ((a[k] - b[k]).abs() > 2e-5).float().mean().item()
        if not frac <= 2e-2:
            bad.append(f"{k}: {frac:.3e} of the weights moved by more than 2e-5")
    return bad


@pytest.mark.parametrize("config", ["mask", "kl", "debias"])
def test_two_ranks_match_one_rank(config):
    one, two = run(config, 1), run(config, 2)
    assert set(COUPLED[config]) <= set(one["keys"])
    for k, x, y in zip(one["keys"], one["losses"], two["losses"]):
        print(f"  {k}: one rank {x.item():.9g}, two ranks {y.item():.9g}")
    if "gaps" in one:
        for name, g in one["gaps"].items():
            print(f"  {name}: relative gaps max |lap| {g[0].item():.3e}, max blur {g[1].item():.3e}, min |lap| {g[2].item():.3e}")
    bad = violations(one, two)
    assert not bad, bad


@pytest.mark.parametrize("config", ["mask", "kl"])
def test_shard_scope_on_two_ranks_misses_the_bounds(config):
    """the control: each rank normalising over its own shard is NOT the one-rank step, and the bounds above notice"""
    bad = violations(run(config, 1), run(config, 2, "shard"))
    print(f"  batch_scope='shard', {config}: {bad}")
    assert bad
    assert any(b.startswith(COUPLED[config][0]) for b in bad), bad


@pytest.mark.parametrize("config,gathers", [("mask", 8), ("kl", 1)])
def test_coupled_steps_under_a_real_one_rank_rccl_group(tmp_path, config, gathers):
    """tests/test_gpu_20_ddp.py::test_two_stream_step_under_a_real_one_rank_rccl_group for the two batch-coupled steps: two bf16 steps with the side
    stream on under a one-rank "nccl" group with TFC_FORCE_COLLECTIVES=1, where the phases run with a real all-gather between them (mask_A's on the
    main stream, the pixel losses' on the side stream). With one record per merge every phase leaves the bits of the unsplit entry point: weights, Adam
    moments, spectral-norm vectors and every logged loss must be BIT-EQUAL to the run without a process group."""
    plain, rccl = str(tmp_path / "plain.pt"), str(tmp_path / "rccl.pt")
    env = dict(os.environ, TFC_TEST_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TFC_FORCE_COLLECTIVES", "TFC_WGRAD_STREAM"):
        env.pop(k, None)
    subprocess.run([sys.executable, RCCL_WORKER, plain, "plain", config], check=True, env=env, timeout=300)
    r = subprocess.run([sys.executable, RCCL_WORKER, rccl, "rccl", config], env=env, timeout=300)
    if r.returncode == 77:
        pytest.skip("a one-rank RCCL process group cannot be created on this box (worker exit code 77)")
    assert r.returncode == 0
    a, b = torch.load(plain, weights_only=True), torch.load(rccl, weights_only=True)
    assert int(b["all_gather"]) == 2 * gathers, int(b["all_gather"])              # per step: 2 per mask forward (A, B, fake) + 2 in the backward; 1 per KL loss
    assert int(b["all_reduce"]) >= 2 * int(b["buckets"]), (int(b["all_reduce"]), int(b["buckets"]))     # every bucket of both networks per step (+ the loss averages)
    assert a["keys"] == b["keys"]
    for k in ("g", "d", "gm", "gv", "dm", "dv", "sn", "loss"):
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())
