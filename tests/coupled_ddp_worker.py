"""Worker of tests/test_gpu_46_coupled_ddp.py::test_two_ranks_match_one_rank_* (alone, or under torch.distributed.run as 2 ranks sharing cuda:0, gloo).
argv: out.pt config scope. One fp32 step of a 4-patch configuration on this rank's shard of a global batch of 4:
    mask   : MASK-4, TrainStep(patches=4, mask=True, **mask_weights())            -- batch extrema of the edge mask
    kl     : TrainStep(patches=4, region_fft="kl", **region_weights("kl"))        -- softmax over the batch
    debias : TrainStep(patches=4, **debias_weights("v1")), explicit labels and gen_labels of the global batch, sharded like the images
scope is TrainStep's batch_scope. Rank 0 saves the updated parameters, the gradients and every logged scalar (TrainStep averages them over the ranks);
the one-rank mask run also saves how far the extrema of the three masked batches are from their runners-up, so that a failure can be told from a
near-tie."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfc_gan_amd as T  # noqa: E402
from oracle import tfcgan_oracle as O  # noqa: E402  (seeded inputs / portable weights only)
from tests import mask_ref  # noqa: E402
from tfc_gan_amd import parallel  # noqa: E402

GLOBAL_BATCH = 4


def networks(config, dev):
    if config == "mask":
        G, D = T.GeneratorUNet((3, 256, 256), mask=True), T.Discriminator1((3, 256, 256))
    elif config == "debias":
        G, D = T.GeneratorUNet((3, 256, 256), labels=3), T.Discriminator1((3, 256, 256), aux_classes=(2, 4, 3))
    else:
        G, D = T.GeneratorUNet((3, 256, 256)), T.Discriminator1((3, 256, 256))
    G, D = O.init_weights_portable(G, seed=61), O.init_weights_portable(D, seed=62)
    if config == "debias":                                       # the head weights at the scale of tests/test_gpu_43_debias.py's fixtures
        with torch.no_grad():
            for k in ("aux_gender", "aux_ethn", "aux_age"):
                getattr(D, k)[0].weight.mul_(0.1)
    return G.to(dev).eval(), D.to(dev).train()                   # eval: no dropout, InstanceNorm unaffected


def extrema_gaps(img):
    """relative gaps between the two largest |lap|, the two largest blurred values and the two smallest |lap| of a batch (fp64 restatement)"""
    parts = mask_ref.mask_parts(img.double().cpu())
    L, Bl = parts["L"].flatten().sort().values, parts["Bl"].flatten().sort().values
    return torch.stack([(L[-1] - L[-2]) / L[-1], (Bl[-1] - Bl[-2]) / Bl[-1], (L[1] - L[0]) / L[-1]])


def run(out_path, config, scope):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.float32)                           # exact-fp32 mode: the only difference left is summation order
    G, D = networks(config, dev)
    kw = {"mask": dict(T.mask_weights(), mask=True), "kl": dict(T.region_weights("kl"), region_fft="kl"), "debias": T.debias_weights("v1")}[config]
    ts = T.TrainStep(G, D, compute_dtype=torch.float32, patches=4, batch_scope=scope, **kw)
    A, B = O.synthetic_pairs(GLOBAL_BATCH, seed=63)
    sl = parallel.shard_slice(GLOBAL_BATCH)
    step_kw = {}
    if config == "debias":
        rng = np.random.default_rng(64)
        labels, gen_labels = (np.stack([rng.integers(0, c, GLOBAL_BATCH) for c in (2, 4, 3)], 1) for _ in range(2))
        step_kw = {"labels": labels[sl].astype(np.float32), "gen_labels": gen_labels[sl]}
    out = ts.step(A[sl].to(dev), B[sl].to(dev), neg_idx=[3, 0, 2, 1], **step_kw)
    torch.cuda.synchronize()
    if parallel.rank() == 0:
        keys = sorted(k for k in out if out[k].numel() == 1)
        saved = {"g": ts.gflat.data.cpu(), "d": ts.dflat.data.cpu(), "gg": ts.gflat.grad.cpu() / world, "dg": ts.dflat.grad.cpu() / world,
                 "keys": keys, "losses": torch.stack([out[k].reshape(()).float() for k in keys]).cpu(),
                 "u3": D.state_dict()["model.3.parametrizations.weight.0._u"].cpu()}
        if config == "mask" and world == 1:
            saved["gaps"] = {"real_A": extrema_gaps(A), "real_B": extrema_gaps(B), "fake": extrema_gaps(out["fake_B"])}
        torch.save(saved, out_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    run(*sys.argv[1:4])
