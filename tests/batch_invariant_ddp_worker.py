"""Worker of tests/test_gpu_37_batch_invariant.py (alone, or under torch.distributed.run: 2 ranks sharing cuda:0, gloo): tests/ddp_worker.py's PATCH-16
step (fp32 mode, generator in eval) on this rank's shard of a global batch of 2, which also keeps what belongs to single samples -- the generated
images and the discriminator logits of the generator step -- gathered in global sample order. TFC_BATCH_INVARIANT comes from the environment."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfc_gan_amd as T  # noqa: E402
from oracle import tfcgan_oracle as O  # noqa: E402  (seeded inputs / portable weights only)
from tfc_gan_amd import parallel  # noqa: E402


def run(out_path, global_batch=2):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.float32)
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(dev).eval()
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(dev).train()
    ts = T.TrainStep(G, D, compute_dtype=torch.float32)
    A, B = O.synthetic_pairs(global_batch, seed=63)
    sl = parallel.shard_slice(global_batch)
    A, B = A[sl].to(dev), B[sl].to(dev)
    with torch.no_grad():                                         # the logits of the pair the generator step scores, before any update (no power iteration)
        fake0, _ = ts.G.forward(A, seed=0, train=False, save=False)
        lg, _ = ts.D.forward(fake0, A, power_iter=False, save=False)
        logits = lg.t[..., lg.coff:lg.coff + 1].float().cpu().contiguous()
    out = ts.step(A, B, neg_idx=[3, 3, 7, 0, 4, 9, 15, 2, 8, 8, 1, 12, 5, 13, 6, 10])
    torch.cuda.synchronize()
    fake = out["fake_B"].float().cpu().contiguous()
    if world > 1:
        fakes, logs = [torch.empty_like(fake) for _ in range(world)], [torch.empty_like(logits) for _ in range(world)]
        dist.all_gather(fakes, fake)
        dist.all_gather(logs, logits)
        fake, logits = torch.cat(fakes), torch.cat(logs)
    if parallel.rank() == 0:
        torch.save({"g": ts.gflat.data.cpu(), "d": ts.dflat.data.cpu(), "gg": ts.gflat.grad.cpu() / world, "dg": ts.dflat.grad.cpu() / world,
                    "fake_B": fake, "logits": logits}, out_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1])
