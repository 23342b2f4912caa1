"""Worker of tests/test_gpu_37_batch_invariant.py (alone, or under torch.distributed.run: 2 ranks sharing cuda:0, gloo): tests/stn21_ddp_worker.py's STN21
step (fp32 mode, no LPIPS, generators and localiser in eval) on this rank's shard of a global batch of 2, which also keeps what belongs to single
samples, gathered in global sample order: theta (the localiser's output as the warp receives it), fake_B, fake_A2, warped_B and the logits of every
discriminator call of the step. TFC_BATCH_INVARIANT and TFC_LOCALISER come from the environment."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfc_gan_amd as T  # noqa: E402
from oracle import tfcgan_oracle as O  # noqa: E402  (seeded inputs / portable weights only)
from tfc_gan_amd import parallel, stn21  # noqa: E402


def run(out_path, global_batch=2):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("gloo")
    T.set_compute_dtype(torch.float32)
    torch.manual_seed(1)
    st = stn21.STN21Step((3, 256, 256), lpips=None, device=dev, bucket_bytes=64 << 20)
    for i, m in enumerate((st.G1, st.G2, st.D1, st.D2, st.net)):
        O.init_weights_portable(m, seed=201 + i)
    with torch.no_grad():
        st.net.fc_loc[6].weight.mul_(4.0)
    st._bump()
    st.G1.eval(); st.G2.eval(); st.net.eval()
    kept = {"theta": [], "logits_D1": [], "logits_D2": []}
    st.net.warp.register_forward_pre_hook(lambda m, args: kept["theta"].append(args[0].detach().float().reshape(args[0].shape[0], -1).cpu()))
    st.D1.register_forward_hook(lambda m, args, out: kept["logits_D1"].append(out.detach().float().reshape(out.shape[0], -1).cpu()))
    st.D2.register_forward_hook(lambda m, args, out: kept["logits_D2"].append(out.detach().float().reshape(out.shape[0], -1).cpu()))
    A, B = O.synthetic_pairs(global_batch, seed=77)
    sl = parallel.shard_slice(global_batch)
    out = st.step(A[sl].to(dev), B[sl].to(dev))
    torch.cuda.synchronize()
    assert len(kept["theta"]) == 1 and len(kept["logits_D1"]) == 4 and len(kept["logits_D2"]) == 4, {k: len(v) for k, v in kept.items()}
    per_sample = {k: torch.cat(v, 1).contiguous() for k, v in kept.items()}        # [n, calls x values]
    for k in ("fake_B", "fake_A2", "warped_B"):
        per_sample[k] = out[k].float().cpu().contiguous()
    if world > 1:
        for k, v in per_sample.items():
            parts = [torch.empty_like(v) for _ in range(world)]
            dist.all_gather(parts, v)
            per_sample[k] = torch.cat(parts)
    if parallel.rank() == 0:
        save = {"g": st.gflat.data.cpu(), "d": st.dflat.data.cpu(), "gg": st.gflat.grad.cpu() / world, "dg": st.dflat.grad.cpu() / world,
                "losses": torch.stack([out[k].float().reshape(()) for k in ("loss_G", "loss_GAN", "recon_loss", "morph_loss", "loss_D")]).cpu()}
        save.update(per_sample)
        torch.save(save, out_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1])
