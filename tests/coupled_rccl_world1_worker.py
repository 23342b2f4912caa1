"""Worker of tests/test_gpu_46_coupled_ddp.py::test_coupled_steps_under_a_real_one_rank_rccl_group. argv: out.pt mode config, mode = "plain" (no process
group) or "rccl" (a ONE-rank group of backend "nccl" = RCCL, TFC_FORCE_COLLECTIVES=1), config = "mask" (MASK-4) or "kl" (region_fft="kl"). Two bf16
steps on two streams with batch_scope="global": under the group the mask and the KL loss run in PHASES, and their records travel through
ProcessGroupNCCL's all-gather between the phases -- identities in value (one record per merge), real in stream ordering: the gathers of mask_A are
issued on the main stream, those of the pixel losses on the side stream. Saves the state and the number of collectives issued."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfc_gan_amd as T  # noqa: E402
from oracle import tfcgan_oracle as O  # noqa: E402  (seeded inputs / portable weights only)
from tfc_gan_amd import nets, parallel  # noqa: E402


def run(out_path, mode, config):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if mode == "rccl":
        os.environ["TFC_FORCE_COLLECTIVES"] = "1"
        try:
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{os.environ['TFC_TEST_PORT']}", rank=0, world_size=1)
            probe = torch.ones(4, device=dev)
            dist.all_reduce(probe)                                   # communicator creation happens here
            torch.cuda.synchronize()
        except Exception as e:                                       # no usable RCCL on this box: an environment problem, not a result (exit code 77 = skip)
            print("RCCL one-rank group unavailable:", repr(e), flush=True)
            sys.exit(77)
        assert parallel.collectives_active() and dist.get_backend() == "nccl"
    T.set_compute_dtype(torch.bfloat16)
    T.set_wgrad_stream(True)
    assert nets.side_stream_on()
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256), mask=config == "mask"), seed=61).to(dev)
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(dev)
    kw = dict(T.mask_weights(), mask=True) if config == "mask" else dict(T.region_weights("kl"), region_fft="kl")
    ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, bucket_bytes=16 << 20, patches=4, batch_scope="global", **kw)
    issued = {"all_reduce": 0, "all_gather": 0}
    if mode == "rccl":
        def counting(name):
            real = getattr(dist, name)

            def call(*a, **k):
                issued[name] += 1
                return real(*a, **k)
            return call
        parallel.dist.all_reduce, parallel.dist.all_gather = counting("all_reduce"), counting("all_gather")
    A, B = O.synthetic_pairs(2, seed=63)
    A, B = A.to(dev), B.to(dev)
    for _ in range(2):
        out = ts.step(A, B)
    torch.cuda.synchronize()
    sn = torch.cat([b.flatten() for b in ts.dbufs.values()])
    keys = sorted(k for k in out if out[k].numel() == 1)
    torch.save({"g": ts.gflat.data.cpu(), "d": ts.dflat.data.cpu(), "gm": ts.gm.cpu(), "gv": ts.gv.cpu(), "dm": ts.dm.cpu(), "dv": ts.dv.cpu(), "sn": sn.cpu(),
                "keys": keys, "loss": torch.stack([out[k].reshape(()).float() for k in keys]).cpu(),
                "buckets": torch.tensor(len(ts.g_reduce.buckets) + len(ts.d_reduce.buckets)),
                "all_reduce": torch.tensor(issued["all_reduce"]), "all_gather": torch.tensor(issued["all_gather"])}, out_path)
    if mode == "rccl":
        dist.destroy_process_group()
    print("worker done", mode, config, issued, flush=True)


if __name__ == "__main__":
    run(*sys.argv[1:4])
