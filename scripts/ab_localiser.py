"""A/B of the STN21 localiser (Net.stn_phi forward + backward, input gradient included) at batch 32 on one GPU: the torch layers (fp32, the
default) against the HIP kernels in fp32 and in bf16, alternated round by round on the same box, with checksums of theta and of the input
gradient. python scripts/ab_localiser.py [batch] [rounds] [iters per round]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tfc_gan_amd as T  # noqa: E402
from tfc_gan_amd import stn21  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = stn21.Net((3, 256, 256)).to(dev)
A, B = T.synthetic_pairs(N, seed=3)
A, B = A.to(dev), B.to(dev).requires_grad_(True)
g = torch.randn(N, 2, 3, device=dev)
FLOP = 338e9 * N / 32                                             # forward + backward
modes = {"torch_fp32": ("torch", torch.float32), "hip_fp32": ("hip", torch.float32), "hip_bf16": ("hip", torch.bfloat16)}


def once(mode):
    loc, dtype = modes[mode]
    net.localiser = loc
    T.set_compute_dtype(dtype)
    B.grad = None
    th = net.stn_phi(torch.cat((A, B), 1)) if loc == "torch" else T.vit.stn_phi(net, A, B)
    (th * g).sum().backward()
    return th


times = {m: [] for m in modes}
sums = {}
for m in modes:                                                   # warm-up (kernel loads, library heuristics) and checksums
    th = once(m)
    torch.cuda.synchronize()
    sums[m] = (th.double().sum().item(), B.grad.double().abs().sum().item())
for r in range(rounds):
    for m in (modes if r % 2 == 0 else reversed(list(modes))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            once(m)
        torch.cuda.synchronize()
        times[m].append((time.perf_counter() - t0) / iters * 1e3)
T.set_compute_dtype(torch.bfloat16)
for m in modes:
    ts = sorted(times[m])
    med = ts[len(ts) // 2]
    print(f"{m:11s} batch {N}: median {med:7.2f} ms  (min {ts[0]:.2f}, max {ts[-1]:.2f})  {FLOP / med / 1e9:6.1f} TFLOP/s  "
          f"checksum theta {sums[m][0]:.6f}  |dB| {sums[m][1]:.6e}", flush=True)
