"""What the GPU evaluation metrics cost: all five (PSNR, SSIM in both window forms, Bhattacharyya, NCC, MI) for 32 pairs of 256 x 256 images.

    python scripts/bench_eval_metrics.py [--pairs 32] [--reps 30] [--warmup 5] [--no-host]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_eval_metrics.py --reps 5 --no-host      # per-kernel times

The GPU figure is the median over --reps repetitions of the time between two events on the stream around ONE EvalAccumulator-style set (psnr and
bhattacharyya on the RGB images, ssim 7 x 7, ssim 7 x 1, ncc and mi on their gray versions; the inputs are already on the device, nothing is read
back). The host figure is the numpy / scipy restatement of the same set (tests/eval_metrics_ref.py) on the CPU of the same host, once. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy / scipy timing")
    args = ap.parse_args()

    import numpy as np
    import torch
    from tfc_gan_amd import metrics as M
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(3)
    real_np = rng.integers(0, 256, (args.pairs, 256, 256, 3), dtype=np.uint8)
    fake_np = np.clip(real_np.astype(np.int16) + rng.integers(-20, 21, real_np.shape), 0, 255).astype(np.uint8)
    real, fake = torch.from_numpy(real_np).cuda(), torch.from_numpy(fake_np).cuda()
    rg, fg = M.to_gray(real), M.to_gray(fake)

    def gpu_set():
        return [M.psnr(real, fake), M.ssim(rg, fg), M.ssim(rg, fg, columns_as_channels=True), M.bhattacharyya(real, fake), M.ncc(rg, fg),
                M.mutual_information(rg, fg)]

    for _ in range(args.warmup):
        gpu_set()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = gpu_set()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    res = {"pairs": args.pairs, "shape": [256, 256], "reps": args.reps, "gpu_ms_median": statistics.median(times), "gpu_ms_min": min(times),
           "gpu_ms_max": max(times), "means": {k: float(v.mean()) for k, v in zip(("psnr", "ssim", "ssim_columns", "bhattacharyya", "ncc", "mi"), out)}}
    if not args.no_host:
        from tests import eval_metrics_ref as R
        rgn, fgn = rg.cpu().numpy(), fg.cpu().numpy()
        t0 = time.perf_counter()
        for i in range(args.pairs):
            R.psnr(real_np[i], fake_np[i])
            R.ssim_2d(rgn[i], fgn[i])
            R.ssim_columns(rgn[i], fgn[i])
            R.bhattacharyya(real_np[i], fake_np[i])
            R.ncc(rgn[i], fgn[i])
            R.mutual_information(R.joint_hist(rgn[i], fgn[i]))
        res["host_numpy_scipy_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
