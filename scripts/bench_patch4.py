"""The 4-patch configurations on bench.py's step: PATCH-4 and GLO-4 (TrainStep(patches=4), fft_mode "patch" / "global") beside PATCH-16, batch 32,
bf16, synthetic pairs, one GPU -- all measured in this one process on one card.

    python scripts/bench_patch4.py [--steps 20] [--warmup 5] [--batch 32] [--repeats 3]

Setup, warm-up and timing follow bench.py's lean headline (same seeds, same weights init, the GPU synchronised before and after the timed steps).
Every configuration is timed `--repeats` times, interleaved (16, 4-patch, 4-global, 16, ...), so that the spread of the PATCH-16 repeats is the
yardstick for the differences. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (("patch16", 16, "patch"), ("patch4", 4, "patch"), ("glo4", 4, "global"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts

    import torch
    import tfc_gan_amd as T
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.bfloat16)
    A, B = T.synthetic_pairs(args.batch, seed=1234)
    A, B = A.to(dev), B.to(dev)
    steps = {}
    for name, patches, mode in CONFIGS:
        torch.manual_seed(42)
        G = T.GeneratorUNet((3, 256, 256)).to(dev)
        D = T.Discriminator1((3, 256, 256)).to(dev)
        G.apply(T.weights_init_normal)
        D.apply(T.weights_init_normal)
        steps[name] = T.TrainStep(G, D, fft_mode=mode, patches=patches)
        for _ in range(args.warmup):
            steps[name].step(A, B)
    torch.cuda.synchronize()
    rates = {name: [] for name, _, _ in CONFIGS}
    losses = {}
    for _ in range(args.repeats):
        for name, _, _ in CONFIGS:
            ts = steps[name]
            ts.step(A, B)                                         # back on this configuration's buffers
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = ts.step(A, B)
            torch.cuda.synchronize()
            rates[name].append(args.batch * args.steps / (time.perf_counter() - t0))
            losses[name] = {k: float(out[k]) for k in ("loss_G", "loss_triplet_patch", "loss_FFT", "loss_D")}
    line = {"metric": "train step throughput, PATCH-4 / GLO-4 beside PATCH-16", "unit": "images/s", "higher_is_better": True, "dtype": "bf16",
            "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    for name, _, _ in CONFIGS:
        r = sorted(rates[name])
        line[name] = {"images_per_s": r[len(r) // 2], "min": r[0], "max": r[-1], "ms_per_step": 1e3 * args.batch / r[len(r) // 2], "runs": rates[name],
                      **losses[name]}
    line["value"] = line["patch4"]["images_per_s"]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
