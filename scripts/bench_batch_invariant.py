"""What batch-invariant mode costs: bench.py's PATCH-16 step (bf16, synthetic pairs, one GPU) at batch 32, 8, 2 and 1 with the mode off and on.

    python scripts/bench_batch_invariant.py [--batches 32,8,2,1] [--rounds 3] [--steps 10] [--warmup 3]

One TrainStep per (batch, setting), same seeds and weights init as bench.py; the settings alternate inside every round (off, on, off, on, ...) so that
clock drift hits both alike, and the figure of a cell is the median over the rounds of the mean step time (the GPU synchronised before and after the
timed steps). At batch 32 the two settings run the same kernels with the same plans, so that row shows the run-to-run spread. Prints one JSON line."""
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
    ap.add_argument("--batches", default="32,8,2,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts

    import torch
    import tfc_gan_amd as T
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.bfloat16)
    rows = []
    for batch in [int(b) for b in args.batches.split(",")]:
        A, B = T.synthetic_pairs(batch, seed=1234)
        A, B = A.to(dev), B.to(dev)
        steps = {}
        for on in (False, True):
            torch.manual_seed(42)
            G = T.GeneratorUNet((3, 256, 256)).to(dev)
            D = T.Discriminator1((3, 256, 256)).to(dev)
            G.apply(T.weights_init_normal)
            D.apply(T.weights_init_normal)
            steps[on] = T.TrainStep(G, D, compute_dtype=torch.bfloat16, fft_mode="patch", batch_invariant=on)
            for _ in range(args.warmup):
                steps[on].step(A, B)
        ms = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    steps[on].step(A, B)
                torch.cuda.synchronize()
                ms[on].append((time.perf_counter() - t0) * 1e3 / args.steps)
        off, on_ = statistics.median(ms[False]), statistics.median(ms[True])
        rows.append({"batch": batch, "ms_off": off, "ms_on": on_, "ratio_on_over_off": on_ / off, "rounds_off": ms[False], "rounds_on": ms[True]})
        del steps
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "PATCH-16 train step, batch-invariant mode off / on", "unit": "ms per step", "dtype": "bf16", "steps": args.steps,
                      "warmup": args.warmup, "rounds": args.rounds, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
