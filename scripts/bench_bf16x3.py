"""The bf16x3 compute mode on bench.py's step: PATCH-16, batch 32, synthetic pairs, one GPU, compute_dtype="bf16x3".

    python scripts/bench_bf16x3.py [--steps 20] [--warmup 5] [--batch 32] [--no-l1]

Setup, warm-up and timing follow bench.py's lean headline exactly (same seeds, same weights init, the GPU synchronised before and after the timed
steps); `generator_l1_vs_oracle` is bench.py's generator-L1 leg (oracle generator with init_weights_portable(seed=3), synthetic_pairs(1, seed=11))
run in bf16x3. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def generator_l1(dev):
    import torch
    import tfc_gan_amd as T
    from oracle import tfcgan_oracle as O
    A, _ = O.synthetic_pairs(1, seed=11)
    Gc = O.init_weights_portable(O.GeneratorUNet((3, 256, 256)), seed=3).eval()
    with torch.no_grad():
        want = Gc(A)
    G = T.GeneratorUNet((3, 256, 256))
    G.load_state_dict(Gc.state_dict())
    G.compute_dtype = "bf16x3"
    G = G.to(dev).eval()
    with torch.no_grad():
        got = G(A.to(dev)).cpu()
    return float((got - want).abs().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-l1", action="store_true", help="leave out generator_l1_vs_oracle (e.g. under a kernel-trace run)")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts

    import torch
    import tfc_gan_amd as T
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype("bf16x3")
    torch.manual_seed(42)
    G = T.GeneratorUNet((3, 256, 256)).to(dev)
    D = T.Discriminator1((3, 256, 256)).to(dev)
    G.apply(T.weights_init_normal)
    D.apply(T.weights_init_normal)
    ts = T.TrainStep(G, D, compute_dtype="bf16x3", fft_mode="patch")
    A, B = T.synthetic_pairs(args.batch, seed=1234)
    A, B = A.to(dev), B.to(dev)
    for _ in range(args.warmup):
        ts.step(A, B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = ts.step(A, B)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ms = elapsed * 1e3 / args.steps
    line = {"metric": "PATCH-16 train step throughput, bf16x3 compute mode", "value": args.batch * args.steps / elapsed, "unit": "images/s",
            "higher_is_better": True, "dtype": "bf16x3", "ms_per_step": ms, "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
            "loss_G": float(out["loss_G"]), "loss_D": float(out["loss_D"])}
    if not args.no_l1:
        line["generator_l1_vs_oracle"] = generator_l1(dev)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
