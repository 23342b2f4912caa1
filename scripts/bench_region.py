"""The regional FFT loss (TrainStep(patches=4, region_fft="l1" | "kl")) on one GPU: what it deviates by, what one call costs, what it adds to the step.

    python scripts/bench_region.py [--steps 20] [--warmup 5] [--batch 32] [--repeats 3] [--calls 50] [--out profiles/region_fft_ab.md]

1. deviations: regional_fft_components / regional_fft_loss against tests/golden/fft_region.npz (the reference's own values), the figures that
   tests/test_gpu_41_region.py bounds;
2. one call of each head at --batch (device events around --calls calls after a warm-up, --repeats windows);
3. the PATCH-4 step without the term and with each form, bf16, synthetic pairs: setup, warm-up and timing as scripts/bench_patch4.py, every
   configuration timed --repeats times, interleaved, so that the spread of the plain PATCH-4 repeats is the yardstick for the differences.
Prints one JSON line and writes the markdown record."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (("patch4", None), ("patch4_region_l1", "l1"), ("patch4_region_kl", "kl"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_fft_ab.md"))
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts

    import numpy as np
    import torch
    import tfc_gan_amd as T
    from tests import region_ref as RR
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.bfloat16)

    # 1. deviations against the reference's values
    g = np.load(os.path.join(ROOT, "tests", "golden", "fft_region.npz"))
    fake, _ = RR.head_inputs(1)
    amp, pha = T.regional_fft_components(fake.to(dev), "eyes")
    a_ref, p_ref = torch.from_numpy(g["amp_eyes0"]), torch.from_numpy(g["pha_eyes0"])
    dphi = (pha[0, 0].cpu() - p_ref).abs()
    dphi = torch.minimum(dphi, 2 * np.pi - dphi)
    dev_rows = [("eyes, sample 0: max abs(amp - ref)", (amp[0, 0].cpu() - a_ref).abs().max().item(), f"2e-6 * {a_ref.max().item():.4g} + 2e-2"),
                ("eyes, sample 0: max(dphi * amp)", (dphi * a_ref).max().item(), "0.05")]
    for kind, n in (("l1", 1), ("l1", 3), ("kl", 2), ("kl", 3)):
        fk, rl = RR.head_inputs(n)
        got = [float(v) for v in T.regional_fft_loss(fk.to(dev), rl.to(dev), kind)]
        want = [float(v) for v in g[f"{kind}_n{n}"]]
        dev_rows += [(f"{kind} N={n}: total, relative", abs(got[0] - want[0]) / want[0], "2e-4"),
                     (f"{kind} N={n}: amplitude part, relative", abs(got[1] - want[1]) / want[1], "1e-4" if kind == "l1" else "2e-4"),
                     (f"{kind} N={n}: phase part, absolute", abs(got[2] - want[2]), "2e-3")]

    # 2. one call of each head
    A, B = T.synthetic_pairs(args.batch, seed=1234)
    A, B = A.to(dev), B.to(dev)
    fake_b = torch.tanh(A * 1.5) * 0.999
    heads = {"regional_fft_loss l1": lambda: T.regional_fft_loss(fake_b, B, "l1"), "regional_fft_loss kl": lambda: T.regional_fft_loss(fake_b, B, "kl"),
             "patch_fft_loss patches=4 (for scale)": lambda: T.patch_fft_loss(fake_b, B, 4)}
    head_ms = {}
    for name, fn in heads.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) / args.calls)
        head_ms[name] = sorted(runs)

    # 3. the step
    steps = {}
    for name, region in CONFIGS:
        torch.manual_seed(42)
        G = T.GeneratorUNet((3, 256, 256)).to(dev)
        D = T.Discriminator1((3, 256, 256)).to(dev)
        G.apply(T.weights_init_normal)
        D.apply(T.weights_init_normal)
        kw = T.region_weights(region) if region else {}
        steps[name] = T.TrainStep(G, D, patches=4, region_fft=region, **kw)
        for _ in range(args.warmup):
            steps[name].step(A, B)
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in CONFIGS}
    for _ in range(args.repeats):
        for name, _ in CONFIGS:
            ts = steps[name]
            ts.step(A, B)                                         # back on this configuration's buffers
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ts.step(A, B)
            torch.cuda.synchronize()
            rates[name].append(args.batch * args.steps / (time.perf_counter() - t0))

    line = {"metric": "train step throughput, PATCH-4 with and without the regional FFT loss", "unit": "images/s", "higher_is_better": True,
            "dtype": "bf16", "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "calls": args.calls,
            "head_ms": {k: v[len(v) // 2] for k, v in head_ms.items()}, "deviations": {k: v for k, v, _ in dev_rows}}
    for name, _ in CONFIGS:
        r = sorted(rates[name])
        line[name] = {"images_per_s": r[len(r) // 2], "min": r[0], "max": r[-1], "ms_per_step": 1e3 * args.batch / r[len(r) // 2], "runs": rates[name]}
    line["value"] = line["patch4_region_l1"]["images_per_s"]
    print(json.dumps(line), flush=True)

    md = ["# Regional FFT loss: deviations, head time, step A/B", "",
          f"`python scripts/bench_region.py --steps {args.steps} --warmup {args.warmup} --batch {args.batch} --repeats {args.repeats} --calls {args.calls}`"
          f" on one MI355X ({torch.cuda.get_device_properties(dev).gcnArchName}; the runtime's device name: {torch.cuda.get_device_name(dev)}),"
          " bf16 step, synthetic pairs, one process.", "",
          "## Deviations from the reference's own values (tests/golden/fft_region.npz)", "", "| quantity | measured | bound of the test |", "|---|---|---|"]
    md += [f"| {k} | {v:.3e} | {b} |" for k, v, b in dev_rows]
    md += ["", f"## One call at N = {args.batch} (device events around {args.calls} calls; median, min .. max of {args.repeats} windows)", "",
           "| head | ms per call |", "|---|---|"]
    md += [f"| {k} | {v[len(v) // 2]:.4f} ({v[0]:.4f} .. {v[-1]:.4f}) |" for k, v in head_ms.items()]
    md += ["", f"## PATCH-4 step, batch {args.batch} ({args.steps} steps per window, {args.repeats} windows per configuration, interleaved)", "",
           "| configuration | images/s (median) | min .. max | ms per step |", "|---|---|---|---|"]
    md += [f"| {name} | {line[name]['images_per_s']:.1f} | {line[name]['min']:.1f} .. {line[name]['max']:.1f} | {line[name]['ms_per_step']:.3f} |"
           for name, _ in CONFIGS]
    md += ["", "The spread of the plain `patch4` windows is the yardstick for the differences between the rows.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(md))


if __name__ == "__main__":
    main()
