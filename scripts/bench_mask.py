"""The edge-mask step (MASK-4) beside PATCH-4, and the mask operator's kernels on their own: batch 32, bf16, synthetic pairs, one GPU, one process.

    python scripts/bench_mask.py [--steps 20] [--warmup 5] [--batch 32] [--repeats 3] [--iters 50] [--stats-csv kernel_stats.csv] [--out profiles/mask_ab.md]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_mask.py --kernels-only        (a run of its own: the per-kernel times)

Calls: device events around `--iters` calls of each entry point (after a warm-up), over a ring of 8 input sets (8 x 25 MB of images plus the
operator's planes: past the 256 MiB Infinity Cache); bytes are what the algorithm has to move, computed from the shapes below, and TB/s is set
against the 6.3 TB/s DESIGN.md uses as achievable. One call is several launches (forward: Laplacian, finaliser, blur, finaliser; backward: dot,
finaliser, blur adjoint, finaliser, Laplacian adjoint), so the per-KERNEL times come from the profiler run: --stats-csv merges its kernel_stats.csv
(the rows of tfc_mask_* and tfc_pack_plane_kernel) into the report. Steps: setup, warm-up and timing as scripts/bench_debias.py (interleaved
repeats; the spread of the PATCH-4 repeats is the yardstick). PATCH-4 here runs the code path of the commit before MASK-4: a step without mask=True
launches none of the new kernels. `mask4_input_only` is MASK-4 with lambda_mask=0: the mask feeds the generator, its loss term is off.
Prints one JSON line; --out also writes the Markdown report."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def call_bytes(N, HW, es):
    """bytes each entry point has to move at batch N, HW pixels, es bytes per activation element; every plane is fp32"""
    img, plane = N * 3 * HW * 4, N * HW * 4
    fwd = (img + plane) + (plane + plane)                         # Laplacian: image in, lap out; blur: lap in, Bl out
    bwd = 2 * plane + (3 * plane + plane) + (2 * plane + img)     # dot: dout, Bl; blur adjoint: dout, Bl, lap in, dMn out; Laplacian adjoint: dMn, lap in, dimg out
    l1 = (3 * plane) + (3 * plane + plane) + (2 * plane + img)    # dot with the L1 form: Bl, ref in, dout out
    return {"mask_fwd": fwd, "mask_scale": 2 * plane, "mask_bwd": bwd, "mask_l1_loss": 2 * fwd + 2 * plane + l1,
            "pack_nhwc8_plane": img + plane + N * HW * 8 * es}


def read_stats(path):
    """rows of a rocprofv3 kernel_stats.csv that belong to mask.hip: name -> (calls, average us)"""
    out = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "tfc_mask_" in name or "tfc_pack_plane_kernel" in name:
            out[name.split("(")[0].replace("void ", "")] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--kernels-only", action="store_true", help="the entry points alone (for a profiler run); no steps, no report")
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --kernels-only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts

    import torch
    import tfc_gan_amd as T
    from tfc_gan_amd import ops
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.bfloat16)
    N, S, dt = args.batch, 256, ops.DT_BF16
    HW = S * S

    # ---- entry points ------------------------------------------------------------------------------------------------------------------------
    ring = 8
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.tanh(torch.randn(*s, device=dev, generator=g))  # noqa: E731
    imgs = [rnd(N, 3, S, S) for _ in range(ring)]
    douts = [torch.randn(N, 1, S, S, device=dev, generator=g) for _ in range(ring)]
    ctxs = [ops.mask_fwd(x) for x in imgs]
    refs = [ops.mask_scale(c) for c in ctxs]
    calls = {"mask_fwd": lambda i: ops.mask_fwd(imgs[i]),
             "mask_scale": lambda i: ops.mask_scale(ctxs[i]),
             "mask_bwd": lambda i: ops.mask_bwd(ctxs[i], dout=douts[i]),
             "mask_l1_loss": lambda i: T.mask_l1_loss(imgs[i], imgs[(i + 1) % ring], scale=0.5),
             "pack_nhwc8_plane": lambda i: ops.pack_nhwc8_plane(dt, imgs[i], ctxs[i].bl, ctxs[i].M)}
    need = call_bytes(N, HW, 2)
    timed = {}
    for name, fn in calls.items():
        for i in range(ring):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(args.iters):
            fn(k % ring)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / args.iters
        timed[name] = {"us": us, "bytes": need[name], "TB_per_s": need[name] / us * 1e-6, "share_of_6.3": need[name] / us * 1e-6 / HBM_TBS}
    if args.kernels_only:
        print(json.dumps({"calls": timed}), flush=True)
        return
    del imgs, douts, ctxs, refs
    torch.cuda.empty_cache()

    # ---- steps -------------------------------------------------------------------------------------------------------------------------------
    A, B = T.synthetic_pairs(N, seed=1234)
    A, B = A.to(dev), B.to(dev)
    configs = (("patch4", None), ("mask4", 0.5), ("mask4_input_only", 0.0))
    steps = {}
    for name, lam in configs:
        torch.manual_seed(42)
        G = T.GeneratorUNet((3, 256, 256), mask=lam is not None).to(dev)
        D = T.Discriminator1((3, 256, 256)).to(dev)
        G.apply(T.weights_init_normal)
        D.apply(T.weights_init_normal)
        kw = {} if lam is None else dict(T.mask_weights(), mask=True, lambda_mask=lam)
        ts = T.TrainStep(G, D, patches=4, **kw)
        steps[name] = lambda ts=ts: ts.step(A, B)
        for _ in range(args.warmup):
            steps[name]()
    torch.cuda.synchronize()
    rates, losses = {name: [] for name, _ in configs}, {}
    for _ in range(args.repeats):
        for name, _ in configs:
            steps[name]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = steps[name]()
            torch.cuda.synchronize()
            rates[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
            losses[name] = {k: float(v) for k, v in out.items() if v.numel() == 1}
    line = {"metric": "train step time, MASK-4 beside PATCH-4", "unit": "ms/step", "higher_is_better": False, "dtype": "bf16",
            "batch": N, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "calls": timed,
            "kernels": read_stats(args.stats_csv) if args.stats_csv else None}
    for name, _ in configs:
        r = sorted(rates[name])
        line[name] = {"ms_per_step": r[len(r) // 2], "min": r[0], "max": r[-1], "runs": rates[name], **losses[name]}
    line["value"] = line["mask4"]["ms_per_step"]
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(line))


def report(r):
    out = ["# The edge-mask step (MASK-4): entry points, kernels and step time (scripts/bench_mask.py)", "",
           f"One MI355X, one process, batch {r['batch']}, bf16, synthetic pairs. Entry points: device events around calls over a ring of 8 input sets "
           "(more than the 256 MiB Infinity Cache); bytes are what the algorithm has to move, computed from the shapes; the share is of the 6.3 TB/s "
           "DESIGN.md uses as achievable. One call is several launches, and the times include the allocation of the call's outputs.", "",
           "| entry point | us | MB moved | TB/s | share of 6.3 TB/s |", "|---|---|---|---|---|"]
    for k, v in r["calls"].items():
        out.append(f"| `{k}` | {v['us']:.1f} | {v['bytes'] / 1e6:.1f} | {v['TB_per_s']:.2f} | {100 * v['share_of_6.3']:.0f} % |")
    if r["kernels"]:
        out += ["", "Per kernel, from a `rocprofv3 --kernel-trace --stats` run of `--kernels-only` (a run of its own; average over its calls):", "",
                "| kernel | calls | us |", "|---|---|---|"]
        for k, (calls, us) in sorted(r["kernels"].items()):
            out.append(f"| `{k}` | {calls} | {us:.1f} |")
    else:
        out += ["", "Per-kernel times: not measured in this run (no --stats-csv)."]
    out += ["", f"Step time, ms ({r['repeats']} interleaved repeats of {r['steps']} steps after {r['warmup']} warm-up steps; median, min .. max). "
            "`patch4` launches none of the new kernels: it is the code path of the commit before MASK-4. `mask4_input_only` is MASK-4 with "
            "lambda_mask=0 (the mask of real_A feeds the generator, the loss term is off).", "",
            "| configuration | ms / step | min .. max |", "|---|---|---|"]
    for k in ("patch4", "mask4", "mask4_input_only"):
        out.append(f"| {k} | {r[k]['ms_per_step']:.2f} | {r[k]['min']:.2f} .. {r[k]['max']:.2f} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
