"""The label-conditioned ("debiased") step beside PATCH-4, and its six kernels on their own: batch 32, bf16, synthetic pairs, one GPU, one process.

    python scripts/bench_debias.py [--steps 20] [--warmup 5] [--batch 32] [--repeats 3] [--iters 50] [--out profiles/debias_ab.md]

Kernels: device events around `--iters` launches (after a warm-up), over a ring of input sets larger than the 256 MiB Infinity Cache, so that the
time is a memory time and not a cache time; bytes are the bytes the algorithm has to move, computed from the shapes below, and TB/s is set against
the 6.3 TB/s DESIGN.md uses as achievable. Steps: setup, warm-up and timing as scripts/bench_patch4.py (interleaved repeats; the spread of the
PATCH-4 repeats is the yardstick). The un-fused down1 backward (the labelled generator needs the input gradient of down1, which turns the fused
first-block weight-gradient kernel off) is measured on the plain generator core: backward with and without need_input_grad.
Prints one JSON line; --out also writes the Markdown report."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3
LABELS = [[1, 3, 2], [0, 1, 0]]


def kernel_bytes(N, HW, es):
    """bytes each kernel has to move at batch N, HW pixels, es bytes per activation element (9 classes)"""
    x8, w, g3 = N * HW * 8 * es, 9 * 6 * HW * 4, N * 3 * HW * 4
    return {"pack_nhwc8_labels": N * 3 * HW * 4 + 4 * HW * 4 + x8, "label_plane_bwd": N * HW * 4 + 4 * HW * 4,
            "aux_heads_fwd": x8 + w, "softmax_ce_heads": N * 9 * 4 * 3, "aux_heads_dgrad": 2 * g3 + w // 2, "aux_heads_wgrad": 2 * x8 + w}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts

    import numpy as np
    import torch
    import tfc_gan_amd as T
    from tfc_gan_amd import nets, ops
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.set_compute_dtype(torch.bfloat16)
    N, S, dt = args.batch, 256, ops.DT_BF16
    HW = S * S

    # ---- kernels -------------------------------------------------------------------------------------------------------------------------
    ring = 8                                                      # 8 x (25 MB of input + 14 MB of weights) and more: past the Infinity Cache
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g) * 2 - 1  # noqa: E731
    imgs = [rnd(N, 3, S, S) for _ in range(ring)]
    x8s = [ops.pack_nhwc8(dt, rnd(N, 3, S, S), rnd(N, 3, S, S)) for _ in range(ring)]
    x8f = [ops.pack_nhwc8(dt, rnd(N, 3, S, S), rnd(N, 3, S, S)) for _ in range(ring)]
    wss = [[rnd(c, 6 * HW) * 0.002 for c in ops.AUX_CLASSES] for _ in range(ring)]
    dws = [[torch.empty(c, 6 * HW, device=dev) for c in ops.AUX_CLASSES] for _ in range(ring)]
    bs = [torch.zeros(c, device=dev) for c in ops.AUX_CLASSES]
    dbs = [torch.empty(c, device=dev) for c in ops.AUX_CLASSES]
    g4s, g3s = [rnd(N, 4, S, S) for _ in range(ring)], [rnd(N, 3, S, S) for _ in range(ring)]
    fcw, fcb = [rnd(HW, 3) for _ in range(ring)], [rnd(HW) for _ in range(ring)]
    dfw, dfb = torch.empty(HW, 3, device=dev), torch.empty(HW, device=dev)
    labels = torch.tensor(np.stack([np.arange(N) % c for c in ops.AUX_CLASSES], 1), dtype=torch.float32, device=dev)
    targets = labels.to(torch.int32)
    logits, dl = rnd(N, 9), rnd(N, 9) * 0.1
    calls = {"pack_nhwc8_labels": lambda i: ops.pack_nhwc8_labels(dt, imgs[i], labels, fcw[i], fcb[i]),
             "label_plane_bwd": lambda i: ops.label_plane_bwd(g4s[i], labels, dfw, dfb),
             "aux_heads_fwd": lambda i: ops.aux_heads_fwd(dt, x8s[i], wss[i], bs),
             "softmax_ce_heads": lambda i: ops.softmax_ce_heads(logits, targets),
             "aux_heads_dgrad": lambda i: ops.aux_heads_dgrad(g3s[i], wss[i], dl),
             "aux_heads_wgrad": lambda i: ops.aux_heads_wgrad(dt, x8s[i], dl, x8f[i], dl, dws[i], dbs)}
    need = kernel_bytes(N, HW, 2)
    kernels = {}
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
        kernels[name] = {"us": us, "bytes": need[name], "TB_per_s": need[name] / us * 1e-6, "share_of_6.3": need[name] / us * 1e-6 / HBM_TBS}
    del imgs, x8s, x8f, wss, dws, g4s, g3s, fcw, fcb
    torch.cuda.empty_cache()

    # ---- the un-fused down1 backward, on the plain generator ----------------------------------------------------------------------------------
    A, B = T.synthetic_pairs(N, seed=1234)
    A, B = A.to(dev), B.to(dev)
    torch.manual_seed(42)
    Gp = T.GeneratorUNet((3, 256, 256)).to(dev)
    Gp.apply(T.weights_init_normal)
    core = nets.GeneratorCore(dt, 3)
    core.set_params({k: p.detach() for k, p in Gp.named_core_params().items()})
    core.repack()
    grads = {k: torch.empty_like(p) for k, p in core.params.items()}
    gfake = torch.randn(N, 3, S, S, device=dev) * 1e-3
    down1 = {}
    for need_gx in (False, True, False, True):
        ts_ = []
        for it in range(4):
            _, gctx = core.forward(A, seed=1, train=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            core.backward(gctx, gfake, grads, need_input_grad=need_gx)
            torch.cuda.synchronize()
            if it:
                ts_.append(1e3 * (time.perf_counter() - t0))
        down1.setdefault("input_grad" if need_gx else "fused", []).append(sorted(ts_)[len(ts_) // 2])
    del core, grads, Gp

    # ---- steps -----------------------------------------------------------------------------------------------------------------------------------
    lab = np.stack([np.arange(N) % c for c in ops.AUX_CLASSES], 1)
    configs = (("patch4", None), ("debias_v1", "v1"), ("debias_v3", "v3"))
    steps = {}
    for name, kind in configs:
        torch.manual_seed(42)
        G = T.GeneratorUNet((3, 256, 256), labels=3 if kind else 0).to(dev)
        D = T.Discriminator1((3, 256, 256), aux_classes=(2, 4, 3) if kind else None).to(dev)
        G.apply(T.weights_init_normal)
        D.apply(T.weights_init_normal)
        ts = T.TrainStep(G, D, patches=4, **(T.debias_weights(kind) if kind else {}))
        steps[name] = (lambda ts=ts: ts.step(A, B, labels=lab)) if kind else (lambda ts=ts: ts.step(A, B))
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
    line = {"metric": "train step time, label-conditioned v1 / v3 beside PATCH-4", "unit": "ms/step", "higher_is_better": False, "dtype": "bf16",
            "batch": N, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "kernels": kernels, "down1_backward_ms": down1}
    for name, _ in configs:
        r = sorted(rates[name])
        line[name] = {"ms_per_step": r[len(r) // 2], "min": r[0], "max": r[-1], "runs": rates[name], **losses[name]}
    line["value"] = line["debias_v1"]["ms_per_step"]
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(line))


def report(r):
    out = ["# The label-conditioned step: kernels and step time (scripts/bench_debias.py)", "",
           f"One MI355X, one process, batch {r['batch']}, bf16, synthetic pairs. Kernels: device events around launches over a ring of 8 input sets "
           "(more than the 256 MiB Infinity Cache); bytes are what the algorithm has to move, computed from the shapes; the share is of the 6.3 TB/s "
           "DESIGN.md uses as achievable. `softmax_ce_heads` is one workgroup on 288 numbers: a launch, not a bandwidth.", "",
           "| kernel | us | MB moved | TB/s | share of 6.3 TB/s |", "|---|---|---|---|---|"]
    for k, v in r["kernels"].items():
        out.append(f"| `{k}` | {v['us']:.1f} | {v['bytes'] / 1e6:.1f} | {v['TB_per_s']:.2f} | {100 * v['share_of_6.3']:.0f} % |")
    out += ["", f"Step time, ms ({r['repeats']} interleaved repeats of {r['steps']} steps after {r['warmup']} warm-up steps; median, min .. max):", "",
            "| configuration | ms / step | min .. max |", "|---|---|---|"]
    for k in ("patch4", "debias_v1", "debias_v3"):
        out.append(f"| {k} | {r[k]['ms_per_step']:.2f} | {r[k]['min']:.2f} .. {r[k]['max']:.2f} |")
    d = r["down1_backward_ms"]
    out += ["", "Generator backward on the plain generator core, ms (host clock around one synchronised backward, median of 3, two rounds): "
            f"fused first-block weight gradient {d['fused'][0]:.2f} / {d['fused'][1]:.2f}; with need_input_grad=True (activation backward, weight gradient "
            f"and input gradient of down1 as separate kernels: what the labelled generator runs) {d['input_grad'][0]:.2f} / {d['input_grad'][1]:.2f}.", ""]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
