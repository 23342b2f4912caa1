"""DarkVisibleStep (TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py) on one GPU: ms per step at batch 12 (the script's default) and 32, bf16, with the seeded
LPIPS term, for both localisers; and the four stride-2 convolutions (TFC_OP_CONV2) of the pix2pix discriminator one by one -- forward, input gradient
and weight gradient beside the least time the chip could take.

    python scripts/bench_darkvisible.py [--iters 20] [--warmup 5] [--layer-batch 32] [--out profiles/darkvisible_ab.md]

Every case runs in a child process of its own under a time limit (a case that faults or hangs ends the run there; nothing else is started on the GPU
after it). A step is timed between two device events, the figure is the median of --iters steps after --warmup. A convolution pass is timed by the
library's own event pairs around its launches (ops.prof_enable: a weight gradient is its kernels, slab reduction and finish pass together), median of
--iters calls after --warmup. The bf16 weight gradient is measured in both of its forms: the one launch of the transposed convolution's phase-fused
kernel with the two tensors exchanged (the default), and the four per-plane launches (TFC_CONV2_WGRAD_PLANES=1, what fp32 and bf16x3 run). Bounds,
priced as scripts/per_layer.py prices the other layers: MFMA = the pass's algorithmic FLOP (2 N OH OW Cin Cout 16) over 2.5 PFLOP/s dense bf16;
HBM = the bytes the pass has to move once (its two activation tensors in bf16 with the channel padding they are stored with, the packed weights, or
the fp32 gradient for the weight gradient) over the chip's 8.0 TB/s. Prints one JSON line; --out also writes the Markdown report."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 2.5e15
PEAK_BYTES = 8.0e12
LAYERS = ((256, 6, 64), (128, 64, 128), (64, 128, 256), (32, 256, 512))     # (H = W of the input, Cin, Cout) of model.0 / 2 / 5 / 8
STEP_BATCHES = (12, 32)
PASSES = ("fwd", "dgrad", "wgrad")


def pad8(c):
    return (c + 7) // 8 * 8


def bounds(N, H, Cin, Cout):
    """pass -> (flop, bytes): what the algorithm needs, from the shapes alone"""
    oh = H // 2
    flop = 2.0 * N * oh * oh * Cin * Cout * 16
    x, y, w = N * H * H * pad8(Cin) * 2, N * oh * oh * pad8(Cout) * 2, 16 * Cin * Cout
    return {"fwd": (flop, x + y + 2 * w), "dgrad": (flop, x + y + 2 * w), "wgrad": (flop, x + y + 4 * w)}


def case_step(batch, localiser, iters, warmup):
    import torch
    import tfc_gan_amd as T
    dev = torch.device("cuda", 0)
    T.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        crit = T.LPIPS().to(dev)
    st = T.DarkVisibleStep((3, 256, 256), lpips=crit, device=dev, seed=3, localiser=localiser)
    A, B = T.synthetic_pairs(batch, seed=1234)
    A, B = A.to(dev), B.to(dev)
    for _ in range(warmup):
        out = st.step(A, B)
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = st.step(A, B)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    losses = {k: float(v) for k, v in out.items() if v.dim() == 0}
    assert all(v == v and abs(v) != float("inf") for v in losses.values()), losses
    return {"ms": ms, "losses": losses, "peak_GB": torch.cuda.max_memory_allocated(dev) / 1e9}


def case_layer(index, batch, iters, warmup):
    import torch
    from tfc_gan_amd import ops
    dev = torch.device("cuda", 0)
    dt, op = ops.DT_BF16, ops.OP_CONV2
    H, Cin, Cout = LAYERS[index]
    g = torch.Generator(device=dev).manual_seed(index)
    x = ops.View(torch.randn((batch, H, H, pad8(Cin)), device=dev, generator=g).to(torch.bfloat16), Cin)
    dy = ops.View(torch.randn((batch, H // 2, H // 2, pad8(Cout)), device=dev, generator=g).to(torch.bfloat16), Cout)
    w = torch.randn((Cout, Cin, 4, 4), device=dev, generator=g) * 0.02
    bias = torch.zeros(Cout, device=dev)
    pf, pd = ops.pack_weight(dt, op, 0, w, Cin, Cout), ops.pack_weight(dt, op, 1, w, Cin, Cout)
    y, dx = ops.new_act(batch, H // 2, H // 2, pad8(Cout), dt, dev), ops.new_act(batch, H, H, pad8(Cin), dt, dev)
    y.C, dx.C = Cout, Cin
    dw = torch.empty_like(w)
    ws = [None]
    stats = torch.zeros((batch, Cout, 2), device=dev)

    def once():
        if index == 0:
            ops.conv_fwd(dt, op, x, Cin, Cout, pf, y, bias=bias, flags=ops.EP_LEAKY)       # block 1: bias + LeakyReLU in the epilogue
        else:
            ops.conv_fwd(dt, op, x, Cin, Cout, pf, y, bias=bias, stats=stats)              # blocks 2-4: bias + InstanceNorm statistics
        ops.conv_dgrad(dt, op, dy, batch, H, H, Cin, Cout, pd, dx)
        ws[0] = ops.conv_wgrad(dt, op, x, dy, Cin, Cout, dw, ws=ws[0])
    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    for _ in range(iters):
        once()
    torch.cuda.synchronize()
    recs = ops.prof_records()
    ops.prof_enable(False)
    per = {p: [] for p in PASSES}
    fin = []
    for r in recs:
        if r["pass"] == 3:
            fin.append(r["ms"])
        else:
            per[PASSES[r["pass"]]].append(r["ms"])
    if fin:                                                       # the finish pass belongs to its weight gradient
        assert len(fin) == len(per["wgrad"])
        per["wgrad"] = [a + b for a, b in zip(per["wgrad"], fin)]
    q = (ctypes_int_array(8))
    plans = {}
    for pas, flags in ((0, ops.EP_BIAS | (ops.EP_LEAKY if index == 0 else ops.EP_STATS)), (1, 0), (2, 0)):
        ops.lib().tfc_conv_plan_query(dt, op, pas, batch, H, H, Cin, Cout, flags, 256, q, 8)
        plans[PASSES[pas]] = list(q)
    return {"us": {p: [1e3 * v for v in per[p]] for p in PASSES}, "plans": plans}


def ctypes_int_array(n):
    import ctypes
    return (ctypes.c_int * n)()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layer-batch", type=int, default=32)
    ap.add_argument("--case-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: step,<batch>,<localiser> or layer,<index>,<batch> (one case, in this process)")
    args = ap.parse_args()
    assert args.iters >= 20, "the median wants at least 20 timed iterations"
    if args.case:
        kind, a, b = args.case.split(",")
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        r = case_step(int(a), b, args.iters, args.warmup) if kind == "step" else case_layer(int(a), int(b), args.iters, args.warmup)
        print("CASE " + json.dumps(r), flush=True)
        return
    layers = [f"layer,{i},{args.layer_batch}" for i in range(len(LAYERS))]
    cases = layers + [c + ",planes" for c in layers] + [f"step,{n},{loc}" for loc in ("hip", "torch") for n in STEP_BATCHES]
    res = {}
    for c in cases:
        env = dict(os.environ)
        env.pop("TFC_CONV2_WGRAD_PLANES", None)
        if c.endswith(",planes"):
            env["TFC_CONV2_WGRAD_PLANES"] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--case", c[:-7] if c.endswith(",planes") else c, "--iters", str(args.iters),
               "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout, env=env)
        if p.returncode != 0:
            raise SystemExit(f"case {c} ended with status {p.returncode}; nothing further is run")
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("CASE ")][-1][5:])
        if c.startswith("step"):
            v = sorted(r.pop("ms"))
            r.update(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1])
            print(f"{c}: {r['median_ms']:.2f} ms per step", file=sys.stderr, flush=True)
        else:
            us = r.pop("us")
            r["median_us"] = {p: statistics.median(us[p]) for p in PASSES}
            r["min_us"] = {p: min(us[p]) for p in PASSES}
            print(f"{c}: " + ", ".join(f"{p} {r['median_us'][p]:.1f} us" for p in PASSES), file=sys.stderr, flush=True)
        res[c] = r
    line = {"metric": "DarkVisibleStep, bf16, batch 12, HIP localiser, seeded LPIPS", "unit": "ms per step", "higher_is_better": False,
            "value": res["step,12,hip"]["median_ms"], "iters": args.iters, "warmup": args.warmup, "layer_batch": args.layer_batch, "cases": res}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(line))


KERNELS = {0: "tfc_igemm_kernel", 1: "tfc_igemm2_kernel", 3: "tfc_conv_c8_kernel", 10: "tfc_wgrad_kernel x4",
           11: "tfc_wgrad22_kernel x4", 13: "tfc_wgrad_kernel<bf16x3> x4", 15: "tfc_wgradT_kernel<NH=1>", 16: "tfc_wgradT_kernel<NH=2>"}


def report(r):
    c, nb = r["cases"], r["layer_batch"]
    out = ["# DarkVisibleStep and the stride-2 convolutions (scripts/bench_darkvisible.py)", "",
           f"One MI355X, bf16, 256 x 256 synthetic pairs, seeded LPIPS. Every case is a process of its own; median of {r['iters']} iterations after "
           f"{r['warmup']} warm-up (min .. max beside it).", "",
           "## The step (`tfc_gan_amd.DarkVisibleStep`, patch 16 localiser = 257 tokens)", "",
           "| batch | localiser | ms per step | peak device memory |", "|---|---|---|---|"]
    for loc in ("hip", "torch"):
        for n in STEP_BATCHES:
            v = c[f"step,{n},{loc}"]
            out.append(f"| {n} | {loc} | {v['median_ms']:.2f} ({v['min_ms']:.2f} .. {v['max_ms']:.2f}) | {v['peak_GB']:.1f} GB |")
    out += ["", f"## The four `TFC_OP_CONV2` layers of the pix2pix discriminator at batch {nb}", "",
            "us = the library's event pairs around the launches of one call (a weight gradient: its kernels, their slab reductions and the "
            "finish pass). MFMA bound = algorithmic FLOP / 2.5 PFLOP/s, HBM bound = bytes moved once / 8.0 TB/s; `x bound` = us over the larger of the two.", "",
            "| layer | pass | kernel (form) | us | GFLOP | MB | MFMA bound us | HBM bound us | binds | x bound |", "|---|---|---|---|---|---|---|---|---|---|"]
    for i, (H, Cin, Cout) in enumerate(LAYERS):
        v = c[f"layer,{i},{nb}"]
        b = bounds(nb, H, Cin, Cout)
        for p, src in (("fwd", v), ("dgrad", v), ("wgrad", v), ("wgrad", c[f"layer,{i},{nb},planes"])):
            flop, byt = b[p]
            tm, th = flop / PEAK_FLOPS * 1e6, byt / PEAK_BYTES * 1e6
            us = src["median_us"][p]
            plan = src["plans"][p]
            kern = KERNELS.get(plan[0], str(plan[0])) + (f" (form {plan[1]})" if plan[1] >= 0 else "") + (f", split {plan[3]}" if p == "wgrad" else "")
            name = p if src is v else "wgrad, per-plane launches"
            out.append(f"| {Cin} -> {Cout} at {H} x {H} | {name} | {kern} | {us:.1f} | {flop / 1e9:.1f} | {byt / 1e6:.1f} | {tm:.1f} | {th:.1f} | "
                       f"{'MFMA' if tm >= th else 'HBM'} | {us / max(tm, th):.1f} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
