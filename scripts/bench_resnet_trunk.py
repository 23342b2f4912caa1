"""The residual trunk of CycleGAN's GeneratorResNet on one GPU, bf16 and fp32: the reflect-padded 3 x 3 convolution (TFC_OP_CONV3R) pass by pass at the
trunk's shape -- batch 32, 64 x 64, 256 -> 256 -- beside its zero-padded sibling TFC_OP_CONV3 and torch's F.conv2d on a reflect-padded tensor; and
GeneratorResNet((3, 256, 256), 9) forward + backward at batch 32 with the trunk on the HIP kernels against the trunk as torch layers.

    python scripts/bench_resnet_trunk.py [--iters 30] [--warmup 10] [--batch 32] [--out profiles/resnet_trunk_ab.md]

Every case runs in a child process of its own under a time limit (a case that faults or hangs ends the run there; nothing else is started on the GPU
after it). The two ops ALTERNATE inside one process (call for call, after a warm-up of every shape), and each such process is run TWICE: the distance
of the two medians is the run-to-run spread that a difference between the ops has to exceed. A convolution pass is timed by the library's own event
pairs around its launches (ops.prof_enable: the input gradient of TFC_OP_CONV3R is its gather GEMM and, listed separately, its fold pass; a weight
gradient is its kernels, slab reduction and finish pass together). torch's calls and the generator are timed between two device events. Share of
peak: the pass's algorithmic FLOP (2 N H W Cin Cout 9) over the dense MFMA peak of the mode (2.5 PFLOP/s bf16, 157.3 TFLOP/s fp32), as
profiles/r02_per_layer.md reports it. Prints one JSON line; --out also writes the Markdown report."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {"bf16": 2.5e15, "fp32": 157.3e12}
H = W = 64
C = 256
MODES = ("bf16", "fp32")
CONV_KEYS = ("conv3r fwd", "conv3r dgrad gemm", "conv3r dgrad fold", "conv3r wgrad", "conv3 fwd", "conv3 dgrad")
TORCH_KEYS = ("torch fwd", "torch dgrad", "torch wgrad")
GEN_TRUNKS = {"bf16": ("hip", "torch-blocks", "torch"), "fp32": ("hip", "torch")}


def _events(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def case_conv(mode, batch, iters, warmup):
    """both ops, alternating: the trunk's call forms (bias + InstanceNorm statistics forward, plain input gradient, weight gradient)"""
    import torch
    from tfc_gan_amd import ops
    dev = torch.device("cuda", 0)
    dt = ops.DT_BF16 if mode == "bf16" else ops.DT_F32
    g = torch.Generator(device=dev).manual_seed(7)
    td = ops.torch_dtype(dt)
    x = ops.View(torch.randn((batch, H, W, C), device=dev, generator=g).to(td), C)
    dy = ops.View(torch.randn((batch, H, W, C), device=dev, generator=g).to(td), C)
    w = torch.zeros((C, C, 4, 4), device=dev)
    w[:, :, :3, :3] = torch.randn((C, C, 3, 3), device=dev, generator=g) * 0.02
    bias = torch.zeros(C, device=dev)
    y, dx = ops.new_act(batch, H, W, C, dt, dev), ops.new_act(batch, H, W, C, dt, dev)
    dw = torch.empty_like(w)
    stats = torch.zeros((batch, C, 2), device=dev)
    packed = {(op, pas): ops.pack_weight(dt, op, pas, w, C, C) for op in (ops.OP_CONV3R, ops.OP_CONV3) for pas in (0, 1)}
    ws = [None]

    def once():
        for op in (ops.OP_CONV3R, ops.OP_CONV3):
            ops.conv_fwd(dt, op, x, C, C, packed[op, 0], y, bias=bias, stats=stats)
            ops.conv_dgrad(dt, op, dy, batch, H, W, C, C, packed[op, 1], dx)
        ws[0] = ops.conv_wgrad(dt, ops.OP_CONV3R, x, dy, C, C, dw, ws=ws[0])
    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    for _ in range(iters):
        once()
    torch.cuda.synchronize()
    recs = ops.prof_records(16 * iters)
    ops.prof_enable(False)
    name = {(ops.OP_CONV3R, 0): "conv3r fwd", (ops.OP_CONV3R, 1): "conv3r dgrad gemm", (ops.OP_CONV3R, 4): "conv3r dgrad fold",
            (ops.OP_CONV3R, 2): "conv3r wgrad", (ops.OP_CONV3R, 3): "conv3r wgrad", (ops.OP_CONV3, 0): "conv3 fwd", (ops.OP_CONV3, 1): "conv3 dgrad"}
    us = {k: [] for k in CONV_KEYS}
    fin = []
    for r in recs:
        if r["pass"] == 3:
            fin.append(1e3 * r["ms"])
        else:
            us[name[r["op"], r["pass"]]].append(1e3 * r["ms"])
    if fin:                                                       # the finish pass belongs to its weight gradient
        assert len(fin) == len(us["conv3r wgrad"])
        us["conv3r wgrad"] = [a + b for a, b in zip(us["conv3r wgrad"], fin)]
    assert all(len(v) == iters for v in us.values()), {k: len(v) for k, v in us.items()}
    import ctypes
    q = (ctypes.c_int * 8)()
    plans = {}
    for key, op, pas, flags in (("conv3r fwd", ops.OP_CONV3R, 0, ops.EP_BIAS | ops.EP_STATS), ("conv3r dgrad gemm", ops.OP_CONV3R, 1, 0),
                                ("conv3r wgrad", ops.OP_CONV3R, 2, 0), ("conv3 fwd", ops.OP_CONV3, 0, ops.EP_BIAS | ops.EP_STATS),
                                ("conv3 dgrad", ops.OP_CONV3, 1, 0)):
        ops.lib().tfc_conv_plan_query(dt, op, pas, batch, H, W, C, C, flags, 256, q, 8)
        plans[key] = list(q)
    return {"us": us, "plans": plans}


def case_torch(mode, batch, iters, warmup):
    """F.conv2d on an already reflect-padded NCHW tensor and its two gradients (aten.convolution_backward, one output at a time)"""
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    td = torch.bfloat16 if mode == "bf16" else torch.float32
    g = torch.Generator(device=dev).manual_seed(7)
    xp = F.pad(torch.randn((batch, C, H, W), device=dev, generator=g), (1, 1, 1, 1), mode="reflect").to(td)
    w = (torch.randn((C, C, 3, 3), device=dev, generator=g) * 0.02).to(td)
    b = torch.zeros(C, device=dev, dtype=td)
    dy = torch.randn((batch, C, H, W), device=dev, generator=g).to(td)
    bwd = torch.ops.aten.convolution_backward
    args = ([C], [1, 1], [0, 0], [1, 1], False, [0, 0], 1)
    fns = {"torch fwd": lambda: F.conv2d(xp, w, b), "torch dgrad": lambda: bwd(dy, xp, w, *args, [True, False, False]),
           "torch wgrad": lambda: bwd(dy, xp, w, *args, [False, True, False])}
    return {"us": {k: [1e3 * v for v in _events(fn, iters, warmup)] for k, fn in fns.items()}}


def case_gen(mode, trunk, batch, iters, warmup):
    """GeneratorResNet((3, 256, 256), 9) forward + backward. trunk="hip": the compute mode `mode`, stem and head fp32 torch layers. trunk="torch": fp32, or
    torch.autocast(bfloat16) over the whole module as the reference's AMP runs it. trunk="torch-blocks" (bf16 only): the all-torch module with autocast
    around the residual blocks alone and the stem and head in fp32 -- the like-for-like partner of the bf16 hip trunk."""
    import contextlib
    import torch
    import tfc_gan_amd as T
    dev = torch.device("cuda", 0)
    T.set_compute_dtype(torch.bfloat16 if mode == "bf16" else torch.float32)
    torch.manual_seed(0)
    G = T.GeneratorResNet((3, 256, 256), 9, trunk="hip" if trunk == "hip" else "torch").to(dev)
    G.apply(T.weights_init_normal)
    x = torch.randn((batch, 3, 256, 256), device=dev)
    go = torch.randn((batch, 3, 256, 256), device=dev) * 1e-3
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if (trunk == "torch" and mode == "bf16") else contextlib.nullcontext()

    first, end = T.models.RESNET_TRUNK_FIRST, T.models.RESNET_TRUNK_FIRST + 9

    def forward():
        if trunk != "torch-blocks":
            with amp:
                return G(x)
        h = T.models._run_layers(G.model[:first], x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = T.models._run_layers(G.model[first:end], h)
        return T.models._run_layers(G.model[end:], h.float())

    def once():
        G.zero_grad(set_to_none=True)
        forward().float().backward(go)
    ms = _events(once, iters, warmup)
    gw = G.model[10].block[1].weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all())
    return {"ms": ms, "peak_GB": torch.cuda.max_memory_allocated(dev) / 1e9}


def _stat(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--case-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: conv,<mode>,<repeat> | torch,<mode>,0 | gen,<mode>,<trunk> (one case, in this process)")
    args = ap.parse_args()
    assert args.iters >= 20, "the median wants at least 20 timed iterations"
    if args.case:
        kind, mode, c = args.case.split(",")
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        if kind == "conv":
            r = case_conv(mode, args.batch, args.iters, args.warmup)
        elif kind == "torch":
            r = case_torch(mode, args.batch, args.iters, args.warmup)
        else:
            r = case_gen(mode, c, args.batch, max(20, args.iters // 2), max(3, args.warmup // 2))
        print("CASE " + json.dumps(r), flush=True)
        return
    cases = [f"conv,{m},{rep}" for m in MODES for rep in (0, 1)] + [f"torch,{m},0" for m in MODES]
    cases += [f"gen,{m},{t}" for m in MODES for t in GEN_TRUNKS[m]]
    res = {}
    for c in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", c, "--iters", str(args.iters), "--warmup", str(args.warmup), "--batch", str(args.batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)
        if p.returncode != 0:
            raise SystemExit(f"case {c} ended with status {p.returncode}; nothing further is run")
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("CASE ")][-1][5:])
        if c.startswith("gen"):
            r.update(_stat(r.pop("ms")))
            print(f"{c}: {r['median']:.1f} ms forward + backward", file=sys.stderr, flush=True)
        else:
            r["us"] = {k: _stat(v) for k, v in r["us"].items()}
            print(f"{c}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in r["us"].items()), file=sys.stderr, flush=True)
        res[c] = r
    line = {"metric": f"TFC_OP_CONV3R forward, bf16, batch {args.batch}, 64 x 64, 256 -> 256", "unit": "us per call", "higher_is_better": False,
            "value": res["conv,bf16,0"]["us"]["conv3r fwd"]["median"], "iters": args.iters, "warmup": args.warmup, "batch": args.batch, "cases": res}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(line))


KERNELS = {0: "tfc_igemm_kernel", 1: "tfc_igemm2_kernel", 10: "tfc_wgrad_kernel", 13: "tfc_wgrad_kernel<bf16x3>"}


def report(r):
    c, nb = r["cases"], r["batch"]
    flop = 2.0 * nb * H * W * C * C * 9
    out = ["# The residual trunk of GeneratorResNet (scripts/bench_resnet_trunk.py)", "",
           f"One MI355X. Every case is a process of its own; median of {r['iters']} calls after {r['warmup']} warm-up calls (min .. max beside it). The two "
           "convolution ops alternate call for call inside one process, and that process is run twice (run A, run B): the distance of the two medians is "
           "the run-to-run spread.", "",
           f"## One convolution at batch {nb}, {H} x {W}, {C} -> {C} ({flop / 1e9:.1f} GFLOP per pass)", "",
           "us = the library's event pairs around the launches of one call (forward with bias + InstanceNorm statistics; a weight gradient: kernel, slab "
           "reduction and finish pass). torch = F.conv2d on the already reflect-padded NCHW tensor / aten.convolution_backward, between two device "
           "events. Share = algorithmic FLOP over the mode's dense MFMA peak (2.5 PFLOP/s bf16, 157.3 TFLOP/s fp32) over the median of run A.", "",
           "| mode | pass | kernel (form) | run A us | run B us | TFLOP/s | share of peak |", "|---|---|---|---|---|---|---|"]
    for m in MODES:
        a, b = c[f"conv,{m},0"], c[f"conv,{m},1"]
        for k in CONV_KEYS:
            va, vb = a["us"][k], b["us"][k]
            plan = a["plans"].get(k)
            kern = "fold pass (elementwise)" if plan is None else KERNELS.get(plan[0], str(plan[0])) + (f" (form {plan[1]})" if plan[1] >= 0 else "") + \
                (f", split {plan[3]}" if k.endswith("wgrad") else "")
            rate = "" if plan is None else f"{flop / (va['median'] * 1e-6) / 1e12:.0f}"
            share = "" if plan is None else f"{flop / (va['median'] * 1e-6) / PEAK[m]:.3f}"
            out.append(f"| {m} | {k} | {kern} | {va['median']:.1f} ({va['min']:.1f} .. {va['max']:.1f}) | {vb['median']:.1f} ({vb['min']:.1f} .. {vb['max']:.1f}) | "
                       f"{rate} | {share} |")
        t = c[f"torch,{m},0"]["us"]
        for k in TORCH_KEYS:
            v = t[k]
            out.append(f"| {m} | {k} | MIOpen through torch | {v['median']:.1f} ({v['min']:.1f} .. {v['max']:.1f}) | | {flop / (v['median'] * 1e-6) / 1e12:.0f} | "
                       f"{flop / (v['median'] * 1e-6) / PEAK[m]:.3f} |")
    out += ["", "### Reflect against zero padding", "",
            "| mode | pass | conv3r - conv3, run A | run B | spread of conv3 (run A - run B) | spread of conv3r |", "|---|---|---|---|---|---|"]
    for m in MODES:
        a, b = c[f"conv,{m},0"]["us"], c[f"conv,{m},1"]["us"]
        for kr, kz in (("conv3r fwd", "conv3 fwd"), ("conv3r dgrad gemm", "conv3 dgrad")):
            out.append(f"| {m} | {kz.split()[1]} | {a[kr]['median'] - a[kz]['median']:+.1f} us | {b[kr]['median'] - b[kz]['median']:+.1f} us | "
                       f"{a[kz]['median'] - b[kz]['median']:+.1f} us | {a[kr]['median'] - b[kr]['median']:+.1f} us |")
    out += ["", f"## GeneratorResNet((3, 256, 256), 9), forward + backward at batch {nb}", "",
            "trunk=hip: the residual blocks in the compute mode of the row, stem and head as fp32 torch layers. trunk=torch: every layer a torch layer, in "
            "fp32, or with the WHOLE module under torch.autocast(bfloat16) in the bf16 row (the reference trains under AMP; its stem and head then run in "
            "bf16 too). trunk=torch-blocks: the all-torch module with autocast around the residual blocks alone, stem and head in fp32 -- what the bf16 "
            "hip trunk replaces, like for like.", "",
            "| mode | trunk | ms forward + backward | peak device memory |", "|---|---|---|---|"]
    for m in MODES:
        for t in GEN_TRUNKS[m]:
            v = c[f"gen,{m},{t}"]
            out.append(f"| {m} | {t} | {v['median']:.1f} ({v['min']:.1f} .. {v['max']:.1f}) | {v['peak_GB']:.1f} GB |")
    out += ["", "## The two conditions", ""]
    for m in MODES:
        a, b = c[f"conv,{m},0"]["us"], c[f"conv,{m},1"]["us"]
        diff = [x["conv3r fwd"]["median"] - x["conv3 fwd"]["median"] for x in (a, b)]
        spread = max(abs(a[k]["median"] - b[k]["median"]) for k in ("conv3 fwd", "conv3r fwd"))
        holds = max(diff) <= spread
        out.append(f"- {m}, reflect forward no dearer than its zero-padded sibling beyond the run-to-run spread: "
                   f"{'HOLDS' if holds else 'DOES NOT HOLD'} (conv3r - conv3 = {diff[0]:+.1f} / {diff[1]:+.1f} us = "
                   f"{100 * diff[0] / a['conv3 fwd']['median']:+.1f} % / {100 * diff[1] / b['conv3 fwd']['median']:+.1f} %, spread {spread:.1f} us).")
        extra = a["conv3r dgrad gemm"]["median"] + a["conv3r dgrad fold"]["median"] - a["conv3 dgrad"]["median"]
        out.append(f"  The input gradient (padded grid + fold pass) costs {extra:+.1f} us ({100 * extra / a['conv3 dgrad']['median']:+.0f} %) over the "
                   "zero-padded one: the padded grid has 9 x 5 tiles per image where the image has 8 x 4.")
        for t in GEN_TRUNKS[m][1:]:
            h, v = c[f"gen,{m},hip"]["median"], c[f"gen,{m},{t}"]["median"]
            out.append(f"- {m}, the hip trunk beats trunk={t}: {'HOLDS' if h < v else 'DOES NOT HOLD'} ({h:.1f} ms against {v:.1f} ms, x{v / h:.2f}).")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
