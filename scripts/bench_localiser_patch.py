"""The STN21 localiser at ViT patch 64 / 32 / 16 (17 / 65 / 257 tokens), "torch" beside "hip", and the tiled attention pair on its own beside the
same attention written as torch matmul + softmax with autograd (the form of stn21._Attention): batch 32, bf16 and fp32, one GPU.

    python scripts/bench_localiser_patch.py [--iters 20] [--warmup 5] [--batch 32] [--remarks build_stderr.txt] [--out profiles/localiser_patch_ab.md]

Every case runs in a child process of its own under a time limit (a case that faults or hangs ends the run there; nothing else is started on
the GPU after it). In a case the two sides alternate, iteration by iteration; each iteration is one forward + backward between two device events,
and the figure is the median of --iters iterations after --warmup. "torch" runs under bf16 autocast in the bf16 cases and in plain fp32 in the
fp32 cases. The localiser cases time Net.stn_phi (ViT + fc_loc) forward and backward to both images and every parameter.
--remarks: the compiler's stderr of a build (-Rpass-analysis=kernel-resource-usage); the tiled kernels' registers, scratch and occupancy are
copied from it into the report. Prints one JSON line; --out also writes the Markdown report."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATCHES = (64, 32, 16)
ATTN_T = (65, 257)
HEADS = 12


def timed_pair(fns, iters, warmup):
    """fns: name -> callable (one forward + backward). Alternates them; -> name -> list of ms"""
    import torch
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def case_localiser(dtype, patch, batch, iters, warmup):
    import torch
    import tfc_gan_amd as T
    from tfc_gan_amd import stn21
    dev = torch.device("cuda", 0)
    bf16 = dtype == "bf16"
    T.set_compute_dtype(torch.bfloat16 if bf16 else torch.float32)
    torch.manual_seed(0)
    nets = {"torch": stn21.Net((3, 256, 256), localiser="torch", patch_size=patch).to(dev)}
    nets["hip"] = copy.deepcopy(nets["torch"])                     # the same weights on both sides
    nets["hip"].localiser = "hip"
    A, B = T.synthetic_pairs(batch, seed=1234)
    A, B = A.to(dev).requires_grad_(True), B.to(dev).requires_grad_(True)
    g = torch.randn(batch, 2, 3, device=dev)

    def run(name):
        net = nets[name]
        net.zero_grad(set_to_none=True)
        A.grad = B.grad = None
        if name == "hip":
            from tfc_gan_amd import vit
            th = vit.stn_phi(net, A, B)
        else:
            with torch.autocast("cuda", torch.bfloat16, enabled=bf16):
                th = net.stn_phi(torch.cat((A, B), 1))
        (th.float() * g).sum().backward()
        return th
    ms = timed_pair({k: (lambda k=k: run(k)) for k in nets}, iters, warmup)
    th_h, th_t = run("hip").detach().float(), run("torch").detach().float()
    diff = ((th_h - th_t).norm() / th_t.norm()).item()
    return {"ms": ms, "theta_rel_diff": diff, "tokens": (256 // patch) ** 2 + 1}


def case_attention(dtype, Tt, batch, iters, warmup):
    import torch
    from tfc_gan_amd import ops
    dev = torch.device("cuda", 0)
    bf16 = dtype == "bf16"
    dt = ops.DT_BF16 if bf16 else ops.DT_F32
    H, D = HEADS, HEADS * 64
    gen = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(batch * Tt, 3 * D, device=dev, generator=gen)
    do = torch.randn(batch * Tt, D, device=dev, generator=gen)
    qkv_t = qkv.clone().requires_grad_(True)

    def hip():
        o, stats = ops.vit_attention_tiled_fwd(dt, qkv, batch, Tt, H, 0.125)
        return o, ops.vit_attention_tiled_bwd(dt, do, qkv, o, stats, batch, Tt, H, 0.125)

    def torch_side():
        qkv_t.grad = None
        with torch.autocast("cuda", torch.bfloat16, enabled=bf16):
            q, k, v = qkv_t.reshape(batch, Tt, 3, H, 64).permute(2, 0, 3, 1, 4)
            att = torch.softmax((q @ k.transpose(-2, -1)) * 0.125, dim=-1)
            o = (att @ v).transpose(1, 2).reshape(batch * Tt, D)
        o.backward(do.to(o.dtype))
        return o, qkv_t.grad
    ms = timed_pair({"torch": torch_side, "hip": hip}, iters, warmup)
    (oh, gh), (ot, gt) = hip(), torch_side()
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    return {"ms": ms, "out_rel_diff": rel(oh, ot), "dqkv_rel_diff": rel(gh, gt), "probs_MB": batch * H * Tt * Tt * 4 / 1e6,
            "stats_MB": batch * H * 3 * Tt * 4 / 1e6}


def parse_remarks(path):
    """the tiled kernels' rows of a -Rpass-analysis=kernel-resource-usage log: name -> {VGPRs, AGPRs, ScratchSize, Occupancy}"""
    out, name = {}, None
    keys = {"VGPRs:": "VGPRs", "AGPRs:": "AGPRs", "ScratchSize [bytes/lane]:": "scratch", "Occupancy [waves/SIMD]:": "occupancy"}
    for line in open(path):
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split("[")[0].strip()
            name = name if "tfc_vit_attn_tiled" in name else None
        elif name:
            for k, short in keys.items():
                if " " + k in line:
                    out.setdefault(name, {})[short] = int(line.split(k)[1].split("[")[0].strip())
    return out


def pretty(name):
    kind = "fwd" if "fwd" in name else ("dq" if "_dq_" in name else "dkv")
    return f"tfc_vit_attn_tiled_{kind}_kernel<{'bf16' if 'ILi0E' in name else 'fp32'}>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--case-timeout", type=int, default=240)
    ap.add_argument("--remarks", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: kind,dtype,size (one case, in this process)")
    args = ap.parse_args()
    assert args.iters >= 20, "the median wants at least 20 timed iterations"
    if args.case:
        kind, dtype, size = args.case.split(",")
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        fn = case_localiser if kind == "localiser" else case_attention
        print("CASE " + json.dumps(fn(dtype, int(size), args.batch, args.iters, args.warmup)), flush=True)
        return
    cases = [("attention", d, t) for d in ("bf16", "fp32") for t in ATTN_T] + [("localiser", d, p) for d in ("bf16", "fp32") for p in PATCHES]
    res = {}
    for kind, dtype, size in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{kind},{dtype},{size}", "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--batch", str(args.batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)      # a failed case ends the run: check=... below
        if p.returncode != 0:
            raise SystemExit(f"case {kind},{dtype},{size} ended with status {p.returncode}; nothing further is run")
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("CASE ")][-1][5:])
        for k in ("torch", "hip"):
            v = sorted(r["ms"][k])
            r[k] = {"median_ms": statistics.median(v), "min_ms": v[0], "max_ms": v[-1]}
        del r["ms"]
        res[f"{kind},{dtype},{size}"] = r
        print(f"{kind} {dtype} {size}: torch {r['torch']['median_ms']:.3f} ms, hip {r['hip']['median_ms']:.3f} ms", file=sys.stderr, flush=True)
    key = f"attention,bf16,{ATTN_T[-1]}"
    line = {"metric": "tiled attention fwd+bwd, bf16, T=257, batch 32", "unit": "ms", "higher_is_better": False, "value": res[key]["hip"]["median_ms"],
            "batch": args.batch, "iters": args.iters, "warmup": args.warmup, "cases": res,
            "resources": parse_remarks(args.remarks) if args.remarks else None}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report(line))


def report(r):
    c = r["cases"]
    out = ["# The localiser at ViT patch 64 / 32 / 16 and the tiled attention pair (scripts/bench_localiser_patch.py)", "",
           f"One MI355X, batch {r['batch']}, 256 x 256 synthetic pairs. Every case is a process of its own; in it the two sides alternate, one forward + "
           f"backward between two device events per iteration, median of {r['iters']} iterations after {r['warmup']} warm-up (min .. max beside it). "
           "`torch` runs under bf16 autocast in the bf16 rows and in plain fp32 in the fp32 rows.", "",
           "## The attention pair alone (N = 32, H = 12, head dim 64)", "",
           "`hip`: `ops.vit_attention_tiled_fwd` + `_bwd`. `torch`: matmul + softmax + matmul with autograd, the form of `stn21._Attention`, on the "
           "same `qkv` and `dout`. The T x T probabilities torch keeps for its backward against the statistics the tiled forward saves:", "",
           "| dtype | T | torch ms | hip ms | hip / torch | T x T tensor | saved statistics | out, dqkv rel. difference |", "|---|---|---|---|---|---|---|---|"]
    for d in ("bf16", "fp32"):
        for t in ATTN_T:
            v = c[f"attention,{d},{t}"]
            out.append(f"| {d} | {t} | {v['torch']['median_ms']:.3f} ({v['torch']['min_ms']:.3f} .. {v['torch']['max_ms']:.3f}) | "
                       f"{v['hip']['median_ms']:.3f} ({v['hip']['min_ms']:.3f} .. {v['hip']['max_ms']:.3f}) | "
                       f"{v['hip']['median_ms'] / v['torch']['median_ms']:.2f} | {v['probs_MB']:.1f} MB | {v['stats_MB']:.2f} MB | "
                       f"{v['out_rel_diff']:.1e}, {v['dqkv_rel_diff']:.1e} |")
    out += ["", "## The localiser (Net.stn_phi: ViT + fc_loc), forward + backward", "",
            "| dtype | patch | tokens | torch ms | hip ms | hip / torch | theta rel. difference |", "|---|---|---|---|---|---|---|"]
    for d in ("bf16", "fp32"):
        for p in PATCHES:
            v = c[f"localiser,{d},{p}"]
            out.append(f"| {d} | {p} | {v['tokens']} | {v['torch']['median_ms']:.2f} ({v['torch']['min_ms']:.2f} .. {v['torch']['max_ms']:.2f}) | "
                       f"{v['hip']['median_ms']:.2f} ({v['hip']['min_ms']:.2f} .. {v['hip']['max_ms']:.2f}) | "
                       f"{v['hip']['median_ms'] / v['torch']['median_ms']:.2f} | {v['theta_rel_diff']:.1e} |")
    out += ["", "## The tiled kernels' resources (the compiler's kernel-resource-usage remarks of the gfx950 build)", ""]
    if r["resources"]:
        out += ["| kernel | VGPRs | AGPRs | scratch bytes / lane | occupancy waves / SIMD |", "|---|---|---|---|---|"]
        for k, v in sorted(r["resources"].items(), key=lambda kv: pretty(kv[0])):
            out.append(f"| `{pretty(k)}` | {v['VGPRs']} | {v['AGPRs']} | {v['scratch']} | {v['occupancy']} |")
    else:
        out.append("Not recorded in this run (no --remarks).")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
