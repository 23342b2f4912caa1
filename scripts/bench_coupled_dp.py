"""What the exchanges of the batch-coupled terms cost: the MASK-4 step and the KL regional step (batch 32, bf16, synthetic pairs, one GPU, one process).

    python scripts/bench_coupled_dp.py --mode plain [--tree DIR] [--label NAME] > a.json      no process group: both scopes are the unsplit launches
    python scripts/bench_coupled_dp.py --mode rccl > b.json                                     a ONE-rank "nccl" group, TFC_FORCE_COLLECTIVES=1
    python scripts/bench_coupled_dp.py --report a.json a2.json b.json --out profiles/coupled_dp_ab.md

--mode plain times TrainStep as it is called without a process group. --tree names another checkout of the package (the parent commit, built there) to
import instead of this one: run the two alternately, each run is a process of its own; the launches are the same and so are the bits (the losses of
the last step are in the JSON line), so the times should agree within the run-to-run spread, which the report shows.
--mode rccl creates the one-rank RCCL group of tests/rccl_world1_worker.py and times, in ONE process and interleaved, the same step with
batch_scope="shard" (the unsplit launches under the group) and batch_scope="global" (phases, eight all-gathers of 32 bytes per MASK-4 step, one of
619,200 bytes per KL step, and the merge kernels). A one-rank group moves nothing between GPUs: this is launch, stream hand-over and merge cost only.
Time between several GPUs is NOT measured by this script.
Setup, warm-up and timing as scripts/bench_mask.py: interleaved repeats of --steps steps, host clock around a synchronised block; median, min .. max.
Prints one JSON line."""
import argparse
import inspect
import json
import os
import sys
import time


def configs(T, which):
    out = {}
    if which in ("mask", "both"):
        out["mask4"] = (True, lambda: dict(T.mask_weights(), mask=True))
    if which in ("kl", "both"):
        out["kl4"] = (False, lambda: dict(T.region_weights("kl"), region_fft="kl"))
    return out


def measure(args):
    tree = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")               # as bench.py, before the HIP runtime starts
    import torch
    import torch.distributed as dist
    import tfc_gan_amd as T
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.mode == "rccl":
        os.environ["TFC_FORCE_COLLECTIVES"] = "1"
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{args.port}", rank=0, world_size=1)
        dist.all_reduce(torch.ones(4, device=dev))               # communicator creation happens here
        torch.cuda.synchronize()
        assert T.parallel.collectives_active()
    T.set_compute_dtype(torch.bfloat16)
    has_scope = "batch_scope" in inspect.signature(T.TrainStep.__init__).parameters
    scopes = ("shard", "global") if args.mode == "rccl" else (None,)
    A, B = T.synthetic_pairs(args.batch, seed=1234)
    A, B = A.to(dev), B.to(dev)
    steps = {}
    for name, (mask, kw) in configs(T, args.config).items():
        for scope in scopes:
            torch.manual_seed(42)
            G = T.GeneratorUNet((3, 256, 256), mask=True).to(dev) if mask else T.GeneratorUNet((3, 256, 256)).to(dev)
            D = T.Discriminator1((3, 256, 256)).to(dev)
            G.apply(T.weights_init_normal)
            D.apply(T.weights_init_normal)
            skw = {"batch_scope": scope} if (scope is not None and has_scope) else {}
            ts = T.TrainStep(G, D, patches=4, **kw(), **skw)
            key = name if scope is None else f"{name}_{scope}"
            steps[key] = lambda ts=ts: ts.step(A, B)
            for _ in range(args.warmup):
                steps[key]()
    torch.cuda.synchronize()
    rates, losses = {k: [] for k in steps}, {}
    for _ in range(args.repeats):
        for k, fn in steps.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = fn()
            torch.cuda.synchronize()
            rates[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            losses[k] = {n: float(v) for n, v in out.items() if v.numel() == 1}
    line = {"metric": "train step time of the batch-coupled 4-patch steps", "unit": "ms/step", "higher_is_better": False, "dtype": "bf16",
            "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "mode": args.mode,
            "label": args.label or ("this commit" if not args.tree else "other tree"), "has_batch_scope": has_scope, "runs": {}}
    for k, r in rates.items():
        s = sorted(r)
        line["runs"][k] = {"ms_per_step": s[len(s) // 2], "min": s[0], "max": s[-1], "all": r, "losses": losses[k]}
    line["value"] = next(iter(line["runs"].values()))["ms_per_step"]
    if args.mode == "rccl":
        dist.destroy_process_group()
    print(json.dumps(line), flush=True)


def report(paths, out_path):
    lines = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    plain, rccl = [r for r in lines if r["mode"] == "plain"], [r for r in lines if r["mode"] == "rccl"]
    first = lines[0]
    out = ["# The batch-coupled steps across data-parallel ranks: what the exchanges cost on one card (scripts/bench_coupled_dp.py)", "",
           f"One MI355X, one process per run, batch {first['batch']}, bf16, synthetic pairs; {first['repeats']} interleaved repeats of {first['steps']} steps "
           f"after {first['warmup']} warm-up steps; median, min .. max of the repeats, host clock around a synchronised block.", "",
           "**Time between several GPUs remains unmeasured.** Everything below ran on ONE card: a one-rank group moves no bytes between devices, so (b) "
           "shows the cost of issuing the gathers (launch, stream hand-over to RCCL's stream and back) and of the record / merge kernels, not of a "
           "network.", "",
           "## (a) No process group: the parent commit against this one", "",
           "Without active collectives `batch_scope` selects nothing: the step issues the launches of the parent commit, and the logged losses of the "
           "last timed step are compared below. The runs are processes of their own, alternated; the spread between two runs of the SAME tree is the "
           "yardstick for the difference between the trees.", "",
           "| run | tree | configuration | ms / step | min .. max |", "|---|---|---|---|---|"]
    for i, r in enumerate(plain):
        for k, v in r["runs"].items():
            out.append(f"| {i + 1} | {r['label']} | {k} | {v['ms_per_step']:.2f} | {v['min']:.2f} .. {v['max']:.2f} |")
    by = {}
    for r in plain:
        for k, v in r["runs"].items():
            by.setdefault(k, {}).setdefault(r["label"], []).append(v)
    for k, trees in by.items():
        if len(trees) == 2:
            (la, a), (lb, b) = trees.items()
            same = all(x["losses"] == a[0]["losses"] for x in a + b)
            med = lambda vs: sorted(x["ms_per_step"] for x in vs)[len(vs) // 2]  # noqa: E731
            spread = max(max(x["ms_per_step"] for x in vs) - min(x["ms_per_step"] for x in vs) for vs in (a, b))
            out += ["", f"`{k}`: {la} {med(a):.2f} ms, {lb} {med(b):.2f} ms (difference {med(b) - med(a):+.2f} ms; largest spread between runs of one tree "
                    f"{spread:.2f} ms). Logged losses of the last timed step {'bit-equal in every run of both trees' if same else 'DIFFER between runs'}."]
    out += ["", "## (b) One-rank RCCL group, `TFC_FORCE_COLLECTIVES=1`: `batch_scope=\"shard\"` against `\"global\"`", "",
            "Both scopes in one process, interleaved. `shard` issues the unsplit launches under the group (the gradient buckets and the loss average go "
            "through RCCL either way); `global` runs the phases: per MASK-4 step eight all-gathers of one 32-byte record each (two per mask forward of "
            "real_A, real_B and fake, two in the backward) and eight merge launches, per KL step one all-gather of 3 x 25,800 x 2 floats (619,200 bytes) "
            "and one merge launch.", "",
            "| configuration | scope | ms / step | min .. max |", "|---|---|---|---|"]
    for r in rccl:
        for k, v in r["runs"].items():
            name, scope = k.rsplit("_", 1)
            out.append(f"| {name} | {scope} | {v['ms_per_step']:.2f} | {v['min']:.2f} .. {v['max']:.2f} |")
        for name in sorted({k.rsplit("_", 1)[0] for k in r["runs"]}):
            s, g = r["runs"][f"{name}_shard"], r["runs"][f"{name}_global"]
            same = s["losses"] == g["losses"]
            out += ["", f"`{name}`: global - shard = {g['ms_per_step'] - s['ms_per_step']:+.2f} ms per step. With one rank the merged values are the shard's own: "
                    f"logged losses of the last timed step {'bit-equal between the scopes' if same else 'DIFFER between the scopes'}."]
    if not rccl:
        out += ["", "Not measured in this run."]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("plain", "rccl"), default="plain")
    ap.add_argument("--config", choices=("mask", "kl", "both"), default="both")
    ap.add_argument("--tree", default=None, help="another checkout of the package to import (the parent commit), built there")
    ap.add_argument("--label", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--port", type=int, default=29541)
    ap.add_argument("--report", nargs="+", default=None, help="JSON lines of earlier runs -> the Markdown report (no GPU needed)")
    ap.add_argument("--out", default="profiles/coupled_dp_ab.md")
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out)
    else:
        measure(args)


if __name__ == "__main__":
    main()
