"""A/B of the loss heads between two checkouts (bit identity of every array the heads produce, and what one call costs).

    python scripts/ab_loss_heads.py --dump FILE.npz        every array output of the cases below
    python scripts/ab_loss_heads.py --time FILE.json       one call of each head at N = 32
    python scripts/ab_loss_heads.py --compare A.npz B.npz  exact comparison of two dumps (no GPU)

Run --dump / --time from the root of each checkout (the script imports the package of the directory it lies in) and compare the files.
Dumped: patch_triplet gradients (grid 4 and 2, N = 1 and 3, gscale 1.0 / 0.5 / 3.0), fft_spectrum at (S, wx, wy) = (64, 4, 4), (128, 2, 2), (256, 1, 1)
with both shifts on the FFT and the direct-DFT path, fft_spectrum_rect at the six parameter rows of tests/test_gpu_41_region.py. The inputs are the fixed
synthetic images of the tests. The scalar losses are NOT dumped: they go through double atomics whose arrival order moves the last float bit between
two runs of one build; the tolerance tests cover them.
--time follows scripts/bench_region.py: device events around --calls calls after a warm-up, --repeats windows, median and min .. max."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEG16 = [3, 7, 0, 12, 9, 1, 15, 4, 4, 10, 2, 8, 13, 6, 11, 5]
NEG4 = [2, 0, 3, 1]
RECT_ROWS = [(100, 0, 100, 2, False, False), (100, 0, 100, 2, True, False), (7, 3, 0, 1, True, False), (6, 0, 250, 2, False, False),
             (2, 0, 0, 1, True, False), (100, 0, 100, 2, True, True)]          # H, row0, step, wins, shift, strided view


def dump(path):
    import numpy as np
    import torch
    from oracle import tfcgan_oracle as O
    from tests import patch4_ref as R4
    from tfc_gan_amd import ops
    dev = "cuda:0"
    out = {}
    for N in (1, 3):
        fk, rl = O.synthetic_pairs(N, seed=31)
        fk, rl = torch.tanh(fk * 1.5).to(dev), rl.to(dev)
        for grid, neg in ((4, NEG16), (2, NEG4)):
            for gs in (1.0, 0.5, 3.0):
                _, d = ops.patch_triplet(fk, rl, neg, want_grad=True, gscale=gs)
                out[f"triplet_grid{grid}_n{N}_gscale{gs}"] = d.cpu().numpy()
    x = R4.spectrum_inputs(3)
    big = torch.zeros(3, 3, 272, 512)
    big[:, :, 16:, 100:356] = x
    xd, view = x.to(dev), big.to(dev)[:, :, 16:, 100:356]
    for S, wx, wy in ((64, 4, 4), (128, 2, 2), (256, 1, 1)):
        for shift in (True, False):
            for direct in (False, True):
                amp, pha = ops.fft_spectrum(xd, S, wx, wy, shift=shift, direct=direct)
                tag = f"spectrum_s{S}_shift{int(shift)}_{'direct' if direct else 'fft'}"
                out[tag + "_amp"], out[tag + "_pha"] = amp.cpu().numpy(), pha.cpu().numpy()
    for i, (H, row0, step, wins, shift, strided) in enumerate(RECT_ROWS):
        amp, pha = ops.fft_spectrum_rect(view if strided else xd, H, row0, step, wins, shift=shift)
        out[f"rect{i}_h{H}_amp"], out[f"rect{i}_h{H}_pha"] = amp.cpu().numpy(), pha.cpu().numpy()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(a_path, b_path):
    import numpy as np
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    bad = []
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))     # bit patterns: -0 != +0, NaN == NaN
        print(f"{'equal  ' if same else 'DIFFERS'} {k} {a[k].shape}" + ("" if same else f" ({int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum())} elements)"))
        if not same:
            bad.append(k)
    print(f"{len(a.files) - len(bad)} of {len(a.files)} arrays bit-identical")
    return 1 if bad else 0


def time_heads(path, batch, calls, repeats):
    import torch
    import tfc_gan_amd as T
    from tfc_gan_amd import ops
    dev = torch.device("cuda", 0)
    A, B = T.synthetic_pairs(batch, seed=1234)
    A, B = A.to(dev), B.to(dev)
    fake = torch.tanh(A * 1.5) * 0.999
    neg16, neg4 = [(5 * k + 3) % 16 for k in range(16)], NEG4
    heads = {"patch_triplet 16 patches, with gradient": lambda: ops.patch_triplet(fake, B, neg16),
             "patch_triplet 4 patches, with gradient": lambda: ops.patch_triplet(fake, B, neg4),
             "patch_fft_loss patches=16": lambda: T.patch_fft_loss(fake, B, 16), "patch_fft_loss patches=4": lambda: T.patch_fft_loss(fake, B, 4),
             "global_fft_loss": lambda: T.global_fft_loss(fake, B),
             "regional_fft_loss l1": lambda: T.regional_fft_loss(fake, B, "l1"), "regional_fft_loss kl": lambda: T.regional_fft_loss(fake, B, "kl")}
    res = {}
    for name, fn in heads.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) / calls)
        res[name] = sorted(runs)
        print(f"{name}: {res[name][len(runs) // 2]:.4f} ms ({res[name][0]:.4f} .. {res[name][-1]:.4f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"batch": batch, "calls": calls, "repeats": repeats, "ms_per_call": res}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--time")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if args.dump:
        dump(args.dump)
    if args.time:
        time_heads(args.time, args.batch, args.calls, args.repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
