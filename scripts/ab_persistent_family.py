"""A/B of the persistent layer kernels between two checkouts (bit identity of their outputs, and what one call costs): tfc_conv_first_fwd with and
without sign words, tfc_upconv_head_fwd, tfc_conv_dgrad_image, tfc_upconv_head_dgrad.

    python scripts/ab_persistent_family.py --dump FILE.npz        the outputs at the shapes of test_persistent_layer_kernels_walk_tiles, default grid
    python scripts/ab_persistent_family.py --time FILE.json       one call of each entry point at the step's shapes (batch 32, 256 x 256 images)
    python scripts/ab_persistent_family.py --compare A.npz B.npz  exact comparison of two dumps (no GPU)

Run --dump / --time from the root of each checkout (the script imports the package of the directory it lies in) and compare the files.
--time follows scripts/ab_loss_heads.py: device events around --calls calls after a warm-up, --repeats windows, median and min .. max."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def rnd(shape, seed, scale=1.0):
    import numpy as np
    import torch
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def nhwc(x_nchw, pad_to=None):
    """NCHW fp32 CPU -> bf16 NHWC View on the GPU, channels zero-padded to a multiple of 8"""
    import torch
    from tfc_gan_amd import ops
    n, c, h, w = x_nchw.shape
    t = torch.zeros((n, h, w, pad_to or ops.pad8(c)), dtype=torch.float32)
    t[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return ops.View(t.to(DEV).to(torch.bfloat16).contiguous(), c)


def calls(N, first_hw, head_hw, sentinel=True):
    """entry point -> (function that runs it once, its destination tensors). first_hw: the image (input of the first convolution, result of its
    image gradient); head_hw: the 128-channel features the generator head reads."""
    import torch
    from tfc_gan_amd import _lib, ops
    dt = ops.DT_BF16
    full = torch.full if sentinel else (lambda shape, value, **kw: torch.empty(shape, **kw))
    (H, W), (hh, hw) = first_hw, head_hw
    out = {}
    # first convolution, Cin = 6 -> 64, bias + LeakyReLU
    xv = nhwc(rnd((N, 6, H, W), 5))
    w1 = rnd((64, 6, 4, 4), 6, 1.0 / 96 ** 0.5).to(DEV)
    pk = ops.pack_weight(dt, ops.OP_CONV, 0, w1, 6, 64)
    b1 = rnd((64,), 7, 0.5).to(DEV)
    for masked in (False, True):
        y = ops.View(full((N, H - 1, W - 1, 64), 7.0, dtype=torch.bfloat16, device=DEV), 64)
        mask = full((N, H - 1, W - 1, 8), 0xA5, dtype=torch.uint8, device=DEV) if masked else None
        out["conv_first_fwd" + ("_sign_mask" if masked else "")] = (
            lambda y=y, mask=mask: ops.conv_first_fwd(dt, xv, 6, 64, pk, y, bias=b1, flags=ops.EP_LEAKY, sign_mask=mask), [y.t] + ([mask] if masked else []))
    # generator head, 128 -> 3, tanh, NCHW
    hx = nhwc(rnd((N, 128, hh, hw), 8))
    wh = rnd((3, 128, 4, 4), 9, 0.02).to(DEV)
    bh = rnd((3,), 10, 0.1).to(DEV)
    img = full((N, 3, 2 * hh, 2 * hw), 7.0, dtype=torch.float32, device=DEV)
    out["upconv_head_fwd"] = (lambda: ops.upconv_head_fwd(dt, hx, wh, bh, img), [img])
    # D block 1, gradient w.r.t. the generated image
    gy = nhwc(rnd((N, 64, H - 1, W - 1), 11))
    wd = rnd((64, 6, 4, 4), 12, 0.1).to(DEV)
    osc = torch.tensor([0.41], device=DEV)
    gimg = full((N, 3, H, W), 7.0, dtype=torch.float32, device=DEV)
    out["conv_dgrad_image"] = (lambda: _lib.check(ops.lib().tfc_conv_dgrad_image(ops.stream_ptr(), dt, gy.ptr, gy.pitch, N, H, W, 6, 64, ops._p(wd), ops._p(osc),
                                                                                  3, ops._p(gimg)), "tfc_conv_dgrad_image"), [gimg])
    # input gradient of the generator head, into a 128-channel window of a 160-pitch buffer
    gh = nhwc(rnd((N, 3, 2 * hh, 2 * hw), 13))
    buf = full((N, hh, hw, 160), 3.0, dtype=torch.bfloat16, device=DEV)
    out["upconv_head_dgrad"] = (lambda: ops.upconv_head_dgrad(dt, gh, N, hh, hw, wh, ops.View(buf, 128, 0)), [buf])
    return out


def dump(path):
    import numpy as np
    import torch
    out = {}
    # the shapes of test_persistent_layer_kernels_walk_tiles (first convolution 24 x 40, its image gradient 20 x 40, heads 20 x 24), each for every entry
    for hw in ((24, 40), (20, 40), (20, 24)):
        for name, (fn, dst) in calls(2, hw, hw).items():
            fn()
            torch.cuda.synchronize()
            for i, t in enumerate(dst):
                out[f"{name}_{hw[0]}x{hw[1]}_{i}"] = t.contiguous().cpu().view(torch.uint8).numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(a_path, b_path):
    import numpy as np
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    bad = []
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k])                   # raw bytes: -0 != +0, NaN == NaN
        print(f"{'equal  ' if same else 'DIFFERS'} {k} {a[k].shape}")
        if not same:
            bad.append(k)
    print(f"{len(a.files) - len(bad)} of {len(a.files)} arrays bit-identical")
    return 1 if bad else 0


def time_calls(path, batch, ncalls, repeats):
    import torch
    res = {}
    for name, (fn, _) in calls(batch, (256, 256), (128, 128), sentinel=False).items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ncalls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) / ncalls)
        res[name] = sorted(runs)
        print(f"{name}: {res[name][len(runs) // 2]:.4f} ms ({res[name][0]:.4f} .. {res[name][-1]:.4f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"batch": batch, "calls": ncalls, "repeats": repeats, "ms_per_call": res}, f)


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
        time_calls(args.time, args.batch, args.calls, args.repeats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
