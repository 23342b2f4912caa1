"""CPU emulation of the order of operations of tfc_dft_rect_cols_kernel (csrc/losses.hip), with and without the removal of the column mean.

    python scripts/emulate_rect_cols.py [--batch 2] [--rows 100]

The kernel takes a direct H-point DFT of each of the 129 columns of row spectra: a sequential fp32 sum over y of R[y] * exp(-2 pi i ky y / H), the
factor read from a table of H entries rounded once from double. Before the sum it subtracts the column mean and returns the column sum at ky = 0
(DESIGN.md section 3.4). This script restates that sum in numpy float32, once as the kernel does it and once as a plain direct sum, and prints per
window what each deviates by from numpy's float64 rfft2: the figures the fixture test of tests/test_gpu_41_region.py bounds (amplitude
2e-6 * max + 2e-2, max(dphi * amp) <= 0.05). It is the record behind the extra pass; it runs no GPU code.

What it does not model: the row transform (taken in float64 and rounded to float32 once), fused multiply-adds, and the kernel's lane-strided order
of the column sum (numpy's pairwise float32 sum stands in; the kx = 0 column is integer-valued and exact either way)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def column_dft_fp32(R, remove_mean):
    """R: complex [H,129] row spectra. The kernel's column pass in float32: table exp(-2 pi i m / H) rounded once from double, index (ky * y) mod H,
    sequential sum over y; remove_mean: subtract sum/H first and put the sum back at ky = 0. Im = +0 at the self-conjugate bins. -> complex64 [H,129]"""
    f32 = np.float32
    H = R.shape[0]
    x, y = R.real.astype(f32), R.imag.astype(f32)
    m = np.arange(H)
    tc, ts = np.cos(2 * np.pi * m / H).astype(f32), (-np.sin(2 * np.pi * m / H)).astype(f32)
    sx, sy = x.sum(axis=0, dtype=f32), y.sum(axis=0, dtype=f32)
    if remove_mean:
        inv_h = f32(1.0) / f32(H)
        x, y = x - sx * inv_h, y - sy * inv_h
    ky = np.arange(H)
    re, im = np.zeros((H, R.shape[1]), f32), np.zeros((H, R.shape[1]), f32)
    for r in range(H):
        t = (ky * r) % H
        ex, ey = tc[t][:, None], ts[t][:, None]
        re = re + (x[r][None, :] * ex - y[r][None, :] * ey)
        im = im + (x[r][None, :] * ey + y[r][None, :] * ex)
    if remove_mean:
        re[0], im[0] = sx, sy
    for kx in (0, R.shape[1] - 1):
        im[0, kx] = 0.0
        if H % 2 == 0:
            im[H // 2, kx] = 0.0
    return re + 1j * im


def deviations(luma, remove_mean):
    """luma: uint8 [H,256] -> (max |amp - ref|, max(dphi * amp_ref), max amp_ref) of the emulated spectrum against numpy's float64 rfft2"""
    ref = np.fft.rfft2(luma.astype(np.float64))
    rows = np.fft.rfft(luma.astype(np.float64), axis=1).astype(np.complex64)
    got = column_dft_fp32(rows, remove_mean)
    a_ref = np.abs(ref)
    dphi = np.abs(np.arctan2(got.imag, got.real).astype(np.float64) - np.arctan2(ref.imag, ref.real))
    dphi = np.minimum(dphi, 2 * np.pi - dphi)
    return np.abs(np.abs(got) - a_ref).max(), (dphi * a_ref).max(), a_ref.max()


def main():
    from tests import patch4_ref as R4
    from tests import region_ref as RR
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--rows", type=int, default=100)
    args = ap.parse_args()
    fake, _ = RR.head_inputs(args.batch)
    print("| sample | rows | max amp | plain sum: amp error | plain sum: max(dphi * amp) | mean removed: amp error | mean removed: max(dphi * amp) |")
    print("|---|---|---|---|---|---|---|")
    for n in range(args.batch):
        for row0 in (0, args.rows):
            luma = np.asarray(R4.luma_of(fake[n][:, row0:row0 + args.rows, :256]))
            (a0, p0, mx), (a1, p1, _) = deviations(luma, False), deviations(luma, True)
            print(f"| {n} | {row0}..{row0 + args.rows - 1} | {mx:.4g} | {a0:.3e} | {p0:.3e} | {a1:.3e} | {p1:.3e} |")


if __name__ == "__main__":
    main()
