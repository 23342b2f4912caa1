"""python -m tfc_gan_amd.evaluate --real DIR --fake DIR [--real-a DIR] [--csv OUT]

Scores a directory of generated images against a directory of targets on the GPU: one CSV row per image pair with psnr, ssim (7 x 7), ssim_columns
(the reference's literal 7 x 1 form), bhattacharyya, ncc and mi -- the numbers of the reference's evaluation_psnr_ssim.py, evaluation_bhatt.py,
calc_NCC.py and calc_MI.py. Files are paired by the numbers in their names (re.findall(r"\\d+", name), as the scripts merge them) and decoded with
PIL. psnr and bhattacharyya see the decoded image (RGB or gray); ssim, ncc and mi its gray version (metrics.to_gray: cv2's integer BGR2GRAY formula
restated, parity unpinned, exact for R = G = B). ncc and mi compare --real-a (default: --real) with --fake, so `--real real_A --fake reg_B` gives the
STN21 scripts' "after registration" numbers. Prints the per-metric means; --csv writes the table.
"""
import argparse
import csv
import os
import re
import sys

import numpy as np

COLUMNS = ("psnr", "ssim", "ssim_columns", "bhattacharyya", "ncc", "mi")


def numbered_files(directory):
    """{numbers in the file name: path} of the regular files of a directory"""
    out = {}
    for name in sorted(os.listdir(directory)):
        path = os.path.join(directory, name)
        if not os.path.isfile(path):
            continue
        key = tuple(int(s) for s in re.findall(r"\d+", os.path.splitext(name)[0]))
        if not key:
            continue
        if key in out:
            raise SystemExit(f"{directory}: {os.path.basename(out[key])} and {name} carry the same numbers {key}")
        out[key] = path
    return out


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB"):
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


def evaluate_dirs(real_dir, fake_dir, real_a_dir=None, batch=32):
    """rows (key, real path, fake path, {metric: value}) in key order"""
    import torch
    from . import metrics
    dirs = [numbered_files(real_dir), numbered_files(fake_dir)] + ([numbered_files(real_a_dir)] if real_a_dir else [])
    keys = sorted(set(dirs[0]).intersection(*dirs[1:]))
    if not keys:
        raise SystemExit("no file numbers are common to the directories")
    groups = {}                                                    # images of one shape share a batch
    for k in keys:
        imgs = [decode(d[k]) for d in dirs]
        if any(i.shape != imgs[0].shape for i in imgs):
            raise SystemExit(f"images numbered {k} differ in shape: {[i.shape for i in imgs]}")
        groups.setdefault(imgs[0].shape, []).append((k, imgs))
    rows = {}
    for items in groups.values():
        acc = metrics.EvalAccumulator()
        for i in range(0, len(items), batch):
            stacks = [torch.from_numpy(np.stack([it[1][j] for it in items[i:i + batch]])) for j in range(len(dirs))]
            acc.update(stacks[0], stacks[1], stacks[2] if real_a_dir else stacks[0])
        res = acc.result()
        for n, (k, _) in enumerate(items):
            rows[k] = {m: float(res[m]["values"][n]) for m in COLUMNS}
    return [(k, dirs[0][k], dirs[1][k], rows[k]) for k in keys]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tfc_gan_amd.evaluate", description=__doc__.split("\n\n")[1])
    ap.add_argument("--real", required=True, help="directory of target images (real_B)")
    ap.add_argument("--fake", required=True, help="directory of generated images (fake_B / reg_B)")
    ap.add_argument("--real-a", default=None, help="directory ncc / mi compare --fake with (default: --real)")
    ap.add_argument("--csv", default=None, help="write one row per image pair to this file")
    opt = ap.parse_args(argv)
    rows = evaluate_dirs(opt.real, opt.fake, opt.real_a)
    if opt.csv:
        with open(opt.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(("number", "real", "fake") + COLUMNS)
            for k, r, fk, vals in rows:
                w.writerow(["_".join(map(str, k)), os.path.basename(r), os.path.basename(fk)] + [repr(vals[m]) for m in COLUMNS])
    for m in COLUMNS:
        print(f"{m}: mean {np.mean([v[m] for *_, v in rows]):.6f} over {len(rows)} pairs")
    return 0


if __name__ == "__main__":
    sys.exit(main())
