"""A/B of everything nets.py, models.py and the step engines drive, between two checkouts: the bits of what they compute, and the sequence of
library launches they issue.

    python scripts/ab_net_cores.py --dump FILE.npz [--trace FILE.json]     run the cases; raw bytes of every result (of one above 1 MiB: the
                                                                           BLAKE2b digest of its bytes) / every launch
    python scripts/ab_net_cores.py --compare A B [--unstable A2]           exact comparison of two dumps (.npz) or two traces (.json); no GPU

Cases: the stand-alone UNetDown / UNetUp (norm, no norm, dropout, 3 input channels), GeneratorUNet / Discriminator1 / Pix2PixDiscriminator through
autograd, the label / mask / auxiliary-head forwards, two TrainStep.step calls of seven configurations with the side stream on and off, one
STN21Step.step and one DarkVisibleStep.step. Run --dump / --trace from the root of each checkout (the script imports the package of the directory
it lies in; it uses only names both checkouts have) and compare the files.

--trace wraps the library handle in a recorder: for every tfc_* call whose first argument is a stream it notes the entry point, whether that
stream is the side stream of nets.py or the caller's, and every integer and float argument -- no pointers. Of a TrainStep configuration the second
step is recorded. Equal traces mean the same launches with the same arguments on the same streams in the same order, which a comparison of
results cannot show.

--compare A B --unstable A2: A2 is a second dump of A's checkout. An array that differs between A and A2 is not reproducible there; it is named
and left out, and it may only belong to the two STN steps (library GEMMs under autograd). Exit status 1 when anything else differs."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
BIG = 1 << 20                                                    # bytes; a larger array is dumped as its digest
STEP_CONFIGS = {                                                  # name -> (compute dtype, TrainStep keywords, generator keywords, aux heads)
    "bf16": ("bf16", {}, {}, False),
    "fp32": ("fp32", {}, {}, False),
    "bf16x3": ("bf16x3", {}, {}, False),
    "patch4": ("bf16", {"patches": 4}, {}, False),
    "patch4_labels": ("bf16", {"patches": 4, "labels": "generated"}, {"labels": 3}, True),
    "patch4_mask": ("bf16", {"patches": 4, "mask": True}, {"mask": True}, False),
    "patch4_kl": ("bf16", {"patches": 4, "region_fft": "kl"}, {}, False),
}


def rnd(shape, seed, scale=1.0):
    import numpy as np
    import torch
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def torch_dtype(name):
    import torch
    return {"bf16": torch.bfloat16, "fp32": torch.float32, "bf16x3": "bf16x3"}[name]


class Recorder:
    """stands in for the library handle: tfc_* calls that take a stream are noted in `self.sections` while `self.on` names a section"""

    def __init__(self, lib):
        self._lib, self.on, self.sections = lib, None, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tfc_"):
            return fn

        def call(*args):
            if self.on is not None and args and isinstance(args[0], ctypes.c_void_p):
                from tfc_gan_amd import nets
                side = {st.cuda_stream for st in nets._SIDE["streams"].values()}
                vals = [("ptr" if isinstance(a, int) and abs(a) >= 1 << 40 else a) for a in args[1:] if isinstance(a, (bool, int, float))]
                self.sections[self.on].append([name, "side" if args[0].value in side else "caller", vals])
            return fn(*args)
        return call

    def section(self, name):
        self.on = name
        if name is not None:
            self.sections[name] = []


def install_recorder():
    from tfc_gan_amd import _lib, ops
    rec = Recorder(_lib.load())
    _lib.load = lambda: rec                                        # ops.lib() and the modules that load the handle themselves
    ops.lib = lambda: rec
    return rec


class Out:
    def __init__(self, rec):
        self.arrays, self.rec = {}, rec

    def put(self, name, t):
        import torch
        if isinstance(t, (tuple, list)):
            for i, v in enumerate(t):
                self.put(f"{name}.{i}", v)
        elif t is not None:
            raw = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy()
            if raw.nbytes > BIG:                                  # flat parameter buffers, images: the digest of the raw bytes stands for them
                import hashlib
                import numpy as np
                self.arrays[name + ".blake2b"] = np.frombuffer(hashlib.blake2b(raw).digest() + str(tuple(t.shape)).encode(), dtype=np.uint8)
            else:
                self.arrays[name] = raw

    def section(self, name):
        if self.rec is not None:
            import torch
            torch.cuda.synchronize()
            self.rec.section(name)


def blocks(out):
    """stand-alone UNetDown / UNetUp at the sizes of test_blocks_vs_reference_goldens, bf16 and fp32"""
    import torch
    import tfc_gan_amd as T
    from oracle import tfcgan_oracle as O
    for dname in ("bf16", "fp32"):
        T.set_compute_dtype(torch_dtype(dname))
        cases = [("down_norm", T.UNetDown(8, 16), [(2, 8, 16, 16)], False),
                 ("down_nonorm", T.UNetDown(8, 16, normalize=False), [(2, 8, 15, 15)], False),
                 ("down_dropout", T.UNetDown(8, 16, dropout=0.5), [(2, 8, 16, 16)], True),
                 ("down_cin3", T.UNetDown(3, 16), [(2, 3, 16, 16)], False),
                 ("up", T.UNetUp(16, 8), [(2, 16, 7, 7), (2, 8, 14, 14)], False),
                 ("up_dropout", T.UNetUp(16, 8, dropout=0.5), [(2, 16, 7, 7), (2, 8, 14, 14)], True)]
        for i, (tag, mod, shapes, train) in enumerate(cases):
            O.init_weights_portable(mod, 21 + i)
            mod = mod.to(DEV).train(train)
            object.__setattr__(mod, "_drop_seed", 1234 + i)
            xs = [rnd(s, 40 + i + j).to(DEV).requires_grad_(True) for j, s in enumerate(shapes)]
            out.section(f"block.{dname}.{tag}")
            y = mod(*xs)
            y.backward(rnd(tuple(y.shape), 60 + i).to(DEV))
            out.section(None)
            out.put(f"block.{dname}.{tag}", [y, xs[0].grad, next(mod.parameters()).grad])


def modules(out):
    """the three networks through autograd at N = 2 (output, input gradient, every parameter gradient), and the forwards that have no autograd"""
    import torch
    import tfc_gan_amd as T
    from oracle import tfcgan_oracle as O
    for dname in ("bf16", "fp32"):
        T.set_compute_dtype(torch_dtype(dname))
        nets_ = [("generator", T.GeneratorUNet((3, 128, 128)), [(2, 3, 128, 128)]),
                 ("discriminator", T.Discriminator1((3, 64, 64)), [(2, 3, 64, 64)] * 2),
                 ("pix2pix", T.Pix2PixDiscriminator((3, 32, 48)), [(2, 3, 32, 48)] * 2)]
        for i, (tag, mod, shapes) in enumerate(nets_):
            O.init_weights_portable(mod, 71 + i)
            mod = mod.to(DEV).train()
            object.__setattr__(mod, "_drop_seed", 4321 + i)
            xs = [rnd(s, 80 + i + j, 0.5).to(DEV) for j, s in enumerate(shapes)]
            xs[0].requires_grad_(True)
            out.section(f"module.{dname}.{tag}")
            y = mod(*xs)
            y.backward(rnd(tuple(y.shape), 90 + i, 1e-2).to(DEV))
            out.section(None)
            out.put(f"module.{dname}.{tag}.out", y)
            out.put(f"module.{dname}.{tag}.gx", xs[0].grad)
            for k, p in mod.named_parameters():
                out.put(f"module.{dname}.{tag}.grad.{k}", p.grad)
    T.set_compute_dtype(torch.bfloat16)
    x, x2 = rnd((2, 3, 128, 128), 101, 0.5).to(DEV), rnd((2, 3, 128, 128), 102, 0.5).to(DEV)
    with torch.no_grad():
        for tag, mod, args in (("generator_labels", T.GeneratorUNet((3, 128, 128), labels=3), (x, torch.tensor([[1.0, 3.0, 2.0], [0.0, 1.0, 0.0]]).to(DEV))),
                               ("generator_mask", T.GeneratorUNet((3, 128, 128), mask=True), (x, rnd((2, 1, 128, 128), 103).abs().to(DEV))),
                               ("discriminator_aux", T.Discriminator1((3, 128, 128), aux_classes=(2, 4, 3)), (x, x2))):
            O.init_weights_portable(mod, 110)
            mod = mod.to(DEV).eval()
            object.__setattr__(mod, "_drop_seed", 999)
            out.section(f"module.bf16.{tag}")
            y = mod(*args)
            out.section(None)
            out.put(f"module.bf16.{tag}.out", y)


def train_steps(out):
    """two TrainStep.step calls at N = 2, 256 x 256 of every configuration, side stream on and off"""
    import numpy as np
    import torch
    import tfc_gan_amd as T
    from oracle import tfcgan_oracle as O
    A, B = (t.to(DEV) for t in T.synthetic_pairs(2, seed=5))
    labels = np.array([[1, 3, 2], [0, 1, 0]], dtype=np.int64)
    for side in (True, False):
        prev = T.nets.set_wgrad_stream(side)
        for name, (dname, kw, gkw, aux) in STEP_CONFIGS.items():
            tag = f"step.{name}.{'side' if side else 'one_stream'}"
            T.set_compute_dtype(torch_dtype(dname))
            G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256), **gkw), seed=3).to(DEV)
            D = O.init_weights_portable(T.Discriminator1((3, 256, 256), aux_classes=(2, 4, 3) if aux else None), seed=4).to(DEV)
            ts = T.TrainStep(G, D, compute_dtype=torch_dtype(dname), seed=7, **kw)
            skw = {"labels": labels} if aux else {}
            for step in (1, 2):
                if step == 2:
                    out.section(tag)
                res = ts.step(A, B, **skw)
                torch.cuda.synchronize()
                out.section(None)
                for k, v in res.items():
                    out.put(f"{tag}.{step}.{k}", v)
            for k, v in (("gflat", ts.gflat.data), ("dflat", ts.dflat.data), ("gm", ts.gm), ("gv", ts.gv), ("dm", ts.dm), ("dv", ts.dv)):
                out.put(f"{tag}.{k}", v)
            for k, v in ts.dbufs.items():
                out.put(f"{tag}.{k}", v)
            del ts, G, D
            print(tag, flush=True)
        T.nets.set_wgrad_stream(prev)
    T.set_compute_dtype(torch.bfloat16)


def stn_steps(out):
    """one STN21Step.step and one DarkVisibleStep.step, lpips=None, localiser="torch", 256 x 256"""
    import torch
    import tfc_gan_amd as T
    T.set_compute_dtype(torch.bfloat16)
    A, B = (t.to(DEV) for t in T.synthetic_pairs(2, seed=21))
    for tag, cls in (("stn21", T.STN21Step), ("darkvisible", T.DarkVisibleStep)):
        torch.manual_seed(7)
        st = cls((3, 256, 256), lpips=None, device=DEV, seed=3, localiser="torch")
        out.section(f"step.{tag}")
        res = st.step(A, B)
        torch.cuda.synchronize()
        out.section(None)
        for k, v in res.items():
            out.put(f"{tag}.{k}", v)
        for k, v in (("gflat", st.gflat.data), ("dflat", st.dflat.data), ("gm", st.gm), ("gv", st.gv), ("dm", st.dm), ("dv", st.dv)):
            out.put(f"{tag}.{k}", v)
        for D, dn in ((st.D1, "D1"), (st.D2, "D2")):
            for k, v in D.named_core_buffers().items():
                out.put(f"{tag}.{dn}.{k}", v)
        del st
        print(tag, flush=True)


def run(dump_path, trace_path):
    import numpy as np
    rec = install_recorder() if trace_path else None
    out = Out(rec)
    for part in (blocks, modules, train_steps, stn_steps):
        part(out)
    for path in (dump_path, trace_path):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if dump_path:
        np.savez(dump_path, **out.arrays)
        print(f"{len(out.arrays)} arrays -> {dump_path}")
    if trace_path:
        with open(trace_path, "w") as f:
            json.dump(rec.sections, f)
        print(f"{sum(len(v) for v in rec.sections.values())} launches in {len(rec.sections)} sections -> {trace_path}")


def compare_traces(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    bad = 0
    for k in sorted(a):
        same = a[k] == b[k]
        first = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        print(f"{'equal  ' if same else 'DIFFERS'} {k}: {len(a[k])} / {len(b[k])} launches" + ("" if same else f", first difference at {first}: "
              f"{a[k][first] if first < len(a[k]) else None} / {b[k][first] if first < len(b[k]) else None}"))
        bad += not same
    print(f"{len(a) - bad} of {len(a)} sections equal, {sum(len(v) for v in a.values())} / {sum(len(v) for v in b.values())} launches")
    return 1 if bad else 0


def compare(a_path, b_path, unstable_path):
    if a_path.endswith(".json"):
        return compare_traces(a_path, b_path)
    import numpy as np
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    same = lambda x, y: x.shape == y.shape and np.array_equal(x, y)  # noqa: E731  raw bytes: -0 != +0, NaN == NaN
    unstable = []
    if unstable_path:
        a2 = np.load(unstable_path)
        unstable = [k for k in sorted(a.files) if not same(a[k], a2[k])]
        for k in unstable:
            print(f"not reproducible in the first checkout: {k}")
        wrong = [k for k in unstable if not k.startswith(("stn21.", "darkvisible."))]
        if wrong:
            print(f"NOT REPRODUCIBLE outside the STN steps: {wrong}")
            return 1
    keys = [k for k in sorted(a.files) if k not in unstable]
    bad = [k for k in keys if not same(a[k], b[k])]
    for k in bad:
        print(f"DIFFERS {k} {a[k].shape}")
    print(f"{len(keys) - len(bad)} of {len(keys)} arrays bit-identical ({len(unstable)} left out as not reproducible)")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--trace")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--unstable")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare, args.unstable)
    if args.dump or args.trace:
        run(args.dump, args.trace)
    return 0


if __name__ == "__main__":
    sys.exit(main())
