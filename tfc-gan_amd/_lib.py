"""ctypes binding of libtfcgan_hip.so (C ABI declared in include/tfc_gan.h).

The library is built in-tree with hipcc for gfx950 (``build()``); nothing here falls back to a CPU or PyTorch
implementation: if the shared object is missing or a call fails, a RuntimeError is raised.

The header is the only place where the ABI is written down: PROTOTYPES, the DT_* / OP_* / EP_* constants (and ops.py's VIT_* constants and
VitGemm fields) are parsed from it at import. A new entry point needs its declaration there, its definition in csrc/api.hip and its wrapper
in ops.py; nothing in this file changes.
"""
import ctypes
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(_HERE, "libtfcgan_hip.so")
SOURCES = ["api.hip", "igemm.hip", "elementwise.hip", "losses.hip", "stn.hip", "lpips.hip", "input.hip", "probe.hip", "vit.hip", "metrics.hip", "debias.hip", "mask.hip"]
HEADERS = ["common.h", "tfc_desc.h", "pack_math.h"]
PUBLIC_HEADER = os.path.join(_ROOT, "include", "tfc_gan.h")

_lock = threading.Lock()
_lib = None


def _stale():
    if not os.path.exists(SO_PATH):
        return True
    t = os.path.getmtime(SO_PATH)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [PUBLIC_HEADER]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 into tfc-gan_amd/libtfcgan_hip.so (cross-compiles without a GPU). Safe under `torch.distributed.run`:
    ranks that find the library stale take a file lock, ONE of them compiles, the others wait and load its result."""
    if not force and not _stale():
        return SO_PATH
    import fcntl
    try:
        lk = open(SO_PATH + ".lock", "w")
    except OSError:                                               # read-only tree: nothing to coordinate with
        return _build_locked(verbose)
    with lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if not force and not _stale():                        # another rank built it while this one waited
                return SO_PATH
            return _build_locked(verbose)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


def hipcc():
    path = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return path if os.path.exists(path) else "hipcc"


def _build_locked(verbose):
    cmd = [hipcc(),"--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
           "-Wl,-rpath,/opt/rocm/lib", "-Wl,-z,defs",             # -z defs: a launcher that is declared and called but defined nowhere fails the link
           "-o", SO_PATH + ".tmp"] + [os.path.join(CSRC, f) for f in SOURCES]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + "\n".join(l for l in res.stderr.splitlines() if "remark:" not in l)[-8000:])
    unmatched = unmatched_guards(res.stderr)
    if unmatched:
        raise RuntimeError("GUARDED_KERNELS entries that match no compiled kernel (renamed or removed? they guard nothing): " + ", ".join(unmatched))
    bad = check_no_spills(res.stderr)
    if bad:
        raise RuntimeError("hand-scheduled kernels must not spill (their asm loads carry hand-counted waits the compiler cannot see): " + "; ".join(bad))
    os.replace(SO_PATH + ".tmp", SO_PATH)
    return SO_PATH


# The K loops of tfc_igemm2_kernel and the weight-gradient kernels issue global_load / ds_read through asm volatile with hand-counted s_waitcnt: correct only
# while hipcc keeps their destination registers in place (no scratch, no VGPR spill) between the load and the wait. The compiler's resource remarks
# (-Rpass-analysis=kernel-resource-usage) are checked at every build, so a toolchain or flag change that makes one of them spill fails loudly here
# instead of silently producing wrong convolutions.
# The 4-patch loss heads (tfc_patch_triplet_kernel<2> with four float2 rows in flight, the 128-point FFT kernels) ride the same check: they were sized
# to run without scratch, and a spill there would be a silent slowdown of every PATCH-4 / GLO-4 step.
# So do the kernels of the rectangular-window spectra (the regional FFT loss): the rows kernel is tfc_fft_rows_kernel<256, true> (the row FFT of
# the square spectra with the checks of a ragged row count compiled in; "ILi256E" matches both 256-point instantiations), the columns kernel a 100 x 100 inner loop per output that was written to live in registers.
# Entries are substrings of the MANGLED names in the remarks; one that matches no compiled kernel fails the build (unmatched_guards).
GUARDED_KERNELS = ("tfc_igemm2_kernel", "tfc_wgrad", "tfc_patch_triplet_kernelILi2E", "tfc_fft_rows_kernelILi128E", "tfc_fft_rows_kernelILi256E",
                   "tfc_fft_cols_kernelILi128E", "tfc_spectrum_kernelILi128E", "tfc_dft_rect_cols_kernel",
                   # the label plane and the auxiliary heads (debias.hip): up to 96 weights or sums per thread, sized to stay in registers
                   "tfc_pack_labels_kernel", "tfc_label_plane_bwd_kernel", "tfc_aux_heads_fwd_kernel", "tfc_aux_heads_dgrad_kernel",
                   "tfc_aux_heads_wgrad_kernel", "tfc_softmax_ce_heads_kernel",
                   # the edge mask (mask.hip): tile kernels with their taps and four outputs per thread in registers
                   "tfc_mask_lap_kernel", "tfc_mask_blur_kernel", "tfc_mask_blur_bwd_kernel", "tfc_mask_lap_bwd_kernel", "tfc_mask_dot_kernel",
                   "tfc_mask_final_extrema_kernel", "tfc_mask_final_sums_kernel", "tfc_mask_scale_kernel", "tfc_pack_plane_kernel",
                   # their phase forms for a batch spread over ranks: the record and merge kernels (mask.hip), the two walks of the KL loss (losses.hip)
                   "tfc_mask_record_extrema_kernel", "tfc_mask_record_sums_kernel", "tfc_mask_merge_kernel", "tfc_batch_kl_stats_kernel",
                   "tfc_batch_kl_merge_kernel", "tfc_batch_kl_terms_kernel",
                   # the tiled attention (vit.hip): 16-row statistics, P, dP and the accumulators of a 32 x 32 quarter per lane, sized for registers
                   "tfc_vit_attn_tiled_fwd_kernel", "tfc_vit_attn_tiled_dq_kernel", "tfc_vit_attn_tiled_dkv_kernel",
                   # the persistent layer kernels (igemm.hip): their shared pieces pass the register-held halo (uint4 hv[NHV]) and the accumulator arrays
                   # through helpers; one that stops being inlined or unrolled would send those arrays to scratch, and only this check would tell.
                   # (tfc_conv_c8_kernel<true>, "ILb1E", is not listed: it spills 3 VGPRs, 16 bytes of scratch per lane; profiles/persistent_family_ab.md.)
                   "tfc_upconv_head_kernel", "tfc_dgrad_rows4_kernel", "tfc_dgrad_head_kernel", "tfc_conv_c8_kernelILb0E")


def check_no_spills(remarks):
    """remarks: hipcc stderr with kernel-resource-usage remarks. Returns a list of complaints about guarded kernels (empty = fine)."""
    bad, name = [], None
    for line in remarks.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split("[")[0].strip()
        elif name and any(g in name for g in GUARDED_KERNELS):
            for key in ("ScratchSize [bytes/lane]:", "VGPRs Spill:"):
                if key in line:
                    val = int(line.split(key)[1].split("[")[0].strip())
                    if val != 0:
                        bad.append(f"{name[:80]}: {key} {val}")
    return bad


def unmatched_guards(remarks):
    """remarks: hipcc stderr of a WHOLE build. Returns the GUARDED_KERNELS entries that occur in no `Function Name:` remark: a guard that names
    no kernel (after a rename, say) would check nothing and tell nobody."""
    names = [line.split("Function Name:")[1] for line in remarks.splitlines() if "Function Name:" in line]
    return [g for g in GUARDED_KERNELS if not any(g in n for n in names)]


# ---- the ctypes layer, read from include/tfc_gan.h at import: the header is the one place where the C ABI is written down ----
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong, "uint32_t": ctypes.c_uint32, "uint8_t": ctypes.c_uint8, "size_t": ctypes.c_size_t}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char"}


def _ctype(text, structs, what, ret=False):
    """ctypes class of the C type `text`; every pointer is c_void_p (a `const char*` return: c_char_p). Raises on a type it does not know."""
    words = [w for w in re.sub(r"(\*|\[\w*\])", r" \1 ", text).split() if w not in ("const", "struct")]
    base = " ".join(w for w in words if w[0] not in "*[")
    if len(words) > len(base.split()):                           # a pointer or an array parameter
        if base not in _POINTEES and base not in structs:
            raise ValueError(f"{what}: pointer to unknown type {text.strip()!r}")
        return ctypes.c_char_p if ret and base == "char" and words.count("*") == 1 else ctypes.c_void_p
    if ret and base == "void":
        return None
    if base not in _SCALARS:
        raise ValueError(f"{what}: unknown type {text.strip()!r}")
    return _SCALARS[base]


def _declarator(text, structs, what):
    """a parameter `type name`, `type name[n]` or `type` (the name is optional, as in C) -> ctypes class"""
    try:
        return _ctype(text, structs, what)
    except ValueError:
        m = re.fullmatch(r"(.*?)\b[A-Za-z_]\w*\s*((?:\[\w*\]\s*)*)", text.strip(), re.S)
        if not m or not m.group(1).strip():
            raise
        return _ctype(m.group(1) + m.group(2), structs, what)


def parse_header(text):
    """C ABI of a header in the style of include/tfc_gan.h -> (prototypes, constants, structs):
    prototypes {name: (restype, [argtypes])} of every function declaration, constants {NAME: int} of every `#define TFC_NAME integer`,
    structs {name: [(field, ctype)]} of every `typedef struct`. Anything it cannot classify raises ValueError naming the symbol."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+TFC_(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        try:
            constants[name] = int(value, 0)
        except ValueError:
            raise ValueError(f"TFC_{name}: {value!r} is not an integer literal") from None
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    structs = {}

    def struct(m):
        body, name = m.groups()
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m2 = re.fullmatch(r"(.*?)\b(\w+(?:\s*,\s*\w+)*)", decl, re.S)                    # `type a, b, c`: scalars, or one pointer; no arrays
            if not m2 or ("*" in decl and "," in decl):
                raise ValueError(f"{name}: cannot classify field declaration {decl!r}")
            ct = _ctype(m2.group(1), structs, f"{name}: field declaration {decl!r}")
            fields += [(f.strip(), ct) for f in m2.group(2).split(",")]
        structs[name] = fields
        return ""

    text = re.sub(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    prototypes = {}
    for stmt in filter(None, (s.strip(" \t\n}") for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(tfc_\w+)\s*\(([^()]*)\)", stmt, re.S)
        if not m:
            raise ValueError(f"cannot classify declaration {' '.join(stmt.split())[:80]!r} (not a tfc_* function)")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        prototypes[name] = (_ctype(ret, structs, f"{name}, return type", ret=True),
                            [_declarator(p, structs, f"{name}, argument {i + 1}") for i, p in enumerate(params)])
    return prototypes, constants, structs


with open(PUBLIC_HEADER) as _f:
    PROTOTYPES, CONSTANTS, STRUCTS = parse_header(_f.read())
globals().update({k: v for k, v in CONSTANTS.items() if k.startswith(("DT_", "OP_", "EP_"))})     # DT_BF16, OP_CONV, EP_BIAS, ...


def parse_switch(value):
    """an on/off knob of the environment: unset, '' and '0' are off, anything else is on"""
    return value not in (None, "", "0")


# Batch-invariant mode. The setting is process-wide HERE and per thread in the library (like every host-side hook of it), and the
# kernels of one step are launched from several threads (the caller's, autograd's backward workers): every thread re-applies the current setting
# the next time it fetches the library handle.
_BATCH_INVARIANT = {"on": parse_switch(os.environ.get("TFC_BATCH_INVARIANT")), "gen": 1}
_tls = threading.local()


def set_batch_invariant(on):
    _BATCH_INVARIANT["on"] = bool(on)
    _BATCH_INVARIANT["gen"] += 1


def get_batch_invariant():
    return _BATCH_INVARIANT["on"]


def load():
    """Load the shared object (building it when stale) and attach prototypes. torch must be imported first so that the
    process already holds the HIP runtime torch ships; our library then binds to that same libamdhip64.so.7."""
    lib = _load()
    gen = _BATCH_INVARIANT["gen"]
    if getattr(_tls, "gen", 0) != gen:
        lib.tfc_set_batch_invariant(1 if _BATCH_INVARIANT["on"] else 0)
        _tls.gen = gen
    return lib


def _load():
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (HIP runtime first)
        so = os.environ.get("TFC_SO_OVERRIDE")                    # development only: A/B a differently compiled library
        if not so:
            build()
            so = SO_PATH
        lib = ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)      # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


class TfcError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        msg = load().tfc_last_error().decode("utf-8", "replace")
        raise TfcError(f"libtfcgan_hip: {what} failed ({rc}): {msg}")
