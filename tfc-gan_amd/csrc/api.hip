// extern "C" surface of libtfcgan_hip.so (declared in include/tfc_gan.h): argument checking, gather-descriptor
// construction for every convolution op / pass of the PATCH-16 path, launch, per-kernel timing hooks, and the
// host-side emulator of the gather model used by the CPU tests.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../include/tfc_gan.h"
#include "tfc_desc.h"
#include "pack_math.h"

// ---- error handling --------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
static int hipfail(hipError_t e, const char* where) { return fail(-100 - (int)e, "%s: %s", where, hipGetErrorString(e)); }
#define CHECK_HIP(expr, where) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hipfail(e_, where); } while (0)
#define REQUIRE(cond, ...) do { if (!(cond)) return fail(-1, __VA_ARGS__); } while (0)

extern "C" const char* tfc_last_error(void) { return g_err.c_str(); }
extern "C" int tfc_abi_version(void) { return 3; }              // 2: deterministic reductions (part_ws arguments); 3: tfc_lpips_head takes part_ws too
extern "C" size_t tfc_part_ws_floats(void) { return (size_t)TFC_PART_WS_FLOATS; }

static inline int pad8(int c) { return (c + 7) / 8 * 8; }
static inline int es_of(int dt) { return dt == TFC_DT_BF16 ? 2 : 4; }

// ---- profiling: hipEvents around the two MFMA kernel classes ---------------------------------------------------
// Per-THREAD state (the thread that enables profiling is the thread that launches and collects). Each record keeps the call's shape,
// so tfc_prof_records() gives a per-layer table; TFC_LAUNCH_LOG=<file> (read once) additionally appends one line per conv-class call
// "kclass op pass N H W Cin Cout flop nlaunch" -- the join key scripts/per_layer.py uses to split a rocprofv3 kernel trace by layer.
namespace {
struct ProfRec { hipEvent_t a, b; int kclass; double flop; int meta[7]; };
thread_local bool g_prof_on = false;
thread_local std::vector<ProfRec> g_prof;
thread_local std::vector<hipEvent_t> g_event_pool;
FILE* launch_log() {
  static FILE* f = [] { const char* p = getenv("TFC_LAUNCH_LOG"); return (p && *p) ? fopen(p, "a") : (FILE*)nullptr; }();
  return f;
}
hipEvent_t get_event() {
  if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}
struct ProfScope {
  bool on;
  hipStream_t st;
  ProfRec rec;
  long long launches0;
  ProfScope(int kclass, double flop, hipStream_t s, int op, int pass, int N, int H, int W, int Cin, int Cout) : st(s) {
    on = g_prof_on;
    rec.kclass = kclass; rec.flop = flop;
    const int m[7] = {op, pass, N, H, W, Cin, Cout};
    memcpy(rec.meta, m, sizeof m);
    launches0 = g_tfc_launch_count;
    if (on) { rec.a = get_event(); rec.b = get_event(); hipEventRecord(rec.a, st); }
  }
  ~ProfScope() {
    if (on) { hipEventRecord(rec.b, st); g_prof.push_back(rec); }
    if (FILE* f = launch_log()) {
      fprintf(f, "%d %d %d %d %d %d %d %d %.0f %lld\n", rec.kclass, rec.meta[0], rec.meta[1], rec.meta[2], rec.meta[3], rec.meta[4], rec.meta[5],
              rec.meta[6], rec.flop, g_tfc_launch_count - launches0);
      fflush(f);
    }
  }
};
}  // namespace

extern "C" int tfc_prof_enable(int on) {
  g_prof_on = on != 0;
  return 0;
}
extern "C" int tfc_prof_collect(int kclass, double* total_ms, double* flop, long long* launches) {
  double ms = 0, fl = 0;
  long long n = 0;
  std::vector<ProfRec> keep;
  for (auto& r : g_prof) {
    if (r.kclass != kclass) { keep.push_back(r); continue; }
    float t = 0.f;
    hipError_t e = hipEventElapsedTime(&t, r.a, r.b);
    if (e != hipSuccess) return hipfail(e, "tfc_prof_collect (synchronise before collecting)");
    ms += t; fl += r.flop; ++n;
    g_event_pool.push_back(r.a);
    g_event_pool.push_back(r.b);
  }
  g_prof.swap(keep);
  if (total_ms) *total_ms = ms;
  if (flop) *flop = fl;
  if (launches) *launches = n;
  return 0;
}
// per-call detail of the records gathered so far on this thread (does not consume them): returns the number of records written
extern "C" int tfc_prof_records(int max_records, int* kclass, double* ms, double* flop, int* meta7) {
  int n = 0;
  for (auto& r : g_prof) {
    if (n >= max_records) break;
    float t = 0.f;
    hipError_t e = hipEventElapsedTime(&t, r.a, r.b);
    if (e != hipSuccess) return hipfail(e, "tfc_prof_records (synchronise before collecting)");
    if (kclass) kclass[n] = r.kclass;
    if (ms) ms[n] = t;
    if (flop) flop[n] = r.flop;
    if (meta7) memcpy(meta7 + 7 * n, r.meta, sizeof r.meta);
    ++n;
  }
  return n;
}

// ---------------------------------------------------------------------------------------------------------------
// descriptor construction.  (N,H,W,Cin,Cout) always describe the op's FORWARD input.
//   pass 0 = forward, 1 = dgrad (source = dy, result = dx), 2 = wgrad (forward geometry, K = pixels)
// ---------------------------------------------------------------------------------------------------------------
struct WeightMap { int Nreal, Creal; long long sn, sc; };

static int out_hw(int op, int h) {
  if (op == TFC_OP_CONV2) return h / 2;
  return op == TFC_OP_CONV ? h - 1 : ((op == TFC_OP_PADCONV || op == TFC_OP_CONV3 || op == TFC_OP_CONV3R) ? h : 2 * h);
}
// phases = descriptors of one pass that are packed / launched one after the other: the four sub-pixel output phases of the 2x-upsampling ops (forward
// and weight gradient) and of the stride-2 convolution's input gradient; the four source parity planes of the stride-2 convolution's weight gradient
static int num_phases(int op, int pass) {
  if (op == TFC_OP_CONV2) return pass == 0 ? 1 : 4;
  return ((op == TFC_OP_CONVT || op == TFC_OP_UPCONV) && pass != 1) ? 4 : 1;
}
// the phases of (op, pass) have one shape and fold into the grid of ONE gather-GEMM launch (phase-0 descriptor + per-phase shifts)
static bool fold_phases(int op, int pass) { return pass == 0 ? (op == TFC_OP_CONVT || op == TFC_OP_UPCONV) : (pass == 1 && op == TFC_OP_CONV2); }
static void set_fold(TfcGather& d, int op) { d.ph_n = 4; d.ph_d0 = (op == TFC_OP_UPCONV) ? 0 : 1; d.ph_oo = 1; }   // convT / conv2 dgrad: dy0 = py - 1; all: OOY = py

// source parity planes of a stride-2 gather (transposed-conv dgrad, stride-2 conv forward / weight gradient): source row 2 i - 1 + k of filter tap k lies in
// parity plane 0 for k in {1, 3} (plane rows i, i + 1) and in plane 1 for k in {0, 2} (plane rows i - 1, i)
static void set_parity_plane(TfcPlane& p, int ppy, int ppx) {
  static const int kOf[2][2] = {{1, 3}, {0, 2}};
  p.py = ppy; p.px = ppx; p.dy0 = ppy ? -1 : 0; p.dx0 = ppx ? -1 : 0; p.hh = 9; p.hw = 17; p.ntaps = 4;
  for (int jy = 0; jy < 2; ++jy)
    for (int jx = 0; jx < 2; ++jx) {
      const int t = jy * 2 + jx;
      p.tap_dy[t] = jy; p.tap_dx[t] = jx; p.tap_mask[t] = 1 << (kOf[ppy][jy] * 4 + kOf[ppx][jx]);
    }
}

static void set_tiles(TfcGather& d) {
  d.tiles_y = (d.GH + TFC_TILE_H - 1) / TFC_TILE_H;
  d.tiles_x = (d.GW + TFC_TILE_W - 1) / TFC_TILE_W;
}

// UPCONV: out[2a+p] reads source row a + off(p,k), off(0,.) = {-1,-1,0,0}, off(1,.) = {-1,0,0,1}
static const int kUpOff[2][4] = {{-1, -1, 0, 0}, {-1, 0, 0, 1}};

static int build_desc(int op, int pass, int phase, int N, int H, int W, int Cin, int Cout, int in_pitch, int out_pitch,
                      TfcGather* dp, WeightMap* wm) {
  TfcGather& d = *dp;
  memset(&d, 0, sizeof d);
  const int OH = out_hw(op, H), OW = out_hw(op, W);
  d.nimg = N;
  d.in_pitch = in_pitch;
  d.out_pitch = out_pitch;
  d.SS = 1; d.OS = 1; d.OOY = 0; d.OOX = 0;
  d.nplanes = 1;
  d.ph_n = 1; d.ph_d0 = 0; d.ph_oo = 0;
  const int py = phase >> 1, px = phase & 1;
  const bool fwd_geom = (pass != 1);
  if (fwd_geom) {
    d.IH = H; d.IW = W; d.Cin_pad = pad8(Cin);
    d.OH = OH; d.OW = OW; d.Nout = Cout;
    TfcPlane& p = d.plane[0];
    switch (op) {
      case TFC_OP_CONV:
      case TFC_OP_PADCONV: {
        const int o0 = (op == TFC_OP_CONV) ? -1 : -2;
        d.GH = OH; d.GW = OW;
        p.dy0 = o0; p.dx0 = o0; p.hh = 11; p.hw = 19; p.ntaps = 16;
        for (int ky = 0; ky < 4; ++ky)
          for (int kx = 0; kx < 4; ++kx) { const int t = ky * 4 + kx; p.tap_dy[t] = ky; p.tap_dx[t] = kx; p.tap_mask[t] = 1 << t; }
        if (wm) *wm = {Cout, Cin, (long long)Cin * 16, 16};
        break;
      }
      case TFC_OP_CONVT: {
        d.GH = H; d.GW = W; d.OS = 2; d.OOY = py; d.OOX = px;
        p.dy0 = py - 1; p.dx0 = px - 1; p.hh = 9; p.hw = 17; p.ntaps = 4;
        for (int jy = 0; jy < 2; ++jy)
          for (int jx = 0; jx < 2; ++jx) {
            const int t = jy * 2 + jx;
            p.tap_dy[t] = 1 - jy; p.tap_dx[t] = 1 - jx;
            p.tap_mask[t] = 1 << ((1 - py + 2 * jy) * 4 + (1 - px + 2 * jx));
          }
        if (wm) *wm = {Cout, Cin, 16, (long long)Cout * 16};   // ConvTranspose2d weight [Cin][Cout][4][4]
        break;
      }
      case TFC_OP_UPCONV: {
        // out[2a+p] reads source row a + off(p,k): the 4 filter rows hit only 2 (p=0) or 3 (p=1) distinct source rows, so the
        // duplicated taps are collapsed (their weights add): 2x2 / 2x3 / 3x2 / 3x3 distinct source offsets instead of 16 taps per
        // phase. Every phase is laid out on the SAME 3 x 3 offset grid (an offset a phase lacks gets mask 0 = zero weights): the four
        // phases then share one tap pattern and one halo geometry and fold into ONE launch like the transposed convolution.
        d.GH = H; d.GW = W; d.OS = 2; d.OOY = py; d.OOX = px;
        const int ny = 3, nx = 3;
        p.dy0 = -1; p.dx0 = -1; p.hh = 8 + ny - 1; p.hw = 16 + nx - 1; p.ntaps = ny * nx;
        for (int iy = 0; iy < ny; ++iy)
          for (int ix = 0; ix < nx; ++ix) {
            const int t = iy * nx + ix;
            int mask = 0;
            for (int ky = 0; ky < 4; ++ky)
              for (int kx = 0; kx < 4; ++kx)
                if (kUpOff[py][ky] + 1 == iy && kUpOff[px][kx] + 1 == ix) mask |= 1 << (ky * 4 + kx);
            p.tap_dy[t] = iy; p.tap_dx[t] = ix; p.tap_mask[t] = mask;
          }
        if (wm) *wm = {Cout, Cin, (long long)Cin * 16, 16};
        break;
      }
      case TFC_OP_CONV3R:                                         // the same gather with the reflect rule on the image's one-pixel ring (forward and weight gradient)
        d.reflect = 1;
        [[fallthrough]];
      case TFC_OP_CONV3: {
        // nn.Conv2d(k3, s1, p1) (VGG16 feature stack of LPIPS): the 3 x 3 filter is handed over zero-padded to the 4 x 4 torch layout of the other
        // ops ([Cout][Cin][4][4], taps (ky, kx) with ky, kx <= 2 used), so packing shares every code path; 3 x 3 raster = tap pattern 6
        d.GH = OH; d.GW = OW;
        p.dy0 = -1; p.dx0 = -1; p.hh = 10; p.hw = 18; p.ntaps = 9;
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) { const int t = ky * 3 + kx; p.tap_dy[t] = ky; p.tap_dx[t] = kx; p.tap_mask[t] = 1 << (ky * 4 + kx); }
        if (wm) *wm = {Cout, Cin, (long long)Cin * 16, 16};
        break;
      }
      case TFC_OP_CONV2: {
        // nn.Conv2d(k4, s2, p1): out[o] = sum_k x[2 o - 1 + k] W[k] -- a stride-2 gather over the four parity planes of x (the tap sets of the transposed
        // convolution's dgrad) with the weight map of the plain convolution. The weight gradient (pass 2) takes the planes one by one (phase = plane):
        // each fills its own four filter taps.
        d.GH = OH; d.GW = OW; d.SS = 2;
        if (pass == 2) set_parity_plane(p, py, px);
        else {
          d.nplanes = 4;
          for (int q = 0; q < 4; ++q) set_parity_plane(d.plane[q], q >> 1, q & 1);
        }
        if (wm) *wm = {Cout, Cin, (long long)Cin * 16, 16};
        break;
      }
      default: return fail(-1, "unknown op %d", op);
    }
  } else {
    // dgrad: source = dy [N][OH][OW][Cout], result = dx [N][H][W][Cin]
    d.IH = OH; d.IW = OW; d.Cin_pad = pad8(Cout);
    d.OH = H; d.OW = W; d.Nout = Cin;
    d.GH = H; d.GW = W;
    switch (op) {
      case TFC_OP_CONV:
      case TFC_OP_PADCONV: {
        TfcPlane& p = d.plane[0];
        const int o0 = (op == TFC_OP_CONV) ? -2 : -1;
        p.dy0 = o0; p.dx0 = o0; p.hh = 11; p.hw = 19; p.ntaps = 16;
        for (int ky = 0; ky < 4; ++ky)
          for (int kx = 0; kx < 4; ++kx) { const int t = ky * 4 + kx; p.tap_dy[t] = ky; p.tap_dx[t] = kx; p.tap_mask[t] = 1 << ((3 - ky) * 4 + (3 - kx)); }
        if (wm) *wm = {Cin, Cout, 16, (long long)Cin * 16};    // Conv2d weight [Cout][Cin][4][4], n = ci, c = co
        break;
      }
      case TFC_OP_CONV3R:
        // the gradient of the reflect-PADDED input, E[e] = sum_k dy[e - k] W[k] over e = 0 .. H + 1 (padded row e = i + 1): the taps and the packed stream of
        // TFC_OP_CONV3 on a (H + 2) x (W + 2) result grid, zero outside dy. tfc_conv_dgrad folds the one-pixel ring of E into the interior (the exact
        // adjoint of the padding) behind this launch.
        d.OH = H + 2; d.OW = W + 2; d.GH = H + 2; d.GW = W + 2;
        [[fallthrough]];
      case TFC_OP_CONV3: {
        TfcPlane& p = d.plane[0];                                 // dx[i] = sum_k dy[i + 1 - k] W[k], k = 0..2: plane offsets 0..2 from i - 1, flipped taps
        p.dy0 = op == TFC_OP_CONV3R ? -2 : -1; p.dx0 = p.dy0; p.hh = 10; p.hw = 18; p.ntaps = 9;
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) { const int t = ky * 3 + kx; p.tap_dy[t] = ky; p.tap_dx[t] = kx; p.tap_mask[t] = 1 << ((2 - ky) * 4 + (2 - kx)); }
        if (wm) *wm = {Cin, Cout, 16, (long long)Cin * 16};
        break;
      }
      case TFC_OP_CONVT: {
        // dx[i] = sum_k dy[2i-1+k] W[k]: parity plane 0 holds k in {1,3} at plane rows {i, i+1}; plane 1 holds k in {0,2} at {i-1, i}
        d.SS = 2; d.nplanes = 4;
        for (int q = 0; q < 4; ++q) set_parity_plane(d.plane[q], q >> 1, q & 1);
        if (wm) *wm = {Cin, Cout, (long long)Cout * 16, 16};   // W[ci][co][k]: n = ci, c = co
        break;
      }
      case TFC_OP_CONV2: {
        // dx[2 a + py] = sum_j dy[a + py - j] W[1 - py + 2 j]: the four output phases of the transposed convolution's forward, on the Conv2d weight
        TfcPlane& p = d.plane[0];
        d.GH = OH; d.GW = OW; d.OS = 2; d.OOY = py; d.OOX = px;
        p.dy0 = py - 1; p.dx0 = px - 1; p.hh = 9; p.hw = 17; p.ntaps = 4;
        for (int jy = 0; jy < 2; ++jy)
          for (int jx = 0; jx < 2; ++jx) {
            const int t = jy * 2 + jx;
            p.tap_dy[t] = 1 - jy; p.tap_dx[t] = 1 - jx;
            p.tap_mask[t] = 1 << ((1 - py + 2 * jy) * 4 + (1 - px + 2 * jx));
          }
        if (wm) *wm = {Cin, Cout, 16, (long long)Cin * 16};    // Conv2d weight [Cout][Cin][4][4]: n = ci, c = co
        break;
      }
      case TFC_OP_UPCONV: {
        // du[a] = sum over parity planes p of dy, taps k with a' = a - off(p,k):  plane row a' = a + (-off)
        d.SS = 2; d.nplanes = 4;
        for (int ppy = 0; ppy < 2; ++ppy)
          for (int ppx = 0; ppx < 2; ++ppx) {
            TfcPlane& p = d.plane[ppy * 2 + ppx];
            p.py = ppy; p.px = ppx; p.dy0 = ppy ? -1 : 0; p.dx0 = ppx ? -1 : 0; p.hh = 10; p.hw = 18; p.ntaps = 16;
            for (int ky = 0; ky < 4; ++ky)
              for (int kx = 0; kx < 4; ++kx) {
                const int t = ky * 4 + kx;
                p.tap_dy[t] = -kUpOff[ppy][ky] - p.dy0; p.tap_dx[t] = -kUpOff[ppx][kx] - p.dx0; p.tap_mask[t] = 1 << t;
              }
          }
        if (wm) *wm = {Cin, Cout, 16, (long long)Cin * 16};    // Conv2d weight [Cout][Cin][4][4]: n = ci, c = co
        break;
      }
      default: return fail(-1, "unknown op %d", op);
    }
  }
  set_tiles(d);
  // sanity: every tap must stay inside the staged halo
  for (int pl = 0; pl < d.nplanes; ++pl) {
    const TfcPlane& p = d.plane[pl];
    if (p.hh > TFC_MAX_HH || p.hw > TFC_MAX_HW) return fail(-1, "halo too large");
    for (int t = 0; t < p.ntaps; ++t)
      if (p.tap_dy[t] < 0 || p.tap_dx[t] < 0 || p.tap_dy[t] + TFC_TILE_H > p.hh || p.tap_dx[t] + TFC_TILE_W > p.hw)
        return fail(-1, "tap %d of plane %d leaves the halo (op %d pass %d)", t, pl, op, pass);
  }
  return 0;
}

// the gather-GEMM main loop consumes k-substeps in pairs
static int check_desc(const TfcGather& d, int dt) {
  for (int pl = 0; pl < d.nplanes; ++pl)
    REQUIRE(tfc_nsub(d.plane[pl].ntaps, tfc_pb(d.Cin_pad, es_of(dt))) % 2 == 0,
            "unsupported shape: %d taps with %d-byte channel chunks give an odd number of k-substeps", d.plane[pl].ntaps, tfc_pb(d.Cin_pad, es_of(dt)));
  return 0;
}

static int check_common(int dt, int op, int N, int H, int W, int Cin, int Cout) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype %d", dt);
  REQUIRE(op >= 0 && op <= 6, "bad op %d", op);
  REQUIRE(op != TFC_OP_CONV3R || (H >= 2 && W >= 2), "TFC_OP_CONV3R (reflection padding 1) needs H >= 2 and W >= 2 (H=%d W=%d)", H, W);
  REQUIRE(N > 0 && H > 1 && W > 1 && Cin > 0 && Cout > 0, "bad dims N=%d H=%d W=%d Cin=%d Cout=%d", N, H, W, Cin, Cout);
  REQUIRE(op != TFC_OP_CONV2 || (H % 2 == 0 && W % 2 == 0), "TFC_OP_CONV2 (stride 2) needs an even H and W (H=%d W=%d)", H, W);
  REQUIRE((long long)N * (2 * H) * (2 * W) * (long long)(pad8(Cin) > pad8(Cout) ? pad8(Cin) : pad8(Cout)) < 2147483647LL,
          "tensor exceeds 2^31 elements");
  const int es = es_of(dt);
  REQUIRE(pad8(Cin) * es <= 64 || (pad8(Cin) * es) % 64 == 0, "Cin=%d: padded channel bytes must be <= 64 or a multiple of 64", Cin);
  REQUIRE(pad8(Cout) * es <= 64 || (pad8(Cout) * es) % 64 == 0, "Cout=%d: padded channel bytes must be <= 64 or a multiple of 64", Cout);
  // 9 taps do not fill whole 64-byte K chunks with narrow channels: the caller pads the image to 64 bytes of channels (lpips.py does)
  REQUIRE((op != TFC_OP_CONV3 && op != TFC_OP_CONV3R) || ((pad8(Cin) * es) % 64 == 0 && (pad8(Cout) * es) % 64 == 0),
          "TFC_OP_CONV3 / TFC_OP_CONV3R need channel bytes in multiples of 64 (Cin=%d Cout=%d)", Cin, Cout);
  return 0;
}
static int check_pitch(int dt, int pitch, int cpad, const char* what) {
  const int ue = 16 / es_of(dt);
  REQUIRE(pitch >= cpad && pitch % ue == 0, "%s pitch %d must be >= %d and a multiple of %d", what, pitch, cpad, ue);
  return 0;
}
static int check_dt(int dt) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype %d", dt);
  return 0;
}
static int check_ptr16(const void* p, const char* what) {
  REQUIRE(p != nullptr && (((uintptr_t)p) & 15) == 0, "%s must be a 16-byte aligned device pointer", what);
  return 0;
}

// byte offset of phase `ph` inside the packed stream of (op, pass); ph == num_phases gives the total size
static size_t phase_packed_offset(int dt, int op, int pass, int Cin, int Cout, int ph) {
  size_t off = 0;
  for (int q = 0; q < ph; ++q) {
    TfcGather d;
    if (build_desc(op, pass, q, 1, 16, 16, Cin, Cout, pad8(Cin), pad8(Cout), &d, nullptr)) return 0;
    off += tfc_packed_bytes(d, es_of(dt));
  }
  return off;
}

extern "C" size_t tfc_conv_packed_bytes(int dt, int op, int pass, int Cin, int Cout) {
  if (pass < 0 || pass > 1 || op < 0 || op > 6) return 0;
  return phase_packed_offset(dt, op, pass, Cin, Cout, num_phases(op, pass));
}

extern "C" int tfc_conv_pack(void* stream, int dt, int op, int pass, const float* w, const float* scale, void* packed, int Cin, int Cout) {
  if (int e = check_common(dt, op, 1, 16, 16, Cin, Cout)) return e;
  REQUIRE(pass == 0 || pass == 1, "pass must be 0 (fwd) or 1 (dgrad)");
  if (int e = check_ptr16(packed, "packed")) return e;
  REQUIRE(w != nullptr, "w is null");
  for (int ph = 0; ph < num_phases(op, pass); ++ph) {
    TfcGather d;
    WeightMap wm;
    if (int e = build_desc(op, pass, ph, 1, 16, 16, Cin, Cout, pad8(Cin), pad8(Cout), &d, &wm)) return e;
    CHECK_HIP(tfc_launch_pack(dt, d, w, scale, (char*)packed + phase_packed_offset(dt, op, pass, Cin, Cout, ph), wm.Nreal, wm.Creal, wm.sn, wm.sc, (hipStream_t)stream), "tfc_conv_pack");
  }
  return 0;
}

static double conv_flop(int op, int N, int H, int W, int Cin, int Cout) {
  const double oh = out_hw(op, H), ow = out_hw(op, W);
  const double taps = (op == TFC_OP_CONVT) ? 4.0 : ((op == TFC_OP_CONV3 || op == TFC_OP_CONV3R) ? 9.0 : 16.0);
  return 2.0 * N * oh * ow * (double)Cin * Cout * taps;
}

extern "C" int tfc_conv_fwd(void* stream, int dt, int op, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout,
                            const void* packed, void* y, int y_pitch, const float* bias, float* stats, float* out_nchw, const float* oscale, int flags,
                            float* part_ws) {
  if (int e = check_common(dt, op, N, H, W, Cin, Cout)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(packed, "packed")) return e;
  if (int e = check_pitch(dt, x_pitch, pad8(Cin), "x")) return e;
  if (flags & TFC_EP_TANH_NCHW) { REQUIRE(out_nchw != nullptr, "out_nchw is null"); }
  else {
    REQUIRE(y != nullptr, "y is null");
    REQUIRE(y_pitch >= Cout, "y pitch %d < Cout %d", y_pitch, Cout);
    if (dt == TFC_DT_BF16 && Cout >= 8) REQUIRE(y_pitch % 8 == 0 && (((uintptr_t)y) & 15) == 0, "bf16 outputs are stored in 16-byte units: y must be 16-byte aligned with pitch %% 8 == 0");
  }
  if (flags & TFC_EP_BIAS) REQUIRE(bias != nullptr, "bias is null");
  if (flags & TFC_EP_STATS) REQUIRE(stats != nullptr && part_ws != nullptr, "TFC_EP_STATS needs stats and part_ws");
  int nph = num_phases(op, 0);
  const bool fold = fold_phases(op, 0);                           // equal-shaped phases: fold all four into the grid of one launch
  if (fold) nph = 1;
  ProfScope prof(0, conv_flop(op, N, H, W, Cin, Cout), (hipStream_t)stream, op, 0, N, H, W, Cin, Cout);
  for (int ph = 0; ph < nph; ++ph) {
    TfcGather d;
    if (int e = build_desc(op, 0, ph, N, H, W, Cin, Cout, x_pitch, y_pitch, &d, nullptr)) return e;
    if (fold) set_fold(d, op);                                    // phase 0 descriptor + per-phase shifts (convT: dy0 = py-1; both: OOY = py)
    if (int e = check_desc(d, dt)) return e;
    CHECK_HIP(tfc_launch_igemm(dt, d, x, (const char*)packed + phase_packed_offset(dt, op, 0, Cin, Cout, ph), y, bias, stats, part_ws, out_nchw, oscale, flags, (hipStream_t)stream), "tfc_conv_fwd");
  }
  return 0;
}

extern "C" int tfc_conv_first_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout, const void* packed, void* y,
                                  int y_pitch, const float* bias, const float* oscale, int flags, uint8_t* sign_mask) {
  REQUIRE(dt == TFC_DT_BF16 && tfc_first_block_bwd_supported(dt, Cin, Cout), "tfc_conv_first_fwd: bf16, Cin <= 8, Cout == 64 (use tfc_conv_fwd otherwise)");
  if (int e = check_common(dt, TFC_OP_CONV, N, H, W, Cin, Cout)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(packed, "packed")) return e;
  if (int e = check_ptr16(y, "y")) return e;
  REQUIRE(x_pitch == 8 && y_pitch >= Cout && y_pitch % 8 == 0, "pitches: x %d (must be 8), y %d", x_pitch, y_pitch);
  REQUIRE((flags & ~(TFC_EP_BIAS | TFC_EP_LEAKY)) == 0 && (!(flags & TFC_EP_BIAS) || bias), "flags: TFC_EP_BIAS (with bias) | TFC_EP_LEAKY only");
  REQUIRE(!sign_mask || (((uintptr_t)sign_mask) & 7) == 0, "sign_mask must be 8-byte aligned");
  TfcGather d;
  if (int e = build_desc(TFC_OP_CONV, 0, 0, N, H, W, Cin, Cout, x_pitch, y_pitch, &d, nullptr)) return e;
  REQUIRE(tfc_conv_c8_eligible(d, flags), "unexpected descriptor");
  ProfScope prof(0, conv_flop(TFC_OP_CONV, N, H, W, Cin, Cout), (hipStream_t)stream, TFC_OP_CONV, 0, N, H, W, Cin, Cout);
  CHECK_HIP(tfc_launch_conv_c8(d, x, packed, y, bias, oscale, flags, sign_mask, (hipStream_t)stream), "tfc_conv_first_fwd");
  return 0;
}

extern "C" int tfc_first_block_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout, const void* packed, const float* bias,
                                   const float* oscale, float slope, int act_after_rounding, void* out, int out_pitch, uint8_t* sign_mask) {
  REQUIRE(dt == TFC_DT_BF16 && tfc_first_block_bwd_supported(dt, Cin, Cout), "tfc_first_block_fwd: bf16, Cin <= 8, Cout == 64");
  if (int e = check_common(dt, TFC_OP_CONV, N, H, W, Cin, Cout)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(packed, "packed")) return e;
  REQUIRE(out && (((uintptr_t)out) & 7) == 0 && out_pitch >= 64 && out_pitch % 4 == 0, "out must be 8-byte aligned with pitch >= 64 and a multiple of 4");
  REQUIRE(x_pitch == 8 && H >= 6 && W >= 6, "x pitch %d (must be 8); the reflect padding of the pooling needs a 5 x 5 convolution output at least", x_pitch);
  REQUIRE(!sign_mask || (((uintptr_t)sign_mask) & 7) == 0, "sign_mask must be 8-byte aligned");
  // 2 x (the convolution on the 1.33x overlapping regions) is what the kernel executes; the algorithmic work of the block is the convolution's
  ProfScope prof(0, conv_flop(TFC_OP_CONV, N, H, W, Cin, Cout), (hipStream_t)stream, TFC_OP_CONV, 0, N, H, W, Cin, Cout);
  CHECK_HIP(tfc_launch_first_block_fwd(x, N, H, W, packed, bias, oscale, slope, act_after_rounding, out, out_pitch, sign_mask, (hipStream_t)stream),
            "tfc_first_block_fwd");
  return 0;
}

extern "C" int tfc_conv_dgrad_image(void* stream, int dt, const void* dy, int dy_pitch, int N, int H, int W, int Cin, int Cout, const float* w,
                                   const float* oscale, int nch, float* dx_nchw) {
  REQUIRE(dt == TFC_DT_BF16 && Cout == 64 && Cin >= 1 && nch >= 1 && nch <= 4 && nch <= Cin, "tfc_conv_dgrad_image: bf16, Cout == 64, nch <= min(4, Cin) only");
  REQUIRE(dy && w && dx_nchw && N > 0 && H > 4 && W > 4 && dy_pitch >= 64 && dy_pitch % 8 == 0, "bad args");
  if (int e = check_ptr16(dy, "dy")) return e;
  ProfScope prof(0, 2.0 * N * (H - 1.0) * (W - 1.0) * nch * Cout * 16.0, (hipStream_t)stream, TFC_OP_CONV, 1, N, H, W, nch, Cout);
  CHECK_HIP(tfc_launch_dgrad_rows4(dy, dy_pitch, N, H, W, w, Cin, oscale, nch, dx_nchw, (hipStream_t)stream), "tfc_conv_dgrad_image");
  return 0;
}

extern "C" int tfc_upconv_head_dgrad(void* stream, int dt, const void* dy, int dy_pitch, int N, int H, int W, int Cin, int Cout, const float* w, void* dx,
                                     int dx_pitch) {
  REQUIRE(dt == TFC_DT_BF16 && Cin == 128 && Cout >= 1 && Cout <= 8, "tfc_upconv_head_dgrad: bf16, Cin == 128, Cout <= 8 only (use tfc_conv_dgrad(TFC_OP_UPCONV) otherwise)");
  REQUIRE(dy && w && dx && N > 0 && H > 1 && W > 1 && dy_pitch >= 8 && dy_pitch % 8 == 0 && dx_pitch >= 128 && dx_pitch % 8 == 0, "bad args");
  REQUIRE((long long)N * H * W * dx_pitch < 2147483647LL, "tensor exceeds 2^31 elements");
  if (int e = check_ptr16(dy, "dy")) return e;
  if (int e = check_ptr16(dx, "dx")) return e;
  if (int e = check_ptr16(w, "w")) return e;
  ProfScope prof(0, conv_flop(TFC_OP_UPCONV, N, H, W, Cin, Cout), (hipStream_t)stream, TFC_OP_UPCONV, 1, N, H, W, Cin, Cout);
  CHECK_HIP(tfc_launch_dgrad_head(dy, dy_pitch, N, H, W, w, Cout, dx, dx_pitch, (hipStream_t)stream), "tfc_upconv_head_dgrad");
  return 0;
}

extern "C" int tfc_upconv_head_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout, const float* w,
                                  const float* bias, float* out_nchw) {
  REQUIRE(dt == TFC_DT_BF16 && Cin == 128 && Cout >= 1 && Cout <= 4, "tfc_upconv_head_fwd: bf16, Cin == 128, Cout <= 4 only (use tfc_conv_fwd(TFC_OP_UPCONV) otherwise)");
  REQUIRE(x && w && out_nchw && N > 0 && H > 1 && W > 1 && x_pitch >= 128 && x_pitch % 8 == 0, "bad args");
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(w, "w")) return e;
  ProfScope prof(0, conv_flop(TFC_OP_UPCONV, N, H, W, Cin, Cout), (hipStream_t)stream, TFC_OP_UPCONV, 0, N, H, W, Cin, Cout);
  CHECK_HIP(tfc_launch_upconv_head(x, x_pitch, N, H, W, w, bias, Cout, out_nchw, (hipStream_t)stream), "tfc_upconv_head_fwd");
  return 0;
}

// Scratch of the TFC_OP_CONV3R input gradient: the padded gradient E [N][H + 2][W + 2][pad8(Cin)] in the storage type. tfc_conv_dgrad keeps its
// signature, so the buffer is handed over per calling THREAD (like the other host-side hooks); it is used by the launches of one stream at a time.
static thread_local void* g_dgrad_ws = nullptr;
static thread_local size_t g_dgrad_ws_bytes = 0;
extern "C" size_t tfc_conv_dgrad_ws_bytes(int dt, int op, int N, int H, int W, int Cin, int Cout) {
  (void)Cout;
  if (op != TFC_OP_CONV3R || N <= 0 || H < 2 || W < 2 || Cin <= 0) return 0;
  return (size_t)N * (H + 2) * (W + 2) * pad8(Cin) * es_of(dt);
}
extern "C" int tfc_conv_dgrad_set_ws(void* ws, size_t bytes) {
  REQUIRE(ws == nullptr || (((uintptr_t)ws) & 15) == 0, "ws must be 16-byte aligned");
  g_dgrad_ws = ws;
  g_dgrad_ws_bytes = ws ? bytes : 0;
  return 0;
}

extern "C" int tfc_conv_dgrad(void* stream, int dt, int op, const void* dy, int dy_pitch, int N, int H, int W, int Cin, int Cout,
                              const void* packed, void* dx, int dx_pitch, const float* oscale, int flags) {
  if (int e = check_common(dt, op, N, H, W, Cin, Cout)) return e;
  if (int e = check_ptr16(dy, "dy")) return e;
  if (int e = check_ptr16(packed, "packed")) return e;
  if (int e = check_pitch(dt, dy_pitch, pad8(Cout), "dy")) return e;
  REQUIRE(dx != nullptr && dx_pitch >= Cin, "dx null or pitch %d < Cin %d", dx_pitch, Cin);
  if (dt == TFC_DT_BF16 && Cin >= 8) REQUIRE(dx_pitch % 8 == 0 && (((uintptr_t)dx) & 15) == 0, "bf16 outputs are stored in 16-byte units: dx must be 16-byte aligned with pitch %% 8 == 0");
  REQUIRE((flags & ~TFC_EP_ACCUM) == 0, "dgrad supports only TFC_EP_ACCUM");
  TfcGather d;
  if (op == TFC_OP_CONV3R) {
    // The exact adjoint of reflection padding in two steps. (1) the TFC_OP_CONV3 taps on the (H + 2) x (W + 2) grid of the PADDED input -> E in the
    // calling thread's scratch (tfc_conv_dgrad_set_ws). (2) the fold: every ring pixel of E goes back to the interior pixel the forward read it from
    // (corners fold on both axes), TFC_EP_ACCUM adds the existing dx. A reflection of dy cannot express this: dx[1] gets dy[0] W[0] on top of its
    // three zero-padding terms, a fourth tap that only the border rows have.
    const size_t need = tfc_conv_dgrad_ws_bytes(dt, op, N, H, W, Cin, Cout);
    REQUIRE(g_dgrad_ws != nullptr && g_dgrad_ws_bytes >= need && (((uintptr_t)g_dgrad_ws) & 15) == 0,
            "TFC_OP_CONV3R input gradient needs %zu bytes of 16-byte aligned scratch on this thread (tfc_conv_dgrad_set_ws: %zu given)", need, g_dgrad_ws_bytes);
    const int e_pitch = pad8(Cin);
    if (int e = build_desc(op, 1, 0, N, H, W, Cin, Cout, dy_pitch, e_pitch, &d, nullptr)) return e;
    if (int e = check_desc(d, dt)) return e;
    {
      ProfScope prof(0, conv_flop(op, N, H, W, Cin, Cout), (hipStream_t)stream, op, 1, N, H, W, Cin, Cout);
      CHECK_HIP(tfc_launch_igemm(dt, d, dy, packed, g_dgrad_ws, nullptr, nullptr, nullptr, nullptr, oscale, 0, (hipStream_t)stream), "tfc_conv_dgrad");
    }
    if (int e = check_pitch(dt, dx_pitch, pad8(Cin), "dx")) return e;
    if (int e = check_ptr16(dx, "dx")) return e;
    ProfScope prof(4, 0.0, (hipStream_t)stream, op, 4, N, H, W, Cin, Cout);   // class 4: the fold pass (no algorithmic FLOP of its own)
    CHECK_HIP(tfc_launch_reflect_fold(dt, g_dgrad_ws, e_pitch, dx, dx_pitch, N, H, W, pad8(Cin), (flags & TFC_EP_ACCUM) ? 1 : 0, (hipStream_t)stream),
              "tfc_conv_dgrad (reflect fold)");
    return 0;
  }
  if (int e = build_desc(op, 1, 0, N, H, W, Cin, Cout, dy_pitch, dx_pitch, &d, nullptr)) return e;
  if (fold_phases(op, 1)) set_fold(d, op);                        // stride-2 convolution: the four output phases in one launch
  if (int e = check_desc(d, dt)) return e;
  ProfScope prof(0, conv_flop(op, N, H, W, Cin, Cout), (hipStream_t)stream, op, 1, N, H, W, Cin, Cout);
  CHECK_HIP(tfc_launch_igemm(dt, d, dy, packed, dx, nullptr, nullptr, nullptr, nullptr, oscale, flags, (hipStream_t)stream), "tfc_conv_dgrad");
  return 0;
}

// ---- planned packing: host builds a job table once (geometry and buffers fixed), the caller keeps a device copy ----
extern "C" size_t tfc_pack_plan_bytes(int nlayers) { return (size_t)nlayers * 4 * sizeof(TfcPackJob); }
// fills plan_host with one job per (layer, pass, phase); returns the number of jobs (<0 on error) and the grid size in *nblocks
extern "C" int tfc_pack_plan_build(int dt, int nlayers, const int* ops, const int* passes, const float* const* w, void* const* packed,
                                   const int* Cin, const int* Cout, void* plan_host, int* nblocks) {
  REQUIRE(nlayers > 0 && ops && passes && w && packed && Cin && Cout && plan_host && nblocks, "bad args");
  TfcPackJob* jobs = (TfcPackJob*)plan_host;
  int nj = 0, blk = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (int e = check_common(dt, ops[l], 1, 16, 16, Cin[l], Cout[l])) return e;
    REQUIRE(passes[l] == 0 || passes[l] == 1, "pass must be 0 or 1");
    for (int ph = 0; ph < num_phases(ops[l], passes[l]); ++ph) {
      TfcPackJob& j = jobs[nj];
      WeightMap wm;
      if (int e = build_desc(ops[l], passes[l], ph, 1, 16, 16, Cin[l], Cout[l], pad8(Cin[l]), pad8(Cout[l]), &j.d, &wm)) return e;
      j.w = w[l];
      j.wp = (uint4*)((char*)packed[l] + phase_packed_offset(dt, ops[l], passes[l], Cin[l], Cout[l], ph));
      j.sn = wm.sn; j.sc = wm.sc; j.Nreal = wm.Nreal; j.Creal = wm.Creal;
      j.NB32 = tfc_nb32_padded(j.d.Nout);
      j.units = tfc_total_substeps(j.d, es_of(dt)) * j.NB32 * 64;
      j.threads = j.NB32 * 32 * ((j.d.Cin_pad * es_of(dt)) / 16);   // one thread per (output channel, 16-byte channel unit)
      j.first_block = blk;
      blk += (j.threads + 255) / 256;
      ++nj;
    }
  }
  *nblocks = blk;
  return nj;
}
extern "C" int tfc_conv_pack_planned(void* stream, int dt, const void* plan_dev, int njobs, int nblocks) {
  REQUIRE(plan_dev && njobs > 0 && nblocks > 0, "bad args");
  CHECK_HIP(tfc_launch_pack_planned(dt, plan_dev, njobs, nblocks, (hipStream_t)stream), "tfc_conv_pack_planned");
  return 0;
}

extern "C" int tfc_patchgan_head_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int C, const float* w,
                                     void* y, int y_pitch) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype");
  if (int e = check_ptr16(x, "x")) return e;
  const int ue = 16 / es_of(dt);
  REQUIRE(w && y && N > 0 && H > 0 && W > 0 && C > 0 && C % ue == 0 && C <= 2048 && x_pitch >= C && x_pitch % ue == 0 && y_pitch >= 1, "bad args");
  CHECK_HIP(tfc_launch_head_fwd(dt, x, x_pitch, w, y, y_pitch, N, H, W, C, (hipStream_t)stream), "tfc_patchgan_head_fwd");
  return 0;
}

// wgrad scratch = [split-K slabs | fp32 accumulator 16 x Cout x Cin]: at most 512 workgroups x 4 waves x 8 tiles x 4 KiB = 64 MiB of slabs.
// The slabs come FIRST so that the accumulator (which must stay all-zero between calls) starts at the same offset for every layer
// that shares one scratch buffer.
static size_t wgrad_acc_bytes(int Cin, int Cout) { return (((size_t)16 * Cin * Cout * sizeof(float)) + 255) & ~(size_t)255; }
static const size_t kWgradSlabBytes = (size_t)512 * 4 * 8 * 4 * 64 * 16;
extern "C" size_t tfc_conv_wgrad_ws_bytes(int op, int Cin, int Cout) { (void)op; return wgrad_acc_bytes(Cin, Cout) + kWgradSlabBytes; }

// The stride-2 convolution's weight gradient dW[co][ci][k] = sum_o dy[o] x[2 o - 1 + k] IS the transposed convolution's (dW[ci][co][k] =
// sum_a x[a] dy[2 a - 1 + k], tfc_wgradT_kernel) with the two tensors exchanged: dy plays its input (the small grid), x its output gradient (the four
// parity planes), and the result lands as [slot][n = ci][c = co]. bf16 runs that one launch; TFC_CONV2_WGRAD_PLANES=1 (A/B knob for profiling, ignored
// in batch-invariant mode) keeps the four per-plane launches that the other compute modes use.
static bool conv2_wgrad_mirrored(int dt) {
  static const bool planes_env = [] { const char* e = getenv("TFC_CONV2_WGRAD_PLANES"); return e && atoi(e) != 0; }();
  return dt == TFC_DT_BF16 && !(planes_env && !g_tfc_batch_invariant);
}

extern "C" int tfc_conv_wgrad(void* stream, int dt, int op, const void* x, int x_pitch, const void* dy, int dy_pitch, int N, int H, int W,
                              int Cin, int Cout, void* ws, float* dw, int accumulate) {
  if (int e = check_common(dt, op, N, H, W, Cin, Cout)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(dy, "dy")) return e;
  if (int e = check_pitch(dt, x_pitch, pad8(Cin), "x")) return e;
  if (int e = check_pitch(dt, dy_pitch, pad8(Cout), "dy")) return e;
  REQUIRE(ws != nullptr && dw != nullptr, "ws / dw null");
  REQUIRE(op != TFC_OP_CONV3, "TFC_OP_CONV3 (frozen VGG features of the LPIPS term) has no weight-gradient pass");   // its reflect-padded sibling TFC_OP_CONV3R has
  hipStream_t st = (hipStream_t)stream;
  WeightMap wm{};                                                // the accumulator part of ws is all-zero on entry (caller zeroes it ONCE) and again on exit
  TfcWgradFin fin{dw, 0, 0, accumulate, false};
  int fin_n = Cout, fin_c = Cin;                                  // the accumulator the finish pass lays out is [slot][fin_n][fin_c]
  {
    ProfScope prof(1, conv_flop(op, N, H, W, Cin, Cout), st, op, 2, N, H, W, Cin, Cout);
    bool fused = false;
    if ((op == TFC_OP_CONVT || op == TFC_OP_UPCONV) && dt == TFC_DT_BF16) {   // all four sub-pixel phases in one launch
      TfcGather d0;
      if (int e = build_desc(op, 2, 0, N, H, W, Cin, Cout, x_pitch, dy_pitch, &d0, &wm)) return e;   // wm: the weight layout map
      fin.sn = wm.sn; fin.sc = wm.sc;
      hipError_t herr = hipSuccess;
      fused = tfc_launch_wgrad_phases_fused(op == TFC_OP_UPCONV, x, N, H, W, x_pitch, pad8(Cin), dy, dy_pitch, Cout, Cin,
                                            (float*)((char*)ws + kWgradSlabBytes), ws, st, &herr, &fin);
      if (fused) CHECK_HIP(herr, "tfc_conv_wgrad (phase-fused)");
    } else if (op == TFC_OP_CONV2 && conv2_wgrad_mirrored(dt)) {
      wm = {Cin, Cout, 16, (long long)Cin * 16};                 // Conv2d weight [Cout][Cin][4][4] read as n = ci, c = co
      fin.sn = wm.sn; fin.sc = wm.sc;
      hipError_t herr = hipSuccess;
      fused = tfc_launch_wgrad_phases_fused(0, dy, N, H / 2, W / 2, dy_pitch, pad8(Cout), x, x_pitch, Cin, Cout,
                                            (float*)((char*)ws + kWgradSlabBytes), ws, st, &herr, &fin);
      if (fused) { CHECK_HIP(herr, "tfc_conv_wgrad (stride 2, parity-fused)"); fin_n = Cin; fin_c = Cout; }
    }
    const int nph = num_phases(op, 2);
    for (int ph = 0; ph < nph && !fused; ++ph) {
      TfcGather d;
      if (int e = build_desc(op, 2, ph, N, H, W, Cin, Cout, x_pitch, dy_pitch, &d, &wm)) return e;
      fin.sn = wm.sn; fin.sc = wm.sc;
      CHECK_HIP(tfc_launch_wgrad(dt, d, dy, x, (float*)((char*)ws + kWgradSlabBytes), ws, pad8(Cout), Cout, Cin, st, nph == 1 ? &fin : nullptr), "tfc_conv_wgrad");
    }
  }
  if (!fin.done) {
    ProfScope prof(2, 0.0, st, op, 3, N, H, W, Cin, Cout);     // class 2: the finish pass (layout + re-zero), no algorithmic FLOP of its own
    CHECK_HIP(tfc_launch_wgrad_finish((float*)((char*)ws + kWgradSlabBytes), dw, fin_n, fin_c, wm.sn, wm.sc, accumulate, st), "tfc_conv_wgrad finish");
  }
  return 0;
}

// ---- fused first-block backward --------------------------------------------------------------------------------------------------------

extern "C" int tfc_first_block_bwd_supported(int dt, int Cin, int Cout) { return dt == TFC_DT_BF16 && Cin > 0 && Cin <= 8 && Cout == 64 ? 1 : 0; }
extern "C" int tfc_first_block_bwd_wgrad(void* stream, int dt, const void* x, int x_pitch, const void* y, int y_pitch, const void* dy_pooled, int dyp_pitch,
                                         int N, int H, int W, int Cin, int Cout, float slope, void* ws, float* dw, int accumulate, float* bias_sums,
                                         float* part_ws, const uint8_t* sign_mask) {
  REQUIRE(tfc_first_block_bwd_supported(dt, Cin, Cout), "fused first-block backward: bf16, Cin <= 8, Cout == 64 (dt=%d Cin=%d Cout=%d)", dt, Cin, Cout);
  if (int e = check_common(dt, TFC_OP_CONV, N, H, W, Cin, Cout)) return e;
  REQUIRE(x && (y || sign_mask) && dy_pooled && ws && dw, "null argument (y may be null only when sign_mask is given)");
  REQUIRE(!bias_sums || part_ws, "bias_sums needs part_ws");
  REQUIRE(x_pitch == 8 && (!y || (y_pitch >= 64 && y_pitch % 8 == 0)) && dyp_pitch >= 64 && dyp_pitch % 8 == 0, "pitches: x %d (must be 8), y %d, dy %d", x_pitch, y_pitch, dyp_pitch);
  REQUIRE(H >= 4 && W >= 4, "reflect padding of the blur needs a 3 x 3 activation at least");
  if (int e = check_ptr16(x, "x")) return e;
  if (y) { if (int e = check_ptr16(y, "y")) return e; }
  if (sign_mask) REQUIRE((((uintptr_t)sign_mask) & 7) == 0, "sign_mask must be 8-byte aligned");
  if (int e = check_ptr16(dy_pooled, "dy_pooled")) return e;
  hipStream_t st = (hipStream_t)stream;
  TfcGather d;
  WeightMap wm{};
  if (int e = build_desc(TFC_OP_CONV, 2, 0, N, H, W, Cin, Cout, x_pitch, y_pitch, &d, &wm)) return e;
  REQUIRE(d.plane[0].ntaps == 16 && d.plane[0].hh <= TFC_MAX_HH && d.plane[0].hw <= TFC_MAX_HW, "unexpected descriptor");
  const int Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;          // pooled size of the (H-1) x (W-1) activation
  {
    // class 3, not 1: this launch also carries the transposed blur that used to be an elementwise pass of its own -- keeping it out of the
    // weight-gradient class keeps that class comparable across rounds. The slab reduction writes the torch-layout gradient itself (no finish pass).
    ProfScope prof(3, conv_flop(TFC_OP_CONV, N, H, W, Cin, Cout), st, TFC_OP_CONV, 2, N, H, W, Cin, Cout);
    TfcWgradFin fin{dw, wm.sn, wm.sc, accumulate, false};
    CHECK_HIP(tfc_launch_first_block_bwd(d, y, y_pitch, dy_pooled, dyp_pitch, Ho, Wo, x, ws, (float*)((char*)ws + kWgradSlabBytes), bias_sums, part_ws, slope, Cout, Cin,
                                         sign_mask, &fin, st), "tfc_first_block_bwd_wgrad");
  }
  return 0;
}

// ---- fused activation family ------------------------------------------------------------------------------------
static int fill_act(ActParams& p, int dt, int N, int H, int W, int C, int x_pitch, int o_pitch, int norm, float slope, int pool,
                    float drop_p, uint32_t seed) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype");
  const int ue = 16 / es_of(dt);
  REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "bad dims N=%d H=%d W=%d C=%d", N, H, W, C);
  REQUIRE(C % ue == 0, "C=%d must be a multiple of %d", C, ue);
  const int cv = C / ue;                                          // > 0 from here on: 256 % cv below must not divide by zero
  REQUIRE(cv <= 256 && (256 % cv) == 0, "C/%d = %d must divide 256", ue, cv);
  REQUIRE(pool >= 0 && pool <= 2, "bad pool %d", pool);
  REQUIRE(pool == 0 || (H >= 3 && W >= 3), "reflect pad needs H,W >= 3");
  REQUIRE(x_pitch % ue == 0 && o_pitch % ue == 0, "pitches must be multiples of %d", ue);
  REQUIRE(drop_p >= 0.f && drop_p < 1.f, "drop_p out of range");
  p.N = N; p.H = H; p.W = W; p.C = C;
  p.Ho = pool == 2 ? (H - 1) / 2 + 1 : H;
  p.Wo = pool == 2 ? (W - 1) / 2 + 1 : W;
  p.x_pitch = x_pitch; p.o_pitch = o_pitch; p.pool = pool; p.norm = norm; p.slope = slope; p.eps = 1e-5f;
  p.drop_thresh24 = (unsigned)lrintf(drop_p * 16777216.f);
  p.seed = seed;
  p.drop_scale = 1.f / (1.f - drop_p);
  return 0;
}

extern "C" int tfc_act_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int C, const float* stats, int norm,
                           float slope, int pool, float drop_p, uint32_t seed, void* y, int y_pitch, float* stats_out, float* part_ws) {
  ActParams p;
  if (int e = fill_act(p, dt, N, H, W, C, x_pitch, y_pitch, norm, slope, pool, drop_p, seed)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(y, "y")) return e;
  REQUIRE(!norm || stats, "stats is null");
  REQUIRE(!stats_out || part_ws, "stats_out needs part_ws");
  CHECK_HIP(tfc_launch_act_fwd(dt, p, x, stats, y, stats_out, part_ws, (hipStream_t)stream), "tfc_act_fwd");
  return 0;
}

extern "C" int tfc_norm_add_fwd(void* stream, int dt, const void* x, int x_pitch, const void* res, int res_pitch, int N, int H, int W, int C,
                                const float* stats, void* y, int y_pitch) {
  ActParams p;
  if (int e = fill_act(p, dt, N, H, W, C, x_pitch, y_pitch, 1, 1.f, 0, 0.f, 0)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(res, "res")) return e;
  if (int e = check_ptr16(y, "y")) return e;
  REQUIRE(stats != nullptr, "stats is null");
  REQUIRE(x_pitch >= C && y_pitch >= C && res_pitch >= C && res_pitch % (16 / es_of(dt)) == 0, "pitches: x %d, res %d, y %d must be >= C=%d in 16-byte units", x_pitch, res_pitch, y_pitch, C);
  CHECK_HIP(tfc_launch_norm_add(dt, p, x, stats, res, res_pitch, y, (hipStream_t)stream), "tfc_norm_add_fwd");
  return 0;
}

extern "C" int tfc_act_bwd(void* stream, int dt, int mode, const void* dy, int dy_pitch, const void* x, int x_pitch, int N, int H, int W, int C,
                           const float* stats, int norm, float slope, int pool, float drop_p, uint32_t seed, float* rstats, void* dx, int dx_pitch,
                           float* part_ws) {
  ActParams p;
  if (int e = fill_act(p, dt, N, H, W, C, x ? x_pitch : C, dy_pitch, norm, slope, pool, drop_p, seed)) return e;
  REQUIRE(mode >= 0 && mode <= 2, "bad mode");
  if (int e = check_ptr16(dy, "dy")) return e;
  REQUIRE(!norm || (stats && x), "norm needs stats and x");
  REQUIRE(mode == 0 || (norm && rstats), "modes 1/2 need norm and rstats");   // mode 0: rstats (nullable) = float[C] += column sums of dx
  REQUIRE(mode == 1 || dx, "dx is null");
  REQUIRE(!dx || dx_pitch % (16 / es_of(dt)) == 0, "dx pitch %d must be a multiple of %d", dx_pitch, 16 / es_of(dt));
  REQUIRE(!(mode == 1 || (mode == 0 && rstats)) || part_ws, "a reduction into rstats needs part_ws");
  const void* xx = x ? x : dy;
  CHECK_HIP(tfc_launch_act_bwd(dt, mode, p, dy, xx, stats, rstats, dx ? dx : (void*)dy, x ? 1 : 0, dx_pitch, part_ws, (hipStream_t)stream), "tfc_act_bwd");
  return 0;
}

extern "C" int tfc_act_bwd_signs(void* stream, int dt, const void* dy, int dy_pitch, const unsigned char* sign_mask, int N, int H, int W, int C, float slope,
                                 float* rstats, void* dx, int dx_pitch, float* part_ws) {
  ActParams p;
  REQUIRE(dt == TFC_DT_BF16 && C == 64, "tfc_act_bwd_signs: bf16, 64 channels");
  if (int e = fill_act(p, dt, N, H, W, C, C, dy_pitch, 0, slope, 2, 0.f, 0)) return e;
  if (int e = check_ptr16(dy, "dy")) return e;
  REQUIRE(sign_mask && dx, "sign_mask / dx is null");
  REQUIRE(dx_pitch % 8 == 0, "dx pitch %d must be a multiple of 8", dx_pitch);
  REQUIRE(!rstats || part_ws, "a reduction into rstats needs part_ws");
  CHECK_HIP(tfc_launch_act_pool2_bwd_signs(p, dy, sign_mask, rstats, dx, dx_pitch, part_ws, (hipStream_t)stream), "tfc_act_bwd_signs");
  return 0;
}

extern "C" int tfc_dropout_mask(void* stream, uint8_t* keep, long long n, float drop_p, uint32_t seed) {
  REQUIRE(keep && n > 0, "bad args");
  CHECK_HIP(tfc_launch_dropout_mask(keep, n, seed, (unsigned)lrintf(drop_p * 16777216.f), (hipStream_t)stream), "tfc_dropout_mask");
  return 0;
}

extern "C" int tfc_pack_nhwc8(void* stream, int dt, const float* a, int Ca, const float* b, int Cb, void* out, int N, int H, int W) {
  REQUIRE(a && out && N > 0 && H > 0 && W > 0 && Ca > 0 && Cb >= 0 && Ca + Cb <= 8 && (Cb == 0 || b), "bad args");
  CHECK_HIP(tfc_launch_pack_nhwc8(dt, a, Ca, b, Cb, out, N, H * W, (hipStream_t)stream), "tfc_pack_nhwc8");
  return 0;
}
extern "C" int tfc_unpack_nchw(void* stream, int dt, const void* in, int pitch, int c0, int C, float* out, int N, int H, int W, float alpha, float beta) {
  REQUIRE(in && out && C > 0 && c0 >= 0 && c0 + C <= pitch, "bad args");
  CHECK_HIP(tfc_launch_unpack_nchw(dt, in, pitch, c0, C, out, N, H * W, alpha, beta, (hipStream_t)stream), "tfc_unpack_nchw");
  return 0;
}
extern "C" int tfc_tanh_bwd_pack(void* stream, int dt, const float* g, const float* y, void* dyraw, float* dbias, int N, int C, int H, int W, float* part_ws) {
  REQUIRE(g && y && dyraw && N > 0 && H > 0 && W > 0 && C > 0 && C <= 4, "bad args (C <= 4)");
  REQUIRE(!dbias || part_ws, "dbias needs part_ws");
  CHECK_HIP(tfc_launch_tanh_bwd_pack(dt, g, y, dyraw, dbias, part_ws, N, C, H * W, (hipStream_t)stream), "tfc_tanh_bwd_pack");
  return 0;
}
extern "C" int tfc_colsum(void* stream, int dt, const void* x, long long rows, int pitch, int C, float* out, float* part_ws) {
  if (int e = check_dt(dt)) return e;
  const int ue = 16 / es_of(dt);
  REQUIRE(out && rows > 0 && C > 0 && C % ue == 0, "bad args");
  if (int e = check_ptr16(x, "x")) return e;                      // the kernel reads 16-byte units at x + row * pitch + cv * ue
  if (int e = check_pitch(dt, pitch, C, "x")) return e;
  CHECK_HIP(tfc_launch_colsum(dt, x, rows, pitch, C, out, part_ws, (hipStream_t)stream), "tfc_colsum");
  return 0;
}
extern "C" int tfc_cast(void* stream, int dt, int to_f32, const void* x, void* y, long long n) {
  REQUIRE(x && y && n > 0, "bad args");
  CHECK_HIP(tfc_launch_cast(dt, to_f32, x, y, n, (hipStream_t)stream), "tfc_cast");
  return 0;
}
extern "C" int tfc_axpby(void* stream, float* out, const float* x, const float* y, long long n, float a, float b) {
  REQUIRE(out && x && n > 0, "bad args");
  CHECK_HIP(tfc_launch_axpby(out, x, y, n, a, b, (hipStream_t)stream), "tfc_axpby");
  return 0;
}

extern "C" size_t tfc_spectral_norm_batched_ws_floats(int nlayers, const int* R, const int* K) {
  size_t n = 0;                                                   // per layer: (R / 32 row-block partials of W^T u) x K  +  s = W v (R)
  for (int i = 0; i < nlayers; ++i) n += (size_t)((R[i] + 31) / 32) * K[i] + R[i];
  return n;
}
extern "C" int tfc_spectral_norm_step_batched(void* stream, int nlayers, const float* const* W, float* const* u, float* const* v,
                                              float* const* sigma2, float* const* u_snap, float* const* v_snap, const int* R,
                                              const int* K, float* ws, int power_iter) {
  REQUIRE(nlayers >= 1 && nlayers <= 4 && W && u && v && sigma2 && R && K && ws, "bad args (1..4 layers)");
  SnBatch b{};
  b.n = nlayers;
  float* wp = ws;                                                // [t partials of layer 0 | s_0 | t partials of layer 1 | s_1 | ...]
  for (int i = 0; i < nlayers; ++i) {
    REQUIRE(W[i] && u[i] && v[i] && sigma2[i] && R[i] > 0 && K[i] > 0 && R[i] <= 4096, "bad layer %d", i);
    b.W[i] = W[i]; b.u[i] = u[i]; b.v[i] = v[i]; b.sigma2[i] = sigma2[i];
    b.us[i] = u_snap ? u_snap[i] : nullptr;
    b.vs[i] = v_snap ? v_snap[i] : nullptr;
    b.R[i] = R[i]; b.K[i] = K[i];
    b.t[i] = wp; wp += (size_t)((R[i] + 31) / 32) * K[i];
    b.s[i] = wp; wp += R[i];
  }
  CHECK_HIP(tfc_launch_sn_step_batched(b, power_iter, 1e-12f, (hipStream_t)stream), "tfc_spectral_norm_step_batched");
  return 0;
}
extern "C" int tfc_spectral_norm_step(void* stream, const float* W, float* u, float* v, float* sigma2, float* ws, int R, int K, int power_iter) {
  REQUIRE(W && u && v && sigma2 && ws && R > 0 && K > 0, "bad args");
  return tfc_spectral_norm_step_batched(stream, 1, &W, &u, &v, &sigma2, nullptr, nullptr, &R, &K, ws, power_iter);
}
extern "C" int tfc_spectral_norm_bwd(void* stream, const float* G, const float* W, const float* u, const float* v, const float* sigma2,
                                     float* ws, float* gout, int R, int K, int accumulate) {
  REQUIRE(G && W && u && v && sigma2 && ws && gout && R > 0 && K > 0 && (((uintptr_t)ws) & 7) == 0, "bad args (ws: 256 floats, 8-byte aligned)");
  CHECK_HIP(tfc_launch_sn_bwd(G, W, u, v, sigma2, ws, gout, R, K, accumulate, (hipStream_t)stream), "tfc_spectral_norm_bwd");
  return 0;
}

// the patch triplet head on a grid x grid patch grid (grid 4 IS tfc_patch16_triplet, whichever entry point it came through)
static int patch_triplet(void* stream, const float* fake, const float* real, const int* neg_idx_host, int grid, int N, int C, float* loss, float* dfake,
                         float gscale) {
  REQUIRE(fake && real && neg_idx_host && loss && N > 0 && C > 0, "bad args");
  if (grid == 2)
    REQUIRE(((uintptr_t)fake & 7) == 0 && ((uintptr_t)real & 7) == 0 && ((uintptr_t)dfake & 7) == 0, "fake / real / dfake must be 8-byte aligned (pixel pairs)");
  for (int i = 0; i < grid * grid; ++i) REQUIRE(neg_idx_host[i] >= 0 && neg_idx_host[i] < grid * grid, "neg_idx[%d]=%d out of range", i, neg_idx_host[i]);
  CHECK_HIP(tfc_launch_patch_triplet(grid, fake, real, neg_idx_host, N, C, 1.0f, 1e-6f, loss, dfake, gscale, (hipStream_t)stream),
            grid == 4 ? "tfc_patch16_triplet" : "tfc_patch_triplet");
  return 0;
}
extern "C" int tfc_patch16_triplet(void* stream, const float* fake, const float* real, const int* neg_idx_host, int N, int C, float* loss, float* dfake, float gscale) {
  return patch_triplet(stream, fake, real, neg_idx_host, 4, N, C, loss, dfake, gscale);
}
extern "C" int tfc_patch_triplet(void* stream, const float* fake, const float* real, const int* neg_idx_host, int grid, int N, int C, float* loss, float* dfake, float gscale) {
  REQUIRE(grid == 2 || grid == 4, "grid=%d: the patch grid is 2 (four 128 x 128 patches) or 4 (sixteen 64 x 64 patches)", grid);
  return patch_triplet(stream, fake, real, neg_idx_host, grid, N, C, loss, dfake, gscale);
}
extern "C" size_t tfc_fft_spectrum_ws_bytes(int S, int nwin) { return (S == 64 || S == 128 || S == 256) && nwin > 0 ? tfc_fft_ws_bytes(S, S, nwin) : 0; }
extern "C" int tfc_fft_spectrum(void* stream, const float* img, long long batch_stride, long long chan_stride, int row_stride, int C, int S,
                                int wins_x, int wins_y, int N, float* amp, float* pha, int shift, void* ws) {
  REQUIRE(img && amp && pha && (S == 64 || S == 128 || S == 256) && (C == 1 || C == 3) && wins_x > 0 && wins_y > 0 && N > 0, "bad args");
  if (ws) { if (int e = check_ptr16(ws, "ws")) return e; }
  const TfcWinGrid g = {batch_stride, chan_stride, row_stride, C, 0, S, S, wins_x, wins_x * wins_y};
  CHECK_HIP(tfc_launch_spectrum(img, g, S, S, false, N * wins_x * wins_y, amp, pha, shift, ws, (hipStream_t)stream), "tfc_fft_spectrum");
  return 0;
}
extern "C" size_t tfc_fft_spectrum_rect_ws_bytes(int H, int nwin) { return H >= 2 && H <= 256 && nwin > 0 ? tfc_fft_ws_bytes(256, H, nwin) : 0; }
extern "C" int tfc_fft_spectrum_rect(void* stream, const float* img, long long batch_stride, long long chan_stride, int row_stride, int C, int img_h,
                                     int img_w, int H, int row0, int row_step, int wins_per_img, int N, float* amp, float* pha, int shift, void* ws) {
  REQUIRE(H >= 2 && H <= 256, "H=%d: a rectangular window has 2 .. 256 rows", H);
  REQUIRE(img_w >= 256, "image width %d: a rectangular window is 256 columns wide", img_w);
  REQUIRE(img && amp && pha && (C == 1 || C == 3) && wins_per_img > 0 && N > 0 && row0 >= 0 && row_step >= 0 && row_stride >= img_w, "bad args");
  REQUIRE((long long)row0 + (long long)(wins_per_img - 1) * row_step + H <= img_h, "windows of %d rows from row %d every %d rows (%d per image) pass the image height %d",
          H, row0, row_step, wins_per_img, img_h);
  if (int e = check_ptr16(ws, "ws")) return e;
  const TfcWinGrid g = {batch_stride, chan_stride, row_stride, C, row0, row_step, 0, 1, wins_per_img};
  CHECK_HIP(tfc_launch_spectrum(img, g, 256, H, true, N * wins_per_img, amp, pha, shift, ws, (hipStream_t)stream), "tfc_fft_spectrum_rect");
  return 0;
}
extern "C" int tfc_batch_kl_sum(void* stream, const float* af, const float* pf, const float* ar, int N, long long M, float scale, float* out) {
  REQUIRE(af && pf && ar && out && N > 0 && M > 0, "bad args");
  CHECK_HIP(tfc_launch_batch_kl(af, pf, ar, N, M, scale, out, (hipStream_t)stream), "tfc_batch_kl_sum");
  return 0;
}
extern "C" int tfc_batch_kl_stats(void* stream, const float* af, const float* pf, const float* ar, int N, long long M, void* rec) {
  REQUIRE(af && pf && ar && rec, "null argument");
  REQUIRE(N > 0 && M >= 1, "bad dims N=%d M=%lld (N >= 1, M >= 1)", N, M);
  REQUIRE((((uintptr_t)rec) & 7) == 0, "rec must be 8-byte aligned");
  CHECK_HIP(tfc_launch_batch_kl_stats(af, pf, ar, N, M, rec, (hipStream_t)stream), "tfc_batch_kl_stats");
  return 0;
}
extern "C" int tfc_batch_kl_merge(void* stream, const void* recs, int world, long long M, void* glob) {
  REQUIRE(recs && glob, "null argument");
  REQUIRE(world >= 1 && world <= 64, "world=%d (1 .. 64 records)", world);
  REQUIRE(M >= 1, "M=%lld (M >= 1)", M);
  REQUIRE(((((uintptr_t)recs) | ((uintptr_t)glob)) & 7) == 0, "recs / glob must be 8-byte aligned");
  CHECK_HIP(tfc_launch_batch_kl_merge(recs, world, M, glob, (hipStream_t)stream), "tfc_batch_kl_merge");
  return 0;
}
extern "C" int tfc_batch_kl_terms(void* stream, const float* af, const float* pf, const float* ar, int N, long long M, const void* glob, float scale,
                                  float* out) {
  REQUIRE(af && pf && ar && glob && out, "null argument");
  REQUIRE(N > 0 && M >= 1, "bad dims N=%d M=%lld (N >= 1, M >= 1)", N, M);
  REQUIRE((((uintptr_t)glob) & 7) == 0, "glob must be 8-byte aligned");
  CHECK_HIP(tfc_launch_batch_kl_terms(af, pf, ar, N, M, glob, scale, out, (hipStream_t)stream), "tfc_batch_kl_terms");
  return 0;
}
extern "C" int tfc_logmag_mse(void* stream, const float* amp_a, const float* amp_b, int S, int nwin, float* out) {
  REQUIRE(amp_a && amp_b && out && (S == 64 || S == 128 || S == 256) && nwin > 0, "bad args");
  CHECK_HIP(tfc_launch_logmag_mse(amp_a, amp_b, S, nwin, out, 0, (hipStream_t)stream), "tfc_logmag_mse");
  return 0;
}
extern "C" int tfc_logmag_mae(void* stream, const float* amp_a, const float* amp_b, int S, int nwin, float* out) {
  REQUIRE(amp_a && amp_b && out && (S == 64 || S == 128 || S == 256) && nwin > 0, "bad args");
  CHECK_HIP(tfc_launch_logmag_mse(amp_a, amp_b, S, nwin, out, 1, (hipStream_t)stream), "tfc_logmag_mae");
  return 0;
}
// ---- evaluation metrics (metrics.hip) ----------------------------------------------------------------------------------------------------------
#define TFC_METRIC_MAX_COUNT (1ll << 23)    // elements per image: keeps count * (sum of squares) of the NCC finaliser inside 63 bits
#define TFC_METRIC_MAX_N 65535              // images per call (a grid dimension)
extern "C" size_t tfc_pair_moments_ws_bytes(int N, long long count) {
  return N > 0 && count > 0 && count <= TFC_METRIC_MAX_COUNT ? (size_t)N * tfc_moments_groups(count) * 10 * sizeof(long long) : 0;
}
extern "C" int tfc_pair_moments_u8(void* stream, const uint8_t* a, long long a_stride, const uint8_t* b, long long b_stride, long long count, int N,
                                   void* ws, long long* moments, double* psnr, double* ncc) {
  REQUIRE(a && b && ws && moments, "a, b, ws and moments must be device pointers");
  REQUIRE(N > 0 && N <= TFC_METRIC_MAX_N, "N = %d: 1 .. %d images per call", N, TFC_METRIC_MAX_N);
  REQUIRE(count > 0 && count <= TFC_METRIC_MAX_COUNT, "count = %lld: 1 .. 2^23 elements per image", count);
  REQUIRE(a_stride >= count && b_stride >= count, "image strides (%lld, %lld) are smaller than the image (%lld bytes)", a_stride, b_stride, count);
  REQUIRE((((uintptr_t)ws | (uintptr_t)moments) & 7) == 0, "ws and moments must be 8-byte aligned");
  CHECK_HIP(tfc_launch_pair_moments(a, b, a_stride, b_stride, count, N, (long long*)ws, moments, psnr, ncc, (hipStream_t)stream), "tfc_pair_moments_u8");
  return 0;
}
extern "C" size_t tfc_ssim_ws_bytes(int N, int H, int W, int wy, int wx) {
  if (N <= 0 || wy <= 0 || wx <= 0 || H < wy || W < wx) return 0;
  int tx, ty;
  tfc_ssim_tiles(H, W, wy, wx, &tx, &ty);
  return (size_t)N * tx * ty * sizeof(double);
}
extern "C" int tfc_ssim_u8(void* stream, const uint8_t* a, long long a_img_stride, int a_row_stride, const uint8_t* b, long long b_img_stride,
                           int b_row_stride, int N, int H, int W, int wy, int wx, double data_range, void* ws, double* out) {
  REQUIRE(a && b && ws && out, "a, b, ws and out must be device pointers");
  REQUIRE((wy == 7 && wx == 7) || (wy == 7 && wx == 1), "window (wy, wx) = (%d, %d): (7, 7) and (7, 1) are supported", wy, wx);
  REQUIRE(H >= wy && W >= wx, "image %d x %d is smaller than the %d x %d SSIM window", H, W, wy, wx);
  REQUIRE(N > 0 && N <= TFC_METRIC_MAX_N, "N = %d: 1 .. %d images per call", N, TFC_METRIC_MAX_N);
  REQUIRE((long long)H * W <= TFC_METRIC_MAX_COUNT, "image %d x %d: at most 2^23 pixels", H, W);
  REQUIRE(a_row_stride >= W && b_row_stride >= W && a_img_stride >= (long long)(H - 1) * a_row_stride + W &&
          b_img_stride >= (long long)(H - 1) * b_row_stride + W, "strides do not cover a %d x %d image", H, W);
  REQUIRE(data_range > 0.0, "data_range must be positive");
  REQUIRE((((uintptr_t)ws | (uintptr_t)out) & 7) == 0, "ws and out must be 8-byte aligned");
  CHECK_HIP(tfc_launch_ssim(a, a_img_stride, a_row_stride, b, b_img_stride, b_row_stride, N, H, W, wy, wx, data_range, (double*)ws, out, (hipStream_t)stream),
            "tfc_ssim_u8");
  return 0;
}
extern "C" int tfc_hist_u8_color(void* stream, const uint8_t* img, long long img_stride, long long pix_stride, long long chan_stride, long long npix, int N,
                                 uint32_t* hist) {
  REQUIRE(img && hist && (((uintptr_t)hist) & 3) == 0, "img and hist must be device pointers");
  REQUIRE(N > 0 && N <= TFC_METRIC_MAX_N, "N = %d: 1 .. %d images per call", N, TFC_METRIC_MAX_N);
  REQUIRE(npix > 0 && npix <= TFC_METRIC_MAX_COUNT, "npix = %lld: 1 .. 2^23 pixels per image", npix);
  REQUIRE(pix_stride > 0 && chan_stride >= 0 && img_stride >= (npix - 1) * pix_stride + 2 * chan_stride + 1,
          "strides (image %lld, pixel %lld, channel %lld) do not cover %lld pixels", img_stride, pix_stride, chan_stride, npix);
  CHECK_HIP(tfc_launch_hist_color(img, img_stride, pix_stride, chan_stride, npix, N, hist, (hipStream_t)stream), "tfc_hist_u8_color");
  return 0;
}
extern "C" int tfc_hist_u8_joint(void* stream, const uint8_t* a, long long a_stride, const uint8_t* b, long long b_stride, long long count, int N,
                                 const uint8_t* lut_a, const uint8_t* lut_b, int nb, uint32_t* hist) {
  REQUIRE(a && b && lut_a && lut_b && hist && (((uintptr_t)hist) & 3) == 0, "a, b, the tables and hist must be device pointers");
  REQUIRE(N > 0 && N <= TFC_METRIC_MAX_N, "N = %d: 1 .. %d images per call", N, TFC_METRIC_MAX_N);
  REQUIRE(count > 0 && count <= TFC_METRIC_MAX_COUNT && a_stride >= count && b_stride >= count, "count = %lld (1 .. 2^23) with strides %lld, %lld", count,
          a_stride, b_stride);
  REQUIRE(nb >= 1 && nb <= 32, "nb = %d: 1 .. 32 bins per axis", nb);
  CHECK_HIP(tfc_launch_hist_joint(a, b, a_stride, b_stride, count, N, lut_a, lut_b, nb, hist, (hipStream_t)stream), "tfc_hist_u8_joint");
  return 0;
}
extern "C" int tfc_mi_bin_lut(void* stream, const long long* moments, int N, int nb, int edge_f32, uint8_t* lut_a, uint8_t* lut_b) {
  REQUIRE(moments && lut_a && lut_b, "moments and the tables must be device pointers");
  REQUIRE(N > 0 && N <= TFC_METRIC_MAX_N && nb >= 1 && nb <= 32, "N = %d (1 .. %d), nb = %d (1 .. 32)", N, TFC_METRIC_MAX_N, nb);
  CHECK_HIP(tfc_launch_mi_lut(moments, N, nb, edge_f32 ? 1 : 0, lut_a, lut_b, (hipStream_t)stream), "tfc_mi_bin_lut");
  return 0;
}
extern "C" int tfc_bhattacharyya(void* stream, const uint32_t* h1, const uint32_t* h2, int N, int nbins, double* out) {
  REQUIRE(h1 && h2 && out && N > 0 && nbins > 0 && (((uintptr_t)out) & 7) == 0, "bad args");
  CHECK_HIP(tfc_launch_bhattacharyya(h1, h2, N, nbins, out, (hipStream_t)stream), "tfc_bhattacharyya");
  return 0;
}
extern "C" int tfc_mutual_information(void* stream, const uint32_t* hist, int N, int nb, double* out) {
  REQUIRE(hist && out && N > 0 && nb >= 1 && nb <= 32 && (((uintptr_t)out) & 7) == 0, "bad args");
  CHECK_HIP(tfc_launch_mutual_information(hist, N, nb, out, (hipStream_t)stream), "tfc_mutual_information");
  return 0;
}
extern "C" int tfc_vectorize_temps(void* stream, const float* img, long long batch_stride, int row_stride, int N, int H, int W,
                                  const float* lut256, float* out) {
  REQUIRE(img && lut256 && out && N > 0 && H > 0 && W > 0 && row_stride >= W && batch_stride >= (long long)H * row_stride, "bad args");
  CHECK_HIP(tfc_launch_vectorize_temps(img, batch_stride, row_stride, N, H, W, lut256, out, (hipStream_t)stream), "tfc_vectorize_temps");
  return 0;
}
extern "C" int tfc_row_triplet(void* stream, const float* anchor, const float* positive, const float* negative, long long rows, int W,
                              float margin, float* loss) {
  REQUIRE(anchor && positive && negative && loss && rows > 0 && W > 0, "bad args");
  CHECK_HIP(tfc_launch_row_triplet(anchor, positive, negative, rows, W, margin, 1e-6f, loss, (hipStream_t)stream), "tfc_row_triplet");
  return 0;
}
extern "C" int tfc_affine_warp_fwd(void* stream, const float* src, const float* theta, float* out, int N, int C, int H, int W) {
  REQUIRE(src && theta && out && N > 0 && C > 0 && H > 1 && W > 1, "bad args");
  CHECK_HIP(tfc_launch_affine_warp_fwd(src, theta, out, N, C, H, W, 1, (hipStream_t)stream), "tfc_affine_warp_fwd");
  return 0;
}
extern "C" int tfc_affine_warp_bwd(void* stream, const float* src, const float* theta, const float* gout, float* dtheta, float* dsrc, int N, int C,
                                   int H, int W, float* part_ws) {
  REQUIRE(src && theta && gout && dtheta && part_ws && N > 0 && C > 0 && H > 1 && W > 1, "bad args");
  CHECK_HIP(tfc_launch_affine_warp_bwd(src, theta, gout, dtheta, dsrc, part_ws, N, C, H, W, 1, (hipStream_t)stream), "tfc_affine_warp_bwd");
  return 0;
}
// the same pair with the sampling convention as an argument (sample_align_corners != 0: the bits of the pair above); H and W >= 1
extern "C" int tfc_affine_warp_mode_fwd(void* stream, const float* src, const float* theta, float* out, int N, int C, int H, int W, int sample_align_corners) {
  REQUIRE(src && theta && out && N > 0 && C > 0 && H > 0 && W > 0, "bad args");
  REQUIRE((long long)N * C * H * W < (1LL << 40) && (long long)H * W < 2147483647LL, "image too large");
  CHECK_HIP(tfc_launch_affine_warp_fwd(src, theta, out, N, C, H, W, sample_align_corners ? 1 : 0, (hipStream_t)stream), "tfc_affine_warp_mode_fwd");
  return 0;
}
extern "C" int tfc_affine_warp_mode_bwd(void* stream, const float* src, const float* theta, const float* gout, float* dtheta, float* dsrc, int N, int C,
                                        int H, int W, int sample_align_corners, float* part_ws) {
  REQUIRE(src && theta && gout && dtheta && part_ws && N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0, "bad args (1 <= N <= 65535)");
  REQUIRE((long long)H * W < 2147483647LL, "image too large");
  CHECK_HIP(tfc_launch_affine_warp_bwd(src, theta, gout, dtheta, dsrc, part_ws, N, C, H, W, sample_align_corners ? 1 : 0, (hipStream_t)stream),
            "tfc_affine_warp_mode_bwd");
  return 0;
}
// ---- STN21 localiser (vit.hip) ----
static bool vit_unfold_ok(const TfcVitGemm& g, int rows, int cols) {
  if (g.uc <= 0 || g.up <= 0 || g.uh <= 0 || g.uw <= 0 || g.uh % g.up || g.uw % g.up) return false;
  return cols <= 2 * g.uc * g.up * g.up && rows % ((g.uh / g.up) * (g.uw / g.up)) == 0;
}
extern "C" int tfc_vit_gemm(void* stream, int dt, const TfcVitGemm* gp, float* part_ws) {
  REQUIRE(gp, "bad args");
  const TfcVitGemm& g = *gp;
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32, "tfc_vit_gemm: dt %d (bf16 or fp32 only; the ViT kernels do not support TFC_DT_BF16X3)", dt);
  REQUIRE(g.M > 0 && g.N > 0 && g.K > 0 && g.a && g.b, "tfc_vit_gemm: bad shape / operands (%d x %d x %d)", g.M, g.N, g.K);
  REQUIRE(g.a_mode >= TFC_VIT_A_ROWS && g.a_mode <= TFC_VIT_A_UNFOLD && g.b_mode >= TFC_VIT_B_WEIGHT && g.b_mode <= TFC_VIT_B_UNFOLD &&
          (g.c_mode == TFC_VIT_C_ROWS || g.c_mode == TFC_VIT_C_UNFOLD) && g.act >= TFC_VIT_ACT_NONE && g.act <= TFC_VIT_DACT_SIGMOID, "tfc_vit_gemm: mode");
  REQUIRE(g.a_mode != TFC_VIT_A_ROWS || g.a_rg > 0 || g.lda >= g.K, "tfc_vit_gemm: lda");
  REQUIRE(g.a_mode != TFC_VIT_A_TRANS || g.a_rg > 0 || g.lda >= g.M, "tfc_vit_gemm: lda");
  REQUIRE(g.b_mode != TFC_VIT_B_WEIGHT || g.ldb >= g.K, "tfc_vit_gemm: ldb");
  REQUIRE(g.b_mode != TFC_VIT_B_ROWS || g.ldb >= g.N, "tfc_vit_gemm: ldb");
  REQUIRE(g.a_mode != TFC_VIT_A_UNFOLD || (g.a2 && vit_unfold_ok(g, g.M, g.K)), "tfc_vit_gemm: A unfold geometry");
  REQUIRE(g.b_mode != TFC_VIT_B_UNFOLD || (g.b2 && vit_unfold_ok(g, g.K, g.N)), "tfc_vit_gemm: B unfold geometry");
  REQUIRE(g.c_mode != TFC_VIT_C_ROWS || (g.c && (g.c_rg > 0 || g.ldc >= g.N)), "tfc_vit_gemm: C");
  REQUIRE(g.c_mode != TFC_VIT_C_UNFOLD || ((g.c || g.c2) && !g.res && vit_unfold_ok(g, g.M, g.N)), "tfc_vit_gemm: C unfold geometry");
  REQUIRE(g.act == TFC_VIT_ACT_NONE || g.act == TFC_VIT_ACT_RELU || g.act == TFC_VIT_ACT_SIGMOID || (g.aux && g.ldaux >= g.N), "tfc_vit_gemm: aux");
  CHECK_HIP(tfc_launch_vit_gemm(dt, g, part_ws, (hipStream_t)stream), "tfc_vit_gemm");
  return 0;
}
extern "C" int tfc_vit_layernorm_fwd(void* stream, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int rows, int D,
                                     float eps) {
  REQUIRE(x && gamma && beta && y && mean && rstd && rows > 0 && D > 0 && D % 64 == 0 && D <= 1024, "bad args");
  CHECK_HIP(tfc_launch_vit_ln_fwd(x, gamma, beta, y, mean, rstd, rows, D, eps, (hipStream_t)stream), "tfc_vit_layernorm_fwd");
  return 0;
}
extern "C" int tfc_vit_layernorm_bwd(void* stream, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dres,
                                     float* dx, float* dgb, int rows, int D, float* part_ws) {
  REQUIRE(dy && x && mean && rstd && gamma && dx && rows > 0 && D > 0 && D % 64 == 0 && D <= 1024 && (!dgb || part_ws), "bad args");
  CHECK_HIP(tfc_launch_vit_ln_bwd(dy, x, mean, rstd, gamma, dres, dx, dgb, rows, D, part_ws, (hipStream_t)stream), "tfc_vit_layernorm_bwd");
  return 0;
}
extern "C" int tfc_vit_colsum(void* stream, const float* v, long long ld, int rows, int L, float* out, float* part_ws) {
  REQUIRE(v && out && part_ws && rows > 0 && L > 0 && ld >= L, "bad args");
  CHECK_HIP(tfc_launch_vit_colsum(v, ld, rows, L, nullptr, nullptr, nullptr, out, part_ws, (hipStream_t)stream), "tfc_vit_colsum");
  return 0;
}
extern "C" int tfc_vit_attention_fwd(void* stream, int dt, const float* qkv, float* out, float* probs, int N, int T, int H, float scale) {
  REQUIRE(qkv && out && probs && N > 0 && T > 0 && T <= 64 && H > 0, "bad args");
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32, "dt %d: the ViT kernels run bf16 or fp32 only (TFC_DT_BF16X3 is not supported)", dt);
  CHECK_HIP(tfc_launch_vit_attn_fwd(dt, qkv, out, probs, N, T, H, scale, (hipStream_t)stream), "tfc_vit_attention_fwd");
  return 0;
}
extern "C" int tfc_vit_attention_bwd(void* stream, int dt, const float* dout, const float* qkv, const float* probs, float* dqkv, int N, int T, int H,
                                     float scale) {
  REQUIRE(dout && qkv && probs && dqkv && N > 0 && T > 0 && T <= 64 && H > 0, "bad args");
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32, "dt %d: the ViT kernels run bf16 or fp32 only (TFC_DT_BF16X3 is not supported)", dt);
  CHECK_HIP(tfc_launch_vit_attn_bwd(dt, dout, qkv, probs, dqkv, N, T, H, scale, (hipStream_t)stream), "tfc_vit_attention_bwd");
  return 0;
}
// the tiled pair: any 1 <= T <= 1025 (512 x 512 at patch 16); every refusal names its entry point
#define REQUIRE_ATTN_TILED(name, ptrs_ok) do { \
    REQUIRE(ptrs_ok, name ": null pointer"); \
    REQUIRE(T >= 1 && T <= 1025, name ": T = %d tokens (1 <= T <= 1025)", T); \
    REQUIRE(N > 0 && N <= 65535 && H > 0 && H <= 65535, name ": bad dims N=%d H=%d", N, H); \
    REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32, name ": dt %d: the ViT kernels run bf16 or fp32 only (TFC_DT_BF16X3 is not supported)", dt); \
  } while (0)
extern "C" int tfc_vit_attention_tiled_fwd(void* stream, int dt, const float* qkv, float* out, float* stats, int N, int T, int H, float scale) {
  REQUIRE_ATTN_TILED("tfc_vit_attention_tiled_fwd", qkv && out && stats);
  CHECK_HIP(tfc_launch_vit_attn_tiled_fwd(dt, qkv, out, stats, N, T, H, scale, (hipStream_t)stream), "tfc_vit_attention_tiled_fwd");
  return 0;
}
extern "C" int tfc_vit_attention_tiled_bwd(void* stream, int dt, const float* dout, const float* qkv, const float* stats, float* dqkv, int N, int T, int H,
                                           float scale, float* ws) {
  REQUIRE_ATTN_TILED("tfc_vit_attention_tiled_bwd", dout && qkv && stats && dqkv && ws);
  CHECK_HIP(tfc_launch_vit_attn_tiled_bwd(dt, dout, qkv, stats, dqkv, ws, N, T, H, scale, (hipStream_t)stream), "tfc_vit_attention_tiled_bwd");
  return 0;
}
extern "C" int tfc_vit_tokens_fwd(void* stream, float* x, const float* cls, const float* pos, int N, int T, int D) {
  REQUIRE(x && cls && pos && N > 0 && T > 0 && D > 0, "bad args");
  CHECK_HIP(tfc_launch_vit_tokens_fwd(x, cls, pos, N, T, D, (hipStream_t)stream), "tfc_vit_tokens_fwd");
  return 0;
}
extern "C" int tfc_morph_grad_fwd(void* stream, const float* x, float* out, uint8_t* arg, long long planes, int H, int W) {
  REQUIRE(x && out && planes > 0 && H > 0 && W > 0, "bad args");
  CHECK_HIP(tfc_launch_morph_grad_fwd(x, out, arg, planes, H, W, (hipStream_t)stream), "tfc_morph_grad_fwd");
  return 0;
}
extern "C" int tfc_morph_grad_bwd(void* stream, const float* gout, const uint8_t* arg, float* dx, long long planes, int H, int W) {
  REQUIRE(gout && arg && dx && planes > 0 && H > 0 && W > 0, "bad args");
  CHECK_HIP(tfc_launch_morph_grad_bwd(gout, arg, dx, planes, H, W, (hipStream_t)stream), "tfc_morph_grad_bwd");
  return 0;
}
extern "C" int tfc_row_triplet_grad(void* stream, const float* anchor, const float* positive, const float* negative, long long rows, int W,
                                   float margin, float gscale, float* loss, float* danchor) {
  REQUIRE(anchor && positive && negative && loss && rows > 0 && W > 0, "bad args");
  CHECK_HIP(tfc_launch_row_triplet_grad(anchor, positive, negative, rows, W, margin, 1e-6f, gscale, loss, danchor, (hipStream_t)stream), "tfc_row_triplet_grad");
  return 0;
}
// ---- input pipeline (input.hip) ---------------------------------------------------------------------------------------------------
namespace {
// Pillow's bicubic kernel (a = -0.5) and coefficient precomputation (src/libImaging/Resample.c: bicubic_filter, precompute_coeffs,
// normalize_coeffs_8bpc), restated: the SAME double arithmetic in the same order, so the quantised taps are identical to PIL's.
double pil_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
int pil_ksize(int in_size, int out_size) {
  double fs = (double)in_size / out_size;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(2.0 * fs) * 2 + 1;
}
// bounds[out][2], coef[out][ksize]
void pil_coeffs(int in_size, int out_size, int ksize, int* bounds, int* coef) {
  const double scale = (double)in_size / out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 2.0 * filterscale, ss = 1.0 / filterscale;
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double w = pil_bicubic((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = 0; x < ksize; ++x) {
      const double v = x < xmax ? k[x] : 0.0;
      coef[xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
}
int pil_round_half_even(int w) {                                   // Image.crop rounds its float box with Python's round(): w / 2 for odd w
  if (w % 2 == 0) return w / 2;
  const int k = w / 2;                                             // w / 2 = k + 0.5
  return (k % 2 == 0) ? k : k + 1;
}
size_t resize_plan_ints(int H, int W, int out) {
  const int xs = pil_round_half_even(W);
  const int kA = pil_ksize(xs, out), kB = pil_ksize(W - xs, out), kV = pil_ksize(H, out);
  return (sizeof(TfcResizePlan) + 3) / 4 + (size_t)out * (6 + kA + kB + kV);
}
}  // namespace

extern "C" size_t tfc_resize_plan_bytes(int H, int W, int out) { return (H > 0 && W > 1 && out > 0) ? 4 * resize_plan_ints(H, W, out) : 0; }
extern "C" int tfc_resize_plan_build(int H, int W, int out, void* plan_host) {
  REQUIRE(H > 0 && W > 1 && out > 0 && plan_host, "bad args");
  REQUIRE((long long)H * W < (1 << 28), "image too large");
  TfcResizePlan p;
  memset(&p, 0, sizeof p);
  p.out = out; p.H = H; p.W = W; p.xsplit = pil_round_half_even(W);
  int* base = (int*)plan_host;
  int off = (int)((sizeof(TfcResizePlan) + 3) / 4);
  TfcResizeAxis* axes[3] = {&p.hA, &p.hB, &p.v};
  const int sizes[3] = {p.xsplit, W - p.xsplit, H};
  for (int i = 0; i < 3; ++i) {
    TfcResizeAxis& a = *axes[i];
    a.in_size = sizes[i];
    a.ksize = pil_ksize(sizes[i], out);
    a.bounds_off = off; off += 2 * out;
    a.coef_off = off; off += a.ksize * out;
    pil_coeffs(sizes[i], out, a.ksize, base + a.bounds_off, base + a.coef_off);
  }
  memcpy(plan_host, &p, sizeof p);
  return 0;
}
extern "C" size_t tfc_pair_resize_ws_bytes(int N, int H, int out) { return (N > 0 && H > 0 && out > 0) ? (size_t)N * 2 * H * out * 3 : 0; }
extern "C" int tfc_pair_resize_normalize(void* stream, const uint8_t* src, long long img_stride, int row_stride, int N, const void* plan_host,
                                         const void* plan_dev, void* ws, const float* lut256, float* A, float* B, float* TB, uint8_t* A8, uint8_t* B8) {
  REQUIRE(src && plan_host && plan_dev && ws && A && B && N > 0, "bad args");
  REQUIRE(TB == nullptr || lut256 != nullptr, "T_B needs the 256-entry temperature table");
  TfcResizePlan p;
  memcpy(&p, plan_host, sizeof p);
  REQUIRE(p.out > 0 && p.H > 0 && p.W > 1 && p.xsplit > 0 && p.xsplit < p.W, "corrupt plan header");
  REQUIRE(row_stride >= 3 * p.W && img_stride >= (long long)row_stride * p.H, "strides smaller than the %d x %d RGB image of the plan", p.W, p.H);
  CHECK_HIP(tfc_launch_pair_resize(src, img_stride, row_stride, N, p, (const int*)plan_dev, (uint8_t*)ws, lut256, A, B, TB, A8, B8, (hipStream_t)stream),
            "tfc_pair_resize_normalize");
  return 0;
}

// ---- LPIPS term (lpips.hip) ------------------------------------------------------------------------------------------------------

extern "C" int tfc_lpips_input_fwd(void* stream, int dt, const float* x, const float* shift, const float* scale, void* out, int N, int C, int H, int W,
                                   int pitch) {
  REQUIRE(x && shift && scale && out && N > 0 && C > 0 && C <= 8 && H > 0 && W > 0 && pitch >= 8 && pitch % 8 == 0, "bad args");
  if (int e = check_dt(dt)) return e;
  if (int e = check_ptr16(out, "out")) return e;
  // the kernel writes channels [0, 8) of every pixel; channels [8, pitch) keep what the caller put there (zeros)
  CHECK_HIP(tfc_launch_lpips_input(dt, x, shift, scale, out, N, C, (long long)H * W, pitch, (hipStream_t)stream), "tfc_lpips_input_fwd");
  return 0;
}
extern "C" int tfc_lpips_input_bwd(void* stream, int dt, const void* g, const float* scale, float* dx, int N, int C, int H, int W, int pitch, float alpha,
                                   int accumulate) {
  REQUIRE(g && scale && dx && N > 0 && C > 0 && C <= 8 && H > 0 && W > 0 && pitch >= 8 && pitch % 8 == 0, "bad args");
  if (int e = check_dt(dt)) return e;
  CHECK_HIP(tfc_launch_lpips_input_bwd(dt, g, scale, dx, N, C, (long long)H * W, pitch, alpha, accumulate, (hipStream_t)stream), "tfc_lpips_input_bwd");
  return 0;
}
extern "C" int tfc_maxpool2_fwd(void* stream, int dt, const void* x, void* y, int N, int H, int W, int C) {
  REQUIRE(x && y && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0, "bad args");
  if (int e = check_dt(dt)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(y, "y")) return e;
  CHECK_HIP(tfc_launch_maxpool2(dt, 0, x, nullptr, y, N, H, W, C, (hipStream_t)stream), "tfc_maxpool2_fwd");
  return 0;
}
extern "C" int tfc_maxpool2_bwd(void* stream, int dt, const void* x, const void* dy, void* dx, int N, int H, int W, int C) {
  REQUIRE(x && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0, "bad args");
  if (int e = check_dt(dt)) return e;
  if (int e = check_ptr16(x, "x")) return e;
  if (int e = check_ptr16(dy, "dy")) return e;
  if (int e = check_ptr16(dx, "dx")) return e;
  CHECK_HIP(tfc_launch_maxpool2(dt, 1, x, dy, dx, N, H, W, C, (hipStream_t)stream), "tfc_maxpool2_bwd");
  return 0;
}
extern "C" int tfc_relu_bwd(void* stream, int dt, const void* dy, const void* y, const void* extra, void* dz, long long n) {
  REQUIRE(dy && y && dz && n > 0 && n % 8 == 0, "bad args");
  if (int e = check_dt(dt)) return e;
  if (int e = check_ptr16(dy, "dy")) return e;
  if (int e = check_ptr16(y, "y")) return e;
  if (int e = check_ptr16(dz, "dz")) return e;
  if (extra) { if (int e = check_ptr16(extra, "extra")) return e; }
  CHECK_HIP(tfc_launch_relu_bwd(dt, dy, y, extra, dz, n, (hipStream_t)stream), "tfc_relu_bwd");
  return 0;
}
extern "C" int tfc_lpips_head(void* stream, int dt, const void* fx, const void* fy, const float* w, float* out, void* dfx, int N, int H, int W, int C,
                              float gscale, float* part_ws) {
  REQUIRE(fx && fy && w && out && N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "bad args");
  REQUIRE(part_ws, "tfc_lpips_head adds its workgroup partials in a fixed order: part_ws is required");
  if (int e = check_dt(dt)) return e;
  if (int e = check_ptr16(fx, "fx")) return e;
  if (int e = check_ptr16(fy, "fy")) return e;
  if (dfx) { if (int e = check_ptr16(dfx, "dfx")) return e; }
  CHECK_HIP(tfc_launch_lpips_head(dt, fx, fy, w, out, dfx, part_ws, N, (long long)H * W, C, gscale, (hipStream_t)stream), "tfc_lpips_head");
  return 0;
}
extern "C" int tfc_l1_sum(void* stream, const float* a, const float* b, long long n, float scale, float* out, int zero_first) {
  REQUIRE(a && b && out && n > 0, "bad args");
  if (zero_first) CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float), (hipStream_t)stream), "tfc_l1_sum memset");
  CHECK_HIP(tfc_launch_l1_sum(a, b, n, scale, out, (hipStream_t)stream), "tfc_l1_sum");
  return 0;
}
extern "C" int tfc_bce_relativistic(void* stream, int dt, const void* a, const void* b, int n, int stride, float t1, float t2, int mode,
                                    float* loss, void* da, void* db, float gscale) {
  REQUIRE(a && b && loss && n > 0 && stride > 0 && (mode == 0 || mode == 1), "bad args");
  CHECK_HIP(tfc_launch_bce_rel(dt, a, b, n, stride, t1, t2, mode, loss, da, db, gscale, (hipStream_t)stream), "tfc_bce_relativistic");
  return 0;
}
extern "C" int tfc_adam_step(void* stream, float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps,
                             int step, float gscale) {
  REQUIRE(p && g && m && v && n > 0 && step >= 1, "bad args");
  const float bc1 = 1.f - powf(b1, (float)step);
  const float bc2 = 1.f - powf(b2, (float)step);
  CHECK_HIP(tfc_launch_adam(p, g, m, v, n, lr, b1, b2, eps, bc1, sqrtf(bc2), gscale, (hipStream_t)stream), "tfc_adam_step");
  return 0;
}
extern "C" int tfc_debug_set_igemm_config(int cfg) {
  REQUIRE(cfg >= -1 && cfg <= 31, "cfg must be -1 (heuristic) or tile 0 (128x128) | 1 (128x64) | 2 (128x32) | 3 (128x128, 4 n-waves) | 15 (heuristic tile), "
          "optionally + 16 = the one-tile-per-workgroup gather GEMM instead of the persistent one");
  g_tfc_force_cfg = cfg;
  return 0;
}
extern "C" int tfc_debug_set_persistent_grid(int workgroups) {
  REQUIRE(workgroups >= 0, "workgroups must be 0 (default: occupancy x compute units) or the largest grid of the persistent layer kernels");
  g_tfc_persistent_grid = workgroups;
  return 0;
}
// ---- batch-invariant mode and the launch-plan query ------------------------------------------------------------------------
extern "C" int tfc_set_batch_invariant(int on) {                  // per thread, like the other host-side hooks
  g_tfc_batch_invariant = on ? 1 : 0;
  return 0;
}
extern "C" int tfc_get_batch_invariant(void) { return g_tfc_batch_invariant; }
// Host only, launches nothing: the plan the launchers of (dt, op, pass) would choose on a chip of `ncu` compute units, through the launchers' own decision
// functions. flags: the TFC_EP_* bits of the call, | TFC_PLAN_FIRST_BLOCK for the fused first-block kernels (pass 0: forward, pass 2: backward).
extern "C" int tfc_conv_plan_query(int dt, int op, int pass, int N, int H, int W, int Cin, int Cout, int flags, int ncu, int* out, int n) {
  if (int e = check_common(dt, op, N, H, W, Cin, Cout)) return e;
  REQUIRE(pass >= 0 && pass <= 2 && ncu > 0 && out && n >= 0, "bad pass / ncu / out");
  const bool inv = g_tfc_batch_invariant != 0;
  TfcConvPlan p{};
  if (flags & TFC_PLAN_FIRST_BLOCK) {
    REQUIRE(op == TFC_OP_CONV && pass != 1 && tfc_first_block_bwd_supported(dt, Cin, Cout), "the fused first block: TFC_OP_CONV, bf16, Cin <= 8, Cout == 64, pass 0 or 2");
    tfc_plan_first_block(pass, N, H, W, ncu, inv, &p);
    // what the launcher refuses, the query refuses: one 32 KB slab per workgroup, 2048 of them (batch-invariant mode keeps the reference batch's
    // workgroups per image, so this is N <= 128 at 256 x 256 there)
    REQUIRE(pass != 2 || (long long)N * p.wpi <= 2048, "fused first-block backward: %d images x %d workgroups per image exceed the 2048 slabs of the scratch", N, p.wpi);
  } else if (pass == 2) {
    REQUIRE(op != TFC_OP_CONV3, "TFC_OP_CONV3 has no weight-gradient pass");
    TfcGather d;
    WeightMap wm{};
    if (int e = build_desc(op, 2, 0, N, H, W, Cin, Cout, pad8(Cin), pad8(Cout), &d, &wm)) return e;
    bool fused = false;
    if ((op == TFC_OP_CONVT || op == TFC_OP_UPCONV) && dt == TFC_DT_BF16)
      fused = tfc_plan_wgrad_phases(op == TFC_OP_UPCONV, N, H, W, pad8(Cin), pad8(Cin), Cout, wm.sn % 4 == 0 && wm.sc % 4 == 0, inv, &p);
    if (op == TFC_OP_CONV2 && conv2_wgrad_mirrored(dt))           // as tfc_conv_wgrad: the transposed convolution's launch with the tensors exchanged
      fused = tfc_plan_wgrad_phases(0, N, H / 2, W / 2, pad8(Cout), pad8(Cout), Cin, true, inv, &p);
    if (!fused) tfc_plan_wgrad(dt, d, pad8(Cout), inv, &p, 0);
  } else {
    TfcGather d;
    if (int e = build_desc(op, pass, 0, N, H, W, Cin, Cout, pass ? pad8(Cout) : pad8(Cin), pass ? pad8(Cin) : pad8(Cout), &d, nullptr)) return e;
    if (fold_phases(op, pass)) set_fold(d, op);                   // as tfc_conv_fwd / tfc_conv_dgrad fold the phases
    if (int e = check_desc(d, dt)) return e;
    tfc_plan_igemm(dt, d, flags & 0xffff, ncu, inv, &p);
    if (!(flags & TFC_EP_STATS)) p.nparts = 0;
  }
  const int rec[8] = {p.kernel, p.form, p.nparts, p.nsplit, p.wpi, p.pat, 0, p.per};   // slot 6 (once: flushed with float atomics) is always 0
  for (int i = 0; i < n && i < 8; ++i) out[i] = rec[i];
  return 8;
}
// ---- label plane + auxiliary classifier heads (debias.hip) -----------------------------------------------------------------------------------

static inline bool al16(const void* p) { return p != nullptr && (((uintptr_t)p) & 15) == 0; }
#define REQUIRE_IMAGE(N, H, W) do { \
    REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "bad dims N=%d H=%d W=%d (1 <= N <= 65535)", N, H, W); \
    REQUIRE((long long)H * W < (1LL << 24) && ((long long)H * W) % 4 == 0, "H*W=%lld must be a multiple of 4 below 2^24 (16-byte units of a plane)", (long long)H * W); \
  } while (0)
// class counts of the three heads -> total (<= 16), or a refusal
static int aux_classes(const int* nc, int* total) {
  REQUIRE(nc != nullptr, "nclass3 is null");
  int ct = 0;
  for (int h = 0; h < 3; ++h) {
    REQUIRE(nc[h] >= 1 && nc[h] <= 16, "head %d has %d classes (1 .. 16)", h, nc[h]);
    ct += nc[h];
  }
  REQUIRE(ct <= 16, "%d classes in all: the head kernels hold at most 16 rows", ct);
  *total = ct;
  return 0;
}

extern "C" int tfc_pack_nhwc8_labels(void* stream, int dt, const float* img, const float* labels, const float* fc_w, const float* fc_b, void* out,
                                     int N, int H, int W) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype %d", dt);
  REQUIRE_IMAGE(N, H, W);
  REQUIRE(labels != nullptr, "labels is null");
  REQUIRE(al16(img) && al16(fc_w) && al16(fc_b) && al16(out), "img / fc_w / fc_b / out must be 16-byte aligned device pointers");
  CHECK_HIP(tfc_launch_pack_labels(dt, img, labels, fc_w, fc_b, out, N, H * W, (hipStream_t)stream), "tfc_pack_nhwc8_labels");
  return 0;
}

extern "C" int tfc_label_plane_bwd(void* stream, const float* g, int gC, int ch, const float* labels, float* d_fc_w, float* d_fc_b, int N, int H, int W,
                                   int accumulate) {
  REQUIRE_IMAGE(N, H, W);
  REQUIRE(gC >= 1 && gC <= 8 && ch >= 0 && ch < gC, "channel %d of a %d-channel gradient", ch, gC);
  REQUIRE(labels != nullptr, "labels is null");
  REQUIRE(al16(g) && al16(d_fc_w) && al16(d_fc_b), "g / d_fc_w / d_fc_b must be 16-byte aligned device pointers");
  const long long HW = (long long)H * W;
  CHECK_HIP(tfc_launch_label_plane_bwd(g + (size_t)ch * HW, (long long)gC * HW, labels, d_fc_w, d_fc_b, N, (int)HW, accumulate ? 1 : 0, (hipStream_t)stream),
            "tfc_label_plane_bwd");
  return 0;
}

extern "C" int tfc_aux_heads_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, const float* const* w3, const float* const* b3,
                                 const int* nclass3_host, float* logits, float* part_ws) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype %d", dt);
  REQUIRE_IMAGE(N, H, W);
  REQUIRE(x_pitch == 8, "x pitch %d: the heads read the packed 8-channel discriminator input", x_pitch);
  int ct = 0;
  if (int rc = aux_classes(nclass3_host, &ct)) return rc;
  REQUIRE(w3 && b3 && logits && part_ws && al16(x), "null argument (x must be 16-byte aligned)");
  REQUIRE((long long)N * tfc_aux_fwd_nparts(H * W) * ct <= (long long)TFC_PART_WS_FLOATS, "N=%d x H*W=%d: the partial sums pass part_ws", N, H * W);
  TfcAuxRows rows = {};
  for (int h = 0, o = 0; h < 3; ++h) {
    REQUIRE(al16(w3[h]) && b3[h], "head %d: weight must be a 16-byte aligned device pointer, bias non-null", h);
    for (int r = 0; r < nclass3_host[h]; ++r, ++o) { rows.w[o] = w3[h] + (size_t)r * 6 * H * W; rows.b[o] = b3[h] + r; }
  }
  CHECK_HIP(tfc_launch_aux_heads_fwd(dt, x, rows, ct, logits, part_ws, N, H * W, (hipStream_t)stream), "tfc_aux_heads_fwd");
  return 0;
}

extern "C" int tfc_softmax_ce_heads(void* stream, const float* logits, const int* targets, const int* targets_host, const int* nclass3_host,
                                    const float* w3_host, float scale, int N, float* probs, float* losses4, float* dlogits) {
  REQUIRE(N > 0 && N <= (1 << 20), "bad N=%d", N);
  int ct = 0;
  if (int rc = aux_classes(nclass3_host, &ct)) return rc;
  REQUIRE(logits && targets && w3_host && probs && losses4, "null argument");
  TfcCeHeads a;
  for (int h = 0, off = 0; h < 3; ++h) { a.nc[h] = nclass3_host[h]; a.off[h] = off; a.w[h] = w3_host[h]; off += nclass3_host[h]; }
  a.scale = scale;
  if (targets_host)
    for (int n = 0; n < N; ++n)
      for (int h = 0; h < 3; ++h)
        REQUIRE(targets_host[n * 3 + h] >= 0 && targets_host[n * 3 + h] < a.nc[h], "target %d of sample %d, head %d: outside [0, %d)", targets_host[n * 3 + h], n, h, a.nc[h]);
  CHECK_HIP(tfc_launch_softmax_ce_heads(logits, targets, a, ct, N, probs, losses4, dlogits, (hipStream_t)stream), "tfc_softmax_ce_heads");
  return 0;
}

extern "C" int tfc_aux_heads_dgrad(void* stream, float* g, int gC, int N, int H, int W, const float* const* w3, const int* nclass3_host, const float* dlogits) {
  REQUIRE_IMAGE(N, H, W);
  REQUIRE(gC >= 3 && gC <= 8, "gradient of %d channels (3 .. 8: the first three are img_A's)", gC);
  int ct = 0;
  if (int rc = aux_classes(nclass3_host, &ct)) return rc;
  REQUIRE(w3 && dlogits && al16(g), "null argument (g must be 16-byte aligned)");
  TfcAuxRows rows = {};
  for (int h = 0, o = 0; h < 3; ++h) {
    REQUIRE(al16(w3[h]), "head %d: weight must be a 16-byte aligned device pointer", h);
    for (int r = 0; r < nclass3_host[h]; ++r, ++o) rows.w[o] = w3[h] + (size_t)r * 6 * H * W;
  }
  CHECK_HIP(tfc_launch_aux_heads_dgrad(g, (long long)gC * H * W, rows, ct, dlogits, N, H * W, (hipStream_t)stream), "tfc_aux_heads_dgrad");
  return 0;
}

extern "C" int tfc_aux_heads_wgrad(void* stream, int dt, const void* x_r, const float* dl_r, const void* x_f, const float* dl_f, int x_pitch, int N, int H,
                                   int W, float* const* dw3, float* const* db3, const int* nclass3_host, int accumulate) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype %d", dt);
  REQUIRE_IMAGE(N, H, W);
  REQUIRE(x_pitch == 8, "x pitch %d: the heads read the packed 8-channel discriminator input", x_pitch);
  int ct = 0;
  if (int rc = aux_classes(nclass3_host, &ct)) return rc;
  REQUIRE(al16(x_r) && dl_r && dw3 && db3, "null argument (x_r must be 16-byte aligned)");
  REQUIRE((x_f == nullptr) == (dl_f == nullptr) && (!x_f || al16(x_f)), "x_f and dl_f come together (x_f 16-byte aligned)");
  TfcAuxGradRows rows = {};
  for (int h = 0, o = 0; h < 3; ++h) {
    REQUIRE(al16(dw3[h]) && db3[h], "head %d: weight gradient must be a 16-byte aligned device pointer, bias gradient non-null", h);
    for (int r = 0; r < nclass3_host[h]; ++r, ++o) { rows.w[o] = dw3[h] + (size_t)r * 6 * H * W; rows.b[o] = db3[h] + r; }
  }
  CHECK_HIP(tfc_launch_aux_heads_wgrad(dt, x_r, dl_r, x_f, dl_f, rows, ct, N, H * W, accumulate ? 1 : 0, (hipStream_t)stream), "tfc_aux_heads_wgrad");
  return 0;
}

// ---- edge mask of the MASK-4 script (mask.hip) -------------------------------------------------------------------------------------------------

// both filters reflect once (padding 3 and 4): a side below 8 would need a second reflection for the blur of an 8 x 8 tile's halo
#define REQUIRE_MASK_IMAGE(N, H, W) do { \
    REQUIRE(N > 0 && N <= 65535 && H >= 8 && W >= 8 && H <= (1 << 20) && W <= (1 << 20), "bad dims N=%d H=%d W=%d (1 <= N <= 65535; H, W >= 8)", N, H, W); \
    REQUIRE((long long)N * H * W < (1LL << 31), "N*H*W=%lld must stay below 2^31", (long long)N * H * W); \
  } while (0)

extern "C" size_t tfc_mask_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H < 8 || W < 8) return 0;
  return (size_t)tfc_mask_stats_floats() * sizeof(float) + (size_t)tfc_mask_nblk(N, H, W) * 16;
}

extern "C" int tfc_mask_fwd(void* stream, const float* img, float* lap, float* bl, void* ws, int N, int H, int W) {
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(img) && al16(lap) && al16(bl) && al16(ws), "img / lap / bl / ws must be 16-byte aligned device pointers");
  CHECK_HIP(tfc_launch_mask_fwd(img, lap, bl, ws, N, H, W, (hipStream_t)stream), "tfc_mask_fwd");
  return 0;
}

extern "C" int tfc_mask_scale(void* stream, const float* bl, const void* ws, float* mask, int N, int H, int W) {
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(bl) && al16(ws) && al16(mask), "bl / ws / mask must be 16-byte aligned device pointers");
  CHECK_HIP(tfc_launch_mask_scale(bl, ws, mask, (long long)N * H * W, (hipStream_t)stream), "tfc_mask_scale");
  return 0;
}

extern "C" int tfc_mask_bwd(void* stream, const float* lap, const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf,
                            float* dmn, float* dimg, int N, int H, int W) {
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(lap) && al16(bl) && al16(ws), "lap / bl / ws must be 16-byte aligned device pointers");
  REQUIRE((dout != nullptr) != (ref != nullptr), "exactly one of dout (an upstream gradient) and ref (the L1 loss against it) is given");
  REQUIRE(al16(dout ? dout : ref), "dout / ref must be a 16-byte aligned device pointer");
  REQUIRE(!ref || al16(dout_buf), "with ref, dout_buf (N*H*W floats, 16-byte aligned) receives the loss's gradient w.r.t. the mask");
  REQUIRE(dimg == nullptr || (al16(dimg) && al16(dmn)), "dimg and dmn (N*H*W floats) must be 16-byte aligned device pointers");
  REQUIRE(dimg != nullptr || ref != nullptr, "without dimg only the L1 loss (ref) is left to compute");
  CHECK_HIP(tfc_launch_mask_bwd(lap, bl, ws, dout, ref, scale, dout_buf, dmn, dimg, N, H, W, (hipStream_t)stream), "tfc_mask_bwd");
  return 0;
}

// the phases of tfc_mask_fwd / tfc_mask_bwd; records are TFC_MASK_RECORD_BYTES each
static inline bool al8(const void* p) { return p != nullptr && (((uintptr_t)p) & 7) == 0; }
extern "C" int tfc_mask_fwd_lap(void* stream, const float* img, float* lap, void* ws, void* rec, int N, int H, int W) {
  REQUIRE(img && lap && ws && rec, "null argument");
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(img) && al16(lap) && al16(ws) && al8(rec), "img / lap / ws must be 16-byte aligned device pointers, rec 8-byte aligned");
  CHECK_HIP(tfc_launch_mask_phase_f1(img, lap, ws, rec, N, H, W, (hipStream_t)stream), "tfc_mask_fwd_lap");
  return 0;
}

extern "C" int tfc_mask_fwd_blur(void* stream, const float* lap, float* bl, void* ws, void* rec, int N, int H, int W) {
  REQUIRE(lap && bl && ws && rec, "null argument");
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(lap) && al16(bl) && al16(ws) && al8(rec), "lap / bl / ws must be 16-byte aligned device pointers, rec 8-byte aligned");
  CHECK_HIP(tfc_launch_mask_phase_f2(lap, bl, ws, rec, N, H, W, (hipStream_t)stream), "tfc_mask_fwd_blur");
  return 0;
}

extern "C" int tfc_mask_merge(void* stream, void* ws, const void* recs, int world, int which) {
  REQUIRE(ws && recs, "null argument");
  REQUIRE(world >= 1 && world <= 64, "world=%d (1 .. 64 records)", world);
  REQUIRE(which >= 0 && which <= 3, "which=%d (0: after F1, 1: after F2, 2: after B0, 3: after B1)", which);
  REQUIRE(al16(ws) && al8(recs), "ws must be a 16-byte aligned device pointer, recs 8-byte aligned");
  CHECK_HIP(tfc_launch_mask_merge(ws, recs, world, which, (hipStream_t)stream), "tfc_mask_merge");
  return 0;
}

extern "C" int tfc_mask_bwd_dot(void* stream, const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf, void* rec,
                                int N, int H, int W) {
  REQUIRE(bl && ws && rec, "null argument");
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(bl) && al16(ws) && al8(rec), "bl / ws must be 16-byte aligned device pointers, rec 8-byte aligned");
  REQUIRE((dout != nullptr) != (ref != nullptr), "exactly one of dout (an upstream gradient) and ref (the L1 loss against it) is given");
  REQUIRE(al16(dout ? dout : ref), "dout / ref must be a 16-byte aligned device pointer");
  REQUIRE(!ref || al16(dout_buf), "with ref, dout_buf (N*H*W floats, 16-byte aligned) receives the loss's gradient w.r.t. the mask");
  CHECK_HIP(tfc_launch_mask_phase_b0(bl, ws, dout, ref, scale, dout_buf, rec, N, H, W, (hipStream_t)stream), "tfc_mask_bwd_dot");
  return 0;
}

extern "C" int tfc_mask_bwd_blur(void* stream, const float* lap, const float* bl, void* ws, const float* dout, float* dmn, void* rec, int N, int H, int W) {
  REQUIRE(lap && bl && ws && dout && dmn && rec, "null argument");
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(lap) && al16(bl) && al16(ws) && al16(dout) && al16(dmn) && al8(rec),
          "lap / bl / ws / dout / dmn must be 16-byte aligned device pointers, rec 8-byte aligned");
  CHECK_HIP(tfc_launch_mask_phase_b1(lap, bl, ws, dout, dmn, rec, N, H, W, (hipStream_t)stream), "tfc_mask_bwd_blur");
  return 0;
}

extern "C" int tfc_mask_bwd_lap(void* stream, const float* lap, const void* ws, const float* dmn, float* dimg, int N, int H, int W) {
  REQUIRE(lap && ws && dmn && dimg, "null argument");
  REQUIRE_MASK_IMAGE(N, H, W);
  REQUIRE(al16(lap) && al16(ws) && al16(dmn) && al16(dimg), "lap / ws / dmn / dimg must be 16-byte aligned device pointers");
  CHECK_HIP(tfc_launch_mask_phase_b2(lap, ws, dmn, dimg, N, H, W, (hipStream_t)stream), "tfc_mask_bwd_lap");
  return 0;
}

extern "C" int tfc_pack_nhwc8_plane(void* stream, int dt, const float* img, const float* plane, const float* plane_div, void* out, int N, int H, int W) {
  REQUIRE(dt == TFC_DT_BF16 || dt == TFC_DT_F32 || dt == TFC_DT_BF16X3, "bad dtype %d", dt);
  REQUIRE_IMAGE(N, H, W);
  REQUIRE(al16(img) && al16(plane) && al16(out), "img / plane / out must be 16-byte aligned device pointers");
  CHECK_HIP(tfc_launch_pack_plane(dt, img, plane, plane_div, out, N, H * W, (hipStream_t)stream), "tfc_pack_nhwc8_plane");
  return 0;
}

extern "C" int tfc_probe_mfma(void* stream, float* out) {
  REQUIRE(out, "out is null");
  CHECK_HIP(tfc_launch_probe(out, (hipStream_t)stream), "tfc_probe_mfma");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// host emulator of the gather model (CPU tests only): consumes the SAME descriptors and the SAME packed operand
// stream layout as the kernels (fp32 units), so descriptor / packing / phase bugs show up without a GPU.
//   pass 0: x [N][H][W][pad8(Cin)]    -> y [N][OH][OW][pad8(Cout)]
//   pass 1: x = dy [N][OH][OW][pad8(Cout)] -> y = dx [N][H][W][pad8(Cin)]
//   pass 2: x [N][H][W][pad8(Cin)], w_host = dy [N][OH][OW][pad8(Cout)] -> y = dw (torch layout)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int tfc_host_emulate_conv(int op, int pass, int es, const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout) {
  REQUIRE(pass >= 0 && pass <= 2 && op >= 0 && op <= 6 && (es == 2 || es == 4), "bad op/pass/es");
  REQUIRE(op != TFC_OP_CONV2 || (H % 2 == 0 && W % 2 == 0), "TFC_OP_CONV2 needs an even H and W");
  REQUIRE(op != TFC_OP_CONV3R || (H >= 2 && W >= 2), "TFC_OP_CONV3R (reflection padding 1) needs H >= 2 and W >= 2 (H=%d W=%d)", H, W);
  const int UE = 16 / es;                                        // elements per 16-byte unit in the emulated geometry
  const int OH = out_hw(op, H), OW = out_hw(op, W);
  const int inC = pass == 1 ? pad8(Cout) : pad8(Cin);
  const int outC = pass == 1 ? pad8(Cin) : pad8(Cout);
  // TFC_OP_CONV3R, pass 1: the gather fills the padded gradient E [N][H + 2][W + 2], which is folded into dx below (as tfc_conv_dgrad does)
  std::vector<float> ering;
  float* const dx_folded = y;
  if (op == TFC_OP_CONV3R && pass == 1) { ering.assign((size_t)N * (H + 2) * (W + 2) * outC, 0.f); y = ering.data(); }
  if (pass == 2) {
    std::vector<double> acc((size_t)16 * Cout * Cin, 0.0);
    WeightMap wm{};
    for (int ph = 0; ph < num_phases(op, 2); ++ph) {
      TfcGather d;
      if (int e = build_desc(op, 2, ph, N, H, W, Cin, Cout, inC, outC, &d, &wm)) return e;
      const TfcPlane& p = d.plane[0];
      for (int img = 0; img < N; ++img)
        for (int a = 0; a < d.GH; ++a)
          for (int b = 0; b < d.GW; ++b) {
            const int oy = a * d.OS + d.OOY, ox = b * d.OS + d.OOX;
            const float* dyp = w + ((size_t)(img * d.OH + oy) * d.OW + ox) * outC;
            const int ta = a % TFC_TILE_H, tb = b % TFC_TILE_W, a0 = a - ta, b0 = b - tb;
            for (int t = 0; t < p.ntaps; ++t) {
              int sy = (a0 + p.dy0 + ta + p.tap_dy[t]) * d.SS + p.py, sx = (b0 + p.dx0 + tb + p.tap_dx[t]) * d.SS + p.px;
              if (d.reflect) { sy = tfc_reflect1(sy, d.IH); sx = tfc_reflect1(sx, d.IW); }
              if (sy < 0 || sy >= d.IH || sx < 0 || sx >= d.IW) continue;
              const float* xp = x + ((size_t)(img * d.IH + sy) * d.IW + sx) * inC;
              for (int n = 0; n < Cout; ++n)
                for (int c = 0; c < Cin; ++c)
                  for (int m = p.tap_mask[t]; m; m &= m - 1)
                    acc[((size_t)__builtin_ctz(m) * Cout + n) * Cin + c] += (double)dyp[n] * xp[c];
            }
          }
    }
    for (int n = 0; n < Cout; ++n)
      for (int c = 0; c < Cin; ++c)
        for (int s = 0; s < 16; ++s) y[(long long)n * wm.sn + (long long)c * wm.sc + s] = (float)acc[((size_t)s * Cout + n) * Cin + c];
    return 0;
  }
  for (int ph = 0; ph < num_phases(op, pass); ++ph) {
    TfcGather d;
    WeightMap wm;
    if (int e = build_desc(op, pass, ph, N, H, W, Cin, Cout, inC, outC, &d, &wm)) return e;
    // pack on the host with the kernel's index math
    const int NB32 = tfc_nb32_padded(d.Nout);
    const int total_sub = tfc_total_substeps(d, es);
    const int total_units = total_sub * NB32 * 64;
    std::vector<float> wp((size_t)total_units * UE);
    for (int idx = 0; idx < total_units; ++idx) {
      int n, mask, c0;
      tfc_pack_locate(d, es, NB32, idx, &n, &mask, &c0);
      for (int e = 0; e < UE; ++e) {
        const int c = c0 + e;
        float a = 0.f;
        if (n < wm.Nreal && c < wm.Creal)
          for (int m = mask; m; m &= m - 1) a += w[(long long)n * wm.sn + (long long)c * wm.sc + __builtin_ctz(m)];
        wp[(size_t)idx * UE + e] = a;
      }
    }
    const int PB = tfc_pb(d.Cin_pad, es), UPP = PB >> 4, CK = PB / es;
    const int nchunks = d.Cin_pad * es / PB;
    for (int img = 0; img < N; ++img)
      for (int tyb = 0; tyb < d.tiles_y; ++tyb)
        for (int txb = 0; txb < d.tiles_x; ++txb) {
          const int a0 = tyb * TFC_TILE_H, b0 = txb * TFC_TILE_W;
          for (int ty = 0; ty < TFC_TILE_H; ++ty)
            for (int tx = 0; tx < TFC_TILE_W; ++tx) {
              const int a = a0 + ty, b = b0 + tx;
              if (a >= d.GH || b >= d.GW) continue;
              const int oy = a * d.OS + d.OOY, ox = b * d.OS + d.OOX;
              for (int n = 0; n < d.Nout; ++n) {
                const int nb = n >> 5, rn = n & 31;
                double acc = 0.0;
                int gs = 0;
                for (int cc = 0; cc < nchunks; ++cc)
                  for (int pl = 0; pl < d.nplanes; ++pl) {
                    const TfcPlane& p = d.plane[pl];
                    const int nsub = tfc_nsub(p.ntaps, PB);
                    for (int s = 0; s < nsub; ++s, ++gs)
                      for (int h = 0; h < 2; ++h) {
                        const int u = 2 * s + h, tap = u / UPP, g = u % UPP;
                        int sy = (a0 + p.dy0 + ty + p.tap_dy[tap]) * d.SS + p.py;
                        int sx = (b0 + p.dx0 + tx + p.tap_dx[tap]) * d.SS + p.px;
                        if (d.reflect) { sy = tfc_reflect1(sy, d.IH); sx = tfc_reflect1(sx, d.IW); }
                        if (sy < 0 || sy >= d.IH || sx < 0 || sx >= d.IW) continue;
                        const float* xp = x + ((size_t)(img * d.IH + sy) * d.IW + sx) * inC + cc * CK + g * UE;
                        const float* wq = &wp[((size_t)(gs * NB32 + nb) * 64 + (h * 32 + rn)) * UE];
                        for (int e = 0; e < UE; ++e) acc += (double)xp[e] * wq[e];
                      }
                  }
                y[((size_t)(img * d.OH + oy) * d.OW + ox) * outC + n] = (float)acc;
              }
            }
        }
  }
  if (!ering.empty())                                            // dx[i][j] = sum of the padded positions that reflect onto (i, j): the adjoint of the padding
    for (int img = 0; img < N; ++img)
      for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j)
          for (int c = 0; c < outC; ++c) {
            double acc = 0.0;
            for (int ey = 0; ey < H + 2; ++ey)
              for (int ex = 0; ex < W + 2; ++ex)
                if (tfc_reflect1(ey - 1, H) == i && tfc_reflect1(ex - 1, W) == j) acc += ering[((size_t)(img * (H + 2) + ey) * (W + 2) + ex) * outC + c];
            dx_folded[((size_t)(img * H + i) * W + j) * outC + c] = (float)acc;
          }
  return 0;
}
