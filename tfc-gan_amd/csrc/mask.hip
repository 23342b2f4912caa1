// The edge mask of the MASK-4 script (reference TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_experiment.py "4X" :385-390), forward and exact backward:
//   g    = 0.299 R + 0.587 G + 0.114 B
//   lap  = (S49(g) - 49 g) / 96          S49: 7x7 box sum, reflect padding 3 (kornia's normalised Laplacian: ones, centre 1 - 49, / sum |k|)
//   L    = |lap|;  mn, mx = min, max of L over the WHOLE batch tensor;  Mn = (L - mn) / (mx - mn)
//   Bl   = gauss9(Mn)                    separable 9 taps, sigma 1.6, reflect padding 4
//   mask = Bl / M,  M = max(Bl) over the batch
// A constant image (mx == mn) gives NaN, as in the reference; nothing guards it.
// Structure: a 16 x 64 tile plus halo is staged in LDS (reflect indexing at the load for the forward filters, zero extension for their adjoints), a
// horizontal pass writes a second LDS tile, the vertical pass produces four consecutive columns per thread (16-byte stores where W % 4 == 0).
// Extrema go to one fixed slot per workgroup as (value bits, tie count) and a one-workgroup finaliser combines them: min / max and integer counts
// do not depend on the order. The backward's global sums leave every workgroup as a pair of doubles in its slot and are added by one workgroup in
// a fixed order. No atomics, no host synchronisation: extrema, tie counts and sums stay in the `stats` floats at the head of the workspace.
// The adjoint of a reflect-padded filter is NOT the filter: x'[j] = sum_d w[d] (y0[j-d] + [j >= 1] y0[-j-d] + [j <= n-2] y0[2n-2-j-d]) with y0 the
// zero extension of y -- the two extra terms fold the contributions of the padding back onto the border pixels they were copied from.
#include "common.h"

#define MK_TH 16
#define MK_TW 64
struct TfcMaskTaps { float w[9]; };
// floats at the head of the workspace
enum { MS_MN = 0, MS_MX, MS_CMN, MS_CMX, MS_M, MS_CM, MS_DM, MS_LOSS, MS_DMX, MS_DMN, MS_FLOATS = 16 };

__device__ __forceinline__ int mk_reflect(int i, int n) {        // one reflection (no edge repeat), clamped: a ragged tile's overhang stays in bounds
  i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return min(max(i, 0), n - 1);
}

// ---- the tile: a[(16+2P) x (64+2P)] staged by `stage(row, col)`, b[(16+2P) x 64] after the horizontal pass, out[4] after the vertical one
template <int P, bool BOX, bool ADJ, class Stage>
__device__ __forceinline__ void mask_tile(Stage stage, const TfcMaskTaps& taps, float* a, float* b, int H, int W, int x0, int y0, float* out) {
  constexpr int AR = MK_TH + 2 * P, AC = MK_TW + 2 * P;
  const int t = threadIdx.x;
  for (int idx = t; idx < AR * AC; idx += 256) {
    const int i = idx / AC, j = idx - i * AC;
    const int y = y0 - P + i, x = x0 - P + j;
    float v;
    if (ADJ) v = (y >= 0 && y < H && x >= 0 && x < W) ? stage(y, x) : 0.f;
    else v = stage(mk_reflect(y, H), mk_reflect(x, W));
    a[idx] = v;
  }
  __syncthreads();
  for (int idx = t; idx < AR * MK_TW; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    const float* ar = a + i * AC;
    float s = 0.f;
#pragma unroll
    for (int d = -P; d <= P; ++d) s += BOX ? ar[j + P + d] : taps.w[d + P] * ar[j + P + d];
    if (ADJ) {
      const int x = x0 + j;
      if (x >= 1 && x <= P) {                                     // left fold: padding column -x was a copy of column x
#pragma unroll
        for (int d = -P; d <= P; ++d) {
          const int cc = -x - d, k = cc - x0 + P;
          if (cc >= 0 && cc < W && k >= 0 && k < AC) s += BOX ? ar[k] : taps.w[d + P] * ar[k];
        }
      }
      if (x <= W - 2 && x >= W - 1 - P) {                         // right fold: padding column 2W-2-x
#pragma unroll
        for (int d = -P; d <= P; ++d) {
          const int cc = 2 * W - 2 - x - d, k = cc - x0 + P;
          if (cc >= 0 && cc < W && k >= 0 && k < AC) s += BOX ? ar[k] : taps.w[d + P] * ar[k];
        }
      }
    }
    b[idx] = s;
  }
  __syncthreads();
  const int cu = t & 15, i = t >> 4, y = y0 + i;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int d = -P; d <= P; ++d) {
    const float4 v = *reinterpret_cast<const float4*>(b + (i + P + d) * MK_TW + 4 * cu);
    const float wd = BOX ? 1.f : taps.w[d + P];
    s[0] += wd * v.x; s[1] += wd * v.y; s[2] += wd * v.z; s[3] += wd * v.w;
  }
  if (ADJ) {
    if (y >= 1 && y <= P) {
#pragma unroll
      for (int d = -P; d <= P; ++d) {
        const int rr = -y - d, k = rr - y0 + P;
        if (rr >= 0 && rr < H && k >= 0 && k < AR) {
          const float4 v = *reinterpret_cast<const float4*>(b + k * MK_TW + 4 * cu);
          const float wd = BOX ? 1.f : taps.w[d + P];
          s[0] += wd * v.x; s[1] += wd * v.y; s[2] += wd * v.z; s[3] += wd * v.w;
        }
      }
    }
    if (y <= H - 2 && y >= H - 1 - P) {
#pragma unroll
      for (int d = -P; d <= P; ++d) {
        const int rr = 2 * H - 2 - y - d, k = rr - y0 + P;
        if (rr >= 0 && rr < H && k >= 0 && k < AR) {
          const float4 v = *reinterpret_cast<const float4*>(b + k * MK_TW + 4 * cu);
          const float wd = BOX ? 1.f : taps.w[d + P];
          s[0] += wd * v.x; s[1] += wd * v.y; s[2] += wd * v.z; s[3] += wd * v.w;
        }
      }
    }
  }
  out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = s[3];
}

__device__ __forceinline__ void mk_store4(float* p, const float* v, int x, int W) {   // p: address of column x of a row; x % 4 == 0
  if ((W & 3) == 0) {
    if (x < W) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (x + c < W) p[c] = v[c];
  }
}

__device__ __forceinline__ int mk_block_id() { return (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// (value, tie count) pairs of 256 threads -> thread 0. MAXI: keep the larger value; equal values add their counts.
template <bool MAXI, typename C>
__device__ __forceinline__ void mk_extremum(float& v, C& c, float* lv, C* lc) {
  const int t = threadIdx.x;
  lv[t] = v; lc[t] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      const float v2 = lv[t + o];
      const C c2 = lc[t + o];
      if (v2 == lv[t]) lc[t] += c2;
      else if (MAXI ? v2 > lv[t] : v2 < lv[t]) { lv[t] = v2; lc[t] = c2; }
    }
    __syncthreads();
  }
  v = lv[0]; c = lc[0];
  __syncthreads();
}

// two doubles of 256 threads -> thread 0, a fixed tree
__device__ __forceinline__ void mk_sum2(double& s0, double& s1, double* l0, double* l1) {
  const int t = threadIdx.x;
  l0[t] = s0; l1[t] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { l0[t] += l0[t + o]; l1[t] += l1[t + o]; }
    __syncthreads();
  }
  s0 = l0[0]; s1 = l1[0];
  __syncthreads();
}

// ---- forward (a): signed lap + per-workgroup (min, ties, max, ties) of |lap|
__global__ void __launch_bounds__(256)
tfc_mask_lap_kernel(const float* __restrict__ img, float* __restrict__ lap, uint4* __restrict__ part, int H, int W) {
  constexpr int P = 3;
  __shared__ __align__(16) float a[(MK_TH + 2 * P) * (MK_TW + 2 * P)];
  __shared__ __align__(16) float b[(MK_TH + 2 * P) * MK_TW];
  __shared__ float lv[256];
  __shared__ unsigned lc[256];
  const int n = blockIdx.z, x0 = blockIdx.x * MK_TW, y0 = blockIdx.y * MK_TH;
  const size_t HW = (size_t)H * W;
  const float* im = img + (size_t)n * 3 * HW;
  TfcMaskTaps none;
  float s[4];
  mask_tile<P, true, false>([&](int y, int x) {
    const float* p = im + (size_t)y * W + x;
    return 0.299f * p[0] + 0.587f * p[HW] + 0.114f * p[2 * HW];
  }, none, a, b, H, W, x0, y0, s);
  const int cu = threadIdx.x & 15, i = threadIdx.x >> 4, y = y0 + i, x = x0 + 4 * cu;
  float mn = __builtin_inff(), mx = -1.f;
  unsigned cmn = 0, cmx = 0;
  float v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float g = a[(i + P) * (MK_TW + 2 * P) + 4 * cu + c + P];
    v[c] = (s[c] - 49.f * g) * (1.f / 96.f);
    if (y < H && x + c < W) {
      const float L = fabsf(v[c]);
      if (L == mn) ++cmn; else if (L < mn) { mn = L; cmn = 1; }
      if (L == mx) ++cmx; else if (L > mx) { mx = L; cmx = 1; }
    }
  }
  if (y < H) mk_store4(lap + ((size_t)n * H + y) * W + x, v, x, W);
  mk_extremum<false>(mn, cmn, lv, lc);
  mk_extremum<true>(mx, cmx, lv, lc);
  if (threadIdx.x == 0) part[mk_block_id()] = make_uint4(__float_as_uint(mn), cmn, __float_as_uint(mx), cmx);
}

// ---- one workgroup: the partials -> stats. which 0: (mn, mx, ties) of |lap|; which 1: (M, ties) of Bl
__global__ void __launch_bounds__(256)
tfc_mask_final_extrema_kernel(const uint4* __restrict__ part, int nblk, float* __restrict__ stats, int which) {
  __shared__ float lv[256];
  __shared__ unsigned long long lc[256];
  float mn = __builtin_inff(), mx = -1.f;
  unsigned long long cmn = 0, cmx = 0;
  for (int k = threadIdx.x; k < nblk; k += 256) {
    const uint4 p = part[k];
    const float a = __uint_as_float(p.x), c = __uint_as_float(p.z);
    if (a == mn) cmn += p.y; else if (a < mn) { mn = a; cmn = p.y; }
    if (c == mx) cmx += p.w; else if (c > mx) { mx = c; cmx = p.w; }
  }
  mk_extremum<false>(mn, cmn, lv, lc);
  mk_extremum<true>(mx, cmx, lv, lc);
  if (threadIdx.x == 0) {
    if (which == 0) { stats[MS_MN] = mn; stats[MS_MX] = mx; stats[MS_CMN] = (float)cmn; stats[MS_CMX] = (float)cmx; }
    else { stats[MS_M] = mx; stats[MS_CM] = (float)cmx; }
  }
}

// ---- forward (b): Bl = gauss9((|lap| - mn) / (mx - mn)) + per-workgroup (max, ties)
__global__ void __launch_bounds__(256)
tfc_mask_blur_kernel(const float* __restrict__ lap, float* __restrict__ bl, uint4* __restrict__ part, const float* __restrict__ stats, TfcMaskTaps taps,
                     int H, int W) {
  constexpr int P = 4;
  __shared__ __align__(16) float a[(MK_TH + 2 * P) * (MK_TW + 2 * P)];
  __shared__ __align__(16) float b[(MK_TH + 2 * P) * MK_TW];
  __shared__ float lv[256];
  __shared__ unsigned lc[256];
  const int n = blockIdx.z, x0 = blockIdx.x * MK_TW, y0 = blockIdx.y * MK_TH;
  const float* lp = lap + (size_t)n * H * W;
  const float mn = stats[MS_MN], D = stats[MS_MX] - mn;
  float s[4];
  mask_tile<P, false, false>([&](int y, int x) { return (fabsf(lp[(size_t)y * W + x]) - mn) / D; }, taps, a, b, H, W, x0, y0, s);
  const int cu = threadIdx.x & 15, i = threadIdx.x >> 4, y = y0 + i, x = x0 + 4 * cu;
  float mx = -__builtin_inff();
  unsigned cmx = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (y < H && x + c < W) {
      if (s[c] == mx) ++cmx; else if (s[c] > mx) { mx = s[c]; cmx = 1; }
    }
  if (y < H) mk_store4(bl + ((size_t)n * H + y) * W + x, s, x, W);
  mk_extremum<true>(mx, cmx, lv, lc);
  if (threadIdx.x == 0) part[mk_block_id()] = make_uint4(0x7f800000u, 0u, __float_as_uint(mx), cmx);
}

// ---- mask = Bl / M
__global__ void __launch_bounds__(256)
tfc_mask_scale_kernel(const float* __restrict__ bl, const float* __restrict__ stats, float* __restrict__ mask, long long total) {
  const long long q = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
  if (q >= total) return;
  const float M = stats[MS_M];
  if (q + 3 < total) {
    const float4 v = *reinterpret_cast<const float4*>(bl + q);
    *reinterpret_cast<float4*>(mask + q) = make_float4(v.x / M, v.y / M, v.z / M, v.w / M);
  } else {
    for (long long k = q; k < total; ++k) mask[k] = bl[k] / M;
  }
}

// ---- backward phase 0: per-workgroup (sum |Bl/M - ref|, sum dout Bl). With `ref` the upstream gradient of the L1 loss is formed here
// (dout = gs * sign(Bl/M - ref), written to dout_w); without it dout is read.
__global__ void __launch_bounds__(256)
tfc_mask_dot_kernel(const float* __restrict__ bl, const float* __restrict__ stats, const float* __restrict__ dout, const float* __restrict__ ref,
                    float gs, float* __restrict__ dout_w, double* __restrict__ part, long long total) {
  __shared__ double l0[256], l1[256];
  const long long q = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
  const float M = stats[MS_M];
  double sl = 0.0, sd = 0.0;
  if (q < total) {
    const bool full = q + 3 < total;
    const float* u = ref ? ref : dout;                            // the second operand: the L1 loss's reference, or the upstream gradient itself
    float vb[4], vu[4], vd[4];
    if (full) {
      const float4 t = *reinterpret_cast<const float4*>(bl + q); vb[0] = t.x; vb[1] = t.y; vb[2] = t.z; vb[3] = t.w;
      const float4 w = *reinterpret_cast<const float4*>(u + q); vu[0] = w.x; vu[1] = w.y; vu[2] = w.z; vu[3] = w.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool ok = q + c < total;
        vb[c] = ok ? bl[q + c] : 0.f;
        vu[c] = ok ? u[q + c] : 0.f;
      }
    }
    float fl = 0.f, fd = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool ok = full || q + c < total;
      float d = vu[c];
      if (ref) {
        const float diff = vb[c] / M - vu[c];
        fl += ok ? fabsf(diff) : 0.f;
        d = !ok ? 0.f : (diff > 0.f ? gs : (diff < 0.f ? -gs : 0.f));
      }
      vd[c] = d;
      fd = fmaf(d, vb[c], fd);
    }
    if (ref) {
      if (full) *reinterpret_cast<float4*>(dout_w + q) = make_float4(vd[0], vd[1], vd[2], vd[3]);
      else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (q + c < total) dout_w[q + c] = vd[c];
      }
    }
    sl = fl; sd = fd;
  }
  mk_sum2(sl, sd, l0, l1);
  if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = sl; part[2 * (size_t)blockIdx.x + 1] = sd; }
}

// ---- one workgroup: pairs of doubles -> stats, fixed order. which 0: (loss, d/dM per tie) from (sum |diff|, sum dout Bl);
// which 1: (d/dmx, d/dmn per tie) from (sum dMn (L - mn), sum dMn (L - mx))
__global__ void __launch_bounds__(256)
tfc_mask_final_sums_kernel(const double* __restrict__ part, int nblk, float* __restrict__ stats, int which, float loss_scale) {
  __shared__ double l0[256], l1[256];
  double s0 = 0.0, s1 = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) { s0 += part[2 * (size_t)k]; s1 += part[2 * (size_t)k + 1]; }
  mk_sum2(s0, s1, l0, l1);
  if (threadIdx.x == 0) {
    if (which == 0) {
      const double M = stats[MS_M];
      stats[MS_LOSS] = (float)(s0 * (double)loss_scale);
      stats[MS_DM] = (float)(-(s1 / (M * M)) / (double)stats[MS_CM]);
    } else {
      const double D = (double)stats[MS_MX] - (double)stats[MS_MN];
      stats[MS_DMX] = (float)(-(s0 / (D * D)) / (double)stats[MS_CMX]);
      stats[MS_DMN] = (float)((s1 / (D * D)) / (double)stats[MS_CMN]);
    }
  }
}

// ---- backward phase 1: dMn = gauss9^T(dout / M + [Bl == M] dM) + per-workgroup (sum dMn (L - mn), sum dMn (L - mx))
__global__ void __launch_bounds__(256)
tfc_mask_blur_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ bl, const float* __restrict__ lap, float* __restrict__ dmn,
                         double* __restrict__ part, const float* __restrict__ stats, TfcMaskTaps taps, int H, int W) {
  constexpr int P = 4;
  __shared__ __align__(16) float a[(MK_TH + 2 * P) * (MK_TW + 2 * P)];
  __shared__ __align__(16) float b[(MK_TH + 2 * P) * MK_TW];
  __shared__ double l0[256], l1[256];
  const int n = blockIdx.z, x0 = blockIdx.x * MK_TW, y0 = blockIdx.y * MK_TH;
  const size_t base = (size_t)n * H * W;
  const float M = stats[MS_M], dM = stats[MS_DM], mn = stats[MS_MN], mx = stats[MS_MX];
  float s[4];
  mask_tile<P, false, true>([&](int y, int x) {
    const size_t k = base + (size_t)y * W + x;
    return dout[k] / M + (bl[k] == M ? dM : 0.f);
  }, taps, a, b, H, W, x0, y0, s);
  const int cu = threadIdx.x & 15, i = threadIdx.x >> 4, y = y0 + i, x = x0 + 4 * cu;
  float fa = 0.f, fb = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (y < H && x + c < W) {
      const float L = fabsf(lap[base + (size_t)y * W + x + c]);
      fa = fmaf(s[c], L - mn, fa);
      fb = fmaf(s[c], L - mx, fb);
    }
  if (y < H) mk_store4(dmn + base + (size_t)y * W + x, s, x, W);
  double sa = fa, sb = fb;
  mk_sum2(sa, sb, l0, l1);
  if (threadIdx.x == 0) { part[2 * (size_t)mk_block_id()] = sa; part[2 * (size_t)mk_block_id() + 1] = sb; }
}

// ---- backward phase 2: dlap = sign(lap) (dMn / (mx - mn) + [L == mx] dmx + [L == mn] dmn); dg = (S49^T(dlap) - 49 dlap) / 96; dimg = coef dg
__global__ void __launch_bounds__(256)
tfc_mask_lap_bwd_kernel(const float* __restrict__ dmn, const float* __restrict__ lap, float* __restrict__ dimg, const float* __restrict__ stats, int H, int W) {
  constexpr int P = 3;
  __shared__ __align__(16) float a[(MK_TH + 2 * P) * (MK_TW + 2 * P)];
  __shared__ __align__(16) float b[(MK_TH + 2 * P) * MK_TW];
  const int n = blockIdx.z, x0 = blockIdx.x * MK_TW, y0 = blockIdx.y * MK_TH;
  const size_t HW = (size_t)H * W, base = (size_t)n * HW;
  const float mn = stats[MS_MN], mx = stats[MS_MX], D = mx - mn, dmx = stats[MS_DMX], dmn_e = stats[MS_DMN];
  TfcMaskTaps none;
  float s[4];
  mask_tile<P, true, true>([&](int y, int x) {
    const size_t k = base + (size_t)y * W + x;
    const float l = lap[k], L = fabsf(l);
    const float dL = dmn[k] / D + (L == mx ? dmx : 0.f) + (L == mn ? dmn_e : 0.f);
    return l > 0.f ? dL : (l < 0.f ? -dL : 0.f);
  }, none, a, b, H, W, x0, y0, s);
  const int cu = threadIdx.x & 15, i = threadIdx.x >> 4, y = y0 + i, x = x0 + 4 * cu;
  if (y >= H) return;
  float dg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dg[c] = (s[c] - 49.f * a[(i + P) * (MK_TW + 2 * P) + 4 * cu + c + P]) * (1.f / 96.f);
  const float coef[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float v[4] = {coef[ch] * dg[0], coef[ch] * dg[1], coef[ch] * dg[2], coef[ch] * dg[3]};
    mk_store4(dimg + ((size_t)n * 3 + ch) * HW + (size_t)y * W + x, v, x, W);
  }
}

// ---- the same work in phases, for a batch that is spread over `world` ranks -------------------------------------------------------
// Between two phases every rank leaves a RECORD of four 64-bit words, the caller gathers the records of all ranks in rank order, and a one-workgroup
// merge kernel turns them into the stats floats the next phase reads -- the same floats on every rank, because every rank merges the same records
// in the same order. Extrema travel as (fp32 bits, 64-bit tie count) and merge by the rule of tfc_mask_final_extrema_kernel (the smaller / larger
// value wins with its count, equal values add their counts); sums travel as doubles and are added in rank order. With one record the stats floats
// are the ones the unsplit finalisers write, bit for bit.
//   after F1: {bits(mn), ties(mn), bits(mx), ties(mx)}     after F2: {bits(M), ties(M), 0, 0}
//   after B0: {sum |mask - ref|, sum dout Bl, 0, 0}        after B1: {sum dMn (L - mn), sum dMn (L - mx), 0, 0}     (doubles)
#define MK_REC_WORDS 4

// one workgroup: the extrema partials of this rank -> its record (which 0: after F1, which 1: after F2). The reduction of tfc_mask_final_extrema_kernel.
__global__ void __launch_bounds__(256)
tfc_mask_record_extrema_kernel(const uint4* __restrict__ part, int nblk, unsigned long long* __restrict__ rec, int which) {
  __shared__ float lv[256];
  __shared__ unsigned long long lc[256];
  float mn = __builtin_inff(), mx = -1.f;
  unsigned long long cmn = 0, cmx = 0;
  for (int k = threadIdx.x; k < nblk; k += 256) {
    const uint4 p = part[k];
    const float a = __uint_as_float(p.x), c = __uint_as_float(p.z);
    if (a == mn) cmn += p.y; else if (a < mn) { mn = a; cmn = p.y; }
    if (c == mx) cmx += p.w; else if (c > mx) { mx = c; cmx = p.w; }
  }
  mk_extremum<false>(mn, cmn, lv, lc);
  mk_extremum<true>(mx, cmx, lv, lc);
  if (threadIdx.x == 0) {
    if (which == 0) { rec[0] = __float_as_uint(mn); rec[1] = cmn; rec[2] = __float_as_uint(mx); rec[3] = cmx; }
    else { rec[0] = __float_as_uint(mx); rec[1] = cmx; rec[2] = 0ull; rec[3] = 0ull; }
  }
}

// one workgroup: the pairs of doubles of this rank -> its record, the fixed order of tfc_mask_final_sums_kernel. With loss_out (after B0) this rank's
// own L1 loss, scale * mean over ITS samples of |mask - ref| (masks normalised by the merged extrema), goes to the stats.
__global__ void __launch_bounds__(256)
tfc_mask_record_sums_kernel(const double* __restrict__ part, int nblk, double* __restrict__ rec, float* __restrict__ loss_out, float loss_scale) {
  __shared__ double l0[256], l1[256];
  double s0 = 0.0, s1 = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) { s0 += part[2 * (size_t)k]; s1 += part[2 * (size_t)k + 1]; }
  mk_sum2(s0, s1, l0, l1);
  if (threadIdx.x == 0) {
    rec[0] = s0; rec[1] = s1; rec[2] = 0.0; rec[3] = 0.0;
    if (loss_out) loss_out[0] = (float)(s0 * (double)loss_scale);
  }
}

// one workgroup, one lane: the records of `world` ranks (rank order) -> stats. which 0: (mn, mx, ties) of |lap|; 1: (M, ties) of Bl;
// 2: d/dM per tie from the sum of dout Bl over all ranks; 3: (d/dmx, d/dmn per tie) from the two sums of B1 over all ranks.
__global__ void __launch_bounds__(64)
tfc_mask_merge_kernel(const unsigned long long* __restrict__ recs, int world, float* __restrict__ stats, int which) {
  if (threadIdx.x != 0) return;
  if (which <= 1) {
    float mn = __builtin_inff(), mx = -1.f;
    unsigned long long cmn = 0, cmx = 0;
    for (int r = 0; r < world; ++r) {
      const unsigned long long* p = recs + (size_t)r * MK_REC_WORDS;
      if (which == 0) {
        const float a = __uint_as_float((unsigned)p[0]);
        if (a == mn) cmn += p[1]; else if (a < mn) { mn = a; cmn = p[1]; }
      }
      const float c = __uint_as_float((unsigned)p[which == 0 ? 2 : 0]);
      const unsigned long long cc = p[which == 0 ? 3 : 1];
      if (c == mx) cmx += cc; else if (c > mx) { mx = c; cmx = cc; }
    }
    if (which == 0) { stats[MS_MN] = mn; stats[MS_MX] = mx; stats[MS_CMN] = (float)cmn; stats[MS_CMX] = (float)cmx; }
    else { stats[MS_M] = mx; stats[MS_CM] = (float)cmx; }
  } else {
    const double* d = reinterpret_cast<const double*>(recs);
    double s0 = d[0], s1 = d[1];                                  // starts from rank 0's doubles, not from +0.0: one record passes through unchanged
    for (int r = 1; r < world; ++r) { s0 += d[(size_t)r * MK_REC_WORDS]; s1 += d[(size_t)r * MK_REC_WORDS + 1]; }
    if (which == 2) {
      const double M = stats[MS_M];
      stats[MS_DM] = (float)(-(s1 / (M * M)) / (double)stats[MS_CM]);
    } else {
      const double D = (double)stats[MS_MX] - (double)stats[MS_MN];
      stats[MS_DMX] = (float)(-(s0 / (D * D)) / (double)stats[MS_CMX]);
      stats[MS_DMN] = (float)((s1 / (D * D)) / (double)stats[MS_CMN]);
    }
  }
}

// ---- torch.cat((img, plane), 1) -> NHWC8 of the compute dtype: channels 0..2 img, 3 the plane (divided by *Mdev when given: Bl -> mask), 4..7 zero
template <typename T>
__global__ void __launch_bounds__(256)
tfc_pack_plane_kernel(const float* __restrict__ img, const float* __restrict__ plane, const float* __restrict__ Mdev, T* __restrict__ out, int HW) {
  const int q = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (4 * (long long)q >= HW) return;
  float c[4][4];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float4 t = *reinterpret_cast<const float4*>(img + ((size_t)n * 3 + ch) * HW + (size_t)4 * q);
    c[ch][0] = t.x; c[ch][1] = t.y; c[ch][2] = t.z; c[ch][3] = t.w;
  }
  {
    const float4 t = *reinterpret_cast<const float4*>(plane + (size_t)n * HW + (size_t)4 * q);
    c[3][0] = t.x; c[3][1] = t.y; c[3][2] = t.z; c[3][3] = t.w;
    if (Mdev) { const float M = Mdev[0]; c[3][0] /= M; c[3][1] /= M; c[3][2] /= M; c[3][3] /= M; }
  }
  T* o = out + ((size_t)n * HW + (size_t)4 * q) * 8;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v[8] = {c[0][j], c[1][j], c[2][j], c[3][j], 0.f, 0.f, 0.f, 0.f};
    if (sizeof(T) == 2) {
      *reinterpret_cast<uint4*>(o + 8 * j) = pack16<bf16_t>(v);
    } else {
      *reinterpret_cast<uint4*>(o + 8 * j) = pack16<float>(v);
      *reinterpret_cast<uint4*>(o + 8 * j + 4) = pack16<float>(v + 4);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
static TfcMaskTaps gauss_taps() {
  TfcMaskTaps t;
  double w[9], s = 0.0;
  for (int k = 0; k < 9; ++k) { const double x = k - 4; w[k] = exp(-x * x / (2.0 * 1.6 * 1.6)); s += w[k]; }
  for (int k = 0; k < 9; ++k) t.w[k] = (float)(w[k] / s);
  return t;
}
static dim3 tile_grid(int N, int H, int W) { return dim3((unsigned)((W + MK_TW - 1) / MK_TW), (unsigned)((H + MK_TH - 1) / MK_TH), (unsigned)N); }

long long tfc_mask_nblk(int N, int H, int W) { return (long long)N * ((H + MK_TH - 1) / MK_TH) * ((W + MK_TW - 1) / MK_TW); }
int tfc_mask_stats_floats(void) { return MS_FLOATS; }

hipError_t tfc_launch_mask_fwd(const float* img, float* lap, float* bl, void* ws, int N, int H, int W, hipStream_t st) {
  float* stats = (float*)ws;
  uint4* part = (uint4*)(stats + MS_FLOATS);
  const dim3 grid = tile_grid(N, H, W);
  const int nblk = (int)tfc_mask_nblk(N, H, W);
  hipLaunchKernelGGL(tfc_mask_lap_kernel, grid, dim3(256), 0, st, img, lap, part, H, W);
  hipLaunchKernelGGL(tfc_mask_final_extrema_kernel, dim3(1), dim3(256), 0, st, (const uint4*)part, nblk, stats, 0);
  hipLaunchKernelGGL(tfc_mask_blur_kernel, grid, dim3(256), 0, st, (const float*)lap, bl, part, (const float*)stats, gauss_taps(), H, W);
  hipLaunchKernelGGL(tfc_mask_final_extrema_kernel, dim3(1), dim3(256), 0, st, (const uint4*)part, nblk, stats, 1);
  return hipGetLastError();
}

hipError_t tfc_launch_mask_scale(const float* bl, const void* ws, float* mask, long long total, hipStream_t st) {
  hipLaunchKernelGGL(tfc_mask_scale_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, st, bl, (const float*)ws, mask, total);
  return hipGetLastError();
}

// dout: the upstream gradient [N,1,H,W], or null with ref (the L1 loss against ref: dout_buf receives scale / numel * sign(mask - ref)).
// dimg null: the loss alone (phase 0 and its finaliser).
hipError_t tfc_launch_mask_bwd(const float* lap, const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf,
                               float* dmn, float* dimg, int N, int H, int W, hipStream_t st) {
  float* stats = (float*)ws;
  double* part = (double*)(stats + MS_FLOATS);
  const long long total = (long long)N * H * W;
  const int nd = (int)((total + 1023) / 1024);
  const float gs = (float)((double)scale / (double)total);
  hipLaunchKernelGGL(tfc_mask_dot_kernel, dim3((unsigned)nd), dim3(256), 0, st, bl, (const float*)stats, dout, ref, gs, dout_buf, part, total);
  hipLaunchKernelGGL(tfc_mask_final_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nd, stats, 0, gs);
  if (dimg) {
    const dim3 grid = tile_grid(N, H, W);
    const int nblk = (int)tfc_mask_nblk(N, H, W);
    hipLaunchKernelGGL(tfc_mask_blur_bwd_kernel, grid, dim3(256), 0, st, ref ? (const float*)dout_buf : dout, bl, lap, dmn, part, (const float*)stats,
                       gauss_taps(), H, W);
    hipLaunchKernelGGL(tfc_mask_final_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nblk, stats, 1, 0.f);
    hipLaunchKernelGGL(tfc_mask_lap_bwd_kernel, grid, dim3(256), 0, st, (const float*)dmn, lap, dimg, (const float*)stats, H, W);
  }
  return hipGetLastError();
}

// ---- the phases: each launcher runs the kernels of one phase of tfc_launch_mask_fwd / tfc_launch_mask_bwd, with the record kernel in the finaliser's place
hipError_t tfc_launch_mask_phase_f1(const float* img, float* lap, void* ws, void* rec, int N, int H, int W, hipStream_t st) {
  uint4* part = (uint4*)((float*)ws + MS_FLOATS);
  hipLaunchKernelGGL(tfc_mask_lap_kernel, tile_grid(N, H, W), dim3(256), 0, st, img, lap, part, H, W);
  hipLaunchKernelGGL(tfc_mask_record_extrema_kernel, dim3(1), dim3(256), 0, st, (const uint4*)part, (int)tfc_mask_nblk(N, H, W), (unsigned long long*)rec, 0);
  return hipGetLastError();
}

hipError_t tfc_launch_mask_phase_f2(const float* lap, float* bl, void* ws, void* rec, int N, int H, int W, hipStream_t st) {
  float* stats = (float*)ws;
  uint4* part = (uint4*)(stats + MS_FLOATS);
  hipLaunchKernelGGL(tfc_mask_blur_kernel, tile_grid(N, H, W), dim3(256), 0, st, lap, bl, part, (const float*)stats, gauss_taps(), H, W);
  hipLaunchKernelGGL(tfc_mask_record_extrema_kernel, dim3(1), dim3(256), 0, st, (const uint4*)part, (int)tfc_mask_nblk(N, H, W), (unsigned long long*)rec, 1);
  return hipGetLastError();
}

hipError_t tfc_launch_mask_merge(void* ws, const void* recs, int world, int which, hipStream_t st) {
  hipLaunchKernelGGL(tfc_mask_merge_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)recs, world, (float*)ws, which);
  return hipGetLastError();
}

hipError_t tfc_launch_mask_phase_b0(const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf, void* rec, int N, int H,
                                    int W, hipStream_t st) {
  float* stats = (float*)ws;
  double* part = (double*)(stats + MS_FLOATS);
  const long long total = (long long)N * H * W;
  const int nd = (int)((total + 1023) / 1024);
  const float gs = (float)((double)scale / (double)total);
  hipLaunchKernelGGL(tfc_mask_dot_kernel, dim3((unsigned)nd), dim3(256), 0, st, bl, (const float*)stats, dout, ref, gs, dout_buf, part, total);
  hipLaunchKernelGGL(tfc_mask_record_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nd, (double*)rec, stats + MS_LOSS, gs);
  return hipGetLastError();
}

hipError_t tfc_launch_mask_phase_b1(const float* lap, const float* bl, void* ws, const float* dout, float* dmn, void* rec, int N, int H, int W, hipStream_t st) {
  float* stats = (float*)ws;
  double* part = (double*)(stats + MS_FLOATS);
  hipLaunchKernelGGL(tfc_mask_blur_bwd_kernel, tile_grid(N, H, W), dim3(256), 0, st, dout, bl, lap, dmn, part, (const float*)stats, gauss_taps(), H, W);
  hipLaunchKernelGGL(tfc_mask_record_sums_kernel, dim3(1), dim3(256), 0, st, (const double*)part, (int)tfc_mask_nblk(N, H, W), (double*)rec, (float*)nullptr, 0.f);
  return hipGetLastError();
}

hipError_t tfc_launch_mask_phase_b2(const float* lap, const void* ws, const float* dmn, float* dimg, int N, int H, int W, hipStream_t st) {
  hipLaunchKernelGGL(tfc_mask_lap_bwd_kernel, tile_grid(N, H, W), dim3(256), 0, st, dmn, lap, dimg, (const float*)ws, H, W);
  return hipGetLastError();
}

hipError_t tfc_launch_pack_plane(int dt, const float* img, const float* plane, const float* Mdev, void* out, int N, int HW, hipStream_t st) {
  const dim3 grid((unsigned)((HW / 4 + 255) / 256), (unsigned)N);
  if (dt == TFC_DT_BF16) hipLaunchKernelGGL((tfc_pack_plane_kernel<bf16_t>), grid, dim3(256), 0, st, img, plane, Mdev, (bf16_t*)out, HW);
  else hipLaunchKernelGGL((tfc_pack_plane_kernel<float>), grid, dim3(256), 0, st, img, plane, Mdev, (float*)out, HW);
  return hipGetLastError();
}
