// Kernels of the STN21 localiser (reference STN:150-201: kornia VisionTransformer(256, 64, 6) + the fc_loc MLP; Net.stn_phi), forward and backward:
//
//   tfc_vit_gemm_kernel     one dense GEMM for every nn.Linear pass:  Y = X Wt + b,  dX = dY W,  dW = dYt X  (operand addressing modes below),
//                           with the patch embedding's unfold as an addressing mode of A (forward) / B (weight gradient) / C (input gradient:
//                           patches do not overlap, so the scatter back to NCHW is a permutation), and the epilogues bias, residual add,
//                           GELU (storing the pre-activation), ReLU, Sigmoid and the GELU' / ReLU' / Sigmoid' factor of the dgrad that consumes them.
//                           v_mfma_f32_32x32x16_bf16 on bf16-rounded operands (bf16 mode) or v_mfma_f32_32x32x2_f32 (fp32 mode: an exact k-ordered
//                           fmaf chain); fp32 accumulate and fp32 storage in both.
//   tfc_vit_gemm_reduce     split-K finish: adds the K-slices in slice order, then the same epilogue.
//   tfc_vit_ln_fwd / _bwd   nn.LayerNorm(768, eps) rows (saving mean / rstd), and its input gradient (+ the residual gradient that flows past it).
//   tfc_vit_colsum          fixed-order column sums over row chunks (bias, gamma / beta, class-token / position gradients), finished by
//                           tfc_part_reduce_kernel.
//   tfc_vit_attn_fwd / _bwd softmax(q kt / sqrt(d)) v per (image, head) for T <= 64 tokens, head dim 64, q / k / v read in place from the qkv GEMM's
//                           output (the reshape(n, t, 3, heads, d) layout of _Attention); the probabilities are saved for the backward.
//   tfc_vit_attn_tiled_*    the same attention for any T (patch 32 / 16: 65 / 257 tokens), tiled 64 x 64 on the matrix core, LDS independent of T;
//                           per-row softmax statistics are saved instead of the probabilities (the section further down).
//   tfc_vit_tokens_fwd      class token + positions around the patch tokens.
//
// BATCH INVARIANCE: every tile shape and split-K count is a function of the layer shape (N, K), never of M: a sample's rows are computed by the same
// instruction sequence wherever they sit in the batch, so tokens, theta and the input gradient are bit-identical for any batch size. DETERMINISM:
// no float atomics; sums across rows (parameter gradients) are chunk partials added in a fixed order.
#include "../../include/tfc_gan.h"
#include "common.h"

namespace {
constexpr int BM = 64, BN = 64, BK = 32, LP = 68;                  // LDS row pitch (floats): 68 keeps the k-major stores of the K-contiguous loader spread

__device__ __forceinline__ float rnd_bf16(float x) { return bf16_to_f32(f32_to_bf16(x)); }

__device__ __forceinline__ long long rowoff(long long r, int rg, long long rso, long long ld) {
  return rg > 0 ? (r / rg) * rso + (r % rg) * ld : r * ld;
}

// element (m, k) of the patch matrix: m = image * patches + patch, k = channel * P * P + i * P + j; channels [0, uc) from `a`, [uc, 2 uc) from `a2`
__device__ __forceinline__ long long unfold_off(const TfcVitGemm& g, long long m, long long k, int& second) {
  const int pw = g.uw / g.up, np = (g.uh / g.up) * pw, pp = g.up * g.up;
  const long long n = m / np;
  const int pi = (int)(m % np), ph = pi / pw, px = pi % pw;
  int c = (int)(k / pp);
  const int rem = (int)(k % pp), i = rem / g.up, j = rem % g.up;
  second = c >= g.uc;
  if (second) c -= g.uc;
  return ((n * g.uc + c) * g.uh + (long long)ph * g.up + i) * g.uw + (long long)px * g.up + j;
}

__device__ __forceinline__ float ld_a(const TfcVitGemm& g, int m, int k, int kend) {
  if (m >= g.M || k >= kend) return 0.f;
  if (g.a_mode == TFC_VIT_A_ROWS) return g.a[rowoff(m, g.a_rg, g.a_rso, g.lda) + k];
  if (g.a_mode == TFC_VIT_A_TRANS) return g.a[rowoff(k, g.a_rg, g.a_rso, g.lda) + m];
  int s;
  const long long o = unfold_off(g, m, k, s);
  return (s ? g.a2 : g.a)[o];
}
__device__ __forceinline__ float ld_b(const TfcVitGemm& g, int k, int n, int kend) {
  if (n >= g.N || k >= kend) return 0.f;
  if (g.b_mode == TFC_VIT_B_WEIGHT) return g.b[(long long)n * g.ldb + k];
  if (g.b_mode == TFC_VIT_B_ROWS) return g.b[(long long)k * g.ldb + n];
  int s;
  const long long o = unfold_off(g, k, n, s);
  return (s ? g.b2 : g.b)[o];
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  const float pdf = expf(-0.5f * x * x) * 0.39894228040143268f;
  return cdf + x * pdf;
}

// bias -> residual -> activation / activation-derivative factor -> store (row m, column n of the GEMM)
__device__ __forceinline__ void epilogue(const TfcVitGemm& g, int m, int n, float v) {
  if (g.bias) v += g.bias[n];
  const long long co = g.c_mode == TFC_VIT_C_ROWS ? rowoff(m, g.c_rg, g.c_rso, g.ldc) + n : 0;
  if (g.res) v += g.res[co];
  const long long xo = (long long)m * g.ldaux + n;
  switch (g.act) {
    case TFC_VIT_ACT_GELU: g.aux[xo] = v; v = gelu_f(v); break;
    case TFC_VIT_ACT_RELU: v = v > 0.f ? v : 0.f; break;
    case TFC_VIT_ACT_SIGMOID: v = 1.f / (1.f + expf(-v)); break;
    case TFC_VIT_DACT_GELU: v *= gelu_d(g.aux[xo]); break;
    case TFC_VIT_DACT_RELU: v = g.aux[xo] > 0.f ? v : 0.f; break;
    case TFC_VIT_DACT_SIGMOID: { const float s = g.aux[xo]; v = v * (1.f - s) * s; } break;
    default: break;
  }
  if (g.c_mode == TFC_VIT_C_ROWS) {
    g.c[co] = v;
  } else {
    int s;
    const long long o = unfold_off(g, m, n, s);
    float* dst = s ? g.c2 : g.c;
    if (dst) dst[o] = v;
  }
}
}  // namespace

// grid (N / 64, rows of this launch / 64, K-slices); 4 waves, each owns a 32 x 32 quarter of the 64 x 64 tile. K-slice z covers [z kc, (z+1) kc).
// part == nullptr: epilogue in place; otherwise the raw slice sums go to part[z][m - m0][n].
template <int DT>
__global__ void __launch_bounds__(256)
tfc_vit_gemm_kernel(const TfcVitGemm g, int m0, int mrows, int kc, float* __restrict__ part) {
  __shared__ float As[BK][LP], Bs[BK][LP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w & 1, wn = w >> 1;
  const int tm = m0 + blockIdx.y * BM, tn = blockIdx.x * BN, z = blockIdx.z;
  const int kbeg = z * kc, kend = min(g.K, kbeg + kc);
  const int mend = m0 + mrows;
  // loader lane maps: K-contiguous operands (A rows / unfold, B weight) walk k across lanes, the others walk the row / column index
  const bool a_kc = g.a_mode != TFC_VIT_A_TRANS, b_kc = g.b_mode == TFC_VIT_B_WEIGHT;
  float ra[8], rb[8];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int m, k;
      if (a_kc) { k = k0 + (tid & 31); m = tm + (tid >> 5) + 8 * i; }
      else { m = tm + (tid & 63); k = k0 + (tid >> 6) + 4 * i; }
      ra[i] = m < mend ? ld_a(g, m, k, kend) : 0.f;
      int n;
      if (b_kc) { k = k0 + (tid & 31); n = tn + (tid >> 5) + 8 * i; }
      else { n = tn + (tid & 63); k = k0 + (tid >> 6) + 4 * i; }
      rb[i] = ld_b(g, k, n, kend);
    }
  };
  f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (a_kc) As[tid & 31][(tid >> 5) + 8 * i] = ra[i];
      else As[(tid >> 6) + 4 * i][tid & 63] = ra[i];
      if (b_kc) Bs[tid & 31][(tid >> 5) + 8 * i] = rb[i];
      else Bs[(tid >> 6) + 4 * i][tid & 63] = rb[i];
    }
    __syncthreads();
    if (k0 + BK < kend) load(k0 + BK);                              // next tile's loads in flight under this tile's MFMAs
    const int r = lane & 31, h = lane >> 5;
    if constexpr (DT == TFC_DT_BF16) {
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        bf16x8_t fa, fb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          fa[j] = (__bf16)As[16 * s + 8 * h + j][wm * 32 + r];
          fb[j] = (__bf16)Bs[16 * s + 8 * h + j][wn * 32 + r];
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < BK / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + h][wm * 32 + r], Bs[2 * s + h][wn * 32 + r], acc, 0, 0, 0);
    }
  }
  const int col = tn + wn * 32 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = tm + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (row < mend && col < g.N) {
      if (part) part[((size_t)z * mrows + (row - m0)) * g.N + col] = acc[i];
      else epilogue(g, row, col, acc[i]);
    }
  }
}

__global__ void __launch_bounds__(256)
tfc_vit_gemm_reduce_kernel(const TfcVitGemm g, int m0, int mrows, int nslices, const float* __restrict__ part) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, tot = (long long)mrows * g.N;
  if (idx >= tot) return;
  float v = part[idx];
  for (int z = 1; z < nslices; ++z) v += part[(size_t)z * tot + idx];
  epilogue(g, m0 + (int)(idx / g.N), (int)(idx % g.N), v);
}

// K-slices: a function of K alone (the shapes of this network: K = 24576 -> 8 slices of 3072, K = 13056 -> 5 of 2624, K <= 4096 -> 1)
static int vit_kslice(int K, int* nslices) {
  const int ktiles = (K + BK - 1) / BK;
  int s = K > 4096 ? (K + 3071) / 3072 : 1;
  const int kt = (ktiles + s - 1) / s;
  *nslices = (ktiles + kt - 1) / kt;
  return kt * BK;
}

hipError_t tfc_launch_vit_gemm(int dt, const TfcVitGemm& g, float* part_ws, hipStream_t st) {
  int ns;
  const int kc = vit_kslice(g.K, &ns);
  if (ns == 1) {
    const dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, 1);
    if (dt == TFC_DT_BF16) hipLaunchKernelGGL(tfc_vit_gemm_kernel<TFC_DT_BF16>, grid, dim3(256), 0, st, g, 0, g.M, kc, (float*)nullptr);
    else hipLaunchKernelGGL(tfc_vit_gemm_kernel<TFC_DT_F32>, grid, dim3(256), 0, st, g, 0, g.M, kc, (float*)nullptr);
    return hipGetLastError();
  }
  if (!part_ws) return hipErrorInvalidValue;
  // rows per launch so that the slices fit the scratch: row chunks are multiples of the tile height, so every row still sees the same tiles
  long long cap = (long long)TFC_PART_WS_FLOATS / ((long long)ns * g.N) / BM * BM;
  if (cap < BM) return hipErrorInvalidValue;
  for (int m0 = 0; m0 < g.M; m0 += (int)cap) {
    const int mr = (int)std::min<long long>(cap, (long long)g.M - m0);
    const dim3 grid((g.N + BN - 1) / BN, (mr + BM - 1) / BM, ns);
    if (dt == TFC_DT_BF16) hipLaunchKernelGGL(tfc_vit_gemm_kernel<TFC_DT_BF16>, grid, dim3(256), 0, st, g, m0, mr, kc, part_ws);
    else hipLaunchKernelGGL(tfc_vit_gemm_kernel<TFC_DT_F32>, grid, dim3(256), 0, st, g, m0, mr, kc, part_ws);
    const long long tot = (long long)mr * g.N;
    hipLaunchKernelGGL(tfc_vit_gemm_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, g, m0, mr, ns, (const float*)part_ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- LayerNorm: one wave per row of D (a multiple of 64, <= 1024) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
tfc_vit_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gam, const float* __restrict__ bet, float* __restrict__ y, float* __restrict__ mean,
                      float* __restrict__ rstd, int rows, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int nv = D >> 6;
  const float* xr = x + (size_t)row * D;
  float v[16], s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) if (i < nv) { v[i] = xr[i * 64 + lane]; s += v[i]; }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) if (i < nv) { const float d = v[i] - mu; q += d * d; }
  const float rs = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
  float* yr = y + (size_t)row * D;
#pragma unroll
  for (int i = 0; i < 16; ++i) if (i < nv) { const int c = i * 64 + lane; yr[c] = (v[i] - mu) * rs * gam[c] + bet[c]; }
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// dx = dres + rstd (gdy - mean(gdy) - xhat mean(gdy xhat)),  gdy = gamma * dy
__global__ void __launch_bounds__(256)
tfc_vit_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                      const float* __restrict__ gam, const float* dres, float* dx, int rows, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int nv = D >> 6;
  const size_t ro = (size_t)row * D;
  const float mu = mean[row], rs = rstd[row];
  float gd[16], xh[16], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < nv) {
      const int c = i * 64 + lane;
      gd[i] = gam[c] * dy[ro + c];
      xh[i] = (x[ro + c] - mu) * rs;
      s1 += gd[i];
      s2 += gd[i] * xh[i];
    }
  const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < nv) {
      const int c = i * 64 + lane;
      const float v = rs * (gd[i] - m1 - xh[i] * m2);
      dx[ro + c] = dres ? dres[ro + c] + v : v;
    }
}

// ---- column sums over chunks of 32 rows: part[chunk][j] = sum x[r][j]; with x_ln: part[chunk][j] = sum dy xhat, part[chunk][L + j] = sum dy -----------
constexpr int kColChunk = 32;
__global__ void __launch_bounds__(256)
tfc_vit_colsum_kernel(const float* __restrict__ v, long long ld, int rows, int L, const float* __restrict__ x_ln, const float* __restrict__ mean,
                      const float* __restrict__ rstd, float* __restrict__ part) {
  const int j = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
  if (j >= L) return;
  const int r0 = ch * kColChunk, r1 = min(rows, r0 + kColChunk);
  float s = 0.f, sx = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float d = v[(size_t)r * ld + j];
    s += d;
    if (x_ln) sx += d * ((x_ln[(size_t)r * L + j] - mean[r]) * rstd[r]);
  }
  if (x_ln) { part[(size_t)ch * 2 * L + j] = sx; part[(size_t)ch * 2 * L + L + j] = s; }
  else part[(size_t)ch * L + j] = s;
}

// ---- attention per (image, head): T <= 64 tokens, head dim 64 --------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
constexpr int AP = 65;                                             // LDS row pitch of the [T][64] / [T][T] tiles

// x . y over the head dim as an unevaluated sum hi + lo, about twice fp32's precision (Ogita / Rump / Oishi Dot2: the product's error by fma, the
// sum's by TwoSum; no contraction, or the error terms are not the errors). A logit kept in ONE fp32 is known to ulp(|logit|) only: at logits of
// +-100 that is 4e-6 absolute, it is the RELATIVE error of every small probability of a row, and the query / key gradients of a nearly one-hot
// row are made of exactly those: 1e-6 rel-L2 on the probabilities and up to 3e-5 on dqkv against fp64, whatever the order of an fp32 sum
// (test_attention_fp32_large_logits; with hi + lo: 2e-8 and 3e-7).
__device__ __forceinline__ void dot64_2(const float* x, const float* y, float& hi, float& lo) {
#pragma clang fp contract(off)
  float s = 0.f, c = 0.f;
  for (int d = 0; d < 64; ++d) {
    const float a = x[d], b = y[d];
    const float p = a * b, pe = fmaf(a, b, -p);
    const float t = s + p, z = t - s, se = (s - (t - z)) + (p - z);
    s = t;
    c += pe + se;
  }
  hi = s; lo = c;
}

template <int DT>
__global__ void __launch_bounds__(256)
tfc_vit_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ probs, int T, int H, float scale) {
  extern __shared__ float sm[];
  float* q = sm; float* k = q + T * AP; float* v = k + T * AP; float* p = v + T * AP;
  const int h = blockIdx.x, n = blockIdx.y, D = H * 64, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto op = [](float x) { return DT == TFC_DT_BF16 ? rnd_bf16(x) : x; };
  for (int i = threadIdx.x; i < T * 64; i += 256) {
    const int t = i >> 6, d = i & 63;
    const size_t b = ((size_t)n * T + t) * 3 * D + h * 64 + d;
    q[t * AP + d] = op(qkv[b]); k[t * AP + d] = op(qkv[b + D]); v[t * AP + d] = op(qkv[b + 2 * D]);
  }
  __syncthreads();
  for (int i = w; i < T; i += 4) {
    const int j = lane;
    float hi = -INFINITY, lo = 0.f;
    if (j < T) { dot64_2(q + i * AP, k + j * AP, hi, lo); if (scale < 0.f) { hi = -hi; lo = -lo; } }   // the maximum of the SCALED logits
    // the maximum is subtracted from hi + lo, so the rounding to one fp32 happens on the DIFFERENCE: the entries that carry weight have a small one
    const float mh = wave_max(hi);
    const float ml = wave_max(hi == mh ? lo : -INFINITY);
    const float e = j < T ? expf(((hi - mh) + (lo - ml)) * fabsf(scale)) : 0.f;
    const float pij = e / wave_sum(e);
    if (j < T) { probs[(((size_t)n * H + h) * T + i) * T + j] = pij; p[i * AP + j] = op(pij); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * 64; i += 256) {
    const int t = i >> 6, d = i & 63;
    float a = 0.f;
    for (int j = 0; j < T; ++j) a = fmaf(p[t * AP + j], v[j * AP + d], a);
    out[((size_t)n * T + t) * D + h * 64 + d] = a;
  }
}

template <int DT>
__global__ void __launch_bounds__(256)
tfc_vit_attn_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ qkv, const float* __restrict__ probs, float* __restrict__ dqkv, int T, int H,
                        float scale) {
  extern __shared__ float sm[];
  float* q = sm; float* k = q + T * AP; float* v = k + T * AP; float* go = v + T * AP; float* p = go + T * AP; float* ds = p + T * AP;
  const int h = blockIdx.x, n = blockIdx.y, D = H * 64, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto op = [](float x) { return DT == TFC_DT_BF16 ? rnd_bf16(x) : x; };
  for (int i = threadIdx.x; i < T * 64; i += 256) {
    const int t = i >> 6, d = i & 63;
    const size_t b = ((size_t)n * T + t) * 3 * D + h * 64 + d;
    q[t * AP + d] = op(qkv[b]); k[t * AP + d] = op(qkv[b + D]); v[t * AP + d] = op(qkv[b + 2 * D]);
    go[t * AP + d] = op(dout[((size_t)n * T + t) * D + h * 64 + d]);
  }
  for (int i = threadIdx.x; i < T * T; i += 256) p[(i / T) * AP + i % T] = probs[((size_t)n * H + h) * T * T + i];
  __syncthreads();
  for (int i = w; i < T; i += 4) {                                  // dS = P (dP - rowsum(P dP)) * scale,  dP = dO vt
    const int j = lane;
    float dp = 0.f, pij = 0.f;
    if (j < T) {
      for (int d = 0; d < 64; ++d) dp = fmaf(go[i * AP + d], v[j * AP + d], dp);
      pij = p[i * AP + j];
    }
    const float t = wave_sum(pij * dp);
    if (j < T) ds[i * AP + j] = op(pij * (dp - t) * scale);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * 64; i += 256) {
    const int t = i >> 6, d = i & 63;
    float dq = 0.f, dk = 0.f, dv = 0.f;
    for (int j = 0; j < T; ++j) {
      dq = fmaf(ds[t * AP + j], k[j * AP + d], dq);               // dQ[t] = sum_j dS[t][j] k[j]
      dk = fmaf(ds[j * AP + t], q[j * AP + d], dk);               // dK[t] = sum_i dS[i][t] q[i]
      dv = fmaf(op(p[j * AP + t]), go[j * AP + d], dv);           // dV[t] = sum_i P[i][t] dO[i]
    }
    const size_t b = ((size_t)n * T + t) * 3 * D + h * 64 + d;
    dqkv[b] = dq; dqkv[b + D] = dk; dqkv[b + 2 * D] = dv;
  }
}

// ---- tiled attention per (image, head, tile): any T, head dim 64 -----------------------------------------------------------------------------------
// Query rows and key rows are cut into tiles of TQ = TK = 64 (tests/test_gpu_47_localiser_patch.py runs T = 63, 64, 65 and 127, 128, 129 around
// them). LDS holds one [64][AP] image per operand tile whatever T is, and no T x T tensor exists in memory: the forward saves three floats per
// (image, head, query row) -- the row maximum of the signed logits as hi + lo and the sum l of exp((logit - max) |scale|) -- and the backward
// recomputes P = exp(..) / l tile by tile. Every product runs on the matrix core through mma64 (bf16 mode: v_mfma_f32_32x32x16_bf16 on the
// bf16-rounded operands; fp32 mode: v_mfma_f32_32x32x2_f32), except the fp32-mode logits, which stay the compensated hi + lo dot product of
// dot64_2 on the VALU until the row maximum is subtracted. Rounding points as in the kernels above: q, k, v, dO when loaded, the NORMALISED P
// before P v and Pt dO, dS (formed from the fp32 P) before dS k and dSt q. So each kernel walks the key tiles twice: row statistics (forward:
// maximum and sum; backward: delta = rowsum(P dP)) first, products second; nothing unnormalised is rescaled after the fact.
// A workgroup = 4 waves; wave (wm, wn) owns the 32 x 32 quarter of the 64 x 64 tile product and holds it in the MFMA result layout
// (column = lane & 31, row = acc_row(register, lane >> 5)), in fp32 mode too. Tile shapes and loop orders depend on T and H only; dK / dV are
// summed over the query tiles in tile order by the workgroup that owns the key tile; no atomics.
constexpr int TQ = 64, TK = 64;

__device__ __forceinline__ int acc_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

// acc += sum over k < 64 of A(m, k) B(k, n), (m, n) in the wave's 32 x 32 quarter: A(m, k) = a[m * AM + k * AK], B(k, n) = b[n * BN + k * BKS].
// With pitch AP = 65 a read with the lane on the row (stride 65) and one with the lane on the column (stride 1) are both conflict free.
template <int DT, int AM, int AK, int BN, int BKS>
__device__ __forceinline__ void mma64(f32x16_t& acc, const float* a, const float* b) {
  const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
  if constexpr (DT == TFC_DT_BF16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8_t fa, fb;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        fa[j] = (__bf16)a[r * AM + (16 * s + 8 * h + j) * AK];      // exact: the tiles hold bf16-rounded values
        fb[j] = (__bf16)b[r * BN + (16 * s + 8 * h + j) * BKS];
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int s = 0; s < 32; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r * AM + (2 * s + h) * AK], b[r * BN + (2 * s + h) * BKS], acc, 0, 0, 0);
  }
}

// rows [row0, row0 + 64) of a [T][ld] matrix (64 columns from src) into a [64][AP] tile, rounded where the mode rounds; rows past T are zero
template <int DT>
__device__ __forceinline__ void load_tile(float* dst, const float* __restrict__ src, size_t ld, int row0, int T) {
  const int d = threadIdx.x & 63, t0 = threadIdx.x >> 6;
  float x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {                                    // all 16 loads in flight before the first store (a row past T re-reads row T - 1)
    const int row = row0 + t0 + 4 * i;
    const float v = src[(size_t)min(row, T - 1) * ld + d];
    x[i] = row < T ? v : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) dst[(t0 + 4 * i) * AP + d] = DT == TFC_DT_BF16 ? rnd_bf16(x[i]) : x[i];
}

// dot64_2 for the 16 rows of a lane at once (the key row is read once per d); qs at the wave's first query row, kr at the lane's key row
__device__ __forceinline__ void dot64_2x16(const float* qs, const float* kr, int half, float (&hi)[16], float (&lo)[16]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 16; ++i) { hi[i] = 0.f; lo[i] = 0.f; }
  for (int d = 0; d < 64; ++d) {
    const float b = kr[d];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float a = qs[acc_row(i, half) * AP + d];
      const float p = a * b, pe = fmaf(a, b, -p);
      const float s = hi[i], t = s + p, z = t - s, se = (s - (t - z)) + (p - z);
      hi[i] = t;
      lo[i] += pe + se;
    }
  }
}

// signed logits of the wave's quarter as hi + lo (bf16 mode: products of bf16 values are exact in fp32 and the MFMA sum is the logit, lo = 0)
template <int DT>
__device__ __forceinline__ void tile_logits(const float* qs, const float* ks, float sgn, float (&hi)[16], float (&lo)[16]) {
  const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
  if constexpr (DT == TFC_DT_BF16) {
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    mma64<DT, AP, 1, AP, 1>(acc, qs, ks);
#pragma unroll
    for (int i = 0; i < 16; ++i) { hi[i] = sgn * acc[i]; lo[i] = 0.f; }
  } else {
    dot64_2x16(qs, ks + r * AP, h, hi, lo);
#pragma unroll
    for (int i = 0; i < 16; ++i) { hi[i] *= sgn; lo[i] *= sgn; }
  }
}

// (mh + ml, l) <- merged with (mh2 + ml2, l2): the larger maximum (hi first, then lo) stays, the other side's sum is rescaled to it. The result
// has the same bits whichever side is "self" (the products and the sum commute), so a butterfly leaves every lane with one value.
__device__ __forceinline__ void stat_merge(float& mh, float& ml, float& l, float mh2, float ml2, float l2, float as) {
  if (mh2 == -INFINITY) return;                                     // the other side has seen no column
  if (mh == -INFINITY) { mh = mh2; ml = ml2; l = l2; return; }
  const bool other = mh2 > mh || (mh2 == mh && ml2 > ml);
  const float e = expf((other ? (mh - mh2) + (ml - ml2) : (mh2 - mh) + (ml2 - ml)) * as);
  l = other ? l * e + l2 : l + l2 * e;
  if (other) { mh = mh2; ml = ml2; }
}

__device__ __forceinline__ float tile_prob(float hi, float lo, float mh, float ml, float l, float as) {
  return expf(((hi - mh) + (lo - ml)) * as) / l;
}

// grid (query tiles, H, N). stats [N][H][3][T]: maximum hi, maximum lo, l.
template <int DT>
__global__ void __launch_bounds__(256)
tfc_vit_attn_tiled_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ stats, int T, int H, float scale) {
  extern __shared__ float sm[];
  float* Qs = sm; float* Ks = Qs + 64 * AP; float* Vs = Ks + 64 * AP; float* Ps = Vs + 64 * AP; float* red = Ps + 64 * AP;   // red [2][64][3]
  const int q0 = blockIdx.x * TQ, hd = blockIdx.y, n = blockIdx.z, D = H * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w & 1, wn = w >> 1, r = lane & 31, hf = lane >> 5;
  const size_t ld = 3 * (size_t)D;
  const float* qb = qkv + (size_t)n * T * ld + hd * 64;
  const float sgn = scale < 0.f ? -1.f : 1.f, as = fabsf(scale);
  const int nkt = (T + TK - 1) / TK;
  auto op = [](float x) { return DT == TFC_DT_BF16 ? rnd_bf16(x) : x; };
  load_tile<DT>(Qs, qb, ld, q0, T);
  float mh[16], ml[16], l[16], hi[16], lo[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { mh[i] = -INFINITY; ml[i] = 0.f; l[i] = 0.f; }
  for (int kt = 0; kt < nkt; ++kt) {                                // walk 1: each lane folds its own column of every key tile
    __syncthreads();
    load_tile<DT>(Ks, qb + D, ld, kt * TK, T);
    __syncthreads();
    tile_logits<DT>(Qs + wm * 32 * AP, Ks + wn * 32 * AP, sgn, hi, lo);
    if (kt * TK + wn * 32 + r < T) {
#pragma unroll
      for (int i = 0; i < 16; ++i) stat_merge(mh[i], ml[i], l[i], hi[i], lo[i], 1.f, as);
    }
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {                                // the 32 columns of the half wave that shares the rows
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float a = __shfl_xor(mh[i], o, 64), b = __shfl_xor(ml[i], o, 64), c = __shfl_xor(l[i], o, 64);
      stat_merge(mh[i], ml[i], l[i], a, b, c, as);
    }
  }
  if (r == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float* d = red + (wn * 64 + wm * 32 + acc_row(i, hf)) * 3;
      d[0] = mh[i]; d[1] = ml[i]; d[2] = l[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {                                    // the two column halves, in one order for every wave
    const int row = wm * 32 + acc_row(i, hf);
    const float* a = red + row * 3;
    const float* b = red + (64 + row) * 3;
    mh[i] = a[0]; ml[i] = a[1]; l[i] = a[2];
    stat_merge(mh[i], ml[i], l[i], b[0], b[1], b[2], as);
    if (wn == 0 && r == 0 && q0 + row < T) {
      float* st = stats + ((size_t)n * H + hd) * 3 * T + q0 + row;
      st[0] = mh[i]; st[T] = ml[i]; st[2 * (size_t)T] = l[i];
    }
  }
  f32x16_t o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {                                // walk 2: normalised P, rounded, times v
    __syncthreads();
    load_tile<DT>(Ks, qb + D, ld, kt * TK, T);
    load_tile<DT>(Vs, qb + 2 * D, ld, kt * TK, T);
    __syncthreads();
    tile_logits<DT>(Qs + wm * 32 * AP, Ks + wn * 32 * AP, sgn, hi, lo);
    const bool cv = kt * TK + wn * 32 + r < T;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      Ps[(wm * 32 + acc_row(i, hf)) * AP + wn * 32 + r] = cv ? op(tile_prob(hi[i], lo[i], mh[i], ml[i], l[i], as)) : 0.f;
    __syncthreads();
    mma64<DT, AP, 1, 1, AP>(o, Ps + wm * 32 * AP, Vs + wn * 32);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = q0 + wm * 32 + acc_row(i, hf);
    if (row < T) out[((size_t)n * T + row) * D + hd * 64 + wn * 32 + r] = o[i];
  }
}

// the fp32 P and dP = dO vt of the wave's quarter for one (query tile, key tile); st: the rows' statistics (LDS [4][64]: mh, ml, l, delta)
template <int DT>
__device__ __forceinline__ void tile_p_dp(const float* Qs, const float* Ks, const float* Vs, const float* dOs, const float* st, bool cv, float sgn, float as,
                                          float (&p)[16], f32x16_t& dp) {
  const int w = threadIdx.x >> 6, wm = w & 1, wn = w >> 1, hf = (threadIdx.x >> 5) & 1;
  float hi[16], lo[16];
  tile_logits<DT>(Qs + wm * 32 * AP, Ks + wn * 32 * AP, sgn, hi, lo);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = wm * 32 + acc_row(i, hf);
    p[i] = cv && st[192 + row] != 0.f ? tile_prob(hi[i], lo[i], st[row], st[64 + row], st[128 + row], as) : 0.f;
    dp[i] = 0.f;
  }
  mma64<DT, AP, 1, AP, 1>(dp, dOs + wm * 32 * AP, Vs + wn * 32 * AP);
}

// the statistics of query rows [q0, q0 + 64) into st [4][64]: mh, ml, l and 1 (a row of the sequence) or 0 (past T: its P is forced to 0)
__device__ __forceinline__ void load_row_stats(float* st, const float* __restrict__ stats, int q0, int T) {
  if (threadIdx.x < 64) {
    const int row = q0 + threadIdx.x;
    const bool v = row < T;
    st[threadIdx.x] = v ? stats[row] : 0.f;
    st[64 + threadIdx.x] = v ? stats[T + row] : 0.f;
    st[128 + threadIdx.x] = v ? stats[2 * (size_t)T + row] : 1.f;
    st[192 + threadIdx.x] = v ? 1.f : 0.f;
  }
}

// grid (query tiles, H, N): delta[n][h][row] = sum_j P dP (walk 1), dQ = sum over key tiles of round(P (dP - delta) scale) k (walk 2)
template <int DT>
__global__ void __launch_bounds__(256)
tfc_vit_attn_tiled_dq_kernel(const float* __restrict__ dout, const float* __restrict__ qkv, const float* __restrict__ stats, float* __restrict__ dqkv,
                             float* __restrict__ delta, int T, int H, float scale) {
  extern __shared__ float sm[];
  float* Qs = sm; float* Ks = Qs + 64 * AP; float* Vs = Ks + 64 * AP; float* dOs = Vs + 64 * AP; float* dSs = dOs + 64 * AP;
  float* st = dSs + 64 * AP; float* red = st + 256;                 // st [4][64], red [2][64]
  const int q0 = blockIdx.x * TQ, hd = blockIdx.y, n = blockIdx.z, D = H * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w & 1, wn = w >> 1, r = lane & 31, hf = lane >> 5;
  const size_t ld = 3 * (size_t)D;
  const float* qb = qkv + (size_t)n * T * ld + hd * 64;
  const float sgn = scale < 0.f ? -1.f : 1.f, as = fabsf(scale);
  const int nkt = (T + TK - 1) / TK;
  auto op = [](float x) { return DT == TFC_DT_BF16 ? rnd_bf16(x) : x; };
  load_tile<DT>(Qs, qb, ld, q0, T);
  load_tile<DT>(dOs, dout + (size_t)n * T * D + hd * 64, D, q0, T);
  load_row_stats(st, stats + ((size_t)n * H + hd) * 3 * T, q0, T);
  float p[16], dl[16];
  f32x16_t dp;
#pragma unroll
  for (int i = 0; i < 16; ++i) dl[i] = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    load_tile<DT>(Ks, qb + D, ld, kt * TK, T);
    load_tile<DT>(Vs, qb + 2 * D, ld, kt * TK, T);
    __syncthreads();
    tile_p_dp<DT>(Qs, Ks, Vs, dOs, st, kt * TK + wn * 32 + r < T, sgn, as, p, dp);
#pragma unroll
    for (int i = 0; i < 16; ++i) dl[i] = fmaf(p[i], dp[i], dl[i]);
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) dl[i] += __shfl_xor(dl[i], o, 64);
  }
  if (r == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wn * 64 + wm * 32 + acc_row(i, hf)] = dl[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = wm * 32 + acc_row(i, hf);
    dl[i] = red[row] + red[64 + row];
    if (wn == 0 && r == 0 && q0 + row < T) delta[((size_t)n * H + hd) * T + q0 + row] = dl[i];
  }
  f32x16_t dq;
#pragma unroll
  for (int i = 0; i < 16; ++i) dq[i] = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    load_tile<DT>(Ks, qb + D, ld, kt * TK, T);
    load_tile<DT>(Vs, qb + 2 * D, ld, kt * TK, T);
    __syncthreads();
    tile_p_dp<DT>(Qs, Ks, Vs, dOs, st, kt * TK + wn * 32 + r < T, sgn, as, p, dp);
#pragma unroll
    for (int i = 0; i < 16; ++i) dSs[(wm * 32 + acc_row(i, hf)) * AP + wn * 32 + r] = op(p[i] * (dp[i] - dl[i]) * scale);
    __syncthreads();
    mma64<DT, AP, 1, 1, AP>(dq, dSs + wm * 32 * AP, Ks + wn * 32);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = q0 + wm * 32 + acc_row(i, hf);
    if (row < T) dqkv[((size_t)n * T + row) * ld + hd * 64 + wn * 32 + r] = dq[i];
  }
}

// grid (key tiles, H, N): dV = sum_i round(P)[i][.] dO[i], dK = sum_i round(dS)[i][.] q[i], the query tiles taken in order
template <int DT>
__global__ void __launch_bounds__(256)
tfc_vit_attn_tiled_dkv_kernel(const float* __restrict__ dout, const float* __restrict__ qkv, const float* __restrict__ stats, const float* __restrict__ delta,
                              float* __restrict__ dqkv, int T, int H, float scale) {
  extern __shared__ float sm[];
  float* Qs = sm; float* Ks = Qs + 64 * AP; float* Vs = Ks + 64 * AP; float* dOs = Vs + 64 * AP; float* Ps = dOs + 64 * AP; float* dSs = Ps + 64 * AP;
  float* st = dSs + 64 * AP; float* dls = st + 256;                 // st [4][64], dls [64]
  const int k0 = blockIdx.x * TK, hd = blockIdx.y, n = blockIdx.z, D = H * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w & 1, wn = w >> 1, r = lane & 31, hf = lane >> 5;
  const size_t ld = 3 * (size_t)D;
  const float* qb = qkv + (size_t)n * T * ld + hd * 64;
  const float sgn = scale < 0.f ? -1.f : 1.f, as = fabsf(scale);
  const int nqt = (T + TQ - 1) / TQ;
  const bool cv = k0 + wn * 32 + r < T;
  auto op = [](float x) { return DT == TFC_DT_BF16 ? rnd_bf16(x) : x; };
  load_tile<DT>(Ks, qb + D, ld, k0, T);
  load_tile<DT>(Vs, qb + 2 * D, ld, k0, T);
  float p[16];
  f32x16_t dp, dk, dv;
#pragma unroll
  for (int i = 0; i < 16; ++i) { dk[i] = 0.f; dv[i] = 0.f; }
  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();
    load_tile<DT>(Qs, qb, ld, qt * TQ, T);
    load_tile<DT>(dOs, dout + (size_t)n * T * D + hd * 64, D, qt * TQ, T);
    load_row_stats(st, stats + ((size_t)n * H + hd) * 3 * T, qt * TQ, T);
    if (threadIdx.x < 64) dls[threadIdx.x] = qt * TQ + threadIdx.x < T ? delta[((size_t)n * H + hd) * T + qt * TQ + threadIdx.x] : 0.f;
    __syncthreads();
    tile_p_dp<DT>(Qs, Ks, Vs, dOs, st, cv, sgn, as, p, dp);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = wm * 32 + acc_row(i, hf);
      Ps[row * AP + wn * 32 + r] = op(p[i]);
      dSs[row * AP + wn * 32 + r] = op(p[i] * (dp[i] - dls[row]) * scale);
    }
    __syncthreads();
    mma64<DT, 1, AP, 1, AP>(dv, Ps + wm * 32, dOs + wn * 32);       // the sum runs over the query rows: both operands are read by columns
    mma64<DT, 1, AP, 1, AP>(dk, dSs + wm * 32, Qs + wn * 32);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = k0 + wm * 32 + acc_row(i, hf);
    if (row < T) {
      const size_t b = ((size_t)n * T + row) * ld + hd * 64 + wn * 32 + r;
      dqkv[b + D] = dk[i]; dqkv[b + 2 * D] = dv[i];
    }
  }
}

// x[n][0] = cls + pos[0]; x[n][t] += pos[t] for t >= 1 (the patch GEMM wrote the patch tokens, bias included, into rows 1..T-1)
__global__ void __launch_bounds__(256)
tfc_vit_tokens_fwd_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos, int N, int T, int D) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * T * D) return;
  const int c = (int)(idx % D), t = (int)((idx / D) % T);
  x[idx] = (t == 0 ? cls[c] : x[idx]) + pos[(size_t)t * D + c];
}

hipError_t tfc_launch_vit_ln_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, int rows, int D, float eps, hipStream_t st) {
  hipLaunchKernelGGL(tfc_vit_ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, g, b, y, mean, rstd, rows, D, eps);
  return hipGetLastError();
}

hipError_t tfc_launch_vit_colsum(const float* v, long long ld, int rows, int L, const float* x_ln, const float* mean, const float* rstd, float* out,
                                 float* part_ws, hipStream_t st) {
  const int nch = (rows + kColChunk - 1) / kColChunk, width = x_ln ? 2 * L : L;
  if (!part_ws || (long long)nch * width > (long long)TFC_PART_WS_FLOATS) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(out, 0, sizeof(float) * width, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tfc_vit_colsum_kernel, dim3((L + 255) / 256, nch), dim3(256), 0, st, v, ld, rows, L, x_ln, mean, rstd, part_ws);
  return tfc_launch_part_reduce(part_ws, out, 1, nch, width, st);
}

hipError_t tfc_launch_vit_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, const float* dres, float* dx,
                                 float* dgb, int rows, int D, float* part_ws, hipStream_t st) {
  if (dgb) {
    const hipError_t e = tfc_launch_vit_colsum(dy, D, rows, D, x, mean, rstd, dgb, part_ws, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tfc_vit_ln_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, dy, x, mean, rstd, g, dres, dx, rows, D);
  return hipGetLastError();
}

static hipError_t attn_lds(const void* fn, size_t bytes) {
  return bytes > 65536 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipSuccess;
}

hipError_t tfc_launch_vit_attn_fwd(int dt, const float* qkv, float* out, float* probs, int N, int T, int H, float scale, hipStream_t st) {
  const size_t lds = sizeof(float) * 4 * T * AP;
  const void* fn = dt == TFC_DT_BF16 ? (const void*)&tfc_vit_attn_fwd_kernel<TFC_DT_BF16> : (const void*)&tfc_vit_attn_fwd_kernel<TFC_DT_F32>;
  hipError_t e = attn_lds(fn, lds);
  if (e != hipSuccess) return e;
  if (dt == TFC_DT_BF16) hipLaunchKernelGGL(tfc_vit_attn_fwd_kernel<TFC_DT_BF16>, dim3(H, N), dim3(256), lds, st, qkv, out, probs, T, H, scale);
  else hipLaunchKernelGGL(tfc_vit_attn_fwd_kernel<TFC_DT_F32>, dim3(H, N), dim3(256), lds, st, qkv, out, probs, T, H, scale);
  return hipGetLastError();
}

hipError_t tfc_launch_vit_attn_bwd(int dt, const float* dout, const float* qkv, const float* probs, float* dqkv, int N, int T, int H, float scale,
                                   hipStream_t st) {
  const size_t lds = sizeof(float) * 6 * T * AP;
  const void* fn = dt == TFC_DT_BF16 ? (const void*)&tfc_vit_attn_bwd_kernel<TFC_DT_BF16> : (const void*)&tfc_vit_attn_bwd_kernel<TFC_DT_F32>;
  hipError_t e = attn_lds(fn, lds);
  if (e != hipSuccess) return e;
  if (dt == TFC_DT_BF16) hipLaunchKernelGGL(tfc_vit_attn_bwd_kernel<TFC_DT_BF16>, dim3(H, N), dim3(256), lds, st, dout, qkv, probs, dqkv, T, H, scale);
  else hipLaunchKernelGGL(tfc_vit_attn_bwd_kernel<TFC_DT_F32>, dim3(H, N), dim3(256), lds, st, dout, qkv, probs, dqkv, T, H, scale);
  return hipGetLastError();
}

template <typename K>
static hipError_t attn_tiled_lds(K* bf16_fn, K* f32_fn, int dt, size_t bytes) {
  return attn_lds(dt == TFC_DT_BF16 ? (const void*)bf16_fn : (const void*)f32_fn, bytes);
}

hipError_t tfc_launch_vit_attn_tiled_fwd(int dt, const float* qkv, float* out, float* stats, int N, int T, int H, float scale, hipStream_t st) {
  const size_t lds = sizeof(float) * (4 * 64 * AP + 2 * 64 * 3);
  const hipError_t e = attn_tiled_lds(&tfc_vit_attn_tiled_fwd_kernel<TFC_DT_BF16>, &tfc_vit_attn_tiled_fwd_kernel<TFC_DT_F32>, dt, lds);
  if (e != hipSuccess) return e;
  const dim3 grid((T + TQ - 1) / TQ, H, N);
  if (dt == TFC_DT_BF16) hipLaunchKernelGGL(tfc_vit_attn_tiled_fwd_kernel<TFC_DT_BF16>, grid, dim3(256), lds, st, qkv, out, stats, T, H, scale);
  else hipLaunchKernelGGL(tfc_vit_attn_tiled_fwd_kernel<TFC_DT_F32>, grid, dim3(256), lds, st, qkv, out, stats, T, H, scale);
  return hipGetLastError();
}

// ws: N * H * T floats (delta, written by the dQ kernel and read by the dK / dV kernel behind it on the stream)
hipError_t tfc_launch_vit_attn_tiled_bwd(int dt, const float* dout, const float* qkv, const float* stats, float* dqkv, float* ws, int N, int T, int H,
                                         float scale, hipStream_t st) {
  const size_t lq = sizeof(float) * (5 * 64 * AP + 4 * 64 + 2 * 64), lk = sizeof(float) * (6 * 64 * AP + 4 * 64 + 64);
  hipError_t e = attn_tiled_lds(&tfc_vit_attn_tiled_dq_kernel<TFC_DT_BF16>, &tfc_vit_attn_tiled_dq_kernel<TFC_DT_F32>, dt, lq);
  if (e != hipSuccess) return e;
  e = attn_tiled_lds(&tfc_vit_attn_tiled_dkv_kernel<TFC_DT_BF16>, &tfc_vit_attn_tiled_dkv_kernel<TFC_DT_F32>, dt, lk);
  if (e != hipSuccess) return e;
  const dim3 gq((T + TQ - 1) / TQ, H, N), gk((T + TK - 1) / TK, H, N);
  if (dt == TFC_DT_BF16) {
    hipLaunchKernelGGL(tfc_vit_attn_tiled_dq_kernel<TFC_DT_BF16>, gq, dim3(256), lq, st, dout, qkv, stats, dqkv, ws, T, H, scale);
    hipLaunchKernelGGL(tfc_vit_attn_tiled_dkv_kernel<TFC_DT_BF16>, gk, dim3(256), lk, st, dout, qkv, stats, (const float*)ws, dqkv, T, H, scale);
  } else {
    hipLaunchKernelGGL(tfc_vit_attn_tiled_dq_kernel<TFC_DT_F32>, gq, dim3(256), lq, st, dout, qkv, stats, dqkv, ws, T, H, scale);
    hipLaunchKernelGGL(tfc_vit_attn_tiled_dkv_kernel<TFC_DT_F32>, gk, dim3(256), lk, st, dout, qkv, stats, (const float*)ws, dqkv, T, H, scale);
  }
  return hipGetLastError();
}

hipError_t tfc_launch_vit_tokens_fwd(float* x, const float* cls, const float* pos, int N, int T, int D, hipStream_t st) {
  const long long tot = (long long)N * T * D;
  hipLaunchKernelGGL(tfc_vit_tokens_fwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x, cls, pos, N, T, D);
  return hipGetLastError();
}
