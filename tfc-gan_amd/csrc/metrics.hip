// Evaluation metrics on uint8 images (include/tfc_gan.h, "evaluation metrics"): PSNR, SSIM, colour-histogram Bhattacharyya distance, normalised
// cross-correlation and mutual information -- what the reference reads off saved PNGs with cv2 / scikit-image / numpy (TFC-GAN-FFT/eval/*/
// evaluation_psnr_ssim.py, evaluation_bhatt.py; TFC-STN/evaluation/calc_NCC.py, calc_MI.py).
//
// EXACT BY CONSTRUCTION: every sum over pixels is an INTEGER sum (64-bit moments, 32-bit window sums and histogram bins), so no summation order can
// change it; only the tiny fp64 finalisers round, and they add in a fixed order. No float atomics. The workgroups of one image and their partial
// slots depend on the image's size alone: a sample's result is the same bits in any batch, on every run.
#include "common.h"

#define TFC_MOM_SLOTS 10          // sum a, sum b, sum a^2, sum b^2, sum ab, sum (a-b)^2, min a, max a, min b, max b
#define TFC_MOM_CHUNK 65536       // bytes of one image per workgroup: 256 threads x 16 units of 16 bytes; 256 elements per thread keep every per-thread
                                  // sum below 256 * 65025 < 2^32, a wave's below 2^30
#define TFC_SSIM_TH 16            // SSIM output tile of a workgroup: 16 rows x 64 columns, 4 outputs per thread
#define TFC_SSIM_TW 64
#define TFC_SSIM_WMAX 7

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {        // butterfly: every lane ends with the same bits, the order is fixed by the lane map
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// fixed-order sum of one double per thread over a 256-thread workgroup; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* s4) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// ---- pair moments ------------------------------------------------------------------------------------------------------------------------------
// grid (G, N), G = ceil(count / TFC_MOM_CHUNK): workgroup g of pair n reduces bytes [g * CHUNK, (g + 1) * CHUNK) and leaves its 10 numbers in slot (n, g)
__global__ __launch_bounds__(256) void tfc_pair_moments_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long long a_stride,
                                                               long long b_stride, long long count, int vec, long long* __restrict__ part) {
  const int n = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const uint8_t* pa = a + (long long)n * a_stride;
  const uint8_t* pb = b + (long long)n * b_stride;
  unsigned sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0, mna = 255, mxa = 0, mnb = 255, mxb = 0;
  auto acc = [&](unsigned x, unsigned y) {
    sa += x; sb += y; saa += x * x; sbb += y * y; sab += x * y;
    mna = min(mna, x); mxa = max(mxa, x); mnb = min(mnb, y); mxb = max(mxb, y);
  };
  const long long base = (long long)g * TFC_MOM_CHUNK;
  for (int it = 0; it < TFC_MOM_CHUNK / (256 * 16); ++it) {
    const long long off = base + (long long)(it * 256 + tid) * 16;
    if (off >= count) break;
    if (vec && off + 16 <= count) {                               // 128-bit loads: the host checked that both bases and strides are 16-byte aligned
      const uint4 ua = *reinterpret_cast<const uint4*>(pa + off), ub = *reinterpret_cast<const uint4*>(pb + off);
      const unsigned wa[4] = {ua.x, ua.y, ua.z, ua.w}, wb[4] = {ub.x, ub.y, ub.z, ub.w};
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc((wa[w] >> (8 * k)) & 255u, (wb[w] >> (8 * k)) & 255u);
    } else {
      for (int k = 0; k < 16 && off + k < count; ++k) acc(pa[off + k], pb[off + k]);
    }
  }
  __shared__ unsigned long long s_sum[4][5];
  __shared__ unsigned s_mm[4][4];
  sa = wave_sum_u32(sa); sb = wave_sum_u32(sb); saa = wave_sum_u32(saa); sbb = wave_sum_u32(sbb); sab = wave_sum_u32(sab);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mna = min(mna, (unsigned)__shfl_xor(mna, o, 64)); mxa = max(mxa, (unsigned)__shfl_xor(mxa, o, 64));
    mnb = min(mnb, (unsigned)__shfl_xor(mnb, o, 64)); mxb = max(mxb, (unsigned)__shfl_xor(mxb, o, 64));
  }
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    s_sum[w][0] = sa; s_sum[w][1] = sb; s_sum[w][2] = saa; s_sum[w][3] = sbb; s_sum[w][4] = sab;
    s_mm[w][0] = mna; s_mm[w][1] = mxa; s_mm[w][2] = mnb; s_mm[w][3] = mxb;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long t[5];
    for (int i = 0; i < 5; ++i) t[i] = s_sum[0][i] + s_sum[1][i] + s_sum[2][i] + s_sum[3][i];
    long long* o = part + ((long long)n * gridDim.x + g) * TFC_MOM_SLOTS;
    o[0] = (long long)t[0]; o[1] = (long long)t[1]; o[2] = (long long)t[2]; o[3] = (long long)t[3]; o[4] = (long long)t[4];
    o[5] = (long long)(t[2] + t[3] - 2 * t[4]);                   // sum (a-b)^2 = sum a^2 + sum b^2 - 2 sum ab, exact in integers
    o[6] = min(min(s_mm[0][0], s_mm[1][0]), min(s_mm[2][0], s_mm[3][0]));
    o[7] = max(max(s_mm[0][1], s_mm[1][1]), max(s_mm[2][1], s_mm[3][1]));
    o[8] = min(min(s_mm[0][2], s_mm[1][2]), min(s_mm[2][2], s_mm[3][2]));
    o[9] = max(max(s_mm[0][3], s_mm[1][3]), max(s_mm[2][3], s_mm[3][3]));
  }
}

// one wave per pair: adds the G slots, writes the moments and the two metrics that need nothing else.
//   PSNR (evaluation_psnr_ssim.py:56-64): mse == 0 -> 100, else 20 log10(255 / sqrt(mse)), mse = sum (a-b)^2 / count.
//   NCC (calc_NCC.py:44-64): (1 / (n-1)) sum norm(a) norm(b) with norm = (x - mean) / std(ddof=1) = Pearson's r; in integers
//   r = (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)) -- the /255 of ToTensor cancels, a constant image gives 0 / 0 = NaN as the script's does.
__global__ __launch_bounds__(64) void tfc_pair_moments_finish_kernel(const long long* __restrict__ part, int G, long long count, long long* __restrict__ mom,
                                                                     double* __restrict__ psnr, double* __restrict__ ncc) {
  const int n = blockIdx.x, lane = threadIdx.x;
  long long s[6] = {0, 0, 0, 0, 0, 0};
  int mna = 255, mxa = 0, mnb = 255, mxb = 0;
  for (int g = lane; g < G; g += 64) {
    const long long* p = part + ((long long)n * G + g) * TFC_MOM_SLOTS;
    for (int i = 0; i < 6; ++i) s[i] += p[i];
    mna = min(mna, (int)p[6]); mxa = max(mxa, (int)p[7]); mnb = min(mnb, (int)p[8]); mxb = max(mxb, (int)p[9]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    for (int i = 0; i < 6; ++i) s[i] += __shfl_xor(s[i], o, 64);
    mna = min(mna, __shfl_xor(mna, o, 64)); mxa = max(mxa, __shfl_xor(mxa, o, 64));
    mnb = min(mnb, __shfl_xor(mnb, o, 64)); mxb = max(mxb, __shfl_xor(mxb, o, 64));
  }
  if (lane != 0) return;
  long long* o = mom + (long long)n * TFC_MOM_SLOTS;
  for (int i = 0; i < 6; ++i) o[i] = s[i];
  o[6] = mna; o[7] = mxa; o[8] = mnb; o[9] = mxb;
  if (psnr) {
    const double mse = (double)s[5] / (double)count;
    psnr[n] = s[5] == 0 ? 100.0 : 20.0 * log10(255.0 / sqrt(mse));
  }
  if (ncc) {                                                      // count <= 2^23 (checked by the entry point): every product below fits 63 bits
    const long long num = count * s[4] - s[0] * s[1], va = count * s[2] - s[0] * s[0], vb = count * s[3] - s[1] * s[1];
    ncc[n] = (double)num / sqrt((double)va * (double)vb);
  }
}

// ---- SSIM --------------------------------------------------------------------------------------------------------------------------------------
// skimage.metrics.structural_similarity for uint8 input (win 7, K1 0.01, K2 0.03, sample covariance): the mean of the SSIM map over the region whose
// windows lie inside the image, so no border mode exists. Output pixel (oy, ox), oy < H - wy + 1, ox < W - wx + 1, owns the window of input rows
// [oy, oy + wy) and columns [ox, ox + wx). A workgroup stages its tile plus the window overhang in LDS, forms the five horizontal window sums per row
// and column (integers), adds wy of them down each column as a running sum, evaluates the formula in fp64 and leaves ONE partial in slot (n, tile).
__global__ __launch_bounds__(256) void tfc_ssim_kernel(const uint8_t* __restrict__ a, long long a_is, int a_rs, const uint8_t* __restrict__ b, long long b_is,
                                                       int b_rs, int H, int W, int wy, int wx, double c1, double c2, double* __restrict__ part) {
  constexpr int TH = TFC_SSIM_TH, TW = TFC_SSIM_TW, RH = TH + TFC_SSIM_WMAX - 1, RW = TW + TFC_SSIM_WMAX - 1;
  __shared__ uint8_t s_a[RH][RW + 2], s_b[RH][RW + 2];
  __shared__ int s_h[5][RH][TW];
  __shared__ double s_red[4];
  const int n = blockIdx.z, tid = threadIdx.x;
  const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
  const int rows = TH + wy - 1, cols = TW + wx - 1;
  const uint8_t* pa = a + (long long)n * a_is;
  const uint8_t* pb = b + (long long)n * b_is;
  for (int i = tid; i < rows * cols; i += 256) {
    const int r = i / cols, c = i - r * cols, y = oy0 + r, x = ox0 + c;
    const bool in = y < H && x < W;                               // outside the image: zeros that only masked-out outputs read
    s_a[r][c] = in ? pa[(long long)y * a_rs + x] : 0;
    s_b[r][c] = in ? pb[(long long)y * b_rs + x] : 0;
  }
  __syncthreads();
  for (int i = tid; i < rows * TW; i += 256) {
    const int r = i / TW, c = i - r * TW;
    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int k = 0; k < wx; ++k) {
      const int x = s_a[r][c + k], y = s_b[r][c + k];
      sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
    }
    s_h[0][r][c] = sx; s_h[1][r][c] = sy; s_h[2][r][c] = sxx; s_h[3][r][c] = syy; s_h[4][r][c] = sxy;
  }
  __syncthreads();
  const int c = tid & (TW - 1), r0 = (tid >> 6) * (TH / 4);       // a wave owns 4 output rows of the tile, a thread one column of them
  int run[5];
  for (int q = 0; q < 5; ++q) {
    run[q] = 0;
    for (int k = 0; k < wy; ++k) run[q] += s_h[q][r0 + k][c];
  }
  const double np = (double)(wx * wy), cov_norm = np / (np - 1.0);
  double acc = 0.0;
  for (int j = 0; j < TH / 4; ++j) {
    const int r = r0 + j;
    if (j > 0)
      for (int q = 0; q < 5; ++q) run[q] += s_h[q][r + wy - 1][c] - s_h[q][r - 1][c];
    if (oy0 + r < H - wy + 1 && ox0 + c < W - wx + 1) {
      const double ux = (double)run[0] / np, uy = (double)run[1] / np, uxx = (double)run[2] / np, uyy = (double)run[3] / np, uxy = (double)run[4] / np;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
      acc += (a1 * a2) / (b1 * b2);
    }
  }
  const double tot = block_sum_f64(acc, s_red);
  if (tid == 0) part[((long long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

// out[n] = (sum of the image's tile partials, thread-strided then the fixed tree) / outputs
__global__ __launch_bounds__(256) void tfc_ssim_finish_kernel(const double* __restrict__ part, int tiles, double outputs, double* __restrict__ out) {
  __shared__ double s_red[4];
  const int n = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 256) acc += part[(long long)n * tiles + t];
  const double tot = block_sum_f64(acc, s_red);
  if (threadIdx.x == 0) out[n] = tot / outputs;
}

// ---- histograms --------------------------------------------------------------------------------------------------------------------------------
// (a) colour histogram of evaluation_bhatt.py:55 (cv2.calcHist, 8 x 8 x 8 bins over [0, 256)): bin (c0 >> 5, c1 >> 5, c2 >> 5). Integer atomics only:
// LDS bins per workgroup, flushed into the (zeroed) global bins -- integer addition commutes, the result does not depend on the order.
#define TFC_HIST_PIX 16384        // pixels of one image per workgroup
__global__ __launch_bounds__(256) void tfc_hist_color_kernel(const uint8_t* __restrict__ img, long long img_stride, long long pix_stride, long long chan_stride,
                                                             long long npix, unsigned* __restrict__ hist) {
  __shared__ unsigned s_h[512];
  const int n = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < 512; i += 256) s_h[i] = 0;
  __syncthreads();
  const uint8_t* p = img + (long long)n * img_stride;
  const long long base = (long long)blockIdx.x * TFC_HIST_PIX;
  for (int it = 0; it < TFC_HIST_PIX / 256; ++it) {
    const long long px = base + it * 256 + tid;
    if (px >= npix) break;
    const uint8_t* q = p + px * pix_stride;
    const unsigned c0 = q[0], c1 = q[chan_stride], c2 = q[2 * chan_stride];
    atomicAdd(&s_h[((c0 >> 5) * 8 + (c1 >> 5)) * 8 + (c2 >> 5)], 1u);
  }
  __syncthreads();
  for (int i = tid; i < 512; i += 256)
    if (s_h[i]) atomicAdd(&hist[(long long)n * 512 + i], s_h[i]);
}

// (b) joint histogram of two gray images through per-image look-up tables gray level -> bin: hist[n][lut_a[a]][lut_b[b]], nb <= 32
__global__ __launch_bounds__(256) void tfc_hist_joint_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long long a_stride, long long b_stride,
                                                             long long count, const uint8_t* __restrict__ lut_a, const uint8_t* __restrict__ lut_b, int nb,
                                                             unsigned* __restrict__ hist) {
  __shared__ unsigned s_h[32 * 32];
  __shared__ uint8_t s_la[256], s_lb[256];
  const int n = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < nb * nb; i += 256) s_h[i] = 0;
  s_la[tid] = lut_a[(long long)n * 256 + tid];
  s_lb[tid] = lut_b[(long long)n * 256 + tid];
  __syncthreads();
  const uint8_t* pa = a + (long long)n * a_stride;
  const uint8_t* pb = b + (long long)n * b_stride;
  const long long base = (long long)blockIdx.x * TFC_HIST_PIX;
  for (int it = 0; it < TFC_HIST_PIX / 256; ++it) {
    const long long px = base + it * 256 + tid;
    if (px >= count) break;
    atomicAdd(&s_h[s_la[pa[px]] * nb + s_lb[pb[px]]], 1u);
  }
  __syncthreads();
  for (int i = tid; i < nb * nb; i += 256)
    if (s_h[i]) atomicAdd(&hist[(long long)n * nb * nb + i], s_h[i]);
}

// Bin tables of np.histogram2d(a / 255, b / 255, bins = nb) on float32 pixels (calc_MI.py:59; ToTensor's x / 255 in float32), from the min / max the
// moments kernel found. numpy: edges = linspace(min, max, nb + 1) = arange(nb + 1) * ((max - min) / nb) + min with the last edge set to max, the
// range widened to (min - 0.5, max + 0.5) when min == max; bin = (number of edges <= x) - 1, right-open except the last. edge_f32 == 0: the edges
// are float64 (numpy 1.x, where float32 scalars promote against Python floats by value: the reference's era); 1: float32 (numpy >= 2, NEP 50).
// One multiply, one add, each rounded on its own: contracted into an fma an edge moves by an ulp and a pixel crosses it. hipcc contracts by default,
// and through __dmul_rn / __dadd_rn too (plain operators in its headers), so the arithmetic of this kernel is spelled out under contract(off).
#pragma clang fp contract(off)
__device__ __forceinline__ double tfc_edge_f64(int j, int nb, double lo, double hi, double step) {
  const double p = (double)j * step;
  return j == nb ? hi : p + lo;
}
__device__ __forceinline__ float tfc_edge_f32(int j, int nb, float lo, float hi, float step) {
  const float p = (float)j * step;
  return j == nb ? hi : p + lo;
}
__global__ __launch_bounds__(256) void tfc_mi_lut_kernel(const long long* __restrict__ mom, int nb, int edge_f32, uint8_t* __restrict__ lut_a,
                                                         uint8_t* __restrict__ lut_b) {
  const int n = blockIdx.x, which = blockIdx.y, g = threadIdx.x;
  const long long* m = mom + (long long)n * TFC_MOM_SLOTS + 6 + 2 * which;
  const float x = __fdiv_rn((float)g, 255.0f), fmn = __fdiv_rn((float)m[0], 255.0f), fmx = __fdiv_rn((float)m[1], 255.0f);
  int idx = 0;
  if (edge_f32) {
    float lo = fmn, hi = fmx;
    if (lo == hi) { lo = lo - 0.5f; hi = hi + 0.5f; }
    const float step = __fdiv_rn(hi - lo, (float)nb);
    for (int j = 0; j <= nb; ++j) idx += tfc_edge_f32(j, nb, lo, hi, step) <= x;
    if (x == hi) idx -= 1;
  } else {
    double lo = fmn, hi = fmx;
    if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
    const double step = (hi - lo) / (double)nb;
    for (int j = 0; j <= nb; ++j) idx += tfc_edge_f64(j, nb, lo, hi, step) <= (double)x;
    if ((double)x == hi) idx -= 1;
  }
  (which ? lut_b : lut_a)[(long long)n * 256 + g] = (uint8_t)min(max(idx - 1, 0), nb - 1);   // levels outside [min, max] do not occur in the image
}
#pragma clang fp contract(fast)

// ---- finalisers ----------------------------------------------------------------------------------------------------------------------------------
// cv2.compareHist(HISTCMP_BHATTACHARYYA) (evaluation_bhatt.py:55-61): sqrt(max(1 - sum sqrt(h1 h2) / sqrt(sum h1 * sum h2), 0)). The script L2-normalises
// both histograms first (cv2.normalize) and swaps BGR <-> RGB in both images: a common scale of h1 (and of h2) divides out of the ratio, and the
// swap permutes the bins of both histograms alike, so both cancel algebraically and the raw counts in file order give the same number.
__global__ __launch_bounds__(256) void tfc_bhattacharyya_kernel(const unsigned* __restrict__ h1, const unsigned* __restrict__ h2, int nbins, double* __restrict__ out) {
  __shared__ double s_red[4];
  __shared__ unsigned long long s_cnt[2][4];
  const int n = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  unsigned t1 = 0, t2 = 0;
  for (int i = tid; i < nbins; i += 256) {
    const unsigned x = h1[(long long)n * nbins + i], y = h2[(long long)n * nbins + i];
    t1 += x; t2 += y;
    acc += sqrt((double)((unsigned long long)x * y));
  }
  t1 = wave_sum_u32(t1); t2 = wave_sum_u32(t2);
  if ((tid & 63) == 0) { s_cnt[0][tid >> 6] = t1; s_cnt[1][tid >> 6] = t2; }
  const double bc = block_sum_f64(acc, s_red);                    // (its barrier also publishes s_cnt)
  if (tid == 0) {
    const unsigned long long n1 = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3], n2 = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
    out[n] = sqrt(fmax(1.0 - bc / sqrt((double)n1 * (double)n2), 0.0));
  }
}

// calc_MI.py:72-82: sum over the non-zero cells of pxy log(pxy / (px py)), pxy = h / sum h. The marginals are integer row / column sums.
__global__ __launch_bounds__(64) void tfc_mutual_information_kernel(const unsigned* __restrict__ hist, int nb, double* __restrict__ out) {
  __shared__ unsigned s_row[32], s_col[32];
  const int n = blockIdx.x, lane = threadIdx.x;
  const unsigned* h = hist + (long long)n * nb * nb;
  if (lane < nb) {
    unsigned r = 0, c = 0;
    for (int k = 0; k < nb; ++k) { r += h[lane * nb + k]; c += h[k * nb + lane]; }
    s_row[lane] = r; s_col[lane] = c;
  }
  __syncthreads();
  unsigned long long total = 0;
  for (int k = 0; k < nb; ++k) total += s_row[k];
  const double tot = (double)total;
  double acc = 0.0;
  for (int i = lane; i < nb * nb; i += 64) {
    const unsigned v = h[i];
    if (v) {
      const double pxy = (double)v / tot, px = (double)s_row[i / nb] / tot, py = (double)s_col[i % nb] / tot;
      acc += pxy * log(pxy / (px * py));
    }
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) out[n] = acc;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------
int tfc_moments_groups(long long count) { return (int)((count + TFC_MOM_CHUNK - 1) / TFC_MOM_CHUNK); }
void tfc_ssim_tiles(int H, int W, int wy, int wx, int* tx, int* ty) {
  *tx = (W - wx + 1 + TFC_SSIM_TW - 1) / TFC_SSIM_TW;
  *ty = (H - wy + 1 + TFC_SSIM_TH - 1) / TFC_SSIM_TH;
}
hipError_t tfc_launch_pair_moments(const uint8_t* a, const uint8_t* b, long long a_stride, long long b_stride, long long count, int N, long long* ws,
                                   long long* mom, double* psnr, double* ncc, hipStream_t st) {
  const int G = tfc_moments_groups(count);
  const int vec = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)a_stride | (uintptr_t)b_stride) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(tfc_pair_moments_kernel, dim3(G, N), dim3(256), 0, st, a, b, a_stride, b_stride, count, vec, ws);
  hipLaunchKernelGGL(tfc_pair_moments_finish_kernel, dim3(N), dim3(64), 0, st, (const long long*)ws, G, count, mom, psnr, ncc);
  return hipGetLastError();
}
hipError_t tfc_launch_ssim(const uint8_t* a, long long a_is, int a_rs, const uint8_t* b, long long b_is, int b_rs, int N, int H, int W, int wy, int wx,
                           double data_range, double* ws, double* out, hipStream_t st) {
  int tx, ty;
  tfc_ssim_tiles(H, W, wy, wx, &tx, &ty);
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  hipLaunchKernelGGL(tfc_ssim_kernel, dim3(tx, ty, N), dim3(256), 0, st, a, a_is, a_rs, b, b_is, b_rs, H, W, wy, wx, c1, c2, ws);
  hipLaunchKernelGGL(tfc_ssim_finish_kernel, dim3(N), dim3(256), 0, st, (const double*)ws, tx * ty, (double)(H - wy + 1) * (double)(W - wx + 1), out);
  return hipGetLastError();
}
hipError_t tfc_launch_hist_color(const uint8_t* img, long long img_stride, long long pix_stride, long long chan_stride, long long npix, int N, unsigned* hist,
                                 hipStream_t st) {
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * 512 * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tfc_hist_color_kernel, dim3((unsigned)((npix + TFC_HIST_PIX - 1) / TFC_HIST_PIX), N), dim3(256), 0, st, img, img_stride, pix_stride,
                     chan_stride, npix, hist);
  return hipGetLastError();
}
hipError_t tfc_launch_hist_joint(const uint8_t* a, const uint8_t* b, long long a_stride, long long b_stride, long long count, int N, const uint8_t* lut_a,
                                 const uint8_t* lut_b, int nb, unsigned* hist, hipStream_t st) {
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * nb * nb * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tfc_hist_joint_kernel, dim3((unsigned)((count + TFC_HIST_PIX - 1) / TFC_HIST_PIX), N), dim3(256), 0, st, a, b, a_stride, b_stride, count,
                     lut_a, lut_b, nb, hist);
  return hipGetLastError();
}
hipError_t tfc_launch_mi_lut(const long long* mom, int N, int nb, int edge_f32, uint8_t* lut_a, uint8_t* lut_b, hipStream_t st) {
  hipLaunchKernelGGL(tfc_mi_lut_kernel, dim3(N, 2), dim3(256), 0, st, mom, nb, edge_f32, lut_a, lut_b);
  return hipGetLastError();
}
hipError_t tfc_launch_bhattacharyya(const unsigned* h1, const unsigned* h2, int N, int nbins, double* out, hipStream_t st) {
  hipLaunchKernelGGL(tfc_bhattacharyya_kernel, dim3(N), dim3(256), 0, st, h1, h2, nbins, out);
  return hipGetLastError();
}
hipError_t tfc_launch_mutual_information(const unsigned* hist, int N, int nb, double* out, hipStream_t st) {
  hipLaunchKernelGGL(tfc_mutual_information_kernel, dim3(N), dim3(64), 0, st, hist, nb, out);
  return hipGetLastError();
}
