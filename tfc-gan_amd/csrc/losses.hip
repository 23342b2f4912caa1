// Loss heads of the PATCH-16 training step (gfx950).
//   triplet   : the 16-patch "contrastive" head  (reference TFCGAN_multigpu_patchFFT_16P.py:75, :558-583) and its 4-patch form
//   spectrum  : ToPILImage -> convert("L") -> np.fft.rfft2 -> fftshift -> |.|, atan2  (reference :271-319)
//   l1 mean   : nn.L1Loss over amplitude / phase arrays (reference :323-375)
#include "common.h"

// ---------------------------------------------------------------------------------------------------
// Patch triplet on a GRID x GRID grid of P x P patches, P = 256 / GRID: GRID = 4 is the 16-patch head of PATCH-16 (make_16_patches, reference :227-253),
// GRID = 2 the 4-patch head of PATCH-4 / GLO-4 (reference TFCGAN_multigpu_patchFFT.py:468-481).  Patch k (0-based) = rows P*(k/GRID).., cols P*(k%GRID)..
// (first flat NCHW index of patch k = P*(k%GRID) + 256*P*(k/GRID)).  F.triplet_margin_loss(margin 1, p 2, eps 1e-6):
//   d(x,y) = || x - y + eps ||_2 over the LAST dim (one P-pixel patch row); loss_k = mean_{n,c,row} max(1 + d_ap - d_an, 0)
//   total = (1/GRID^2) sum_k loss_k.  One wave per patch row, P / 64 adjacent pixels per lane (one 8-byte access at GRID = 2), wave-shuffle reductions.
//   Row id = ((n*C + c)*256 + y)*GRID + kx.
// grad wrt anchor (fake):  [hinge>0] * ((a-p+eps)/d_ap - (a-n+eps)/d_an) * factor.  The factor is rounded as each head has always rounded it
// (tfc_launch_patch_triplet): the 16-patch head multiplies by coef = 1 / (16 N C 64) and then by gscale; the 4-patch head multiplies ONCE, by
// coef = gscale / (4 N C 128) rounded on the host, so that a sample's gradient at batch N with gscale = N is the same bits as that sample alone with
// gscale = 1 (everything else in a row's arithmetic is per sample); its kernel does not read gscale.
// A slot per grid: the 4-patch head may run beside a 16-patch call of another stream.
// ---------------------------------------------------------------------------------------------------
template <int GRID> struct NegIdx { int r[GRID * GRID]; };
static __device__ TfcRedSlot g_trip_slot, g_trip4_slot, g_l1_slot;

// sum of squares of a lane's pixels, in the expression shapes the two grids have always had (device code contracts a*b + c*d into one fma)
template <int PPL> __device__ __forceinline__ float tfc_sq_sum(const float* d) {
  if constexpr (PPL == 1) return d[0] * d[0];
  else return d[0] * d[0] + d[1] * d[1];
}

// a lane's PPL adjacent pixels: one float, or one float2 (a single 8-byte access)
template <int PPL> struct TfcPix;
template <> struct TfcPix<1> { float v; __device__ __forceinline__ float& operator[](int) { return v; } };
template <> struct TfcPix<2> { float2 v; __device__ __forceinline__ float& operator[](int i) { return i ? v.y : v.x; } };

template <int GRID>
__global__ void __launch_bounds__(256)
tfc_patch_triplet_kernel(const float* __restrict__ fake, const float* __restrict__ real, const NegIdx<GRID> neg, int N, int C,
                         float margin, float eps, float* loss, float* dfake, float coef, float gscale) {
  static_assert(GRID == 2 || GRID == 4, "2 x 2 patches of 128 pixels or 4 x 4 patches of 64");
  constexpr int LG = GRID == 4 ? 2 : 1, P = 256 / GRID, PPL = P / 64;          // log2 GRID, patch side, pixels per lane
  typedef TfcPix<PPL> vec_t;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const long long nrows = (long long)N * C * 256 * GRID;
  float lsum = 0.f;
  // four rows per iteration: their loads are issued together (one dependent load -> reduce -> store chain per row leaves the
  // memory pipeline idle most of the time)
  constexpr int R = 4;
  const long long stride = (long long)gridDim.x * 4;
  for (long long row0 = (long long)blockIdx.x * 4 + w; row0 < nrows; row0 += stride * R) {
    vec_t a[R], p[R], ng[R];
    size_t ia[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * stride;
      ok[r] = row < nrows;
      const long long rw = ok[r] ? row : row0;
      const int kx = (int)(rw & (GRID - 1));
      const long long r2 = rw >> LG;
      const int y = (int)(r2 & 255);
      const long long nc = r2 >> 8;                              // n*C + c
      const int k = (y / P) * GRID + kx;
      const int rk = neg.r[k];
      const size_t plane = (size_t)nc * 65536;
      ia[r] = plane + (size_t)y * 256 + kx * P + PPL * lane;
      const size_t in_ = plane + (size_t)((rk >> LG) * P + (y & (P - 1))) * 256 + (rk & (GRID - 1)) * P + PPL * lane;
      a[r] = *reinterpret_cast<const vec_t*>(fake + ia[r]);
      p[r] = *reinterpret_cast<const vec_t*>(real + ia[r]);
      ng[r] = *reinterpret_cast<const vec_t*>(real + in_);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!ok[r]) continue;                                      // wave-uniform
      float dp[PPL], dn[PPL];
#pragma unroll
      for (int i = 0; i < PPL; ++i) { dp[i] = a[r][i] - p[r][i] + eps; dn[i] = a[r][i] - ng[r][i] + eps; }
      const float sp = wave_sum(tfc_sq_sum<PPL>(dp)), sn = wave_sum(tfc_sq_sum<PPL>(dn));
      const float dap = sqrtf(sp), dan = sqrtf(sn);
      const float hinge = margin + dap - dan;
      vec_t g = {};
      if (hinge > 0.f) {
        lsum += hinge;                                           // identical on all lanes
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
          g[i] = ((dap > 0.f ? dp[i] / dap : 0.f) - (dan > 0.f ? dn[i] / dan : 0.f)) * coef;
          if constexpr (GRID == 4) g[i] *= gscale;
        }
      }
      if (dfake) *reinterpret_cast<vec_t*>(dfake + ia[r]) = g;
    }
  }
  const double tot = tfc_block_sum4(lsum, red);
  if (threadIdx.x == 0) tfc_block_commit(GRID == 4 ? &g_trip_slot : &g_trip4_slot, tot / ((double)(GRID * GRID) * N * C * (double)P), loss, true);
}

// ---------------------------------------------------------------------------------------------------
// Spectrum of an S x S window of an NCHW fp32 image in [-1,1]:
//   u8 = (uint8) trunc(x*255)  (wraps mod 256 exactly like tensor.mul(255).byte());  L = (19595 R + 38470 G + 7471 B + 32768) >> 16
//   F = rfft2(L)  (S x (S/2+1)),  amp = |F|, pha = atan2(Im, Re); optional fftshift of both axes on store.
// Direct DFT in LDS with an exact sincospi twiddle table: rows (real input) then columns. A workgroup owns one window
// and a group of KG output columns, so S=256 (GLO-16) fits LDS as well as S=64 (PATCH-16) and S=128 (PATCH-4).
// The four self-conjugate bins have Im forced to +0 (numpy's pocketfft yields exact zeros there).
// The windows lie on a TfcWinGrid (tfc_desc.h); the luma and the window origin are shared with the FFT row pass below.
// ---------------------------------------------------------------------------------------------------
// first pixel (channel 0) of window w
__device__ __forceinline__ const float* tfc_window_origin(const float* img, const TfcWinGrid& g, int w) {
  const int n = w / g.wins_per_img, kw = w % g.wins_per_img;
  return img + (size_t)n * g.bs + (size_t)(g.row0 + (kw / g.wins_x) * g.row_step) * g.rs + (kw % g.wins_x) * g.col_step;
}
// uint8 luma of the pixel whose channel-0 value is px[0] (channel stride cs; C = 1: the one channel three times)
__device__ __forceinline__ int tfc_luma_u8(const float* px, long long cs, int C) {
  int q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = px[(size_t)(C == 1 ? 0 : c) * cs] * 255.f;
    q[c] = ((int)v) & 255;
  }
  return (19595 * q[0] + 38470 * q[1] + 7471 * q[2] + 32768) >> 16;
}

template <int S, int KG>
__global__ void __launch_bounds__(256)
tfc_spectrum_kernel(const float* __restrict__ img, const TfcWinGrid g, float* __restrict__ amp, float* __restrict__ pha, int shift) {
  constexpr int NB = S / 2 + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* lum = smem;                                     // S*S bytes
  float* tw = reinterpret_cast<float*>(smem + S * S);            // 2*S floats (cos, sin)
  float* R = tw + 2 * S;                                         // S*KG*2 floats
  const int w = blockIdx.x;
  const int kx0 = blockIdx.y * KG;
  const float* base = tfc_window_origin(img, g, w);
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int y = i / S, x = i % S;
    lum[i] = (unsigned char)tfc_luma_u8(base + (size_t)y * g.rs + x, g.cs, g.C);
  }
  for (int i = threadIdx.x; i < S; i += 256) {
    float sn, cn;
    sincospif(2.f * (float)i / (float)S, &sn, &cn);
    tw[2 * i] = cn; tw[2 * i + 1] = sn;
  }
  __syncthreads();
  // rows: R[y][kk] = sum_x L[y][x] * exp(-2 pi i x kx / S)
  for (int o = threadIdx.x; o < S * KG; o += 256) {
    const int y = o / KG, kk = o % KG, kx = kx0 + kk;
    float re = 0.f, im = 0.f;
    if (kx < NB) {
      for (int x = 0; x < S; ++x) {
        const int t = (x * kx) & (S - 1);
        const float v = (float)lum[y * S + x];
        re += v * tw[2 * t];
        im -= v * tw[2 * t + 1];
      }
    }
    R[2 * o] = re; R[2 * o + 1] = im;
  }
  __syncthreads();
  // columns: F[ky][kx] = sum_y R[y][kx] * exp(-2 pi i y ky / S)
  for (int o = threadIdx.x; o < S * KG; o += 256) {
    const int ky = o / KG, kk = o % KG, kx = kx0 + kk;
    if (kx >= NB) continue;
    float re = 0.f, im = 0.f;
    for (int y = 0; y < S; ++y) {
      const int t = (y * ky) & (S - 1);
      const float c = tw[2 * t], s = tw[2 * t + 1];
      const float rr = R[2 * (y * KG + kk)], ri = R[2 * (y * KG + kk) + 1];
      re += rr * c + ri * s;                                     // (rr + i ri) * (c - i s)
      im += ri * c - rr * s;
    }
    if ((kx == 0 || kx == S / 2) && (ky == 0 || ky == S / 2)) im = 0.f;
    int oy = ky, ox = kx;
    if (shift) { oy = (ky + S / 2) % S; ox = (kx + NB / 2) % NB; }
    const size_t oi = ((size_t)w * S + oy) * NB + ox;
    amp[oi] = sqrtf(re * re + im * im);
    pha[oi] = atan2f(im, re);
  }
}

// out[0] += scale * sum |a - b|
__global__ void __launch_bounds__(256)
tfc_l1_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, float scale, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += fabsf(a[i] - b[i]);
  const double tot = tfc_block_sum4(wave_sum(s), red);
  if (threadIdx.x == 0) tfc_block_commit(&g_l1_slot, tot * (double)scale, out);
}

// Full-spectrum log-magnitude MSE of the evaluation scripts (Devcom_MagMSE.py:91-118: mean_squared_error(log|fftshift(fft2(a))|,
// log|fftshift(fft2(b))|)) from the HALF spectra amp_a / amp_b [W][S][S/2+1]: |F[ky][kx]| = |F[-ky][-kx]| for real input, so the columns
// 1..S/2-1 count twice and columns 0 and S/2 once. out[w] += sum / S^2. One workgroup per (window, row block).
template <bool ABS>
__global__ void __launch_bounds__(256)
tfc_logmag_err_kernel(const float* __restrict__ a, const float* __restrict__ b, int S, float* out) {
  __shared__ float red[4];
  const int NB = S / 2 + 1;
  const int w = blockIdx.x;                                       // one workgroup per window, fixed summation order: no atomics, no memset
  const size_t base = (size_t)w * S * NB;
  float acc = 0.f;
  for (int i = threadIdx.x; i < S * NB; i += 256) {
    const int kx = i % NB;
    const float d = logf(a[base + i]) - logf(b[base + i]);
    acc += ((kx == 0 || kx == S / 2) ? 1.f : 2.f) * (ABS ? fabsf(d) : d * d);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[w] = (((red[0] + red[1]) + red[2]) + red[3]) / ((float)S * (float)S);
}
hipError_t tfc_launch_logmag_mse(const float* a, const float* b, int S, int nwin, float* out, int absolute, hipStream_t st) {
  if (absolute) hipLaunchKernelGGL(tfc_logmag_err_kernel<true>, dim3(nwin), dim3(256), 0, st, a, b, S, out);
  else hipLaunchKernelGGL(tfc_logmag_err_kernel<false>, dim3(nwin), dim3(256), 0, st, a, b, S, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Temperature head (reference :255-268 vectorize_temps + datasets_temp.py:14-35 TempVector_PyTorch, loss :587-595).
//   vectorize : red channel of ToPILImage(x) = (uint8) trunc(x*255) (wraps mod 256) -> lut[u8]  (lut = float32(np.linspace(24,38,256)))
//   row triplet: F.triplet_margin_loss on [N,1,H,W] tensors: d(x,y) = ||x - y + eps||_2 over the last dim (one image row),
//                loss = mean_rows max(margin + d(a,p) - d(a,n), 0).  One wave per row.  No gradient (the reference detaches via PIL).
// ---------------------------------------------------------------------------------------------------
static __device__ TfcRedSlot g_rowtrip_slot;

__global__ void __launch_bounds__(256)
tfc_vectorize_temps_kernel(const float* __restrict__ x, long long bs, int rs, int H, int W, long long total,
                           const float* __restrict__ lut, float* __restrict__ out) {
  __shared__ float sl[256];
  sl[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int xw = (int)(i % W);
    const long long r = i / W;
    const int y = (int)(r % H);
    const long long n = r / H;
    const float v = x[(size_t)n * bs + (size_t)y * rs + xw] * 255.f;
    out[i] = sl[((int)v) & 255];
  }
}

__global__ void __launch_bounds__(256)
tfc_row_triplet_kernel(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ ng, long long rows, int W,
                       float margin, float eps, float* loss) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  float lsum = 0.f;
  for (long long row = (long long)blockIdx.x * 4 + w; row < rows; row += (long long)gridDim.x * 4) {
    const size_t o = (size_t)row * W;
    float sp = 0.f, sn = 0.f;
    for (int xw = lane; xw < W; xw += 64) {
      const float av = a[o + xw];
      const float dp = av - p[o + xw] + eps, dn = av - ng[o + xw] + eps;
      sp += dp * dp; sn += dn * dn;
    }
    sp = wave_sum(sp); sn = wave_sum(sn);
    const float hinge = margin + sqrtf(sp) - sqrtf(sn);
    if (hinge > 0.f) lsum += hinge;
  }
  const double tot = tfc_block_sum4(lsum, red);
  if (threadIdx.x == 0) tfc_block_commit(&g_rowtrip_slot, tot / (double)rows, loss, true);
}
hipError_t tfc_launch_vectorize_temps(const float* x, long long bs, int rs, int N, int H, int W, const float* lut, float* out, hipStream_t st) {
  const long long total = (long long)N * H * W;
  long long nb = (total + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(tfc_vectorize_temps_kernel, dim3((int)nb), dim3(256), 0, st, x, bs, rs, H, W, total, lut, out);
  return hipGetLastError();
}
hipError_t tfc_launch_row_triplet(const float* a, const float* p, const float* ng, long long rows, int W, float margin, float eps,
                                  float* loss, hipStream_t st) {
  long long nb = (rows + 3) / 4;                                  // the last workgroup to arrive STORES the mean (tfc_block_commit set): no memset launch
  if (nb > 512) nb = 512;
  hipLaunchKernelGGL(tfc_row_triplet_kernel, dim3((int)nb), dim3(256), 0, st, a, p, ng, rows, W, margin, eps, loss);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
template <int GRID>
static void launch_patch_triplet(const float* fake, const float* real, const int* neg_idx, int N, int C, float margin, float eps, float* loss, float* dfake,
                                 float coef, float gscale, hipStream_t st) {
  NegIdx<GRID> ni;
  for (int i = 0; i < GRID * GRID; ++i) ni.r[i] = neg_idx[i];
  long long nb = ((long long)N * C * 256 * GRID + 3) / 4;        // rows / 4
  if (nb > 512) nb = 512;                                        // one double atomic + one ticket per workgroup on a single address
  hipLaunchKernelGGL(tfc_patch_triplet_kernel<GRID>, dim3((int)nb), dim3(256), 0, st, fake, real, ni, N, C, margin, eps, loss, dfake, coef, gscale);
}
hipError_t tfc_launch_patch_triplet(int grid, const float* fake, const float* real, const int* neg_idx, int N, int C, float margin, float eps,
                                    float* loss, float* dfake, float gscale, hipStream_t st) {
  // the gradient's factor: see the kernel's header
  if (grid == 4) launch_patch_triplet<4>(fake, real, neg_idx, N, C, margin, eps, loss, dfake, 1.f / (16.f * (float)N * (float)C * 64.f), gscale, st);
  else launch_patch_triplet<2>(fake, real, neg_idx, N, C, margin, eps, loss, dfake, (float)((double)gscale / (4.0 * N * C * 128.0)), gscale, st);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// The same spectra by FFT (S = 64 or 256 = 4^3 / 4^4, or S = 128 = 4^3 * 2 for the 2x2 patch grid of PATCH-4): radix-4 Stockham autosort passes
// in LDS (at S = 128 followed by one radix-2 pass), no bit reversal, exact sincospi twiddle table.
// The direct DFT above costs S^2 MACs per output row; at S = 256 (GLO-16, G16:294-313) that was 1.04 ms per call = 15 % of the GLO-16 step.
//   pass 1 (rows)   : a workgroup owns 32 consecutive rows of one window; two REAL rows are packed into one complex transform
//                     (z = row0 + i row1;  R0[k] = (Z[k] + conj Z[S-k]) / 2,  R1[k] = (Z[k] - conj Z[S-k]) / 2i); the half spectra go through an
//                     LDS tile to the scratch  T[window][kx][y], y < H  (transposed, so that pass 2 reads whole columns as contiguous runs).
//                     The window has H rows, a run-time value: H = S for the square spectra; at S = 256 any H in 2 .. 256 (the rectangular
//                     windows below), where row pairs past the last row are skipped and the second row of the last pair of an odd H is zeros;
//   pass 2 (columns): complex transforms of CB columns per workgroup; amp = |F|, pha = atan2(Im, Re) (Im forced to +0 at the four self-conjugate
//                     bins, as the direct kernel does), staged in LDS and stored with the optional fftshift of both axes.
// One transform is carried by S/4 lanes (one radix-4 butterfly each per pass): a wave runs one 256-point, two 128-point or four 64-point transforms
// at a time.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(const float2 a, const float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// N-point forward transform of b0 (natural order in, natural order out); j = this lane's butterfly index 0 .. N/4-1; tw[k] = exp(-2 pi i k / N).
// The N/4 lanes of a transform belong to ONE wave: LDS accesses of a wave execute in program order, a compiler-level fence is all that is needed.
// N = 4^m: m radix-4 passes.  N = 2 * 4^m (128): the same m passes (Ns = 1, 4, .., 4^(m-1)), then one radix-2 pass with Ns = N/2, in which each of
// the N/4 lanes does two of the N/2 butterflies  out[jj] = in[jj] + tw[jj] in[jj + N/2],  out[jj + N/2] = in[jj] - tw[jj] in[jj + N/2].
constexpr int tfc_pow4_floor(int n) { int p = 1; while (p * 4 <= n) p *= 4; return p; }
template <int N>
__device__ __forceinline__ float2* tfc_fft_r4(float2* b0, float2* b1, const float2* __restrict__ tw, int j) {
  constexpr int N4 = tfc_pow4_floor(N);                          // product of the radix-4 passes
  static_assert(N4 == N || 2 * N4 == N, "N must be 4^m or 2 * 4^m");
#pragma unroll
  for (int Ns = 1; Ns < N4; Ns *= 4) {
    const int k = j & (Ns - 1);
    const int ts = k * (N / (4 * Ns));
    float2 v0 = b0[j], v1 = b0[j + N / 4], v2 = b0[j + N / 2], v3 = b0[j + 3 * N / 4];
    if (Ns > 1) { v1 = cmul(v1, tw[ts]); v2 = cmul(v2, tw[2 * ts]); v3 = cmul(v3, tw[3 * ts]); }
    const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
    const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y), a3 = make_float2(v1.y - v3.y, v3.x - v1.x);   // -i (v1 - v3)
    const int j0 = ((j - k) << 2) + k;
    b1[j0] = make_float2(a0.x + a2.x, a0.y + a2.y);
    b1[j0 + Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
    b1[j0 + 2 * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
    b1[j0 + 3 * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float2* t = b0; b0 = b1; b1 = t;
  }
  if constexpr (2 * N4 == N) {
#pragma unroll
    for (int jj = j; jj < N / 2; jj += N / 4) {
      const float2 v0 = b0[jj], v1 = cmul(b0[jj + N / 2], tw[jj]);
      b1[jj] = make_float2(v0.x + v1.x, v0.y + v1.y);
      b1[jj + N / 2] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float2* t = b0; b0 = b1; b1 = t;
  }
  return b0;
}

// tw[i] = exp(-2 pi i * i / S), i < S, from the exact sincospi; every thread of the workgroup calls it, the caller synchronises
template <int S>
__device__ __forceinline__ void tfc_fill_twiddles(float2* tw) {
  for (int i = threadIdx.x; i < S; i += 256) {
    float sn, cn;
    sincospif(2.f * (float)i / (float)S, &sn, &cn);
    tw[i] = make_float2(cn, -sn);
  }
}

template <int S, bool RAGGED>
__global__ void __launch_bounds__(256)
tfc_fft_rows_kernel(const float* __restrict__ img, const TfcWinGrid g, int H, float2* __restrict__ T) {
  constexpr int NB = S / 2 + 1, G = S / 4, FPW = 64 / G, RPB = 32;          // lanes per transform, transforms per wave at a time, rows per workgroup
  // RAGGED = false: PRECONDITION H even and a multiple of 32 (the square windows, H = S: tfc_launch_spectrum passes nothing else); every row pair of
  // every row block is read and transformed without a check.  RAGGED = true: any H; row pairs past H are skipped.  A skip jumps over the wave barriers
  // of tfc_fft_r4, so it must be wave-uniform: ONE transform per wave, S = 256 only (the other sizes carry 4 or 2 transforms per wave).
  static_assert(!RAGGED || FPW == 1, "a ragged row count needs one transform per wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* tw = reinterpret_cast<float2*>(smem);                   // [S]
  float2* wbuf = tw + S;                                          // [4 waves][2][FPW][S]
  float2* tile = wbuf + 4 * 2 * FPW * S;                          // [NB][RPB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = lane / G, j = lane % G;
  const int nrb = (H + RPB - 1) / RPB;                            // row blocks per window; the last one is ragged when H % 32 != 0
  const int w = blockIdx.x / nrb, y0 = (blockIdx.x % nrb) * RPB;
  const float* base = tfc_window_origin(img, g, w);
  tfc_fill_twiddles<S>(tw);
  __syncthreads();
  float2* b0 = wbuf + ((wave * 2 + 0) * FPW + f) * S;
  float2* b1 = wbuf + ((wave * 2 + 1) * FPW + f) * S;
  auto luma = [&](int y, int x) -> float { return (float)tfc_luma_u8(base + (size_t)y * g.rs + x, g.cs, g.C); };
  for (int it = 0; it < RPB / 2 / (4 * FPW); ++it) {
    const int pr = (it * 4 + wave) * FPW + f;                     // row pair of this workgroup (0 .. 15)
    const int ya = y0 + 2 * pr;
    if (RAGGED && ya >= H) continue;                              // wave-uniform: the whole transform lies past the window
    const bool two = !RAGGED || ya + 1 < H;                       // odd H: the last row is paired with zeros
#pragma unroll
    for (int r = 0; r < 4; ++r) b0[j + r * G] = make_float2(luma(ya, j + r * G), two ? luma(ya + 1, j + r * G) : 0.f);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float2* Z = tfc_fft_r4<S>(b0, b1, tw, j);
    for (int k = j; k < NB; k += G) {
      const float2 a = Z[k], b = Z[(S - k) & (S - 1)];
      tile[k * RPB + 2 * pr] = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
      tile[k * RPB + 2 * pr + 1] = make_float2(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  float2* Tw = T + (size_t)w * NB * H;
  for (int i = tid; i < NB * RPB; i += 256) {
    const int kx = i / RPB, y = y0 + i % RPB;
    if (!RAGGED || y < H) Tw[(size_t)kx * H + y] = tile[i];       // ragged: tile rows past H were never written and are not read
  }
}

template <int S, int CB>
__global__ void __launch_bounds__(256)
tfc_fft_cols_kernel(const float2* __restrict__ T, float* __restrict__ amp, float* __restrict__ pha, int shift) {
  constexpr int NB = S / 2 + 1, G = S / 4, FPW = 64 / G;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* tw = reinterpret_cast<float2*>(smem);                   // [S]
  float2* wbuf = tw + S;                                          // [4 waves][2][FPW][S]
  float* ta = reinterpret_cast<float*>(wbuf + 4 * 2 * FPW * S);   // [S][CB] amplitude
  float* tp = ta + S * CB;                                        // [S][CB] phase
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = lane / G, j = lane % G;
  constexpr int NCB = (NB + CB - 1) / CB;
  const int w = blockIdx.x / NCB, c0 = (blockIdx.x % NCB) * CB;
  tfc_fill_twiddles<S>(tw);
  __syncthreads();
  float2* b0 = wbuf + ((wave * 2 + 0) * FPW + f) * S;
  float2* b1 = wbuf + ((wave * 2 + 1) * FPW + f) * S;
  for (int it = 0; it < CB / (4 * FPW); ++it) {
    const int ci = (it * 4 + wave) * FPW + f;
    const int c = c0 + ci;
    if (c < NB) {                                                 // uniform per group of G lanes (a whole wave when FPW == 1)
      const float2* src = T + ((size_t)w * NB + c) * S;
#pragma unroll
      for (int r = 0; r < 4; ++r) b0[j + r * G] = src[j + r * G];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float2* F = tfc_fft_r4<S>(b0, b1, tw, j);               // columns past the half spectrum transform stale LDS: results unused
    if (c < NB)
      for (int ky = j; ky < S; ky += G) {
        float re = F[ky].x, im = F[ky].y;
        if ((c == 0 || c == S / 2) && (ky == 0 || ky == S / 2)) im = 0.f;
        ta[ky * CB + ci] = sqrtf(re * re + im * im);
        tp[ky * CB + ci] = atan2f(im, re);
      }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  for (int i = tid; i < S * CB; i += 256) {
    const int ky = i / CB, ci = i % CB, c = c0 + ci;
    if (c >= NB) continue;
    int oy = ky, ox = c;
    if (shift) { oy = (ky + S / 2) % S; ox = (c + NB / 2) % NB; }
    const size_t oi = ((size_t)w * S + oy) * NB + ox;
    amp[oi] = ta[i];
    pha[oi] = tp[i];
  }
}

hipError_t tfc_launch_l1_sum(const float* a, const float* b, long long n, float scale, float* out, hipStream_t st) {
  long long nb = (n + 255) / 256;
  if (nb > 512) nb = 512;
  hipLaunchKernelGGL(tfc_l1_sum_kernel, dim3((int)nb), dim3(256), 0, st, a, b, n, scale, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Rectangular windows: H rows x 256 columns, H a run-time value in 2 .. 256 (the regional FFT loss of TFCGAN_multigpu_patchFFT_withregion_FFT.py:353-401
// and ..._withregion_FFT_KL.py:357-420 takes the spectra of rows 0..99 and 100..199, 100 x 129 bins each).  Window k of image n starts at image
// row row0 + k * row_step, column 0.  Same luma, same rfft2, same amp / atan2 as above; amp / pha: [windows][H][129].
//   pass 1 (rows)   : tfc_fft_rows_kernel<256> with H rows: a workgroup owns 32 consecutive rows, a wave one pair of real rows per 256-point
//                     transform.  The half spectra go to the scratch T[window][kx][y] with y < H.
//   pass 2 (columns): H = 100 = 4 * 5 * 5 is no 4^m or 2 * 4^m, so each of the 129 columns takes a DIRECT H-point DFT from an exact table
//                     exp(-2 pi i m / H), m < H (sincospi in double, rounded once), indexed by the integer (ky * y) mod H that is carried along
//                     as t += ky.  A workgroup owns RECT_CB = 13 columns of one window (129 = 9 * 13 + 12), staged in LDS as col[y][column]; a lane
//                     owns one (ky, column) output, so per y the lanes of a wave read 13 consecutive float2 of col (conflict-free) and up to six
//                     table entries (64 consecutive outputs span five or six ky), whose banks are not controlled.
//                     The column MEAN is taken out before the sum and comes back at ky = 0 (sum_y exp(-2 pi i ky y / H) = 0 for every other ky):
//                     F[0] = sum_y R[y],  F[ky] = sum_y (R[y] - F[0] / H) exp(-2 pi i ky y / H).  Column kx = 0 holds the row sums, about 32 000 each
//                     for a mid-grey image, whose direct sum would carry partial sums near 1e6 (ulp 0.06) into bins of a few thousand; without the
//                     mean the terms are as small as the bins they make.
//   Im is forced to +0 at the self-conjugate bins kx in {0, 128} x (ky = 0, and ky = H/2 for even H).
//   fftshift on store: ky -> (ky + H/2) % H (numpy's shift for even and odd H), kx -> (kx + 64) % 129.
// ---------------------------------------------------------------------------------------------------
constexpr int RECT_CB = 13;

__global__ void __launch_bounds__(256)
tfc_dft_rect_cols_kernel(const float2* __restrict__ T, int H, float* __restrict__ amp, float* __restrict__ pha, int shift) {
  constexpr int NB = 129, CB = RECT_CB, NCB = (NB + CB - 1) / CB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* tw = reinterpret_cast<float2*>(smem);                   // [H]      exp(-2 pi i m / H)
  float2* col = tw + H;                                           // [H][CB]  the columns, mean removed
  float2* csum = col + H * CB;                                    // [CB]     sum_y R[y] = F[0]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = blockIdx.x / NCB, c0 = (blockIdx.x % NCB) * CB;
  const int ncol = NB - c0 < CB ? NB - c0 : CB;
  for (int i = tid; i < H; i += 256) {
    double sn, cn;
    sincospi(2.0 * (double)i / (double)H, &sn, &cn);
    tw[i] = make_float2((float)cn, (float)-sn);
  }
  const float2* src = T + ((size_t)w * NB + c0) * H;              // ncol columns of H values, contiguous
  for (int o = tid; o < ncol * H; o += 256) {
    const int ci = o / H, y = o - ci * H;
    col[y * CB + ci] = src[o];
  }
  __syncthreads();
  for (int ci = wave; ci < ncol; ci += 4) {                       // fixed order: lane-strided partial sums, then the xor tree
    float sx = 0.f, sy = 0.f;
    for (int y = lane; y < H; y += 64) { const float2 v = col[y * CB + ci]; sx += v.x; sy += v.y; }
    sx = wave_sum(sx); sy = wave_sum(sy);
    if (lane == 0) csum[ci] = make_float2(sx, sy);
  }
  __syncthreads();
  const float inv_h = 1.f / (float)H;
  for (int o = tid; o < H * CB; o += 256) {
    const int ci = o % CB;
    if (ci < ncol) { col[o].x -= csum[ci].x * inv_h; col[o].y -= csum[ci].y * inv_h; }
  }
  __syncthreads();
  for (int o = tid; o < H * CB; o += 256) {
    const int ky = o / CB, ci = o - ky * CB, c = c0 + ci;
    if (ci >= ncol) continue;
    float re = 0.f, im = 0.f;
    int t = 0;                                                    // (ky * y) mod H
    for (int y = 0; y < H; ++y) {
      const float2 v = col[y * CB + ci], e = tw[t];
      re += v.x * e.x - v.y * e.y;
      im += v.x * e.y + v.y * e.x;
      t += ky;
      if (t >= H) t -= H;
    }
    if (ky == 0) { re = csum[ci].x; im = csum[ci].y; }
    if ((c == 0 || c == NB - 1) && (ky == 0 || 2 * ky == H)) im = 0.f;
    int oy = ky, ox = c;
    if (shift) { oy = (ky + H / 2) % H; ox = (c + NB / 2) % NB; }
    const size_t oi = ((size_t)w * H + oy) * NB + ox;
    amp[oi] = sqrtf(re * re + im * im);
    pha[oi] = atan2f(im, re);
  }
}

// ---------------------------------------------------------------------------------------------------
// Spectra of nwin windows of H rows x S columns on the grid g; amp / pha: [nwin][H][S/2+1].  S in {64, 128, 256}.
//   rect = false: square windows (H = S): row FFT + column FFT through the scratch ws, or, with no scratch, the direct DFT;
//   rect = true : S = 256, H in 2 .. 256: row FFT + direct H-point column DFT through ws.
// ws holds T[nwin][S/2+1][H] (tfc_fft_ws_bytes).
// ---------------------------------------------------------------------------------------------------
size_t tfc_fft_ws_bytes(int S, int H, int nwin) { return (size_t)nwin * (S / 2 + 1) * H * sizeof(float2); }
template <int S, bool RAGGED>
static void launch_fft_rows(const float* img, const TfcWinGrid& g, int H, int nwin, void* ws, hipStream_t st) {
  constexpr int NB = S / 2 + 1, FPW = 64 / (S / 4);
  const size_t lds = (size_t)(S + 4 * 2 * FPW * S + NB * 32) * sizeof(float2);
  hipLaunchKernelGGL((tfc_fft_rows_kernel<S, RAGGED>), dim3(nwin * ((H + 31) / 32)), dim3(256), lds, st, img, g, H, (float2*)ws);
}
template <int S, int CB>
static void launch_fft_cols(int nwin, float* amp, float* pha, int shift, void* ws, hipStream_t st) {
  constexpr int NB = S / 2 + 1, FPW = 64 / (S / 4);
  static_assert(CB % (4 * FPW) == 0, "a workgroup's four waves transform 4 * FPW columns at a time");
  const size_t lds = (size_t)(S + 4 * 2 * FPW * S) * sizeof(float2) + (size_t)2 * S * CB * sizeof(float);
  hipLaunchKernelGGL((tfc_fft_cols_kernel<S, CB>), dim3(nwin * ((NB + CB - 1) / CB)), dim3(256), lds, st, (const float2*)ws, amp, pha, shift);
}
template <int S, int KG>
static hipError_t launch_direct(const float* img, const TfcWinGrid& g, int nwin, float* amp, float* pha, int shift, hipStream_t st) {
  constexpr int NB = S / 2 + 1;
  constexpr size_t lds = S * S + 2 * S * 4 + S * KG * 2 * 4;     // 51 200 B at <128, 33>
  if constexpr (lds > 65536) {                                   // > 64 KiB of dynamic LDS needs an explicit opt-in (once)
    static bool attr_set = false;
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tfc_spectrum_kernel<S, KG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      attr_set = true;
    }
  }
  hipLaunchKernelGGL((tfc_spectrum_kernel<S, KG>), dim3(nwin, (NB + KG - 1) / KG), dim3(256), lds, st, img, g, amp, pha, shift);
  return hipSuccess;
}
hipError_t tfc_launch_spectrum(const float* img, const TfcWinGrid& g, int S, int H, bool rect, int nwin, float* amp, float* pha, int shift, void* ws,
                               hipStream_t st) {
  if (rect ? (S != 256 || !ws) : (H != S)) return hipErrorInvalidValue;
  if (rect) {
    const size_t lds_c = (size_t)(H + H * RECT_CB + RECT_CB) * sizeof(float2);          // 28 776 B at H = 256
    launch_fft_rows<256, true>(img, g, H, nwin, ws, st);
    hipLaunchKernelGGL(tfc_dft_rect_cols_kernel, dim3(nwin * ((129 + RECT_CB - 1) / RECT_CB)), dim3(256), lds_c, st, (const float2*)ws, H, amp, pha, shift);
  } else if (ws) {
    if (S == 64) { launch_fft_rows<64, false>(img, g, H, nwin, ws, st); launch_fft_cols<64, 16>(nwin, amp, pha, shift, ws, st); }
    else if (S == 128) { launch_fft_rows<128, false>(img, g, H, nwin, ws, st); launch_fft_cols<128, 8>(nwin, amp, pha, shift, ws, st); }
    else if (S == 256) { launch_fft_rows<256, false>(img, g, H, nwin, ws, st); launch_fft_cols<256, 8>(nwin, amp, pha, shift, ws, st); }
    else return hipErrorInvalidValue;
  } else {                                                        // no scratch given: direct DFT (also the independent cross-check of the FFT path)
    hipError_t e = S == 64 ? launch_direct<64, 33>(img, g, nwin, amp, pha, shift, st)
                 : S == 128 ? launch_direct<128, 33>(img, g, nwin, amp, pha, shift, st)      // two column groups (33 + 32 of the 65 columns)
                 : S == 256 ? launch_direct<256, 16>(img, g, nwin, amp, pha, shift, st) : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// KL form of the regional loss (TFCGAN_multigpu_patchFFT_withregion_FFT_KL.py:400-418): every spectrum goes through F.log_softmax(., dim=0) -- over
// the BATCH -- and nn.KLDivLoss(reduction="mean", log_target=True), the mean over all elements of exp(t) (t - x).  af, pf, ar: [N][M] (fake amplitude,
// fake phase, real amplitude); the reference takes the real PHASE target from the real amplitudes as well (:401, :404), so ar is the target of both:
//   t = ar_n - lse_n(ar),  xa = af_n - lse_n(af),  xp = pf_n - lse_n(pf);   out[0] += scale * sum exp(t) (t - xa),  out[1] += scale * sum exp(t) (t - xp).
// One lane owns one bin and walks the N batch entries twice (the bin index is the fastest one: coalesced): an online max / sum exp(x - max), then the
// terms.  The log-softmax is max-subtracted in fp32, (x - max) - log(sum exp(x - max)) -- amplitudes reach 3.3e6.  exp(t) = 0 contributes nothing,
// whatever t - x is.  At N = 1 every term is exp(0) * (0 - 0).  Slots of this kernel's own (logged scalars, tfc_block_commit); like the triplet and L1 heads it runs on the SIDE stream only
// (engine.step: pixel_losses).
// ---------------------------------------------------------------------------------------------------
static __device__ TfcRedSlot g_kl_amp_slot, g_kl_pha_slot;

// one step of the online log-sum-exp: afterwards m = max(m, x) and z = sum exp(. - m) over the entries seen so far (m = -inf, z = 0 before the first:
// 0 * exp(-inf) + 1 = 1)
static __device__ __forceinline__ void kl_online(float x, float& m, float& z) {
  if (x > m) { z = z * expf(m - x) + 1.f; m = x; }
  else z += expf(x - m);
}

__global__ void __launch_bounds__(256)
tfc_batch_kl_kernel(const float* __restrict__ af, const float* __restrict__ pf, const float* __restrict__ ar, int N, long long M, float scale,
                    float* out) {
  __shared__ float red[2][4];
  float sa = 0.f, sp = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) {
    float ma = -INFINITY, mp = -INFINITY, mr = -INFINITY, za = 0.f, zp = 0.f, zr = 0.f;
    for (int n = 0; n < N; ++n) {                                 // first walk: running max m and z = sum exp(x - m), re-based when the max moves
      const size_t o = (size_t)n * M + i;
      kl_online(af[o], ma, za); kl_online(pf[o], mp, zp); kl_online(ar[o], mr, zr);
    }
    const float la = logf(za), lp = logf(zp), lr = logf(zr);
    for (int n = 0; n < N; ++n) {
      const size_t o = (size_t)n * M + i;
      const float t = (ar[o] - mr) - lr;
      const float e = expf(t);
      if (e > 0.f) {                                              // exp(t) = 0: no term (never 0 * inf)
        sa += e * (t - ((af[o] - ma) - la));
        sp += e * (t - ((pf[o] - mp) - lp));
      }
    }
  }
  sa = wave_sum(sa); sp = wave_sum(sp);                           // two sums behind ONE barrier: tfc_block_sum4 would cost a second one
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sa; red[1][threadIdx.x >> 6] = sp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tfc_block_commit(&g_kl_amp_slot, ((double)red[0][0] + (double)red[0][1] + (double)red[0][2] + (double)red[0][3]) * (double)scale, out);
    tfc_block_commit(&g_kl_pha_slot, ((double)red[1][0] + (double)red[1][1] + (double)red[1][2] + (double)red[1][3]) * (double)scale, out + 1);
  }
}
hipError_t tfc_launch_batch_kl(const float* af, const float* pf, const float* ar, int N, long long M, float scale, float* out, hipStream_t st) {
  long long nb = (M + 255) / 256;
  if (nb > 512) nb = 512;
  hipLaunchKernelGGL(tfc_batch_kl_kernel, dim3((int)nb), dim3(256), 0, st, af, pf, ar, N, M, scale, out);
  return hipGetLastError();
}

// ---- the same loss in phases, for a batch that is spread over `world` ranks: the softmax runs over the batch, so the state of the
// online log-sum-exp, one (max, sum) pair per bin and spectrum, is what the ranks exchange between the two walks.
//   K1    : first walk over this rank's N entries -> rec [3][M][2] = (m, z) of af, pf, ar
//   merge : recs [world][3][M][2] -> glob [3][M][2] = (max, log sum) over all ranks. The pairs are folded in rank order by the re-basing rule of
//           kl_online, with a rank's z in the place of the single entry's 1: the same floats on every rank. One record gives (m, logf(z)).
//   K2    : second walk with the global pair: this rank's terms, through the slots and the grid of tfc_batch_kl_kernel (same stream rule)
__global__ void __launch_bounds__(256)
tfc_batch_kl_stats_kernel(const float* __restrict__ af, const float* __restrict__ pf, const float* __restrict__ ar, int N, long long M,
                          float2* __restrict__ rec) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) {
    float ma = -INFINITY, mp = -INFINITY, mr = -INFINITY, za = 0.f, zp = 0.f, zr = 0.f;
    for (int n = 0; n < N; ++n) {
      const size_t o = (size_t)n * M + i;
      kl_online(af[o], ma, za); kl_online(pf[o], mp, zp); kl_online(ar[o], mr, zr);
    }
    rec[i] = make_float2(ma, za); rec[M + i] = make_float2(mp, zp); rec[2 * M + i] = make_float2(mr, zr);
  }
}

__global__ void __launch_bounds__(1024)
tfc_batch_kl_merge_kernel(const float2* __restrict__ recs, int world, long long M3, float2* __restrict__ glob) {
  for (long long i = threadIdx.x; i < M3; i += 1024) {            // one workgroup; every bin folds its `world` pairs in rank order
    float m = -INFINITY, z = 0.f;
    for (int r = 0; r < world; ++r) {
      const float2 p = recs[(size_t)r * M3 + i];
      if (p.x > m) { z = z * expf(m - p.x) + p.y; m = p.x; }
      else z += p.y * expf(p.x - m);
    }
    glob[i] = make_float2(m, logf(z));
  }
}

__global__ void __launch_bounds__(256)
tfc_batch_kl_terms_kernel(const float* __restrict__ af, const float* __restrict__ pf, const float* __restrict__ ar, int N, long long M,
                          const float2* __restrict__ glob, float scale, float* out) {
  __shared__ float red[2][4];
  float sa = 0.f, sp = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) {
    const float2 ga = glob[i], gp = glob[M + i], gr = glob[2 * M + i];
    const float ma = ga.x, la = ga.y, mp = gp.x, lp = gp.y, mr = gr.x, lr = gr.y;
    for (int n = 0; n < N; ++n) {
      const size_t o = (size_t)n * M + i;
      const float t = (ar[o] - mr) - lr;
      const float e = expf(t);
      if (e > 0.f) {
        sa += e * (t - ((af[o] - ma) - la));
        sp += e * (t - ((pf[o] - mp) - lp));
      }
    }
  }
  sa = wave_sum(sa); sp = wave_sum(sp);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sa; red[1][threadIdx.x >> 6] = sp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tfc_block_commit(&g_kl_amp_slot, ((double)red[0][0] + (double)red[0][1] + (double)red[0][2] + (double)red[0][3]) * (double)scale, out);
    tfc_block_commit(&g_kl_pha_slot, ((double)red[1][0] + (double)red[1][1] + (double)red[1][2] + (double)red[1][3]) * (double)scale, out + 1);
  }
}

static int kl_grid(long long M) {
  long long nb = (M + 255) / 256;
  return (int)(nb > 512 ? 512 : nb);
}
hipError_t tfc_launch_batch_kl_stats(const float* af, const float* pf, const float* ar, int N, long long M, void* rec, hipStream_t st) {
  hipLaunchKernelGGL(tfc_batch_kl_stats_kernel, dim3(kl_grid(M)), dim3(256), 0, st, af, pf, ar, N, M, (float2*)rec);
  return hipGetLastError();
}
hipError_t tfc_launch_batch_kl_merge(const void* recs, int world, long long M, void* glob, hipStream_t st) {
  hipLaunchKernelGGL(tfc_batch_kl_merge_kernel, dim3(1), dim3(1024), 0, st, (const float2*)recs, world, 3 * M, (float2*)glob);
  return hipGetLastError();
}
hipError_t tfc_launch_batch_kl_terms(const float* af, const float* pf, const float* ar, int N, long long M, const void* glob, float scale, float* out,
                                     hipStream_t st) {
  hipLaunchKernelGGL(tfc_batch_kl_terms_kernel, dim3(kl_grid(M)), dim3(256), 0, st, af, pf, ar, N, M, (const float2*)glob, scale, out);
  return hipGetLastError();
}
