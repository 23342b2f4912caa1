// The label-conditioned ("debiased") 4-patch scripts on the GPU (reference TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_debiased.py "DB1", ..._V2.py, ..._V3.py):
//   label plane    : fc = nn.Linear(3, H*W) of the labels, reshaped [H,W], 4th input channel of down1                      (DB1:146-151, :171-174)
//   auxiliary heads: three nn.Linear(6*H*W, 2|4|3) + Softmax on the raw concatenated discriminator input (NCHW-flattened)    (DB1:216-233)
//   label loss     : nn.CrossEntropyLoss applied to the softmax OUTPUT (a second log-softmax inside the loss), reproduced as is (DB1:522, :603-606)
// Everything here is streaming work (designed HBM-bound; profiles/debias_ab.md has what each kernel reaches): 16-byte loads and stores, fp32
// accumulation, no float atomics. Sums over the batch run in ascending n inside one
// thread; the only sum that crosses workgroups (the heads' logits) leaves every wave as a partial in a fixed slot of part_ws and is added by
// tfc_part_reduce_kernel. The grids run over (sample, fixed 256-pixel chunk) or over the chunk alone with the batch walked inside: nothing that
// shapes the arithmetic of one sample depends on N.
// The heads keep their torch layout ([C_h][6*H*W] rows of three separate parameters): a kernel gets the <= 16 row pointers in its argument block.
// The reference's 9 classes run with the chunk's 54 weights in registers, staged through LDS so that global memory sees 16-byte accesses only;
// other class counts (10..16 rows in all: more than 64 KB of staging) take the same kernels with 4-byte weight accesses.
#include "common.h"

#define TFC_AUX_CHUNK 256                                        // pixels per workgroup of the head kernels = threads

template <typename T> __device__ __forceinline__ void load_pixel8(const T* p, float* v);
template <> __device__ __forceinline__ void load_pixel8<bf16_t>(const bf16_t* p, float* v) { unpack16<bf16_t>(*reinterpret_cast<const uint4*>(p), v); }
template <> __device__ __forceinline__ void load_pixel8<float>(const float* p, float* v) {
  unpack16<float>(*reinterpret_cast<const uint4*>(p), v);
  unpack16<float>(*reinterpret_cast<const uint4*>(p + 4), v + 4);
}
template <typename T> __device__ __forceinline__ void store_pixel8(T* p, const float* v);
template <> __device__ __forceinline__ void store_pixel8<bf16_t>(bf16_t* p, const float* v) { *reinterpret_cast<uint4*>(p) = pack16<bf16_t>(v); }
template <> __device__ __forceinline__ void store_pixel8<float>(float* p, const float* v) {
  *reinterpret_cast<uint4*>(p) = pack16<float>(v);
  *reinterpret_cast<uint4*>(p + 4) = pack16<float>(v + 4);
}

// ---- (a) torch.cat((x, fc(labels).view(N,1,H,W)), 1) -> NHWC8. One thread per (sample, 4 pixels). plane = ((b + l0 w0) + l1 w1) + l2 w2 in fp32 fmas.
template <typename T>
__global__ void __launch_bounds__(256)
tfc_pack_labels_kernel(const float* __restrict__ img, const float* __restrict__ labels, const float* __restrict__ fw, const float* __restrict__ fb,
                       T* __restrict__ out, int HW) {
  const int q = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (4 * (long long)q >= HW) return;
  const float l0 = labels[n * 3], l1 = labels[n * 3 + 1], l2 = labels[n * 3 + 2];
  float w[12], b[4], c[3][4];
  const float4* fw4 = reinterpret_cast<const float4*>(fw + (size_t)12 * q);
#pragma unroll
  for (int i = 0; i < 3; ++i) { const float4 t = fw4[i]; w[4 * i] = t.x; w[4 * i + 1] = t.y; w[4 * i + 2] = t.z; w[4 * i + 3] = t.w; }
  { const float4 t = *reinterpret_cast<const float4*>(fb + (size_t)4 * q); b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w; }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float4 t = *reinterpret_cast<const float4*>(img + ((size_t)n * 3 + ch) * HW + (size_t)4 * q);
    c[ch][0] = t.x; c[ch][1] = t.y; c[ch][2] = t.z; c[ch][3] = t.w;
  }
  T* o = out + ((size_t)n * HW + (size_t)4 * q) * 8;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float plane = fmaf(l2, w[3 * j + 2], fmaf(l1, w[3 * j + 1], fmaf(l0, w[3 * j], b[j])));
    const float v[8] = {c[0][j], c[1][j], c[2][j], plane, 0.f, 0.f, 0.f, 0.f};
    store_pixel8<T>(o + 8 * j, v);
  }
}

// ---- (b) d fc.weight[p][k] = sum_n g[n][p] l[n][k], d fc.bias[p] = sum_n g[n][p]; g = channel plane of an fp32 NCHW gradient (sample stride gs).
__global__ void __launch_bounds__(256)
tfc_label_plane_bwd_kernel(const float* __restrict__ g, long long gs, const float* __restrict__ labels, float* __restrict__ dw, float* __restrict__ db,
                           int N, int HW, int accumulate) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (4 * (long long)q >= HW) return;
  float aw[12], ab[4];
#pragma unroll
  for (int i = 0; i < 12; ++i) aw[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) ab[i] = 0.f;
  for (int n = 0; n < N; ++n) {                                   // ascending n, one thread: a fixed order
    const float4 t = *reinterpret_cast<const float4*>(g + (size_t)n * gs + (size_t)4 * q);
    const float v[4] = {t.x, t.y, t.z, t.w};
    const float l[3] = {labels[n * 3], labels[n * 3 + 1], labels[n * 3 + 2]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ab[j] += v[j];
#pragma unroll
      for (int k = 0; k < 3; ++k) aw[3 * j + k] = fmaf(v[j], l[k], aw[3 * j + k]);
    }
  }
  float4* dw4 = reinterpret_cast<float4*>(dw + (size_t)12 * q);
  float4* db4 = reinterpret_cast<float4*>(db + (size_t)4 * q);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float4 o = make_float4(aw[4 * i], aw[4 * i + 1], aw[4 * i + 2], aw[4 * i + 3]);
    if (accumulate) { const float4 p = dw4[i]; o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
    dw4[i] = o;
  }
  float4 o = make_float4(ab[0], ab[1], ab[2], ab[3]);
  if (accumulate) { const float4 p = db4[0]; o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
  db4[0] = o;
}

template <int CT> struct AuxStage { static constexpr bool lds = (size_t)6 * CT * TFC_AUX_CHUNK * sizeof(float) <= 65536; };

// the chunk's 6 * ct weights of pixel p0 + threadIdx.x into w[] (rows >= ct: zeros). LDS form: 16-byte global loads, one ds_write_b128 per unit, then
// every thread reads its column (consecutive lanes, consecutive banks).
template <int CT>
__device__ __forceinline__ void aux_load_weights(const TfcAuxRows& rows, int ct, int p0, int HW, float* lw, float* w) {
  const int t = threadIdx.x;
  if (AuxStage<CT>::lds) {
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), u = t & 63;   // a wave per weight row: the row pointer is a scalar load
    for (int j = wv; j < 6 * ct; j += 4) {
      const int o = j / 6, c = j - 6 * o;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p0 + 4 * u < HW) v = *reinterpret_cast<const float4*>(rows.w[o] + (size_t)c * HW + p0 + 4 * u);   // HW % 4 == 0: whole units
      *reinterpret_cast<float4*>(lw + j * TFC_AUX_CHUNK + 4 * u) = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 6 * CT; ++j) w[j] = j < 6 * ct ? lw[j * TFC_AUX_CHUNK + t] : 0.f;
  } else {
    const bool ok = p0 + t < HW;
#pragma unroll
    for (int j = 0; j < 6 * CT; ++j) w[j] = (ok && j < 6 * ct) ? rows.w[j / 6][(size_t)(j % 6) * HW + p0 + t] : 0.f;
  }
}

// ---- (c) logits[n][o] = b[o] + sum_{c < 6, p} x[n][p][c] W[o][c HW + p]. One workgroup per 256-pixel chunk; the chunk's weights are read ONCE and stay in
// registers while the workgroup walks the batch. part[n][chunk * 4 + wave][ct]: one slot per wave (its 64-lane butterfly sum: a fixed order); the
// bias rides in slot 0.
template <typename T, int CT>
__global__ void __launch_bounds__(256)
tfc_aux_heads_fwd_kernel(const T* __restrict__ x, TfcAuxRows rows, int ct, float* __restrict__ part, int N, int HW) {
  __shared__ __attribute__((aligned(16))) float lw[AuxStage<CT>::lds ? 6 * CT * TFC_AUX_CHUNK : 4];
  const int t = threadIdx.x, p0 = blockIdx.x * TFC_AUX_CHUNK, p = p0 + t;
  float w[6 * CT];
  aux_load_weights<CT>(rows, ct, p0, HW, lw, w);
  const bool ok = p < HW;
  const int slot = blockIdx.x * 4 + (t >> 6), nparts = gridDim.x * 4;
  float bias[CT];
#pragma unroll
  for (int o = 0; o < CT; ++o) bias[o] = (slot == 0 && o < ct) ? rows.b[o][0] : 0.f;
#pragma unroll 2
  for (int n = 0; n < N; ++n) {
    float xv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) load_pixel8<T>(x + ((size_t)n * HW + p) * 8, xv);
    float* dst = part + ((size_t)n * nparts + slot) * ct;
#pragma unroll
    for (int o = 0; o < CT; ++o) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < 6; ++c) a = fmaf(xv[c], w[o * 6 + c], a);
      a = wave_sum(a);
      if ((t & 63) == 0 && o < ct) dst[o] = a + bias[o];
    }
  }
}

// ---- (e) g[n][c][p] += sum_o dl[n][o] W[o][c HW + p], c < 3 (the generated image's half of the discriminator input). One thread per (channel, 4 pixels);
// its ct float4 of weights are read once, the batch is walked inside.
template <int CT>
__global__ void __launch_bounds__(256)
tfc_aux_heads_dgrad_kernel(float* __restrict__ g, long long gs, TfcAuxRows rows, int ct, const float* __restrict__ dl, int N, int HW) {
  const int q = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (4 * (long long)q >= HW) return;
  float4 w[CT];
#pragma unroll
  for (int o = 0; o < CT; ++o)
    w[o] = o < ct ? *reinterpret_cast<const float4*>(rows.w[o] + (size_t)c * HW + (size_t)4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int n = 0; n < N; ++n) {
    float4* gp = reinterpret_cast<float4*>(g + (size_t)n * gs + (size_t)c * HW + (size_t)4 * q);
    float4 v = *gp;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int o = 0; o < CT; ++o) {
      if (o < ct) {
        const float d = dl[n * ct + o];
        a.x = fmaf(d, w[o].x, a.x); a.y = fmaf(d, w[o].y, a.y); a.z = fmaf(d, w[o].z, a.z); a.w = fmaf(d, w[o].w, a.w);
      }
    }
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    *gp = v;
  }
}

// ---- (f) dW[o][c HW + p] (+)= sum_n dl_r[n][o] x_r[n][p][c] + sum_n dl_f[n][o] x_f[n][p][c]; db[o] (+)= sum_n dl_r[n][o] + sum_n dl_f[n][o].
// One thread per pixel, 6 * ct sums in registers, real pair first, n ascending; written straight into the torch-layout gradient rows.
template <typename T, int CT>
__global__ void __launch_bounds__(256)
tfc_aux_heads_wgrad_kernel(const T* __restrict__ xr, const float* __restrict__ dlr, const T* __restrict__ xf, const float* __restrict__ dlf,
                           TfcAuxGradRows rows, int ct, int N, int HW, int accumulate) {
  __shared__ __attribute__((aligned(16))) float lw[AuxStage<CT>::lds ? 6 * CT * TFC_AUX_CHUNK : 4];
  const int t = threadIdx.x, p0 = blockIdx.x * TFC_AUX_CHUNK, p = p0 + t;
  const bool ok = p < HW;
  float acc[6 * CT];
#pragma unroll
  for (int j = 0; j < 6 * CT; ++j) acc[j] = 0.f;
#pragma unroll 1
  for (int pair = 0; pair < 2; ++pair) {
    const T* x = pair ? xf : xr;
    const float* dl = pair ? dlf : dlr;
    if (!x) continue;
#pragma unroll 2
    for (int n = 0; n < N; ++n) {
      float xv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (ok) load_pixel8<T>(x + ((size_t)n * HW + p) * 8, xv);
#pragma unroll
      for (int o = 0; o < CT; ++o) {
        if (o < ct) {
          const float d = dl[n * ct + o];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc[o * 6 + c] = fmaf(d, xv[c], acc[o * 6 + c]);
        }
      }
    }
  }
  if (AuxStage<CT>::lds) {
#pragma unroll
    for (int j = 0; j < 6 * CT; ++j) lw[j * TFC_AUX_CHUNK + t] = acc[j];
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), u = t & 63;   // a wave per gradient row
    for (int j = wv; j < 6 * ct; j += 4) {
      const int o = j / 6, c = j - 6 * o;
      if (p0 + 4 * u >= HW) continue;
      float4 v = *reinterpret_cast<const float4*>(lw + j * TFC_AUX_CHUNK + 4 * u);
      float4* dst = reinterpret_cast<float4*>(rows.w[o] + (size_t)c * HW + p0 + 4 * u);
      if (accumulate) { const float4 q = *dst; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
      *dst = v;
    }
  } else if (ok) {
#pragma unroll
    for (int j = 0; j < 6 * CT; ++j) {
      if (j < 6 * ct) {
        float* dst = rows.w[j / 6] + (size_t)(j % 6) * HW + p;
        *dst = accumulate ? *dst + acc[j] : acc[j];
      }
    }
  }
  if (blockIdx.x == 0 && t < ct) {
    float s = 0.f;
    if (xr) for (int n = 0; n < N; ++n) s += dlr[n * ct + t];
    if (xf) for (int n = 0; n < N; ++n) s += dlf[n * ct + t];
    for (int o = 0; o < ct; ++o)                                  // o is uniform: the bias pointer is a scalar load
      if (t == o) rows.b[o][0] = accumulate ? rows.b[o][0] + s : s;
  }
}

// ---- (d) per head h: p = softmax(z_h) (the reference's *_hat), loss_h = mean_n( logsumexp(p) - p[y] ) = CrossEntropyLoss(p, y): the SECOND softmax is
// the reference's (DB1:218-220 + :522). total = scale * sum_h w_h loss_h; dlogits = d total / d z through both softmaxes. One workgroup; doubles inside
// (N * 9 values: free), thread t takes samples t, t + 256, ... ascending, then a fixed butterfly + four wave partials in order. A target outside
// [0, C_h) (the host entry point refuses those it can see) gives a NaN loss and no one-hot term: never an out-of-range access.
__global__ void __launch_bounds__(256)
tfc_softmax_ce_heads_kernel(const float* __restrict__ logits, const int* __restrict__ targets, TfcCeHeads a, int ct, int N, float* __restrict__ probs,
                            float* __restrict__ losses, float* __restrict__ dlogits) {
  __shared__ double red[3][4];
  const int t = threadIdx.x;
  double ls[3] = {0.0, 0.0, 0.0};
  for (int n = t; n < N; n += 256) {
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int C = a.nc[h], off = a.off[h], y = targets[n * 3 + h];
      const bool yok = y >= 0 && y < C;
      double z[TFC_AUX_MAXC], pr[TFC_AUX_MAXC];
      double m = -1.0e300;
#pragma unroll
      for (int j = 0; j < TFC_AUX_MAXC; ++j) { z[j] = j < C ? (double)logits[n * ct + off + j] : 0.0; if (j < C && z[j] > m) m = z[j]; }
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < TFC_AUX_MAXC; ++j) { pr[j] = j < C ? exp(z[j] - m) : 0.0; s += pr[j]; }
      double m2 = 0.0, py = 0.0;
#pragma unroll
      for (int j = 0; j < TFC_AUX_MAXC; ++j) {
        pr[j] = pr[j] / s;
        if (j < C) { probs[n * ct + off + j] = (float)pr[j]; if (pr[j] > m2) m2 = pr[j]; if (j == y) py = pr[j]; }
      }
      double s2 = 0.0;
#pragma unroll
      for (int j = 0; j < TFC_AUX_MAXC; ++j) { z[j] = j < C ? exp(pr[j] - m2) : 0.0; s2 += z[j]; }   // z: now the second softmax's numerators
      const double lse = m2 + log(s2);
      ls[h] += yok ? lse - py : __longlong_as_double(0x7ff8000000000000LL);
      if (dlogits) {
        const double coef = (double)a.scale * (double)a.w[h] / (double)N;
        double dot = 0.0;
#pragma unroll
        for (int j = 0; j < TFC_AUX_MAXC; ++j) { z[j] = (z[j] / s2 - ((yok && j == y) ? 1.0 : 0.0)) * coef; dot += z[j] * pr[j]; }   // z: d total / d p
#pragma unroll
        for (int j = 0; j < TFC_AUX_MAXC; ++j) if (j < C) dlogits[n * ct + off + j] = (float)(pr[j] * (z[j] - dot));
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    double v = ls[h];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((t & 63) == 0) red[h][t >> 6] = v;
  }
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int h = 0; h < 3; ++h) {
      const double mean = (((red[h][0] + red[h][1]) + red[h][2]) + red[h][3]) / (double)N;
      losses[h] = (float)mean;
      tot += (double)a.w[h] * mean;
    }
    losses[3] = (float)((double)a.scale * tot);
  }
}

// ---- launchers (arguments already checked by the entry points in api.hip) -----------------------------------------------------------------
static inline bool aux_bf16(int dt) { return dt == TFC_DT_BF16; }   // fp32 and bf16x3 store fp32

hipError_t tfc_launch_pack_labels(int dt, const float* img, const float* labels, const float* fw, const float* fb, void* out, int N, int HW, hipStream_t st) {
  const dim3 grid((unsigned)((HW / 4 + 255) / 256), (unsigned)N);
  if (aux_bf16(dt)) hipLaunchKernelGGL((tfc_pack_labels_kernel<bf16_t>), grid, dim3(256), 0, st, img, labels, fw, fb, (bf16_t*)out, HW);
  else hipLaunchKernelGGL((tfc_pack_labels_kernel<float>), grid, dim3(256), 0, st, img, labels, fw, fb, (float*)out, HW);
  return hipGetLastError();
}

hipError_t tfc_launch_label_plane_bwd(const float* g, long long gs, const float* labels, float* dw, float* db, int N, int HW, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(tfc_label_plane_bwd_kernel, dim3((unsigned)((HW / 4 + 255) / 256)), dim3(256), 0, st, g, gs, labels, dw, db, N, HW, accumulate);
  return hipGetLastError();
}

int tfc_aux_fwd_nparts(int HW) { return (HW + TFC_AUX_CHUNK - 1) / TFC_AUX_CHUNK * 4; }

hipError_t tfc_launch_aux_heads_fwd(int dt, const void* x, const TfcAuxRows& rows, int ct, float* logits, float* part_ws, int N, int HW, hipStream_t st) {
  const int nchunk = (HW + TFC_AUX_CHUNK - 1) / TFC_AUX_CHUNK;
  if (!part_ws || (long long)N * nchunk * 4 * ct > (long long)TFC_PART_WS_FLOATS) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(logits, 0, sizeof(float) * (size_t)N * ct, st);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)nchunk);
  if (ct == 9) {
    if (aux_bf16(dt)) hipLaunchKernelGGL((tfc_aux_heads_fwd_kernel<bf16_t, 9>), grid, dim3(256), 0, st, (const bf16_t*)x, rows, ct, part_ws, N, HW);
    else hipLaunchKernelGGL((tfc_aux_heads_fwd_kernel<float, 9>), grid, dim3(256), 0, st, (const float*)x, rows, ct, part_ws, N, HW);
  } else {
    if (aux_bf16(dt)) hipLaunchKernelGGL((tfc_aux_heads_fwd_kernel<bf16_t, TFC_AUX_MAXC>), grid, dim3(256), 0, st, (const bf16_t*)x, rows, ct, part_ws, N, HW);
    else hipLaunchKernelGGL((tfc_aux_heads_fwd_kernel<float, TFC_AUX_MAXC>), grid, dim3(256), 0, st, (const float*)x, rows, ct, part_ws, N, HW);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return tfc_launch_part_reduce(part_ws, logits, N, nchunk * 4, ct, st);
}

hipError_t tfc_launch_aux_heads_dgrad(float* g, long long gs, const TfcAuxRows& rows, int ct, const float* dl, int N, int HW, hipStream_t st) {
  const dim3 grid((unsigned)((HW / 4 + 255) / 256), 3);
  if (ct == 9) hipLaunchKernelGGL((tfc_aux_heads_dgrad_kernel<9>), grid, dim3(256), 0, st, g, gs, rows, ct, dl, N, HW);
  else hipLaunchKernelGGL((tfc_aux_heads_dgrad_kernel<TFC_AUX_MAXC>), grid, dim3(256), 0, st, g, gs, rows, ct, dl, N, HW);
  return hipGetLastError();
}

hipError_t tfc_launch_aux_heads_wgrad(int dt, const void* xr, const float* dlr, const void* xf, const float* dlf, const TfcAuxGradRows& rows, int ct,
                                      int N, int HW, int accumulate, hipStream_t st) {
  const dim3 grid((unsigned)((HW + TFC_AUX_CHUNK - 1) / TFC_AUX_CHUNK));
  if (ct == 9) {
    if (aux_bf16(dt)) hipLaunchKernelGGL((tfc_aux_heads_wgrad_kernel<bf16_t, 9>), grid, dim3(256), 0, st, (const bf16_t*)xr, dlr, (const bf16_t*)xf, dlf, rows, ct, N, HW, accumulate);
    else hipLaunchKernelGGL((tfc_aux_heads_wgrad_kernel<float, 9>), grid, dim3(256), 0, st, (const float*)xr, dlr, (const float*)xf, dlf, rows, ct, N, HW, accumulate);
  } else {
    if (aux_bf16(dt)) hipLaunchKernelGGL((tfc_aux_heads_wgrad_kernel<bf16_t, TFC_AUX_MAXC>), grid, dim3(256), 0, st, (const bf16_t*)xr, dlr, (const bf16_t*)xf, dlf, rows, ct, N, HW, accumulate);
    else hipLaunchKernelGGL((tfc_aux_heads_wgrad_kernel<float, TFC_AUX_MAXC>), grid, dim3(256), 0, st, (const float*)xr, dlr, (const float*)xf, dlf, rows, ct, N, HW, accumulate);
  }
  return hipGetLastError();
}

hipError_t tfc_launch_softmax_ce_heads(const float* logits, const int* targets, const TfcCeHeads& a, int ct, int N, float* probs, float* losses,
                                       float* dlogits, hipStream_t st) {
  hipLaunchKernelGGL(tfc_softmax_ce_heads_kernel, dim3(1), dim3(256), 0, st, logits, targets, a, ct, N, probs, losses, dlogits);
  return hipGetLastError();
}
