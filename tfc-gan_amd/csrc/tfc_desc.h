// Shared host/device descriptors of the TFC-GAN gather-GEMM engine (gfx950).
//
// Every convolution-shaped op of the PATCH-16 hot path (reference:
// TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_16P.py:102-211 -- Conv2d k4 s1 p1, ConvTranspose2d k4 s2 p1,
// Upsample+ZeroPad+Conv2d, ZeroPad+Conv2d, and all of their dgrad / wgrad passes) is expressed as one
// table-driven "gather GEMM":
//
//     out[img][a*OS+OOY][b*OS+OOX][n] = sum over planes pl, taps t in pl, channels c of
//         in[img][(a + dy0[pl] + dy[t])*SS + py[pl]][(b + dx0[pl] + dx[t])*SS + px[pl]][c]
//           * W[n][slot(pl,t)][c]                       (zero outside the source image)
//
// (a,b) runs over a GH x GW "gather grid"; a workgroup owns an 8 x 16 tile of that grid, stages the
// (8+span) x (16+span) halo of the source once per 64-byte channel chunk in LDS and replays it for
// every tap, so the im2col matrix is never materialised and each source byte crosses HBM/L2 once per
// chunk instead of once per tap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tfc_gan.h"   // TFC_DT_*, TFC_OP_*, TFC_EP_* and TfcVitGemm: the public values are written down there and nowhere else

#define TFC_TILE_H 8
#define TFC_TILE_W 16
#define TFC_LDS_P 24          // halo row pitch in pixels (== 8 mod 16: conflict-free ds_read_b128, see igemm.hip)
#define TFC_MAX_HH 11         // max halo rows (8 + 3)
#define TFC_MAX_HW 19         // max halo cols (16 + 3)
#define TFC_MAX_TAPS 16
#define TFC_MAX_PLANES 4
#define TFC_WPAD 16           // slack k-substeps at the end of a packed weight stream (prefetch distance headroom)
#define TFC_PART_WS_FLOATS (8 << 20)   // floats of the per-stream partial-sum scratch every reducing entry point takes (32 MiB; include/tfc_gan.h)
#define TFC_SN_BWD_PARTS 128           // workgroup partials (doubles) of the spectral-norm backward's dot product

struct TfcPlane {
  int dy0, dx0;               // halo origin relative to the tile origin, in plane coordinates
  int py, px;                 // source = plane*SS + (py,px)
  int hh, hw;                 // halo rows / cols actually used (<= TFC_MAX_HH / TFC_MAX_HW)
  int ntaps;
  int pad_;
  int tap_dy[TFC_MAX_TAPS];   // tap position inside the halo (>= 0)
  int tap_dx[TFC_MAX_TAPS];
  int tap_mask[TFC_MAX_TAPS]; // bit (ky*4+kx) set for every 4x4 filter tap of the torch weight this gather tap multiplies
                              // (one bit normally; several when duplicated taps of an upsampled input are collapsed: their weights add)
};

struct TfcGather {
  int IH, IW, in_pitch, SS;   // source tensor (NHWC, pitch in elements), source stride 1 or 2
  int Cin_pad;                // gathered channels, multiple of 8
  int GH, GW;                 // gather grid per image
  int tiles_y, tiles_x, nimg;
  int nplanes;
  int OH, OW, OS, OOY, OOX;   // output tensor dims, output stride / offset (sub-pixel phases)
  int out_pitch, Nout;        // output pixel pitch (elements), real output channels
  int ph_n;                   // sub-pixel phases folded into ONE launch (1 or 4): phase (py,px) = (ph >> 1, ph & 1)
  int ph_d0, ph_oo;           // per phase bit: shift of the halo origin (dy0/dx0) and of the output offset (OOY/OOX)
  int reflect;                // 1: nn.ReflectionPad2d(1) instead of zero padding (TFC_OP_CONV3R): source row -1 reads row 1, row IH reads row IH - 2 (columns
                              // alike); every halo stage a 3 x 3 shape reaches applies tfc_reflect1 to the SOURCE coordinate, so a tile border never reflects
  struct TfcPlane plane[TFC_MAX_PLANES];
};

// The reflect rule of TfcGather::reflect, per axis: only the one-pixel ring is remapped (a halo pixel further out serves outputs past the image
// alone and stays zero). n >= 2; with n == 2 both borders land on the image's own two rows.
static inline __host__ __device__ int tfc_reflect1(int v, int n) { return v == -1 ? 1 : (v == n ? n - 2 : v); }

// Derived constants (host and device agree through these helpers).
static inline __host__ __device__ int tfc_pb(int cin_pad, int es) { int b = cin_pad * es; return b < 64 ? b : 64; }  // chunk bytes per pixel
static inline __host__ __device__ int tfc_ps(int pb) { return pb == 16 ? 16 : pb + 16; }                             // LDS pixel stride (bytes)
static inline __host__ __device__ int tfc_nsub(int ntaps, int pb) { return ntaps * (pb >> 4) / 2; }                  // k-substeps of one plane per chunk

// fused normalisation / activation / blur-pool kernels (elementwise.hip)
struct ActParams {
  int N, H, W, C;            // pre-pool tensor dims (x)
  int Ho, Wo;                // post-pool dims (== H,W when pool == 0 or 1)
  int x_pitch, o_pitch;      // pixel pitches (elements) of x / of the pooled-side tensor
  int pool;                  // 0 none, 1 blur stride 1, 2 blur stride 2
  int norm;                  // apply InstanceNorm using stats
  float slope;               // LeakyReLU slope (0 => ReLU, 1 => identity)
  float eps;
  unsigned drop_thresh24;    // 0 => no dropout
  unsigned seed;
  float drop_scale;
};

#ifdef __cplusplus
// Host-side hooks shared by the translation units of the library. All per-THREAD (the reference calls forward from several Python
// threads; nothing in the library is process-global mutable state).
extern thread_local int g_tfc_force_cfg;          // test hook (tfc_debug_set_igemm_config): -1 = heuristic tile choice
extern thread_local int g_tfc_persistent_grid;    // test hook (tfc_debug_set_persistent_grid): 0 = occupancy x CUs, n >= 1 = at most n workgroups
extern thread_local long long g_tfc_launch_count; // kernel launches issued by the conv-class launchers on this thread (profiling join key)
#define TFC_LAUNCH(...) do { ++g_tfc_launch_count; hipLaunchKernelGGL(__VA_ARGS__); } while (0)
extern thread_local int g_tfc_batch_invariant;    // tfc_set_batch_invariant: launch plans from the per-image geometry alone

// Launch plan of one convolution pass: what the launchers choose and what tfc_conv_plan_query reports (one decision function per family, igemm.hip).
// Batch-invariant mode evaluates every rule at TFC_REF_BATCH images on TFC_REF_CUS compute units -- the batch and the chip the forms were tuned at.
#define TFC_REF_BATCH 32
#define TFC_REF_CUS 256
enum {
  TFC_K_IGEMM = 0, TFC_K_IGEMM2 = 1, TFC_K_CONV_C8 = 3,                                               // forward / dgrad gather GEMM (profiles record the ids: 2 stays free)
  TFC_K_WGRAD = 10, TFC_K_WGRAD22 = 11, TFC_K_WGRAD_C8 = 12, TFC_K_WGRAD_X3 = 13,                     // weight gradient
  TFC_K_WGRADT_UP = 14, TFC_K_WGRADT = 15, TFC_K_WGRADT2 = 16, TFC_K_WGRAD_HEAD = 17,
  TFC_K_FIRST_FWD = 20, TFC_K_FIRST_BWD = 21                                                            // fused first block
};
struct TfcConvPlan {
  int kernel;                 // TFC_K_*
  int form;                   // tile form 0 <2,2,2,2>, 1 <2,1,2,2>, 2 <1,1,4,1>, 3 <4,1,1,4>; -1 = the kernel has one form
  int nparts;                 // partial slots per image that tfc_part_reduce_kernel adds in order (0: the pass keeps no per-image sums)
  int nsplit;                 // split count over pixel tiles (weight gradients; 1 otherwise)
  int wpi;                    // workgroups per image where the kernel's slot layout depends on it (first-block backward; 0 otherwise)
  int pat;                    // compile-time tap pattern (0: table driven)
  int per;                    // tiles per workgroup where the kernel walks a fixed run of tiles (first-block kernels; 0 otherwise)
};
void tfc_plan_igemm(int dt, const TfcGather& d, int flags, int ncu, bool inv, TfcConvPlan* p);
void tfc_plan_wgrad(int dt, const TfcGather& d, int Nn_pad, bool inv, TfcConvPlan* p, int pair0);   // pair0: first pair of the round (0: what the query reports)
bool tfc_plan_wgrad_phases(int up, int N, int IH, int IW, int x_pitch, int Cin_pad, int Cout, bool have_fin, bool inv, TfcConvPlan* p);
void tfc_plan_first_block(int pass, int N, int H, int W, int ncu, bool inv, TfcConvPlan* p);
int tfc_act_grid_cap(int N, bool inv);             // elementwise.hip: grid-stride workgroups per image of the fused activation passes

// fixed-order sum of per-workgroup partials (elementwise.hip): out[g][j] += sum_p part[(g * nparts + p) * L + j]
hipError_t tfc_launch_part_reduce(const float* part, float* out, int G, int nparts, int L, hipStream_t st);

// torch-layout destination of a weight gradient, handed to the wgrad launchers: when a launch can reduce its split-K slabs straight into it
// (tfc_wgrad_reduce_fin_kernel) it sets `done` and the caller skips the separate finish pass
struct TfcWgradFin { float* grad; long long sn, sc; int accumulate; bool done; };

// Spectrum windows (losses.hip): the strides of an NCHW fp32 image (unit stride on W, C = 1 or 3) and the window grid on it. Window w is window
// kw = w % wins_per_img of image w / wins_per_img; its first pixel is row row0 + (kw / wins_x) * row_step, column (kw % wins_x) * col_step.
struct TfcWinGrid { long long bs, cs; int rs, C; int row0, row_step, col_step, wins_x, wins_per_img; };

// ---- input pipeline (input.hip): resampling plan of one (H, W) file geometry -> 2 x (out x out). The plan buffer starts with this header,
// followed by the int tables the offsets (in ints from the start of the buffer) point at: bounds[out][2] = {first source index, tap count},
// coef[out][ksize] = taps in 22-bit fixed point.
struct TfcResizeAxis { int ksize; int bounds_off; int coef_off; int in_size; };
struct TfcResizePlan { TfcResizeAxis hA, hB, v; int out; int xsplit; int H; int W; };

// ---- what crosses translation units: every launcher, planner and helper that one .hip defines and another calls, and every struct that is
// passed by value between them, is declared HERE and nowhere else; api.hip and every defining file include this header, so a definition that
// drifts from its declaration is an overload nobody defines, and the link (-z defs) refuses it.
// igemm.hip
// One launch packs every operand stream of a network: a device-resident plan (built once by the host for fixed geometry and
// fixed buffers) lists the jobs; a workgroup finds its job from the prefix sums of the unit counts.
struct TfcPackJob {
  TfcGather d;
  const float* w;
  uint4* wp;
  long long sn, sc;
  int NB32, Nreal, Creal, units;                                  // units = 16-byte units of this job
  int first_block, threads;                                       // first 256-thread workgroup of this job in the planned grid; its thread count
};
int tfc_total_substeps(const TfcGather& d, int es);
int tfc_nb32(int nout);
int tfc_nb32_padded(int nout);
size_t tfc_packed_bytes(const TfcGather& d, int es);
hipError_t tfc_launch_pack(int dt, const TfcGather& d, const float* w, const float* scale, void* wp, int Nreal, int Creal, long long sn, long long sc, hipStream_t st);
hipError_t tfc_launch_igemm(int dt, const TfcGather& d, const void* in, const void* wp, void* out, const float* bias, float* stats, float* part_ws, float* out_nchw, const float* oscale, int flags, hipStream_t st);
hipError_t tfc_launch_first_block_fwd(const void* in, int N, int IH, int IW, const void* wp, const float* bias, const float* oscale, float slope, int gform,
                                      void* out, int o_pitch, unsigned char* sign_mask, hipStream_t st);
bool tfc_conv_c8_eligible(const TfcGather& d, int flags);
hipError_t tfc_launch_conv_c8(const TfcGather& d, const void* in, const void* wp, void* out, const float* bias, const float* oscale, int flags,
                              unsigned char* sign_mask, hipStream_t st);
hipError_t tfc_launch_wgrad(int dt, const TfcGather& d, const void* dO, const void* in, float* dwacc, void* slab, int Nn_pad, int Nn_real, int Cw_real, hipStream_t st, TfcWgradFin* fin);
hipError_t tfc_launch_dgrad_rows4(const void* dy, int dy_pitch, int N, int H, int W, const float* w, int Cin, const float* oscale, int NC, float* dx, hipStream_t st);
hipError_t tfc_launch_upconv_head(const void* x, int x_pitch, int N, int H, int W, const float* w, const float* bias, int Cout, float* out, hipStream_t st);
bool tfc_launch_wgrad_phases_fused(int up, const void* x, int N, int IH, int IW, int x_pitch, int Cin_pad, const void* dy, int dy_pitch, int Cout,
                                   int Cin, float* dwacc, void* slab, hipStream_t st, hipError_t* err, TfcWgradFin* fin);
hipError_t tfc_launch_wgrad_finish(float* acc, float* grad, int Nn, int Cw, long long sn, long long sc, int accumulate, hipStream_t st);
hipError_t tfc_launch_pack_planned(int dt, const void* plan_dev, int njobs, int nblocks, hipStream_t st);
hipError_t tfc_launch_dgrad_head(const void* dy, int dy_pitch, int N, int H, int W, const float* w, int Cout, void* dx, int dx_pitch, hipStream_t st);
hipError_t tfc_launch_first_block_bwd(const TfcGather& d, const void* yact, int y_pitch, const void* dyp, int dyp_pitch, int Ho, int Wo, const void* in,
                                      void* slab, float* dwacc, float* rstats, float* part_ws, float slope, int Nn_real, int Cw_real,
                                      const unsigned char* sign_mask, TfcWgradFin* fin, hipStream_t st);
// elementwise.hip
struct SnBatch {
  const float* W[4];
  float* u[4]; float* v[4]; float* sigma2[4];
  float* us[4]; float* vs[4];                                    // per-call snapshots of u, v for the backward (nullable)
  float* s[4]; float* t[4];                                      // scratch
  int R[4], K[4];
  int n;
};
hipError_t tfc_launch_sn_step_batched(const SnBatch& b, int power_iter, float eps, hipStream_t st);
hipError_t tfc_launch_act_fwd(int dt, const ActParams& p, const void* x, const float* stats, void* out, float* stats_out, float* part_ws, hipStream_t st);
hipError_t tfc_launch_norm_add(int dt, const ActParams& p, const void* x, const float* stats, const void* res, int res_pitch, void* out, hipStream_t st);
hipError_t tfc_launch_reflect_fold(int dt, const void* e, int e_pitch, void* dx, int dx_pitch, int N, int H, int W, int C, int accumulate, hipStream_t st);
hipError_t tfc_launch_act_bwd(int dt, int mode, const ActParams& p, const void* dout, const void* x, const float* stats, float* rstats, void* dx, int use_x, int dx_pitch, float* part_ws, hipStream_t st);
hipError_t tfc_launch_act_pool2_bwd_signs(const ActParams& p, const void* dout, const unsigned char* sign_mask, float* rstats, void* dx, int dx_pitch, float* part_ws, hipStream_t st);
hipError_t tfc_launch_colsum(int dt, const void* x, long long rows, int pitch, int C, float* out, float* part_ws, hipStream_t st);
hipError_t tfc_launch_pack_nhwc8(int dt, const float* a, int Ca, const float* b, int Cb, void* out, int N, int HW, hipStream_t st);
hipError_t tfc_launch_unpack_nchw(int dt, const void* in, int pitch, int c0, int C, float* out, int N, int HW, float alpha, float beta, hipStream_t st);
hipError_t tfc_launch_tanh_bwd_pack(int dt, const float* g, const float* y, void* out, float* dbias, float* part_ws, int N, int C, int HW, hipStream_t st);
hipError_t tfc_launch_sn_bwd(const float* G, const float* W, const float* u, const float* v, const float* sigma2, float* dot_ws, float* gout, int R, int K, int accumulate, hipStream_t st);
hipError_t tfc_launch_bce_rel(int dt, const void* a, const void* b, int n, int stride, float t1, float t2, int mode, float* loss, void* da, void* db, float gscale, hipStream_t st);
hipError_t tfc_launch_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt, float gscale, hipStream_t st);
hipError_t tfc_launch_axpby(float* out, const float* x, const float* y, long long n, float a, float b, hipStream_t st);
hipError_t tfc_launch_dropout_mask(unsigned char* out, long long n, unsigned seed, unsigned thresh24, hipStream_t st);
hipError_t tfc_launch_cast(int dt, int to_f32, const void* x, void* y, long long n, hipStream_t st);
hipError_t tfc_launch_head_fwd(int dt, const void* x, int x_pitch, const float* w, void* y, int y_pitch, int N, int H, int W, int C, hipStream_t st);
// losses.hip
hipError_t tfc_launch_patch_triplet(int grid, const float* fake, const float* real, const int* neg_idx, int N, int C, float margin, float eps, float* loss, float* dfake, float gscale, hipStream_t st);
hipError_t tfc_launch_spectrum(const float* img, const TfcWinGrid& g, int S, int H, bool rect, int nwin, float* amp, float* pha, int shift, void* ws, hipStream_t st);
size_t tfc_fft_ws_bytes(int S, int H, int nwin);
hipError_t tfc_launch_l1_sum(const float* a, const float* b, long long n, float scale, float* out, hipStream_t st);
hipError_t tfc_launch_batch_kl(const float* af, const float* pf, const float* ar, int N, long long M, float scale, float* out, hipStream_t st);
hipError_t tfc_launch_batch_kl_stats(const float* af, const float* pf, const float* ar, int N, long long M, void* rec, hipStream_t st);
hipError_t tfc_launch_batch_kl_merge(const void* recs, int world, long long M, void* glob, hipStream_t st);
hipError_t tfc_launch_batch_kl_terms(const float* af, const float* pf, const float* ar, int N, long long M, const void* glob, float scale, float* out,
                                     hipStream_t st);
hipError_t tfc_launch_logmag_mse(const float* a, const float* b, int S, int nwin, float* out, int absolute, hipStream_t st);
hipError_t tfc_launch_vectorize_temps(const float* x, long long bs, int rs, int N, int H, int W, const float* lut, float* out, hipStream_t st);
hipError_t tfc_launch_row_triplet(const float* a, const float* p, const float* ng, long long rows, int W, float margin, float eps,
                                  float* loss, hipStream_t st);
// probe.hip
hipError_t tfc_launch_probe(float* out, hipStream_t st);
// metrics.hip
int tfc_moments_groups(long long count);
void tfc_ssim_tiles(int H, int W, int wy, int wx, int* tx, int* ty);
hipError_t tfc_launch_pair_moments(const uint8_t* a, const uint8_t* b, long long a_stride, long long b_stride, long long count, int N, long long* ws,
                                   long long* mom, double* psnr, double* ncc, hipStream_t st);
hipError_t tfc_launch_ssim(const uint8_t* a, long long a_is, int a_rs, const uint8_t* b, long long b_is, int b_rs, int N, int H, int W, int wy, int wx,
                           double data_range, double* ws, double* out, hipStream_t st);
hipError_t tfc_launch_hist_color(const uint8_t* img, long long img_stride, long long pix_stride, long long chan_stride, long long npix, int N, unsigned* hist,
                                 hipStream_t st);
hipError_t tfc_launch_hist_joint(const uint8_t* a, const uint8_t* b, long long a_stride, long long b_stride, long long count, int N, const uint8_t* lut_a,
                                 const uint8_t* lut_b, int nb, unsigned* hist, hipStream_t st);
hipError_t tfc_launch_mi_lut(const long long* mom, int N, int nb, int edge_f32, uint8_t* lut_a, uint8_t* lut_b, hipStream_t st);
hipError_t tfc_launch_bhattacharyya(const unsigned* h1, const unsigned* h2, int N, int nbins, double* out, hipStream_t st);
hipError_t tfc_launch_mutual_information(const unsigned* hist, int N, int nb, double* out, hipStream_t st);
// stn.hip
hipError_t tfc_launch_affine_warp_fwd(const float* src, const float* theta, float* out, int N, int C, int H, int W, int sac, hipStream_t st);
hipError_t tfc_launch_affine_warp_bwd(const float* src, const float* theta, const float* gout, float* dtheta, float* dsrc, float* part_ws, int N, int C, int H, int W, int sac, hipStream_t st);
hipError_t tfc_launch_morph_grad_fwd(const float* x, float* out, unsigned char* arg, long long planes, int H, int W, hipStream_t st);
hipError_t tfc_launch_morph_grad_bwd(const float* gout, const unsigned char* arg, float* dx, long long planes, int H, int W, hipStream_t st);
hipError_t tfc_launch_row_triplet_grad(const float* a, const float* p, const float* ng, long long rows, int W, float margin, float eps, float gscale,
                                       float* loss, float* da, hipStream_t st);
// vit.hip
hipError_t tfc_launch_vit_gemm(int dt, const TfcVitGemm& g, float* part_ws, hipStream_t st);
hipError_t tfc_launch_vit_ln_fwd(const float* x, const float* g, const float* b, float* y, float* mean, float* rstd, int rows, int D, float eps, hipStream_t st);
hipError_t tfc_launch_vit_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, const float* dres, float* dx,
                                 float* dgb, int rows, int D, float* part_ws, hipStream_t st);
hipError_t tfc_launch_vit_colsum(const float* v, long long ld, int rows, int L, const float* x_ln, const float* mean, const float* rstd, float* out,
                                 float* part_ws, hipStream_t st);
hipError_t tfc_launch_vit_attn_fwd(int dt, const float* qkv, float* out, float* probs, int N, int T, int H, float scale, hipStream_t st);
hipError_t tfc_launch_vit_attn_tiled_fwd(int dt, const float* qkv, float* out, float* stats, int N, int T, int H, float scale, hipStream_t st);
hipError_t tfc_launch_vit_attn_tiled_bwd(int dt, const float* dout, const float* qkv, const float* stats, float* dqkv, float* ws, int N, int T, int H,
                                         float scale, hipStream_t st);
hipError_t tfc_launch_vit_attn_bwd(int dt, const float* dout, const float* qkv, const float* probs, float* dqkv, int N, int T, int H, float scale,
                                   hipStream_t st);
hipError_t tfc_launch_vit_tokens_fwd(float* x, const float* cls, const float* pos, int N, int T, int D, hipStream_t st);
// input.hip
hipError_t tfc_launch_pair_resize(const uint8_t* src, long long img_stride, int row_stride, int N, const TfcResizePlan& p, const int* plan,
                                  uint8_t* tmp, const float* lut, float* A, float* B, float* TB, uint8_t* A8, uint8_t* B8, hipStream_t st);
// lpips.hip
hipError_t tfc_launch_lpips_input(int dt, const float* x, const float* shift, const float* scale, void* out, int N, int C, long long HW, int pitch, hipStream_t st);
hipError_t tfc_launch_lpips_input_bwd(int dt, const void* g, const float* scale, float* dx, int N, int C, long long HW, int pitch, float alpha, int accumulate, hipStream_t st);
hipError_t tfc_launch_maxpool2(int dt, int bwd, const void* x, const void* dy, void* out, int N, int H, int W, int C, hipStream_t st);
hipError_t tfc_launch_relu_bwd(int dt, const void* dy, const void* y, const void* extra, void* dz, long long n, hipStream_t st);
hipError_t tfc_launch_lpips_head(int dt, const void* fx, const void* fy, const float* w, float* out, void* dfx, float* part_ws, int N, long long HW, int C, float gscale, hipStream_t st);
// debias.hip: the <= TFC_AUX_MAXC head rows travel in the kernels' argument block
#define TFC_AUX_MAXC 16
struct TfcAuxRows { const float* w[TFC_AUX_MAXC]; const float* b[TFC_AUX_MAXC]; };
struct TfcAuxGradRows { float* w[TFC_AUX_MAXC]; float* b[TFC_AUX_MAXC]; };
struct TfcCeHeads { int nc[3]; int off[3]; float w[3]; float scale; };
hipError_t tfc_launch_pack_labels(int dt, const float* img, const float* labels, const float* fw, const float* fb, void* out, int N, int HW, hipStream_t st);
hipError_t tfc_launch_label_plane_bwd(const float* g, long long gs, const float* labels, float* dw, float* db, int N, int HW, int accumulate, hipStream_t st);
hipError_t tfc_launch_aux_heads_fwd(int dt, const void* x, const TfcAuxRows& rows, int ct, float* logits, float* part_ws, int N, int HW, hipStream_t st);
hipError_t tfc_launch_aux_heads_dgrad(float* g, long long gs, const TfcAuxRows& rows, int ct, const float* dl, int N, int HW, hipStream_t st);
hipError_t tfc_launch_aux_heads_wgrad(int dt, const void* xr, const float* dlr, const void* xf, const float* dlf, const TfcAuxGradRows& rows, int ct,
                                      int N, int HW, int accumulate, hipStream_t st);
hipError_t tfc_launch_softmax_ce_heads(const float* logits, const int* targets, const TfcCeHeads& a, int ct, int N, float* probs, float* losses,
                                       float* dlogits, hipStream_t st);
int tfc_aux_fwd_nparts(int HW);
// mask.hip
long long tfc_mask_nblk(int N, int H, int W);
int tfc_mask_stats_floats(void);
hipError_t tfc_launch_mask_fwd(const float* img, float* lap, float* bl, void* ws, int N, int H, int W, hipStream_t st);
hipError_t tfc_launch_mask_scale(const float* bl, const void* ws, float* mask, long long total, hipStream_t st);
hipError_t tfc_launch_mask_bwd(const float* lap, const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf,
                               float* dmn, float* dimg, int N, int H, int W, hipStream_t st);
hipError_t tfc_launch_mask_phase_f1(const float* img, float* lap, void* ws, void* rec, int N, int H, int W, hipStream_t st);
hipError_t tfc_launch_mask_phase_f2(const float* lap, float* bl, void* ws, void* rec, int N, int H, int W, hipStream_t st);
hipError_t tfc_launch_mask_merge(void* ws, const void* recs, int world, int which, hipStream_t st);
hipError_t tfc_launch_mask_phase_b0(const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf, void* rec, int N, int H,
                                    int W, hipStream_t st);
hipError_t tfc_launch_mask_phase_b1(const float* lap, const float* bl, void* ws, const float* dout, float* dmn, void* rec, int N, int H, int W, hipStream_t st);
hipError_t tfc_launch_mask_phase_b2(const float* lap, const void* ws, const float* dmn, float* dimg, int N, int H, int W, hipStream_t st);
hipError_t tfc_launch_pack_plane(int dt, const float* img, const float* plane, const float* Mdev, void* out, int N, int HW, hipStream_t st);
#endif
