/*
 * tfc_gan.h -- C ABI of libtfcgan_hip.so: the MI355X (gfx950) kernels of the TFC-GAN PATCH-16 training hot path.
 *
 * The reference (nudro/TFC-GAN) has NO native or FFI layer: its hot path is the PyTorch op sequence inside
 * TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_16P.py ("P16" below), lines 545-638.  Each entry point here replaces one
 * stock-op sequence of that script; the host-side mirror of the reference's Python surface (GeneratorUNet,
 * Discriminator1, make_16_patches, ...) lives in tfc-gan_amd/ and binds these symbols with ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named *_host; `stream` is a hipStream_t passed as void* (0 = null stream);
 *   - activations are NHWC with an explicit pixel pitch (elements), dtype `dt` (TFC_DT_BF16 storage / fp32 accumulate,
 *     or TFC_DT_F32 = exact-fp32 parity mode using v_mfma_f32_32x32x2_f32); channel counts that are gathered or
 *     produced by MFMA tiles are padded to a multiple of 8 by the caller (3 -> 8, 6 -> 8, 1 -> 8);
 *   - weights / gradients / statistics / losses are fp32 in the torch layouts of the reference's state_dict;
 *   - return value 0 = success, otherwise a negative code; tfc_last_error() gives the thread-local message.
 *     No entry point allocates, frees or synchronises (all are hipGraph-capturable).
 *   - DETERMINISM: no entry point of the training path adds floats with atomics. Sums that cross workgroups (InstanceNorm statistics, their
 *     backward reductions, bias gradients, spectral-norm products, split-K weight gradients) leave every workgroup as a partial in a
 *     FIXED slot of a scratch buffer and are added in a fixed order behind the kernel: the same inputs give the same bits on every run.
 *     Entry points that reduce therefore take `part_ws`: tfc_part_ws_floats() floats (32 MiB) of device scratch that only launches
 *     of ONE stream use at a time (the Python side keeps one per (device, stream)); contents are undefined between calls.
 */
#ifndef TFC_GAN_H
#define TFC_GAN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TFC_DT_BF16 0
#define TFC_DT_F32 1
/* TFC_DT_BF16X3: fp32 storage (every layout, pitch and scratch size as TFC_DT_F32), fp32 results on the bf16 matrix cores. The convolution
 * family (tfc_conv_pack, the pack plan, tfc_conv_fwd, tfc_conv_dgrad, tfc_conv_wgrad) splits each fp32 operand value a into hi = bf16_rn(a),
 * lo = bf16_rn(a - hi) and accumulates hi*hi + hi*lo + lo*hi in fp32: at most 2^-16 (3 + 2^-7) |a b| of error per product. Every other entry
 * point that takes TFC_DT_F32 takes it and computes as in TFC_DT_F32; the bf16-only entry points (first block, generator head kernels,
 * tfc_conv_dgrad_image) and the tfc_vit_* kernels refuse it. Non-finite inputs stay non-finite. */
#define TFC_DT_BF16X3 2

/* convolution ops of the path */
#define TFC_OP_CONV 0     /* nn.Conv2d(k4,s1,p1)                              P16:105 (UNetDown), :189 (Discriminator1 blocks) */
#define TFC_OP_PADCONV 1  /* nn.ZeroPad2d((1,0,1,0)) + nn.Conv2d(k4,p1)       P16:201-202 (PatchGAN head)                    */
#define TFC_OP_CONVT 2    /* nn.ConvTranspose2d(k4,s2,p1)                     P16:122 (UNetUp)                               */
#define TFC_OP_UPCONV 3   /* nn.Upsample(x2)+nn.ZeroPad2d((1,0,1,0))+nn.Conv2d(k4,p1) [+Tanh]   P16:153-158 (generator head)  */
#define TFC_OP_CONV3 4    /* nn.Conv2d(k3,s1,p1): VGG16 features of criterion_lpips (P16:70-73, :598). Weights are passed zero-padded to
                             [Cout][Cin][4][4] (filter in rows / columns 0..2); forward and input gradient only (frozen network)          */
#define TFC_OP_CONV2 5    /* nn.Conv2d(k4,s2,p1): the pix2pix PatchGAN blocks of TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py:370-423. H and W even
                             (an odd size is refused), output H/2 x W/2, weights [Cout][Cin][4][4]; forward (four source parity planes in one gather),
                             input gradient (four output phases in one launch), weight gradient (bf16: the transposed convolution's phase-fused
                             launch with the two tensors exchanged; fp32 / bf16x3: one launch per parity plane into disjoint filter taps; slabs
                             added in a fixed order, no float atomics); every compute mode                                                 */
#define TFC_OP_CONV3R 6   /* nn.ReflectionPad2d(1) + nn.Conv2d(C, C', 3)  (cyclegan_og/models.py:34-35, :38-39): the residual blocks of CycleGAN's
                             GeneratorResNet. Output H x W; weights as for TFC_OP_CONV3 ([Cout][Cin][4][4], filter in rows / columns 0..2) and the same
                             channel-byte rule; H >= 2 and W >= 2 (smaller is refused, as torch refuses it). Per axis source coordinate -1 reads 1 and H
                             reads H - 2, at the IMAGE border only. Every compute mode, all three passes: forward (TFC_EP_BIAS | TFC_EP_STATS |
                             TFC_EP_RELU), weight gradient (the forward's reflect halo; slabs added in a fixed order; the seven unused taps of the slot
                             are written as zeros, or kept under `accumulate`), input gradient = the EXACT adjoint: the TFC_OP_CONV3 taps on the
                             (H + 2) x (W + 2) grid of the padded input into scratch, then a fold pass that adds the one-pixel ring into the pixels the
                             forward read it from (corners fold on both axes) and honours TFC_EP_ACCUM. The scratch: tfc_conv_dgrad_set_ws. No atomics */

/* epilogue flags of tfc_conv_fwd / tfc_conv_dgrad */
#define TFC_EP_BIAS 1       /* + bias[Cout]                                                                                   */
#define TFC_EP_STATS 2      /* stats[N][Cout][2] += (sum, sum of squares) of the result: nn.InstanceNorm2d statistics, P16:107 (needs part_ws) */
#define TFC_EP_ACCUM 4      /* result += existing output (skip-connection gradient accumulation, torch.cat backward P16:133)  */
#define TFC_EP_TANH_NCHW 8  /* nn.Tanh (P16:157) and store fp32 NCHW to `out_nchw`                                            */
#define TFC_EP_LEAKY 16     /* nn.LeakyReLU(0.2) of Discriminator1 (P16:190) applied to the result before it is stored          */
#define TFC_EP_RELU 32      /* nn.ReLU applied to the result before it is stored (VGG16 feature stack of LPIPS)                    */

const char* tfc_last_error(void);
int tfc_abi_version(void);
size_t tfc_part_ws_floats(void);   /* size (floats) of the per-stream partial-sum scratch `part_ws` */

/* ---- weights ------------------------------------------------------------------------------------------------- */
/* pass: 0 = forward operand stream, 1 = dgrad operand stream.  w is the torch-layout fp32 weight
 * (Conv2d [Cout][Cin][4][4]; ConvTranspose2d [Cin][Cout][4][4]); *scale (nullable device scalar) multiplies every
 * element (1/sigma of spectral_norm, P16:188).  Replaces the implicit weight cast of torch.cuda.amp.autocast. */
size_t tfc_conv_packed_bytes(int dt, int op, int pass, int Cin, int Cout);
int tfc_conv_pack(void* stream, int dt, int op, int pass, const float* w, const float* scale, void* packed, int Cin, int Cout);

/* Planned packing: all operand streams of a network in ONE launch. Build the job table once on the host (geometry, weight and
 * stream pointers are fixed for the lifetime of an engine), copy it to the device, then call tfc_conv_pack_planned per update. */
size_t tfc_pack_plan_bytes(int nlayers);
int tfc_pack_plan_build(int dt, int nlayers, const int* ops_host, const int* passes_host, const float* const* w_host,
                        void* const* packed_host, const int* Cin_host, const int* Cout_host, void* plan_host, int* nblocks_host);
int tfc_conv_pack_planned(void* stream, int dt, const void* plan_dev, int njobs, int nblocks);

/* ---- forward: y = oscale * op(x) + bias ; x: [N][H][W][x_pitch], y: [N][OH][OW][y_pitch] (OH = H-1 | H | 2H | 2H) ---
 * oscale: nullable DEVICE scalar multiplying the accumulator before the bias -- 1/sigma of spectral_norm (P16:188), so the
 * discriminator's operand streams are packed once per weight update and not once per forward. */
int tfc_conv_fwd(void* stream, int dt, int op, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout,
                 const void* packed, void* y, int y_pitch, const float* bias, float* stats, float* out_nchw, const float* oscale, int flags,
                 float* part_ws /* nullable unless TFC_EP_STATS */);
/* ---- the FIRST convolution of either network (UNetDown(channels, 64, normalize=False) P16:140; discriminator_block(2 * channels, 64) P16:194): bf16,
 * Cin <= 8 (x: NHWC8), Cout == 64, weights-stationary kernel. Same result as tfc_conv_fwd(TFC_OP_CONV) with flags in {TFC_EP_BIAS, TFC_EP_LEAKY}; in
 * addition sign_mask (nullable, 8-byte aligned): uint8 [N][H-1][W-1][8], bit c of a pixel's 64-bit word = (stored y[c] > 0) -- all that the backward of
 * the block needs of y when only its weight / bias gradient is wanted (tfc_first_block_bwd_wgrad reads 8 bytes per pixel instead of 128). */
int tfc_conv_first_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout, const void* packed, void* y, int y_pitch,
                       const float* bias, const float* oscale, int flags, uint8_t* sign_mask);
/* the whole first block forward in ONE kernel: BlurPool(stride 2)(LeakyReLU(slope)(oscale * conv(x) + bias)) -> out [N][Ho][Wo] (out_pitch), Ho = (H-2)/2+1,
 * for discriminator_block(2 * channels, 64) (P16:187-196; act_after_rounding = 0: the activation runs before the bf16 rounding, as in the conv epilogue of
 * the unfused chain) and UNetDown(channels, 64, normalize=False) (P16:140; act_after_rounding = 1: the raw conv output is rounded, the activation runs in
 * fp32 inside the pooling). The 266 MB conv output is never written; sign_mask (nullable) receives its sign words as tfc_conv_first_fwd would leave them.
 * Same numbers as tfc_conv_first_fwd + tfc_act_fwd(pool = 2) up to the fp32 summation order of the 16 blur taps (<= 1 bf16 ulp on rare elements). */
int tfc_first_block_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout, const void* packed, const float* bias,
                        const float* oscale, float slope, int act_after_rounding, void* out, int out_pitch, uint8_t* sign_mask);
/* ---- PatchGAN head forward, P16:201-202: ZeroPad2d((1,0,1,0)) + Conv2d(C,1,k4,p1,no bias) as a wave-per-pixel dot product
 * (w: torch-layout fp32 [1][C][4][4], y: [N][H][W][y_pitch] channel 0). Same result as tfc_conv_fwd(TFC_OP_PADCONV, Cout=1). */
int tfc_patchgan_head_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int C, const float* w,
                          void* y, int y_pitch);
/* generator head, P16:150-157: nn.Upsample(2) -> nn.ZeroPad2d((1,0,1,0)) -> nn.Conv2d(128, Cout <= 4, 4, padding=1) -> nn.Tanh, forward,
 * bf16 only: x [N][H][W][x_pitch] (128 channels), w torch-layout fp32 [Cout][128][4][4], out fp32 NCHW [N][Cout][2H][2W].
 * Same result as tfc_conv_fwd(TFC_OP_UPCONV, TFC_EP_BIAS | TFC_EP_TANH_NCHW); the four sub-pixel phases share one 16-wide MFMA tile. */
int tfc_upconv_head_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int Cin, int Cout, const float* w,
                        const float* bias, float* out_nchw);
/* its input gradient: dy NHWC8 [N][2H][2W][8] (Cout <= 8 real channels) -> dx NHWC [N][H][W] channels [0,128) at dx_pitch, overwritten.
 * w: the fp32 torch-layout filter [Cout][128][4][4] (the collapsed taps are summed in fp32 and rounded to bf16 once, as in the forward). */
int tfc_upconv_head_dgrad(void* stream, int dt, const void* dy, int dy_pitch, int N, int H, int W, int Cin, int Cout, const float* w, void* dx, int dx_pitch);

/* input gradient of the FIRST discriminator convolution (nn.Conv2d(Cin, 64, 4, stride 1, padding 1), P16:188) w.r.t. its first `nch`
 * (<= 4) input channels -- the generated image inside cat(img_A, img_B), P16:205 -- written as fp32 NCHW [N][nch][H][W]; bf16 only.
 * dy: [N][H-1][W-1][dy_pitch] (64 channels), w: torch-layout fp32 [64][Cin][4][4], oscale: nullable device scalar (1/sigma).
 * Same numbers as tfc_conv_dgrad(TFC_OP_CONV) + tfc_unpack_nchw restricted to those channels. */
int tfc_conv_dgrad_image(void* stream, int dt, const void* dy, int dy_pitch, int N, int H, int W, int Cin, int Cout, const float* w,
                         const float* oscale, int nch, float* dx_nchw);

/* ---- input gradient: dx = oscale * op^T(dy) (flags: TFC_EP_ACCUM) ------------------------------------------------ */
int tfc_conv_dgrad(void* stream, int dt, int op, const void* dy, int dy_pitch, int N, int H, int W, int Cin, int Cout,
                   const void* packed, void* dx, int dx_pitch, const float* oscale, int flags);
/* Scratch of the TFC_OP_CONV3R input gradient: tfc_conv_dgrad_ws_bytes() bytes (0 for every other op) = the padded gradient [N][H+2][W+2][pad8(Cin)]
 * in the storage type; contents undefined between calls. tfc_conv_dgrad keeps its signature, so the buffer is registered per calling THREAD (as the
 * test hooks are) and read at each TFC_OP_CONV3R call of that thread: 16-byte aligned, used by the launches of one stream at a time; the call refuses
 * a missing or smaller buffer. ws = NULL withdraws it. Nothing is allocated or synchronised. */
size_t tfc_conv_dgrad_ws_bytes(int dt, int op, int N, int H, int W, int Cin, int Cout);
int tfc_conv_dgrad_set_ws(void* ws, size_t bytes);
/* ---- weight gradient: dw (torch layout, fp32) = or += x (*) dy ; ws: tfc_conv_wgrad_ws_bytes() of scratch = [64 MiB of split-K
 *      slabs | fp32 accumulator]. Zero it once after allocation: the accumulator part must be ALL ZERO on entry and is left all
 *      zero on return (the slab part is scratch). One buffer sized for the largest layer may be shared by every layer. The slabs
 *      hold the partial sums of 512 workgroups in every compute mode; a layer with more (output-block, input-block) pairs than that
 *      runs in rounds of 512 pairs, each added to the accumulator in a fixed order before the next reuses the slabs. ------------ */
size_t tfc_conv_wgrad_ws_bytes(int op, int Cin, int Cout);
int tfc_conv_wgrad(void* stream, int dt, int op, const void* x, int x_pitch, const void* dy, int dy_pitch, int N, int H, int W,
                   int Cin, int Cout, void* ws, float* dw, int accumulate);

/* ---- fused normalisation / activation / anti-aliased pooling ------------------------------------------------------
 * forward  : y = Dropout( Blur_{pool}( Act_{slope}( norm ? InstanceNorm(x; stats) : x ) ) )      P16:106-111, :123-128, :191-192
 *   pool: 0 none, 1 antialiased_cnns.BlurPool(stride=1), 2 BlurPool(stride=2) (reflect pad 1/2, [1,3,3,1]^2/64)
 *   slope: 0.2 LeakyReLU, 0 ReLU, 1 identity; stats: [N][C][2] (sum, sumsq) of x over H*W; eps 1e-5, biased variance
 *   stats_out (nullable): [N][C][2] += (sum, sumsq) of y  (InstanceNorm that FOLLOWS the blur in UNetUp)
 *   dropout: drop_p in [0,1): counter-based mask of (seed, element index), identical in forward and backward
 * backward : mode 0: dx = g'            (norm == 0); rstats (nullable) = float[N][C] += per-image column sums of dx = the bias gradient of the
 *                     convolution that produced x (Discriminator1 blocks, P16:189)
 *            mode 1: rstats[N][C][2] += (sum g', sum g' * xhat)          (InstanceNorm backward, reduction phase)
 *            mode 2: dx = rstd * (g' - mean g' - xhat * mean(g' xhat))   (apply phase)
 *            g' = Blur^T(dropmask * dy) * Act'(xhat) ; x == NULL => Act' = 1
 *   part_ws: needed whenever stats_out (forward) or a reduction into rstats (backward mode 1, mode 0 with rstats) is requested
 *   C / (one 16-byte unit) must divide 256; every pitch (x, y, dy, dx, res) is a multiple of one 16-byte unit (8 bf16 / 4 fp32), or the call is refused
 */
int tfc_act_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, int C, const float* stats, int norm,
                float slope, int pool, float drop_p, uint32_t seed, void* y, int y_pitch, float* stats_out, float* part_ws);
/* second half of a residual block (cyclegan_og/models.py:40, :44): y = res + InstanceNorm(x; stats), one pass, stored in the storage type of dt.
 * stats [N][C][2] = (sum, sum of squares) of x as the convolution epilogue leaves them; the fp32 constants of tfc_act_fwd: m = s1 / HW,
 * var = max(s2 / HW - m^2, 0), eps 1e-5. y may alias x or res. Backward: tfc_act_bwd (norm, slope 1, pool 0) through the norm, g itself to the skip. */
int tfc_norm_add_fwd(void* stream, int dt, const void* x, int x_pitch, const void* res, int res_pitch, int N, int H, int W, int C,
                     const float* stats, void* y, int y_pitch);
int tfc_act_bwd(void* stream, int dt, int mode, const void* dy, int dy_pitch, const void* x, int x_pitch, int N, int H, int W, int C,
                const float* stats, int norm, float slope, int pool, float drop_p, uint32_t seed, float* rstats, void* dx, int dx_pitch, float* part_ws);
/* tfc_act_bwd(mode 0, pool 2, norm 0) for a 64-channel bf16 tensor x that was never stored: sign_mask = its sign words (uint8 [N][H][W][8], bit c of the
 * 64-bit word of a pixel = (x[c] > 0), as tfc_first_block_fwd / tfc_conv_first_fwd leave them). Same dx bits as tfc_act_bwd on the stored tensor. */
int tfc_act_bwd_signs(void* stream, int dt, const void* dy, int dy_pitch, const unsigned char* sign_mask, int N, int H, int W, int C, float slope,
                      float* rstats, void* dx, int dx_pitch, float* part_ws);
int tfc_dropout_mask(void* stream, uint8_t* keep, long long n, float drop_p, uint32_t seed);   /* test hook: the mask itself */

/* ---- layout plumbing at the NCHW fp32 module boundary -------------------------------------------------------------- */
int tfc_pack_nhwc8(void* stream, int dt, const float* a, int Ca, const float* b, int Cb, void* out, int N, int H, int W);   /* torch.cat((a,b),1), P16:207 */
int tfc_unpack_nchw(void* stream, int dt, const void* in, int pitch, int c0, int C, float* out, int N, int H, int W, float alpha, float beta);
/* nn.Tanh backward of the generator head (P16:157) + NHWC8 packing: dyraw = g * (1 - y^2); dbias (nullable, needs part_ws): float[C] += column sums */
int tfc_tanh_bwd_pack(void* stream, int dt, const float* g, const float* y, void* dyraw, float* dbias, int N, int C, int H, int W, float* part_ws);
/* bias gradient: out[C] += column sums of x [rows][pitch]; part_ws (nullable): lets many rows be split over workgroups.
   x 16-byte aligned, pitch >= C, C and pitch multiples of one 16-byte unit (8 bf16 / 4 fp32), as for every activation pointer */
int tfc_colsum(void* stream, int dt, const void* x, long long rows, int pitch, int C, float* out, float* part_ws);
int tfc_cast(void* stream, int dt, int to_f32, const void* x, void* y, long long n);
int tfc_axpby(void* stream, float* out, const float* x, const float* y, long long n, float a, float b);

/* ---- spectral norm: torch.nn.utils.parametrizations.spectral_norm, P16:188 ---------------------------------------- */
/* W: [R][K] fp32; u[R], v[K] updated in place when power_iter != 0 (u <- norm(W v), v <- norm(W^T u)); sigma2 = {sigma, 1/sigma} with
 * sigma = u . (W v), evaluated as (W^T u) . v after a power iteration (the same number up to fp32 round-off, one pass over W less);
 * ws: tfc_spectral_norm_batched_ws_floats(1, &R, &K) floats */
int tfc_spectral_norm_step(void* stream, const float* W, float* u, float* v, float* sigma2, float* ws, int R, int K, int power_iter);
/* the same for up to 4 layers in 3 launches (host arrays of device pointers / sizes); u_snap / v_snap (nullable arrays of
 * nullable pointers) receive copies of the updated u, v for the backward of THIS forward call; ws: ..._ws_floats() floats
 * (W^T u is formed from per-row-block partials that are added in a fixed order: no atomics) */
size_t tfc_spectral_norm_batched_ws_floats(int nlayers, const int* R_host, const int* K_host);
int tfc_spectral_norm_step_batched(void* stream, int nlayers, const float* const* W_host, float* const* u_host, float* const* v_host,
                                   float* const* sigma2_host, float* const* u_snap_host, float* const* v_snap_host,
                                   const int* R_host, const int* K_host, float* ws, int power_iter);
/* gW_orig (=/+=) (G - <G, W/sigma> u v^T) / sigma ; ws: 256 floats, 8-byte aligned (per-workgroup partials of <G, W>, added in a fixed order) */
int tfc_spectral_norm_bwd(void* stream, const float* G, const float* W, const float* u, const float* v, const float* sigma2,
                          float* ws, float* gout, int R, int K, int accumulate);

/* ---- loss heads --------------------------------------------------------------------------------------------------- */
/* 16-patch triplet ("contrastive") head: make_16_patches P16:227-253 + nn.TripletMarginLoss(margin=1,p=2) P16:75 applied
 * 16x with negatives real-patch[neg_idx_host[k]] P16:562-583.  fake/real: fp32 NCHW [N][C][256][256].
 * loss[0] = (1/16) sum_k mean(...);  dfake (nullable) = gscale * d loss / d fake. */
int tfc_patch16_triplet(void* stream, const float* fake, const float* real, const int* neg_idx_host, int N, int C,
                        float* loss, float* dfake, float gscale);
/* the same head on a grid x grid patch grid (patches of 256/grid pixels): grid 4 IS tfc_patch16_triplet (same bits); grid 2 = the four 128 x 128
 * patches of TFCGAN_multigpu_patchFFT.py:468-481, loss[0] = (1/4) sum_k mean(...).  neg_idx_host: grid*grid ints in [0, grid*grid).
 * dfake (nullable) is written for every pixel (zero where the hinge is inactive).  One kernel for both grids (tfc_patch_triplet_kernel<grid>). */
int tfc_patch_triplet(void* stream, const float* fake, const float* real, const int* neg_idx_host, int grid, int N, int C,
                      float* loss, float* dfake, float gscale);
/* spectra: ToPILImage -> convert("L") -> np.fft.rfft2 -> fftshift -> abs / arctan2, P16:271-319.
 * img: fp32 [N][C][rows][rs] window grid: S in {64,128,256}; windows per image = wins_x*wins_y tiles of S x S starting at the
 * image origin; amp/pha: [N*wins][S][S/2+1] fp32; shift != 0 applies np.fft.fftshift to both axes. */
int tfc_fft_spectrum(void* stream, const float* img, long long batch_stride, long long chan_stride, int row_stride, int C, int S,
                     int wins_x, int wins_y, int N, float* amp, float* pha, int shift, void* ws);
/* ws: tfc_fft_spectrum_ws_bytes(S, N * wins_x * wins_y) bytes of scratch (row-transformed half spectra) -> radix-4 FFT in LDS (rows, then
 * columns; S = 128 = 4^3 * 2 adds one radix-2 pass); ws == NULL -> direct DFT (S^2 work per output row: fine for one 64 x 64 window, 1 ms per call for 32 whole 256 x 256 images). */
size_t tfc_fft_spectrum_ws_bytes(int S, int nwin);
/* the same spectra of RECTANGULAR windows of H rows x 256 columns, H in 2 .. 256 (the regional FFT loss of TFCGAN_multigpu_patchFFT_withregion_FFT.py:353-401
 * uses H = 100): wins_per_img windows per image, window k starting at image row row0 + k * row_step, column 0. img: fp32 [N][C][img_h][row_stride] with
 * img_w >= 256 valid columns; amp/pha: [N*wins_per_img][H][129] fp32; shift != 0: ky -> (ky + H/2) % H, kx -> (kx + 64) % 129 (np.fft.fftshift, even and odd H).
 * Rows: the row pass of tfc_fft_spectrum at S = 256 with H rows (tfc_fft_rows_kernel<256, true>); columns: a direct H-point DFT with the column mean taken out. Im = +0 at kx in {0,128} x (ky = 0, ky = H/2 for even H).
 * ws: tfc_fft_spectrum_rect_ws_bytes(H, N * wins_per_img) bytes of scratch (16-byte aligned; 0 for an H outside 2 .. 256).
 * Refused (non-zero, tfc_last_error): H outside 2 .. 256, row0 + (wins_per_img - 1) * row_step + H > img_h, img_w < 256. */
int tfc_fft_spectrum_rect(void* stream, const float* img, long long batch_stride, long long chan_stride, int row_stride, int C, int img_h, int img_w,
                          int H, int row0, int row_step, int wins_per_img, int N, float* amp, float* pha, int shift, void* ws);
size_t tfc_fft_spectrum_rect_ws_bytes(int H, int nwin);
/* KL form of the regional loss (..._withregion_FFT_KL.py:400-418): log_softmax over the BATCH, KLDivLoss(reduction="mean", log_target=True). af, pf, ar:
 * fp32 [N][M] (fake amplitude, fake phase, REAL AMPLITUDE: the reference takes the target of the phase term from the real amplitudes too, :401, :404).
 * out[0] += scale * sum exp(t)(t - xa), out[1] += scale * sum exp(t)(t - xp), t = log_softmax_n(ar), xa = log_softmax_n(af), xp = log_softmax_n(pf).
 * A logged scalar (no gradient); N >= 1. Side stream only when two streams are in use, like tfc_l1_sum and the triplet heads. */
int tfc_batch_kl_sum(void* stream, const float* af, const float* pf, const float* ar, int N, long long M, float scale, float* out);
/* tfc_batch_kl_sum in phases, for a batch of world * N entries spread over `world` ranks (the softmax runs over ALL of them). Between the phases
 * the caller gathers every rank's record in rank order; nothing returns to the host, nothing is allocated. rec / recs / glob: 8-byte aligned.
 *   tfc_batch_kl_stats: first walk over this rank's N entries -> rec, float [3][M][2] = (max, sum exp(. - max)) per bin of af, pf, ar
 *   tfc_batch_kl_merge: recs, float [world][3][M][2], world in 1 .. 64 -> glob, float [3][M][2] = (max, log sum) per bin over all ranks; one workgroup,
 *                       the pairs of a bin are folded in rank order by the re-basing rule of the online log-sum-exp: the same bits on every rank
 *   tfc_batch_kl_terms: second walk with the global pairs: out[0], out[1] += scale * (this rank's terms); the mean over ranks of the results with
 *                       scale = 1 / (N * bins of a region) is the loss of the gathered batch. Stream rule of tfc_batch_kl_sum (same slots).
 * With world == 1 the three calls leave the bits of tfc_batch_kl_sum. */
int tfc_batch_kl_stats(void* stream, const float* af, const float* pf, const float* ar, int N, long long M, void* rec);
int tfc_batch_kl_merge(void* stream, const void* recs, int world, long long M, void* glob);
int tfc_batch_kl_terms(void* stream, const float* af, const float* pf, const float* ar, int N, long long M, const void* glob, float scale, float* out);
/* evaluation metric of TFC-GAN-FFT/Devcom_MagMSE.py:91-118 (mse_spec): per window MSE(log|fft2(a)|, log|fft2(b)|) over the FULL S x S
 * spectrum, computed from the half spectra amp_a / amp_b [nwin][S][S/2+1] of tfc_fft_spectrum (S in {64,128,256}); out[nwin] */
int tfc_logmag_mse(void* stream, const float* amp_a, const float* amp_b, int S, int nwin, float* out);
/* the companion metric of TFC-GAN-FFT/eval/Eurecom/Eurecom_MagOther.py:90-118 (other_spec): mean_absolute_error of the same two log-magnitude spectra */
int tfc_logmag_mae(void* stream, const float* amp_a, const float* amp_b, int S, int nwin, float* out);
/* ---- evaluation metrics ---- */
/* What the reference reads off saved PNGs with cv2 / scikit-image / numpy (TFC-GAN-FFT/eval/<set>/evaluation_psnr_ssim.py, evaluation_bhatt.py;
 * TFC-STN/evaluation/calc_NCC.py, calc_MI.py), on uint8 images that are already on the device. Every sum over pixels is an integer sum (exact, in
 * any order); the finalisers are fp64 and add in a fixed order; no float atomics. The workgroups of an image depend on its size alone, so the
 * result of a pair is the same bits in any batch. At most 65535 images of at most 2^23 elements per call. Images a / b: image n at a + n * a_stride
 * (bytes), `count` contiguous bytes each (any channel count: count = H * W * C).
 *
 * tfc_pair_moments_u8: moments[n][10] (int64) = sum a, sum b, sum a^2, sum b^2, sum ab, sum (a-b)^2, min a, max a, min b, max b.
 *   psnr (nullable) [N] = calculate_psnr of evaluation_psnr_ssim.py:56-64: mse == 0 -> 100, else 20 log10(255 / sqrt(mse));
 *   ncc (nullable) [N] = ncc of calc_NCC.py:44-64 = Pearson's r with ddof = 1 (the /255 of ToTensor cancels; a constant image gives NaN).
 *   ws: tfc_pair_moments_ws_bytes(N, count) bytes of scratch, 8-byte aligned. 128-bit loads when both bases and strides are 16-byte aligned. */
size_t tfc_pair_moments_ws_bytes(int N, long long count);
int tfc_pair_moments_u8(void* stream, const uint8_t* a, long long a_stride, const uint8_t* b, long long b_stride, long long count, int N, void* ws,
                        long long* moments, double* psnr, double* ncc);
/* skimage.metrics.structural_similarity on uint8 gray images (evaluation_psnr_ssim.py:119): uniform window of wy rows x wx columns, K1 = 0.01,
 * K2 = 0.03, sample covariance (cov_norm = NP / (NP - 1)), data_range in uint8 units (255); out[n] = mean of the SSIM map over the positions whose
 * window lies inside the image -- skimage's crop by (w - 1) / 2, which makes the filter's border mode irrelevant. (wy, wx) = (7, 7): the 2-D metric.
 * (7, 1): what the script's multichannel=True computes on a 2-D image (every column a 1-D channel): 3 rows cropped at the top and bottom only,
 * the mean over (H - 6) * W values. Rows are a_row_stride / b_row_stride bytes apart (unit stride along W). Refuses H < wy or W < wx.
 * ws: tfc_ssim_ws_bytes() bytes, 8-byte aligned (one fp64 partial per 16 x 64 output tile, added in a fixed order). */
size_t tfc_ssim_ws_bytes(int N, int H, int W, int wy, int wx);
int tfc_ssim_u8(void* stream, const uint8_t* a, long long a_img_stride, int a_row_stride, const uint8_t* b, long long b_img_stride, int b_row_stride,
                int N, int H, int W, int wy, int wx, double data_range, void* ws, double* out);
/* tfc_hist_u8, (a) colour: cv2.calcHist([img], [0, 1, 2], None, [8, 8, 8], [0, 256] * 3) of evaluation_bhatt.py:55: hist[n][c0 >> 5][c1 >> 5][c2 >> 5]
 * (uint32 [N][512], overwritten). Channel c of pixel p of image n is img[n * img_stride + p * pix_stride + c * chan_stride]: (3, 1) for HWC, (1, H * W)
 * for CHW, (1, 0) reads a gray image as R = G = B. */
int tfc_hist_u8_color(void* stream, const uint8_t* img, long long img_stride, long long pix_stride, long long chan_stride, long long npix, int N,
                      uint32_t* hist);
/* tfc_hist_u8, (b) joint: hist[n][lut_a[n][a]][lut_b[n][b]] over the `count` pixels of two gray images (uint32 [N][nb][nb], overwritten; nb <= 32);
 * lut_a / lut_b: uint8 [N][256], gray level -> bin. */
int tfc_hist_u8_joint(void* stream, const uint8_t* a, long long a_stride, const uint8_t* b, long long b_stride, long long count, int N,
                      const uint8_t* lut_a, const uint8_t* lut_b, int nb, uint32_t* hist);
/* the bin tables of np.histogram2d(a / 255, b / 255, bins = nb) on float32 pixels (calc_MI.py:59) from the min / max in `moments` (as
 * tfc_pair_moments_u8 wrote them): edges linspace(min, max, nb + 1), bins right-open except the last, range (min - 0.5, max + 0.5) when min == max.
 * edge_f32 = 0: float64 edges (numpy 1.x, the reference's); 1: float32 edges (numpy >= 2 keeps the pixels' dtype). Each edge is one multiply and
 * one add, rounded separately, as numpy's. */
int tfc_mi_bin_lut(void* stream, const long long* moments, int N, int nb, int edge_f32, uint8_t* lut_a, uint8_t* lut_b);
/* cv2.compareHist(h1, h2, HISTCMP_BHATTACHARYYA) per image: out[n] = sqrt(max(1 - sum sqrt(h1 h2) / sqrt(sum h1 * sum h2), 0)); h1, h2: [N][nbins] counts */
int tfc_bhattacharyya(void* stream, const uint32_t* h1, const uint32_t* h2, int N, int nbins, double* out);
/* mutual_information of calc_MI.py:72-82 per image: out[n] = sum over the non-zero cells of pxy log(pxy / (px py)); hist: [N][nb][nb] counts */
int tfc_mutual_information(void* stream, const uint32_t* hist, int N, int nb, double* out);

/* temperature head, P16:255-268 (vectorize_temps) over TFC-GAN-FFT/datasets_temp.py:14-35 (TempVector_PyTorch): the red channel of
 * ToPILImage(img[n]) = (uint8) trunc(x*255) (wraps mod 256) looked up in lut256 (float32(np.linspace(24,38,256)), device).
 * img: fp32 NCHW, channel 0 is read ([n*batch_stride + y*row_stride + x]); out: [N][H][W] fp32 temperatures in Celsius. */
int tfc_vectorize_temps(void* stream, const float* img, long long batch_stride, int row_stride, int N, int H, int W,
                        const float* lut256, float* out);
/* nn.TripletMarginLoss(margin, p=2, eps=1e-6) on row-major [rows][W] fp32 operands (distance over the last dim, mean over rows):
 * criterion_temp of P16:80, :595.  loss[0] = mean_rows max(margin + ||a-p+eps|| - ||a-n+eps||, 0).  Forward only (the
 * reference's temperature term carries no gradient: tensor -> PIL -> numpy, P16:263-265). */
int tfc_row_triplet(void* stream, const float* anchor, const float* positive, const float* negative, long long rows, int W,
                    float margin, float* loss);
/* out[0] (=/+=) scale * sum |a-b| : nn.L1Loss pieces of calculate_ffts, P16:323-375 */
int tfc_l1_sum(void* stream, const float* a, const float* b, long long n, float scale, float* out, int zero_first);
/* relativistic BCEWithLogits, P16:554 (mode 0) and P16:628-630 (mode 1); a,b: n logits in dt, `stride` elements apart
 * (the PatchGAN head stores its single channel at pixel pitch 8); loss fp32 scalar; da/db (nullable) = gscale * dloss. With stride == 8 the
 * WHOLE 8-channel pixel of da / db is written (gradient, seven zeros): the head's input-gradient pass reads all eight, no pre-zeroing needed */
int tfc_bce_relativistic(void* stream, int dt, const void* a, const void* b, int n, int stride, float t1, float t2, int mode,
                         float* loss, void* da, void* db, float gscale);
/* torch.optim.Adam step (P16:461-462) on flat fp32 buffers; step >= 1; gscale multiplies the gradient (1/world size) */
int tfc_adam_step(void* stream, float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps,
                  int step, float gscale);

/* ---- STN21 configuration: TFC-STN/TFCGAN_STN21_Original_NewModel3_Official.py ("STN") ---------------- */
/* Net.forward, STN:228-229: F.affine_grid(theta, size, align_corners=True) + F.grid_sample(src, grid, mode='bicubic', padding_mode='border',
 * align_corners=True), fused (the grid is never stored). src / out: fp32 NCHW [N][C][H][W]; theta: [N][2][3] (identity already added, STN:208-211). */
int tfc_affine_warp_fwd(void* stream, const float* src, const float* theta, float* out, int N, int C, int H, int W);
/* backward: dtheta[N][6] = d loss / d theta (the trainable path: theta comes from the localiser; per-workgroup partials in part_ws, added in a
 * fixed order); dsrc (nullable) = d loss / d src (a scatter: float atomics, the one order-dependent output of the library -- the STN21 step
 * never asks for it). Both are overwritten (zeroed inside). gout: d loss / d out. */
int tfc_affine_warp_bwd(void* stream, const float* src, const float* theta, const float* gout, float* dtheta, float* dsrc, int N, int C, int H, int W,
                        float* part_ws);
/* The same pair with the SAMPLING convention as an argument: the grid is F.affine_grid(align_corners=True) in both; sample_align_corners != 0 samples
 * it with align_corners=True (the bits of the pair above), 0 with align_corners=False: ix = ((gx + 1) W - 1) / 2, d ix / d gx = W / 2, taps clipped
 * one by one as above -- the mixed form of TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py:205-206. H and W may be 1 (base coordinate 0, as torch). */
int tfc_affine_warp_mode_fwd(void* stream, const float* src, const float* theta, float* out, int N, int C, int H, int W, int sample_align_corners);
int tfc_affine_warp_mode_bwd(void* stream, const float* src, const float* theta, const float* gout, float* dtheta, float* dsrc, int N, int C, int H, int W,
                             int sample_align_corners, float* part_ws);
/* morph_triplet, STN:444-449: kornia.morphology.gradient(x, [[0,1,0],[1,1,1],[0,1,0]]) = dilation - erosion with geodesic borders (neighbours
 * outside the image never win). x / out: fp32, `planes` images of H x W; arg (nullable): per pixel arg-max | arg-min << 4 for the backward. */
int tfc_morph_grad_fwd(void* stream, const float* x, float* out, uint8_t* arg, long long planes, int H, int W);
int tfc_morph_grad_bwd(void* stream, const float* gout, const uint8_t* arg, float* dx, long long planes, int H, int W);
/* criterion_morph = nn.TripletMarginLoss(margin=1.0, p=2) (STN:99, :457) over the last dim with its gradient w.r.t. the anchor:
 * loss[0] = mean_rows max(margin + ||a-p+eps|| - ||a-n+eps||, 0); danchor (nullable) = gscale * d loss / d anchor. */
int tfc_row_triplet_grad(void* stream, const float* anchor, const float* positive, const float* negative, long long rows, int W, float margin,
                         float gscale, float* loss, float* danchor);

/* ---- STN21 localiser (STN:150-201, Net.stn_phi): kornia VisionTransformer(256, patch 64, 6 channels; 768 wide, 12 pre-norm blocks of 12 heads,
 * 4x GELU MLP, LayerNorm eps 1e-6) + the fc_loc MLP, forward and backward on the matrix cores. Activations, gradients, LayerNorm statistics and
 * softmax are fp32 in every mode; dt = TFC_DT_BF16 rounds the GEMM (and attention matmul) operands to bf16, TFC_DT_F32 keeps them exact (f32 MFMA).
 * BATCH INVARIANT: no tile size, split-K count or summation order depends on the number of rows; a sample's outputs and input gradient are
 * bit-identical for any batch. No float atomics: parameter gradients (sums over rows) are chunk partials added in a fixed order (part_ws).
 *
 * tfc_vit_gemm: C(m, n) = epilogue(sum_k A(m, k) B(k, n)), M x N x K, all fp32 in memory:
 *   A: ROWS  A(m, k) = a[row(m) + k]        TRANS A(m, k) = a[row(k) + m]      UNFOLD A(m, k) = patch matrix of the images (a, a2)
 *      row(r) = a_rg > 0 ? (r / a_rg) * a_rso + (r % a_rg) * lda : r * lda  (patch rows inside the [N][17][768] token tensor)
 *   B: WEIGHT B(k, n) = b[n * ldb + k] (nn.Linear forward)   ROWS B(k, n) = b[k * ldb + n]   UNFOLD B(k, n) = patch matrix of (b, b2)
 *   C: ROWS c[row_c(m) + n] (row_c as row() with c_rg / c_rso / ldc)       UNFOLD: scatter to the NCHW images (c, c2; a NULL image is skipped)
 *   patch matrix: row m = image * patches + patch (row-major over the uh/up x uw/up grid), column k = channel * up^2 + i * up + j; channels
 *   [0, uc) of the first image, [uc, 2 uc) of the second (Conv2d(2 uc, D, up, stride up) over torch.cat((a, a2), 1) as unfold + GEMM).
 *   epilogue: + bias[n] (nullable) -> + res[row_c(m) + n] (nullable, ROWS only; may alias c) -> act -> store. act: GELU stores the
 *   pre-activation in aux[m * ldaux + n]; DACT_* multiply by the derivative of the activation whose input (GELU) / output (ReLU, Sigmoid) is
 *   aux[m * ldaux + n]. K > 4096 is split into slices of ~3072 (a function of K alone) added in slice order: needs part_ws.
 * tfc_vit_layernorm_fwd: y = LN(x) rows of D (64 | D <= 1024), saves mean / rstd [rows].
 * tfc_vit_layernorm_bwd: dx = dres (nullable) + d LN / d x; dgb (nullable) = [2][D]: (d gamma, d beta), overwritten.
 * tfc_vit_colsum: out[L] = sum over rows of v[r * ld + j] (overwritten): bias, class-token and position gradients.
 * tfc_vit_attention_fwd / _bwd: per (image, head), T <= 64 tokens, head dim 64, H heads: qkv [N][T][3][H][64] (the qkv Linear's output),
 *   out / dout [N][T][H][64], probs [N][H][T][T] (softmax(q kt * scale), written by the forward, read by the backward), dqkv like qkv.
 * tfc_vit_attention_tiled_fwd / _bwd: the same attention for 1 <= T <= 1025 tokens, tiled over 64 query rows x 64 key rows with LDS use independent
 *   of T and no T x T tensor in memory. stats [N][H][3][T] (written by the forward, read by the backward): the row maximum of the signed logits
 *   as hi + lo and the sum l of exp((logit - max) |scale|); the backward recomputes P = exp(..) / l tile by tile. ws: N * H * T floats of scratch
 *   (delta = rowsum(P dP)). Same rounding points as the pair above (bf16 mode: q, k, v, dO when loaded, the normalised P before P v and Pt dO, dS
 *   before dS k and dSt q), all products on the matrix core (fp32 mode: the logits as a compensated hi + lo dot product on the VALU).
 *   Deterministic and batch invariant: dK / dV are summed over the query tiles in tile order, no atomics.
 * tfc_vit_tokens_fwd: x[n][0] = cls + pos[0], x[n][t] += pos[t] (t >= 1), x [N][T][D]. ---- */
#define TFC_VIT_A_ROWS 0
#define TFC_VIT_A_TRANS 1
#define TFC_VIT_A_UNFOLD 2
#define TFC_VIT_B_WEIGHT 0
#define TFC_VIT_B_ROWS 1
#define TFC_VIT_B_UNFOLD 2
#define TFC_VIT_C_ROWS 0
#define TFC_VIT_C_UNFOLD 1
#define TFC_VIT_ACT_NONE 0
#define TFC_VIT_ACT_GELU 1
#define TFC_VIT_ACT_RELU 2
#define TFC_VIT_ACT_SIGMOID 3
#define TFC_VIT_DACT_GELU 4
#define TFC_VIT_DACT_RELU 5
#define TFC_VIT_DACT_SIGMOID 6
typedef struct TfcVitGemm {
  int M, N, K;
  int a_mode, a_rg;
  const float* a;
  const float* a2;
  long long lda, a_rso;
  int b_mode, c_mode;
  const float* b;
  const float* b2;
  long long ldb;
  float* c;
  float* c2;
  long long ldc, c_rso;
  int c_rg, act;
  const float* bias;
  const float* res;
  float* aux;
  long long ldaux;
  int uc, uh, uw, up;
} TfcVitGemm;
int tfc_vit_gemm(void* stream, int dt, const TfcVitGemm* g_host, float* part_ws);
int tfc_vit_layernorm_fwd(void* stream, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int rows, int D,
                          float eps);
int tfc_vit_layernorm_bwd(void* stream, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dres,
                          float* dx, float* dgb, int rows, int D, float* part_ws);
int tfc_vit_colsum(void* stream, const float* v, long long ld, int rows, int L, float* out, float* part_ws);
int tfc_vit_attention_fwd(void* stream, int dt, const float* qkv, float* out, float* probs, int N, int T, int H, float scale);
int tfc_vit_attention_bwd(void* stream, int dt, const float* dout, const float* qkv, const float* probs, float* dqkv, int N, int T, int H, float scale);
int tfc_vit_attention_tiled_fwd(void* stream, int dt, const float* qkv, float* out, float* stats, int N, int T, int H, float scale);
int tfc_vit_attention_tiled_bwd(void* stream, int dt, const float* dout, const float* qkv, const float* stats, float* dqkv, int N, int T, int H,
                                float scale, float* ws);
int tfc_vit_tokens_fwd(void* stream, float* x, const float* cls, const float* pos, int N, int T, int D);

/* ---- first block, backward, fused: UNetDown(channels, 64, normalize=False) (P16:133) and discriminator_block(2 * channels, 64) (P16:183-196) are
 * conv -> LeakyReLU -> BlurPool(stride 2) with no normalisation. When the gradient of the convolution OUTPUT is needed by nothing but the weight
 * (and bias) gradient, it is never written: = tfc_act_bwd(mode 0, pool 2) + tfc_conv_wgrad(TFC_OP_CONV) in one kernel, same bits.
 * x: NHWC8 input image [N][H][W][8]; y: the stored conv output [N][H-1][W-1] (its sign is all that is read: pre- or post-activation);
 * dy_pooled: gradient of the pooled output [N][Ho][Wo], Ho = (H-2)/2+1; dw: torch-layout gradient [Cout][Cin][4][4] (=/+=);
 * bias_sums (nullable, needs part_ws): float[N][Cout] += per-image sums of the conv-output gradient; ws: tfc_conv_wgrad_ws_bytes() of scratch (zeroed once).
 * sign_mask (nullable): the word tfc_conv_first_fwd left; when given, y is not read (and may be NULL). The transposed blur runs as a GEMM against the
 * tile's tap matrix on the matrix core: d_raw may differ from the unfused chain's by 1 bf16 ulp on rare elements (different fp32 summation order). ---- */
int tfc_first_block_bwd_supported(int dt, int Cin, int Cout);
int tfc_first_block_bwd_wgrad(void* stream, int dt, const void* x, int x_pitch, const void* y, int y_pitch, const void* dy_pooled, int dyp_pitch, int N, int H,
                              int W, int Cin, int Cout, float slope, void* ws, float* dw, int accumulate, float* bias_sums, float* part_ws,
                              const uint8_t* sign_mask);

/* ---- input pipeline: ImageDataset.__getitem__, TFC-GAN-FFT/datasets_temp.py:38-123 --------------------------
 * A decoded file is one RGB uint8 image [H][W][3] with the visible image A in columns [0, xsplit) and the thermal image B in [xsplit, W),
 * xsplit = round-half-even(W / 2) as Image.crop((0, 0, w / 2, h)) does (:54-55). Each half is resized to out x out with PIL's BICUBIC
 * resampler (:63-66; restated bit-exactly: antialiased separable convolution, 22-bit fixed-point taps, uint8 after each pass), then
 * ToTensor + Normalize(0.5, 0.5) (P16:479-482) -> fp32 NCHW, and T_B = linspace(24, 38, 256)[B red channel] (:41-42, :69-70).
 * The plan (tap tables of one file geometry) is built on the host and uploaded by the caller; all files of a batch share (H, W). */
size_t tfc_resize_plan_bytes(int H, int W, int out);
int tfc_resize_plan_build(int H, int W, int out, void* plan_host);
size_t tfc_pair_resize_ws_bytes(int N, int H, int out);
/* src: device uint8, image n at src + n * img_stride, rows row_stride bytes apart. plan_host / plan_dev: the same plan bytes on the host
 * (header) and on the device (tables). A, B: fp32 [N][3][out][out]; TB (nullable): fp32 [N][out][out]; A8 / B8 (nullable): the resized
 * uint8 images [N][out][out][3] (what PIL's resize returns, for callers that keep 8-bit copies). */
int tfc_pair_resize_normalize(void* stream, const uint8_t* src, long long img_stride, int row_stride, int N, const void* plan_host,
                              const void* plan_dev, void* ws, const float* lut256, float* A, float* B, float* TB, uint8_t* A8, uint8_t* B8);

/* ---- LPIPS term of loss_G: criterion_lpips = lpips.LPIPS(net_type='vgg', version='0.1'), P16:70-73, used at
 * P16:598 inside loss_G. lpips_pytorch is a pip dependency that is absent from the reference tree; its published algorithm is restated
 * (PARITY UNPINNED): z-score the inputs, VGG16 features at relu1_2 / 2_2 / 3_3 / 4_3 / 5_3 (3x3 convolutions = TFC_OP_CONV3 with
 * TFC_EP_RELU), channel-normalise, squared difference, 1x1 "lin" head, spatial mean, sum over layers (and over the batch: the package
 * returns torch.sum(torch.cat(res, 0), 0, True)). Activations NHWC in dt with pitch == C. ---- */
/* (x - shift[c]) / scale[c], fp32 NCHW [N][C][H][W] -> NHWC channels [0,8) of a `pitch`-channel image (C <= 8; the rest zero / untouched) */
int tfc_lpips_input_fwd(void* stream, int dt, const float* x, const float* shift, const float* scale, void* out, int N, int C, int H, int W, int pitch);
/* dx fp32 NCHW (=/+=) alpha * g[..c] / scale[c] */
int tfc_lpips_input_bwd(void* stream, int dt, const void* g, const float* scale, float* dx, int N, int C, int H, int W, int pitch, float alpha,
                        int accumulate);
/* nn.MaxPool2d(2, 2) of torchvision's vgg16.features; backward routes to the first maximum of each window */
int tfc_maxpool2_fwd(void* stream, int dt, const void* x, void* y, int N, int H, int W, int C);
int tfc_maxpool2_bwd(void* stream, int dt, const void* x, const void* dy, void* dx, int N, int H, int W, int C);
/* dz = (y > 0) ? dy (+ extra, nullable) : 0 over n elements (n % 8 == 0); dz may alias dy */
int tfc_relu_bwd(void* stream, int dt, const void* dy, const void* y, const void* extra, void* dz, long long n);
/* one LPIPS layer: out[n] += mean_pixels sum_c w[c] (fx/(|fx|+1e-10) - fy/(|fy|+1e-10))_c^2 ; dfx (nullable) = gscale * d out[n] / d fx.
 * At an all-zero fx pixel the norm term of the gradient is defined as 0: dfx_c = (gscale / HW) * 2 w[c] * (-ny_c) / 1e-10.
 * out[n] and dfx[n] have the same bits in every run and in every batch the image is part of: the workgroups of an image (their number depends on
 * H * W and C only, at most 64) leave their sums in part_ws (required; N * 64 floats at most, N <= 65535) and are added in a fixed order. */
int tfc_lpips_head(void* stream, int dt, const void* fx, const void* fy, const float* w, float* out, void* dfx, int N, int H, int W, int C,
                   float gscale, float* part_ws);

/* ---- measurement -------------------------------------------------------------------------------------------------- */
/* When enabled every gather-GEMM / wgrad launch is bracketed by hipEvents on its own stream; tfc_prof_collect()
 * (call after synchronising) sums them per kernel class: 0 = tfc_igemm_kernel family, 1 = tfc_wgrad family (+ slab reduce),
 * 2 = the wgrad finish pass, 3 = the fused first-block backward (transposed blur + weight gradient in one launch), 4 = the fold pass of the
 * TFC_OP_CONV3R input gradient (meta pass 4). */
int tfc_prof_enable(int on);
int tfc_prof_collect(int kclass, double* total_ms, double* algorithmic_flop, long long* launches);
/* per-call detail of the records gathered on this thread since the last collect (kclass 2 = the wgrad finish pass): arrays of max_records entries,
 * meta7 = {op, pass (0 fwd, 1 dgrad, 2 wgrad, 3 wgrad finish), N, H, W, Cin, Cout} per record; returns the number of records, < 0 on error.
 * The profiling state is per THREAD: enable, launch and collect from the same thread. */
int tfc_prof_records(int max_records, int* kclass, double* ms, double* algorithmic_flop, int* meta7);

/* ---- test hooks (host side, no GPU): the table-driven gather model evaluated on the CPU with the SAME descriptors and
 * the SAME packed operand stream the kernels consume.  Never called by the product path. */
int tfc_host_emulate_conv(int op, int pass, int elem_size, const float* x_host, const float* w_host, float* y_host,
                          int N, int H, int W, int Cin, int Cout);   /* pass 2 = wgrad: w_host is dy, y_host is dw */
/* force the gather-GEMM workgroup tile (0: 128 px x 128 ch, 1: x64, 2: x32; -1: heuristic) so the tests reach every variant */
int tfc_debug_set_igemm_config(int cfg);
/* A hook for tests, not an option for users (no Python wrapper, no environment variable): cap the grid of the persistent layer kernels
 * (tfc_conv_first_fwd, tfc_upconv_head_fwd, tfc_conv_dgrad_image, tfc_upconv_head_dgrad) and of the persistent gather GEMM (tfc_conv_fwd / tfc_conv_dgrad
 * in bf16) at `workgroups` >= 1, so that small shapes reach walks of several tiles and of unequal length; 0 = the default, min(tiles, occupancy x compute units). Per calling thread. The results do not depend on it. */
int tfc_debug_set_persistent_grid(int workgroups);
/* Batch-invariant mode (per calling thread; 0 = off, the default): every launch choice that shapes the arithmetic of one sample -- tile form, kernel
 * variant, InstanceNorm / bias partial slots per image, split count, workgroups per image -- is taken from the layer's per-image geometry alone (the rules
 * are evaluated at the reference batch of 32 on 256 compute units, profiling knobs of the environment ignored), so a sample's activations, statistics
 * and gradients are bit-identical whatever batch it is computed in. At batch 32 on the MI355X the plans equal the default ones. */
int tfc_set_batch_invariant(int on);
int tfc_get_batch_invariant(void);
/* Host only, launches nothing, works without a GPU: what the launchers of (dt, op, pass: 0 forward, 1 dgrad, 2 wgrad) would choose on a chip of `ncu`
 * compute units (256 on the MI355X), under the calling thread's batch-invariant setting. flags: the TFC_EP_* bits of the call, | TFC_PLAN_FIRST_BLOCK
 * for the fused first-block kernels (pass 0 / 2). Writes min(n, 8) ints -- kernel id, tile form (0: 128 px x 128 ch in 2 x 2 waves, 1: x 64, 2: x 32,
 * 3: 128 x 128 in 4 n-waves, -1: none), partial slots per image, split count (of the first round where a weight gradient runs in several), workgroups per image, tap pattern, 0 (reserved:
 * once "flushed with float atomics", which no weight gradient does any more), tiles per workgroup -- and returns 8, or a negative error. */
#define TFC_PLAN_FIRST_BLOCK 0x10000
int tfc_conv_plan_query(int dt, int op, int pass, int N, int H, int W, int Cin, int Cout, int flags, int ncu, int* out, int n);
/* device probe of the MFMA / transposing-read lane maps the kernels rely on (writes 3*64*16 floats) */
int tfc_probe_mfma(void* stream, float* out);

/* ---- label-conditioned ("debiased") 4-patch scripts: label plane of the generator, auxiliary classifier heads of the discriminator ------------
 * Reference TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_debiased.py (DB1) :146-151, :171-174 (fc + 4th input channel), :216-233 (three Linear + Softmax
 * heads on the flattened 6 x H x W discriminator input), :522 / :603-606 (CrossEntropyLoss on the softmax output). All pointers are device pointers
 * unless named *_host; image-sized pointers 16-byte aligned; H * W a multiple of 4. The heads are given as three weight pointers (torch layout
 * [C_h][6*H*W] fp32), three bias pointers and three class counts (each >= 1, at most 16 in all); outputs order the classes head after head. */
/* out [N][H][W][8] in the compute dtype: channels 0..2 = img [N][3][H][W] fp32, channel 3 = fc(labels) (labels [N][3], fc_w [H*W][3], fc_b [H*W],
 * fp32 fmas, rounded once), channels 4..7 = 0 */
int tfc_pack_nhwc8_labels(void* stream, int dt, const float* img, const float* labels, const float* fc_w, const float* fc_b, void* out, int N, int H, int W);
/* g: fp32 NCHW gradient [N][gC][H][W] whose channel `ch` is the plane's: d_fc_w[p][k] (+)= sum_n g[n][ch][p] labels[n][k], d_fc_b[p] (+)= sum_n g[n][ch][p]
 * (n ascending inside one thread) */
int tfc_label_plane_bwd(void* stream, const float* g, int gC, int ch, const float* labels, float* d_fc_w, float* d_fc_b, int N, int H, int W, int accumulate);
/* x: the packed discriminator input [N][H][W][8] (x_pitch must be 8; channels 0..2 img_A, 3..5 img_B; column c*H*W + p of a weight row).
 * logits [N][sum C_h] fp32 = bias + x . W^T: fp32 sums, per-wave partials in fixed part_ws slots. Every weight element is read once per launch. */
int tfc_aux_heads_fwd(void* stream, int dt, const void* x, int x_pitch, int N, int H, int W, const float* const* w3, const float* const* b3,
                      const int* nclass3_host, float* logits, float* part_ws);
/* probs [N][sum C_h] = per-head softmax(logits); losses[0..2] = mean_n(logsumexp(probs_h) - probs_h[y]) (the reference's double softmax),
 * losses[3] = scale * sum_h w3_host[h] * losses[h]; dlogits (nullable) = d losses[3] / d logits. targets: int32 [N][3] on the device;
 * targets_host (nullable): the same values on the host, refused when one lies outside [0, C_h). One workgroup, fixed-order sums. */
int tfc_softmax_ce_heads(void* stream, const float* logits, const int* targets, const int* targets_host, const int* nclass3_host,
                         const float* w3_host, float scale, int N, float* probs, float* losses4, float* dlogits);
/* g [N][gC][H][W] fp32 (gC >= 3): g[n][c][p] += sum_o dlogits[n][o] W[o][c*H*W + p] for c < 3 (the img_A half of the input) */
int tfc_aux_heads_dgrad(void* stream, float* g, int gC, int N, int H, int W, const float* const* w3, const int* nclass3_host, const float* dlogits);
/* dw3[h][o][c*H*W + p] (+)= sum_n dl_r[n][o] x_r[n][p][c] + sum_n dl_f[n][o] x_f[n][p][c], db3[h][o] (+)= sum_n dl_r[n][o] + sum_n dl_f[n][o]
 * (real pair first, n ascending inside one thread; x_f / dl_f nullable together), written into the torch-layout gradients directly */
int tfc_aux_heads_wgrad(void* stream, int dt, const void* x_r, const float* dl_r, const void* x_f, const float* dl_f, int x_pitch, int N, int H, int W,
                        float* const* dw3, float* const* db3, const int* nclass3_host, int accumulate);

/* ---- edge mask of the MASK-4 script (TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_experiment.py "4X" :385-390), forward and exact backward -----------
 * g = 0.299 R + 0.587 G + 0.114 B; lap = (S49(g) - 49 g) / 96 (7x7 box sum, reflect padding 3); L = |lap|; mn, mx = min, max of L over the whole
 * batch; Mn = (L - mn) / (mx - mn); Bl = gauss9(Mn) (sigma 1.6, reflect padding 4); M = max Bl over the batch; mask = Bl / M. fp32 throughout.
 * Any H, W >= 8 (N*H*W < 2^31); a constant image (mx == mn) gives NaN as in the reference. All pointers are 16-byte aligned device pointers.
 * ws: tfc_mask_ws_bytes(N, H, W) bytes that belong to ONE forward: the extrema, their tie counts and the backward's global sums live there between
 * launches (floats 0..9: mn, mx, ties(mn), ties(mx), M, ties(M), dM per tie, L1 loss, dmx per tie, dmn per tie); nothing returns to the host. */
size_t tfc_mask_ws_bytes(int N, int H, int W);
/* img [N][3][H][W] -> lap [N][H][W] (signed), bl [N][H][W] (= Bl), ws */
int tfc_mask_fwd(void* stream, const float* img, float* lap, float* bl, void* ws, int N, int H, int W);
/* mask [N][H][W] = bl / M */
int tfc_mask_scale(void* stream, const float* bl, const void* ws, float* mask, int N, int H, int W);
/* dimg [N][3][H][W] = d/d img of sum(dout * mask) (dout [N][H][W] given, ref null), or of scale * mean|mask - ref| (ref [N][H][W] given, dout null;
 * the loss is left in float 7 of ws and its gradient w.r.t. the mask in dout_buf). Exact: d/dM, d/dmx, d/dmn go to every position that attains the
 * extremum, split evenly; sign(0) = 0 through the abs; both filters run as the true adjoints of their reflect-padded forms. dmn: N*H*W floats of
 * scratch. dimg null (with ref): the loss alone. */
int tfc_mask_bwd(void* stream, const float* lap, const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf,
                 float* dmn, float* dimg, int N, int H, int W);
/* tfc_mask_fwd / tfc_mask_bwd in phases, for a batch spread over `world` ranks whose extrema and sums are those of ALL ranks' samples. Each phase
 * runs the kernels of the unsplit entry point on this rank's N samples and leaves a RECORD of TFC_MASK_RECORD_BYTES (four 64-bit words, 8-byte
 * aligned device memory); the caller gathers the records of all ranks in rank order (raw bytes) and tfc_mask_merge -- one workgroup, fixed order,
 * world in 1 .. 64 -- writes the stats floats of ws that the next phase reads, the same bits on every rank. Nothing returns to the host.
 *   F1 tfc_mask_fwd_lap : lap; record {bits(mn), ties(mn), bits(mx), ties(mx)} of this rank's |lap| (fp32 bits and 64-bit counts)
 *      merge which = 0  : floats 0..3. The smaller (larger) value wins with its count; equal values add their counts.
 *   F2 tfc_mask_fwd_blur: bl from the merged mn / mx; record {bits(M), ties(M), 0, 0}
 *      merge which = 1  : floats 4, 5. tfc_mask_scale and tfc_pack_nhwc8_plane then read the global M.
 *   B0 tfc_mask_bwd_dot : arguments as tfc_mask_bwd; record of doubles {sum |mask - ref|, sum dout Bl, 0, 0} over this rank. Float 7 receives THIS
 *                         rank's loss, scale * mean over its own samples (masks normalised globally): the mean over equal shards is the loss of
 *                         the gathered batch. With ref, dout_buf receives scale / (N H W) * sign(mask - ref).
 *      merge which = 2  : float 6 = d/dM per tie from the sum of `sum dout Bl` in rank order, the global M and its global tie count
 *   B1 tfc_mask_bwd_blur: dmn (dout: the upstream gradient, dout_buf after a B0 with ref); record of doubles {sum dMn (L - mn), sum dMn (L - mx), 0, 0}
 *      merge which = 3  : floats 8, 9 = d/dmx, d/dmn per tie from the sums over all ranks and the global tie counts
 *   B2 tfc_mask_bwd_lap : dimg = the gradient of the SUM over ranks of the ranks' losses (or of sum dout * mask) w.r.t. this rank's images; with the
 *                         1/world of a gradient mean the parameters receive the gradient of the gathered-batch loss.
 * Tie counts reach the stats as floats, exact up to 2^24: the caller keeps world * N * H * W <= 2^24. With world == 1 (one record per merge) lap, bl,
 * floats 0..9 and dimg are the bits of tfc_mask_fwd / tfc_mask_bwd. */
#define TFC_MASK_RECORD_BYTES 32
int tfc_mask_fwd_lap(void* stream, const float* img, float* lap, void* ws, void* rec, int N, int H, int W);
int tfc_mask_fwd_blur(void* stream, const float* lap, float* bl, void* ws, void* rec, int N, int H, int W);
int tfc_mask_merge(void* stream, void* ws, const void* recs, int world, int which);
int tfc_mask_bwd_dot(void* stream, const float* bl, void* ws, const float* dout, const float* ref, float scale, float* dout_buf, void* rec, int N, int H,
                     int W);
int tfc_mask_bwd_blur(void* stream, const float* lap, const float* bl, void* ws, const float* dout, float* dmn, void* rec, int N, int H, int W);
int tfc_mask_bwd_lap(void* stream, const float* lap, const void* ws, const float* dmn, float* dimg, int N, int H, int W);
/* out [N][H][W][8] in the compute dtype: channels 0..2 = img [N][3][H][W] fp32, channel 3 = plane [N][H][W] fp32 (divided by *plane_div, a device
 * float, when it is not null: Bl with its M), channels 4..7 = 0. H * W a multiple of 4. */
int tfc_pack_nhwc8_plane(void* stream, int dt, const float* img, const float* plane, const float* plane_div, void* out, int N, int H, int W);

#ifdef __cplusplus
}
#endif
#endif
