/*
 * coattn_ext.h -- entry points of libcoattn_hip.so after 0.22.0.  include/coattn.h declares the 78 functions of 0.22.0 and stays as
 * it is; what a later version adds is declared here, under the same conventions (every pointer a DEVICE pointer unless marked
 * "host", the caller owns every buffer, calls asynchronous on `stream`, 0 on success and < 0 with a coattn_last_error message
 * otherwise).  vqa_amd/_lib.py tables these functions in EXT_SIGNATURES, as it tables coattn.h's in SIGNATURES.
 *
 * v0.23.0: image preprocessing -- the reference's per-sample transform Resize((S, S)) -> ToTensor -> Normalize
 * (/root/reference/main.py:126) for a whole batch of decoded uint8 images of different sizes, in one launch.
 * v0.24.0: the frozen VGG encoder in EVAL mode -- BatchNorm on its running statistics, the convolution bias, the ReLU and the
 * 2x2 pool in one launch per group, the first group from the image.
 */
#ifndef COATTN_EXT_H
#define COATTN_EXT_H

#include "coattn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- image preprocessing: bilinear resize to S x S, scale to [0, 1], normalise (v0.23.0; csrc/preprocess.hip) ----
 * The GPU receives the decoded pixels (a third of the bytes of the fp32 tensor at 448 px) and writes the network's input.
 *   pixels      : pixel_bytes bytes; image b is uint8 [h_b][w_b][3], RGB interleaved, rows 3 w_b bytes apart without padding,
 *                 starting at byte desc[b].offset.  No alignment is required of an image's start or of its rows (every pixel
 *                 byte is read with a one-byte load); packers put image starts on 16-byte boundaries all the same
 *   desc        : B rows of coattn_preprocess_desc, below; 8-byte aligned; read on the device only, never on the host
 *   coef        : coef_count int32: the coefficient tables, below; 4-byte aligned
 *   lut         : fp32 [3][256]: lut[c][u] is the network's value of byte u in channel c; 4-byte aligned
 *   out         : fp32 [B][3][S][S] at the element strides sB, sC, sH, sW (any: NCHW, channels-last, a view into a larger
 *                 buffer); 4-byte aligned; every element of the B images is written, nothing else is
 *   bad_images  : one int32 on the device, may be NULL; the call ADDS to it (one integer atomic per bad image), the caller
 *                 zeroes it
 *   max_h, max_w: the largest source height and width the call is to take; they size the workgroup's LDS window, and a
 *                 descriptor beyond them is bad.  coattn_preprocess_supported(B, S, max_h, max_w) must return 1
 *
 * THE ARITHMETIC IS THE CONTRACT: Pillow's Image.resize((S, S), Image.BILINEAR) on 8-bit pixels, bit for bit, then a table
 * lookup.  The device does integer arithmetic only; every float operation is the host's, in the tables.
 *   Coefficient table of one axis, `in` source samples to S outputs -- built by the HOST in IEEE double, operation by operation:
 *     scale = in / S;   fs = max(scale, 1);   support = fs;   ss = 1 / fs;
 *     output o:   center = (o + 0.5) * scale;
 *       lo = max(0, (int)(center - support + 0.5));   hi = min(in, (int)(center + support + 0.5));      (int): toward zero
 *       w_j = max(0, 1 - |(j + lo - center + 0.5) * ss|) for j = 0 .. hi - lo - 1;
 *       ww = w_0 + w_1 + ... added left to right;   k_j = w_j / ww;   K_j = (int)(0.5 + k_j * 4194304)     (4194304 = 2^22)
 *     The table is S rows of 2 + taps int32: lo, n = hi - lo, K_0 .. K_{n-1}, zeros up to `taps` (any taps >= the largest n).
 *   Two passes with a uint8 between them (the rounding to uint8 after the first pass is part of the bits):
 *     horizontal, every source row r:   t[r][x][c] = clip8((2097152 + sum_j Kx_j * p[r][lo_x + j][c]) >> 22)
 *     vertical:                         u[y][x][c] = clip8((2097152 + sum_j Ky_j * t[lo_y + j][x][c]) >> 22)
 *     in int32 (255 * sum K is about 2^30), >> arithmetic, clip8(v) = min(max(v, 0), 255).  in == S gives K = (2^22, 0): the
 *     identity.
 *   out[b][c][y][x] = lut[c][u[y][x][c]].  With lut[c][u] = ((float)u / 255 - mean_c) / std_c, each a correctly rounded fp32
 *     operation (torch: arange(256).float().div(255).sub(mean).div(std)), this is ToTensor + Normalize bit for bit.
 * One workgroup of COATTN_PREPROCESS_THREADS threads owns a band of COATTN_PREPROCESS_ROWS output rows of one image: it takes
 * the band's window of source rows from the vertical table, runs the horizontal pass of just those rows into LDS as uint8
 * [rows][S][3], then the vertical pass and the lookup out of LDS.  Adjacent bands recompute the few source rows their windows
 * share; the intermediate never reaches memory.  Same inputs, same bits, in every output layout.
 *
 * A descriptor is BAD if h or w is below 1 or above max_h / max_w, if offset < 0 or offset + 3 h w > pixel_bytes, if a taps
 * field is outside [1, COATTN_PREPROCESS_MAX_TAPS], or if a table does not lie inside coef ([tab, tab + S (2 + taps)) within
 * [0, coef_count)).  A bad image's output is all +0 and adds exactly 1 to *bad_images; its neighbours are untouched.  The
 * device never forms an address from a bad descriptor.  Table contents are the caller's: a `lo` or `n` that would leave the
 * image (or the band's LDS window) is clamped into it (memory safety, not a result), and a band whose window passes the LDS
 * rows of max_h is written as +0.
 * Supported (the query returns 1): B >= 1, 1 <= S <= COATTN_PREPROCESS_MAX_S, 1 <= max_h, max_w <= COATTN_PREPROCESS_MAX_IN,
 * B times the bands of an image below 2^31, and the window of the largest downscale inside the 160 KiB of LDS:
 *     3072 + 16 * ceil(3 S rows / 16) <= 163840,   rows = min(max_h, (int)((ROWS - 1) * s + 2 * max(s, 1) + 1) + 1),   s = max_h / S
 * (no band's window is taller than that: lo > center - support - 0.5 and hi <= center + support + 0.5).  max_w is not limited by
 * LDS.  For S = 224 that is max_h <= 3135, for S = 448 max_h <= 3109.
 * Argument errors -- an unsupported shape, a NULL pixels, desc, coef, lut or out, pixel_bytes or coef_count < 1, a misaligned
 * buffer --: -1 with a coattn_last_error message before any device work.  No allocation, no synchronisation, nothing read on
 * the host: the call can be captured into a HIP graph. */
#define COATTN_PREPROCESS_ROWS 16
#define COATTN_PREPROCESS_THREADS 256
#define COATTN_PREPROCESS_MAX_S 2048
#define COATTN_PREPROCESS_MAX_IN 8192
#define COATTN_PREPROCESS_MAX_TAPS 1024
typedef struct coattn_preprocess_desc {
  long long offset;     /* byte offset of the image's first pixel in `pixels` */
  int h, w;             /* the source's height and width */
  int tab_x, tab_y;     /* where the horizontal (w -> S) and the vertical (h -> S) table start in `coef`, in int32 elements */
  int taps_x, taps_y;   /* the tables' widths: a row is 2 + taps int32 */
} coattn_preprocess_desc;
int coattn_preprocess_supported(int B, int S, int max_h, int max_w);
int coattn_preprocess_images(const void* pixels, long long pixel_bytes, const void* desc, const void* coef, long long coef_count,
                             const void* lut, void* out, int64_t sB, int64_t sC, int64_t sH, int64_t sW, int32_t* bad_images,
                             int B, int S, int max_h, int max_w, void* stream);

/* ---- the frozen encoder in eval mode: running statistics, one launch per group (v0.24.0; csrc/encoder.hip) ----
 * Train mode (coattn.h: coattn_bn_exact_forward, 0.15.0, and the conv1 forms, 0.16.0 / 0.22.0) has to sum the batch first.  In
 * eval mode BatchNorm2d is an elementwise map with per-channel constants, so everything after the convolution rides on ONE read
 * of its output x, and the first group goes from the image to y without x ever existing.  fp32, physically [B][H][W][C]
 * (channels_last), forward only, no workspace.
 *   x            : fp32 [B][H][W][C], the convolution output (without its bias, if conv_bias is given); 16-byte aligned
 *   conv_bias    : fp32 [C] or NULL; 16-byte aligned
 *   gamma, beta  : fp32 [C], BatchNorm2d's weight and bias; 16-byte aligned
 *   running_mean, running_var : fp32 [C]; 16-byte aligned; READ ONLY -- eval mode moves no statistic
 *   y            : fp32 [B][H/2][W/2][C] (pool) or [B][H][W][C]; 16-byte aligned; every element written, nothing else; not x
 *   relu         : 0 leaves the ReLU out
 *
 * THE ARITHMETIC IS THE CONTRACT: the stock chain's bits, that is MIOpen's spatial inference kernel behind the stock
 * convolution's separate bias add.  Per channel c, once:
 *     e      = (float)eps                                   the double rounded to fp32 first
 *     a      = fabs(running_var[c] + e)                     one fp32 add; the absolute value: a negative variance gives no NaN
 *     invstd = rsqrt(a)                                     the device library's fp32 rsqrt (HIP's rsqrtf, OpenCL's rsqrt): v_rsq_f32,
 *                                                           with a small a -- a subnormal one too -- scaled by an even power of
 *                                                           two first and the result by its root.  Not the bare instruction (a
 *                                                           subnormal a gives another result) and not 1 / sqrt(a)
 * Per element, in fp32, each line one rounding:
 *     v = x + conv_bias[c]                                  only with conv_bias; without it v = x, no operation (-0 stays -0)
 *     d = v - running_mean[c]
 *     n = d * invstd
 *     t = fma(gamma[c], n, beta[c])                         one rounding
 * pool: m = max(max(t00, t01), max(t10, t11)) over the window rows 2 ho, 2 ho + 1 and columns 2 wo, 2 wo + 1 (floor mode: an odd
 * last row or column is never read), where max(a, b) = a if a > b or a is NaN, else b: a NaN wins, as in PyTorch.  The affine map
 * goes first because gamma may be negative.  relu: y = m < 0 ? 0 : m (a NaN stays).  A NaN or an infinity of one sample stays in
 * the elements and windows it belongs to.
 * Supported: what the kernels need and no more -- coattn_bn_supported's conditions (coattn.h: C a power of two in 16 .. 512, B H W
 * below 2^31, B H W C below 2^31, at least two pixels, H and W >= 2 with pool); NOT coattn_bn_exact_geometry's observed shapes, which
 * exist for the order of a sum and nothing is summed here.  coattn_conv1_bn_eval_*: Cin = 3, Cout = 64 too, and at most
 * 65535 * COATTN_CONV1_RECOMPUTE_CHUNK samples.
 *
 * coattn_conv1_bn_eval_forward: the first group.  image fp32 [B][H][W][3] and weight fp32 [64][3][3][3] = [co][ky][kx][c], both
 * 4-byte aligned; x = the 3x3 / padding-1 convolution in the stock convolution's arithmetic -- one chain of sixteen
 * v_mfma_f32_32x32x2_f32 from 0 over the 27 terms (ky, kx, c) padded to 32, in the term order coattn.h gives for
 * coattn_conv1_bn_exact_forward -- then exactly the lines above.  It is the third kernel of coattn_conv1_bn_recompute_forward with the
 * bias and the running statistics in place of the saved ones: tiles of 2 rows x 16 columns (pool) or 32 pixels, one workgroup per
 * tile and chunk of COATTN_CONV1_RECOMPUTE_CHUNK samples.  Its y is coattn_bn_eval_forward's of the x of
 * coattn_conv1_bn_exact_forward, bit for bit.  The ReLU is always applied.
 *
 * Argument errors -- an unsupported shape, a NULL pointer other than conv_bias, a misaligned pointer, y == x or y == image,
 * eps <= 0 --: -1 with a coattn_last_error message before any HIP call.  *_supported makes no GPU call.  No allocation, no
 * synchronisation: the calls can be captured into a HIP graph.
 *
 * coattn_bn_eval_probe is the developer's slow form for tools/probe_encoder_eval.py (one thread per element, no pool, no ReLU, no
 * bias), every choice of the candidate space switchable: rsqrt 0 v_rsq_f32, 1 the device library's rsqrt, 2 1 / sqrt, 3 the scaled
 * v_rsq_f32 spelled out; step 0 fma, 1 multiply then add; eps_mode 0 var + (float)eps, 1 (float)((double)var + eps). */
int coattn_bn_eval_supported(int B, int H, int W, int C, int pool, int dtype);
int coattn_bn_eval_forward(const void* x, const void* conv_bias, const void* gamma, const void* beta, const void* running_mean,
                           const void* running_var, double eps, void* y, int B, int H, int W, int C, int pool, int relu, int dtype,
                           void* stream);
int coattn_conv1_bn_eval_supported(int B, int H, int W, int Cin, int Cout, int pool, int dtype);
int coattn_conv1_bn_eval_forward(const void* image, const void* weight, const void* conv_bias, const void* gamma, const void* beta,
                                 const void* running_mean, const void* running_var, double eps, void* y, int B, int H, int W,
                                 int Cin, int Cout, int pool, int dtype, void* stream);
int coattn_bn_eval_probe(const void* x, const void* gamma, const void* beta, const void* running_mean, const void* running_var,
                         double eps, void* y, int B, int H, int W, int C, int rsqrt, int step, int eps_mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif
