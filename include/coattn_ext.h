/*
 * coattn_ext.h -- entry points of libcoattn_hip.so after 0.22.0.  include/coattn.h declares the 78 functions of 0.22.0 and stays as
 * it is; what a later version adds is declared here, under the same conventions (every pointer a DEVICE pointer unless marked
 * "host", the caller owns every buffer, calls asynchronous on `stream`, 0 on success and < 0 with a coattn_last_error message
 * otherwise).  vqa_amd/_lib.py tables these functions in EXT_SIGNATURES, as it tables coattn.h's in SIGNATURES.
 *
 * v0.23.0: image preprocessing -- the reference's per-sample transform Resize((S, S)) -> ToTensor -> Normalize
 * (/root/reference/main.py:126) for a whole batch of decoded uint8 images of different sizes, in one launch.
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

#ifdef __cplusplus
}
#endif
#endif
