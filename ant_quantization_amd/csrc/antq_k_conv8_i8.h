// antq_k_conv8_i8.h -- conv2d in the INTEGER domain as an implicit GEMM from BYTE codes (W8A8): the kernels of
// antq_conv2d8_i8 and antq_conv2d8_i8_sk (fp32, bf16 and f16 outputs).  xq is the int8 image of an NHWC activation
// [B, H, W, C], the codes hold the weight one byte per element as [N = Cout][R][S][C] (tap-major), y is NHWC [B, Ho, Wo, N]:
//     S[(b, ho, wo), n] = sum over r, s, c of X[b, ho sh - ph + r dh, wo sw - pw + s dw, c] . v[n, r, s, c]
// with v = image_w[code] (a code >= m reads 0), X = xq + x_offset inside the image and X = 0 for a tap outside it.  Nothing
// here is a new product: with M = B Ho Wo rows and K = R S C it is k_linear8_i8's (tiled) and k_linear8_i8_sk's (split-K)
// with the im2col gather of antq_k_conv_i8.h as the A side -- the tiled body antq_k_linear8_i8_tile.h (included inside both
// kernels), i8b_sk_tile (antq_k_linear8_i8.h) and I8ConvX, shared and not copied.  C % 32 == 0 keeps a 16-byte piece of xq AND a 16-byte piece of the byte codes inside one tap: for a
// fixed n the tap-major codes are one contiguous row of K bytes, which is all the B sides ask for.  Part of libantq's batched
// translation unit (antq_batch.hip includes it); gfx950 only.
//
//   offset     x_offset = 128 serves UNSIGNED 8-bit activations (0 .. 255, a CNN's post-ReLU tensors): xq holds value - 128.
//              The MFMA sums S' = sum xq . v; the sum that is wanted is S' + 128 sum_k v[n, k] over the k that count.  A
//              piece of xq that does not count -- a tap outside the image, m >= M, k >= K -- is filled with the byte 0x80
//              instead of 0 (I8ConvX's fill word, 0x80808080), so that xq + 128 = 0 there and EVERY k of every row carries
//              the same + 128: the correction is 128 wsum[n] with wsum[n] = sum_k v[n, k] over all of K, the caller's
//              array, whatever the padding.  A codes piece with k >= K or n >= N is exact zeros on the B side, so the fill of
//              the K tail multiplies zeros.  x_offset = 0: the fill word is 0 and wsum null -- one kernel for both.
//   where      the correction is an integer add in the epilogue (acc + 128 wsum[n], one load per column and tile, a register
//              that lives only after the loop), not the accumulators' initial value: the add costs no VGPR in the loop and
//              no load before it.  Split-K: the slice blockIdx.y == 0 adds it to the partial sums it stores, k_i8_sk_finish
//              is unchanged; a DIRECT launch adds it in its epilogue.  The launcher's bound 256 I_w K < 2^31 keeps
//              |S'| + |128 wsum| inside int32 wherever it is added.
//   tiled      k_conv2d8_i8<T, TABLE, WAVES, MT>: ownership, the xq image and its swizzle, the B image (one ds_write_b128
//              per piece at slot col ^ (4 j + kg) ^ 8 (col & 1)), the XOR / TABLE decode, the MFMA step, the accumulators
//              and the epilogue are antq_k_linear8_i8_tile.h's; the A side is I8ConvX<XL, RSTEP, true> of the (WAVES, MT) tile.
//   split-K    k_conv2d8_i8_sk<T, TABLE, MT, DIRECT>: i8b_sk_tile -- two 16-byte nontemporal loads of codes per lane and
//              stage straight into the operands, three stages in flight, no LDS for weights -- with the walker started at
//              the slice's first stage (I8ConvX::seek) and row tiles of 64 in grid z, as in k_conv2d_i8_sk.  KEEP mode: a
//              piece that does not count is replaced at the LDS write, (xn & keep) | (fill & ~keep).  Slices: i8b_sk_slices.
// Bounds are k_conv2d_i8's (xq) and k_linear8_i8's (codes: row min(n, N - 1), offset min(k, K - 16) of N K bytes).
// LDS: the tiled body's and i8b_sk_tile's.  Registers and measurements: DESIGN.md 5w, profiles/int_conv8.md.
#ifndef ANTQ_K_CONV8_I8_H
#define ANTQ_K_CONV8_I8_H

#include "antq_k_conv_i8_sk.h"
#include "antq_k_linear8_i8.h"

namespace antq {

// the word of a piece of xq that does not count, for x_offset 0 / 128
static inline uint32_t conv8_fill(int x_offset) { return x_offset == 128 ? 0x80808080u : 0u; }

template <typename T, bool TABLE, int WAVES, int MT>
__global__ void __launch_bounds__(64 * WAVES) ANTQ_I8_KERNEL
k_conv2d8_i8(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
             uint32_t M, uint32_t N, uint32_t K, const ConvGeom g, const float *__restrict__ alpha_w, int per_row, int I_w,
             const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x, uint32_t fill,
             const int32_t *__restrict__ wsum)
{
    using TL = I8Tile<WAVES, MT>;
    using XS = I8ConvX<TL::XL, TL::RSTEP, true>;
    XS xs;
    xs.g = g;
    xs.fill = fill;
    xs.init(M, blockIdx.y * (uint32_t)TL::BM, threadIdx.x & 7u, threadIdx.x >> 3);
#include "antq_k_linear8_i8_tile.h"
}

template <typename T, bool TABLE, int MT, bool DIRECT>
__global__ void __launch_bounds__(256) ANTQ_I8_KERNEL
k_conv2d8_i8_sk(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
                int *__restrict__ workspace, uint32_t M, uint32_t N, uint32_t K, const ConvGeom g, const float *__restrict__ alpha_w,
                int per_row, int I_w, const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x,
                uint32_t per_slice, uint32_t fill, const int32_t *__restrict__ wsum)
{
    static_assert(16 * MT <= (int)kConvSkBM, "a row tile holds the MT tiles of 16 rows");
    const uint32_t m0 = blockIdx.z * kConvSkBM;
    I8ConvX<I8SkTile<MT>::XL, 32, true> xs;
    xs.g = g;
    xs.fill = fill;
    xs.init(M, m0, threadIdx.x & 7u, threadIdx.x >> 3, blockIdx.y * per_slice);
    i8b_sk_tile<T, TABLE, MT, DIRECT>(codes, xq, bias, y, workspace, M, N, K, alpha_w, per_row, I_w, image_w, m, alpha_x, I_x, per_slice,
                                      m0, xs, wsum);
}

}  // namespace antq

#endif  // ANTQ_K_CONV8_I8_H
