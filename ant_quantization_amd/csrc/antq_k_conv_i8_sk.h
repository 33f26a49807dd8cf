// antq_k_conv_i8_sk.h -- the integer-domain conv2d from 4-bit codes for outputs of up to 1024 rows, with K = R S C split
// across workgroups: the kernel of antq_conv2d4_i8_sk (fp32, bf16 and f16 outputs).  The contract is antq_conv2d4_i8's, letter
// for letter (include/antq.h): xq int8 NHWC, the codes tap-major [N][R][S][C], plain books, C % 32 == 0, groups = 1, S the
// exact int32 sum, the epilogue i8_sk_store, y NHWC = [M = B Ho Wo, N] row-major; the bits of y equal k_conv2d_i8's.
// k_conv2d_i8 gives a 7 x 7 output of 512 channels eight workgroups that each walk all of K (up to 4608) through LDS; here
// the split-K form of the linear (antq_k_linear_i8_sk.h) is carried over: the tile is i8_sk_tile, shared and not copied, and
// so are the finish (k_i8_sk_finish) and the slice rule (i8_sk_slices, with ceil(M / 64) row tiles).  Part of libantq's
// batched translation unit (antq_batch.hip includes it); gfx950 only.
//
//   ownership  grid x = tiles of 64 output channels n, grid y = the slices of K in whole 128-k stages, grid z = tiles of 64
//              flattened output rows (m0 = 64 blockIdx.z; k_linear_i8_sk has one).  MT = 1 / 2 / 4 tiles of 16 rows from
//              min(M, 64); four wavefronts, wavefront w owns channels n0 + 16 w .. + 15 for all MT row tiles.
//   B side     k_linear_i8_sk's exactly: for a fixed n the tap-major codes are one contiguous row of K / 2 bytes.  16 bytes per
//              lane and stage, nontemporal, three stages in flight, i8_decode_word into the operands of the stage's two MFMA
//              steps, no LDS for weights; k map 128 c + 32 kg + 16 j: the A operand of (j, kg) is piece 2 kg + j.
//   A side     the im2col gather of I8ConvX (antq_k_conv_i8.h), staged once per workgroup into the [rows][8] image -- piece p
//              of row r at 8 r + (p ^ (r & 7)) -- two images, one barrier per stage.  A thread keeps ONE tap walker for its
//              piece p = tid & 7 and per owned row (xr0 + 32 i, at most two) one origin and one packed (hi0, wi0).  The walker
//              starts at the slice's first stage: k = 128 c0 + 16 p is decomposed into (r, s, c) by division once at entry
//              (I8ConvX::seek), then moves with I8ConvX's carries.  A slice may begin inside a tap (C = 160).
//   loads      every load is unconditional from a clamped address; the zero of a tap outside the image, m >= M or k >= K is a
//              mask applied at the LDS write, not a select at the load (antq_k_linear_i8_sk.h on why).  The tile asks for two
//              stages past the slice's end: the walker goes on into the next slice's stages, or past K, where r >= R reads the
//              stand-in at offset c0 <= C - 16 -- in bounds either way, written to an image no one reads.
//   slices     DIRECT (one slice): the epilogue in registers, one launch, no workspace.  Otherwise slice s stores its int32
//              accumulators to workspace[s][m][n] with ordinary vector stores and k_i8_sk_finish, unchanged, adds them as
//              integers and runs the epilogue.  No atomics, nothing is zeroed.
// LDS and registers: i8_sk_tile's (8 / 8 / 16 KiB of xq images + 544 bytes); the walker adds about 20 VGPRs.
// Measured: profiles/int_conv4_sk.md.
#ifndef ANTQ_K_CONV_I8_SK_H
#define ANTQ_K_CONV_I8_SK_H

#include "antq_k_conv_i8.h"
#include "antq_k_linear_i8_sk.h"

namespace antq {

constexpr uint32_t kConvSkBM = 64;         // flattened output rows per row tile (grid z)

template <typename T, int MT, bool DIRECT>
__global__ void __launch_bounds__(256) ANTQ_I8_KERNEL
k_conv2d_i8_sk(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
               int *__restrict__ workspace, uint32_t M, uint32_t N, uint32_t K, const ConvGeom g, const float *__restrict__ alpha_w,
               int per_row, int I_w, const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x,
               uint32_t per_slice)
{
    static_assert(16 * MT <= (int)kConvSkBM, "a row tile holds the MT tiles of 16 rows");
    const uint32_t m0 = blockIdx.z * kConvSkBM;
    I8ConvX<I8SkTile<MT>::XL, 32> xs;
    xs.g = g;
    xs.init(M, m0, threadIdx.x & 7u, threadIdx.x >> 3, blockIdx.y * per_slice);
    i8_sk_tile<T, false, MT, DIRECT>(codes, xq, bias, y, workspace, M, N, K, alpha_w, per_row, I_w, image_w, m, 0, alpha_x, I_x, per_slice,
                                     m0, xs);
}

}  // namespace antq

#endif  // ANTQ_K_CONV_I8_SK_H
