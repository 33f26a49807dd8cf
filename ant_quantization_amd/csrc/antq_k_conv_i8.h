// antq_k_conv_i8.h -- conv2d in the INTEGER domain as an implicit GEMM, straight from the packed 4-bit codes: the kernel of
// antq_conv2d4_i8 (fp32, bf16 and f16 outputs).  xq is the int8 image of an NHWC activation [B, H, W, C] (antq_quant_i8), the
// codes hold the weight as [N = Cout][R][S][C] (tap-major), y is NHWC [B, Ho, Wo, N]:
//     S[(b, ho, wo), n] = sum over r, s, c of xq[b, ho sh - ph + r dh, wo sw - pw + s dw, c] . v[n, r, s, c]
// a tap outside the image contributes 0, v = image_w[code].  With M = B Ho Wo flattened rows and K = R S C this IS
// k_linear_i8's product of an [M, K] matrix that never exists in memory, and y is its [M, N] row-major result: ownership,
// the fragment-ordered double-buffered B image, the register decode, the xq image in LDS with its swizzle, the accumulators
// and the epilogue are i8_tile (antq_k_linear_i8.h), shared and not copied.  Part of libantq's batched translation unit;
// gfx950 only.  Plain books (m <= 16) only: the pair rule ties flat neighbours and does not survive the tap-major order.
//
// The new part is the A side, I8ConvX -- the im2col gather:
//   pieces     a thread's XL = 2 MT staged pieces share the piece index p = tid & 7 and differ in the row alone, so the
//              thread keeps ONE tap walker (r, s, c0) for k = 128 stage + 16 p.  C % 32 == 0: a 16-byte piece of xq (and a
//              16-byte piece of codes) lies inside one tap; a stage may span several taps (C = 32: four) and a tap may begin
//              in the middle of a stage (C = 160).  The walker moves by 128 k per stage with carries: 128 = at C + ac and
//              at = ar S + as are decomposed ONCE at entry (wave-uniform), a step is c0 += ac, s += as, r += ar and at most
//              one carry each -- no division in the loop.
//   rows       M is decomposed once, at entry, and nowhere else: per owned row the thread keeps `origin` = the byte offset of
//              xq[b, hi0, wi0, 0] (hi0 = ho sh - ph, wi0 = wo sw - pw; as a 32-bit number it may wrap below 0 -- only sums
//              that land inside the image are used) and (hi0, wi0) packed as two int16 (the launcher's limits keep both in
//              range).  A row m >= M keeps hi0 = -32768, which no tap lifts to 0: it never counts.
//   address    per stage ONE tap offset ((r dh) W + s dw) C + c0 for all rows; per row origin + tap offset, and the test
//              hi0 + r dh < H, wi0 + s dw < W (unsigned: below 0 fails too), r < R (k < K).  Every load is unconditional:
//              a piece that does not count -- a tap outside the image, m >= M, k >= K -- reads the 16 bytes at offset c0 of
//              the tensor instead and becomes zero in registers before the LDS write, exact zeros as the padding demands
//              (antq_k_linear_i8_sk.h on why no branch goes around a load).
//   bounds     a piece that counts has 0 <= hi < H, 0 <= wi < W, c0 + 16 <= C, b < B: its 16 bytes lie inside the B H W C
//              bytes of xq; the stand-in at c0 <= C - 16 does too.  The launcher keeps B H W C below 2^31.
// Rows run over the flattened B Ho Wo: a tile may cross image and batch boundaries.  xq is read once per tap it takes part
// in (no LDS halo tile), K is not split.  One launch, no workspace, no atomics; capturable.  The split-K form for outputs of
// up to 1024 rows, which starts the same walker at a slice's first stage: antq_k_conv_i8_sk.h.
#ifndef ANTQ_K_CONV_I8_H
#define ANTQ_K_CONV_I8_H

#include "antq_k_linear_i8.h"

namespace antq {

// the geometry of a call, as the kernel takes it
struct ConvGeom {
    uint32_t H, W, C, R, S, Wo, HoWo;      // input image, taps, output image
    uint32_t sh, sw, dh, dw;               // strides, dilations
    int32_t ph, pw;                        // paddings (top, left)
};

// XL: the pieces a thread stages per stage, RSTEP: the rows between them (k_conv2d_i8: I8Tile's; antq_k_conv_i8_sk.h: 1 or 2
// pieces, 32 rows apart).  FILL: a piece that does not count becomes four copies of the word `fill` instead of zeros
// (antq_k_conv8_i8.h: 0x80808080 for an image stored as value - 128); without it the member is never set or read.
template <int XL, int RSTEP, bool FILL = false>
struct I8ConvX {
    static constexpr bool kFill = FILL;
    ConvGeom g;
    uint32_t fill;                         // (FILL) the word of a piece that does not count
    uint32_t origin[XL];                   // byte offset of xq[b, hi0, wi0, 0] (mod 2^32)
    uint32_t hw0[XL];                      // hi0 in the low, wi0 in the high 16 bits (int16 each)
    uint32_t r, s, c0;                     // the tap and channel of k = 128 stage + 16 p
    uint32_t ar, as, ac;                   // 128 k as tap rows, taps and channels

    // the walker at piece xp of `stage`: k = 128 stage + 16 xp as (r, s, c0), by division -- once, at entry (a stage past
    // the last one gives r >= R, which never counts)
    __device__ __forceinline__ ANTQ_I8_KERNEL void seek(uint32_t stage, uint32_t xp)
    {
        const uint32_t k = stage * (uint32_t)kGemmBK + 16u * xp, t0 = k / g.C;
        c0 = k % g.C;
        r = t0 / g.S;
        s = t0 % g.S;
    }

    // stage: the first one load() will be asked for (k_conv2d_i8: 0; a slice of K: its first)
    __device__ __forceinline__ ANTQ_I8_KERNEL void init(uint32_t M, uint32_t m0, uint32_t xp, uint32_t xr0, uint32_t stage = 0u)
    {
        const uint32_t at = (uint32_t)kGemmBK / g.C;
        ac = (uint32_t)kGemmBK % g.C;
        ar = at / g.S;
        as = at % g.S;
        seek(stage, xp);
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t row = m0 + xr0 + (uint32_t)(RSTEP * i);
            const uint32_t rc = min(row, M - 1u);
            const uint32_t b = rc / g.HoWo, rem = rc % g.HoWo, ho = rem / g.Wo, wo = rem % g.Wo;
            const int32_t hi0 = (int32_t)(ho * g.sh) - g.ph, wi0 = (int32_t)(wo * g.sw) - g.pw;
            origin[i] = ((b * g.H + (uint32_t)hi0) * g.W + (uint32_t)wi0) * g.C;
            hw0[i] = ((uint32_t)(row < M ? hi0 : -32768) & 0xffffu) | ((uint32_t)wi0 << 16);
        }
    }

    // The next stage's pieces (the stages are asked for in order from init's: the walker moves on after each).  KEEP: a piece
    // that does not count stays as loaded and xkeep[i] says so -- all ones, or zero -- for the caller to apply at its LDS write
    // (antq_k_linear_i8_sk.h on why); else it is zeroed here.
    template <bool KEEP>
    __device__ __forceinline__ ANTQ_I8_KERNEL void gather(const int8_t *__restrict__ xq, u32x4_t (&xn)[XL], uint32_t (&xkeep)[XL])
    {
        const uint32_t rdh = r * g.dh, sdw = s * g.dw;
        const uint32_t tap = (rdh * g.W + sdw) * g.C + c0;
        const bool kok = r < g.R;
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t hi = (uint32_t)((int32_t)(hw0[i] << 16) >> 16) + rdh, wi = (uint32_t)((int32_t)hw0[i] >> 16) + sdw;
            const bool ok = kok && hi < g.H && wi < g.W;
            const uint32_t off = ok ? origin[i] + tap : c0;
            u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(reinterpret_cast<const char *>(xq) + off);
            if constexpr (KEEP) xkeep[i] = ok ? 0xffffffffu : 0u;
            else if (!ok) v = FILL ? u32x4_t{fill, fill, fill, fill} : u32x4_t{0u, 0u, 0u, 0u};
            xn[i] = v;
        }
        c0 += ac;
        s += as;
        r += ar;
        if (c0 >= g.C) { c0 -= g.C; s++; }
        if (s >= g.S) { s -= g.S; r++; }
    }
    __device__ __forceinline__ ANTQ_I8_KERNEL void load(const int8_t *__restrict__ xq, u32x4_t (&xn)[XL])
    {
        uint32_t unused[XL];
        gather<false>(xq, xn, unused);
    }
    __device__ __forceinline__ ANTQ_I8_KERNEL void load(const int8_t *__restrict__ xq, u32x4_t (&xn)[XL], uint32_t (&xkeep)[XL])
    {
        gather<true>(xq, xn, xkeep);
    }
    // (FILL) a KEEP-mode piece as the caller writes it to LDS: as loaded where it counts, the fill word where it does not
    __device__ __forceinline__ ANTQ_I8_KERNEL u32x4_t masked(u32x4_t v, uint32_t keep) const
    {
        const uint32_t f = fill & ~keep;
        return (v & u32x4_t{keep, keep, keep, keep}) | u32x4_t{f, f, f, f};
    }
};

template <typename T, int WAVES, int MT>
__global__ void __launch_bounds__(64 * WAVES) ANTQ_I8_KERNEL
k_conv2d_i8(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
            uint32_t M, uint32_t N, uint32_t K, const ConvGeom g, const float *__restrict__ alpha_w, int per_row, int I_w,
            const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x)
{
    using TL = I8Tile<WAVES, MT>;
    I8ConvX<TL::XL, TL::RSTEP> xs;
    xs.g = g;
    xs.init(M, blockIdx.y * (uint32_t)TL::BM, threadIdx.x & 7u, threadIdx.x >> 3);
    i8_tile<T, false, WAVES, MT>(codes, xq, bias, y, M, N, K, alpha_w, per_row, I_w, image_w, m, 0, alpha_x, I_x, xs);
}

}  // namespace antq

#endif  // ANTQ_K_CONV_I8_H
