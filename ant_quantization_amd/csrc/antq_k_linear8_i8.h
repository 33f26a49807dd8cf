// antq_k_linear8_i8.h -- the integer-domain linear straight from BYTE codes of W [N, K] (antq_encode8's layout, one byte per
// weight): the kernels of antq_linear8_i8 and antq_linear8_i8_sk (fp32, bf16 and f16 outputs).  The contract is
// antq_linear4_i8's with bytes in place of nibbles (include/antq.h): v[n, k] = image_w[code[n, k]] (a code >= m reads 0),
// S = sum_k xq[m, k] v[n, k] an exact int32 sum on v_mfma_i32_16x16x64_i8, the scales applied once per output.  Plain books only:
// a pair-rule byte book has no int8 image.  Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
// Everything below but the source of the A operand is shared with antq_k_conv8_i8.h: the tiled kernel's body is
// antq_k_linear8_i8_tile.h, included inside both kernels (as an inlined function it compiled to other control flow), the
// split-K kernel's is the function i8b_sk_tile; the two kernels here are those bodies with the matrix A side (I8Matrix).
//
//   decode     two kinds, chosen by the launcher from the image on the host (i8b_image_is_xor):
//              XOR    m == 256 and image[c] == c - 128 (ANT's signed int8 book): the code IS the weight plus 128, so sixteen
//                     codes become an MFMA operand with four v_xor_b32 0x80808080 -- one VALU instruction per four weights,
//                     no table, no LDS (the 4-bit kernels pay 15 VALU per 8 weights).
//              TABLE  every other plain book: a 256-byte LDS table, zero beyond m, built once per workgroup; one ds_read_u8 and
//                     a merge per weight.  The slow, general form (measured separately: profiles/int_linear8.md).
//
// k_linear8_i8<T, TABLE, WAVES, MT> -- the tiled kernel.  Ownership (a workgroup of WAVES = 2 / 4 wavefronts owns 16 MT WAVES
// rows of xq by 64 output rows n, i8_shape), the xq image and its swizzle, the MFMA step (k = 128 c + 64 j + 16 kg .. + 15 for
// lane group kg of step j), the accumulator layout and the epilogue are k_linear_i8's (antq_k_linear_i8.h).  The B side is new:
//   W          a stage of 128 k is 64 rows x 128 bytes of codes = 512 pieces of 16 bytes.  Piece q = (n = q >> 3, p = q & 7)
//              holds the k 16 p .. + 15 of output row n: it already IS the operand of lane group kg = p & 3 in step j = p >> 2,
//              so it goes to LDS as ONE ds_write_b128 after the XOR or the look-ups -- no interleave, no second half.  Thread
//              t owns the pieces t, t + 64 WAVES, ... (two at 4 wavefronts, four at 2); eight consecutive lanes read one
//              row's full 128-byte line.
//   B image    [step j][n tile nt][kg][16 slots of 16 bytes], slot = col ^ (4 j + kg) ^ 8 (col & 1) with col = n & 15.
//              LDS has 16 bank groups of 16 bytes; a slot's group is the slot itself (every [kg] block starts at a multiple of
//              256 bytes).  Writes: the 8 lanes of one row share col and hold p = 4 j + kg = 0 .. 7: slots col ^ p are the 8
//              of col's aligned octet, each once; the next 8 lanes hold row n + 1, whose col differs in bit 0 -- the term
//              8 (col & 1) moves it to the OTHER octet, so 16 consecutive lanes cover the 16 groups once.  (k_linear_i8's
//              XOR, col ^ (4 j + (kg & 2)), was chosen for 2 rows x 4 pieces per 8 lanes and would put these 8 writes on 4
//              groups.)  Fragment reads: the 16 lanes of one kg read, for fixed (j, nt), slot col ^ const ^ 8 (col & 1) of
//              one 256-byte block; col -> that slot is a bijection of 0 .. 15 (bit 0 of col is bit 0 of the slot ^ const), so
//              they read the 16 groups once each, and the four kg read four different blocks.  Two images (2 x 8 KiB).
//   codes      every load is unconditional from a clamped address (row min(n, N - 1), offset min(k, K - 16)) and a piece with
//              n >= N or k >= K is zeroed when its operand is formed: a load inside a divergent branch makes the compiler wait
//              for every load in flight at the branch's end (antq_k_linear_i8_sk.h).  A stage's loads are issued one stage
//              before its decode, as in k_linear_i8: while stage c is computed and stage c + 1 written to its image, the
//              loads of stage c + 2 are in flight.
//
// k_linear8_i8_sk<T, TABLE, MT, DIRECT> -- 1 .. 64 rows of xq, K split across workgroups: k_linear_i8_sk's structure
// (antq_k_linear_i8_sk.h).  Grid x = tiles of 64 output rows, grid y = the slices of K (whole stages of 128 k); wavefront w of
// 4 owns the 16 output rows n0 + 16 w .. + 15 for all MT = 1 / 2 / 4 tiles of 16 rows of xq; W never touches LDS; xq is staged
// once per workgroup in two images with one barrier per stage.
//   W          lane (col, kg) loads the 32 bytes 128 c + 32 kg .. + 31 of ITS row as two nontemporal 16-byte loads (the four
//              kg lanes of a row read its full 128-byte line).  After the XOR or the look-ups load j IS the B operand of step
//              j: the k 128 c + 32 kg + 16 j .. + 15, whose A operand is piece 2 kg + j of the stage's xq (k_linear_i8_sk's k
//              map).  Three stages of codes (six registers of four) live in registers: stage c is used while the loads of
//              c + 1 and c + 2 are in flight, so no load is used in the stage it was issued in.
//   slices     partial sums to workspace[s][m][n], added as integers by k_i8_sk_finish; DIRECT (one slice): the epilogue in
//              registers.  Both and i8_sk_store are antq_k_linear_i8_sk.h's, unchanged.  The launcher's rule is this kernel's
//              own (i8b_sk_slices): i8_sk_slices with the traffic cap K / (8 M), because the codes are N K bytes here.
// Sums are exact (the launcher refuses I_x I_w K >= 2^31; xq may hold -128 when I_x = 128): no result depends on the tile, the
// decode kind or the slices.  Epilogue: fl32(S), * u_x, * u_w[n], + bias[n], separate fp32 operations, one conversion.
// LDS: tiled 8 / 16 / 32 KiB of xq image (64 / 128 / 256 rows of 128 bytes) + 16 KiB of B images + the 256-byte table;
// split-K 8 / 8 / 16 KiB of xq images (MT = 1 / 2 / 4) + the table.
#ifndef ANTQ_K_LINEAR8_I8_H
#define ANTQ_K_LINEAR8_I8_H

#include "antq_k_linear_i8_sk.h"

namespace antq {

// whether the m bytes of an image (on the host) are the XOR kind: all 256 codes, image[c] == c - 128
static inline bool i8b_image_is_xor(const int8_t *image, int m)
{
    if (m != 256) return false;
    for (int c = 0; c < 256; c++)
        if ((int)image[c] != c - 128) return false;
    return true;
}

// The slices of K of k_linear8_i8_sk: i8_sk_slices (antq_k_linear_i8.h) with the traffic cap derived again for byte codes --
// above S = K / (8 Mt) the 8 S Mt N bytes of partial traffic exceed the N K bytes of codes.  Like i8_sk_slices it counts the
// ceil(M / 64) row tiles of the conv form (antq_k_conv8_i8.h) with Mt = min(M, 64) rows each; the linear has M <= 64: one.
static inline int i8b_sk_slices(size_t M, size_t N, size_t K, int cus, int forced, size_t &per_slice)
{
    const size_t tiles = ((N + 63) / 64) * ((M + 63) / 64), stages = (K + 127) / 128;
    size_t S = 16;
    for (size_t s = 1; s <= 16; s *= 2)
        if (tiles * s >= 2 * (size_t)std::max(cus, 1)) { S = s; break; }
    S = std::min(S, std::max<size_t>(K / (8 * std::min<size_t>(M, 64)), 1));
    if (forced >= 1) S = (size_t)std::min(forced, 16);
    S = std::max<size_t>(std::min(S, stages), 1);
    per_slice = (stages + S - 1) / S;
    return (int)((stages + per_slice - 1) / per_slice);
}

// sixteen codes -> the sixteen int8 of an MFMA operand; tab: the 256-byte table (TABLE only)
template <bool TABLE>
__device__ __forceinline__ ANTQ_I8_KERNEL u32x4_t i8b_operand(u32x4_t w, const uint8_t *tab)
{
    if constexpr (TABLE) {
        auto look = [&](uint32_t c) __attribute__((always_inline)) {
            return (uint32_t)tab[c & 0xffu] | ((uint32_t)tab[(c >> 8) & 0xffu] << 8) | ((uint32_t)tab[(c >> 16) & 0xffu] << 16) |
                   ((uint32_t)tab[c >> 24] << 24);
        };
        return u32x4_t{look(w.x), look(w.y), look(w.z), look(w.w)};
    } else {
        return w ^ u32x4_t{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    }
}

template <typename T, bool TABLE, int WAVES, int MT>
__global__ void __launch_bounds__(64 * WAVES) ANTQ_I8_KERNEL
k_linear8_i8(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
             uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w,
             const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x)
{
    using XS = std::conditional_t<(WAVES > 0), I8Matrix, void>;      // (I8Matrix, as a dependent type: the body's discarded branches)
    [[maybe_unused]] XS xs;
    [[maybe_unused]] const int32_t *const wsum = nullptr;
#include "antq_k_linear8_i8_tile.h"
}

// One (64 output rows n, slice of K, 16 MT rows m0 .. of the A operand) tile of the byte split-K form and its stores: everything
// of k_linear8_i8_sk but where a piece of the A operand comes from -- the matrix xq [M, K] (XS = I8Matrix, m0 = 0), or whatever
// xs.load(xq, xn, xkeep) gathers for the next stage, asked in order from the slice's first one (antq_k_conv8_i8.h).  wsum as
// in antq_k_linear8_i8_tile.h: DIRECT adds 128 wsum[n] in its epilogue, otherwise the slice blockIdx.y == 0 adds it to the partial sums it stores.
template <typename T, bool TABLE, int MT, bool DIRECT, typename XS>
__device__ __forceinline__ ANTQ_I8_KERNEL void
i8b_sk_tile(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
            int *__restrict__ workspace, uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w,
            const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x, uint32_t per_slice,
            const uint32_t m0, XS &xs, const int32_t *__restrict__ wsum)
{
    constexpr int ROWS = 16 * MT;                      // rows of xq of the workgroup
    constexpr int XROWS = ROWS < 32 ? 32 : ROWS;       // ... of the image: every thread stages (rows >= M are zeros anyway)
    constexpr int PIECES = kGemmBK / 16;               // 16-byte pieces of a row of xq per stage
    constexpr int XP = XROWS * PIECES;                 // pieces of xq per stage
    constexpr int XL = XP / 256;                       // ... per thread
    static_assert((MT == 1 || MT == 2 || MT == 4) && PIECES == 8 && kGemmBK == 128 && kGemmBN == 64, "the maps below");
    struct Lds {
        u32x4_t xs[2][XP];                             // the staged xq of two stages: piece p of row r at [8 r + (p ^ (r & 7))]
        __attribute__((aligned(16))) uint8_t tab[256]; // (TABLE) the int8 of a code byte, zero beyond m
    };
    struct Codes { u32x4_t h[2]; };                    // a lane's 32 codes of one stage: h[j] becomes the operand of step j
    __shared__ Lds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t n = blockIdx.x * (uint32_t)kGemmBN + 16u * wave + col;       // this lane's output row
    const uint32_t nstages = (K + (uint32_t)kGemmBK - 1u) / (uint32_t)kGemmBK;
    const uint32_t c0 = blockIdx.y * per_slice, c1 = min(nstages, c0 + per_slice);      // this slice's stages (never empty)
    const char *crow = reinterpret_cast<const char *>(codes) + (size_t)min(n, N - 1u) * K;

    // Every load below is unconditional, from a clamped address, and a piece that must not count is zeroed afterwards
    // (antq_k_linear_i8_sk.h says why).  This thread's pieces of xq: piece tid & 7 of rows (tid >> 3) + 32 i.
    const uint32_t xp = tid & 7u, xr0 = tid >> 3;
    u32x4_t xn[XL];
    uint32_t xkeep[XL];                                // all ones, or zero for a piece that is zeros: applied at the write
    auto load_x = [&](uint32_t c) __attribute__((always_inline)) {
        if constexpr (std::is_same<XS, I8Matrix>::value) {
            const uint32_t k0 = min(c, c1 - 1u) * (uint32_t)kGemmBK + 16u * xp;
            const bool kok = k0 < K;
            const size_t koff = (size_t)min(k0, K - 16u);
#pragma unroll
            for (int i = 0; i < XL; i++) {
                const uint32_t r = xr0 + 32u * i;
                xn[i] = *(const ANTQ_GLOBAL u32x4_t *)(reinterpret_cast<const char *>(xq) + (size_t)min(r, M - 1u) * K + koff);
                xkeep[i] = (kok && r < M) ? 0xffffffffu : 0u;
            }
        } else xs.load(xq, xn, xkeep);                 // (the stages c0, c0 + 1, ... in order, past the slice's end too)
    };
    auto write_x = [&](uint32_t buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = xr0 + 32u * i;
            if constexpr (XS::kFill) lds.xs[buf][r * PIECES + (xp ^ (r & 7u))] = xs.masked(xn[i], xkeep[i]);
            else lds.xs[buf][r * PIECES + (xp ^ (r & 7u))] = xn[i] & u32x4_t{xkeep[i], xkeep[i], xkeep[i], xkeep[i]};
        }
    };
    // this lane's codes of stage c: the 32 k from 128 c + 32 kg; they count when n < N and k < K (K % 32 == 0: both halves or
    // neither; a stage past the slice is loaded from the slice's last one and never used)
    auto piece_ok = [&](uint32_t c) __attribute__((always_inline)) { return n < N && c * (uint32_t)kGemmBK + 32u * kg < K; };
    auto load_codes = [&](uint32_t c) __attribute__((always_inline)) {
        const uint32_t off = min(min(c, c1 - 1u) * (uint32_t)kGemmBK + 32u * kg, K - 32u);
        Codes w;
        w.h[0] = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow + off));
        w.h[1] = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow + off + 16u));
        return w;
    };

    // __syncthreads(), spelled out: a function without this kernel's target attribute is not inlined into it
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };

    load_x(c0);                                        // in flight while the table is built
    Codes w0 = load_codes(c0), w1 = load_codes(c0 + 1u), w2 = load_codes(c0 + 2u);
    if constexpr (TABLE) lds.tab[tid] = tid < m ? (uint8_t)image_w[tid] : (uint8_t)0;      // (read after the loop's first barrier)
    write_x(0u);
    load_x(c0 + 1u);

    i32x4_t acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = i32x4_t{0, 0, 0, 0};

    // Stage c from the codes in cw (loaded three stages ago), then the staging of c + 1 and the loads of c + 2 (xq) and c + 3
    // (codes, into cw).  The loop below is unrolled by the three code registers by hand: a rotation w0 = w1 would be a use of
    // the load in flight.
    auto stage = [&](uint32_t c, Codes &cw) __attribute__((always_inline)) {
        const uint32_t buf = (c - c0) & 1u;
        sync();                               // image `buf` (and the table) written; every wavefront is done with the other one
        const bool ok = piece_ok(c);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            // (a piece that does not count: exact zeros, not the entry of whatever code was loaded)
            u32x4_t bv = i8b_operand<TABLE>(cw.h[j], lds.tab);
            if (!ok) bv = u32x4_t{0u, 0u, 0u, 0u};
            const i32x4_t b = __builtin_bit_cast(i32x4_t, bv);
            const uint32_t p = 2u * kg + (uint32_t)j;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const i32x4_t a = __builtin_bit_cast(i32x4_t, lds.xs[buf][(16u * mt + col) * PIECES + (p ^ (col & 7u))]);
                acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[mt], 0, 0, 0);
            }
        }
        write_x(buf ^ 1u);                    // stage c + 1 (past the slice: never read)
        load_x(c + 2u);
        cw = load_codes(c + 3u);
    };
    for (uint32_t c = c0; c < c1; c += 3u) {
        stage(c, w0);
        if (c + 1u < c1) stage(c + 1u, w1);
        if (c + 2u < c1) stage(c + 2u, w2);
    }

    // C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg
    if (n >= N) return;
    int corr = 0;                             // (the offset form) 128 wsum[n], added once: by the DIRECT epilogue, or by slice 0
    if constexpr (XS::kFill) corr = (wsum && (DIRECT || blockIdx.y == 0u)) ? wsum[n] * 128 : 0;
    if constexpr (DIRECT) {
        const float u_x = ld_global(alpha_x) / (float)I_x;
        const float u_w = ld_global(alpha_w + (per_row ? n : 0u)) / (float)I_w;
        const float bv = bias ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + 16u * mt + 4u * kg + r;
                if (mrow < M) i8_sk_store<T>(y, (size_t)mrow * N + n, acc[mt][r] + corr, u_x, u_w, bias != nullptr, bv);
            }
    } else {
        int *part = workspace + (size_t)blockIdx.y * M * N + n;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + 16u * mt + 4u * kg + r;
                if (mrow < M) part[(size_t)mrow * N] = acc[mt][r] + corr;
            }
    }
}

template <typename T, bool TABLE, int MT, bool DIRECT>
__global__ void __launch_bounds__(256) ANTQ_I8_KERNEL
k_linear8_i8_sk(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
                int *__restrict__ workspace, uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w,
                const int8_t *__restrict__ image_w, uint32_t m, const float *__restrict__ alpha_x, int I_x, uint32_t per_slice)
{
    I8Matrix xs;
    i8b_sk_tile<T, TABLE, MT, DIRECT>(codes, xq, bias, y, workspace, M, N, K, alpha_w, per_row, I_w, image_w, m, alpha_x, I_x, per_slice,
                                      0u, xs, nullptr);
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR8_I8_H
