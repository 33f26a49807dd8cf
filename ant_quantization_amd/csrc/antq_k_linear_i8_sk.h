// antq_k_linear_i8_sk.h -- the integer-domain 4-bit linear for 1 .. 64 rows of xq with K split across workgroups: the kernels
// of antq_linear4_i8_sk (fp32, bf16 and f16 outputs).  The contract is antq_linear4_i8's, letter for letter (include/antq.h):
// S the exact int32 sum on v_mfma_i32_16x16x64_i8, the scales applied once per output; the bits of y equal k_linear_i8's.
// k_linear_i8 gives such a call ceil(N / 64) workgroups that each walk all of K through LDS; here the weights never touch
// LDS, no two wavefronts share one, and K is cut into S slices (the launcher's rule: i8_sk_slices) -- the one place in the
// library where that costs no determinism, because an exact sum has no order.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.  Everything below but the source of the
// A operand lives in i8_sk_tile, which antq_k_conv_i8_sk.h shares: k_linear_i8_sk is i8_sk_tile with the matrix A side.
//
//   ownership  grid x = tiles of 64 output rows n, grid y = the S slices of K, a slice = per_slice stages of 128 k (the last
//              one may be shorter).  A workgroup has 4 wavefronts; wavefront w owns the 16 output rows n0 + 16 w .. + 15 for
//              all MT = 1 / 2 / 4 tiles of 16 rows of xq (the smallest MT that covers M).
//   W          never in LDS.  Lane (col = lane & 15, kg = lane >> 4) loads 16 bytes of ITS output row n0 + 16 w + col per
//              stage, nontemporal: the 32 consecutive k  128 c + 32 kg .. + 31  (the four kg lanes of a row read 64
//              contiguous bytes).  Three stages of codes live in registers: stage c is decoded while the loads of c + 1 and
//              c + 2 are in flight.  The 32 nibbles become 32 int8 in eight registers, decoded in place: plain books with
//              i8_decode_word (15 VALU per 8 weights), pair-rule books through the 256-entry LDS pair table (i8_pair_entry,
//              built once per workgroup).
//   k map      the sum has no order, so the k of a stage are dealt to the MFMA steps as the loads deliver them: the B operand
//              of (step j, lane group kg) is the k  128 c + 32 kg + 16 j .. + 15  -- registers 4 j .. 4 j + 3 of the lane's
//              decoded piece -- and the A operand of the same (j, kg) holds the same k of xq: piece 2 kg + j of the stage's
//              eight 16-byte pieces of the row.  (k_linear_i8's map is 64 j + 16 kg: piece 4 j + kg.)
//   xq         through LDS once per workgroup, all four wavefronts read the same fragments: per stage 16 MT rows x 128 bytes
//              in full lines (8 consecutive lanes one row), k_linear_i8's image -- piece p of row r at 8 r + (p ^ (r & 7)) --
//              so that the 8 rows 8 consecutive lanes of an A fragment's ds_read_b128 read fall on the 8 different 16-byte
//              bank groups.  Two images: stage c + 1 is written (from registers loaded one stage earlier) beside the MFMAs of
//              stage c, ONE barrier per stage.
//   edges      K % 32 == 0, N arbitrary.  A piece of codes with n >= N or k >= K clamps its address and its operand is exact
//              zeros (not the entry of a code); a piece of xq with m >= M or k >= K clamps its address and is staged as zeros.
//              Padded outputs are neither stored nor written to the workspace.
//   slices     DIRECT (S = 1): the epilogue of k_linear_i8 in registers, y stored through the C / D map (column n =
//              lane & 15, row m = 4 (lane >> 4) + reg); no workspace, one launch.  Otherwise slice s stores its raw int32
//              accumulators to workspace[s][m][n] with ordinary vector stores and k_i8_sk_finish adds the S partials of each
//              output as integers (exact: the launcher refuses I_x I_w K >= 2^31) and runs the same epilogue.  No atomics,
//              no tickets, no order between the workgroups of a launch; every word of the workspace that is read was written
//              by the launch before, so nothing needs zeroing.
//   epilogue   fl32(S), * u_x, * u_w[n], + bias[n]: separate fp32 operations, one conversion (i8_sk_store; -ffp-contract=off,
//              no packed fp32), u_x = alpha_x / I_x and u_w[n] = alpha_w[n] / I_w true fp32 divisions.
// LDS: 8 / 8 / 16 KiB of xq images (MT = 1 / 2 / 4; at least 32 rows, so that every thread stages) + 544 bytes of tables.
// Measured (profiles/int_linear4_sk.md): 0.10 ... 0.71 of k_linear_i8's time at every one of 80 points of 1 ... 64 rows.
#ifndef ANTQ_K_LINEAR_I8_SK_H
#define ANTQ_K_LINEAR_I8_SK_H

#include "antq_k_linear_i8.h"

namespace antq {

// one output: the contract's epilogue on the exact sum S, then ONE conversion
template <typename T>
__device__ __forceinline__ ANTQ_I8_KERNEL void i8_sk_store(void *y, size_t idx, int S, float u_x, float u_w, bool has_bias, float bv)
{
    float v = (float)S;
    v = v * u_x;
    v = v * u_w;
    if (has_bias) v = v + bv;
    IO<T>::store1(y, idx, v);
}

// The constants of an MT tile that the split-K kernels and their A sides share
template <int MT>
struct I8SkTile {
    static constexpr int ROWS = 16 * MT;               // rows of xq of the workgroup
    static constexpr int XROWS = ROWS < 32 ? 32 : ROWS;        // ... of the image: every thread stages (rows >= M are zeros anyway)
    static constexpr int PIECES = kGemmBK / 16;        // 16-byte pieces of a row of xq per stage
    static constexpr int XP = XROWS * PIECES;          // pieces of xq per stage
    static constexpr int XL = XP / 256;                // ... per thread: piece tid & 7 of rows (tid >> 3) + 32 i
};

// One (64 output rows n, slice of K, ROWS rows m0 .. of the A operand) tile of the split-K form and its stores, as the header
// states it: everything of k_linear_i8_sk but where a piece of the A operand comes from -- a row-major matrix xq [M, K]
// (XS = I8Matrix, m0 = 0), or whatever xs.load(xq, xn, xkeep) gathers for the next stage, asked in order from the slice's
// first one (antq_k_conv_i8_sk.h: im2col).  y and every slice of the workspace are [M, N] row-major.
template <typename T, bool OVP, int MT, bool DIRECT, typename XS>
__device__ __forceinline__ ANTQ_I8_KERNEL void
i8_sk_tile(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
           int *__restrict__ workspace, uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w,
           const int8_t *__restrict__ image_w, uint32_t m, int n_normal, const float *__restrict__ alpha_x, int I_x,
           uint32_t per_slice, const uint32_t m0, XS &xs)
{
    using TL = I8SkTile<MT>;
    constexpr int PIECES = TL::PIECES, XP = TL::XP, XL = TL::XL;
    static_assert((MT == 1 || MT == 2 || MT == 4) && PIECES == 8 && kGemmBK == 128 && kGemmBN == 64, "the maps below");
    struct Lds {
        u32x4_t xs[2][XP];                             // the staged xq of two stages: piece p of row r at [8 r + (p ^ (r & 7))]
        uint16_t pair[256];                            // (pair rule) the int8 pair of a code byte
        __attribute__((aligned(16))) uint8_t g[32];    // the image, zero beyond m
    };
    __shared__ Lds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t n = blockIdx.x * (uint32_t)kGemmBN + 16u * wave + col;       // this lane's output row
    const uint32_t nstages = (K + (uint32_t)kGemmBK - 1u) / (uint32_t)kGemmBK;
    const uint32_t c0 = blockIdx.y * per_slice, c1 = min(nstages, c0 + per_slice);      // this slice's stages (never empty)
    const uint32_t row_bytes = K >> 1;
    const char *crow = reinterpret_cast<const char *>(codes) + (size_t)min(n, N - 1u) * row_bytes;

    // Every load below is unconditional, from a clamped address, and a piece that must not count is zeroed afterwards: a load
    // inside a divergent branch makes the compiler wait for ALL loads in flight at the branch's end (s_waitcnt vmcnt(0)).
    // this thread's pieces of xq: piece tid & 7 of rows (tid >> 3) + 32 i; one with m >= M or k >= K is zeros
    const uint32_t xp = tid & 7u, xr0 = tid >> 3;
    u32x4_t xn[XL];
    uint32_t xkeep[XL];                                // all ones, or zero for a piece that is zeros: applied at the write -- a
                                                       // select or a mask at the load would wait for the load there and then
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
            lds.xs[buf][r * PIECES + (xp ^ (r & 7u))] = xn[i] & u32x4_t{xkeep[i], xkeep[i], xkeep[i], xkeep[i]};
        }
    };
    // this lane's piece of codes of stage c: the 32 k from 128 c + 32 kg; it counts when n < N and k < K (a stage past the
    // slice is loaded from the slice's last one and never used)
    auto piece_ok = [&](uint32_t c) __attribute__((always_inline)) { return n < N && c * (uint32_t)kGemmBK + 32u * kg < K; };
    auto load_codes = [&](uint32_t c) __attribute__((always_inline)) {
        const uint32_t off = min(min(c, c1 - 1u) * (uint32_t)(kGemmBK / 2) + 16u * kg, row_bytes - 16u);
        return __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow + off));
    };

    // __syncthreads(), spelled out: a function without this kernel's target attribute is not inlined into it
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };

    load_x(c0);                                        // in flight while the tables are built
    u32x4_t w[3] = {load_codes(c0), load_codes(c0 + 1u), load_codes(c0 + 2u)};
    if (tid < 32u) lds.g[tid] = tid < m ? (uint8_t)image_w[tid] : (uint8_t)0;
    sync();
    uint32_t img[4] = {0u, 0u, 0u, 0u};
    if constexpr (OVP) {
        lds.pair[tid] = i8_pair_entry(tid, lds.g, (uint32_t)n_normal);      // (read after the loop's first barrier)
    } else {
        const u32x4_t t = *reinterpret_cast<const u32x4_t *>(lds.g);
        img[0] = t.x; img[1] = t.y; img[2] = t.z; img[3] = t.w;
    }
    write_x(0u);
    load_x(c0 + 1u);

    i32x4_t acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = i32x4_t{0, 0, 0, 0};

    // Stage c from the codes in cw (loaded three stages ago), then the staging of c + 1 and the loads of c + 2 (xq) and c + 3
    // (codes, into cw).  The loop below is unrolled by the three code registers by hand: a rotation w0 = w1 would be a use of
    // the load in flight.
    auto stage = [&](uint32_t c, u32x4_t &cw) __attribute__((always_inline)) {
        const uint32_t buf = (c - c0) & 1u;
        sync();                               // image `buf` written; every wavefront is done with the other one
        const bool ok = piece_ok(c);
        // 32 nibbles -> the operands of the stage's two MFMA steps
        const uint32_t wd[4] = {cw.x, cw.y, cw.z, cw.w};
        uint32_t o[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if constexpr (OVP) {
                o[2 * i] = (uint32_t)lds.pair[wd[i] & 0xffu] | ((uint32_t)lds.pair[(wd[i] >> 8) & 0xffu] << 16);
                o[2 * i + 1] = (uint32_t)lds.pair[(wd[i] >> 16) & 0xffu] | ((uint32_t)lds.pair[wd[i] >> 24] << 16);
            } else i8_decode_word(wd[i], img, o[2 * i], o[2 * i + 1]);
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            // (a piece that does not count: exact zeros, not the entry of whatever code was loaded)
            u32x4_t bv = u32x4_t{o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]};
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
        stage(c, w[0]);
        if (c + 1u < c1) stage(c + 1u, w[1]);
        if (c + 2u < c1) stage(c + 2u, w[2]);
    }

    // C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg
    if (n >= N) return;
    if constexpr (DIRECT) {
        const float u_x = ld_global(alpha_x) / (float)I_x;
        const float u_w = ld_global(alpha_w + (per_row ? n : 0u)) / (float)I_w;
        const float bv = bias ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + 16u * mt + 4u * kg + r;
                if (mrow < M) i8_sk_store<T>(y, (size_t)mrow * N + n, acc[mt][r], u_x, u_w, bias != nullptr, bv);
            }
    } else {
        int *part = workspace + (size_t)blockIdx.y * M * N + n;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + 16u * mt + 4u * kg + r;
                if (mrow < M) part[(size_t)mrow * N] = acc[mt][r];
            }
    }
}

template <typename T, bool OVP, int MT, bool DIRECT>
__global__ void __launch_bounds__(256) ANTQ_I8_KERNEL
k_linear_i8_sk(const uint8_t *__restrict__ codes, const int8_t *__restrict__ xq, const void *__restrict__ bias, void *__restrict__ y,
               int *__restrict__ workspace, uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha_w, int per_row, int I_w,
               const int8_t *__restrict__ image_w, uint32_t m, int n_normal, const float *__restrict__ alpha_x, int I_x,
               uint32_t per_slice)
{
    I8Matrix xs;
    i8_sk_tile<T, OVP, MT, DIRECT>(codes, xq, bias, y, workspace, M, N, K, alpha_w, per_row, I_w, image_w, m, n_normal, alpha_x, I_x,
                                   per_slice, 0u, xs);
}

// y[m, n] from the S partial sums workspace[s][m][n]: added as integers, then the epilogue.  One thread per output.
template <typename T>
__global__ void __launch_bounds__(256) ANTQ_I8_KERNEL
k_i8_sk_finish(const int *__restrict__ workspace, const void *__restrict__ bias, void *__restrict__ y, uint32_t M, uint32_t N, uint32_t S,
               const float *__restrict__ alpha_w, int per_row, int I_w, const float *__restrict__ alpha_x, int I_x)
{
    const size_t total = (size_t)M * N, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t n = (uint32_t)(i % N);
    int sum = 0;
    for (uint32_t s = 0; s < S; s++) sum += workspace[(size_t)s * total + i];
    const float u_x = ld_global(alpha_x) / (float)I_x;
    const float u_w = ld_global(alpha_w + (per_row ? n : 0u)) / (float)I_w;
    i8_sk_store<T>(y, i, sum, u_x, u_w, bias != nullptr, bias ? IO<T>::load1(bias, n) : 0.0f);
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR_I8_SK_H
