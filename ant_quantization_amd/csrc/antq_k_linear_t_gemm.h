// antq_k_linear_t_gemm.h -- y = x . W (+ bias) for 1 .. 4096 rows of x as a tiled matrix-core product, straight from the packed
// 4-bit codes of W stored [K, N]: the layout of GPT-2's Conv1D layers, antq_linear4_t_gemm (bf16 and f16).
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// With the codes stored [K, N] the 8 consecutive k a lane of v_mfma_f32_16x16x32 holds are 8 rows of codes, each with its own
// scale alpha[k] / gmax: k_linear_gemm's finished-output tables per output row do not exist, and k_linear_t_mm
// (antq_k_linear_t_mm.h) finishes every pair per use -- byte extract, ds_read_b64 of the unscaled pair, Lin4Entry::at(s_k), one
// v_perm_b32 per operand register -- which is why it is decode-bound.  Here that cost is paid ONCE per weight and workgroup and
// shared by all 128 or 256 rows of x of the tile: the decoding lane does not feed its own MFMA, it writes the operand registers
// into a fragment-ordered image of B in LDS that every wavefront reads back with one ds_read_b128 per fragment.
//
//   ownership  a workgroup of WAVES = 2 / 4 wavefronts owns one tile of BM = 64 WAVES rows of x by BN = 64 output columns
//              (grid: x = tiles of n, y = tiles of m).  Wavefront w owns rows 64 w .. 64 w + 63 of the tile for all 64 columns:
//              4 x 4 accumulator tiles of v_mfma_f32_16x16x32_{bf16,f16}.  A wavefront whose 64 rows lie past M stages and
//              decodes but runs no MFMA.  WAVES is the launcher's choice (gemm_waves; antq_debug_set key 23 forces it); no sum
//              depends on it.  K is split neither across wavefronts nor across workgroups.
//   W          per stage of BK = 128 k (four MFMA steps of 32 k) the workgroup decodes 128 x 64 weights once: WAVES = 4,
//              wavefront w decodes step w of the stage; WAVES = 2, wavefront w the steps 2 w and 2 w + 1.  The decoding lane is
//              k_linear_t_mm's: lane (c = l & 15, kg = l >> 4) owns the columns 4 c .. 4 c + 3 of the tile and the rows
//              k = 32 s + 8 kg + r of step s: 8 nontemporal code loads of 2 bytes, per row and pair one byte extract, one
//              ds_read_b64 of the unscaled pair and at(s_k), then one v_perm_b32 per operand register.  The four registers of a
//              column (its 8 consecutive k, 16 bytes) go to LDS with one ds_write_b128.
//   B image    [step j][column tile nt][kg][16 slots of 16 bytes], slot = column-in-tile ^ (4 nt + kg): the lanes (col, kg) of a
//              wavefront read the fragment of (j, nt) as 64 different slots of one 1 KiB block -- one ds_read_b128, no bank
//              conflict; the XOR spreads the 64 lanes of a ds_write_b128 (which hold every fourth column) evenly over the
//              16-byte bank groups.  Two images (2 x 16 KiB): the decode of stage c + 1 runs beside the MFMAs of stage c.
//   codes      a stage's code loads are issued one stage before its decode: while stage c is computed and stage c + 1 decoded
//              from registers, the loads of stage c + 2 are in flight.
//   scales     the 128 scales s_k = alpha[k] / gmax of a stage -- true divisions, the decoder's own -- are written by the first
//              128 threads to a small LDS array, double-buffered with the stage: no limit on K, no unstaged branch.  One scale
//              per tensor: one division per workgroup.
//   x          through LDS in full 128-byte lines, as k_linear_gemm stages it: per stage BM rows x 256 bytes, read into
//              registers one stage ahead, written as 16-byte pieces to a [BM][16] image whose piece index is XORed with
//              row & 15; an A fragment is one ds_read_b128 of piece 4 j + kg.  One image, two barriers per stage.
//   sum        y[m, n] is ONE fp32 MFMA accumulator chain from +0: stages in rising order, the four MFMAs of a stage in
//              rising order, inside an MFMA the place of k fixed by (kg, r); then the bias in fp32, then ONE rounding to the
//              type.  The bits depend on row m of x, column n of W, bias[n] and K only -- not on M, N, WAVES, the position in
//              a tile, or the run.  The order is this kernel's own, neither antq_linear4_t's nor antq_linear4_t_mm's.
//   edges      K % 8 == 0, N % 8 == 0.  A k group past K (the last stage only) loads nothing; its W fragment is written as
//              zero and its x piece is staged as zero.  A column group past N loads nothing and is not stored.  Rows m >= M
//              clamp their address, are staged as zero and are not stored.  Padding adds exactly +0 whatever the weights, Inf
//              and NaN included.
//   store      through the fixed C / D map (column = lane & 15, row = 4 (lane >> 4) + reg): 16 consecutive elements per row.
// No atomics, no workspace: one launch, stream-ordered, capturable.  LDS (WAVES = 4): x image 64 KiB, B images 32 KiB, pair
// table 2 KiB, scales 1 KiB -- under 100 KiB of the CU's 160 KiB.
#ifndef ANTQ_K_LINEAR_T_GEMM_H
#define ANTQ_K_LINEAR_T_GEMM_H

#include "antq_k_linear_gemm.h"
#include "antq_k_linear_t_mm.h"

// (every fp32 operation of the decode stays a scalar VALU instruction: one rounding per written operation)
#if defined(__HIP_DEVICE_COMPILE__)
#define ANTQ_T_GEMM_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define ANTQ_T_GEMM_KERNEL
#endif

namespace antq {

template <typename T, bool OVP, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) ANTQ_T_GEMM_KERNEL
k_linear_t_gemm(const uint8_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
                uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
                const float *__restrict__ grid, uint32_t m, int n_normal)
{
    constexpr int MT = kGemmWaveRows / 16, NT = kGemmBN / 16;   // a wavefront's tiles of 16 rows of x, of 16 output columns
    constexpr int BM = kGemmWaveRows * WAVES, NTH = 64 * WAVES;
    constexpr int PIECES = kGemmBK / 8;                // 16-byte pieces of a row of x per stage
    constexpr int XL = BM * PIECES / NTH;              // pieces a thread stages per stage
    constexpr int RSTEP = NTH / PIECES;                // rows between a thread's pieces
    constexpr int SPW = 4 / WAVES;                     // MFMA steps of a stage a wavefront decodes
    constexpr uint32_t BSLOTS = 4u * NT * 64u;         // 16-byte slots of one B image
    static_assert((WAVES == 2 || WAVES == 4) && PIECES == 16 && XL == 16 && kGemmBK == 32 * 4 && NT == 4 && kGemmBN == 64, "the maps below");
    struct Lds {
        u32x4_t xs[BM * PIECES];                       // the staged x: piece p of row r at [16 r + (p ^ (r & 15))]
        u32x4_t b[2][BSLOTS];                          // the B images: fragment (j, nt), lane (col, kg) at [((4 j + nt) 4 + kg) 16 + (col ^ (4 nt + kg))]
        uint2 tab[256];                                // Lin4Entry: the unscaled decoded pair of a code byte
        __attribute__((aligned(16))) float sc[2][kGemmBK];     // the scales of a stage
        float g[32];
        float s_one;                                   // the one scale of a tensor
    };
    __shared__ Lds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t col = lane & 15u, kg = lane >> 4;
    const uint32_t n0 = blockIdx.x * (uint32_t)kGemmBN, m0 = blockIdx.y * (uint32_t)BM;
    const uint32_t nstages = (K + (uint32_t)kGemmBK - 1u) / (uint32_t)kGemmBK;
    const bool active = m0 + (uint32_t)kGemmWaveRows * wave < M;      // (wave-uniform) this wavefront has rows of x

    // the decoding lane: columns n0 + 4 col .. + 3, rows 8 kg + r of the steps SPW wave + i
    const uint32_t dcol0 = n0 + 4u * col;
    const bool live = dcol0 < N;                       // (N % 8 == 0: a group of 4 columns is inside N or past it)
    const size_t row_bytes = (size_t)(N >> 1);
    const ANTQ_GLOBAL uint8_t *cbase = (const ANTQ_GLOBAL uint8_t *)(codes) + (dcol0 >> 1);
    const uint32_t dnt = col >> 2;                     // the column tile of those four columns, which are 4 (col & 3) + jj in it
    const uint32_t dswz = 4u * dnt + kg;

    // this thread's pieces of x: piece tid & 15 of rows (tid >> 4) + RSTEP i
    const uint32_t xp = tid & 15u, xr0 = tid >> 4;
    u32x4_t xn[XL];
    auto load_x = [&](uint32_t c) __attribute__((always_inline)) {
        const uint32_t k0 = c * (uint32_t)kGemmBK + 8u * xp;
        const bool kok = k0 < K;
        const size_t koff = (size_t)min(k0, K - 8u) * 2u;
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = m0 + xr0 + (uint32_t)(RSTEP * i);
            u32x4_t v = *(const ANTQ_GLOBAL u32x4_t *)(static_cast<const char *>(x) + (size_t)min(r, M - 1u) * K * 2u + koff);
            if (!(kok && r < M)) v = u32x4_t{0u, 0u, 0u, 0u};
            xn[i] = v;
        }
    };
    auto write_x = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const uint32_t r = xr0 + (uint32_t)(RSTEP * i);
            lds.xs[r * PIECES + (xp ^ (r & 15u))] = xn[i];
        }
    };
    // the codes of stage c: a k group past the end of K (or a column group past N) loads nothing
    auto load_codes = [&](uint32_t c, uint32_t (&w)[SPW][8]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SPW; i++) {
            const uint32_t k0 = c * (uint32_t)kGemmBK + 32u * (wave * SPW + i) + 8u * kg;
#pragma unroll
            for (int r = 0; r < 8; r++) w[i][r] = 0u;
            if (live && k0 < K) {
#pragma unroll
                for (int r = 0; r < 8; r++)
                    w[i][r] = __builtin_nontemporal_load((const ANTQ_GLOBAL uint16_t *)(cbase + (size_t)(k0 + r) * row_bytes));
            }
        }
    };
    // scale tid of stage c (the first 128 threads; a k past K has none)
    auto load_alpha = [&](uint32_t c) __attribute__((always_inline)) {
        const uint32_t k = c * (uint32_t)kGemmBK + tid;
        return (per_row && tid < (uint32_t)kGemmBK && k < K) ? ld_global(alpha + k) : 0.0f;
    };
    auto write_scale = [&](uint32_t c, float a) __attribute__((always_inline)) {
        if (per_row && tid < (uint32_t)kGemmBK) lds.sc[c & 1u][tid] = a / gmax;        // AQ:536 scale = alpha / max(grid)
    };

    // __syncthreads(), spelled out: a function without this kernel's target attribute is not inlined into it
    auto sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };

    uint32_t cw[SPW][8], cwn[SPW][8];
    load_x(0u);                                        // in flight while the tables are built
    load_codes(0u, cw);
    load_codes(1u, cwn);
    dec4_book(lds.g, tid, grid, m);
    write_scale(0u, load_alpha(0u));
    write_scale(1u, load_alpha(1u));
    if (!per_row && tid == 0u) lds.s_one = ld_global(alpha) / gmax;
    sync();
    for (uint32_t b = tid; b < 256u; b += (uint32_t)NTH) {
        const Lin4Entry<T, OVP> e(b, lds.g, n_normal);
        uint2 pair;
        pair.x = f2u(e.q0);
        pair.y = f2u(e.q1);
        lds.tab[b] = pair;
    }
    const float s_one = per_row ? 0.0f : lds.s_one;
    sync();

    // One quarter (rows 2 q, 2 q + 1 of the lane's k group) of the decode of step i of stage c: register q of the four columns.
    u32x4_t bq[SPW][4];
    auto decode_quarter = [&](uint32_t c, int i, int q) __attribute__((always_inline)) {
        const uint32_t kl = 32u * (wave * SPW + i) + 8u * kg + 2u * q;
        float s0 = s_one, s1 = s_one;
        if (per_row) {
            const float2 s = *reinterpret_cast<const float2 *>(&lds.sc[c & 1u][kl]);
            s0 = s.x;
            s1 = s.y;
        }
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const Lin4Entry<T, OVP> e0 = __builtin_bit_cast(Lin4Entry<T, OVP>, lds.tab[(cw[i][2 * q] >> (8 * p)) & 0xffu]);
            const Lin4Entry<T, OVP> e1 = __builtin_bit_cast(Lin4Entry<T, OVP>, lds.tab[(cw[i][2 * q + 1] >> (8 * p)) & 0xffu]);
            const uint32_t lo = e0.at(s0), hi = e1.at(s1);     // rows 2 q, 2 q + 1: (column 2 p, column 2 p + 1)
            bq[i][2 * p][q] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
            bq[i][2 * p + 1][q] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
        }
    };
    auto write_b = [&](uint32_t c, int i) __attribute__((always_inline)) {
        const uint32_t s = wave * SPW + i;
        const bool kok = c * (uint32_t)kGemmBK + 32u * s + 8u * kg < K;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            u32x4_t v = bq[i][jj];
            if (!kok) v = u32x4_t{0u, 0u, 0u, 0u};
            lds.b[c & 1u][((4u * s + dnt) * 4u + kg) * 16u + ((4u * (col & 3u) + jj) ^ dswz)] = v;
        }
    };

    f32x4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    // MFMA step j of stage c: k = 128 c + 32 j + 8 kg .. + 7
    auto mfma_step = [&](uint32_t c, int j) __attribute__((always_inline)) {
        u32x4_t b[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) b[nt] = lds.b[c & 1u][((4u * j + nt) * 4u + kg) * 16u + (col ^ (4u * nt + kg))];
        const uint32_t p = 4u * j + kg;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const u32x4_t a = lds.xs[((uint32_t)kGemmWaveRows * wave + 16u * mt + col) * PIECES + (p ^ col)];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[mt][nt] = MmOp<T>::mfma(a, b[nt], acc[mt][nt]);
        }
    };

    // stage 0: decoded and staged before the loop
#pragma unroll
    for (int i = 0; i < SPW; i++) {
#pragma unroll
        for (int q = 0; q < 4; q++) decode_quarter(0u, i, q);
        write_b(0u, i);
    }
    write_x();

    for (uint32_t c = 0; c < nstages; c++) {
        sync();                               // x image, B image and scales of stage c (and c + 1's scales) written
        const bool more = c + 1u < nstages;
        const float an = load_alpha(c + 2u);
#pragma unroll
        for (int i = 0; i < SPW; i++)
#pragma unroll
            for (int r = 0; r < 8; r++) cw[i][r] = cwn[i][r];
        if (more) {
            load_x(c + 1u);
            load_codes(c + 2u, cwn);
            // the decode of stage c + 1 beside the MFMAs of stage c
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int i = 0; i < SPW; i++) decode_quarter(c + 1u, i, j);
                if (active) mfma_step(c, j);
            }
#pragma unroll
            for (int i = 0; i < SPW; i++) write_b(c + 1u, i);
        } else if (active) {
#pragma unroll
            for (int j = 0; j < 4; j++) mfma_step(c, j);
        }
        if (!more) break;
        write_scale(c + 2u, an);
        sync();                               // the x image free again
        write_x();
    }

    // C / D map: column (n) = lane & 15, row (m) = 4 (lane >> 4) + reg
    if (!active) return;
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const uint32_t n = n0 + 16u * nt + col;
        if (n >= N) continue;
        const float bv = bias ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t mrow = m0 + (uint32_t)kGemmWaveRows * wave + 16u * mt + 4u * kg + r;
                if (mrow < M) {
                    float v = acc[mt][nt][r];
                    if (bias) v += bv;
                    IO<T>::store1(y, (size_t)mrow * N + n, v);
                }
            }
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR_T_GEMM_H
