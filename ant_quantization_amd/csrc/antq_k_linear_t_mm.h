// antq_k_linear_t_mm.h -- y = x . W (+ bias) for 1 .. 64 rows of x on the matrix cores, straight from the packed 4-bit codes of W
// stored [K, N]: the layout of GPT-2's Conv1D layers, antq_linear4_t_mm (bf16 and f16).
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// v_mfma_f32_16x16x32 wants 8 consecutive k of ONE output column per lane.  With the codes stored [K, N] those are 8 different
// rows of codes, each with its own scale alpha[k] / gmax, so the finished-output table of k_linear_mm (antq_k_linear_mm.h) does
// not carry over: as in k_linear_t (antq_k_linear_t.h) the table holds the UNSCALED decoded pairs and every pair is finished per
// use with the decoder's own pieces -- dec4_book / dec_pair make the pair, Lin4Entry<T, OVP>::at(s_k) scales and rounds it with
// s_k = alpha[k] / gmax as a true division -- so that W[k, n] IS the element antq_decode4 writes.  What the matrix cores buy is that
// this cost per weight is paid once for up to 64 rows of x, not once per 1 .. 8 rows.
//
//   ownership  a workgroup of 8 wavefronts owns TW = 32 PAIRS consecutive output columns (PAIRS = 2: 64) over the whole of K,
//              for all MT = 1 / 2 / 4 tiles of 16 rows of x (the decode is not repeated per M tile).  Lane (c = l & 15,
//              kg = l >> 4) owns the 2 PAIRS columns tile0 + 2 PAIRS c ... and, in step s, the rows k = 32 s + 8 kg + r,
//              r = 0 .. 7.  MFMA j of the step computes the output columns {tile0 + 2 PAIRS c + j}: the store knows the
//              permutation, nothing has to be contiguous per MFMA.
//   B fragment the lane's 8 code loads of PAIRS bytes, nontemporal, one per row k; per row and pair one byte extract, one
//              ds_read_b64 of the unscaled pair and at(s_k): a packed (column 2 p, column 2 p + 1) entry of row k.  The operand
//              register of column j and the k pair (2 i, 2 i + 1) is ONE v_perm_b32 of the entries of rows 2 i and 2 i + 1: no
//              LDS round trip.
//   A fragment one 16-byte cached load of x[row l & 15][32 s + 8 kg ... + 7] per M tile and step (x is re-read by every
//              workgroup and lives in L2)
//   scales     the K scales s_k computed once into LDS where K <= kLinTScales, two ds_read_b128 per lane and step; beyond that
//              a lane divides per use (the same bits).  One scale per tensor: one division per lane.
//   loads      a ring of D steps in registers (D = 4 / 3 / 2 for MT = 1 / 2 / 4): while a step is computed the wavefront's
//              next D - 1 are in flight
//   sum        step s covers k in [32 s, 32 s + 32).  Wavefront w takes the steps w, w + 8, w + 16, ... in rising order,
//              chained in one fp32 MFMA accumulator from +0; inside a step the place of k is fixed (k group kg, element r).  A
//              wavefront without a step contributes +0.  The eight partial tiles meet in LDS (the scales' memory, after a
//              barrier; one M tile per round) and are combined as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)); then
//              the bias is added in fp32, then ONE rounding to the type.  The bits of y[m, n] depend on row m of x, column n
//              of W, bias[n] and K only: not on M, MT, the position of the row in its tile, N, the tile width, the column's
//              place in its tile, the other rows of x, or the run.
//   edges      K % 8 == 0 but K % 32 may not be 0: a k group past the end of K (the last step only, which runs after the ring
//              in the wavefront it falls to) loads nothing and has an all-zero W fragment AND an all-zero x fragment.  A
//              column group past N (N % 8 == 0) loads nothing and is not stored.  Rows m >= M clamp their address into x, have
//              all-zero x fragments and are not stored: a zero against an Inf weight there makes a NaN that nobody sees.
//   store      after the reduction thread t finishes column t % TW of the tile: a wavefront writes 64 consecutive elements
// No atomics, no split of K across workgroups, no workspace: one launch, stream-ordered, capturable.
#ifndef ANTQ_K_LINEAR_T_MM_H
#define ANTQ_K_LINEAR_T_MM_H

#include "antq_k_linear_mm.h"
#include "antq_k_linear_t.h"

namespace antq {

constexpr int kLinTMmWaves = 8;                        // wavefronts per workgroup = ways the steps of K are dealt out
// pairs of columns per lane: the tile is 32 kLinTMmPairs columns wide.  1 (a byte per code load, twice the workgroups) is the tile
// this one was measured against: 4 ... 13 % faster on the long-K, narrow-N layers, up to 7 % slower on wide ones at 32 rows
// (profiles/packed_linear_t_mm.md); the test file holds for both.
constexpr int kLinTMmPairs = 2;

template <int PAIRS> struct LinTMmCode;                // a lane's codes of one row k
template <> struct LinTMmCode<1> { typedef uint8_t type; };
template <> struct LinTMmCode<2> { typedef uint16_t type; };

// MT: tiles of 16 rows of x; PAIRS: pairs of output columns per lane
template <typename T, bool OVP, int MT, int PAIRS>
__global__ void __launch_bounds__(64 * kLinTMmWaves)
k_linear_t_mm(const uint8_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
              uint32_t M, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
              const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef typename LinTMmCode<PAIRS>::type Code;
    constexpr uint32_t CPL = 2 * PAIRS, TW = 16 * CPL;      // columns per lane, per workgroup
    constexpr int D = MT == 1 ? 4 : (MT == 2 ? 3 : 2);
    constexpr uint32_t RED = kLinTMmWaves * 4 * 64 * CPL;   // floats of one round of the reduction: one M tile
    static_assert(kLinTMmWaves == 8 && RED <= kLinTScales && (64u * kLinTMmWaves) % TW == 0, "the reduction below");
    __shared__ __attribute__((aligned(16))) uint2 tab[256];     // Lin4Entry: the unscaled decoded pair of a code byte
    __shared__ float g[32];
    __shared__ __attribute__((aligned(16))) float sc[kLinTScales];     // the scales; after the last step the partial tiles
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t c = lane & 15u, kg = lane >> 4;
    const uint32_t tile0 = __builtin_amdgcn_readfirstlane(blockIdx.x) * TW;
    const uint32_t col0 = tile0 + CPL * c;
    const bool live = col0 < N;                         // (N % 8 == 0: a column group is inside N or past it)
    const size_t row_bytes = (size_t)(N >> 1);
    const ANTQ_GLOBAL uint8_t *cbase = (const ANTQ_GLOBAL uint8_t *)(codes) + (col0 >> 1);
    const uint32_t nfull = K >> 5;                      // whole steps; a partial last one falls to wavefront nfull % 8
    const uint32_t towner = (K & 31u) ? (nfull & (kLinTMmWaves - 1u)) : ~0u;

    const char *xrow[MT];
    bool mok[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        mok[mt] = 16u * mt + c < M;
        xrow[mt] = static_cast<const char *>(x) + (size_t)min(16u * mt + c, M - 1u) * K * 2u;
    }

    uint32_t cw[D][8];
    u32x4_t xa[D][MT];
    // step s into ring slot d.  TAIL: the partial last step, where a k group may lie past the end of K and loads nothing
    auto load_step = [&](uint32_t s, int d, auto tail) {
        const uint32_t k0 = 32u * s + 8u * kg;
        const bool kok = !decltype(tail)::value || k0 < K;
#pragma unroll
        for (int r = 0; r < 8; r++) cw[d][r] = 0u;
        if (live && kok) {
#pragma unroll
            for (int r = 0; r < 8; r++)
                cw[d][r] = __builtin_nontemporal_load((const ANTQ_GLOBAL Code *)(cbase + (size_t)(k0 + r) * row_bytes));
        }
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            u32x4_t v = u32x4_t{0u, 0u, 0u, 0u};
            if (kok) v = *(const ANTQ_GLOBAL u32x4_t *)(xrow[mt] + (size_t)k0 * 2u);
            if (!mok[mt]) v = u32x4_t{0u, 0u, 0u, 0u};
            xa[d][mt] = v;
        }
    };
#pragma unroll
    for (int d = 0; d < D; d++)                         // in flight while the tables are built
        if (wave + kLinTMmWaves * d < nfull) load_step(wave + kLinTMmWaves * d, d, std::false_type());

    dec4_book(g, tid, grid, m);
    const bool staged = per_row && K <= kLinTScales;
    if (staged) {
        for (uint32_t k = tid; k < K; k += 64u * kLinTMmWaves) sc[k] = ld_global(alpha + k) / gmax;   // AQ:536 scale = alpha / max(grid)
    }
    const float s_one = per_row ? 0.0f : ld_global(alpha) / gmax;
    __syncthreads();
    if (tid < 256u) {
        const Lin4Entry<T, OVP> e(tid, g, n_normal);
        tab[tid] = make_uint2(f2u(e.q0), f2u(e.q1));
    }
    __syncthreads();

    f32x4_t acc[MT][CPL];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (uint32_t j = 0; j < CPL; j++) acc[mt][j] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    auto compute = [&](uint32_t s, int d, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        const uint32_t k0 = 32u * s + 8u * kg;
        const bool kok = !TAIL || k0 < K;
        float sk[8];
#pragma unroll
        for (int r = 0; r < 8; r++) sk[r] = s_one;
        if (per_row && kok) {
            if (staged) {
                const float4 a = *reinterpret_cast<const float4 *>(sc + k0), b = *reinterpret_cast<const float4 *>(sc + k0 + 4u);
                sk[0] = a.x; sk[1] = a.y; sk[2] = a.z; sk[3] = a.w;
                sk[4] = b.x; sk[5] = b.y; sk[6] = b.z; sk[7] = b.w;
            } else {
#pragma unroll
                for (int r = 0; r < 8; r++) sk[r] = ld_global(alpha + k0 + r) / gmax;
            }
        }
#pragma unroll
        for (int p = 0; p < PAIRS; p++) {
            uint32_t ent[8];                           // row k0 + r: (column 2 p, column 2 p + 1) in the output type
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const Lin4Entry<T, OVP> e = __builtin_bit_cast(Lin4Entry<T, OVP>, tab[(cw[d][r] >> (8 * p)) & 0xffu]);
                ent[r] = e.at(sk[r]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++) {
                // the column's 8 k: register i = (row 2 i in the low half, row 2 i + 1 in the high half)
                u32x4_t b;
#pragma unroll
                for (int i = 0; i < 4; i++) b[i] = __builtin_amdgcn_perm(ent[2 * i + 1], ent[2 * i], h ? 0x07060302u : 0x05040100u);
                if (TAIL && !kok) b = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                for (int mt = 0; mt < MT; mt++) acc[mt][2 * p + h] = MmOp<T>::mfma(xa[d][mt], b, acc[mt][2 * p + h]);
            }
        }
    };

    for (uint32_t s0 = wave; s0 < nfull; s0 += kLinTMmWaves * D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t s = s0 + kLinTMmWaves * d;
            if (s >= nfull) break;
            compute(s, d, std::false_type());
            if (s + kLinTMmWaves * D < nfull) load_step(s + kLinTMmWaves * D, d, std::false_type());
        }
    }
    if (wave == towner) {                               // the partial last step: the last of the wavefront it falls to
        load_step(nfull, 0, std::true_type());
        compute(nfull, 0, std::true_type());
    }

    // The eight partial tiles meet in LDS (the scales' memory, once every wavefront is done with them), one M tile per round:
    // red[wave][reg][kg][column of the tile].  C / D map of MFMA j: column = CPL c + j, row (m) = 4 kg + reg.
    float *red = sc;
    const uint32_t ocol = tid % TW, n = tile0 + ocol;
    const float bv = (bias && n < N) ? IO<T>::load1(bias, n) : 0.0f;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (uint32_t j = 0; j < CPL; j++) red[((wave * 4u + r) * 64u + lane) * CPL + j] = acc[mt][j][r];
        __syncthreads();
        for (uint32_t o = tid; o < 16u * TW; o += 64u * kLinTMmWaves) {
            const uint32_t row = o / TW;                // of the M tile: k group row >> 2, register row & 3
            const float *p = red + (row & 3u) * (64u * CPL) + (row >> 2) * TW + ocol;      // wavefront w's partial sum: p[W w]
            constexpr uint32_t W = 4u * 64u * CPL;
            float v = ((p[0] + p[W]) + (p[2 * W] + p[3 * W])) + ((p[4 * W] + p[5 * W]) + (p[6 * W] + p[7 * W]));
            const uint32_t mrow = 16u * mt + row;
            if (n < N && mrow < M) {
                if (bias) v += bv;
                IO<T>::store1(y, (size_t)mrow * N + n, v);
            }
        }
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR_T_MM_H
