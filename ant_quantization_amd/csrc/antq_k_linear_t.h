// antq_k_linear_t.h -- y = x . W (+ bias) for 1 .. 8 rows of x, straight from the packed 4-bit codes of W stored [K, N]: the
// layout of GPT-2's Conv1D layers (weight [in, out], y = x @ W + b), antq_linear4_t.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// The row-streaming kernel (antq_k_linear.h) sums along a row of codes with one scale per row.  Here the sum runs ACROSS the
// rows of codes: a row k of codes holds W[k, 0 .. N), its scale alpha[k] belongs to the input feature k, and OliVe's pairs are
// adjacent output columns.  A finished-output byte table per k is not affordable, so the table holds the UNSCALED decoded
// pairs and every pair is finished per use -- with the decoder's own pieces, so that W[k, n] IS the element antq_decode4
// writes: dec4_book / dec_pair (antq_device.h) make the pair, Lin4Entry<T, OVP>::at(s) (antq_k_linear4.h) scales and rounds
// it to the output type with s = alpha[k] / gmax as a true division, Lin4W<T>::get widens it.  The scale is never factored
// out of the sum or folded into x.
//
//   ownership  a workgroup of 8 wavefronts owns 32 consecutive output columns over the whole of K; lane l of wavefront w owns
//              the 8 columns 8 (l % 4) .. + 8 of the tile -- ONE 32-bit code word per row k, four whole pairs -- and the phase
//              P = 16 w + l / 4 of k: it takes k = P, P + 128, P + 256, ... in rising order into acc[M][8].  K is not split
//              across workgroups.  (First built with 64 columns and 64 phases: its time followed K, not N -- the chain of a
//              lane's loads, not bandwidth.  Twice as many workgroups of half the chain measured 1.06 .. 1.66 times faster
//              at M >= 4 and at K >= 3072, and 8 .. 16 % slower at M = 1 with K = 768 / 1600: profiles/packed_linear_t.md.)
//   tables     per workgroup: the 256 unscaled decoded pairs keyed by the code BYTE (2 KiB), and the K scales s_k computed
//              once into LDS where K <= kLinTScales (GPT-2: K <= 6400); beyond that a lane divides per step.  One scale per
//              tensor: one division per lane.
//   loads      codes straight to VGPRs, nontemporal, one word per lane and k, a group of steps (k, k + 128, ...: 8 steps for
//              M <= 2, 4 beyond) in flight at once and the next group issued before this one is computed; x[m, k] is one
//              element per row of x and step, re-read by every workgroup through the cache (M x K elements), loaded with
//              the codes
//   per pair   one byte extract, one ds_read_b64, the two multiplies, make, get, then 2 M fmaf
//   sum        THE TILE RULE, a function of K alone: partial sum P (0 .. 127) of y[m, n] is
//              fmaf(x[m, k], W[k, n], .) over k = P, P + 128, ... < K in rising order, from +0 (a phase with no k stays +0);
//              the 128 partial sums are combined as one fixed tree: inside a wavefront the 16 phases p0 .. p15 as four
//              groups of four, each ((p0 + p2) + (p1 + p3)) (two DPP steps), the groups as (g0 + g1) + (g2 + g3) (two lane
//              exchanges), then the eight wavefronts' sums w0 .. w7 through LDS as
//              ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)); the bias is added in fp32, one rounding to the type.
//              (The number of steps in flight does not enter the order of the sum.)
//              The bits of y[m, n] depend on row m of x, column n of W, bias[n] and K only: not on M, not on N or the place
//              of the column in its tile, not on the other rows of x, not on the run.
//   padding    a step past the end of K and a column group past the end of N load nothing and add nothing (both operands
//              absent: the accumulator keeps its +0) -- never a zero x against a repeated weight; rows of x beyond m_rows
//              repeat the last real row and are not stored
//   store      thread t of the first 32 M: row t / 32, column t % 32 of the tile, one element each, consecutive columns
#ifndef ANTQ_K_LINEAR_T_H
#define ANTQ_K_LINEAR_T_H

#include "antq_device.h"
#include "antq_k_linear4.h"

namespace antq {

constexpr uint32_t kLinTCols = 32;                      // output columns per workgroup: 4 column lanes of 8
constexpr uint32_t kLinTWaves = 8;
constexpr uint32_t kLinTPhases = 128;                   // phases of k per workgroup: 16 per wavefront
constexpr uint32_t kLinTScales = 8192;                  // the most scales staged in LDS (32 KiB)
constexpr int lin_t_steps(int M) { return M <= 2 ? 8 : 4; }     // steps of a lane in flight at once (twice that with the next group's)

// one element of x: the raw word as loaded, and its exact widening to fp32
template <typename T> struct LinTX {
    __device__ __forceinline__ static uint32_t load(const void *x, size_t i) { return (uint32_t)((const ANTQ_GLOBAL uint16_t *)(x))[i]; }
    __device__ __forceinline__ static float get(uint32_t r);
};
template <> __device__ __forceinline__ float LinTX<bf16_tag>::get(uint32_t r) { return u2f(r << 16); }
template <> __device__ __forceinline__ float LinTX<f16_tag>::get(uint32_t r) { return IO<f16_tag>::h2f(r); }
template <> struct LinTX<float> {
    __device__ __forceinline__ static uint32_t load(const void *x, size_t i) { return ((const ANTQ_GLOBAL uint32_t *)(x))[i]; }
    __device__ __forceinline__ static float get(uint32_t r) { return u2f(r); }
};

// M: rows of x the kernel computes (rows >= m_rows repeat the last one and are not stored)
template <typename T, bool OVP, int M>
__global__ void __launch_bounds__(64 * kLinTWaves)
k_linear_t(const uint8_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
           uint32_t m_rows, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
           const float *__restrict__ grid, uint32_t m, int n_normal)
{
    constexpr int U = lin_t_steps(M);
    __shared__ __attribute__((aligned(16))) uint2 tab[256];     // Lin4Entry: the unscaled decoded pair of a code byte
    __shared__ float g[32];
    __shared__ float sc[kLinTScales];
    __shared__ float red[kLinTWaves][M][kLinTCols];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t cl = lane & 3u, P = wave * 16u + (lane >> 2);
    const uint32_t tile0 = __builtin_amdgcn_readfirstlane(blockIdx.x) * kLinTCols;
    const uint32_t col0 = tile0 + cl * 8u;
    const bool live = col0 < N;                         // (N % 8 == 0: a column group is inside N or past it)
    const size_t row_bytes = (size_t)(N >> 1);
    const ANTQ_GLOBAL uint8_t *cbase = (const ANTQ_GLOBAL uint8_t *)(codes) + (col0 >> 1);
    const uint32_t steps = (K + kLinTPhases - 1u) / kLinTPhases;        // of the longest phase
    const uint32_t groups = (steps + U - 1u) / U;
    size_t xoff[M];
#pragma unroll
    for (int i = 0; i < M; i++) xoff[i] = (size_t)min((uint32_t)i, m_rows - 1u) * K;

    uint32_t cw[U], nw[U], xc[M][U], xn[M][U];
    auto load_group = [&](uint32_t gi, uint32_t (&w)[U], uint32_t (&xs)[M][U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t k = P + kLinTPhases * (gi * U + u);
            w[u] = 0u;
#pragma unroll
            for (int i = 0; i < M; i++) xs[i][u] = 0u;
            if (live && k < K) {
                w[u] = __builtin_nontemporal_load((const ANTQ_GLOBAL uint32_t *)(cbase + (size_t)k * row_bytes));
#pragma unroll
                for (int i = 0; i < M; i++) xs[i][u] = LinTX<T>::load(x, xoff[i] + k);
            }
        }
    };
    load_group(0u, cw, xc);                             // in flight while the tables are built

    dec4_book(g, tid, grid, m);
    const bool staged = per_row && K <= kLinTScales;
    if (staged) {
        for (uint32_t k = tid; k < K; k += 64u * kLinTWaves) sc[k] = ld_global(alpha + k) / gmax;   // AQ:536 scale = alpha / max(grid)
    }
    const float s_one = per_row ? 0.0f : ld_global(alpha) / gmax;
    __syncthreads();
    if (tid < 256u) {
        const Lin4Entry<T, OVP> e(tid, g, n_normal);
        tab[tid] = make_uint2(f2u(e.q0), f2u(e.q1));
    }
    __syncthreads();

    float acc[M][8];
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
        for (int c = 0; c < 8; c++) acc[i][c] = 0.0f;

    for (uint32_t gi = 0; gi < groups; gi++) {
        const bool more = gi + 1u < groups;
        if (more) load_group(gi + 1u, nw, xn);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t k = P + kLinTPhases * (gi * U + u);
            if (live && k < K) {
                const float s = !per_row ? s_one : (staged ? sc[k] : ld_global(alpha + k) / gmax);
                float xf[M];
#pragma unroll
                for (int i = 0; i < M; i++) xf[i] = LinTX<T>::get(xc[i][u]);
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const Lin4Entry<T, OVP> e = __builtin_bit_cast(Lin4Entry<T, OVP>, tab[(cw[u] >> (8 * p)) & 0xffu]);
                    float w0, w1;
                    Lin4W<T>::get(e.at(s), w0, w1);
#pragma unroll
                    for (int i = 0; i < M; i++) {
                        acc[i][2 * p] = __builtin_fmaf(xf[i], w0, acc[i][2 * p]);
                        acc[i][2 * p + 1] = __builtin_fmaf(xf[i], w1, acc[i][2 * p + 1]);
                    }
                }
            }
        }
        if (!more) break;
#pragma unroll
        for (int u = 0; u < U; u++) {
            cw[u] = nw[u];
#pragma unroll
            for (int i = 0; i < M; i++) xc[i][u] = xn[i][u];
        }
    }

    // the wavefront's eight phases of every (row, column): all lanes active
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
        for (int c = 0; c < 8; c++) {
            float v = acc[i][c];
            v += lin_dpp<0x128>(v);                     // row_ror:8: lanes l and l ^ 8, phases P and P ^ 2
            v += lin_dpp<0x124>(v);                     // row_ror:4: lanes l < 4 add lane l + 4, phases (P, P ^ 2) and (P ^ 1, P ^ 3)
            v += __shfl_xor(v, 16);                     // phases P ^ 4
            v += __shfl_xor(v, 32);                     // phases P ^ 8
            if (lane < 4u) red[wave][i][cl * 8u + c] = v;
        }
    __syncthreads();
    const uint32_t i = tid / kLinTCols, c = tid % kLinTCols, col = tile0 + c;
    if (i < (uint32_t)M && i < m_rows && col < N) {
        float v = ((red[0][i][c] + red[1][i][c]) + (red[2][i][c] + red[3][i][c])) +
                  ((red[4][i][c] + red[5][i][c]) + (red[6][i][c] + red[7][i][c]));
        if (bias) v += IO<T>::load1(bias, col);
        IO<T>::store1(y, (size_t)i * N + col, v);
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR_T_H
