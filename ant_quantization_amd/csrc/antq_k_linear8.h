// antq_k_linear8.h -- y = x . W^T (+ bias) for 1 .. 8 rows of x, straight from the BYTE codes of W (antq_linear8)
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// k_linear4's launch shape (antq_k_linear4.h: lin4_rows, Lin4X, lin4_wave_sum) with the byte decoder's rule
// (antq_k_decbatch8.h: dec8_book, dec8_slot, Dec8Out), so that W[n, k] IS the element antq_decode8 writes.
//
//   ownership  one-wavefront workgroups, no barrier, no shared state; a wavefront owns R = lin4_rows(M) consecutive output
//              rows over the whole of K
//   loads      codes straight to VGPRs, nontemporal, 16 B (VEC: 16 elements) or 8 B (8 elements) per lane and row, the next
//              step's in flight while this one is computed; x as in k_linear4: plain cached 16-byte loads, one step ahead
//              where that costs few registers
//   decode     a wave-private table of 256 FINISHED outputs per row (per tensor: one), keyed by the code byte, and with the
//              pair rule a second one for the outlier list; entry 255 of both is +0.  An entry is the decoder's own
//              Dec8Out<T>::make(g * s) stored already widened to fp32 (the widening is exact): an element is one ds_read_b32
//              at dec8_slot(c, c_partner) and no conversion.  R x 512 x 4 B = 8 KB of LDS at the most.
//   sum        acc[m][r] = fmaf(x, w, acc) in fp32, lane l over its own k in rising order; then lin4_wave_sum once per
//              value.  The sequence of operations that makes y[m, n] depends on K and on the code path (8 or 16 B per lane)
//              only -- not on M, R, N or the other rows of x.
//   store      lane i keeps value i: bias added in fp32, rounded to the output type, one element store per lane
#ifndef ANTQ_K_LINEAR8_H
#define ANTQ_K_LINEAR8_H

#include "antq_k_decbatch8.h"
#include "antq_k_linear4.h"

namespace antq {

// a finished output of the decoder -> the same value as fp32 (exact)
template <typename T> struct Lin8W;
template <> struct Lin8W<float> {
    __device__ __forceinline__ static float widen(uint32_t e) { return u2f(e); }
};
template <> struct Lin8W<bf16_tag> {
    __device__ __forceinline__ static float widen(uint16_t e) { return u2f((uint32_t)e << 16); }
};
template <> struct Lin8W<f16_tag> {
    __device__ __forceinline__ static float widen(uint16_t e) { return IO<f16_tag>::h2f(e); }
};

// M: rows of x the kernel computes (rows >= m_rows repeat the last one and are not stored); VEC: 16 B of codes per lane
template <typename T, bool OVP, int M, bool VEC>
__global__ void __launch_bounds__(64)
k_linear8(const uint8_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
          uint32_t m_rows, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
          const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
    constexpr int R = lin4_rows(M);
    constexpr int W = VEC ? 2 : 1;                     // groups of 8 elements (two code words) per lane, row and step
    constexpr int XV = Lin4X<T>::V;
    constexpr bool XP = M * XV <= 2;                   // x one step ahead in registers too (where that is few registers)
    constexpr uint32_t TS = OVP ? 512u : 256u;         // entries of one row's table(s)
    __shared__ float tab[R * TS];
    const uint32_t lane = threadIdx.x;
    const uint32_t row0 = __builtin_amdgcn_readfirstlane(blockIdx.x) * (uint32_t)R;
    const uint32_t upr = K / (8u * W);                 // a lane's load units per row (VEC: K % 16 == 0)
    const uint32_t steps = (upr + 63u) >> 6;
    const ANTQ_GLOBAL uint8_t *crow[R];
    const char *xrow[M];
#pragma unroll
    for (int r = 0; r < R; r++) crow[r] = (const ANTQ_GLOBAL uint8_t *)(codes) + (size_t)min(row0 + r, N - 1u) * K;
#pragma unroll
    for (int i = 0; i < M; i++) xrow[i] = static_cast<const char *>(x) + (size_t)min((uint32_t)i, m_rows - 1u) * K * IO<T>::ESIZE;

    uint32_t cw[R][2 * W], nw[R][2 * W];
    uint4 xc[XP ? M : 1][W][XV], xn[XP ? M : 1][W][XV];
    auto load_step = [&](uint32_t s, uint32_t (&w)[R][2 * W], uint4 (&xs)[XP ? M : 1][W][XV]) {
        const uint32_t u = min(s * 64u + lane, upr - 1u);          // (lanes past the row's end repeat its last unit, unused)
#pragma unroll
        for (int r = 0; r < R; r++) {
            if constexpr (VEC) {
                const u32x4_t v = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x4_t *)(crow[r]) + u);
                w[r][0] = v.x; w[r][1] = v.y; w[r][2] = v.z; w[r][3] = v.w;
            } else {
                const u32x2_t v = __builtin_nontemporal_load((const ANTQ_GLOBAL u32x2_t *)(crow[r]) + u);
                w[r][0] = v.x; w[r][1] = v.y;
            }
        }
        if constexpr (XP) {
#pragma unroll
            for (int i = 0; i < M; i++)
#pragma unroll
                for (int j = 0; j < W; j++) Lin4X<T>::load(xrow[i], ((size_t)u * W + j) * 8u, xs[i][j]);
        }
    };
    load_step(0u, cw, xc);                              // in flight while the tables are built

    // the decoder's own table: dec8_book, s = a / gmax, Dec8Out<T>::make -- kept as fp32
    {
        DecDesc D;
        D.grid = grid; D.m = m; D.n_normal = n_normal;
        float nv[4], ov[4];
        dec8_book<OVP>(D, lane, nv, ov);
        for (int r = 0; r < (per_row ? R : 1); r++) {
            const float a = ld_global(alpha + (per_row ? min(row0 + r, N - 1u) : 0u));
            const float s = a / gmax;                   // AQ:536 scale = alpha / max(grid)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t b = lane + 64u * k;
                tab[r * TS + b] = Lin8W<T>::widen(Dec8Out<T>::make(nv[k] * s));
                if (OVP) tab[r * TS + 256u + b] = Lin8W<T>::widen(Dec8Out<T>::make(ov[k] * s));
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t tstride = per_row ? TS : 0u;        // one scale per tensor: one table

    float acc[M][R];
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
        for (int r = 0; r < R; r++) acc[i][r] = 0.0f;

    for (uint32_t s = 0; s < steps; s++) {
        const bool more = s + 1u < steps;
        if (more) load_step(s + 1u, nw, xn);
        const uint32_t u = s * 64u + lane;
        if (u < upr) {
#pragma unroll
            for (int j = 0; j < W; j++) {
                float xf[M][8];
#pragma unroll
                for (int i = 0; i < M; i++) {
                    if constexpr (XP) Lin4X<T>::unpack(xc[i][j], xf[i]);
                    else {
                        uint4 xv[XV];
                        Lin4X<T>::load(xrow[i], ((size_t)u * W + j) * 8u, xv);
                        Lin4X<T>::unpack(xv, xf[i]);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float *t = tab + r * tstride;
                    uint32_t c[8];
#pragma unroll
                    for (int e = 0; e < 4; e++) { c[e] = (cw[r][2 * j] >> (8 * e)) & 0xffu; c[4 + e] = (cw[r][2 * j + 1] >> (8 * e)) & 0xffu; }
                    float wv[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) wv[e] = t[dec8_slot<OVP>(c[e], c[e ^ 1])];    // (flat pairs (2k, 2k + 1))
#pragma unroll
                    for (int e = 0; e < 8; e++)
#pragma unroll
                        for (int i = 0; i < M; i++) acc[i][r] = __builtin_fmaf(xf[i][e], wv[e], acc[i][r]);
                }
            }
        }
        if (!more) break;
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int j = 0; j < 2 * W; j++) cw[r][j] = nw[r][j];
        if constexpr (XP) {
#pragma unroll
            for (int i = 0; i < M; i++)
#pragma unroll
                for (int j = 0; j < W; j++)
#pragma unroll
                    for (int v = 0; v < XV; v++) xc[i][j][v] = xn[i][j][v];
        }
    }

    // value i * R + r ends up in lane i * R + r
    float mine = 0.0f;
#pragma unroll
    for (int i = 0; i < M; i++) {
        // (an empty statement that ties this row's sums to the ones before: R values at a time -- all M * R in flight at once
        // hold four SGPRs each and spill)
#pragma unroll
        for (int r = 0; r < R; r++) asm volatile("" : "+v"(acc[i][r]), "+v"(mine));
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float t = lin4_wave_sum(acc[i][r]);
            if (lane == (uint32_t)(i * R + r)) mine = t;
        }
    }
    const uint32_t i = lane / (uint32_t)R, r = lane % (uint32_t)R, row = row0 + r;
    if (i < m_rows && i < (uint32_t)M && row < N) {
        if (bias) mine += IO<T>::load1(bias, row);
        IO<T>::store1(y, (size_t)i * N + row, mine);
    }
}

}  // namespace antq

#endif  // ANTQ_K_LINEAR8_H
