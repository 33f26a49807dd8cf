// antq_k_linear.h -- y = x . W^T (+ bias) for 1 .. 8 rows of x, straight from the packed codes of W: the row-streaming kernel
// of antq_linear4 and antq_linear8, written once.  A codec (antq_k_linear4.h: Lin4Codec, antq_k_linear8.h: Lin8Codec) says
// how wide a code is, how the decoder's table is built and how 8 weights come out of a lane's code words; everything else is here.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// With few rows of x a linear layer is a weight stream: every weight is used M times and never again.  The codes are a
// quarter (4-bit) or half (bytes) of the bf16 image's bytes, so the kernel streams them and makes the image's values on the
// fly -- through the decoder's own table, so that W[n, k] IS the element antq_decode4 / antq_decode8 writes.
//
//   ownership  one-wavefront workgroups, no barrier, no shared state; a wavefront owns R consecutive output rows over the
//              whole of K (R = 2 for M <= 2, 4 beyond: more wavefronts where the kernel is a stream, more reuse of the
//              unpacked x where it is arithmetic)
//   loads      codes straight to VGPRs, nontemporal, 16 B (VEC) or the codec's narrow load (8 elements) per lane and row, the
//              next step's in flight while this one is computed; x is re-read by every wavefront and lives in L2: plain
//              cached 16-byte loads, one step ahead as well where that costs few registers (M <= 2; fp32: M = 1)
//   decode     a wave-private table per row (per tensor: one), keyed by the code BYTE: the codec's
//   sum        acc[m][r] = fmaf(x, w, acc) in fp32, lane l over its own k in rising order; then ONE cross-lane reduction in
//              a fixed pattern: four DPP steps inside each row of 16 lanes, the four row sums as (r0 + r1) + (r2 + r3).
//              Two contracts, for both codecs:
//              (1) The sequence of operations that makes y[m, n] depends on K and on the code path only (the narrow load
//                  or 16 B per lane, which follows K and the alignment of the codes) -- not on M, not on N, not on the other
//                  rows of x, not on R: a row computed alone has the bits it has in a call of 8.
//              (2) The fmaf order is rising k per lane, both elements of a pair in order, then lin_wave_sum's fixed tree.
//   store      lane i keeps value i: bias added in fp32, rounded to the output type, one element store per lane
#ifndef ANTQ_K_LINEAR_H
#define ANTQ_K_LINEAR_H

#include <type_traits>

#include "antq_device.h"

namespace antq {

constexpr int lin_rows(int M) { return M <= 2 ? 2 : 4; }       // R: output rows per wavefront

// 8 consecutive elements of x (the first at a multiple of 8: 16-byte aligned) as raw vectors, and as floats
template <typename T> struct LinX {
    static constexpr int V = 1;
    __device__ __forceinline__ static void load(const void *x, size_t elem, uint4 (&v)[1]) { v[0] = ld_global(static_cast<const uint4 *>(x) + elem / 8); }
    __device__ __forceinline__ static void unpack(const uint4 (&v)[1], float (&f)[8]) { IO<T>::unpack(v[0], f); }
};
template <> struct LinX<float> {
    static constexpr int V = 2;
    __device__ __forceinline__ static void load(const void *x, size_t elem, uint4 (&v)[2])
    {
        const uint4 *p = static_cast<const uint4 *>(x) + elem / 4;
        v[0] = ld_global(p);
        v[1] = ld_global(p + 1);
    }
    __device__ __forceinline__ static void unpack(const uint4 (&v)[2], float (&f)[8])
    {
        f[0] = u2f(v[0].x); f[1] = u2f(v[0].y); f[2] = u2f(v[0].z); f[3] = u2f(v[0].w);
        f[4] = u2f(v[1].x); f[5] = u2f(v[1].y); f[6] = u2f(v[1].z); f[7] = u2f(v[1].w);
    }
};

template <int CTRL>
__device__ __forceinline__ float lin_dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// the sum over the 64 lanes, the same tree for every value; all lanes active
__device__ __forceinline__ float lin_wave_sum(float v)
{
    v += lin_dpp<0xB1>(v);                              // quad_perm [1,0,3,2]
    v += lin_dpp<0x4E>(v);                              // quad_perm [2,3,0,1]
    v += lin_dpp<0x141>(v);                             // row_half_mirror
    v += lin_dpp<0x140>(v);                             // row_mirror: every lane of a row of 16 holds the row's sum
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// a loaded scalar or vector of N words -> its words
template <int N> struct LinWords { uint32_t w[N]; };
template <typename V, int N>
__device__ __forceinline__ void lin_words(const V &v, uint32_t (&w)[N])
{
    const LinWords<N> t = __builtin_bit_cast(LinWords<N>, v);
#pragma unroll
    for (int j = 0; j < N; j++) w[j] = t.w[j];
}

// C: the codec.  It names
//     Out                      the output type T (x, bias and y are of it)
//     WORDS                    32-bit code words that hold 8 elements
//     Narrow                   the type of the narrow nontemporal load: WORDS words
//     TIE                      whether the final sums are tied R at a time (below)
//     row_bytes(K)             the bytes of one row of codes
//     Lds<R>, TS               the tables of R rows in LDS, `tab` their entries, TS entries per row
//     build<R>(lds, ...)       builds them, ordered before the wavefront's reads
//     fma8(t, w, xf, acc, r)   the 8 weights of the WORDS code words w as fp32 (exact widening; t = the row's table) and
//                              acc[i][r] = fmaf(xf[i][e], weight e, acc[i][r]) for e = 0 .. 7 in this order, every i.  The
//                              loop is the codec's because its shape sets the register count: pair by pair as the entries
//                              are widened (4-bit), or all eight weights first (bytes); the other shape costs each of them
//                              occupancy (profiles/packed_linear_refactor.md).  No sum depends on it: contract (2).
// M: rows of x the kernel computes (rows >= m_rows repeat the last one and are not stored); VEC: 16 B of codes per lane
template <typename C, int M, bool VEC>
__global__ void __launch_bounds__(64)
k_linear(const uint8_t *__restrict__ codes, const void *__restrict__ x, const void *__restrict__ bias, void *__restrict__ y,
         uint32_t m_rows, uint32_t N, uint32_t K, const float *__restrict__ alpha, int per_row, float gmax,
         const float *__restrict__ grid, uint32_t m, int n_normal)
{
    typedef typename C::Out T;
    typedef std::conditional_t<VEC, u32x4_t, typename C::Narrow> Load;
    constexpr int R = lin_rows(M);
    constexpr int CW = sizeof(Load) / 4;               // code words per lane, row and step
    constexpr int W = CW / C::WORDS;                   // groups of 8 elements per lane, row and step
    constexpr int XV = LinX<T>::V;
    constexpr bool XP = M * XV <= 2;                   // x one step ahead in registers too (where that is few registers)
    __shared__ typename C::template Lds<R> lds;
    const uint32_t lane = threadIdx.x;
    const uint32_t row0 = __builtin_amdgcn_readfirstlane(blockIdx.x) * (uint32_t)R;
    const uint32_t upr = K / (8u * W);                 // a lane's load units per row (VEC: K a multiple of 8 W)
    const uint32_t steps = (upr + 63u) >> 6;
    const ANTQ_GLOBAL uint8_t *crow[R];
    const char *xrow[M];
#pragma unroll
    for (int r = 0; r < R; r++) crow[r] = (const ANTQ_GLOBAL uint8_t *)(codes) + (size_t)min(row0 + r, N - 1u) * C::row_bytes(K);
#pragma unroll
    for (int i = 0; i < M; i++) xrow[i] = static_cast<const char *>(x) + (size_t)min((uint32_t)i, m_rows - 1u) * K * IO<T>::ESIZE;   // (the 16-bit tags are empty types)

    uint32_t cw[R][CW], nw[R][CW];
    uint4 xc[XP ? M : 1][W][XV], xn[XP ? M : 1][W][XV];
    auto load_step = [&](uint32_t s, uint32_t (&w)[R][CW], uint4 (&xs)[XP ? M : 1][W][XV]) {
        const uint32_t u = min(s * 64u + lane, upr - 1u);          // (lanes past the row's end repeat its last unit, unused)
#pragma unroll
        for (int r = 0; r < R; r++) lin_words(__builtin_nontemporal_load((const ANTQ_GLOBAL Load *)(crow[r]) + u), w[r]);
        if constexpr (XP) {
#pragma unroll
            for (int i = 0; i < M; i++)
#pragma unroll
                for (int j = 0; j < W; j++) LinX<T>::load(xrow[i], ((size_t)u * W + j) * 8u, xs[i][j]);
        }
    };
    load_step(0u, cw, xc);                              // in flight while the tables are built

    C::template build<R>(lds, lane, row0, N, alpha, per_row, gmax, grid, m, n_normal);
    const uint32_t tstride = per_row ? C::TS : 0u;     // one scale per tensor: one table

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
                    if constexpr (XP) LinX<T>::unpack(xc[i][j], xf[i]);
                    else {
                        uint4 xv[XV];
                        LinX<T>::load(xrow[i], ((size_t)u * W + j) * 8u, xv);
                        LinX<T>::unpack(xv, xf[i]);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; r++) C::fma8(lds.tab + r * tstride, &cw[r][C::WORDS * j], xf, acc, r);
            }
        }
        if (!more) break;
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int j = 0; j < CW; j++) cw[r][j] = nw[r][j];
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
        if constexpr (C::TIE) {
#pragma unroll
            for (int r = 0; r < R; r++) asm volatile("" : "+v"(acc[i][r]), "+v"(mine));
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float t = lin_wave_sum(acc[i][r]);
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

#endif  // ANTQ_K_LINEAR_H
