// antq_k_linear8.h -- the BYTE-code codec of the row-streaming linear (antq_k_linear.h: k_linear; antq_linear8): the byte
// decoder's rule (antq_k_decbatch8.h: dec8_book, dec8_slot, Dec8Out), so that W[n, k] IS the element antq_decode8 writes.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
//   loads      16 B (VEC: 16 elements) or 8 B (8 elements) of codes per lane and row
//   decode     a wave-private table of 256 FINISHED outputs per row (per tensor: one), keyed by the code byte, and with the
//              pair rule a second one for the outlier list; entry 255 of both is +0.  An entry is the decoder's own
//              Dec8Out<T>::make(g * s) stored already widened to fp32 (the widening is exact): an element is one ds_read_b32
//              at dec8_slot(c, c_partner) and no conversion.  R x 512 x 4 B = 8 KB of LDS at the most.
#ifndef ANTQ_K_LINEAR8_H
#define ANTQ_K_LINEAR8_H

#include "antq_k_decbatch8.h"
#include "antq_k_linear.h"

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

template <typename T, bool OVP> struct Lin8Codec {
    typedef T Out;
    typedef unsigned int Narrow __attribute__((ext_vector_type(2)));   // two code words are 8 elements
    static constexpr int WORDS = 2;
    static constexpr uint32_t TS = OVP ? 512u : 256u;  // entries of one row's table(s)
    static constexpr bool TIE = true;
    template <int R> struct Lds { float tab[R * TS]; };
    __device__ __forceinline__ static size_t row_bytes(uint32_t K) { return K; }

    // the decoder's own table: dec8_book, s = a / gmax, Dec8Out<T>::make -- kept as fp32
    template <int R>
    __device__ __forceinline__ static void build(Lds<R> &L, uint32_t lane, uint32_t row0, uint32_t N, const float *alpha, int per_row,
                                                 float gmax, const float *grid, uint32_t m, int n_normal)
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
                L.tab[r * TS + b] = Lin8W<T>::widen(Dec8Out<T>::make(nv[k] * s));
                if (OVP) L.tab[r * TS + 256u + b] = Lin8W<T>::widen(Dec8Out<T>::make(ov[k] * s));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // contract (2) of antq_k_linear.h: every acc[i][r] takes its weights in the order e = 0 .. 7
    template <int M, int R>
    __device__ __forceinline__ static void fma8(const float *t, const uint32_t *w, const float (&xf)[M][8], float (&acc)[M][R], int r)
    {
        uint32_t c[8];
#pragma unroll
        for (int e = 0; e < 4; e++) { c[e] = (w[0] >> (8 * e)) & 0xffu; c[4 + e] = (w[1] >> (8 * e)) & 0xffu; }
        float wv[8];
#pragma unroll
        for (int e = 0; e < 8; e++) wv[e] = t[dec8_slot<OVP>(c[e], c[e ^ 1])];    // (flat pairs (2k, 2k + 1))
#pragma unroll
        for (int e = 0; e < 8; e++)
#pragma unroll
            for (int i = 0; i < M; i++) acc[i][r] = __builtin_fmaf(xf[i][e], wv[e], acc[i][r]);
    }
};

}  // namespace antq

#endif  // ANTQ_K_LINEAR8_H
