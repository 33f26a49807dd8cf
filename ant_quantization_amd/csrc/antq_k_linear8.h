// antq_k_linear8.h -- the BYTE-code codec of the row-streaming linear (antq_k_linear.h: k_linear; antq_linear8): the byte
// decoder's rule (antq_k_decbatch8.h: dec8_book, dec8_slot, Dec8Out), so that W[n, k] IS the element antq_decode8 writes.  The
// codec's last members are its part of the matrix-core kernel (antq_k_linear_mm.h: k_linear_mm; antq_linear8_mm).
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
#include "antq_k_linear_mm.h"

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

    // The matrix-core kernel's part (antq_k_linear_mm.h: k_linear_mm; bf16 / f16): the same tables for 16 NT rows, of the
    // decoder's finished 16-bit outputs as they are -- Dec8Out<T>::make(g * s), the multiplication done for every entry as the
    // decoder does it.  16 NT rows x 256 or 512 entries x 2 B: 64 KB at the most (NT = 4, pair rule), and nothing else lives
    // in LDS, so no variant needs more than the 64 KB every launch may have.
    typedef typename Dec8Out<T>::Ent MmEnt;
    template <int ROWS> struct MmLds {
        __attribute__((aligned(16))) MmEnt tab[ROWS * TS];
        static_assert(sizeof(MmEnt) == 2 && sizeof(tab) <= 65536, "two entries are one operand register; the tables fit every launch");
    };
    static constexpr bool mm_x_in_ring(int, int, bool) { return true; }
    // (with the pair rule these tiles sit on a register step: the partial chunk's own step after the ring cost them 3 - 4 VGPRs
    // and a wave per SIMD, the select inside the ring costs none -- profiles/packed_linear_specials.md)
    static constexpr bool mm_tail_in_ring(int MT, int NT, bool VEC) { return OVP && ((MT == 1 && NT == 2) || (MT == 2 && NT == 1 && !VEC)); }

    // Every wavefront holds the book in registers (dec8_book's four entries per lane) and builds whole rows r = w, w + NW, ...
    // of a workgroup of NW wavefronts: no staging array and no second barrier.
    template <int ROWS, int NW>
    __device__ __forceinline__ static void mm_rows(MmLds<ROWS> &L, uint32_t tid, uint32_t row0, uint32_t N, const float *alpha, int per_row,
                                                   float gmax, const float *grid, uint32_t m, int n_normal)
    {
        const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        DecDesc D;
        D.grid = grid; D.m = m; D.n_normal = n_normal;
        float nv[4], ov[4];
        dec8_book<OVP>(D, lane, nv, ov);
        for (uint32_t r = wave; r < (per_row ? (uint32_t)ROWS : 1u); r += (uint32_t)NW) {
            const float s = ld_global(alpha + (per_row ? min(row0 + r, N - 1u) : 0u)) / gmax;   // AQ:536 scale = alpha / max(grid)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t b = lane + 64u * k;
                L.tab[r * TS + b] = Dec8Out<T>::make(nv[k] * s);
                if (OVP) L.tab[r * TS + 256u + b] = Dec8Out<T>::make(ov[k] * s);
            }
        }
    }
    template <int ROWS>
    __device__ __forceinline__ static void mm_build(MmLds<ROWS> &L, uint32_t tid, uint32_t row0, uint32_t N, const float *alpha, int per_row,
                                                    float gmax, const float *grid, uint32_t m, int n_normal)
    {
        mm_rows<ROWS, kMmWaves>(L, tid, row0, N, alpha, per_row, gmax, grid, m, n_normal);
        __syncthreads();
    }
    // The tiled kernel's build (antq_k_linear_gemm.h: k_linear_gemm), for a workgroup of NW wavefronts: the same rows, strided by
    // ITS wavefront count.  No barrier at the end: the caller's next one orders the tables before the reads.
    template <int ROWS, int NW>
    __device__ __forceinline__ static void gemm_build(MmLds<ROWS> &L, uint32_t tid, uint32_t row0, uint32_t N, const float *alpha, int per_row,
                                                      float gmax, const float *grid, uint32_t m, int n_normal)
    {
        mm_rows<ROWS, NW>(L, tid, row0, N, alpha, per_row, gmax, grid, m, n_normal);
    }

    // two code words are the step's 8 elements; two 16-bit look-ups are one operand register
    __device__ __forceinline__ static u32x4_t mm_b(const MmEnt *t, const uint32_t *w)
    {
        uint32_t c[8];
#pragma unroll
        for (int e = 0; e < 4; e++) { c[e] = (w[0] >> (8 * e)) & 0xffu; c[4 + e] = (w[1] >> (8 * e)) & 0xffu; }
        uint32_t o[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {                   // (flat pairs (2k, 2k + 1): the partner is the byte next door)
            const uint32_t lo = t[dec8_slot<OVP>(c[2 * p], c[2 * p + 1])], hi = t[dec8_slot<OVP>(c[2 * p + 1], c[2 * p])];
            o[p] = lo | (hi << 16);
        }
        return u32x4_t{o[0], o[1], o[2], o[3]};
    }
};

}  // namespace antq

#endif  // ANTQ_K_LINEAR8_H
