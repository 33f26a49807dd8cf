// antq_k_linear4.h -- the packed 4-bit codec of the row-streaming linear (antq_k_linear.h: k_linear; antq_linear4), and the
// 4-bit byte table's one definition; the codec's last members are its part of the matrix-core kernel (antq_k_linear_mm.h:
// k_linear_mm; antq_linear4_mm).
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
//   loads      16 B (VEC: 32 elements) or 4 B (8 elements) of codes per lane and row
//   decode     a wave-private table of 256 entries per row (per tensor: one), keyed by the code BYTE, entry = the pair's two
//              finished outputs in the output type -- the decoder's own byte table (dec_pair, antq_k_decbatch.h: DecOut),
//              so that W[n, k] IS the element antq_decode4 writes; per pair one ds_read_b32 (bf16 / f16) or ds_read_b64
//              (fp32) and the exact widening to fp32
#ifndef ANTQ_K_LINEAR4_H
#define ANTQ_K_LINEAR4_H

#include "antq_k_decbatch.h"
#include "antq_k_linear.h"
#include "antq_k_linear_mm.h"

namespace antq {

// The 4-bit byte table.  The codebook goes to LDS first (antq_device.h: dec4_book), and the caller orders its writes before
// the first Lin4Entry.
// entry b of the table of scale s = alpha / gmax (AQ:536 scale = alpha / max(grid)): the decoded pair of code byte b, then
// both finished outputs in the output type
template <typename T, bool OVP> struct Lin4Entry {
    float q0, q1;
    __device__ __forceinline__ Lin4Entry(uint32_t b, const float *g, int n_normal) { dec_pair<OVP>(b, g, n_normal, q0, q1); }
    __device__ __forceinline__ typename DecOut<T>::Ent at(float s) const { return DecOut<T>::make(q0 * s, q1 * s); }
};

// a table entry -> the pair's two weights as fp32 (exact widening of the output type)
template <typename T> struct Lin4W;
template <> struct Lin4W<float> {
    __device__ __forceinline__ static void get(const uint2 &e, float &a, float &b) { a = u2f(e.x); b = u2f(e.y); }
};
template <> struct Lin4W<bf16_tag> {
    __device__ __forceinline__ static void get(uint32_t e, float &a, float &b) { a = u2f(e << 16); b = u2f(e & 0xffff0000u); }
};
template <> struct Lin4W<f16_tag> {
    __device__ __forceinline__ static void get(uint32_t e, float &a, float &b)
    {
        a = IO<f16_tag>::h2f(e & 0xffffu);
        b = IO<f16_tag>::h2f(e >> 16);
    }
};

template <typename T, bool OVP> struct Lin4Codec {
    typedef T Out;
    typedef typename DecOut<T>::Ent Ent;
    typedef uint32_t Narrow;                            // one code word is 8 elements
    static constexpr int WORDS = 1;
    static constexpr uint32_t TS = 256u;
    static constexpr bool TIE = false;
    static constexpr bool PAIR = OVP;                   // (antq_k_linear_gemm.h builds this codec's tables in place)
    template <int R> struct Lds {
        __attribute__((aligned(16))) Ent tab[R * 256];
        float g[32];
    };
    __device__ __forceinline__ static size_t row_bytes(uint32_t K) { return (size_t)(K >> 3) * 4u; }

    template <int R>
    __device__ __forceinline__ static void build(Lds<R> &L, uint32_t lane, uint32_t row0, uint32_t N, const float *alpha, int per_row,
                                                 float gmax, const float *grid, uint32_t m, int n_normal)
    {
        dec4_book(L.g, lane, grid, m);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // this lane's four decoded pairs once, before any table is written: the R tables differ in the scale only
        const Lin4Entry<T, OVP> e[4] = {{lane, L.g, n_normal}, {lane + 64u, L.g, n_normal}, {lane + 128u, L.g, n_normal}, {lane + 192u, L.g, n_normal}};
        for (int r = 0; r < (per_row ? R : 1); r++) {
            const float a = ld_global(alpha + (per_row ? min(row0 + r, N - 1u) : 0u));
            const float s = a / gmax;                   // AQ:536 scale = alpha / max(grid)
#pragma unroll
            for (int k = 0; k < 4; k++) L.tab[r * 256 + lane + 64u * k] = e[k].at(s);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // contract (2) of antq_k_linear.h: every acc[i][r] takes its weights in the order e = 0 .. 7 (pair p: 2 p, then 2 p + 1)
    template <int M, int R>
    __device__ __forceinline__ static void fma8(const Ent *t, const uint32_t *w, const float (&xf)[M][8], float (&acc)[M][R], int r)
    {
        Ent e[4];
#pragma unroll
        for (int p = 0; p < 4; p++) e[p] = t[(w[0] >> (8 * p)) & 0xffu];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float w0, w1;
            Lin4W<T>::get(e[p], w0, w1);
#pragma unroll
            for (int i = 0; i < M; i++) {
                acc[i][r] = __builtin_fmaf(xf[i][2 * p], w0, acc[i][r]);
                acc[i][r] = __builtin_fmaf(xf[i][2 * p + 1], w1, acc[i][r]);
            }
        }
    }

    // The matrix-core kernel's part (antq_k_linear_mm.h: k_linear_mm): the same table for 16 NT rows, built by 512 threads
    // with the codebook and the rows' scales staged in LDS.
    typedef Ent MmEnt;
    template <int ROWS> struct MmLds {
        __attribute__((aligned(16))) Ent tab[ROWS * 256];
        float g[32];
        float sc[ROWS];
    };
    // (the 64 x 64 tile with 16 B of codes per lane has no registers for x in the ring)
    static constexpr bool mm_x_in_ring(int MT, int NT, bool VEC) { return !(MT == 4 && NT == 4 && VEC); }
    static constexpr bool mm_tail_in_ring(int, int, bool) { return false; }

    template <int ROWS>
    __device__ __forceinline__ static void mm_build(MmLds<ROWS> &L, uint32_t tid, uint32_t row0, uint32_t N, const float *alpha, int per_row,
                                                    float gmax, const float *grid, uint32_t m, int n_normal)
    {
        dec4_book(L.g, tid, grid, m);
        if (tid < (per_row ? (uint32_t)ROWS : 1u)) L.sc[tid] = ld_global(alpha + (per_row ? min(row0 + tid, N - 1u) : 0u)) / gmax;   // AQ:536 scale = alpha / max(grid)
        __syncthreads();
        const uint32_t b = tid & 255u;                 // threads b and 256 + b make entry b of the even and the odd tables
        const Lin4Entry<T, OVP> e(b, L.g, n_normal);
        for (uint32_t r = tid >> 8; r < (per_row ? (uint32_t)ROWS : 1u); r += 2u) L.tab[r * 256u + b] = e.at(L.sc[r]);
        __syncthreads();
    }

    // one code word is the step's 8 elements: four look-ups ARE the four operand registers
    __device__ __forceinline__ static u32x4_t mm_b(const Ent *t, const uint32_t *w)
    {
        return u32x4_t{t[w[0] & 0xffu], t[(w[0] >> 8) & 0xffu], t[(w[0] >> 16) & 0xffu], t[w[0] >> 24]};
    }
};

}  // namespace antq

#endif  // ANTQ_K_LINEAR4_H
