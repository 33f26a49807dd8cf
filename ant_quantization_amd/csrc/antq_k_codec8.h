// antq_k_codec8.h -- byte-code encoder (antq_encode8): one code per element, books of up to 256 values (pair rule: 255 + 255)
// Part of libantq's single device translation unit (antq_kernels.hip includes it); gfx950 only.
//
// The element encoder of antq_k_codec.h (k_encode) at the byte width: what is here is only what a byte changes -- the
// identifier 255 instead of 15, a unit of 8 or 4 elements (row_len % 8 == 4: two pairs, still inside one row) that becomes
// two code words or one, and codes at any byte address.  No row-table and no 16-bit-domain form: byte codes are encoded
// once per model.
#ifndef ANTQ_K_CODEC8_H
#define ANTQ_K_CODEC8_H

#include "antq_k_codec.h"
#include "antq_decbatch8.h"

namespace antq {

struct Code8 {
    static constexpr int BITS = 8;
    static constexpr uint32_t IDENT = kDec8Ident;
    typedef uint8_t Store;
    static constexpr bool unit_ok(int E) { return E == 8 || E == 4; }
    static bool book_ok(int m, int n_normal, bool ovp) { return dec8_book_ok(m, n_normal, ovp); }
    template <bool OVP, int E>
    __device__ __forceinline__ static void pack(uint32_t (&c)[E], uint32_t (&w)[E / 4])
    {
#pragma unroll
        for (int p = 0; p < E / 2; p++)
            if (OVP) pair_rule(c[2 * p], c[2 * p + 1], IDENT);
#pragma unroll
        for (int q = 0; q < E / 4; q++)
            w[q] = (c[4 * q] & 255u) | ((c[4 * q + 1] & 255u) << 8) | ((c[4 * q + 2] & 255u) << 16) | ((c[4 * q + 3] & 255u) << 24);
    }
    // words: codes is 4-byte aligned -> word stores, otherwise byte stores
    template <int N>
    __device__ __forceinline__ static void store(uint8_t *codes, size_t o, const uint32_t (&w)[N], int words)
    {
        if (words) {
#pragma unroll
            for (int q = 0; q < N; q++) reinterpret_cast<uint32_t *>(codes)[o * N + q] = w[q];
        } else {
#pragma unroll
            for (int e = 0; e < 4 * N; e++) codes[o * (4 * N) + e] = (uint8_t)(w[e / 4] >> (8 * (e % 4)));
        }
    }
};

template <typename T>
static int launch_encode8(const void *x, uint8_t *codes, size_t rows, size_t row_len, const float *alpha, int per_row, float gmax,
                          const PlanArgs &pa, const void *plan_host, const void *plan_dev, int n_normal, bool ovp, hipStream_t st)
{
    if (codec_refuses<Code8>(row_len, 4, pa, n_normal, ovp)) return ANTQ_ERR_UNSUPPORTED;
    if (rows > (size_t)-1 / row_len) return ANTQ_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(x) % IO<T>::ESIZE) return ANTQ_ERR_ALIGN;
    const int E = row_len % 8 == 0 ? 8 : 4;
    const size_t n_units = rows * row_len / E;
    const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0;     // 16-byte vector I/O (a quad of a 16-bit type: 8 bytes)
    size_t n_tasks;
    dim3 gd;
    if (!codec_tasks(n_units, vec ? 256 * kEncU : 256, true, n_tasks, gd)) return ANTQ_ERR_UNSUPPORTED;
    const int zero_code = codec_zero_code(plan_host, pa, n_normal, ovp);
    const int words = reinterpret_cast<uintptr_t>(codes) % 4 == 0 ? 1 : 0;
    return launch_encode_units<Code8, T>(E, x, codes, n_units, row_len, n_tasks, gd, vec, alpha, per_row, gmax, n_normal, zero_code, pa,
                                         plan_dev, ovp, words, st);
}

}  // namespace antq

#endif  // ANTQ_K_CODEC8_H
