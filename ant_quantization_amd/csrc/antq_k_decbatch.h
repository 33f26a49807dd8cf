// antq_k_decbatch.h -- batched packed-4-bit decoder: many tensors' codes -> their fake-quant images in ONE launch
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// The decoder is write-bound (0.5 B of codes read, 2 / 4 B written per element) and has no arithmetic worth the name, so
// the launch is shaped like the streaming kernels that measured best here (antq_k_batch.h): one-wavefront workgroups, no
// barrier, 16-byte nontemporal stores, 1 KiB contiguous per store instruction.  A pair (2k, 2k + 1) lives in one code
// byte, so a row task first builds a wave-private table of 256 entries keyed by that BYTE -- entry = the two finished
// outputs of the pair: fl((g + 0) * s) rounded to the output type, OliVe's pair rule applied -- four entries per lane; then
// every pair is one LDS read (ds_read_b32 for bf16 / f16, ds_read_b64 for fp32) and nothing else.  Tasks of short rows and
// of unaligned jobs decode element by element from the 16-entry codebook, with a scale per lane.
// Every output is bit-identical to antq_decode4 (antq_k_codec.h: k_decode4) on the same job.
#ifndef ANTQ_K_DECBATCH_H
#define ANTQ_K_DECBATCH_H

#include "antq_decbatch.h"
#include "antq_device.h"

namespace antq {

// (the decoded pair of one code byte, dec_pair, and the codebook's load, dec4_book: antq_device.h)
template <typename T> struct DecOut;          // two finished outputs -> the words the table / the store holds
template <> struct DecOut<float> {
    typedef uint2 Ent;                          // fp32: an entry is the pair's two words
    __device__ __forceinline__ static Ent make(float a, float b) { return make_uint2(f2u(a), f2u(b)); }
};
template <> struct DecOut<bf16_tag> {
    typedef uint32_t Ent;
    __device__ __forceinline__ static Ent make(float a, float b) { return IO<bf16_tag>::pk(a, b); }
};
template <> struct DecOut<f16_tag> {
    typedef uint32_t Ent;
    __device__ __forceinline__ static Ent make(float a, float b) { return IO<f16_tag>::f2h(a) | (IO<f16_tag>::f2h(b) << 16); }
};

// One output vector from its code bytes through the byte table: 4 pairs (16-bit types, one code word) or 2 (fp32, half a word).
template <typename T>
__device__ __forceinline__ uint4 dec_vec_tab(uint32_t w, const typename DecOut<T>::Ent *tab)
{
    if constexpr (sizeof(typename DecOut<T>::Ent) == 8) {
        const uint2 a = tab[w & 0xffu], b = tab[(w >> 8) & 0xffu];
        return make_uint4(a.x, a.y, b.x, b.y);
    } else {
        return make_uint4(tab[w & 0xffu], tab[(w >> 8) & 0xffu], tab[(w >> 16) & 0xffu], tab[w >> 24]);
    }
}

// One task of a row job: u x 64 vectors of one row.
template <typename T, bool OVP, int U>
__device__ __forceinline__ void dec_row_task(const DecDesc &D, uint32_t task, const float *g, typename DecOut<T>::Ent *tab, uint32_t lane)
{
    constexpr int EPL = IO<T>::EPL;
    uint32_t row = task, t = 0;
    if (D.tpr != 1u) { row = task / D.tpr; t = task - row * D.tpr; }
    const uint32_t vpr = D.vpr, v0 = t * (64u * U) + lane;
    const size_t base = (size_t)row * vpr;
    // the code words of this lane's vectors first: they are in flight while the table is built
    uint32_t w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t v = base + min(v0 + 64u * u, vpr - 1u);
        if (EPL == 8) w[u] = __builtin_nontemporal_load(((const ANTQ_GLOBAL uint32_t *)(D.codes)) + v);
        else w[u] = (uint32_t)__builtin_nontemporal_load(((const ANTQ_GLOBAL uint16_t *)(D.codes)) + v);
    }
    const float a = ld_global(D.alpha + (D.per_row ? row : 0u));
    const float s = a / D.gmax;                       // AQ:536 scale = alpha / max(grid)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t b = lane + 64u * k;
        float q0, q1;
        dec_pair<OVP>(b, g, D.n_normal, q0, q1);
        tab[b] = DecOut<T>::make(q0 * s, q1 * s);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint4 *out = static_cast<uint4 *>(D.out) + base;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t v = v0 + 64u * u;
        const uint4 o = dec_vec_tab<T>(w[u], tab);
        if (v < vpr) st_stream(out + v, o);
    }
}

// Short rows: u x 64 vectors of the flat tensor, the scale per lane.  ELEM: octets with byte loads and element stores.
template <typename T, bool OVP, bool ELEM>
__device__ __forceinline__ void dec_lane_task(const DecDesc &D, uint32_t task, const float *g, uint32_t lane)
{
    constexpr int EPL = ELEM ? 8 : IO<T>::EPL;       // elements per unit
    constexpr int U = 4;
    static_assert(kDecElemU == 4, "task size of the element-granular kind");
    const uint64_t n_units = D.n_units, first = (uint64_t)task * (64u * U) + lane;
    const uint32_t upr = D.vpr;
    uint32_t w[U];
    float a[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t t = first + 64u * u;
        w[u] = 0u;
        a[u] = 1.0f;
        if (t < n_units) {
            if (ELEM) {
                const ANTQ_GLOBAL uint8_t *c = ((const ANTQ_GLOBAL uint8_t *)(D.codes)) + t * 4u;
                w[u] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
            } else if (EPL == 8) w[u] = ((const ANTQ_GLOBAL uint32_t *)(D.codes))[t];
            else w[u] = (uint32_t) ((const ANTQ_GLOBAL uint16_t *)(D.codes))[t];
            // (row_len % 8 == 0: a unit lies inside one row)
            a[u] = ld_global(D.alpha + (D.per_row ? (n_units <= 0xffffffffull ? (uint64_t)((uint32_t)t / upr) : t / upr) : 0u));
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t t = first + 64u * u;
        if (t >= n_units) continue;
        const float s = a[u] / D.gmax;
        float of[EPL];
#pragma unroll
        for (int p = 0; p < EPL / 2; p++) {
            float q0, q1;
            dec_pair<OVP>(w[u] >> (8 * p), g, D.n_normal, q0, q1);
            of[2 * p] = q0 * s;
            of[2 * p + 1] = q1 * s;
        }
        if constexpr (ELEM) {
#pragma unroll
            for (int e = 0; e < EPL; e++) IO<T>::store1(D.out, t * EPL + e, of[e]);
        } else st_stream(static_cast<uint4 *>(D.out) + t, IO<T>::pack(of));
    }
}

template <typename T, bool OVP>
__global__ void __launch_bounds__(64)
k_decode4_batch(const DecDesc *__restrict__ descs, const uint32_t *__restrict__ block_map)
{
    __shared__ __attribute__((aligned(16))) typename DecOut<T>::Ent tab[256];
    __shared__ float g[32];
    uint32_t blk = blockIdx.x;
    const uint32_t g8 = blk >> 3;
    // (the decision belongs to the group of 8 workgroups: the job of its first task, antq_k_batch.h)
    if ((g8 << 3) + 8u <= gridDim.x && descs[block_map[(g8 << 3) >> 2]].rot) blk = (g8 << 3) + ((blk + g8) & 7u);
    const uint32_t b4 = blk >> 2, sub = blk & 3u;
    const DecDesc &D = descs[block_map[b4]];
    const uint32_t task = __builtin_amdgcn_readfirstlane((b4 - D.first_block) * 4u + sub);
    if (task >= D.total_tasks) return;
    const uint32_t lane = threadIdx.x;
    dec4_book(g, lane, D.grid, D.m);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (D.kind == kDecRow) {
        if (D.u == 4u) dec_row_task<T, OVP, 4>(D, task, g, tab, lane);
        else if (D.u == 3u) dec_row_task<T, OVP, 3>(D, task, g, tab, lane);
        else dec_row_task<T, OVP, 2>(D, task, g, tab, lane);
    } else if (D.kind == kDecLane) dec_lane_task<T, OVP, false>(D, task, g, lane);
    else dec_lane_task<T, OVP, true>(D, task, g, lane);
}

}  // namespace antq

#endif  // ANTQ_K_DECBATCH_H
