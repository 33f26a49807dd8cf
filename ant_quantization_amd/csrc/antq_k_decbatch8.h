// antq_k_decbatch8.h -- byte-code decoder: one code per byte -> the fake-quant image; antq_decode8 (one tensor, its descriptor
// passed by value) and antq_decode8_batch (many tensors in ONE launch) run the same tasks.
// Part of libantq's batched translation unit (antq_batch.hip includes it); gfx950 only.
//
// The twin of antq_k_decbatch.h for books of up to 256 values (pair rule: 255 normal + 255 outlier values).  Write-bound
// (1 B of codes read, 2 / 4 B written per element), so the launch keeps the shape that measured best there: one-wavefront
// workgroups, no block barrier, the code words loaded nontemporally before the table is built, 16-byte nontemporal stores.
// A row task builds a wave-private table of 256 FINISHED outputs keyed by the code byte -- fl((g + 0) * s) rounded to the
// output type, four entries per lane straight from the codebook -- and, with the pair rule, a second one for the outlier
// list; entry 255 of both is +0 (255 is the identifier, never a value).  Every element is then one LDS read:
//     plain      out[i] = tab[c[i]]
//     pair rule  out[i] = tab[c[i] + (c[partner] == 255 ? 256 : 0)]      (a victim reads entry 255: +0)
// Codes beyond the book decode to +0.  Tasks of short rows and of unaligned jobs keep the unscaled codebook in the same LDS
// and scale per lane.
#ifndef ANTQ_K_DECBATCH8_H
#define ANTQ_K_DECBATCH8_H

#include "antq_decbatch8.h"
#include "antq_device.h"

namespace antq {

template <typename T> struct Dec8Out;          // one finished output -> the bits a table entry holds
template <> struct Dec8Out<float> {
    typedef uint32_t Ent;
    __device__ __forceinline__ static Ent make(float a) { return f2u(a); }
};
template <> struct Dec8Out<bf16_tag> {
    typedef uint16_t Ent;
    __device__ __forceinline__ static Ent make(float a) { return (uint16_t)(IO<bf16_tag>::pk(a, 0.0f) & 0xffffu); }
};
template <> struct Dec8Out<f16_tag> {
    typedef uint16_t Ent;
    __device__ __forceinline__ static Ent make(float a) { return (uint16_t)IO<f16_tag>::f2h(a); }
};

// This lane's four entries of the codebook (pair rule: of the normal list and of the outlier list), b = lane + 64 k.
// (+ 0.0f: a codebook's -0 decodes to +0, which is what the reference's (q - d) + d makes of it for every finite d)
template <bool OVP>
__device__ __forceinline__ void dec8_book(const DecDesc &D, uint32_t lane, float (&nv)[4], float (&ov)[4])
{
    const uint32_t nn = OVP ? (uint32_t)D.n_normal : D.m, no = OVP ? D.m - (uint32_t)D.n_normal : 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t b = lane + 64u * k;
        nv[k] = (b < nn && b < (OVP ? kDec8Ident : 256u)) ? ld_global(D.grid + b) + 0.0f : 0.0f;
        ov[k] = (OVP && b < no && b < kDec8Ident) ? ld_global(D.grid + nn + b) + 0.0f : 0.0f;
    }
}

// table slot of element code c whose partner's code is cp
template <bool OVP>
__device__ __forceinline__ uint32_t dec8_slot(uint32_t c, uint32_t cp)
{
    return OVP ? c + (cp == kDec8Ident ? 256u : 0u) : c;
}

// One 16-byte output vector from its codes (16-bit types: two words; fp32: one) through the table of finished outputs.
template <typename T, bool OVP>
__device__ __forceinline__ uint4 dec8_vec_tab(uint32_t w0, uint32_t w1, const typename Dec8Out<T>::Ent *tab)
{
    uint32_t c[8];
#pragma unroll
    for (int e = 0; e < 4; e++) { c[e] = (w0 >> (8 * e)) & 0xffu; c[4 + e] = (w1 >> (8 * e)) & 0xffu; }
    if constexpr (sizeof(typename Dec8Out<T>::Ent) == 4) {
        return make_uint4(tab[dec8_slot<OVP>(c[0], c[1])], tab[dec8_slot<OVP>(c[1], c[0])],
                          tab[dec8_slot<OVP>(c[2], c[3])], tab[dec8_slot<OVP>(c[3], c[2])]);
    } else {
        uint32_t o[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const uint32_t lo = tab[dec8_slot<OVP>(c[2 * p], c[2 * p + 1])], hi = tab[dec8_slot<OVP>(c[2 * p + 1], c[2 * p])];
            o[p] = lo | (hi << 16);
        }
        return make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// One task of a row job: u x 64 vectors of one row.
template <typename T, bool OVP, int U>
__device__ __forceinline__ void dec8_row_task(const DecDesc &D, uint32_t task, uint32_t *lds, uint32_t lane)
{
    constexpr int EPL = IO<T>::EPL;
    typedef typename Dec8Out<T>::Ent Ent;
    Ent *tab = reinterpret_cast<Ent *>(lds);
    uint32_t row = task, t = 0;
    if (D.tpr != 1u) { row = task / D.tpr; t = task - row * D.tpr; }
    const uint32_t vpr = D.vpr, v0 = t * (64u * U) + lane;
    const size_t base = (size_t)row * vpr;
    // the code words of this lane's vectors first: they are in flight while the table is built
    uint32_t w0[U], w1[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t v = base + min(v0 + 64u * u, vpr - 1u);
        const ANTQ_GLOBAL uint32_t *p = ((const ANTQ_GLOBAL uint32_t *)(D.codes)) + v * (EPL / 4);
        w0[u] = __builtin_nontemporal_load(p);
        w1[u] = (EPL == 8) ? __builtin_nontemporal_load(p + 1) : 0u;
    }
    const float a = ld_global(D.alpha + (D.per_row ? row : 0u));
    float nv[4], ov[4];
    dec8_book<OVP>(D, lane, nv, ov);
    const float s = a / D.gmax;                       // AQ:536 scale = alpha / max(grid)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t b = lane + 64u * k;
        tab[b] = Dec8Out<T>::make(nv[k] * s);
        if (OVP) tab[256u + b] = Dec8Out<T>::make(ov[k] * s);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint4 *out = static_cast<uint4 *>(D.out) + base;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t v = v0 + 64u * u;
        const uint4 o = dec8_vec_tab<T, OVP>(w0[u], w1[u], tab);
        if (v < vpr) st_stream(out + v, o);
    }
}

// Short rows and unaligned jobs: 4 x 64 units of the flat tensor, the scale per lane, the unscaled codebook in LDS.
// QUAD: a unit is 4 elements with byte loads and element stores; otherwise one 16-byte output vector.
template <typename T, bool OVP, bool QUAD>
__device__ __forceinline__ void dec8_lane_task(const DecDesc &D, uint32_t task, uint32_t *lds, uint32_t lane)
{
    constexpr int EPL = QUAD ? 4 : IO<T>::EPL;       // elements per unit
    constexpr int U = 4;
    static_assert(kDec8QuadU == 4 && kDec8LaneU == 4, "task size of the per-lane kinds");
    float *tab = reinterpret_cast<float *>(lds);
    const uint64_t n_units = D.n_units, first = (uint64_t)task * (64u * U) + lane;
    const uint32_t upr = D.vpr;
    uint32_t w0[U], w1[U];
    float a[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t t = first + 64u * u;
        w0[u] = 0u; w1[u] = 0u;
        a[u] = 1.0f;
        if (t < n_units) {
            if (QUAD) {
                const ANTQ_GLOBAL uint8_t *c = ((const ANTQ_GLOBAL uint8_t *)(D.codes)) + t * 4u;
                w0[u] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
            } else {
                const ANTQ_GLOBAL uint32_t *p = ((const ANTQ_GLOBAL uint32_t *)(D.codes)) + t * (EPL / 4);
                w0[u] = p[0];
                if (EPL == 8) w1[u] = p[1];
            }
            // (a unit lies inside one row: row_len % 4 == 0, and a vector job's rows are whole vectors)
            a[u] = ld_global(D.alpha + (D.per_row ? (n_units <= 0xffffffffull ? (uint64_t)((uint32_t)t / upr) : t / upr) : 0u));
        }
    }
    float nv[4], ov[4];
    dec8_book<OVP>(D, lane, nv, ov);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        tab[lane + 64u * k] = nv[k];
        if (OVP) tab[256u + lane + 64u * k] = ov[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t t = first + 64u * u;
        if (t >= n_units) continue;
        const float s = a[u] / D.gmax;
        float of[EPL];
#pragma unroll
        for (int p = 0; p < EPL / 2; p++) {
            const uint32_t w = (p < 2) ? w0[u] : w1[u];
            const uint32_t c0 = (w >> (16 * (p & 1))) & 0xffu, c1 = (w >> (16 * (p & 1) + 8)) & 0xffu;
            of[2 * p] = tab[dec8_slot<OVP>(c0, c1)] * s;
            of[2 * p + 1] = tab[dec8_slot<OVP>(c1, c0)] * s;
        }
        if constexpr (QUAD) {
#pragma unroll
            for (int e = 0; e < EPL; e++) IO<T>::store1(D.out, t * EPL + e, of[e]);
        } else st_stream(static_cast<uint4 *>(D.out) + t, IO<T>::pack(of));
    }
}

template <typename T, bool OVP>
__device__ __forceinline__ void dec8_task(const DecDesc &D, uint32_t task, uint32_t *lds, uint32_t lane)
{
    if (D.kind == kDec8Row) {
        if (D.u == 4u) dec8_row_task<T, OVP, 4>(D, task, lds, lane);
        else if (D.u == 3u) dec8_row_task<T, OVP, 3>(D, task, lds, lane);
        else dec8_row_task<T, OVP, 2>(D, task, lds, lane);
    } else if (D.kind == kDec8Lane) dec8_lane_task<T, OVP, false>(D, task, lds, lane);
    else dec8_lane_task<T, OVP, true>(D, task, lds, lane);
}

template <typename T, bool OVP>
__global__ void __launch_bounds__(64)
k_decode8_batch(const DecDesc *__restrict__ descs, const uint32_t *__restrict__ block_map)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[OVP ? 512 : 256];
    uint32_t blk = blockIdx.x;
    const uint32_t g8 = blk >> 3;
    // (the decision belongs to the group of 8 workgroups: the job of its first task, antq_k_batch.h)
    if ((g8 << 3) + 8u <= gridDim.x && descs[block_map[(g8 << 3) >> 2]].rot) blk = (g8 << 3) + ((blk + g8) & 7u);
    const uint32_t b4 = blk >> 2, sub = blk & 3u;
    const DecDesc &D = descs[block_map[b4]];
    const uint32_t task = __builtin_amdgcn_readfirstlane((b4 - D.first_block) * 4u + sub);
    if (task >= D.total_tasks) return;
    dec8_task<T, OVP>(D, task, lds, threadIdx.x);
}

// one tensor: the descriptor arrives by value (in SGPRs), workgroup = task
template <typename T, bool OVP>
__global__ void __launch_bounds__(64)
k_decode8(const DecDesc D)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[OVP ? 512 : 256];
    const uint32_t task = __builtin_amdgcn_readfirstlane(blockIdx.x);
    if (task >= D.total_tasks) return;
    dec8_task<T, OVP>(D, task, lds, threadIdx.x);
}

}  // namespace antq

#endif  // ANTQ_K_DECBATCH8_H
