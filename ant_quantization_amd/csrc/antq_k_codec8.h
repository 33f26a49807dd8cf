// antq_k_codec8.h -- byte-code encoder (antq_encode8): one code per element, books of up to 256 values (pair rule: 255 + 255)
// Part of libantq's single device translation unit (antq_kernels.hip includes it); gfx950 only.
//
// The element encoder of antq_k_codec.h (k_encode4) with a byte for a nibble: the same decision -- the plan's a-table with
// the two values of every entry replaced by their codes, or the d-domain table / the literal scan for plans without one --
// the same pair rule on the outlier bits, the identifier 255 instead of 15, and a unit of 8 or 4 elements (row_len % 8 ==
// 4: two pairs, still inside one row) that becomes two code words or one.  The 4-bit templates are untouched: these stand
// beside them.  No row-table and no 16-bit-domain form: byte codes are encoded once per model.
#ifndef ANTQ_K_CODEC8_H
#define ANTQ_K_CODEC8_H

#include "antq_k_codec.h"
#include "antq_decbatch8.h"

namespace antq {

template <bool OVP>
__device__ __forceinline__ uint32_t code8_of(uint32_t j, float v, int n_normal)
{
    uint32_t c = (OVP && (int)j >= n_normal) ? j - (uint32_t)n_normal : j;
    c &= 255u;
    if (OVP && fabsf(v) > 32.0f) c |= kOutlierBit;                // OQ:314
    return c;
}
template <bool OVP>
__device__ __forceinline__ void atab_to_codes8(const PlanArgs &pa, uint4 *smem, const ATab &A, int n_normal)
{
    for (uint32_t i = threadIdx.x; i < pa.atab_slots; i += blockDim.x) {
        uint4 e = smem[i];
        const uint32_t w = A.idx[i];
        e.z = code8_of<OVP>(w & kIdxMask, u2f(e.z), n_normal);
        e.w = code8_of<OVP>((w >> 16) & kIdxMask, u2f(e.w), n_normal);
        smem[i] = e;
    }
}
// E codes (E / 2 pairs) -> E / 4 words of bytes; OVP: the pair rule on the outlier bits first (OQ:313-320)
template <bool OVP, int E>
__device__ __forceinline__ void pack_codes8(uint32_t (&c)[E], uint32_t (&w)[E / 4])
{
#pragma unroll
    for (int p = 0; p < E / 2; p++) {
        uint32_t c0 = c[2 * p], c1 = c[2 * p + 1];
        if (OVP) {
            const bool me = c0 >= kOutlierBit, mo = c1 >= kOutlierBit;
            const bool ve = mo && !me;
            c0 = ve ? kDec8Ident : c0;                           // the identifier marks the victim
            c1 = me ? kDec8Ident : c1;
        }
        c[2 * p] = c0 & 255u;
        c[2 * p + 1] = c1 & 255u;
    }
#pragma unroll
    for (int q = 0; q < E / 4; q++) w[q] = c[4 * q] | (c[4 * q + 1] << 8) | (c[4 * q + 2] << 16) | (c[4 * q + 3] << 24);
}
// E consecutive elements of one row (the first at an index that is a multiple of E) -> E bytes
template <bool OVP, int E>
__device__ __forceinline__ void encode8_unit_a(const PlanArgs &pa, const uint4 *etab, const float *grid, const ScaleA &sc,
                                               const float (&x)[E], int n_normal, int zero_code, uint32_t (&w)[E / 4])
{
    float dt[E];
    uint32_t c[E];
    const float flim = pa.fastlim * 0.99999f;
#pragma unroll
    for (int e = 0; e < E; e++) dt[e] = x[e] * sc.rs;
    bool nan;
    const float dmax = absmax_nan<E>(dt, nan);
    if (sc.ok && !nan && dmax < flim) {                 // false for NaN / Inf / beyond the table's domain
        uint32_t slot[E];
        a_slots<E>(pa, dt, slot);
        const AEnt *tab0 = reinterpret_cast<const AEnt *>(pa.linear ? etab : etab - 2u * pa.kmin);
        AEnt ents[E];
#pragma unroll
        for (int e = 0; e < E; e++) ents[e] = tab0[slot[e]];      // all reads in flight before the first use
#pragma unroll
        for (int e = 0; e < E; e++) {
            AEnt ent = ents[e];
            ent.pin();
            c[e] = (__builtin_fma(-ent.Mp(), sc.sd, (double)x[e]) >= 0.0) ? ent.hi() : ent.lo();
        }
    } else {
        // the literal sequence (true division, scan) for this lane's unit
#pragma unroll
        for (int e = 0; e < E; e++) {
            int jj;
            const float q = scan_lds(x[e] / sc.s, grid, (int)pa.m, jj);
            c[e] = jj == ANTQ_IDX_NONE ? (uint32_t)zero_code : code8_of<OVP>((uint32_t)jj, q, n_normal);
        }
    }
    pack_codes8<OVP, E>(c, w);
}

// E elements <- one (16-bit, E = 8; fp32, E = 4), two (fp32, E = 8) or half a (16-bit, E = 4) 16-byte vector
template <typename T, int E>
__device__ __forceinline__ void unit8_load(const void *x, size_t o, float (&f)[E])
{
    if constexpr (E == 8) Oct<T>::load(x, o, f);
    else if constexpr (IO<T>::EPL == 4) IO<T>::unpack(ld_stream(static_cast<const uint4 *>(x) + o), f);
    else {
        typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
        const u32x2_t h = __builtin_nontemporal_load(((const ANTQ_GLOBAL u32x2_t *)(x)) + o);
        float f8[8];
        IO<T>::unpack(make_uint4(h.x, h.y, 0u, 0u), f8);
#pragma unroll
        for (int e = 0; e < 4; e++) f[e] = f8[e];
    }
}

// Persistent workgroups (the plan's table is staged once), each looping over tasks of 256 * U units of E elements.
// words: codes is 4-byte aligned -> word stores, otherwise byte stores.
template <typename T, bool OVP, bool VEC, int E>
__global__ void __launch_bounds__(256)
k_encode8(const void *__restrict__ x, uint8_t *__restrict__ codes, size_t n_units, size_t row_len, size_t n_tasks,
          const float *__restrict__ alpha, int per_row, float gmax, int n_normal, int zero_code, int words,
          PlanArgs pa, const uint4 *__restrict__ plan_tab)
{
    constexpr int U = VEC ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4 tab0 = make_uint4(0, 0, 0, 0);
    if (pa.adom) tab0 = atab_prefetch<true>(pa, plan_tab);         // exact decision on x (antq_k_approx.h), with indices
    else if (threadIdx.x < pa.tab_units) tab0 = plan_tab[threadIdx.x];
    PlanLds L;
    ATab A;
    if (pa.adom) {
        A = stage_atab<true>(pa, plan_tab, smem, tab0);
        __syncthreads();
        atab_to_codes8<OVP>(pa, smem, A, n_normal);
    } else L = stage_plan(pa, plan_tab, smem, tab0);
    __syncthreads();
    const size_t upr = row_len / E;                    // row_len % E == 0: a unit (E / 2 pairs) lies inside one row -> one scale
    const float a0 = per_row ? 1.0f : alpha[0];
    const double inv_gmax = 1.0 / (double)gmax;
    for (size_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const size_t first = (task * U) * 256u + threadIdx.x;   // unit index: elements [E o, E o + E)
        float xf[U][E], a[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t o = first + (size_t)u * 256u;
            a[u] = a0;
#pragma unroll
            for (int e = 0; e < E; e++) xf[u][e] = 0.0f;
            if (o < n_units) {
                if (per_row) a[u] = alpha[o / upr];
                if constexpr (VEC) unit8_load<T, E>(x, o, xf[u]);
                else {
#pragma unroll
                    for (int e = 0; e < E; e++) xf[u][e] = IO<T>::load1(x, o * E + e);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t o = first + (size_t)u * 256u;
            if (o >= n_units) continue;
            uint32_t w[E / 4];
            if (pa.adom) encode8_unit_a<OVP, E>(pa, A.tab, A.grid, make_scale_a(a[u], gmax, inv_gmax), xf[u], n_normal, zero_code, w);
            else {
                float of[E];
                int j[E];
                const Scale sc = make_scale(a[u], gmax);
                quant_vec<E, OVP, true>(pa, L, sc, xf[u], of, j);
#pragma unroll
                for (int q = 0; q < E / 4; q++) w[q] = 0u;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const int jj = j[e];
                    uint32_t c;
                    if (jj == ANTQ_IDX_VICTIM) c = kDec8Ident;
                    else if (jj == ANTQ_IDX_NONE) c = (uint32_t)zero_code;
                    else if (OVP && jj >= n_normal) c = (uint32_t)(jj - n_normal);
                    else c = (uint32_t)jj;
                    w[e / 4] |= (c & 255u) << (8 * (e % 4));
                }
            }
            if (words) {
#pragma unroll
                for (int q = 0; q < E / 4; q++) reinterpret_cast<uint32_t *>(codes)[o * (E / 4) + q] = w[q];
            } else {
#pragma unroll
                for (int e = 0; e < E; e++) codes[o * E + e] = (uint8_t)(w[e / 4] >> (8 * (e % 4)));
            }
        }
    }
}

template <typename T>
static int launch_encode8(const void *x, uint8_t *codes, size_t rows, size_t row_len, const float *alpha, int per_row, float gmax,
                          const PlanArgs &pa, const void *plan_host, const void *plan_dev, int n_normal, bool ovp, hipStream_t st)
{
    if (row_len % 4 != 0) return ANTQ_ERR_UNSUPPORTED;
    const int m = (int)pa.m;
    if (!dec8_book_ok(m, n_normal, ovp)) return ANTQ_ERR_UNSUPPORTED;
    if (rows > (size_t)-1 / row_len) return ANTQ_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(x) % IO<T>::ESIZE) return ANTQ_ERR_ALIGN;
    const size_t n = rows * row_len;
    const bool oct = row_len % 8 == 0;
    const size_t n_units = n / (oct ? 8 : 4);
    const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0;     // 16-byte vector I/O (a quad of a 16-bit type: 8 bytes)
    const size_t per_block = vec ? 256 * 2 : 256;                  // units per workgroup and task
    const size_t n_tasks = (n_units + per_block - 1) / per_block;
    size_t blocks = n_tasks;
    if (blocks > (size_t)g_knob_encwg) blocks = (size_t)g_knob_encwg;   // persistent workgroups
    if (blocks > 0x7fffffffull) return ANTQ_ERR_UNSUPPORTED;
    const float *grid_host = plan_grid(plan_host);
    int zero_code = 0;
    for (int i = 0; i < (ovp ? n_normal : m); i++) if (grid_host[i] == 0.0f) zero_code = i;
    const int words = reinterpret_cast<uintptr_t>(codes) % 4 == 0 ? 1 : 0;
    const size_t lds = lds_table(pa, true);
    const dim3 gd((unsigned)blocks), bd(256);
#define ANTQ_ENC8(O, V, E_) hipLaunchKernelGGL((k_encode8<T, O, V, E_>), gd, bd, lds, st, x, codes, n_units, row_len, n_tasks, alpha, per_row, \
                                               gmax, n_normal, zero_code, words, pa, plan_tab_ptr(plan_dev))
#define ANTQ_ENC8E(O, V) do { if (oct) ANTQ_ENC8(O, V, 8); else ANTQ_ENC8(O, V, 4); } while (0)
    if (ovp) { if (vec) ANTQ_ENC8E(true, true); else ANTQ_ENC8E(true, false); }
    else     { if (vec) ANTQ_ENC8E(false, true); else ANTQ_ENC8E(false, false); }
#undef ANTQ_ENC8E
#undef ANTQ_ENC8
    return hipGetLastError() == hipSuccess ? ANTQ_OK : ANTQ_ERR_LAUNCH;
}

}  // namespace antq

#endif  // ANTQ_K_CODEC8_H
