// antq_k_outlier.h -- ANT's `outlier` baseline mode (AQ:417-465): the fused forward and the exact order statistics of |x|
// Part of libantq's single device translation unit (antq_kernels.hip includes it); gfx950 only.
#ifndef ANTQ_K_OUTLIER_H
#define ANTQ_K_OUTLIER_H

#include "antq_device.h"

// (the kernels of this header keep every fp32 operation a scalar VALU instruction: one rounding per written operation)
#if defined(__HIP_DEVICE_COMPILE__)
#define ANTQ_OUTLIER_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define ANTQ_OUTLIER_KERNEL
#endif

namespace antq {

// ------------------------------------------------------------------------------------
// Fused forward (antq_fakequant_outlier).  Per element, every operation rounded on its own:
//     body = p4 > 0 ? nearest(x / s) * s : x                        s = p4 / gmax
//     out  = TAIL && |x| > p4 ? (fine - body) + body : body         fine = (rint((|x| - p4) / step) * step + p4) * sign(x)
// p4 / p16 arrive as device floats and are read as wave-uniform scalars ahead of the data loads; s, 1 / s and step are
// formed once per wavefront.  The body decision is the plan's d-domain table (lut_lookup) after the exact five-operation
// division of div_fast -- the same pair quant_vec uses -- with the literal division + scan for lanes outside the table's
// domain, scan plans and scales outside div_fast's range.  The tail's two true divisions sit behind a wave-level branch
// per element slot: a slot in which no lane of the wavefront holds an outlier skips them.
// ------------------------------------------------------------------------------------
constexpr int kOutlierU = 4;        // 16-byte vectors per lane: a wavefront owns 64 * 4 * kOutlierU contiguous elements

struct OutlierScalars {
    float p4, step;
    Scale sc;
    bool body;          // p4 > 0: the int body is quantised (false also for a NaN p4: the body is x itself)
    bool trusted;       // the plan describes the device grid (outlier_check_grid): its table may decide
};

__device__ __forceinline__ OutlierScalars outlier_scalars(float p4, float p16, float gmax, float levelf, bool trusted)
{
    OutlierScalars k;
    k.p4 = p4;
    k.trusted = trusted;
    k.body = p4 > 0.0f;
    k.sc = make_scale(p4, gmax);
    k.step = (p16 - p4) / levelf;
    return k;
}

template <bool TAIL, int E>
__device__ __forceinline__ void outlier_vec(const PlanArgs &pa, const PlanLds &L, const OutlierScalars &k,
                                            const float (&x)[E], float (&o)[E])
{
    float body[E];
    if (k.body) {
        float d[E], q[E];
        int j[E];
        bool fast = (pa.kind == kPlanLut) && k.sc.ok && k.trusted;
        if (fast) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                d[e] = div_fast(x[e], k.sc.s, k.sc.rs);
                fast = fast && (fabsf(d[e]) < pa.fastlim);      // false for NaN / Inf / huge
            }
        }
        if (fast) {
            lut_lookup<E, false>(pa, L, d, q, j);
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) {
                int jj;
                q[e] = scan_lds(x[e] / k.sc.s, L.grid, (int)pa.m, jj);
            }
        }
#pragma unroll
        for (int e = 0; e < E; e++) body[e] = q[e] * k.sc.s;
    } else {
#pragma unroll
        for (int e = 0; e < E; e++) body[e] = x[e];
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        o[e] = body[e];
        if (TAIL) {
            const float a = fabsf(x[e]);
            const bool t = a > k.p4;
            if (__builtin_amdgcn_ballot_w64(t) != 0) {            // wave-uniform: some lane holds an outlier in this slot
                const float mag = rintf((a - k.p4) / k.step) * k.step + k.p4;
                const float sg = (x[e] > 0.0f ? 1.0f : 0.0f) - (x[e] < 0.0f ? 1.0f : 0.0f);
                const float fine = mag * sg;
                const float r = (fine - body[e]) + body[e];
                if (t) o[e] = r;
            }
        }
    }
}

// The plan as a hint (as antq_nearest_hinted): gcheck, when given, is the DEVICE array the quantiser's grid lives in, and
// the plan only what the host believes it holds.  Every workgroup compares the m values with the plan's own copy, bit for
// bit (g0 = gcheck[threadIdx.x], fetched ahead of the data loads); on any difference it scans the device values
// literally and divides by THEIR maximum (torch.max: a NaN wins) -- a stale plan costs time, never a wrong result.
__device__ __forceinline__ bool outlier_check_grid(const PlanArgs &pa, const PlanLds &L, const float *__restrict__ gcheck,
                                                   float g0, float &gmax)
{
    if (!gcheck) return true;
    int diff = 0;
    if (threadIdx.x < pa.m) diff = f2u(g0) != f2u(L.grid[threadIdx.x]);
    for (uint32_t i = threadIdx.x + 256u; i < pa.m; i += 256u) diff |= f2u(gcheck[i]) != f2u(L.grid[i]);
    if (!__syncthreads_or(diff)) return true;
    float *lg = const_cast<float *>(L.grid);
    for (uint32_t i = threadIdx.x; i < pa.m; i += 256u) lg[i] = gcheck[i];
    __syncthreads();
    float mx = lg[0];
    for (uint32_t i = 1; i < pa.m; i++) {
        const float g = lg[i];
        mx = (g > mx || g != g) ? g : mx;
    }
    gmax = mx;
    return false;
}

// Whole 16-byte vectors of an aligned tensor; the n_tail < 4 elements behind the last vector go to the first lanes of
// the last workgroup.  x and out may be the same buffer: a lane reads its own elements before it writes them, and the
// lanes past the end (which re-read the last vector so that no branch separates the loads) store nothing.
template <bool TAIL>
ANTQ_OUTLIER_KERNEL __global__ void __launch_bounds__(256)
k_fq_outlier(const uint4 *x, uint4 *out, size_t n_vec, uint32_t n_tail, const float *__restrict__ p4_dev,
             const float *__restrict__ p16_dev, float gmax, float levelf, PlanArgs pa, const uint4 *__restrict__ plan_tab,
             const float *__restrict__ gcheck)
{
    constexpr int U = kOutlierU;
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4 tab0 = make_uint4(0, 0, 0, 0);
    if (threadIdx.x < pa.tab_units) tab0 = plan_tab[threadIdx.x];
    float g0 = 0.0f;
    if (gcheck && threadIdx.x < pa.m) g0 = gcheck[threadIdx.x];
    // the scalars FIRST: loads return in order, so the scale is there with the data loads still in flight behind it
    const float p4 = ld_global(p4_dev), p16 = ld_global(p16_dev);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const size_t first = ((size_t)blockIdx.x * 4u + wv) * (64u * U) + lane;
    const bool tail_lane = blockIdx.x == gridDim.x - 1u && threadIdx.x < n_tail;
    const float *xt = reinterpret_cast<const float *>(x + n_vec);
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = ld_stream(x + min(first + 64u * u, n_vec - 1u));
    float t_in[1] = {0.0f};
    if (tail_lane) t_in[0] = ld_global(xt + threadIdx.x);
    const PlanLds L = stage_plan(pa, plan_tab, smem, tab0);
    __syncthreads();
    const bool trusted = outlier_check_grid(pa, L, gcheck, g0, gmax);
    const OutlierScalars k = outlier_scalars(p4, p16, gmax, levelf, trusted);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t vi = first + 64u * u;
        if (vi >= n_vec) continue;
        float xe[4], oe[4];
        IO<float>::unpack(v[u], xe);
        outlier_vec<TAIL, 4>(pa, L, k, xe, oe);
        st_stream(out + vi, IO<float>::pack(oe));
    }
    if (tail_lane) {
        float t_out[1];
        outlier_vec<TAIL, 1>(pa, L, k, t_in, t_out);
        st_global(reinterpret_cast<float *>(out + n_vec) + threadIdx.x, t_out[0]);
    }
}

// Element-granular form for tensors that are not 16-byte aligned or shorter than one vector: the same element code on
// four elements per lane, 256 apart (coalesced dword accesses).
template <bool TAIL>
ANTQ_OUTLIER_KERNEL __global__ void __launch_bounds__(256)
k_fq_outlier_scalar(const float *x, float *out, size_t n, const float *__restrict__ p4_dev,
                    const float *__restrict__ p16_dev, float gmax, float levelf, PlanArgs pa,
                    const uint4 *__restrict__ plan_tab, const float *__restrict__ gcheck)
{
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4 tab0 = make_uint4(0, 0, 0, 0);
    if (threadIdx.x < pa.tab_units) tab0 = plan_tab[threadIdx.x];
    float g0 = 0.0f;
    if (gcheck && threadIdx.x < pa.m) g0 = gcheck[threadIdx.x];
    const float p4 = ld_global(p4_dev), p16 = ld_global(p16_dev);
    const size_t first = (size_t)blockIdx.x * 1024u + threadIdx.x;
    float xe[4], oe[4];
#pragma unroll
    for (int e = 0; e < 4; e++) xe[e] = ld_global(x + min(first + 256u * e, n - 1u));
    const PlanLds L = stage_plan(pa, plan_tab, smem, tab0);
    __syncthreads();
    const bool trusted = outlier_check_grid(pa, L, gcheck, g0, gmax);
    const OutlierScalars k = outlier_scalars(p4, p16, gmax, levelf, trusted);
    outlier_vec<TAIL, 4>(pa, L, k, xe, oe);
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (first + 256u * e < n) st_global(out + first + 256u * e, oe[e]);
}

// ------------------------------------------------------------------------------------
// Exact order statistics of |x| (antq_abs_order_stats): a radix select over the 31-bit pattern of |x| -- fp32 magnitudes
// order like their bits, NaNs above Inf -- with digits of 11 / 10 / 10 bits, one pass over x per digit.
//   k_os_count<P> : every workgroup counts digit P of the elements whose higher digits equal the prefix chosen so far
//                   into an 8 KiB LDS histogram and flushes its non-empty bins with integer atomics (order-independent:
//                   the same bits on every run).  Ranks k and k + 1 may have chosen different prefixes: a pass counts
//                   under both (two 1024-bin histograms; one when the prefixes agree).  Pass 0 also keeps the largest
//                   non-NaN pattern and the number of NaNs.
//   k_os_scan<P>  : one workgroup walks the histogram, writes for each rank the bin that holds it and the rank that is
//                   left inside that bin, and clears the histogram for the next pass; the last one writes the results.
// Workspace (uint32 words): [0, 2048) histogram(s); [2048, 2056) state: prefix of rank k, of rank k + 1, the two
// remaining ranks, max pattern, NaN count.
// ------------------------------------------------------------------------------------
constexpr uint32_t kOsHistWords = 2048;
constexpr uint32_t kOsState = kOsHistWords;
constexpr uint32_t kOsWords = kOsHistWords + 8;
constexpr uint32_t kOsMaxBlocks = 1024;

static __global__ void __launch_bounds__(256) k_os_init(uint32_t *__restrict__ ws, uint32_t k_lo, uint32_t k_hi)
{
    for (uint32_t i = threadIdx.x; i < kOsWords; i += 256u) ws[i] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) { ws[kOsState + 2] = k_lo; ws[kOsState + 3] = k_hi; }
}

// x: the n floats; head of them (< 4) lie before the first 16-byte boundary, n_vec whole vectors follow, the rest (< 4) trail
template <int P>
__global__ void __launch_bounds__(256)
k_os_count(const float *__restrict__ x, size_t n, uint32_t head, size_t n_vec, uint32_t *__restrict__ ws)
{
    __shared__ uint32_t h[kOsHistWords];
    __shared__ uint32_t s_max, s_nan;
    uint32_t pre_lo = 0, pre_hi = 0;
    if (P > 0) { pre_lo = ws[kOsState]; pre_hi = ws[kOsState + 1]; }
    for (uint32_t i = threadIdx.x; i < kOsHistWords; i += 256u) h[i] = 0u;
    if (threadIdx.x == 0) { s_max = 0u; s_nan = 0u; }
    __syncthreads();
    const bool two = pre_lo != pre_hi;
    uint32_t vmax = 0, nans = 0;
    auto count = [&](uint32_t bits) {
        const uint32_t u = bits & 0x7fffffffu;
        if (P == 0) {
            atomicAdd(&h[u >> 20], 1u);
            if (u > 0x7f800000u) nans++;
            else vmax = max(vmax, u);
        } else {
            const uint32_t top = P == 1 ? u >> 20 : u >> 10, dg = (P == 1 ? u >> 10 : u) & 1023u;
            if (top == pre_lo) atomicAdd(&h[dg], 1u);
            if (two && top == pre_hi) atomicAdd(&h[1024u + dg], 1u);
        }
    };
    const uint4 *xv = reinterpret_cast<const uint4 *>(x + head);
    for (size_t base = (size_t)blockIdx.x * 1024u + threadIdx.x; base < n_vec; base += (size_t)gridDim.x * 1024u) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = ld_global(xv + min(base + 256u * u, n_vec - 1u));   // (x is read three times: cached)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (base + 256u * u >= n_vec) continue;
            count(v[u].x); count(v[u].y); count(v[u].z); count(v[u].w);
        }
    }
    if (blockIdx.x == 0) {
        const size_t body_end = (size_t)head + n_vec * 4u;
        if (threadIdx.x < head) count(f2u(x[threadIdx.x]));
        else if (body_end + (threadIdx.x - head) < n) count(f2u(x[body_end + (threadIdx.x - head)]));
    }
    if (P == 0) {
        if (vmax) atomicMax(&s_max, vmax);
        if (nans) atomicAdd(&s_nan, nans);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kOsHistWords; i += 256u) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&ws[i], c);
    }
    if (P == 0 && threadIdx.x == 0) {
        if (s_max) atomicMax(&ws[kOsState + 4], s_max);
        if (s_nan) atomicAdd(&ws[kOsState + 5], s_nan);
    }
}

template <int P>
__global__ void __launch_bounds__(256) k_os_scan(uint32_t *__restrict__ ws, float *__restrict__ stats)
{
    constexpr uint32_t BINS = P == 0 ? 2048u : 1024u, PER = BINS / 256u, BITS = P == 0 ? 11u : 10u;
    __shared__ uint32_t part[256];
    __shared__ uint32_t s_pre[2], s_rem[2];
    const uint32_t t = threadIdx.x;
    const uint32_t pre[2] = {ws[kOsState], ws[kOsState + 1]}, rank[2] = {ws[kOsState + 2], ws[kOsState + 3]};
    const bool two = P > 0 && pre[0] != pre[1];
#pragma unroll 1
    for (int r = 0; r < 2; r++) {
        const uint32_t *hist = ws + ((r == 1 && two) ? 1024u : 0u);
        uint32_t c[PER], s = 0;
#pragma unroll
        for (uint32_t i = 0; i < PER; i++) { c[i] = hist[t * PER + i]; s += c[i]; }
        part[t] = s;
        __syncthreads();
        for (uint32_t off = 1; off < 256u; off <<= 1) {       // inclusive scan of the 256 partial sums
            const uint32_t add = t >= off ? part[t - off] : 0u;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        uint32_t cum = part[t] - s;                            // elements in the bins before this thread's
        if (rank[r] >= cum && rank[r] - cum < s) {             // exactly one thread: the rank lies in one of its bins
#pragma unroll
            for (uint32_t i = 0; i < PER; i++) {
                if (rank[r] >= cum && rank[r] - cum < c[i]) {
                    s_pre[r] = (pre[r] << BITS) | (t * PER + i);
                    s_rem[r] = rank[r] - cum;
                }
                cum += c[i];
            }
        }
        __syncthreads();
    }
    for (uint32_t i = t; i < kOsHistWords; i += 256u) ws[i] = 0u;
    if (t < 2) { ws[kOsState + t] = s_pre[t]; ws[kOsState + 2 + t] = s_rem[t]; }
    if (P == 2 && t == 0) {
        stats[0] = u2f(s_pre[0]);
        stats[1] = u2f(s_pre[1]);
        stats[2] = u2f(ws[kOsState + 4]);
        stats[3] = (float)ws[kOsState + 5];
    }
}

}  // namespace antq

#endif  // ANTQ_K_OUTLIER_H
