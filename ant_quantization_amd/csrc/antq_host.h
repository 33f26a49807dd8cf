// antq_host.h -- host-side helpers shared by libantq's translation units (launchers of antq_fq.hip, antq_batch.hip,
// antq_search.hip, antq_kernels.hip): the development knobs and the plan-blob accessors.  gfx950 only.
#ifndef ANTQ_HOST_H
#define ANTQ_HOST_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/antq.h"
#include "antq_internal.h"
#include "antq_device.h"
#include "antq_k_approx.h"

namespace antq {

// tuning knobs (dev / bench only; see antq_debug_set and the description of every key in include/antq.h).  THREAD-LOCAL:
// they change the dispatch of the calling thread's later calls only, so a probe that forgets to reset them cannot change
// which kernel another thread's calls run, and the library keeps no process-global mutable state.
// ONE list -- X(key of antq_debug_set, name, default) -- makes the declarations below, the definitions and the setter
// (antq_kernels.hip).  A launcher reads knob `name` as g_knob_name.
#define ANTQ_KNOBS(X)                                                                                                      \
    X(0, u, 0)             /* force U of the uniform kernel (0 = heuristic) */                                             \
    X(1, encwg, 2048)      /* persistent workgroups of the 4-bit encoder (256 CUs x 8); a value <= 0 means 2048 */         \
    X(2, x, 1)             /* 0 disables the x-domain row kernel (A/B measurements) */                                     \
    X(3, nearest_fast, 1)  /* 0: antq_nearest always runs the literal scan */                                              \
    X(4, a, 1)             /* 0 disables the approximate-quotient element path (quant_vec_a): exact division */            \
    X(5, lane_rows, 1)     /* 0: rows of a power of two of vectors through the per-row table kernels (A/B) */              \
    X(6, waves, 0)         /* wavefronts per workgroup of the streaming kernels: 0 = the measured default, 1 / 2 / 4 */    \
    X(7, lane_u, 0)        /* vectors per lane of the one-launch-per-tensor lane kernel: 0 = default (A/B) */              \
    X(8, rot, 0)           /* 1: rotate the workgroup -> task map of the batched row kernel per group of 8 (XCD balance) */ \
    X(9, h, 1)             /* 0 disables the 16-bit-domain row kernels (antq_k_hrow.h; A/B measurements) */                \
    X(10, hlds, -1)        /* dynamic LDS of those kernels' workgroups (occupancy, A/B): -1 = kHRowLdsPad */               \
    X(11, dlds, -1)        /* extra dynamic LDS bytes of the d-domain batched kernels' workgroups (occupancy A/B) */       \
    X(12, schunks, 0)      /* clip search: candidate-list chunks (blockIdx.y) forced to this many (A/B; 0 = cost model) */ \
    X(13, exp, 0)          /* experiment switch of the kernel under development (A/B; 0 = off) */                          \
    X(14, hist, 1)         /* clip search of 16-bit per-tensor quantisers on the histogram: 0 off, 1 when it pays, 2 always */ \
    X(15, hist_xmax, 1)    /* antq_calibrate: abs-max of a histogram-searched tensor from the counting pass (1) or its own pass (0) */ \
    X(16, rows_stream, 1)  /* 0: row abs-max of 128..1024-vector rows through the round-5 kernel (A/B) */                   \
    X(17, tk_group, 0)     /* workgroups per ticket group of the one-launch reductions (antq_k_reduce.h; 0 = default, clamped) */ \
    X(18, tk_blocks, 0)    /* workgroups of the one-launch reductions (0 = default, clamped) */                            \
    X(19, sweep, 1)        /* per-row clip searches through the threshold sweep (antq_k_sweep.h): 0 = the direct kernels, 2 = every eligible launch */ \
    X(20, sort, 1)         /* clip searches from the sorted row (antq_k_sortsearch.h): 0 off, 1 the default rule, 2 every eligible launch */ \
    X(21, sort_short, 1)   /* 0: rows of <= 1024 elements through the 4096-key sorted search (A/B) */                       \
    X(22, mm_tile, 0)      /* antq_linear4_mm / antq_linear8_mm: tiles of 16 output rows per workgroup forced to 1 / 2 / 4 (A/B; 0 = the rule) */ \
    X(23, gemm_tile, 0)    /* antq_linear4_gemm / antq_linear8_gemm: wavefronts (tiles of 64 rows of x) per workgroup forced to 2 / 4 (A/B; 0 = the rule) */
#define ANTQ_KNOB_DECLARE(key, name, dflt) extern thread_local int g_knob_##name;
ANTQ_KNOBS(ANTQ_KNOB_DECLARE)
#undef ANTQ_KNOB_DECLARE

static inline bool plan_args_from_host(const void *plan_host, PlanArgs &pa)
{
    const PlanHeader *h = static_cast<const PlanHeader *>(plan_host);
    if (h->magic != kPlanMagic || h->version != kPlanVersion) return false;
    if (h->m < 1 || h->m > ANTQ_MAX_GRID || h->m_pad != ((h->m + 3) & ~3u)) return false;
    pa.kind = h->kind;
    pa.m = h->m;
    pa.m_pad = h->m_pad;
    pa.shift = h->shift;
    pa.kmin = h->kmin;
    pa.kmax = h->kmax;
    pa.keymask = h->keymask;
    pa.nbneg = h->nbneg;
    pa.fastlim = h->fastlim;
    pa.n_entries = (h->kind == kPlanLut) ? h->n_entries : 0;
    pa.tab_units = pa.n_entries + (pa.m_pad >> 2);
    pa.linear = h->linear;
    pa.lin_scale = h->lin_scale;
    pa.lin_bias = h->lin_bias;
    pa.adom = (h->kind == kPlanLut && g_knob_a != 0) ? h->adom : 0u;
    pa.xlim = h->xlim;
    pa.atab_slots = h->atab_slots;
    return true;
}

static inline const uint4 *plan_tab_ptr(const void *plan_dev)
{
    return reinterpret_cast<const uint4 *>(static_cast<const char *>(plan_dev) + sizeof(PlanHeader));
}

// dynamic LDS of a kernel that stages the plan's table (stage_plan) or, for plans with adom, its converted image (stage_atab)
static inline size_t lds_table(const PlanArgs &pa, bool idx)
{
    const size_t plain = (size_t)pa.tab_units * 16;
    return pa.adom ? std::max(plain, (size_t)atab_units(pa.atab_slots, pa.m_pad, idx) * 16) : plain;
}

}  // namespace antq

#endif  // ANTQ_HOST_H
