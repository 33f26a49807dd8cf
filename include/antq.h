/*
 * antq.h -- C ABI of libantq.so: MI355X (gfx950) fake-quant hot path of ANT / OliVe.
 *
 * This is the drop-in boundary for the reference's ONLY native operator,
 *     quant_cuda.quant(x, grid) -> (z, idx)
 *         ant_quantization/quant/quant.cpp:17-29        (pybind entry)
 *         ant_quantization/quant/quant_kernel.cu:11-62  (kernel + launcher)
 * plus fused entry points that replace the PyTorch op sequences the reference
 * runs around that operator on every forward:
 *     Quantizer._forward            ant_quantization/antquant/quant_modules.py:535-551
 *     Quantizer._forward (OliVe)    olive_quantization/antquant/quant_modules.py:294-330
 *     AsymmetricQuantFunction       ant_quantization/antquant/quant_affine.py:95-115
 *     mse_loss / search_mse         ant_quantization/antquant/quant_modules.py:280-326
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary;
 *   - every *_dev pointer is device (HBM) memory owned by the caller; the library
 *     never allocates, frees or synchronises; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream);
 *   - return 0 on success, a negative ANTQ_ERR_* otherwise; no exceptions;
 *   - re-entrant and thread-safe: no process-global mutable state (the antq_debug_set development knobs are
 *     thread-local: they only steer the calling thread's own later calls);
 *     nothing here allocates or synchronises, so every entry point can be captured into a hipGraph;
 *   - results: grid index bit-exact with the reference scan; dequantised floats
 *     bit-identical to the reference's fp32 op sequence (bf16/f16 outputs are the
 *     fp32 result rounded to nearest-even).
 */
#ifndef ANTQ_H
#define ANTQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): antq_search_sse / antq_alpha_grad take a caller workspace before `stream`, antq_absmax initialises its
 * output, the batch blob changed (plan version 8), ANTQ_FLAG_UNORDERED.  3: antq_calibrate / antq_calibrate_workspace_bytes
 * added (nothing else changed).  4 (round 4): the plan blob grew (version 9: 128-byte header + the threshold list of the
 * 16-bit-domain kernels; ANTQ_PLAN_MAX_BYTES with it), the batch blob changed, antq_plan_eval_host_h and
 * antq_prefetch_kernels added.  5: antq_calibrate_batch / antq_calibrate_batch_workspace_bytes and antq_absmax_into added (nothing else changed).
 * 7 (round 6): antq_absmax_t / antq_alpha_grad_t (whole-tensor reductions in ONE launch through a caller-owned ticket block,
 * ANTQ_REDUCE_WS_BYTES) and antq_calibrate_install added (nothing else changed).
 * Still 7: antq_decode4_batch_capacity / antq_decode4_batch_build / antq_decode4_batch added (the batched packed decoder; nothing
 * that existed changed, so callers built against 7 keep working).  antq_linear4 (the packed 4-bit linear) added likewise,
 * and antq_linear4_mm (its matrix-core form for up to 64 rows), and antq_encode8 / antq_decode8 / antq_decode8_batch_capacity /
 * antq_decode8_batch_build / antq_decode8_batch (the byte-code codec), and antq_linear8 (the linear from byte codes), and
 * antq_linear8_mm (its matrix-core form for up to 64 rows), and antq_linear4_gemm (the tiled 4-bit form for up to 4096 rows),
 * and antq_linear8_gemm (the same from byte codes), and antq_linear4_t (the 4-bit linear for weights stored [K, N]),
 * and antq_linear4_t_mm (its matrix-core form for up to 64 rows).
 * A caller built against another version must not call in: the blobs / argument lists differ. */
#define ANTQ_ABI_VERSION 7

/* element types of x / out */
#define ANTQ_F32  0
#define ANTQ_BF16 1
#define ANTQ_F16  2
#define ANTQ_F64  3   /* antq_nearest only (AT_DISPATCH_FLOATING_TYPES: float, double) */

/* error codes */
#define ANTQ_OK               0
#define ANTQ_ERR_ARG        (-1)   /* null pointer, bad size, bad enum               */
#define ANTQ_ERR_UNSUPPORTED (-2)  /* dtype / grid size not supported by this entry  */
#define ANTQ_ERR_PLAN       (-3)   /* plan blob malformed or too small               */
#define ANTQ_ERR_LAUNCH     (-4)   /* hipLaunchKernel failed (hipGetLastError)       */
#define ANTQ_ERR_ALIGN      (-5)   /* pointer not aligned to the element size        */

/* flags of antq_fakequant* */
#define ANTQ_FLAG_OVP        1u    /* OliVe outlier-victim pair masking (OQ:311-320) */
#define ANTQ_FLAG_DYNAMIC    2u    /* antq_batch_build only: alpha computed in the kernel */
#define ANTQ_FLAG_UNORDERED  4u    /* antq_fakequant only: this launch does not depend on the launches queued before it on
                                    * the stream (its inputs are at rest: calibrated weights), so it may START while they are
                                    * still draining -- the dispatch packet goes out without the barrier bit
                                    * (hipExtAnyOrderLaunch).  Ordinary launches queued after it still wait for it.  Worth
                                    * 2-3 us per 33.5 MB tensor when many weight tensors are quantised one launch each.
                                    * The OUTPUT buffer must be at rest too: not one a stream-ordered allocator has just
                                    * recycled from a kernel that may still be running (torch's caching allocator does that:
                                    * the Python binding refuses the flag without a caller-owned `out`).
                                    * A HINT: honoured by the table / lane kernels that serve 4-bit codebooks (the cases it was
                                    * measured on); the uniform-grid, scalar and literal-scan paths launch ordered whatever
                                    * the flag says.  Not with an index output: ANTQ_ERR_ARG. */

/* values written to the optional int16 index output */
#define ANTQ_IDX_NONE    (-1)      /* no grid entry within 102400 (NaN/Inf/huge)     */
#define ANTQ_IDX_VICTIM  (-2)      /* OliVe victim: value forced to zero             */

#define ANTQ_MAX_GRID     1024     /* entries; the reference's LDS array holds 256   */
#define ANTQ_PLAN_MAX_BYTES (128 + 4 * ANTQ_MAX_GRID + 16 * 3072 + 20 * 1024 + 16 * 64)

int         antq_abi_version(void);
const char *antq_strerror(int code);

/* ---------------------------------------------------------------------------
 * quant_cuda.quant replacement (ant_quantization/quant/quant_kernel.cu:11-62).
 *   z[i] = grid[j*],  j* = last j minimising fl32|fl32(x[i]) - fl32(grid[j])|,
 *   z[i] = 0 when no distance is <= 102400 (NaN / Inf / huge inputs).
 * x, z: n elements of `dtype` (F32, F64, BF16, F16).  grid_dev: m entries of the
 * SAME dtype as x for F32/F64 (the reference casts grid.type_as(x)); float for
 * BF16/F16.  idx_dev (nullable): int16 j* per element (the reference allocates an
 * index tensor but never writes it; see quant_kernel.cu:18,49).
 * ------------------------------------------------------------------------- */
int antq_nearest(const void *x_dev, void *z_dev, int16_t *idx_dev, size_t n,
                 const void *grid_dev, int m, int dtype, void *stream);

/* The same operator for a grid the caller knows on the host (a quantiser's static codebook: build the plan once, see
 * below): one table lookup per element instead of the m-step scan -- same z, same j*.  x, z: n elements of F32 / BF16 /
 * F16, 16-byte aligned, n a multiple of 4 (F32) or 8; anything else: ANTQ_ERR_UNSUPPORTED, use antq_nearest. */
int antq_nearest_plan(const void *x_dev, void *z_dev, int16_t *idx_dev, size_t n,
                      const void *plan_host, const void *plan_dev, int dtype, void *stream);

/* quant_cuda.quant (quant_kernel.cu:11-62) with a plan as a HINT.  Contract = antq_nearest on the device array
 * grid_dev (m floats; x of F32 / BF16 / F16): the plan is only what the host believes grid_dev holds (built from an
 * earlier read-back of the same buffer).  Every workgroup compares the m device values with the plan's own copy of the
 * grid bit for bit; if they differ it runs the literal scan on the device values -- a stale plan costs time, never a
 * wrong result -- and stores 1 to *stale (nullable; device-accessible memory, e.g. a pinned host int the caller polls
 * without synchronising).  m must equal the plan's grid size (ANTQ_ERR_ARG otherwise); size / alignment rules of
 * antq_nearest_plan. */
int antq_nearest_hinted(const void *x_dev, void *z_dev, int16_t *idx_dev, size_t n,
                        const float *grid_dev, int m, const void *plan_host, const void *plan_dev,
                        int *stale, int dtype, void *stream);

/* ---------------------------------------------------------------------------
 * Plan: host-side, exact pre-computation of the decision thresholds of the
 * reference scan for one grid (pure CPU, no HIP calls).  The caller keeps the
 * host blob and uploads a copy to the device; both are passed to the fused
 * entry points.  Returns the number of bytes written (>0) or ANTQ_ERR_*.
 *   grid_host : m floats in the order the reference would pass them to the
 *               kernel (ANT: sorted quant_grid; OliVe: cat(quant_grid, outliers)).
 * antq_plan_kind(): 1 = table plan (fast path), 0 = scan plan (the grid is not
 * representable as a table; the kernels fall back to the literal scan).
 * ------------------------------------------------------------------------- */
int antq_plan_build(const float *grid_host, int m, void *plan_host, size_t plan_capacity);
int antq_plan_kind(const void *plan_host);
int antq_plan_bytes(const void *plan_host);

/* Host model of the device element path for one plan (pure CPU): q[i], idx[i] for the
 * grid-domain inputs d[i].  The kernels implement exactly this function; the CPU test
 * suite uses it to check a plan against the literal scan without a GPU. */
int antq_plan_eval_host(const void *plan_host, const float *d, float *q, int16_t *idx, size_t n);

/* Host model of the approximate-quotient element path the small-group / big-table kernels run for plans that allow it
 * (pure CPU): out[i] = fake-quant of x[i] at scale alpha / gmax, idx[i] its grid index, slow[i] (nullable) = 1 where the
 * margin test sent the element to the exact sequence.  rs_ulps: offset of the modelled reciprocal from RN(1 / scale) in
 * ulps (the device's v_rcp_f32 is specified to 1 ulp; results must not depend on it).  ANTQ_ERR_UNSUPPORTED for plans
 * without that path. */
int antq_plan_eval_host_a(const void *plan_host, const float *x, size_t n, float alpha, float gmax, int rs_ulps,
                          float *out, int16_t *idx, uint8_t *slow);

/* Host model of the 16-bit-domain row path (bf16 / f16 rows of at least 128 vectors with a 4- / 5-bit codebook: the
 * headline kernels; pure CPU): one row of n 16-bit patterns x16 at scale alpha / gmax -> the output patterns out16,
 * through the same per-row slot table, sentinel slot, far-clipped arithmetic and literal sequence the kernel uses.
 * path[i] (nullable): 0 = table, 1 = far-clipped arithmetic, 2 = literal sequence.  flags: ANTQ_FLAG_OVP (pairs inside
 * the row: n even).  ANTQ_ERR_UNSUPPORTED when the plan does not allow that path for `dtype` (ANTQ_BF16 / ANTQ_F16). */
int antq_plan_eval_host_h(const void *plan_host, const uint16_t *x16, size_t n, float alpha, float gmax, int dtype,
                          unsigned flags, uint16_t *out16, uint8_t *path);

/* ---------------------------------------------------------------------------
 * Fused Quantizer._forward with a calibrated (static) alpha:
 *     scale = alpha / gmax ; d = x / scale ; q = nearest(d) ; [OVP] ;
 *     out = ((q - d) + d) * scale
 * x/out: [rows, row_len] row-major, dtype F32 / BF16 / F16 (in place allowed).
 * alpha_dev: `rows` floats when alpha_per_row != 0 (is_perchannel), else 1.
 * Group-G quantisation = rows := numel/G, row_len := G on the same buffer.
 * gmax: max of the NORMAL grid (OliVe: without outliers, OQ:296).
 * idx_dev nullable.  flags: ANTQ_FLAG_OVP.
 * ------------------------------------------------------------------------- */
int antq_fakequant(const void *x_dev, void *out_dev, int16_t *idx_dev,
                   size_t rows, size_t row_len,
                   const float *alpha_dev, int alpha_per_row, float gmax,
                   const void *plan_host, const void *plan_dev,
                   unsigned flags, int dtype, void *stream);

/* ---------------------------------------------------------------------------
 * The same for a float64 tensor (a `.double()` model).  The reference's operator narrows to float INSIDE the kernel
 * (quant_kernel.cu:51, :28) while the tensor ops around it run in double: scale = alpha / gmax, d = x / scale,
 * q = grid[nearest(float(d))], [OVP], out = ((q - d) + d) * scale, all in double -- fused here (one read, one write).
 * alpha_dev: doubles (a double model's alpha Parameter is double).  flags: ANTQ_FLAG_OVP only.  8-byte aligned pointers.
 * Bit-identical to that op sequence; not a throughput path (16 B per element, a thread per flat pair).
 * ------------------------------------------------------------------------- */
int antq_fakequant_f64(const double *x_dev, double *out_dev, size_t rows, size_t row_len,
                       const double *alpha_dev, int alpha_per_row, double gmax,
                       const void *plan_host, const void *plan_dev, unsigned flags, void *stream);

/* ---------------------------------------------------------------------------
 * Same, with alpha computed in the kernel from the data (the initial alpha of
 * _init_quant_para, AQ:473-477, times one clip ratio as in search_mse AQ:300):
 *     alpha[r] = fl32(max_c |x[r,c]| * ratio)
 * One quant group (row) per wavefront / workgroup, single read of x.
 * alpha_out_dev (nullable): receives the `rows` alphas.  Per-row only.
 * A NaN in the row gives a NaN alpha, an Inf an Inf alpha (NaN wins over Inf), like antq_absmax.
 * ------------------------------------------------------------------------- */
int antq_fakequant_dynamic(const void *x_dev, void *out_dev, int16_t *idx_dev,
                           float *alpha_out_dev, size_t rows, size_t row_len,
                           float ratio, float gmax,
                           const void *plan_host, const void *plan_dev,
                           unsigned flags, int dtype, void *stream);

/* ---------------------------------------------------------------------------
 * Row abs-max (AQ:289,474 / per-tensor AQ:308,477):  amax[r] = max_c |x[r,c]|.
 * per_row == 0: one value for the whole tensor (workgroup maxima combined with an
 * integer atomicMax on the float's bits: order-independent, so bit-reproducible).
 * amax_dev need not be initialised in either mode.
 * ------------------------------------------------------------------------- */
int antq_absmax(const void *x_dev, float *amax_dev, size_t rows, size_t row_len,
                int per_row, int dtype, void *stream);

/* The whole-tensor abs-max as ONE launch: *amax_dev = max(*amax_dev, max_i |x[i]|) over n elements.  The caller provides
 * the initial value -- 0 for a fresh maximum (e.g. a slot of a buffer zeroed once for many calls: antq_absmax has to spend
 * a launch on that zero, 10.8 -> 7.6 us for a 4096 x 4096 bf16 tensor), or the running maximum of the blocks seen so far
 * (a tensor that arrives in pieces, a row-sharded quantiser's local blocks).  Same combination rule as antq_absmax
 * (integer atomicMax on the float's bits: order-independent, NaN wins). */
int antq_absmax_into(const void *x_dev, float *amax_dev, size_t n, int dtype, void *stream);

/* Whole-tensor reductions in ONE launch with nothing to zero per call (ABI 7).  reduce_ws_dev: ANTQ_REDUCE_WS_BYTES of
 * device memory owned by the caller, 16-byte aligned, ZEROED ONCE after allocation (hipMemsetAsync).  What a call relies on
 * is the ticket counters -- the first 8320 bytes (65 counters, 128 bytes apart) -- and those every call leaves zeroed again,
 * so calls issued one after the other on ONE stream share one block -- two streams never do.  The bytes behind the counters
 * are scratch: the workgroup partials (16 KiB from byte 16384) and the group partials (1 KiB from byte 40960) keep what the
 * last call wrote, no call reads them before it has written them, and the rest of the block is never written
 * (tests/test_gpu_scratch_contracts.py).  Inside:
 * last-arriver tickets, one counter per group of workgroups (no more than 32 atomics ever queue on one address) and the
 * workgroup / group partials, folded in index order: results do not depend on which workgroup finishes last.
 *   antq_absmax_t     : *amax_dev = max_i |x[i]| over n elements, WRITTEN (not accumulated; amax_dev need not be
 *                       initialised).  Same value as antq_absmax(per_row = 0), NaN wins.  A 33.5 MB bf16 tensor: 9.3 us
 *                       (antq_absmax: zeroing launch + 256 atomics on one address) -> see profiles/r06_aux_kernels.log.
 *   antq_alpha_grad_t : *gsum_dev = sum_i fl32(gout[i] * fl32(out[i] - x[i])) in double, the per-tensor form of
 *                       antq_alpha_grad as one launch (that entry point: a second launch adds the partials).  Sums are
 *                       formed in one fixed tree -- bit-reproducible, but not the tree of antq_alpha_grad: the two may
 *                       differ in the last bits of the double. */
#define ANTQ_REDUCE_WS_BYTES 65536
int antq_absmax_t(const void *x_dev, float *amax_dev, size_t n, int dtype, void *reduce_ws_dev, void *stream);
int antq_alpha_grad_t(const void *x_dev, const void *out_dev, const void *gout_dev, size_t n, double *gsum_dev, int dtype,
                      void *reduce_ws_dev, void *stream);

/* ---------------------------------------------------------------------------
 * Backward of antq_fakequant with respect to alpha (QAT: alpha is a Parameter, AQ:39; the autograd graph of
 * AQ:535-551 gives d out / d alpha = (q - d) / max(grid) = (out - x) / alpha and d out / d x = 1):
 *     gsum[r] = sum_c fl32( gout[r,c] * fl32(out[r,c] - x[r,c]) )     fp32 terms, fp64 accumulation
 * The caller divides by alpha[r].  x / out / gout: [rows, row_len] of `dtype` (F32 / BF16 / F16); gsum_dev: `rows`
 * doubles (alpha_per_row) or 1, not initialised.  The per-tensor sum is formed from workgroup partials in
 * workspace_dev (antq_search_workspace_bytes() bytes of scratch, as for antq_search_sse; may be NULL per row) in a
 * fixed order: no floating-point atomics, the same bits on every run.
 * ------------------------------------------------------------------------- */
int antq_alpha_grad(const void *x_dev, const void *out_dev, const void *gout_dev, size_t rows, size_t row_len,
                    int alpha_per_row, double *gsum_dev, void *workspace_dev, int dtype, void *stream);

/* ---------------------------------------------------------------------------
 * mse_loss of a fake-quantised tensor against its source without materialising
 * it (AQ:280-285 applied to AQ:535-551): for every candidate c in [0,ncand)
 *     alpha_c[r] = fl32(xmax[r] * ratios[c])
 *     sse[c, r]  = sum_col ( fl32|fakequant(x; alpha_c)[r,col] - x[r,col]| )^2
 * accumulated in fp32 per lane and fp64 across lanes.  The caller divides by
 * row_len and picks the arg-min (strict '<', first best), as search_mse does.
 * sse_dev: [ncand, rows] doubles (per_row) or [ncand] (per tensor); it need not
 * be initialised.  ratios_dev: ncand floats.  xmax_dev: rows floats or 1.
 * Every sum is formed in one fixed order (no floating-point atomics): the result
 * is bit-identical from run to run, so near-tied candidates resolve the same way
 * every time and on every rank.  A sum over the whole tensor (per_row == 0, or a
 * single row) is formed from workgroup partials kept in workspace_dev:
 * antq_search_workspace_bytes() bytes of device memory owned by the caller, not
 * shared with a call running concurrently on another stream; contents are
 * scratch (no initialisation).  May be NULL for per_row with rows > 1.
 * A bf16 / f16 tensor with ONE scale (per_row == 0 or rows == 1) and at least 2^19 elements (2^20 with ANTQ_FLAG_OVP) is scored on its 65 536-bin
 * histogram (one pass counts the bit patterns, then every pattern with a non-zero count goes through the literal reference
 * sequence for every candidate: count x term, summed in double in one fixed order): the same terms as the element-by-element
 * kernels, added in another order (relative 1e-7 on a sum).  With ANTQ_FLAG_OVP the pass also lists the pairs that hold an
 * outlier-capable element and the scoring corrects the victims' terms from that list; a tensor with too many such pairs
 * (> ~8 %) is searched by the element-by-element kernels instead (decided on the device, no synchronisation).  The workspace
 * holds the slabs and the list: always size it with antq_search_workspace_bytes() (48.3 MiB since ABI 6; 8 MiB before).
 * Per-row searches on rows of >= 128 elements (>= 256 with ANTQ_FLAG_OVP) of codebooks with a threshold list, and fp32
 * tensors with ONE scale from 2^20 elements, are scored from the SORTED row / 4096-element chunk (round 6): counts and sums
 * of the elements beyond every x-domain threshold by binary search into integer prefix sums, the squared error in closed
 * form in double -- the terms are not rounded to fp32 one by one, so these sums lie within 1e-14 of the exact float64 sum of
 * the reference's per-element outputs where the element-by-element kernels lie within 2e-7 (the reference's own fp32
 * reduction: 3e-7).  Same arguments, same workspace, bit-identical from run to run.
 * ------------------------------------------------------------------------- */
size_t antq_search_workspace_bytes(void);
int antq_search_sse(const void *x_dev, size_t rows, size_t row_len,
                    const float *xmax_dev, int per_row,
                    const float *ratios_dev, int ncand, float gmax,
                    const void *plan_host, const void *plan_dev,
                    unsigned flags, int dtype, double *sse_dev, void *workspace_dev, void *stream);

/* The type selection (search_adaptive_numeric_type, AQ:328-415 / OQ:235-256) on ONE read of the tensor: the sums of
 * antq_search_sse for `ntypes` (<= 4) codebooks at once,
 *     sse[t, c, r]  = sum_col ( fl32|fakequant_t(x; xmax[r] * ratios[c])[r,col] - x[r,col]| )^2
 * sse_dev: [ntypes, ncand, rows] doubles (per_row) or [ntypes, ncand], not initialised; workspace_dev as for
 * antq_search_sse (same order-fixed sums).  gmax_host, plan_host, plan_dev: host arrays of ntypes entries.  Every plan must have the x-domain path (all ANT / OliVe codebooks up to 128
 * buckets) and rows must be whole 16-byte vectors, at least 64 of them (1 KiB): otherwise ANTQ_ERR_UNSUPPORTED and the
 * caller issues one antq_search_sse per type. */
int antq_search_sse_multi(const void *x_dev, size_t rows, size_t row_len, const float *xmax_dev, int per_row,
                          const float *ratios_dev, int ncand, int ntypes, const float *gmax_host,
                          const void *const *plan_host, const void *const *plan_dev,
                          unsigned flags, int dtype, double *sse_dev, void *workspace_dev, void *stream);

/* The selection step of search_mse on the device (AQ:299-306 / :317-324): for every row r
 *     score_c = fl32(sse[c, r] / row_len), c ascending; best starts at 1e10 and is replaced on a strict `<`
 *     best_alpha[r] = fl32(xmax[r] * ratios[c*]) of the first best candidate, xmax[r] if none qualifies.
 * na = rows (per-channel) or 1.  Keeps the whole calibration free of device->host syncs. */
int antq_search_pick(const double *sse_dev, const float *xmax_dev, const float *ratios_dev, int ncand,
                     size_t na, size_t row_len, float *best_score_dev, float *best_alpha_dev, void *stream);

/* ---------------------------------------------------------------------------
 * The whole first-call calibration of one quantiser in ONE call, stream-ordered, without a device->host sync
 * (Quantizer._init_quant_para's search: search_mse AQ:287-326 per candidate type, the type choice of
 * search_adaptive_numeric_type AQ:328-415; OliVe OQ:189-256) -- the composition of the entry points above that
 * ant/quant_modules.py and olive/quant_modules.py perform step by step:
 *   x_max      ANTQ_XMAX_ABSMAX: row / tensor abs-max (ANT, AQ:289 / :308) written to xmax_dev;
 *              ANTQ_XMAX_3SIGMA: max(|mean + 3 std|, |mean - 3 std|) (OliVe, OQ:193-197 / :213-218) written to xmax_dev;
 *              ANTQ_XMAX_GIVEN : xmax_dev is an input (a statistic all-reduced over ranks, `no_outlier`, ...)
 *   candidates i = lb, lb + step, ... < ub:  alpha_i[r] = fl32(xmax[r] * fl32(i * 0.01))   (ANT: step 1; OliVe: step 2)
 *   per type t (ntypes codebooks: plan_host / plan_dev / gmax_host arrays), per row r (alpha_per_row) or for the tensor:
 *              alpha_dev[t * na + r] = the candidate with the smallest mean squared error, the first one on ties, x_max
 *              when the candidate list is empty or no error is below 1e10 (AQ:299-306)
 *   score_dev[t] = sum over rows of the best mean squared error (what search_mse returns, AQ:326), summed in double in
 *              one fixed order and rounded to float
 *   type_dev[0]  = the t with the smallest score, the first on ties, NaN scores last (np.argsort(mse)[0], AQ:413-415)
 * na = rows (alpha_per_row) or 1.  flags: ANTQ_FLAG_OVP searches with OliVe's outlier-victim pairs applied.
 * workspace_dev: antq_calibrate_workspace_bytes(...) bytes of caller-owned scratch, 16-byte aligned, not shared with a
 * call running concurrently on another stream.  The host decides lb / ub (ANT: lb = 95 when bit > 6, AQ:291-292) and which
 * codebooks are candidates (the `-float1..4` quirk of AQ:370-397 included: pass float_value(1)'s plan for each).
 * ------------------------------------------------------------------------- */
#define ANTQ_XMAX_GIVEN  0
#define ANTQ_XMAX_ABSMAX 1
#define ANTQ_XMAX_3SIGMA 2
size_t antq_calibrate_workspace_bytes(size_t rows, int alpha_per_row, int lb, int ub, int step, int ntypes);
int antq_calibrate(const void *x_dev, size_t rows, size_t row_len, int alpha_per_row, int dtype,
                   int xmax_mode, float *xmax_dev, int lb, int ub, int step,
                   int ntypes, const float *gmax_host, const void *const *plan_host, const void *const *plan_dev,
                   unsigned flags, float *alpha_dev, float *score_dev, int32_t *type_dev,
                   void *workspace_dev, size_t workspace_bytes, void *stream);

/* What _init_quant_para leaves behind (AQ:468-533, OQ:258-292) for a quantiser with ONE scale whose type was picked ON THE
 * DEVICE by antq_calibrate -- without the host learning the pick (ABI 7).  With t = *type_dev, stream-ordered, two launches:
 *   alpha_out[0] = alpha_dev[t];  mse_out[0] = score_dev[t] (the reference's log value, AQ:519-520);
 *   grid_out[0 .. grid_len) = grids_dev[t][..] (the candidates' codebooks, padded to one length, stacked by the caller;
 *   float32);  outl_out likewise from outl_dev (OliVe; NULL: none);
 *   out = the steady-state _forward of x with codebook t at alpha_dev[t] (AQ:535-551 / OQ:294-330; ANTQ_FLAG_OVP: pairs) --
 *   the calibrating call's own output, one pass over the tensor instead of one per candidate and a gather.
 * The host needs the pick only to NAME the mode (it copies *type_dev to pinned memory and reads it when the model's forward
 * has returned).  x: n elements, 16-byte aligned, n a multiple of the vector's element count (4 fp32 / 8 16-bit), otherwise
 * ANTQ_ERR_UNSUPPORTED (the caller quantises with every candidate and gathers, as before; nothing is written).  ntypes <= 4.
 * A pick outside 0 .. ntypes - 1 is CLAMPED to the nearest end by both launches (a negative *type_dev installs type 0, one of
 * ntypes or more installs type ntypes - 1): no read or write leaves the ntypes entries whatever the device holds.
 * mse_out, outl_dev and outl_out may be NULL (outl_out is written only when both outl pointers are given). */
int antq_calibrate_install(const void *x_dev, void *out_dev, size_t n, int dtype, int ntypes, const float *gmax_host,
                           const void *const *plan_host, const void *const *plan_dev, unsigned flags, const int32_t *type_dev,
                           const float *alpha_dev, const float *score_dev, const float *grids_dev, int grid_len, float *grid_out,
                           const float *outl_dev, int outl_len, float *outl_out, float *alpha_out, float *mse_out, void *stream);

/* The calibration of MANY quantisers in one call: job i is exactly antq_calibrate(jobs[i]...) -- same kernels, same order,
 * same bits -- all enqueued on `stream` one after the other through ONE workspace (antq_calibrate_batch_workspace_bytes: the
 * largest job's need; the jobs are stream-ordered, so they can share it).  The weight quantisers of a model do not depend
 * on any activation: a model calibrates all of them with this call before its first layer runs, reads the n type picks
 * back in ONE copy, and the per-layer host work and read-backs of the reference's first forward (one `if cuda_tensor:` per
 * quantiser, AQ:470, and np.argsort(...cpu()) per type selection, AQ:413) are gone for them.  dtype / flags are common to
 * the batch (a model's weights share a dtype; ANT or OliVe decides the pair rule).  Stops at the first job that fails and
 * returns its error; jobs before it are enqueued. */
typedef struct antq_calib_job {
    const void *x_dev;            /* rows x row_len elements */
    size_t rows, row_len;
    int alpha_per_row;
    int xmax_mode;                /* ANTQ_XMAX_* */
    float *xmax_dev;              /* na floats: output (ABSMAX / 3SIGMA) or input (GIVEN) */
    int lb, ub, step;
    int ntypes;
    const float *gmax_host;       /* ntypes */
    const void *const *plan_host; /* ntypes */
    const void *const *plan_dev;  /* ntypes */
    float *alpha_dev;             /* ntypes x na */
    float *score_dev;             /* ntypes */
    int32_t *type_dev;            /* 1 */
} antq_calib_job;
size_t antq_calibrate_batch_workspace_bytes(const antq_calib_job *jobs, int n);     /* 0: a job has a bad range / type count */
int antq_calibrate_batch(const antq_calib_job *jobs, int n, int dtype, unsigned flags, void *workspace_dev,
                         size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * AsymmetricQuantFunction.forward (ant_quantization/antquant/quant_affine.py:95-115)
 *     scale = (2^k-1)/clamp(max-min,1e-8); zp = round(scale*min) + 2^(k-1)
 *     q = clamp(round(scale*x - zp), -2^(k-1), 2^(k-1)-1); out = (q+zp)/scale
 * xmin_dev/xmax_dev: `rows` floats (per_row) or 1.  q_dev nullable (int32).
 * F32 only (the reference path is fp32 PyTorch).
 * ------------------------------------------------------------------------- */
int antq_affine(const float *x_dev, float *out_dev, int32_t *q_dev,
                size_t rows, size_t row_len, int k,
                const float *xmin_dev, const float *xmax_dev, int per_row,
                void *stream);

/* ---------------------------------------------------------------------------
 * Batched launch: many independent fake-quant jobs (e.g. the 54 weight tensors of a ResNet-50,
 * SURVEY 8a C1) in ONE kernel launch.  Small tensors are launch-bound when issued one by one
 * (~6 us of host time each vs < 1 us of HBM time); here every workgroup looks up its job in a
 * descriptor table that the caller builds once (weights and alphas are static between
 * forwards) and keeps resident on the device.
 *   antq_batch_build : pure host code; writes the descriptor blob (returns its size in bytes).  All jobs share dtype
 *                      and flags.  Jobs whose rows are not a multiple of 16 bytes (conv1: K = 147) or whose
 *                      buffers are not 16-byte aligned run element-granular inside the same launch.
 *                      With ANTQ_FLAG_DYNAMIC every job's alpha_dev is an OUTPUT (NULL: the scales are not stored):
 *                      alpha[r] = max_c |x[r,c]| is computed in the kernel from the registers holding the group / row
 *                      (antq_fakequant_dynamic with ratio 1, many tensors, one launch); per row only, groups of a
 *                      power of two of 16-byte vectors up to 64, or rows of 128 .. 8192 vectors (beyond 512 the plan
 *                      must be x-domain eligible: every ANT / OliVe 4-bit codebook), otherwise ANTQ_ERR_UNSUPPORTED.
 *   antq_fakequant_batch : one launch for all jobs; batch_dev is the caller's device copy.
 * ------------------------------------------------------------------------- */
typedef struct antq_job {
    const void  *x_dev;
    void        *out_dev;
    const float *alpha_dev;
    size_t       rows, row_len;
    int          alpha_per_row;
    float        gmax;
    const void  *plan_host;
    const void  *plan_dev;
} antq_job;

size_t antq_batch_capacity(const antq_job *jobs, int n, int dtype);   /* bytes antq_batch_build needs */
int antq_batch_build(const antq_job *jobs, int n, int dtype, unsigned flags, void *batch_host, size_t capacity);
int antq_fakequant_batch(const void *batch_host, const void *batch_dev, void *stream);

/* ---------------------------------------------------------------------------
 * Packed 4-bit codec: the quantised tensor itself instead of its fake-quant image
 * (SURVEY 8f N4).  Two codes per byte, element 2k in the low nibble.
 *   code = scan-order grid index of the element (what antq_fakequant's idx output holds),
 *   m <= 16 for plain grids (ANT 4-bit: the 16-entry grid incl. its duplicate zero).
 * With ANTQ_FLAG_OVP the grid is OliVe's cat(normal[n_normal <= 15], outliers[<= 15]):
 *   normal value  -> its index 0..n_normal-1
 *   victim        -> 15, the outlier identifier (the paper's reserved code)
 *   outlier       -> index INTO THE OUTLIER LIST; the partner nibble of the pair is 15,
 *                    which is what tells the decoder to use the outlier codebook.
 * antq_decode4 writes fl(v * scale) for the decoded grid value v.  That is bit-identical to antq_fakequant(x) whenever
 * the reference's straight-through step ((q - d) + d) is exact, which holds for every ANT / OliVe 4-bit codebook
 * (adjacent magnitudes within a factor of two: the condition the plan builder records as its x-domain eligibility)
 * and finite inputs within twice the outermost grid values; for arbitrary value lists the two may differ by one ulp.
 * Elements outside the scan's validity range (code would be ANTQ_IDX_NONE) encode as the
 * grid entry holding 0.0.  row_len must be a multiple of 8; x: F32 / BF16 / F16; codes: rows*row_len/2 bytes.
 * (BF16 / F16 rows of at least 1024 elements are encoded in the tensor's own 16-bit domain: the per-row slot table of the
 *  headline kernels holding code bytes instead of output patterns, antq_k_codec.h: k_encode4_hrow.)
 * ------------------------------------------------------------------------- */
int antq_encode4(const void *x_dev, uint8_t *codes_dev, size_t rows, size_t row_len,
                 const float *alpha_dev, int alpha_per_row, float gmax,
                 const void *plan_host, const void *plan_dev, int n_normal,
                 unsigned flags, int dtype, void *stream);
int antq_decode4(const uint8_t *codes_dev, void *out_dev, size_t rows, size_t row_len,
                 const float *alpha_dev, int alpha_per_row, float gmax,
                 const void *plan_host, const void *plan_dev, int n_normal,
                 unsigned flags, int dtype, void *stream);

/* ---------------------------------------------------------------------------
 * Batched decode: many packed tensors (the 54 weights of a ResNet-50, the row blocks of an LLM) -> their fake-quant images
 * in ONE launch, the decode-side counterpart of antq_fakequant_batch.  Job i's output is bit-identical to antq_decode4 on
 * that job alone: fl((g[c] + 0.0f) * (alpha / gmax)) with the pair rule above, bf16 / f16 rounded to nearest even.
 *   antq_decode4_batch_build : pure host code, touches no HIP; writes the descriptor blob (returns its size in bytes).  All
 *                      jobs share dtype (F32 / BF16 / F16) and flags (0 or ANTQ_FLAG_OVP); every job has its own
 *                      codebook.  The codebook is passed as grid_dev -- m floats on the device, the grid in the order a
 *                      plan is built from (ANT: the sorted grid; OliVe: cat(normal, outliers)) -- not as a plan: the
 *                      decoder needs nothing else of a plan, and the builder stays free of the plan format.
 *                      1 <= n <= 65535 jobs (capacity returns 0, build ANTQ_ERR_ARG otherwise); a flag bit other than
 *                      ANTQ_FLAG_OVP: ANTQ_ERR_ARG.
 *                      Refusals as in antq_decode4, reported here, before anything is launched: row_len % 8 != 0, m > 16,
 *                      n_normal outside 1..15 or more than 15 outliers (ANTQ_FLAG_OVP): ANTQ_ERR_UNSUPPORTED; a null
 *                      pointer, an empty job: ANTQ_ERR_ARG; out_dev not aligned to its element: ANTQ_ERR_ALIGN; capacity
 *                      too small: ANTQ_ERR_PLAN.  Jobs whose codes_dev is not 4-byte or whose out_dev is not 16-byte
 *                      aligned run element-granular inside the same launch.  n_normal is read with ANTQ_FLAG_OVP only.
 *   antq_decode4_batch : one launch for all jobs; batch_dev is the caller's device copy of the blob.  No allocation, no
 *                      synchronisation; stream-ordered and capturable.
 * ------------------------------------------------------------------------- */
typedef struct antq_decode_job {
    const uint8_t *codes_dev;   /* rows*row_len/2 bytes, element 2k in the low nibble */
    void          *out_dev;
    const float   *alpha_dev;   /* rows floats (alpha_per_row) or 1 */
    size_t         rows, row_len;
    int            alpha_per_row;
    float          gmax;
    const float   *grid_dev;    /* m floats: the plan's grid as antq_decode4 reads it */
    int            m, n_normal; /* n_normal only with ANTQ_FLAG_OVP */
} antq_decode_job;
size_t antq_decode4_batch_capacity(const antq_decode_job *jobs, int n, int dtype);   /* bytes antq_decode4_batch_build needs; 0: bad arguments */
int    antq_decode4_batch_build(const antq_decode_job *jobs, int n, int dtype, unsigned flags,
                                void *batch_host, size_t capacity);
int    antq_decode4_batch(const void *batch_host, const void *batch_dev, void *stream);

/* ---------------------------------------------------------------------------
 * Byte codes: the same codec with ONE code per byte, for the 5- to 8-bit layers of mixed-precision models (books of up to
 * 256 values) and for rows the 4-bit codec refuses (row_len % 8 == 4).  Element i of the flat tensor is byte i.
 *   plain books: 1 <= m <= 256; code = scan-order grid index of the element (what antq_fakequant's idx output holds).
 * With ANTQ_FLAG_OVP the grid is cat(normal[n_normal], outliers) with 1 <= n_normal <= 255 and 0 <= m - n_normal <= 255:
 *   normal value  -> its index 0..n_normal-1
 *   victim        -> 255, the identifier
 *   outlier       -> index INTO THE OUTLIER LIST (0..254); the partner byte of the pair is 255.
 * The pair rule and the outlier test (|v| > 32) are antq_encode4's, on the flat pairs (2k, 2k + 1); an element outside the
 * scan's validity range (ANTQ_IDX_NONE) encodes as the last grid entry (ANTQ_FLAG_OVP: normal entry) holding 0.0.
 * antq_decode8 writes fl((g[c] + 0.0f) * (alpha / gmax)), the scale formed in the kernel in fp32, bf16 / f16 rounded to nearest
 * even; a victim decodes to +0, and so does a code beyond the book (a byte >= m; with ANTQ_FLAG_OVP a byte >= n_normal other
 * than 255, or an outlier index >= m - n_normal).  As for the 4-bit codec, decode8(encode8(x)) is bit-identical to
 * antq_fakequant(x) whenever the reference's straight-through step ((q - d) + d) is exact: every ANT / OliVe codebook
 * (adjacent magnitudes within a factor of two: the plan builder's x-domain eligibility) and finite inputs within twice the
 * outermost grid values; for arbitrary value lists the two may differ by one ulp.
 * Refusals, all before anything is launched: row_len % 4 != 0 or a book outside the bounds above: ANTQ_ERR_UNSUPPORTED (so is
 * F64 or any other dtype); a null pointer or an empty tensor: ANTQ_ERR_ARG; a flag other than ANTQ_FLAG_OVP: ANTQ_ERR_ARG;
 * x_dev / out_dev not aligned to its element: ANTQ_ERR_ALIGN; (batch) capacity too small: ANTQ_ERR_PLAN.
 * codes_dev: rows*row_len bytes, any alignment.  With row_len % 4 == 0 a code word lies inside one row and a pair never
 * crosses a row.  Codes that are not 4-byte aligned, outputs that are not 16-byte aligned and 16-bit rows of 4 mod 8 elements
 * run element-granular (inside the same launch, in a batch).  x: F32 / BF16 / F16, read 16 bytes per lane when x_dev is
 * 16-byte aligned.  The encoder is the element encoder of antq_encode4 (no row-table, no 16-bit-domain form).
 * The batch entry points are antq_decode4_batch's with antq_decode_job as it is -- codes_dev holds rows*row_len bytes --
 * and the same rules for n, flags and n_normal; the builder is pure host code and touches no HIP.  All launches are
 * stream-ordered and capturable: no allocation, no synchronisation, no workspace.  antq_linear4 and antq_linear4_mm take
 * 4-bit codes only; antq_linear8 (below) is the linear from byte codes for 1 .. 8 rows of x, antq_linear8_mm its matrix-core form.
 * ------------------------------------------------------------------------- */
int antq_encode8(const void *x_dev, uint8_t *codes_dev, size_t rows, size_t row_len,
                 const float *alpha_dev, int alpha_per_row, float gmax,
                 const void *plan_host, const void *plan_dev, int n_normal,
                 unsigned flags, int dtype, void *stream);
int antq_decode8(const uint8_t *codes_dev, void *out_dev, size_t rows, size_t row_len,
                 const float *alpha_dev, int alpha_per_row, float gmax,
                 const void *plan_host, const void *plan_dev, int n_normal,
                 unsigned flags, int dtype, void *stream);
size_t antq_decode8_batch_capacity(const antq_decode_job *jobs, int n, int dtype);   /* bytes antq_decode8_batch_build needs; 0: bad arguments */
int    antq_decode8_batch_build(const antq_decode_job *jobs, int n, int dtype, unsigned flags,
                                void *batch_host, size_t capacity);
int    antq_decode8_batch(const void *batch_host, const void *batch_dev, void *stream);

/* ---------------------------------------------------------------------------
 * Packed 4-bit linear: y = x . W^T (+ bias) for 1 .. ANTQ_LINEAR4_MAX_M rows of x, computed straight from the codes of W
 * (the consumer the codec exists for: a layer with few input rows streams its weights once, and the codes are a quarter
 * of the bf16 image's bytes).  codes: N rows of K codes in antq_encode4's layout; alpha / gmax / grid / m / n_normal as in
 * antq_decode_job, alpha_per_row: one scale per output row n.
 *   W[n,k] is, bit for bit, the element antq_decode4 writes for the same codes, alpha, gmax, grid and flags in `dtype`:
 *          fl((g[c] + 0.0f) * (alpha / gmax)) rounded to `dtype`, the pair rule applied -- not the unrounded product, and not
 *          a scale factored out of the sum.
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[n,k] + bias[n] ), products and sum accumulated in fp32 (fused multiply-adds).
 *   The order of the sum is the kernel's own, but fixed: the same input gives the same bits on every run, and y[m,.] does
 *          not depend on M or on the other rows of x -- a row computed alone has the bits it has inside a call of 8.
 *   No floating-point atomics, no split-K across workgroups, no inter-workgroup communication, no workspace, no allocation,
 *          no synchronisation: stream-ordered and capturable into a graph.
 *   Non-finite values (this entry point and antq_linear4_mm, antq_linear4_gemm, antq_linear8, antq_linear8_mm, antq_linear8_gemm alike): NaN and
 *          Inf in x, in W -- a NaN or Inf alpha, a weight that overflows `dtype`; 0 * Inf is a NaN weight, as in the decoder's
 *          image -- and in bias follow IEEE 754 per product and per sum: a NaN product or bias, 0 * Inf either way, or Inf - Inf
 *          give NaN, Inf of one sign gives that Inf.  A non-finite x[m,k] reaches row m of y only, a non-finite weight or
 *          scale of row n and bias[n] reach column n only.  Padding never reaches a stored y[m,n], whatever the weights:
 *          along K a lane past the end of the row has BOTH operands zero (not a zero x against a repeated weight, whose
 *          0 * Inf would be NaN) and adds exactly +0; padded rows m >= M and n >= N repeat the last real row and may well
 *          compute NaN, but only into accumulator rows and columns of their own, which are not stored.  The accumulators
 *          start at +0: a sum of -0 products, with or without a bias of -0.0, is +0.  (tests/test_gpu_linear_specials.py)
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          a null codes / x / y / alpha / grid, m < 1, a bad dtype, a flag bit other than ANTQ_FLAG_OVP
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  M > ANTQ_LINEAR4_MAX_M; K == 0 or K % 8 != 0; the decoder's refusals: m > 16, with ANTQ_FLAG_OVP
 *                         n_normal outside 1..15 or more than 15 outliers; N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        x_dev not 16-byte aligned, codes_dev not 4-byte aligned, y_dev / bias_dev not aligned to their element
 * Codes are read 16 bytes per lane when K % 32 == 0 and codes_dev is 16-byte aligned, 4 bytes per lane otherwise (the order
 * of the sum differs between the two, nothing else).  F32 / BF16 / F16.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR4_MAX_M 8
int antq_linear4(const uint8_t *codes_dev,          /* N*K/2 bytes, antq_encode4's layout */
                 const void *x_dev,                 /* [M, K] row-major, dtype */
                 const void *bias_dev,              /* N elements of dtype, or NULL */
                 void *y_dev,                       /* [M, N] row-major, dtype */
                 size_t M, size_t N, size_t K,
                 const float *alpha_dev, int alpha_per_row, float gmax,
                 const float *grid_dev, int m, int n_normal,   /* as in antq_decode_job */
                 unsigned flags /* 0 | ANTQ_FLAG_OVP */, int dtype /* F32 | BF16 | F16 */, void *stream);

/* ---------------------------------------------------------------------------
 * Packed 4-bit linear for weights stored [K, N] (GPT-2's Conv1D: weight [in, out], y = x @ W + b): y = x . W (+ bias) for
 * 1 .. ANTQ_LINEAR4_T_MAX_M rows of x, computed straight from the codes of W.  codes: K rows of N codes in antq_encode4's
 * layout (N / 2 bytes per row, element 2 j in the low nibble: OliVe's pairs are adjacent output columns); alpha_per_row: one
 * scale per row k of the codes, that is per INPUT feature; gmax / grid / m / n_normal / flags as in antq_linear4.
 *   W[k,n] is, bit for bit, the element antq_decode4 writes for the same codes, alpha, gmax, grid, flags and dtype: the
 *          decoder's own pair, scaled by alpha[k] / gmax (a true division) and rounded to `dtype` -- the scale is never
 *          factored out of the sum or folded into x.
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[k,n] + bias[n] ), products and sum accumulated in fp32 (fused multiply-adds).
 *   The tile rule, a function of K alone: partial sum P (0 .. 127) takes k = P, P + 128, ... < K in rising order from +0; the
 *          128 partial sums are combined in one fixed tree -- the 16 of a wavefront (P = 16 w + p) as four groups of four, each
 *          (p0 + p2) + (p1 + p3), the groups as (g0 + g1) + (g2 + g3), then the eight wavefronts' sums as
 *          ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) -- then the bias is added in fp32 and the result rounded once.
 *          A workgroup owns 32 consecutive output columns over the whole of K.  The bits of y[m,n] depend only on row m of
 *          x, column n of W, bias[n] and K: not on M, not on N, not on the other rows of x, not on the run.
 *   No floating-point atomics, no split of K across workgroups, no workspace, no allocation, no synchronisation:
 *          stream-ordered and capturable into a graph.  Reads stay inside the buffers: a step past the end of K and a column
 *          group past the end of N load nothing and add nothing (never a zero x against a repeated weight); padded rows of x
 *          repeat the last real row and are not stored.  The accumulators start at +0.
 *   Non-finite values follow IEEE 754 per product and per sum, as for antq_linear4.  With a scale per k, a NaN or Inf
 *          alpha[k] makes ROW k of W non-finite: it reaches every y[m, .], also where x[m,k] == 0 (0 * Inf is NaN), exactly
 *          as a product with the decoded image does.  A non-finite x[m,k] reaches row m of y only.
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          a null codes / x / y / alpha / grid, m < 1, a bad dtype, a flag bit other than ANTQ_FLAG_OVP
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  M > ANTQ_LINEAR4_T_MAX_M; K == 0 or K % 8 != 0; N % 8 != 0; the decoder's refusals (as antq_linear4);
 *                         N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        x_dev not 16-byte aligned, codes_dev not 4-byte aligned, y_dev / bias_dev not aligned to their element
 * F32 / BF16 / F16.  The scales are staged in LDS up to K = 8192 and divided per step beyond (the same bits).  Measured
 * (profiles/packed_linear_t.md; one MI355X, one run, GPT-2 small's and XL's Conv1D shapes, M = 1 / 2 / 4 / 8): faster than
 * antq_decode4 + addmm at every point of M = 1 (1.02 ... 2.26x) and at 21 ... 40 of 48 points beyond; faster than addmm on a
 * decoded image only at M = 1 (30 of 48 points, 0.72 ... 1.28x), slower at every point of M >= 2 (0.34 ... 1.00x); the codes
 * stream at 0.2 ... 4.5 % of 8 TB/s (the kernel is bound by latency and instruction count, not bandwidth).
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR4_T_MAX_M 8
int antq_linear4_t(const uint8_t *codes_dev /* K*N/2 bytes */, const void *x_dev /* [M, K] */, const void *bias_dev /* N or NULL */,
                   void *y_dev /* [M, N] */, size_t M, size_t N, size_t K, const float *alpha_dev, int alpha_per_row, float gmax,
                   const float *grid_dev, int m, int n_normal, unsigned flags, int dtype, void *stream);

/* ---------------------------------------------------------------------------
 * antq_linear4_t's product for 1 .. ANTQ_LINEAR4_T_MM_MAX_M rows of x on the matrix cores (v_mfma_f32_16x16x32_bf16 / _f16), BF16
 * and F16 only.  Parameters, layout and scales as antq_linear4_t: K rows of N / 2 bytes, one scale per row k or one per tensor,
 * OliVe's pairs in adjacent columns.
 *   W[k,n] is, bit for bit, the element antq_decode4 writes for the same codes, alpha, gmax, grid, flags and dtype: the
 *          decoder's own pair, scaled by alpha[k] / gmax (a true division) and rounded to `dtype`, then the MFMA operand as it
 *          is -- no widening, the scale never factored out of the sum or folded into x.
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[k,n] + bias[n] ): products exact, the sum in fp32 in the MFMA accumulator.
 *   The sum:
 *          Step s covers k in [32 s, 32 s + 32).
 *          Wavefront w takes steps w, w + 8, w + 16, ... in rising order.  They are chained in one fp32 MFMA accumulator from +0.
 *          Inside a step the place of k is fixed: k group kg, element r (k = 32 s + 8 kg + r).
 *          A wavefront without a step contributes +0.
 *          The eight partial tiles meet in LDS, in rounds (one tile of 16 rows of x per round, in the scales' memory).
 *          They are combined as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  Then the bias is added in fp32, then ONE
 *          rounding to the type.
 *          The bits of y[m,n] depend on row m of x, column n of W, bias[n] and K only.  They do not depend on M, the number of
 *          16-row tiles, the position of the row in its tile, N, the tile width (64 columns per workgroup), the column's place
 *          in its tile, the other rows of x, or the run.
 *          The order is neither antq_linear4_t's nor antq_linear4_mm's: the same row has different low bits from those entry
 *          points (each within the bound of an fp32 sum).
 *   No atomics, no split of K across workgroups, no workspace, no allocation, no synchronisation: stream-ordered and capturable
 *          into a graph.  Reads stay inside the buffers: K % 32 may not be 0, and a group of 8 k past the end of K loads nothing
 *          and has an all-zero W fragment AND an all-zero x fragment (exactly +0, whatever the weights); a column group past N
 *          loads nothing and is not stored; rows m >= M have all-zero x fragments and are not stored (a zero against an Inf
 *          weight there makes a NaN that nobody sees).
 *   Non-finite values follow IEEE 754 per product and per sum.  A NaN or Inf alpha[k] makes ROW k of W non-finite and reaches
 *          every y[m, .], also where x[m,k] == 0, exactly as a product with the decoded image does.  A non-finite x[m,k] reaches
 *          row m of y only.  Subnormal bf16 / f16 weights are kept by the 16-bit MFMA, as for antq_linear4_mm.
 * Checked before anything touches HIP, in antq_linear4_t's order:
 *   ANTQ_ERR_ARG          a null codes / x / y / alpha / grid, m < 1, a bad dtype, a flag bit other than ANTQ_FLAG_OVP
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  dtype == ANTQ_F32 (the f32-input MFMA runs at the vector rate: such calls stay with antq_linear4_t or
 *                         the image); M > ANTQ_LINEAR4_T_MM_MAX_M; K == 0 or K % 8 != 0; N % 8 != 0; the decoder's refusals (as
 *                         antq_linear4); N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        x_dev not 16-byte aligned, codes_dev not 4-byte aligned, y_dev / bias_dev not aligned to their element
 * The scales are staged in LDS up to K = 8192 and divided per use beyond (the same bits).
 * Measured (profiles/packed_linear_t_mm.md; one MI355X, one run, GPT-2 small's and XL's Conv1D shapes, M = 9 / 16 / 32 / 64, bf16 / f16,
 * two books): faster than antq_decode4 + addmm at 98 of 128 points (0.69 ... 1.84x), faster than addmm on a decoded image at 19 of 128
 * (0.45 ... 1.09x); at M = 8 faster than antq_linear4_t at 32 of 32 points (1.01 ... 1.91x).  Its own time grows 1.35 ... 1.49x from 9 to 64 rows;
 * the codes stream at 0.3 ... 4.4 % of 8 TB/s (bound by the decode's instruction count and by latency, not bandwidth).
 * Loses to antq_decode4 + addmm on the long-K layers [3072, 768] and [6400, 1600] at every M, and to addmm on the image everywhere but at
 * M = 32 on the K = 768 layers and on [1600, 4800] / [1600, 6400], and at M = 9 on those two in bf16 (by at most 9 %): an option for
 * memory and for the scratch buffer's lifetime rule, off by default in the packed bank.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR4_T_MM_MAX_M 64
int antq_linear4_t_mm(const uint8_t *codes_dev /* K*N/2 bytes */, const void *x_dev /* [M, K] */, const void *bias_dev /* N or NULL */,
                      void *y_dev /* [M, N] */, size_t M, size_t N, size_t K, const float *alpha_dev, int alpha_per_row, float gmax,
                      const float *grid_dev, int m, int n_normal, unsigned flags, int dtype /* BF16 | F16 */, void *stream);

/* ---------------------------------------------------------------------------
 * The same product for 1 .. ANTQ_LINEAR4_MM_MAX_M rows of x on the matrix cores (v_mfma_f32_16x16x32_bf16 / _f16), BF16 and
 * F16 only.  Parameters as antq_linear4.
 *   W[n,k] is, bit for bit, the element antq_decode4 writes in `dtype` (the decoder's byte table is the MFMA operand; the scale
 *          is never factored out of the sum).
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[n,k] + bias[n] ): products exact, the sum in fp32 in the MFMA accumulator, the bias
 *          added in fp32, one rounding to `dtype`.
 *   The bits of y[m,n] depend only on row m of x, row n of W, bias[n], K and the code path (below): not on M, not on N, not on
 *          the other rows of x, not on the run.  K is split between the eight wavefronts of a workgroup by a rule of K alone and
 *          their partial sums are combined through LDS in one fixed order.  The order of the sum is NOT antq_linear4's: the
 *          same row has different low bits from the two entry points (both within the bound of an fp32 sum).
 *   No floating-point atomics, no split of K across workgroups, no workspace, no allocation, no synchronisation: stream-ordered
 *          and capturable into a graph.  Reads stay inside the buffers; lanes past the end of K add exactly +0, whatever
 *          the weights, and padded rows are not stored (non-finite values: as antq_linear4).
 *   Subnormal bf16 / f16 weights and inputs are kept by the 16-bit MFMA on gfx950 (measured on an MI355X: a one-hot x returns the
 *          image's subnormal elements bit for bit), so W is the image there too: there is no departure to state.
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          as antq_linear4
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  dtype == ANTQ_F32 (the f32-input MFMA runs at the vector rate: such layers stay with antq_linear4);
 *                         M > ANTQ_LINEAR4_MM_MAX_M; K == 0 or K % 8 != 0; the decoder's refusals; N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        as antq_linear4
 * Codes are read 16 bytes per lane when K % 32 == 0 and codes_dev is 16-byte aligned, 4 bytes per lane otherwise (the order
 * of the sum differs between the two, nothing else).  Measurements: profiles/packed_linear_mm.md.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR4_MM_MAX_M 64
int antq_linear4_mm(const uint8_t *codes_dev, const void *x_dev, const void *bias_dev, void *y_dev,
                    size_t M, size_t N, size_t K,
                    const float *alpha_dev, int alpha_per_row, float gmax,
                    const float *grid_dev, int m, int n_normal,
                    unsigned flags /* 0 | ANTQ_FLAG_OVP */, int dtype /* BF16 | F16 */, void *stream);

/* ---------------------------------------------------------------------------
 * The same product for 1 .. ANTQ_LINEAR4_GEMM_MAX_M rows of x as a tiled matrix-core product, BF16 and F16 only: every workgroup
 * takes one (128 or 256 rows of x, 64 output rows) tile, x is staged through LDS, K is not split.  Parameters as antq_linear4.
 *   W[n,k] is, bit for bit, the element antq_decode4 writes in `dtype` (the decoder's byte table is the MFMA operand; no
 *          widening, the scale is never factored out of the sum).
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[n,k] + bias[n] ): ONE fp32 MFMA accumulator chain over K in steps of 128 elements in
 *          rising order, the bias added in fp32, one rounding to `dtype`.  K is split neither across wavefronts nor across
 *          workgroups.
 *   The bits of y[m,n] depend only on row m of x, row n of W, bias[n], K and the code path (below): not on M, not on N, not on
 *          the other rows of x, not on the tile shape, not on the run.  The order of the sum is this kernel's own -- NOT
 *          antq_linear4's and NOT antq_linear4_mm's: the same row has different low bits from the three entry points (each
 *          within the bound of an fp32 sum).
 *   No floating-point atomics, no workspace, no allocation, no synchronisation: stream-ordered and capturable into a graph.
 *          Rows m >= M, n >= N and k >= K of the last step clamp their addresses into the buffers; k >= K adds exactly +0
 *          whatever the weights, padded rows are not stored (non-finite values: as antq_linear4): no read or write falls
 *          outside codes, x, bias, alpha / grid and y.
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          as antq_linear4
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  dtype == ANTQ_F32; M > ANTQ_LINEAR4_GEMM_MAX_M; K == 0 or K % 8 != 0; the decoder's refusals;
 *                         N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        as antq_linear4
 * Codes are read 16 bytes per lane when K % 32 == 0 and codes_dev is 16-byte aligned, 4 bytes per lane otherwise (the order
 * of the sum differs between the two, nothing else).  Measurements: profiles/packed_linear4_gemm.md.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR4_GEMM_MAX_M 4096
int antq_linear4_gemm(const uint8_t *codes_dev, const void *x_dev, const void *bias_dev, void *y_dev,
                      size_t M, size_t N, size_t K,
                      const float *alpha_dev, int alpha_per_row, float gmax,
                      const float *grid_dev, int m, int n_normal,
                      unsigned flags /* 0 | ANTQ_FLAG_OVP */, int dtype /* BF16 | F16 */, void *stream);

/* ---------------------------------------------------------------------------
 * The byte-code form of antq_linear4_gemm: the same tiled matrix-core product for 1 .. ANTQ_LINEAR8_GEMM_MAX_M rows of x from
 * the byte codes of W, BF16 and F16 only -- one kernel, written once over the two code widths.  Parameters as antq_linear8.
 *   W[n,k] is, bit for bit, the element antq_decode8 writes in `dtype` (antq_linear8_mm's tables of the decoder's finished
 *          16-bit outputs, for the 64 output rows of a tile; two look-ups are one MFMA operand register).
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[n,k] + bias[n] ): ONE fp32 MFMA accumulator chain over K in steps of 128 elements in
 *          rising order, the bias added in fp32, one rounding to `dtype`.  K is split neither across wavefronts nor across
 *          workgroups.
 *   The bits of y[m,n] depend only on row m of x, row n of W, bias[n], K and the code path (below): not on M, not on N, not on
 *          the other rows of x, not on the tile shape, not on the run.  The order of the sum is this kernel's own -- NOT
 *          antq_linear8's and NOT antq_linear8_mm's.
 *   No floating-point atomics, no workspace, no allocation, no synchronisation: stream-ordered and capturable into a graph.
 *          Rows m >= M, n >= N and k >= K of the last step clamp their addresses into the buffers; k >= K adds exactly +0
 *          whatever the weights, padded rows are not stored (non-finite values: as antq_linear4).
 *   At most 128 KB of LDS per workgroup (the pair rule's tables of 64 rows and the staged x of 256 rows).
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          as antq_linear8
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  dtype == ANTQ_F32; M > ANTQ_LINEAR8_GEMM_MAX_M; K == 0 or K % 8 != 0; the byte decoder's refusals;
 *                         N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        x_dev not 16-byte aligned, codes_dev not 8-byte aligned, y_dev / bias_dev not 2-byte aligned
 * Codes are read 16 bytes per load (two loads per lane, output row and step) when K % 16 == 0 and codes_dev is 16-byte aligned,
 * 8 bytes per load (four) otherwise (the order of the sum differs between the two, nothing else).  antq_debug_set key 23
 * forces the tile shape as for antq_linear4_gemm.  Measurements: profiles/packed_linear8_gemm.md.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR8_GEMM_MAX_M 4096
int antq_linear8_gemm(const uint8_t *codes_dev, const void *x_dev, const void *bias_dev, void *y_dev,
                      size_t M, size_t N, size_t K,
                      const float *alpha_dev, int alpha_per_row, float gmax,
                      const float *grid_dev, int m, int n_normal,
                      unsigned flags /* 0 | ANTQ_FLAG_OVP */, int dtype /* BF16 | F16 */, void *stream);

/* ---------------------------------------------------------------------------
 * Packed byte-code linear: antq_linear4 for the byte codes of W -- y = x . W^T (+ bias) for 1 .. ANTQ_LINEAR8_MAX_M rows of x,
 * computed straight from the codes (half the bytes of the bf16 image, a quarter of the fp32 image).  codes: N rows of K
 * bytes in antq_encode8's layout; alpha / gmax / grid / m / n_normal as in antq_decode_job, alpha_per_row: one scale per
 * output row n.
 *   W[n,k] is, bit for bit, the element antq_decode8 writes for the same codes, alpha, gmax, grid and flags in `dtype`:
 *          fl((g[c] + 0.0f) * (alpha / gmax)) rounded to `dtype`, the pair rule applied on the flat pairs (2k, 2k + 1), a victim
 *          and a code beyond the book +0 -- not the unrounded product, and not a scale factored out of the sum.
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[n,k] + bias[n] ), products and sum accumulated in fp32 (fused multiply-adds).
 *   The order of the sum is the kernel's own, but fixed: the same input gives the same bits on every run, and y[m,.] does
 *          not depend on M or on the other rows of x -- a row computed alone has the bits it has inside a call of 8.
 *   No floating-point atomics, no split-K across workgroups, no inter-workgroup communication, no workspace, no allocation,
 *          no synchronisation: stream-ordered and capturable into a graph.  Non-finite values: as antq_linear4.
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          a null codes / x / y / alpha / grid, m < 1, a bad dtype, a flag bit other than ANTQ_FLAG_OVP
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  M > ANTQ_LINEAR8_MAX_M; K == 0 or K % 8 != 0; the byte decoder's refusals: m > 256, with
 *                         ANTQ_FLAG_OVP n_normal outside 1..255 or m - n_normal outside 0..255; N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        x_dev not 16-byte aligned, codes_dev not 8-byte aligned, y_dev / bias_dev not aligned to their element
 * Codes are read 16 bytes per lane when K % 16 == 0 and codes_dev is 16-byte aligned, 8 bytes per lane otherwise (the order
 * of the sum differs between the two, nothing else).  F32 / BF16 / F16.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR8_MAX_M 8
int antq_linear8(const uint8_t *codes_dev,          /* N*K bytes, antq_encode8's layout */
                 const void *x_dev, const void *bias_dev, void *y_dev,
                 size_t M, size_t N, size_t K,
                 const float *alpha_dev, int alpha_per_row, float gmax,
                 const float *grid_dev, int m, int n_normal,   /* as in antq_decode_job */
                 unsigned flags /* 0 | ANTQ_FLAG_OVP */, int dtype /* F32 | BF16 | F16 */, void *stream);

/* ---------------------------------------------------------------------------
 * The same product for 1 .. ANTQ_LINEAR8_MM_MAX_M rows of x on the matrix cores (v_mfma_f32_16x16x32_bf16 / _f16), BF16 and
 * F16 only: antq_linear4_mm for byte codes.  Parameters as antq_linear8.
 *   W[n,k] is, bit for bit, the element antq_decode8 writes in `dtype` (per output row a table of the decoder's finished
 *          16-bit outputs keyed by the code byte, with the pair rule a second one for the outlier list; two look-ups are one
 *          MFMA operand register; the scale is never factored out of the sum).
 *   y[m,n] = round_dtype( sum_k x[m,k] * W[n,k] + bias[n] ): products exact, the sum in fp32 in the MFMA accumulator, the bias
 *          added in fp32, one rounding to `dtype`.
 *   The bits of y[m,n] depend only on row m of x, row n of W, bias[n], K and the code path (below): not on M, not on N, not on
 *          the other rows of x, not on the run.  K is split between the eight wavefronts of a workgroup by a rule of K alone and
 *          their partial sums are combined through LDS in one fixed order.  The order of the sum is NOT antq_linear8's: the
 *          same row has different low bits from the two entry points (both within the bound of an fp32 sum).
 *   No floating-point atomics, no split of K across workgroups, no workspace, no allocation, no synchronisation: stream-ordered
 *          and capturable into a graph.  Reads stay inside the buffers; lanes past the end of K add exactly +0, whatever
 *          the weights, and padded rows are not stored (non-finite values: as antq_linear4).
 *   At most 64 KB of LDS per workgroup (64 output rows with the pair rule), the size every launch may have.
 * Checked before anything touches HIP, in this order:
 *   ANTQ_ERR_ARG          as antq_linear8
 *   ANTQ_OK, no launch    M == 0 or N == 0
 *   ANTQ_ERR_UNSUPPORTED  dtype == ANTQ_F32 (such layers stay with antq_linear8); M > ANTQ_LINEAR8_MM_MAX_M; K == 0 or
 *                         K % 8 != 0; the byte decoder's refusals; N >= 2^31 or K >= 2^31
 *   ANTQ_ERR_ALIGN        x_dev not 16-byte aligned, codes_dev not 8-byte aligned, y_dev / bias_dev not 2-byte aligned
 * Codes are read 16 bytes per lane when K % 16 == 0 and codes_dev is 16-byte aligned, 8 bytes per lane otherwise (the order
 * of the sum differs between the two, nothing else).  Measurements: profiles/packed_linear8_mm.md.
 * ------------------------------------------------------------------------- */
#define ANTQ_LINEAR8_MM_MAX_M 64
int antq_linear8_mm(const uint8_t *codes_dev, const void *x_dev, const void *bias_dev, void *y_dev,
                    size_t M, size_t N, size_t K,
                    const float *alpha_dev, int alpha_per_row, float gmax,
                    const float *grid_dev, int m, int n_normal,
                    unsigned flags /* 0 | ANTQ_FLAG_OVP */, int dtype /* BF16 | F16 */, void *stream);

/* -------------------------------------------------------------------------
 * OliVe's clip statistic on ONE read (replaces t.mean() + t.std() of olive_quantization/antquant/quant_modules.py:193-197
 * and :213-218, which read the tensor at least three times before the clip search reads it again).
 * antq_moments: sums_dev[2 r] = sum of x, sums_dev[2 r + 1] = sum of x^2 over row r (alpha_per_row) or over the whole
 *   tensor (one pair), in double, formed in one fixed order (bit-reproducible; no atomics).  workspace_dev: required for
 *   the whole-tensor form, antq_search_workspace_bytes() bytes.  These are also the numbers a row-sharded per-tensor
 *   quantiser all-reduces across ranks (sum x, sum x^2, n).
 * antq_xmax_3sigma: xmax_dev[r] = max(|mean + 3 std|, |mean - 3 std|) from na pairs of sums over n_per elements each,
 *   unbiased std, with the roundings of `dtype` applied where the reference's tensor ops round (fp32: mean and std to
 *   float; bf16 / fp16: mean, std, 3 * std, sum and difference each rounded to the tensor's dtype).  Agrees with the
 *   reference's torch reductions to their own summation-order noise (relative 1e-6 in fp32: measured against the exact
 *   two-pass statistic, profiles/reductions_exactness.md -- torch's mean / std composition is up to 6.0e-7 away from it,
 *   this entry point returned its bits in all 80 cases, up to 2^24 elements and |mean| = 7.5e6 std).
 * ------------------------------------------------------------------------- */
int antq_moments(const void *x_dev, size_t rows, size_t row_len, int alpha_per_row, int dtype,
                 double *sums_dev, void *workspace_dev, void *stream);
int antq_xmax_3sigma(const double *sums_dev, size_t na, size_t n_per, int dtype, float *xmax_dev, void *stream);

/* Plain device copy with the fake-quant kernels' access pattern (16 B per lane):
 * used by bench.py to measure the empirical HBM ceiling on the same buffers. */
int antq_copy(const void *src_dev, void *dst_dev, size_t bytes, void *stream);

/* Development / benchmark tuning knobs (thread-local: only the calling thread's later calls are affected; not part of
 * the stable surface):
 *   key 0: force the vectors per lane and task (U) of the row kernels -- batched launch 1..4, row-table encoder 2 / 4 / 8,
 *          calibration kernels 4 / 8 (0 = heuristic)
 *   key 1: number of persistent workgroups of antq_encode4's element encoder (0 = default, 2048)
 *   key 2: 0 disables the per-row (x-domain) table kernels, the d-domain kernels run instead (A/B measurements)
 *   key 3: 0 disables the binary-search path of antq_nearest (literal scan only)
 *   key 4: 0 makes the element encoder divide exactly instead of using the approximate-quotient decision
 *   key 5: 0 sends long rows through the per-row table kernels, 2 through the lane kernel in batches too (1 = the measured
 *          default: lane kernel for one-launch-per-tensor calls and fp32 batches)
 *   key 6: wavefronts per workgroup (1 / 2 / 4) of the batched row-table launch and of the one-launch lane kernel (0 = heuristic)
 *   key 7: vectors per lane of the one-launch lane kernel (0 = heuristic)
 *   key 8: workgroup -> task map rotation of the batched row-table launch: 0 per job (default), 1 always, 2 never
 *   key 9: 0 disables the 16-bit-domain row kernels and the 16-bit-domain encoder (bf16 / f16 rows of >= 128 vectors go back to
 *          the fp32-domain row table / row encoder)
 *   key 10: dynamic LDS bytes per workgroup of those kernels (occupancy A/B; -1 = default: 24 workgroups per CU)
 *   key 11: extra dynamic LDS bytes per workgroup of the batched lane-job kernels (occupancy A/B; -1 = default: fp32 static
 *           launches of >= 32768 workgroups are held at 6 workgroups = 24 wavefronts per CU, nothing otherwise)
 *   key 12: clip search: number of candidate-list chunks (0 = cost model)
 *   key 14: the histogram clip search of 16-bit tensors with one scale (antq_search_sse / _multi / antq_calibrate, no pair
 *           rule, or OliVe's pairs through a list of the outlier-capable pairs): 0 off, 1 (default) when the tensor is large
 *           enough for it to pay, 2 for every eligible tensor, 3 as 1 but never with the pair rule
 *   key 15: antq_calibrate with the abs-max statistic on a tensor the histogram search takes: 1 (default) the counting pass
 *           also finds the maximum (no separate abs-max pass), 0 the abs-max pass runs as everywhere else (A/B; same value)
 *   key 13: experiment switch of the kernel under development (0 = off; 1: the 16-bit-domain encoder's 8-vector tasks store
 *           their codes nontemporally instead of through the cache)
 *   key 16-18: the streaming row abs-max (16) and the ticket groups / workgroups of the one-launch reductions (17, 18), A/B
 *   key 19: the threshold-sweep clip search (round 6, first generation): 0 off, 1 (default) where it paid, 2 every eligible
 *           launch -- runs only where key 20 leaves a launch to it
 *   key 20: the sorted-row clip search (round 6: per-row searches from rows of 128 elements, OliVe's pair rule from 576, fp32
 *           tensors with one scale from 1 M elements): 0 off, 1 (default), 2 every eligible launch (rows from 128 elements
 *           with or without the pair rule, one-scale fp32 tensors from 4096)
 *   key 21: 0 sends rows of <= 1024 elements through the 4096-key kernel instead of one row per wavefront (A/B)
 *   key 22: antq_linear4_mm / antq_linear8_mm: tiles of 16 output rows per workgroup, 1 / 2 / 4 (A/B; 0 = the launcher's rule; no result changes)
 *   key 23: antq_linear4_gemm / antq_linear8_gemm: wavefronts per workgroup, 2 / 4, i.e. tiles of 128 / 256 rows of x (A/B; 0 = the launcher's rule:
 *           2 while the tiles of 128 rows number at most 256; no result changes) */
int antq_debug_set(int key, int value);

/* Load the library's GPU code objects for the current device now (HIP would load each of them at the first launch of one
 * of its kernels, ~50 ms in total, i.e. inside the first calibrating forward).  Launches nothing; idempotent. */
int antq_prefetch_kernels(void);

#ifdef __cplusplus
}
#endif
#endif /* ANTQ_H */
