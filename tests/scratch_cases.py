"""Cases of the scratch / output contract tests (test_gpu_scratch_contracts.py), built with numpy alone and held to their
premises by test_scratch_cases_host.py.

include/antq.h promises that the workspaces of the calibration and reduction entry points are scratch: "no initialisation",
a stated size, outputs that "need not be initialised".  The GPU tests put every workspace and every output between guard
bands, fill the workspace with patterns a kernel would trip over if it trusted them, and compare bits.  This module holds
  * the slab layout (guards, alignment) and the patterns, with what each pattern reads as in the widths the layouts use;
  * the workspace layouts restated from the sources (each constant names its source line);
  * the cases: for every one-scale search path the smallest shape that takes it, with the eligibility rule it claims;
  * the tensors of the histogram search's flag test and the header's rule for "outlier-capable pairs", in numpy.

Nothing here imports the HIP library."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# slabs and patterns
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 4096                 # bytes on either side: a condition (wider than any single partial record), not a measurement
GUARD_BYTE = 0xC3
OUTPUT_FILL = 0xFF           # what every output buffer holds before a call
PATTERNS = (0x00, 0xFF, 0x7F, "leftover")     # 0x00 is the baseline every other pattern is compared with
# the widest record one thread writes to a workspace: a workgroup's kPtCand doubles (antq_k_search.h: `part`)
WIDEST_RECORD = 128 * 8


def slab_layout(base_addr, nbytes):
    """(offset of the inner region, total bytes) of a slab allocated at base_addr.  The allocation is exactly
    GUARD + nbytes + GUARD bytes; the inner region starts on a 256-byte boundary, which a 256-byte aligned allocation gives
    because GUARD is a multiple of 256 (asserted: a base that is not makes the slab unusable, it is not silently shifted)."""
    assert GUARD % 256 == 0 and GUARD > WIDEST_RECORD
    assert base_addr % 256 == 0, "device allocations are expected on 256-byte boundaries"
    assert (base_addr + GUARD) % 256 == 0 and (base_addr + GUARD) % 16 == 0
    return GUARD, GUARD + int(nbytes) + GUARD


def pattern_reads_as(byte):
    """What a buffer filled with `byte` holds in the widths the workspace layouts use: (float32, float64, uint32)"""
    b4, b8 = bytes([byte]) * 4, bytes([byte]) * 8
    return (np.frombuffer(b4, np.float32)[0], np.frombuffer(b8, np.float64)[0], int(np.frombuffer(b4, np.uint32)[0]))


# ---------------------------------------------------------------------------------------------------------------------
# workspace layouts, restated
# ---------------------------------------------------------------------------------------------------------------------
K_WS_SLOTS = 8192            # antq_k_search.h kWsSlots: workgroup partials the per-tensor workspace holds
K_PT_CAND = 128              # antq_k_search.h kPtCand: doubles per partial (also antq_k_aux.h kPartialStride)
K_MAX_TYPES = 4              # antq_k_search.h kMaxTypes: codebooks of one single-read search
PARTIAL_CAP = 1024           # antq_kernels.hip launch_moments / launch_alpha_grad: workgroups of a per-tensor sum
K_SWEEP_MAX_CAND = 128       # antq_k_sweep.h kSweepMaxCand
# antq_k_hist.h
HIST_BINS = 32768
HIST_MAX_G = 128
HIST_SEG_CAP = 1024
HIST_SLABS = 2 * HIST_MAX_G * HIST_BINS * 4
HIST_COUNT_OFF = HIST_SLABS
HIST_SEG_COUNT_OFF = HIST_COUNT_OFF + 2 * HIST_BINS * 4
HIST_FLAGS_OFF = HIST_SEG_COUNT_OFF + HIST_MAX_G * 16 * 4
HIST_SEG_OFF = HIST_FLAGS_OFF + 256
HIST_LIST_OFF = HIST_SEG_OFF + HIST_MAX_G * 16 * HIST_SEG_CAP * 4
HIST_WS_BYTES = HIST_LIST_OFF + HIST_MAX_G * 16 * HIST_SEG_CAP * 4
SEARCH_WS_BYTES = max(K_WS_SLOTS * K_PT_CAND * 8, HIST_WS_BYTES)      # antq_search_workspace_bytes()
# antq_k_reduce.h: the ticket block
REDUCE_WS_BYTES = 65536
TK_COUNTER_BYTES = 8320      # kTkCounterBytes: the launch counter and 64 group counters, 128 bytes apart
TK_PARTIAL_OFF = 16384       # kTkPartialOffset: <= 1024 workgroup partials of 16 bytes
TK_GROUP_OFF = 16384 + 16384 + 8192          # kTkGroupOffset: <= 64 group partials of 16 bytes

XMAX_GIVEN, XMAX_ABSMAX, XMAX_3SIGMA = 0, 1, 2
ERR_ARG, ERR_UNSUPPORTED = -1, -2
FLAG_OVP = 1
DTYPE_CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
ESIZE = {"float32": 4, "bfloat16": 2, "float16": 2}
EPL = {"float32": 4, "bfloat16": 8, "float16": 8}


def up256(v):
    return (int(v) + 255) & ~255


def calib_ncand(lb, ub, step):
    return (ub - lb + step - 1) // step if (step > 0 and ub > lb) else 0


def calibrate_regions(na, ncand, ntypes):
    """The five regions calib_layout (csrc/antq_search.hip) cuts the workspace of antq_calibrate into: [(name, bytes)]"""
    c = max(ncand, 1)
    return [("search", up256(SEARCH_WS_BYTES)), ("ratios", up256(c * 4)), ("sse", up256(ntypes * c * na * 8)),
            ("best", up256(ntypes * na * 4)), ("sums", up256(2 * na * 8))]


def calibrate_workspace_bytes(rows, per_row, lb, ub, step, ntypes):
    return sum(b for _, b in calibrate_regions(rows if per_row else 1, calib_ncand(lb, ub, step), ntypes))


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def ratios_of(lo, hi, step):
    return np.asarray([np.float32(i * 0.01) for i in range(int(lo), int(hi), int(step))], dtype=np.float32)


SHORT_RATIOS = ratios_of(80, 150, 10)          # 7 candidates: the searches' list where the case does not need a longer one
OLIVE_SHORT_RATIOS = ratios_of(80, 250, 40)    # 5 candidates


def gauss(n, seed, scale=0.03):
    return (np.random.default_rng(seed).standard_normal(n, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def laplace_outliers(n, seed):
    """The recipe of the sorted-search tests: small values with one element in 300 blown up 8 .. 64 times"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n, dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    idx = rng.integers(0, n, max(1, n // 300))
    x[idx] *= rng.uniform(8, 64, idx.size).astype(np.float32)
    return x


def three_sigma_f32(x):
    """A clip statistic of the 3-sigma kind for a GIVEN-statistic case (an input of the search, not a thing under test)"""
    m, s = np.float64(x.mean(dtype=np.float64)), np.float64(x.std(dtype=np.float64, ddof=1))
    return np.float32(max(abs(m + 3 * s), abs(m - 3 * s)))


# ---------------------------------------------------------------------------------------------------------------------
# one-scale searches: (name, path, dtype, n, form, knobs, ovp, family, ratios, kind of data)
#   path   "direct" | "sorted" | "sweep" | "hist"
#   form   how ONE scale is asked for: "flat" rows = 1, per_row = 0; "folded" 4 rows, per_row = 0; "one_row" rows = 1, per_row = 1
#   knobs  {key: value} of antq_debug_set; 19 sweep, 20 sorted search, 14 histogram (0 off, 1 default rule, 2 every eligible
#          launch), 12 the candidate-list split of the direct kernels (0 = cost model)
# ---------------------------------------------------------------------------------------------------------------------
DIRECT_KNOBS = {19: 0, 20: 0, 14: 0}
CLAMP_CHUNKS = 64                              # knob 12 of the clamp case: the candidate list in 64 chunks of one
CLAMP_RATIOS = ratios_of(75, 139, 1)           # 64 candidates
# fp32 rows of >= 512 vectors take 8 vectors per lane and task (launch_search: U), 16-bit ones 4: elements per task
TASK_ELEMS = {"float32": 64 * 8 * 4, "bfloat16": 64 * 4 * 8, "float16": 64 * 4 * 8}


def direct_blocks(dtype, n, chunks):
    """(workgroups asked for, workgroups after the clamp) of the direct per-tensor kernel (search_grid, pt): one task per
    wavefront, four per workgroup, at most 1024 workgroups, clamped to kWsSlots / chunks partial slots"""
    tasks = (n // EPL[dtype] + TASK_ELEMS[dtype] // EPL[dtype] - 1) // (TASK_ELEMS[dtype] // EPL[dtype])
    asked = min((tasks + 3) // 4, 1024)
    return asked, min(asked, K_WS_SLOTS // chunks)


CLAMP_N = (K_WS_SLOTS // CLAMP_CHUNKS * 4 + 9) * TASK_ELEMS["float32"]      # 130 workgroups' worth of tasks against 128 slots

SEARCH_CASES = [
    dict(name="direct fp32 8192", path="direct", dtype="float32", n=8192, form="flat", knobs=DIRECT_KNOBS, ovp=False,
         family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="direct bf16 8192", path="direct", dtype="bfloat16", n=8192, form="folded", knobs=DIRECT_KNOBS, ovp=False,
         family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="direct fp32 clamp binds", path="direct", dtype="float32", n=CLAMP_N, form="one_row",
         knobs={19: 0, 20: 0, 14: 0, 12: CLAMP_CHUNKS}, ovp=False, family="ant1", ratios=CLAMP_RATIOS, data="gauss"),
    dict(name="sorted fp32 4096 forced", path="sorted", dtype="float32", n=4096, form="flat", knobs={19: 1, 20: 2, 14: 1},
         ovp=False, family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="sorted fp32 2^20 default", path="sorted", dtype="float32", n=1 << 20, form="folded", knobs={19: 1, 20: 1, 14: 1},
         ovp=False, family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="sweep fp32 16384 forced", path="sweep", dtype="float32", n=16384, form="one_row", knobs={19: 2, 20: 0, 14: 1},
         ovp=False, family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="sweep fp32 2^22 default", path="sweep", dtype="float32", n=1 << 22, form="flat", knobs={19: 1, 20: 0, 14: 1},
         ovp=False, family="ant1", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="hist bf16 2^19", path="hist", dtype="bfloat16", n=1 << 19, form="flat", knobs={19: 1, 20: 1, 14: 1},
         ovp=False, family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="hist f16 2^19", path="hist", dtype="float16", n=1 << 19, form="folded", knobs={19: 1, 20: 1, 14: 1},
         ovp=False, family="ant", ratios=SHORT_RATIOS, data="gauss"),
    dict(name="hist bf16 2^20 pairs", path="hist", dtype="bfloat16", n=1 << 20, form="one_row", knobs={19: 1, 20: 1, 14: 2},
         ovp=True, family="olive", ratios=OLIVE_SHORT_RATIOS, data="laplace"),
    dict(name="hist f16 2^20 pairs", path="hist", dtype="float16", n=1 << 20, form="flat", knobs={19: 1, 20: 1, 14: 2},
         ovp=True, family="olive", ratios=OLIVE_SHORT_RATIOS, data="laplace"),
]
# antq_search_sse_multi on the one-scale paths: (case it borrows shape, data and knobs from, codebooks)
MULTI_CASES = [(c, nt) for c in ("direct fp32 8192", "sorted fp32 4096 forced", "sweep fp32 16384 forced", "hist bf16 2^19")
               for nt in (2, 4)]
ANT_TYPES = {"ant": ("int", "flint"), "ant1": ("int",), 2: ("int", "flint"), 4: ("int", "pot", "flint", "float")}


def search_case(name):
    return next(c for c in SEARCH_CASES if c["name"] == name)


def case_rows(case):
    """(rows, row_len, per_row) of the call"""
    n = case["n"]
    return {"flat": (1, n, 0), "folded": (4, n // 4, 0), "one_row": (1, n, 1)}[case["form"]]


def case_data(case, seed=0):
    """(x float32 [n], clip statistic float32) of a search case; 16-bit cases are rounded by the caller"""
    n = case["n"]
    sd = 9100 + seed + sum(map(ord, case["name"]))
    if case["data"] == "gauss":
        x = gauss(n, sd)
        return x, np.float32(np.abs(x).max())
    x = laplace_outliers(n, sd)
    return x, three_sigma_f32(x)


def eligible(case, ncand=None, ntypes=1):
    """The rule of include/antq.h / csrc/antq_search.hip the case claims for its path, on the inner start of a slab (16-byte
    aligned).  Returns (takes the path, would still take it one step smaller)."""
    n, dt, k = case["n"], case["dtype"], case["knobs"]
    ncand = len(case["ratios"]) if ncand is None else ncand
    aligned = (slab_layout(0, n * ESIZE[dt])[0]) % 16 == 0

    def rule(n):
        if case["path"] == "sorted":           # sort_pt_shape_ok: fp32, whole vectors, 2^20 (4096 forced)
            return dt == "float32" and k[20] in (1, 2) and aligned and n % 4 == 0 and n >= (4096 if k[20] == 2 else 1 << 20)
        if case["path"] == "sweep":            # sweep_pt_shape_ok: fp32, sorted search off, 2^22 (16384 forced)
            return (dt == "float32" and k[20] == 0 and k[19] in (1, 2) and aligned and n % 4 == 0 and 1 <= ncand <= K_SWEEP_MAX_CAND
                    and n >= (16384 if k[19] == 2 else 1 << 22))
        if case["path"] == "hist":             # hist_eligible: 16-bit, whole vectors, 2^19 (2^20 and enough work with pairs)
            if dt == "float32" or k[14] == 0 or not aligned or n % 8 != 0 or n >= 1 << 31:
                return False
            if k[14] == 2:
                return True
            return (n >= 1 << 20 and n * ncand * ntypes >= 1.5e8) if case["ovp"] else n >= 1 << 19
        # direct: no front path takes the launch
        return k[19] == 0 and k[20] == 0 and (dt == "float32" or k[14] == 0) and aligned and n % EPL[dt] == 0

    return rule(n), rule(n - EPL[dt])


# ---------------------------------------------------------------------------------------------------------------------
# the histogram search's flag word: a tensor whose pair list overflows, and a clean one
# ---------------------------------------------------------------------------------------------------------------------
FLAG_N = 1 << 20
FLAG_RATIOS = OLIVE_SHORT_RATIOS
HEADER_PAIR_BOUND = 0.08           # include/antq.h: "a tensor with too many such pairs (> ~8 %)"


def flag_tensors():
    """{"overflow": (x, statistic), "clean": (x, statistic)}: float32 values for a bf16 tensor of FLAG_N elements.  overflow:
    the recipe of test_histogram_clip_search_with_outlier_victim_pairs -- gaussian data against a statistic below ONE sigma, so
    that most pairs hold an outlier-capable element; clean: the 3-sigma statistic of data with one large element in 300."""
    over = gauss(FLAG_N, 9301, 0.05)
    clean = laplace_outliers(FLAG_N, 9302)
    return {"overflow": (over, np.float32(0.03)), "clean": (clean, three_sigma_f32(clean))}


def outlier_threshold_over_gmax(grid_with_outliers, n_normal, gmax):
    """hist_outlier_bound: the smallest decision threshold between a normal value and an outlier, in units of gmax, times
    0.999 (the thresholds of the scan are the midpoints of adjacent values)"""
    g = np.asarray(grid_with_outliers, np.float64)
    is_out = np.arange(g.size) >= n_normal
    order = np.argsort(g, kind="stable")
    v, o = g[order], is_out[order]
    mids = [(v[i] + v[i + 1]) / 2 for i in range(v.size - 1) if o[i] != o[i + 1] and v[i] != v[i + 1]]
    return np.float32(min(abs(m) for m in mids) / gmax * 0.999)


def pair_fraction(x_image, statistic, ratios, tmin_over_gmax):
    """Fraction of the flat pairs (2k, 2k + 1) that k_hist16 lists: the larger magnitude of the pair at or above
    statistic * min(ratios) * tmin_over_gmax (antq_k_hist.h: theta; the comparison is made on 16-bit patterns rounded DOWN
    from that bound, which the float comparison here brackets from above)"""
    theta = np.float32(statistic) * np.float32(np.min(ratios)) * np.float32(tmin_over_gmax)
    a = np.abs(np.asarray(x_image, np.float32)).reshape(-1, 2).max(axis=1)
    return float((a >= theta).mean())


def segment_capacity_fraction(n):
    """The fraction of listed pairs at which a wavefront's segment of kHistSegCap words overflows: a tensor of n 16-bit
    elements is n / 2 pair words spread over G workgroups of 16 wavefronts (launch_hist_search: G)"""
    G = min(max(n // 65536, 16), HIST_MAX_G)
    G = (G + 7) & ~7
    return HIST_SEG_CAP / ((n / 2) / (G * 16))


# ---------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------
def sum_sizes(op, dtype):
    """[n]: one workgroup, and more workgroups than the partial cap (launch_moments: 64 * EPL * 4 elements per wavefront,
    launch_alpha_grad: 64 * EPL * 2; four wavefronts per workgroup; at most PARTIAL_CAP workgroups), with a ragged tail"""
    per = 64 * EPL[dtype] * (4 if op == "moments" else 2) * 4
    return [per - 3, (PARTIAL_CAP + 1) * per + per // 2 + 3]


def sum_blocks(op, dtype, n):
    per = 64 * EPL[dtype] * (4 if op == "moments" else 2) * 4
    return (n + per - 1) // per


# (workgroups, workgroups per group) of the ticket tests: knobs 18 / 17; None = the launcher's defaults
TICKET_SETTINGS = [None, (1024, 64), (1024, 16), (64, 1)]
TICKET_SIZES = [1, 1000, (1 << 22) + 4099]      # one element, one workgroup, enough for 1024 workgroups in both reductions


# ---------------------------------------------------------------------------------------------------------------------
# antq_calibrate / antq_calibrate_batch
#   (name, dtype, rows, row_len, per_row, xmax mode, ntypes, (lb, ub, step), path of its searches)
# The full cross of the issue's factors -- dtype x shape x statistic mode x type count x candidate range, 162 cases -- plus the
# bf16 one-scale abs-max tensor of 2^19 elements, where the counting pass of the histogram search delivers the abs-max.
# ---------------------------------------------------------------------------------------------------------------------
FULL, ONE, EMPTY = (75, 150, 1), (100, 101, 1), (150, 150, 1)
RANGES = {"full": FULL, "one candidate": ONE, "empty": EMPTY}
MODES = {"given": XMAX_GIVEN, "absmax": XMAX_ABSMAX, "3sigma": XMAX_3SIGMA}
SHAPES = {"3x256": (3, 256, 1), "257x128": (257, 128, 1), "one scale 4096": (4, 1024, 0)}       # (rows, row_len, per_row)


def _calib_cases():
    out = []
    for dt, short in (("float32", "fp32"), ("bfloat16", "bf16")):
        for sname, (rows, K, per_row) in SHAPES.items():
            for mname, mode in MODES.items():
                for nt in (1, 3, 5):
                    for rname, rng in RANGES.items():
                        r, k = (1, rows * K) if (not per_row and mode != XMAX_ABSMAX) else (rows, K)   # (one scale: flat and folded)
                        path = "none" if rname == "empty" else ("sorted" if per_row else "direct")
                        out.append(dict(name="%s %s %s %d types %s" % (short, sname, mname, nt, rname), dtype=dt, rows=r, row_len=k,
                                        per_row=per_row, mode=mode, ntypes=nt, rng=rng, path=path))
    out.append(dict(name="bf16 one scale 2^19 absmax 3 types", dtype="bfloat16", rows=1, row_len=1 << 19, per_row=0, mode=XMAX_ABSMAX,
                    ntypes=3, rng=(75, 150, 15), path="hist"))
    return out


CALIB_CASES = _calib_cases()
CALIB_TYPES = ("int", "pot", "flint", "float", "int")        # the fifth codebook repeats the first: a tie the first must win
# six jobs of mixed shape, statistic, type count and range for antq_calibrate_batch (one dtype per batch), and two orders
BATCH_JOBS = ["fp32 3x256 absmax 3 types full", "fp32 257x128 absmax 1 types empty", "fp32 one scale 4096 absmax 5 types full",
              "fp32 257x128 3sigma 5 types full", "fp32 3x256 given 1 types one candidate", "fp32 one scale 4096 3sigma 1 types full"]
SMALLEST_CALIB = ("fp32 3x256 given 1 types one candidate", "bf16 one scale 4096 given 1 types one candidate")   # the smallest needs
BATCH_ORDERS = [(0, 1, 2, 3, 4, 5), (3, 5, 2, 0, 4, 1)]


def calib_case(name):
    return next(c for c in CALIB_CASES if c["name"] == name)


def calib_data(case):
    """x float32 [rows, row_len] and, for XMAX_GIVEN, the statistic float32 [na]"""
    rows, K = case["rows"], case["row_len"]
    x = gauss(rows * K, 9500 + sum(map(ord, case["name"]))).reshape(rows, K)
    x[::3] *= np.float32(0.2)
    if case["mode"] == XMAX_3SIGMA:
        x += np.float32(0.004)
    given = None
    if case["mode"] == XMAX_GIVEN:
        given = (np.abs(x).max(axis=1) if case["per_row"] else np.abs(x).max(keepdims=True).reshape(1)).astype(np.float32)
        given = (given * np.float32(0.9)).astype(np.float32)
    return x, given


def xmax_in_hist(case):
    """antq_calibrate: the counting pass of the histogram search delivers the abs-max (one scale, 16-bit, abs-max, no pair
    rule, candidates, the histogram's default rule: 2^19 elements in whole vectors)"""
    n = case["rows"] * case["row_len"]
    return (not case["per_row"] and case["dtype"] != "float32" and case["mode"] == XMAX_ABSMAX and calib_ncand(*case["rng"]) > 0
            and n % 8 == 0 and n >= 1 << 19)
