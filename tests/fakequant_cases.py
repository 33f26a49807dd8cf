"""Input builders for the fp32 fake-quant edge tests (test_gpu_fakequant_edges.py) and for the host test that holds the
builders to their conditions with the CPU oracle alone (test_fakequant_cases_host.py).  What encode4_cases.py already has is
imported, not copied; new here: the wider book set, scales with short mantissas and at the edges of the approximate path's
scale range, windows at the bucket edges of a plan's table and where the straight-through step stops being exact, a dynamic
case whose scales are known before the launch, and the 16-bit patterns as short rows.  A builder takes numpy arrays, the
oracle module where it has to classify a value, and -- for the bucket edges -- the bytes of a plan's header."""
import functools

import numpy as np

import encode4_cases as ec
from encode4_cases import (ULPS, WIN, awkward_alpha, fuzz_case, lay_out, magnitude_case, pair_case, random_book,  # noqa: F401
                           threshold_case, ulp_window)

# ---------------------------------------------------------------------------------------------------------------------------
# 1: books
# ---------------------------------------------------------------------------------------------------------------------------
BOOKS_4BIT = ec.BOOK_NAMES
BOOKS_WIDE = ("int_b8_s", "int_b8_u", "flint_b8_s", "flint_b6_s", "float_b5_s", "olive_int_b8", "olive_flint_b8")
BOOK_NAMES = BOOKS_4BIT + BOOKS_WIDE
OLIVE_NAMES = ("olive_flint", "olive_int", "olive_flint_b8", "olive_int_b8")


@functools.lru_cache(maxsize=None)
def book(name):
    """(name, grid as the kernel takes it, gmax, n_normal, pair rule) like encode4_cases.book, for the wider set"""
    if name in BOOKS_4BIT:
        return ec.book(name)
    if name.startswith("olive_"):
        O = ec.golden("olive_grids.npz")
        gn, go = O["%s_b8_s" % name.split("_")[1]], O["outlier_b8_s"]
        return (name, np.ascontiguousarray(np.concatenate([gn, go]), np.float32), float(gn.max()), int(gn.size), True)
    g = np.ascontiguousarray(ec.golden("ant_grids.npz")[name], np.float32)
    return (name, g, float(g.max()), 0, False)


def n_scales_of(g):
    """64 scales for books of up to 6 bits, 16 for the 8-bit ones (255 x 33 elements per scale), 8 for the 8-bit OliVe books
    (509 entries: the oracle's scan is what a test of these spends its time on)"""
    return 64 if g.size <= 64 else 16 if g.size <= 256 else 8


# ---------------------------------------------------------------------------------------------------------------------------
# 2: scales
# ---------------------------------------------------------------------------------------------------------------------------
def alpha_for_scale(s, gmax):
    """An alpha with fl(alpha / gmax) == s in fp32 (searched among the floats next to fl(s * gmax)), or None"""
    s, gm = np.float32(s), np.float32(gmax)
    a0 = np.float32(np.float64(s) * np.float64(gm))
    for k in sorted(range(-4, 5), key=abs):
        a = ec.ulp_step(a0, k)
        if np.float32(a / gm) == s:
            return np.float32(a)
    return None


def short_mantissa_alphas(gmax):
    """alphas whose scale s = fl(alpha / gmax) is 2^e or 3 / 5 / 7 * 2^e: for such a scale some planted x has x / s exactly on
    a threshold (and the division is exact for many more)"""
    out = []
    for m, e in ((1, -7), (1, 0), (3, -9), (5, -6), (7, -4), (3, 1), (5, -13), (7, 2)):
        a = alpha_for_scale(np.float32(m * 2.0 ** e), gmax)
        if a is not None:
            out.append(a)
    return np.array(out, np.float32)


OK_EDGES = (2.0 ** -40, 2.0 ** 40)      # Scale::ok of the approximate-quotient paths: s in [2^-40, 2^40]


def ok_edge_alphas(gmax):
    """alphas for the floats at and next to s = 2^-40 and s = 2^40, each checked to give that s in fp32: the edge itself, the
    nearest float below and the nearest above that some alpha reaches (fl(alpha / gmax) skips some floats; within 4 ulps)"""
    out = []
    for edge in OK_EDGES:
        for side in (-1, 0, 1):
            for j in ((0,) if side == 0 else (1, 2, 3, 4)):
                a = alpha_for_scale(ec.ulp_step(np.float32(edge), side * j), gmax)
                if a is not None:
                    out.append(a)
                    break
    out = np.array(out, np.float32)
    return out[[1, 4, 0, 5, 2, 3]] if out.size == 6 else out          # (the two ends themselves first: a short draw takes both)


def scales_for(rng, gmax, n):
    """n alphas drawn in turn from awkward ones, the short-mantissa ones and the six around the ends of the approximate path's
    scale range: from 16 up all of the latter two are there, at least a quarter are awkward"""
    pools = [list(awkward_alpha(rng, max(n - 14, n // 4))), list(short_mantissa_alphas(gmax)), list(ok_edge_alphas(gmax))]
    out = []
    while len(out) < n:
        for p in pools:
            if p and len(out) < n:
                out.append(p.pop(0))
    return np.array(out, np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the plan header, bucket edges
# ---------------------------------------------------------------------------------------------------------------------------
# word offsets of csrc/antq_internal.h PlanHeader (32-bit words; the header is 128 bytes)
HDR_WORDS = dict(magic=0, version=1, kind=2, m=3, m_pad=4, shift=5, kmin=6, kmax=7, nb=8, keymask=9, nbneg=10, n_entries=11,
                 bytes=12, fastlim=13, lo_valid=14, hi_valid=15, xdom=16, xlim=17, vout=18, linear=19, lin_scale=20, lin_bias=21,
                 adom=22, atab_slots=23, hdom=24, h_nthr=25, h_nneg=26, hshift=27, tlist_off=28)
HDR_FLOATS = ("fastlim", "lo_valid", "hi_valid", "xlim", "vout", "lin_scale", "lin_bias")
HDR_SIGNED = ("kmin", "kmax")
PLAN_SCAN, PLAN_TABLE = 0, 1


def plan_header(host):
    """The named fields of a plan blob's header (host: the blob's bytes as a uint8 array, Plan.host)"""
    w = np.ascontiguousarray(host[:128]).view(np.uint32)
    h = {}
    for k, at in HDR_WORDS.items():
        h[k] = float(w[at:at + 1].view(np.float32)[0]) if k in HDR_FLOATS else int(w[at:at + 1].view(np.int32)[0]) if k in HDR_SIGNED else int(w[at])
    return h


def bucket_edges(h):
    """The d-domain values at which the table's bucket number changes (float32, both signs where the table has a negative
    half): for a keyed plan the floats whose bits are k << shift, kmin < k <= kmax; for a linear plan (k - lin_bias) /
    lin_scale, 0 < k <= kmax.  A scan plan has none."""
    if h["kind"] != PLAN_TABLE:
        return np.zeros(0, np.float32)
    if h["linear"]:
        k = np.arange(1, h["kmax"] + 1, dtype=np.float64)
        with np.errstate(all="ignore"):
            e = ((k - h["lin_bias"]) / h["lin_scale"]).astype(np.float32)
        return e[np.isfinite(e) & (e != 0)]
    k = np.arange(h["kmin"] + 1, h["kmax"] + 1, dtype=np.int64)
    bits = k << h["shift"]
    bits = bits[(bits > 0x00800000) & (bits < 0x7f800000)]
    e = bits.astype(np.uint32).view(np.float32)
    return np.concatenate([-e[::-1], e]) if h["nbneg"] else e


MAX_EDGE_WINDOWS = 4096
STE_FAR_D = 60000.0                 # far end of the search for a straight-through edge: inside the scan's horizon of 102400
TINY = np.float32(2.0 ** -120)      # centres below it (denormal windows) are left out


def edge_centres(h, g, scale):
    """fl(e * scale) for every bucket edge e and for fl(xlim * scale), where the kernels switch the arithmetic of the
    straight-through step; zeros, denormals and overflows left out"""
    g = np.asarray(g, np.float32)
    c = [bucket_edges(h).astype(np.float64)]
    if h["kind"] == PLAN_TABLE and np.isfinite(h["xlim"]) and h["xlim"] > 0:
        c.append(np.float64([h["xlim"]] + ([-h["xlim"]] if g.min() < 0 else [])))
    with np.errstate(all="ignore"):
        x = (np.concatenate(c) * float(scale)).astype(np.float32)
    return x[np.isfinite(x) & (np.abs(x) >= TINY)]


def outer_centres_d(g):
    """+2 * (largest value) and, for a book with negative values, 2 * (the most negative one), in the d domain"""
    g = np.asarray(g, np.float64)
    return np.float64([2 * g.max()] + ([2 * g.min()] if g.min() < 0 else []))


def outer_centres_x(g, scale):
    with np.errstate(all="ignore"):
        c = (outer_centres_d(g) * float(scale)).astype(np.float32)
    return c[np.isfinite(c) & (np.abs(c) >= TINY)]


def _output_is_qs(oracle, x, alpha, g, gmax):
    """Per element: is the oracle's output fl(q * s), q the value of its index (0 without one), s its row's scale?  Pair rule off."""
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        out, ridx = oracle.forward(x, alpha, g, gmax, False)
        s = (np.asarray(alpha, np.float32).reshape(-1) / np.float32(gmax)).astype(np.float32)
        q = np.where(ridx >= 0, g[np.clip(ridx, 0, g.size - 1)], np.float32(0)).astype(np.float32)
        qs = (q * s[:, None]).astype(np.float32)
    return out.view(np.uint32) == qs.view(np.uint32)


def ste_edges(oracle, alpha, g, gmax, sign):
    """Per scale the first float beyond sign * 2 * (outermost value) * s found by bisection on the bit pattern at which the
    oracle's output stops being fl(q * s): (q - d) + d is q while q is a multiple of d's ulp and, for these books, well past
    |d| = 2 |q|, where the kernels stop relying on it (xlim).  NaN for a scale without such a float between 2 |q| s and
    2^30 times that (zero, huge or tiny scales)."""
    alpha = np.asarray(alpha, np.float32).reshape(-1)
    v = float(np.max(g)) if sign > 0 else float(np.min(g))
    with np.errstate(all="ignore"):
        s = (alpha / np.float32(gmax)).astype(np.float32)
        lo_f = np.abs(2.0 * v * s.astype(np.float64)).astype(np.float32)
        hi_f = np.abs(STE_FAR_D * s.astype(np.float64)).astype(np.float32)
    ok = np.isfinite(hi_f) & (lo_f >= TINY) & np.isfinite(lo_f)
    lo, hi = lo_f.view(np.uint32).astype(np.int64), hi_f.view(np.uint32).astype(np.int64)
    lo, hi = np.where(ok, lo, 0x3f800000), np.where(ok, hi, 0x3f800000)

    def eq(bits):
        x = (bits.astype(np.uint32).view(np.float32) * np.float32(sign)).reshape(-1, 1)
        return _output_is_qs(oracle, np.concatenate([x, x]), np.concatenate([alpha, alpha]), g, gmax)[:alpha.size, 0]

    ok &= eq(lo) & ~eq(hi)
    for _ in range(32):
        mid = (lo + hi) // 2
        e = eq(mid)
        lo, hi = np.where(e, mid, lo), np.where(e, hi, mid)
    ok &= (hi - lo == 1)
    return np.where(ok, hi.astype(np.uint32).view(np.float32) * np.float32(sign), np.float32(np.nan)).astype(np.float32)


def edges_case(oracle, rng, bk, h, row_len, n_scales=None, alpha=None, below=None):
    """The fp32 decision edges of one book in rows of row_len: per scale the +/-16-ulp windows around every threshold
    (encode4_cases.centres), around +/-2 * (outermost value) * s, around every bucket edge of the plan's table and around
    fl(xlim * s), in random order, Gaussian data around them (lay_out).  Scales: scales_for, or `alpha`.  below: one magnitude
    per scale; windows that reach it are left out (the dynamic case: nothing may exceed the row's abs-max).  Also windows
    around ste_edges, where (q - d) + d really stops being q.  Returns dict(x, alpha, windows, outer, ste): [n, WIN] flat
    indices of the elements of the threshold windows / the 2 * outermost windows / the ste_edges windows."""
    _, g, gmax, nn, ovp = bk
    n_scales = n_scales_of(g) if n_scales is None else n_scales
    alpha = scales_for(rng, gmax, n_scales) if alpha is None else np.asarray(alpha, np.float32)
    scale = (alpha / np.float32(gmax)).astype(np.float32)
    unsigned = bool(g.min() >= 0)
    payloads, n_thr, n_out, n_ste = [], [], [], []
    ste_pos = ste_edges(oracle, alpha, g, gmax, 1)
    ste_neg = ste_edges(oracle, alpha, g, gmax, -1) if not unsigned else np.full(alpha.size, np.nan, np.float32)
    edge_budget = max(4, MAX_EDGE_WINDOWS // max(1, bucket_edges(h).size + 4))
    for i, s in enumerate(scale):
        with np.errstate(all="ignore"):
            c, _ = ec.centres(g, s)
            c = c[np.isfinite(c) & (np.abs(c) >= TINY)]
            outer = outer_centres_x(g, s)
            e = edge_centres(h, g, s) if i < edge_budget else np.zeros(0, np.float32)
        ste = np.float32([v for v in (ste_pos[i], ste_neg[i]) if np.isfinite(v)])
        if unsigned:
            e = e[e > 0]
        if below is not None:
            c, outer, e, ste = (v[np.abs(v) * np.float32(1.0001) < below[i]] for v in (c, outer, e, ste))
        parts = [ulp_window(v) for v in c[rng.permutation(c.size)]] + [ulp_window(v) for v in outer] + [ulp_window(v) for v in ste]
        parts += [ulp_window(v) for v in e[rng.permutation(e.size)]]
        payloads.append(np.concatenate(parts).astype(np.float32) if parts else np.zeros(8, np.float32))
        n_thr.append(c.size)
        n_out.append(outer.size)
        n_ste.append(ste.size)
    x, a_rows, starts = lay_out(rng, payloads, alpha, row_len, alpha / 3, unsigned=unsigned)
    win = np.arange(WIN)
    windows = [starts[i] + WIN * k + win for i in range(len(payloads)) for k in range(n_thr[i])]
    outer = [starts[i] + WIN * (n_thr[i] + k) + win for i in range(len(payloads)) for k in range(n_out[i])]
    ste = [starts[i] + WIN * (n_thr[i] + n_out[i] + k) + win for i in range(len(payloads)) for k in range(n_ste[i])]
    return dict(x=x, alpha=a_rows, **{k: np.array(v, np.int64).reshape(-1, WIN) for k, v in (("windows", windows), ("outer", outer), ("ste", ste))})


def windows_straddle(oracle, case, g, gmax, which="windows"):
    """(windows that hold at least two different oracle indices, windows) with the pair rule off: the bare decisions"""
    with np.errstate(all="ignore"):
        _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, False)
    v = ridx.reshape(-1)[case[which]]
    return int((v.max(1) != v.min(1)).sum()), int(v.shape[0])


def windows_mixed(oracle, case, g, gmax, which="ste"):
    """(windows of case[which] that hold both an element whose oracle output is fl(q * s) and one whose output is not, windows)"""
    same = _output_is_qs(oracle, case["x"], case["alpha"], g, gmax).reshape(-1)[case[which]]
    return int((same.any(1) & ~same.all(1)).sum()), int(same.shape[0])


# ---------------------------------------------------------------------------------------------------------------------------
# shapes (fp32; vectors per row = row_len / 4)
# ---------------------------------------------------------------------------------------------------------------------------
ROW_LENS = (16, 12, 20, 72, 508, 512, 516, 576, 768, 1024, 1028, 4004)
PER_TENSOR_SHAPES = ((8, 72), (1, 4099))
RAGGED_ROW_LENS = (147, 27)
PAIR_ROW_LENS = (16, 72, 512, 1024)     # (pair_case lays whole octets out: multiples of 8)
DYN_VPR = (4, 64, 128, 192, 256, 512, 513, 1024, 2048, 2049, 4096, 8192)
DYN_RATIOS = (1.0, float(np.float32(0.3141)))
SEED = 20240


def dyn_rows(vpr):
    return 9 if vpr <= 256 else 5 if vpr <= 1024 else 3


def static_case(oracle, name, h, row_len):
    """The static edge case of (book, row length); deterministic"""
    return edges_case(oracle, np.random.default_rng(SEED + row_len), book(name), h, row_len)


def per_tensor_cases(oracle, name, h):
    """Three scales (an awkward one, a short-mantissa one, s = 2^-40), each with the edge case of one scale laid out in rows of 72
    and of 4099 elements: the per-tensor tensors are cut from these.  [(alpha, case of 72, case of 4099)]"""
    bk = book(name)
    rng = np.random.default_rng(SEED + 1)
    return [(a, edges_case(oracle, rng, bk, h, 72, alpha=[a]), edges_case(oracle, rng, bk, h, 4099, alpha=[a])) for a in scales_for(rng, bk[2], 3)]


def dynamic_case(oracle, name, h, vpr, ratio):
    """Rows of vpr vectors for the in-kernel abs-max forms, dyn_rows(vpr) scales: the windows of edges_case that lie below the
    row's abs-max, every other element below it too, and one element per row (random column and sign) that IS the abs-max m,
    with alpha = fl(m * ratio).  So the scales are known before the launch: case["alpha"], which the host test holds to
    oracle.absmax(x, True, ratio).  (With ratio 1 nothing of a row lies beyond gmax * s; the smaller ratio brings the clipped
    region and the 2 * outermost windows in.)"""
    bk = book(name)
    _, g, gmax, nn, ovp = bk
    rng = np.random.default_rng(SEED + 7 * vpr + int(ratio * 1000))
    n = dyn_rows(vpr)
    target = np.concatenate([awkward_alpha(rng, n - 2), short_mantissa_alphas(gmax)[1:3]])[:n]
    r32 = np.float32(ratio)
    m = (target.astype(np.float64) / float(r32)).astype(np.float32)
    alpha = (m * r32).astype(np.float32)
    case = edges_case(oracle, rng, bk, h, 4 * vpr, alpha=alpha, below=m)
    x = case["x"]
    rows = x.shape[0]
    m_rows = np.repeat(m, rows // n)
    over = np.abs(x) >= m_rows[:, None]
    x[over] *= np.float32(0.25)
    assert (np.abs(x) < m_rows[:, None]).all()
    sign = np.ones(rows, np.float32) if g.min() >= 0 else np.where(rng.random(rows) < 0.5, -1.0, 1.0).astype(np.float32)
    x[np.arange(rows), rng.integers(0, x.shape[1], rows)] = m_rows * sign
    case.update(absmax=m_rows, ratio=float(r32))
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# the 16-bit patterns as short rows
# ---------------------------------------------------------------------------------------------------------------------------
PATTERN_ROW_SCALES = np.float32([1.0, 0.06, 0.0, -0.05, np.nan, 1e-30, 65504.0, 0.37])


def pattern_rows(row_len, shuffled_rng=None):
    """All 65 536 16-bit patterns once per row scale as rows of row_len (the last row of every scale padded with zeros):
    (patterns uint16 [rows, row_len], alpha float32 [rows]) -- eight row scales, each repeated over its rows"""
    pats = np.arange(65536, dtype=np.uint16)
    if shuffled_rng is not None:
        pats = shuffled_rng.permutation(pats)
    rps = -(-65536 // row_len)
    x = np.zeros((PATTERN_ROW_SCALES.size, rps * row_len), np.uint16)
    x[:, :65536] = pats
    return x.reshape(-1, row_len), np.repeat(PATTERN_ROW_SCALES, rps)


def widen16(oracle, x16, dtype_name):
    return oracle.bf16_to_f32(x16) if dtype_name == "bfloat16" else x16.view(np.float16).astype(np.float32)


def round16(oracle, f, dtype_name):
    """The oracle's fp32 sequence rounded once to the 16-bit type: uint16 patterns"""
    if dtype_name == "bfloat16":
        return oracle.f32_to_bf16(f)
    with np.errstate(all="ignore"):
        return np.asarray(f, np.float32).astype(np.float16).view(np.uint16)
