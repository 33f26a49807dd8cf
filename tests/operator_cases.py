"""Input builders for the edge tests of the kernels that replace the reference's operators one for one
(test_gpu_operator_edges.py): antq_nearest (fp32 and float64), antq_nearest_plan / antq_nearest_hinted, antq_affine and
antq_fakequant_f64; and for the host test that holds the builders to their conditions with the CPU oracle alone
(test_operator_cases_host.py).  What encode4_cases.py and fakequant_cases.py already have is imported, not copied.  Nothing
here touches the HIP library.  A builder may use a kernel's documented formulas (fastlim of k_nearest_fast, a plan header's
fields, the affine quantiser's scale and zero point) to PLACE inputs, never to predict an output.

Also the single numpy-float64 restatement of the reference's `.double()` forward (f64_forward_ref)."""
import functools

import numpy as np

import encode4_cases as ec
import fakequant_cases as fc
from encode4_cases import (MANTISSAS, SPECIALS, ULPS, WIN, golden, pair_case, pair_forms_present, random_book,  # noqa: F401
                           ulp_step, ulp_window)
from fakequant_cases import PLAN_SCAN, PLAN_TABLE, book, bucket_edges, pattern_rows, plan_header, round16, widen16  # noqa: F401

TINY = fc.TINY
HORIZON = 102400.0             # the scan's initial sub_min (KQ/quant_kernel.cu:25)
GUARD = 64                     # guard elements on either side of every output
POISON32 = 0x7FC5A5A5          # a NaN whose payload no arithmetic produces
POISON16 = 0x7FA5
POISON64 = 0x7FF85A5A5A5A5A5A
POISON_IDX = 0x5A5A            # > ANTQ_MAX_GRID
POISON_Q = 0x5A5A5A5A          # > 2^23, the largest level of k = 24


# ---------------------------------------------------------------------------------------------------------------------------
# 1: grids for antq_nearest (float64 arrays; the fp32 tests take them narrowed)
# ---------------------------------------------------------------------------------------------------------------------------
ANT_BOOKS = ("flint_b4_s", "int_b4_s", "apot_b4_s", "pot_b6_s", "flint_b6_s", "int_b8_s", "flint_b8_s")
OLIVE_BOOKS = ("olive_flint", "olive_flint_b8")
HAND_SIZES = (1, 2, 3, 63, 64, 65, 128, 255, 256, 257, 1024)
N_RANDOM_BOOKS = 4


def _hand_grids():
    rng = np.random.default_rng(4711)
    n = lambda m, sd: rng.standard_normal(m) * sd                     # noqa: E731  (doubles that float cannot hold)
    # sorted, gaps within a factor of four of each other: the fast path takes it (sorted Gaussian draws exceed the gap ratio)
    ladder = lambda m, step: (np.arange(m) - m / 2 + rng.uniform(-0.3, 0.3, m)) * step          # noqa: E731
    out = {}
    out["m1"] = [5.1]
    out["m2"] = [-1.0, 1.0]
    out["m3_dup_lower"] = [1.0, 3.0, 1.0]          # the tie at 2 goes to index 2: the LOWER value, though 3 is scanned after 1
    out["m3_dup_upper"] = [3.0, 1.0, 3.0]          # the tie at 2 goes to index 2: the UPPER value, though 1 is scanned after 3
    out["zeros_pn"] = [-1.0, 0.0, -0.0, 1.0]
    out["zeros_np"] = [-1.0, -0.0, 0.0, 1.0]
    out["zeros_unsorted"] = [1.0, -0.0, -1.0, 0.0, 0.5]
    out["tenths"] = np.arange(-8, 9) * 0.1
    v = n(63, 3)
    v[10] = v[40]
    out["m63_unsorted"] = v
    v = n(64, 3)
    v[5], v[7], v[33] = v[60], 0.0, -0.0
    out["m64_unsorted"] = v
    out["m65_unsorted"] = n(65, 3)                  # more than 64 entries, not sorted: the literal scan
    out["m65_sorted"] = ladder(65, 0.1)
    v = ladder(128, 0.37)
    v[50] = v[51]
    out["m128_sorted"] = v
    out["m255_sorted"] = ladder(255, 1.1)
    v = ladder(256, 0.013)
    v[0], v[255] = v[1], v[254]
    out["m256_sorted"] = v
    out["m257_sorted"] = np.sort(n(257, 30))
    out["m1024_sorted"] = np.sort(n(1024, 100))
    out["m1024_unsorted"] = n(1024, 100)
    out["mag65536"] = [-65536.0, 0.1, 65536.0]
    out["mag65536_next"] = [-65536.0, 0.1, float(ulp_step(65536.0, 1))]
    out["nan_entry"] = [-2.0, np.nan, 0.5, 3.0]
    out["inf_entry"] = [-2.0, 0.5, np.inf, 3.0, -np.inf]
    for tag, k in (("under", -1), ("at", 0), ("over", 1)):            # largest / smallest gap = 2^19 -/+ one ulp
        out["ratio_" + tag] = [-float(ulp_step(512.0, k)), 0.0, 2.0 ** -10]
    out["plateau"] = [0.0, 1e-3, 1e4]
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def nearest_grids():
    """{name: grid as float64}: the 4-, 6- and 8-bit ANT books, the OliVe cat(normal, outliers) lists (4-bit and the 509-entry
    8-bit one), random_book lists and the hand-made grids"""
    out = {}
    G = golden("ant_grids.npz")
    for k in ANT_BOOKS:
        out[k] = np.asarray(G[k], np.float64)
    for k in OLIVE_BOOKS:
        out[k] = np.asarray(book(k)[1], np.float64)
    for s in range(N_RANDOM_BOOKS):
        out["random_%d" % s] = np.asarray(random_book(np.random.default_rng(900 + s), bool(s % 2))[0], np.float64)
    out.update(_hand_grids())
    return out


def grid32(name):
    return nearest_grids()[name].astype(np.float32)


BOOK_GRIDS = ANT_BOOKS + OLIVE_BOOKS
# the grids every length / launch-form test uses: a small fast-path one, unsorted, the largest fast one, the literal scan
FORM_GRIDS = ("flint_b4_s", "m64_unsorted", "m256_sorted", "m257_sorted")
LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def fastlim_of(g):
    """The magnitude below which k_nearest_fast lets the two neighbouring values decide, restated in float32 from the rules in
    csrc/antq_k_nearest.h; 0: every element takes the literal scan.  Used to place inputs only."""
    g = np.asarray(g, np.float32)
    m = g.size
    f = np.float32
    with np.errstate(all="ignore"):
        if m > 256 or not (np.abs(g) <= f(65536)).all():
            return f(0)
        if m > 64 and not (g[:-1] <= g[1:]).all():
            return f(0)
        sv = np.sort(g)
        gaps = (sv[1:] - sv[:-1]).astype(np.float32)
        pos = gaps[gaps > 0]
        if pos.size == 0 or pos.max() > f(pos.min() * f(524288)):
            return f(0)
        vabs = max(abs(sv[0]), abs(sv[-1]))
        lim = min(f(f(min(pos[0], pos[-1]) * f(4194304)) - vabs), f(65536))
        lim = min(lim, f(f(102399) - vabs))
        return f(lim) if lim > f(2) * vabs else f(0)


# ---------------------------------------------------------------------------------------------------------------------------
# 1: fp32 inputs per grid
# ---------------------------------------------------------------------------------------------------------------------------
def window(c, k=ULPS):
    """2k + 1 floats around c: ulp_window, around zero the k + 1 smallest magnitudes of one sign and the k of the other, nothing
    for a NaN / Inf centre"""
    c = np.float32(c)
    if not np.isfinite(c):
        return np.zeros(0, np.float32)
    if np.abs(c) < TINY:
        b = np.arange(0, k + 1, dtype=np.uint32)
        return np.concatenate([b, b[1:] | np.uint32(0x80000000)]).view(np.float32)
    return ulp_window(c, k).astype(np.float32)


def sorted_distinct(g):
    """the finite values of the grid as float32, sorted, each once (-0.0 counts as 0.0)"""
    g = np.asarray(g).astype(np.float32)
    return np.unique(g[np.isfinite(g)] + np.float32(0))


def nearest_mids(g):
    """(fl32 of the midpoint of every pair of adjacent distinct values, True where that float IS the midpoint: a tie)"""
    gs = sorted_distinct(g)
    m64 = (gs[:-1].astype(np.float64) + gs[1:]) / 2
    c = m64.astype(np.float32)
    return c, c.astype(np.float64) == m64


def specials_f32():
    """magnitude_case's sweep without its scales: both signs of every exponent with MANTISSAS (exponent 0: denormals), SPECIALS"""
    e = np.arange(255, dtype=np.uint32)[:, None] << 23
    mag = (e | np.array(MANTISSAS, np.uint32)[None, :]).reshape(-1)
    return np.concatenate([mag, mag | np.uint32(0x80000000), SPECIALS.view(np.uint32)]).view(np.float32)


def horizon_centres(g):
    """fl32(g -/+ 102400) for the smallest / largest finite entry: where the index turns into ANTQ_IDX_NONE"""
    gs = sorted_distinct(g)
    return np.array([np.float64(gs[0]) - HORIZON, np.float64(gs[-1]) + HORIZON]).astype(np.float32)


def _stack(parts):
    """[(name, [windows of WIN floats])] -> (x, {name: [n, WIN] indices})"""
    xs, where, at = [], {}, 0
    for name, wins in parts:
        wins = [w for w in wins if w.size]
        assert all(w.size == WIN for w in wins)
        where[name] = (at + np.arange(len(wins) * WIN, dtype=np.int64)).reshape(-1, WIN)
        xs.extend(wins)
        at += len(wins) * WIN
    return (np.concatenate(xs) if xs else np.zeros(0, np.float32)).astype(np.float32), where


def nearest_case(g, extra=()):
    """The fp32 inputs of one grid: +/-16-ulp windows around every midpoint (the exact ones are the windows' centres: ties),
    every grid value, +/-fastlim_of(g), +/-65536 and the scan's horizon, then the specials.  extra: more window centres.
    dict(x, mids, values, fastlim, big, horizon, extra: [n, WIN] indices into x; ties: indices of the exact midpoints)"""
    g = np.asarray(g).astype(np.float32)
    c, exact = nearest_mids(g)
    lim = fastlim_of(g)
    x, where = _stack([("mids", [window(v) for v in c]),
                       ("values", [window(v) for v in sorted_distinct(g)]),
                       ("fastlim", [window(s * lim) for s in (1, -1)] if lim > 0 else []),
                       ("big", [window(v) for v in (65536.0, -65536.0)]),
                       ("horizon", [window(v) for v in horizon_centres(g)]),
                       ("extra", [window(v) for v in np.asarray(extra, np.float32)])])
    sp = specials_f32()
    where["ties"] = where["mids"][exact, ULPS] if c.size else np.zeros(0, np.int64)
    where["specials"] = x.size + np.arange(sp.size)
    return dict(x=np.concatenate([x, sp]), **where)


def windows_with_two(values, win):
    """how many of the windows (rows of indices) hold two different entries of `values`"""
    v = np.asarray(values).reshape(-1)[win]
    return int((v.max(1) != v.min(1)).sum()) if v.size else 0


def take(x, n, seed=0):
    """n elements of x in random order (with repeats only when x is shorter): a prefix that still holds windows' elements"""
    rng = np.random.default_rng(seed + n)
    return np.ascontiguousarray(x[rng.choice(x.size, n, replace=x.size < n)])


# ---------------------------------------------------------------------------------------------------------------------------
# 2: float64 inputs per grid
# ---------------------------------------------------------------------------------------------------------------------------
def f64_triples(c, steps=1):
    """For every float32 c (zeros, denormal-sized and non-finite ones left out) and either side: the double halfway between c and
    its float neighbour -- where (float)x changes -- with one double ulp on either side; steps > 1: the same between each of
    the next floats outwards (c + k, c + k + 1 ulps, k < steps).  [n, 2 sides, 3 * steps] float64."""
    c = np.asarray(c, np.float32).reshape(-1)
    c = c[np.isfinite(c) & (np.abs(c) >= TINY) & (np.abs(c) < np.float32(3e38))]
    mag = np.abs(c).view(np.uint32).astype(np.int64)
    sides = []
    for side in (-1, 1):
        k = np.arange(steps + 1, dtype=np.int64)[None, :] * (side * np.sign(c).astype(np.int64))[:, None]
        f = ((mag[:, None] + k).astype(np.uint32).view(np.float32) * np.sign(c)[:, None]).astype(np.float64)
        h = (f[:, :-1] + f[:, 1:]) / 2
        sides.append(np.stack([np.nextafter(h, -np.inf), h, np.nextafter(h, np.inf)], -1).reshape(c.size, 3 * steps))
    return np.stack(sides, 1)


def ulp_window64(c, k=8):
    """the 2k + 1 doubles around each non-zero finite c, flat"""
    c = np.asarray(c, np.float64).reshape(-1)
    c = c[np.isfinite(c) & (c != 0)]
    bits = np.abs(c).view(np.int64)[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]
    return (bits.view(np.float64) * np.sign(c)[:, None]).reshape(-1)


FLT_MAX = float(np.finfo(np.float32).max)


def specials_f64():
    """doubles beyond FLT_MAX (the tie towards Inf at FLT_MAX + 2^103 and its neighbours among them), double denormals, doubles
    that narrow to float denormals or to 0, +/-0, NaNs, +/-Inf"""
    tie = FLT_MAX + 2.0 ** 103
    a = [FLT_MAX, np.nextafter(FLT_MAX, np.inf), np.nextafter(tie, 0.0), tie, np.nextafter(tie, np.inf), 3.5e38, 1e300,
         np.finfo(np.float64).max, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-40, 1.4e-45, 0.7e-45, 0.71e-45, 2.0 ** -150,
         np.nextafter(2.0 ** -150, 1.0), 1e-60, 0.0, np.inf]
    a = np.float64(a)
    return np.concatenate([a, -a, np.float64([np.nan]), np.array([0x7FF0000000000001, 0xFFF8000000000001], np.uint64).view(np.float64)])


def nearest_case_f64(g64):
    """The float64 inputs of one grid (the kernel narrows grid and x to float): the narrowing triples of every float midpoint of
    the narrowed grid, +/-8 double ulps around the midpoint itself, the same around every narrowed grid value and the
    horizon, the fp32 inputs widened, and the float64 specials.
    dict(x, triples: [n, 3] indices (one row per midpoint and side), mids: [n, 17] indices)"""
    g32 = np.asarray(g64).astype(np.float32)
    c, _ = nearest_mids(g32)
    t = f64_triples(c).reshape(-1, 3)
    w = ulp_window64(c.astype(np.float64)).reshape(-1, 17)
    others = np.concatenate([sorted_distinct(g32), horizon_centres(g32)])
    with np.errstate(invalid="ignore"):           # (widening a signalling NaN)
        wide = nearest_case(g32)["x"].astype(np.float64)
    # ulp_window64(g64): doubles next to grid values that float cannot hold (0.1 ...), the grid's own narrowing
    rest = [f64_triples(others).reshape(-1), ulp_window64(others.astype(np.float64)), ulp_window64(np.asarray(g64, np.float64)), wide,
            specials_f64()]
    x = np.concatenate([t.reshape(-1), w.reshape(-1)] + rest)
    return dict(x=x, triples=np.arange(t.size, dtype=np.int64).reshape(-1, 3), mids=t.size + np.arange(w.size, dtype=np.int64).reshape(-1, 17))


# ---------------------------------------------------------------------------------------------------------------------------
# 3: plans
# ---------------------------------------------------------------------------------------------------------------------------
PLAN_GRIDS = dict(small="flint_b4_s", big_linear="int_b8_s", big="olive_flint_b8", scan="m63_unsorted")
VECTOR_COUNTS = (1, 511, 512, 513, 1023, 1024, 1025, 2049)


def tab_units(h):
    """16-byte units of a plan staged into LDS (csrc/antq_host.h: n_entries + m_pad / 4)"""
    return h["n_entries"] + (h["m_pad"] >> 2)


def plan_class(h):
    """'scan', 'small' (LDS <= 2048 bytes: two vectors per lane) or 'big' (four)"""
    if h["kind"] != PLAN_TABLE:
        return "scan"
    return "small" if tab_units(h) * 16 <= 2048 else "big"


def mixed_vectors(g, lim, epl, to16=None):
    """Vectors of epl elements of which one (every position in turn) is at or beyond `lim` -- the plan's fastlim itself, 1.5 x
    it, NaN, Inf, either sign -- and the others sit next to midpoints of the grid: the whole vector must take the scan."""
    c, _ = nearest_mids(g)
    inside = np.concatenate([window(v, 2) for v in c[:: max(1, c.size // 12)]] + [np.float32([0.0, 0.25])]).astype(np.float32)
    beyond = np.float32([lim, -lim, 1.5 * lim, -1.5 * lim, np.nan, np.inf, -np.inf, float(ulp_step(lim, 1))])
    out, k = [], 0
    for b in beyond:
        for pos in range(epl):
            v = inside[(k + np.arange(epl)) % inside.size].copy()
            v[pos] = b
            out.append(v)
            k += epl - 1
    return np.concatenate(out)


def plan_case(g, h):
    """nearest_case of the grid with windows at every bucket edge and at +/-h['fastlim'] added, behind the mixed vectors; padded
    with zeros to whole vectors of 8 elements.  dict(x, n_mixed, edges: [n, WIN] indices into x, one row per bucket edge)"""
    g = np.asarray(g, np.float32)
    edges = bucket_edges(h)
    extra = np.concatenate([edges, np.float32([h["fastlim"], -h["fastlim"]]) if h["fastlim"] > 0 else np.zeros(0, np.float32)])
    mv = mixed_vectors(g, np.float32(h["fastlim"] if h["fastlim"] > 0 else HORIZON), 4)
    case = nearest_case(g, extra)
    x = np.concatenate([mv, case["x"]])
    return dict(x=np.concatenate([x, np.zeros(-x.size % 8, np.float32)]), n_mixed=mv.size, edges=mv.size + case["extra"][:edges.size])


def altered_grids(g):
    """[(tag, device grid)]: one entry one ulp off at position 0, at m - 1 (and at 255 and 256 of a longer grid), 0.0 replaced by
    -0.0, an entry replaced by NaN -- each differs from g in exactly one entry's bits"""
    g = np.asarray(g, np.float32)
    out = []
    for at in [0, g.size - 1] + ([255, 256] if g.size > 256 else []):
        a = g.copy()
        a[at] = ulp_step(a[at], 1) if a[at] != 0 else np.float32(1e-45)
        out.append(("ulp@%d" % at, a))
    z = np.flatnonzero((g == 0) & ~np.signbit(g))
    if z.size:                                        # (the last one in scan order: the zero whose sign the output carries)
        a = g.copy()
        a[z[-1]] = np.float32(-0.0)
        out.append(("-0.0@%d" % z[-1], a))
    a = g.copy()
    a[g.size // 2] = np.float32(np.nan)
    out.append(("nan@%d" % (g.size // 2), a))
    return out


def altered_front(g, a):
    """Inputs that tell the device grid `a` from the plan's grid `g`: +/-16-ulp windows around the entry that differs (its value
    in either grid), its neighbours among the sorted values and the midpoints towards them; whole vectors of 8 (zero padded)"""
    g, a = np.asarray(g, np.float32), np.asarray(a, np.float32)
    at = int(np.flatnonzero(g.view(np.uint32) != a.view(np.uint32))[0])
    gs = sorted_distinct(g)
    k = int(np.searchsorted(gs, g[at] + np.float32(0)))
    nb = gs[max(k - 1, 0):k + 2].astype(np.float64)
    c = np.concatenate([np.float64([g[at], a[at]]), nb, (nb + np.float64(g[at])) / 2]).astype(np.float32)
    x = np.concatenate([window(v) for v in c])
    return np.concatenate([x, np.zeros(-x.size % 8, np.float32)])


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the affine quantiser
# ---------------------------------------------------------------------------------------------------------------------------
AFFINE_K = (1, 2, 4, 8, 16, 24)
AFFINE_ROW_LENS = (4, 12, 20, 1028)


def affine_params(k, mn, mx):
    """(scale, zp) of AQ/quant_affine.py:75-85 in numpy float32: used to place the tie windows"""
    f = np.float32
    with np.errstate(all="ignore"):
        rng_ = f(f(mx) - f(mn))
        if rng_ < f(1e-8):
            rng_ = f(1e-8)
        scale = f(f(f(1.0) / rng_) * f((1 << k) - 1))
        zp = f(np.rint(f(scale * f(mn))) + f(1 << (k - 1)))
    return scale, zp


def affine_levels(rng, k):
    """the levels j whose upper tie j + 0.5 gets a window: all of -half - 1 .. half for k <= 8 (both clamps included), otherwise
    the 40 at each end and 150 drawn ones"""
    half = 1 << (k - 1)
    if k <= 8:
        return np.arange(-half - 1, half + 1, dtype=np.int64)
    ends = np.concatenate([np.arange(-half - 1, -half + 39), np.arange(half - 39, half + 1)])
    return np.concatenate([ends, rng.integers(-half + 39, half - 39, 150)]).astype(np.int64)


def random_ranges(rng, n):
    """awkward (min, max): ranges over seven decades, min anywhere from far below to just above 0"""
    width = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n))
    mn = -width * rng.uniform(-0.2, 1.5, n)
    return np.stack([mn, mn + width], 1).astype(np.float32)


def scale_edge_ranges(k):
    """(0, r) for the r next to (2^k - 1) / 2^40 (k = 24: 1e-5 .. 2e-5) and next to (2^k - 1) * 2^40, where the scale is within a
    few ulps of 2^40 / 2^-40, either side and on it; ranges below the clamp of 1e-8 left out"""
    out = []
    for e in (-40.0, 40.0):
        r0 = np.float32(((1 << k) - 1) * 2.0 ** e)
        for j in (-3, -1, 0, 1, 3):
            r = ulp_step(r0, j)
            if r >= np.float32(2e-8):
                out.append((0.0, r))
    return np.array(out, np.float32).reshape(-1, 2)


def special_ranges(k):
    """max == min, max < min, a range below the clamp, NaN min, min = 0 (twice), a range of 3e38, NaN max and the scale edges; and
    min = 1e20 "with a range of 1": in float32 1e20 + 1 is 1e20, so the range vanishes and is clamped to 1e-8, the scale is
    (2^k - 1) * 1e8 and |num| ~ scale * 1e20 exceeds 2^60.  (No representable range does that: a range of at least one ulp of
    min keeps |num| below (2^k - 1) * 2^23.)  For k <= 8 that scale lies inside the 5-FMA division's domain, so the true
    division is taken because of the numerator alone; for k = 16 and 24 the scale is outside it as well."""
    f = np.float32
    fixed = [(0.3, 0.3), (1.0, -2.0), (1e-9, 2e-9), (np.nan, 1.0), (0.0, 1.7), (0.0, 255.0), (-1.5e38, 1.5e38),
             (1e20, f(f(1e20) + f(1.0))), (-3.0, np.nan)]
    return np.concatenate([np.array(fixed, np.float32), scale_edge_ranges(k)])


def affine_case(rng, k, ranges, row_len):
    """Per range as many rows of row_len as its payload needs (every range the same number; the rest Gaussian over the range):
    +/-16-ulp windows around x = (zp + j + 0.5) / scale for affine_levels (non-finite centres left out), a few specials and
    x = (zp + j) / scale, the middle of each of these levels.
    dict(x [rows, row_len], xmin, xmax (per row), windows [n, WIN] flat indices, level, owner (per window: j, range))"""
    ranges = np.asarray(ranges, np.float32).reshape(-1, 2)
    payloads, meta = [], []
    sp = np.concatenate([SPECIALS, np.float32([1e30, -1e30, 3e38, 1e-30])])
    for i, (mn, mx) in enumerate(ranges):
        scale, zp = affine_params(k, mn, mx)
        lv = affine_levels(rng, k)
        with np.errstate(all="ignore"):
            c = ((np.float64(zp) + lv + 0.5) / np.float64(scale)).astype(np.float32)
        keep = np.isfinite(c) & ((np.abs(c) >= TINY) | (c == 0)) & (np.abs(c) < np.float32(3e38))
        wins = [window(v) for v in c[keep]]
        with np.errstate(all="ignore"):                 # the middle of every level (k <= 8) / of the drawn ones
            mid = ((np.float64(zp) + np.unique(lv)) / np.float64(scale)).astype(np.float32)
        payloads.append(np.concatenate(wins + [sp, mid[np.isfinite(mid)]]).astype(np.float32))
        meta.append(lv[keep])
    rps = max(1, max(-(-p.size // row_len) for p in payloads))
    span = rps * row_len
    with np.errstate(all="ignore"):
        lo = np.nan_to_num(ranges.min(1), nan=0.0).astype(np.float64)
        wd = np.clip(np.nan_to_num(np.abs(ranges[:, 1] - ranges[:, 0]), nan=1.0, posinf=1e30), 1e-6, 1e30).astype(np.float64)
    x = (lo[:, None] + wd[:, None] * rng.uniform(-0.2, 1.2, (ranges.shape[0], span))).astype(np.float32)
    windows, level, owner = [], [], []
    for i, p in enumerate(payloads):
        x[i, :p.size] = p
        nw = meta[i].size
        windows.append(i * span + np.arange(nw * WIN, dtype=np.int64).reshape(nw, WIN))
        level.append(meta[i])
        owner.append(np.full(nw, i))
    return dict(x=x.reshape(-1, row_len), xmin=np.repeat(ranges[:, 0], rps), xmax=np.repeat(ranges[:, 1], rps),
                windows=np.concatenate(windows), level=np.concatenate(level), owner=np.concatenate(owner))


def affine_inner(case, k):
    """the windows whose tie lies strictly inside the clamps: both j and j + 1 are levels"""
    half = 1 << (k - 1)
    return (case["level"] >= -half) & (case["level"] <= half - 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the float64 forward
# ---------------------------------------------------------------------------------------------------------------------------
def f64_forward_parts(oracle, x2, alpha, g, gmax, ovp, per_row):
    """The reference's `.double()` forward (AQ:535-551 / OQ:294-330) restated in numpy float64 around the oracle's scan, which
    narrows to float inside as the reference's kernel does.  x2: float64 [rows, cols]; alpha: `rows` values (per_row) or one.
    Returns (out [rows, cols], the scan's indices (flat), the pair rule's victim mask (flat; all False without it))."""
    x2 = np.asarray(x2, np.float64)
    alpha = np.asarray(alpha).astype(np.float64)
    with np.errstate(all="ignore"):
        scale = alpha.reshape(-1, 1) / gmax if per_row else alpha.reshape(-1)[0] / gmax
        d = x2 / scale
        q, idx = oracle.nearest(d.reshape(-1), np.asarray(g).astype(np.float64))
        victim = np.zeros(q.size, bool)
        if ovp:                                          # OQ:311-320
            mask = np.abs(q) > 32
            vo = np.roll(mask, 1)
            vo[::2] = False
            ve = np.roll(mask & ~vo, -1)
            ve[1::2] = False
            victim = ve | vo
            q = q * (~victim)
        q = q.reshape(x2.shape)
        t = (q - d) + d
        return t * scale, idx, victim


def f64_forward_ref(oracle, x2, alpha, g, gmax, ovp, per_row):
    return f64_forward_parts(oracle, x2, alpha, g, gmax, ovp, per_row)[0]


class F64Decisions:
    """Stands in for the oracle module where a builder's checker of encode4_cases asks for `forward`'s bare indices: answers
    with the float64 restatement's (x and alpha taken as doubles)."""

    def __init__(self, oracle):
        self.oracle = oracle

    def forward(self, x, alpha, g, gmax, ovp):
        x = np.asarray(x, np.float64)
        _, idx, _ = f64_forward_parts(self.oracle, x, alpha, g, gmax, ovp, True)
        return None, idx.reshape(x.shape)


def f64_alpha(alpha32):
    """float32 scales as doubles that float cannot hold (2^-30 relative: a hundredth of a float ulp)"""
    return np.asarray(alpha32, np.float32).astype(np.float64) * (1.0 + 2.0 ** -30)


F64_BOOKS = ("flint_b4_s", "int_b4_s", "int_b8_s", "olive_flint", "scan_list")
F64_ALPHAS = np.float64([0.1, 1.0 / 3.0, 2.7182818284590452, 6.02e-5, 417.3, 0.0, -0.05, np.nan])
F64_ALPHAS_8BIT = F64_ALPHAS[[0, 3, 5, 6, 7]]
BIG_F64 = 2 * 256 * 8192 * 2 + 513       # pairs > 256 * 8192 * 2: every lane of the capped launch loops at least twice


def f64_book(name):
    """(name, grid float32, gmax, n_normal, pair rule) -- `scan_list`: an arbitrary list whose plan is a scan plan"""
    if name == "scan_list":
        g = grid32(PLAN_GRIDS["scan"])
        return (name, g, float(g.max()), 0, False)
    return book(name)


F64_STEPS = 4         # float neighbours on either side of a threshold whose narrowing edges a window holds: the scan's decision is
#                       made on rounded differences and can sit a float ulp or two off the midpoint


def f64_case(bk, h, alphas):
    """One row per scale s = alpha / gmax (float64): x = d * s for the narrowing triples d (F64_STEPS floats outwards on either side) of every threshold of the book and of
    +/-fastlim of the plan, each with +/-8 double ulps of x around it, then the float64 specials; short rows padded by
    repeating.  dict(x [n, L], alpha, windows: [n, 51 * F64_STEPS] flat indices, one row per (scale, threshold, side))"""
    _, g, gmax, nn, ovp = bk
    c, _ = nearest_mids(g)
    t = f64_triples(c, F64_STEPS).reshape(-1, 3 * F64_STEPS)
    lim = f64_triples(np.float32([h["fastlim"], -h["fastlim"]])).reshape(-1) if h["fastlim"] > 0 else np.zeros(0)
    alphas = np.asarray(alphas, np.float64)
    rows, nwin = [], []
    for a in alphas:
        s = a / gmax
        with np.errstate(all="ignore"):
            xw = ulp_window64(t.reshape(-1) * s) if np.isfinite(s) and s != 0 else np.zeros(0)
            xl = ulp_window64(lim * s) if np.isfinite(s) and s != 0 else np.zeros(0)
        ok = xw.size == t.size * 17              # (no product was 0 or Inf)
        rows.append(np.concatenate([xw if ok else t.reshape(-1), xl, specials_f64(), g.astype(np.float64) * (s if np.isfinite(s) else 1.0)]))
        nwin.append(t.shape[0] if ok else 0)
    L = max(r.size for r in rows)
    x = np.stack([np.resize(r, L) for r in rows])
    windows = [i * L + np.arange(nwin[i] * 51 * F64_STEPS, dtype=np.int64).reshape(-1, 51 * F64_STEPS) for i in range(len(rows))]
    return dict(x=x, alpha=alphas, windows=np.concatenate(windows))


def f64_pair_case(bk, row_len=64, n_scales=8):
    """pair_case's octets around the normal | outlier boundary as doubles, on scales that float cannot hold"""
    _, g, gmax, nn, ovp = bk
    case = pair_case(np.random.default_rng(515), g, gmax, nn, row_len, n_scales)
    return dict(x=case["x"].astype(np.float64), alpha=f64_alpha(case["alpha"]), pairs=case["pairs"], alpha32=case["alpha"])


ODD_SHAPES = ((7, 33), (33, 1))


def f64_odd_case(bk, shape, first_outlier, per_row, seed=77):
    """An odd-sized OliVe tensor whose last element pairs with element 0 (torch.roll wraps): element 0 an outlier (the last
    element becomes its victim), or element 0 normal and the last element an outlier (which then stays)."""
    _, g, gmax, nn, ovp = bk
    rng = np.random.default_rng(seed + shape[0])
    rows, cols = shape
    alpha = rng.uniform(0.05, 3.0, rows if per_row else 1)
    s = np.repeat(alpha / gmax, cols) if per_row else np.full(rows * cols, alpha[0] / gmax)
    d = rng.standard_normal(rows * cols) * 14
    d[rng.random(d.size) < 0.15] *= 6
    d[0], d[-1] = (48.0, 3.0) if first_outlier else (3.0, 48.0)
    return dict(x=(d * s).reshape(shape), alpha=alpha)
