"""Input builders for the edge tests of the in-kernel abs-max forward of bf16 / f16 rows (test_gpu_dynamic16_edges.py) and for
the host test that holds the builders to their conditions with the CPU oracle alone (test_dynamic16_cases_host.py).  numpy and
the oracle only; books, widen16 and round16 come from fakequant_cases.  New here: the row lengths at every boundary of the
16-bit-domain dynamic kernels' launch shapes, rows whose abs-max is planted at the positions where a mask, a half-word, a
vector step or a wavefront can go missing, abs-max values from the smallest subnormal to NaN, every 16-bit pattern below a
maximum, and numpy restatements of the wrong ways to take the abs-max (which the case set must tell from the right one)."""
import functools

import numpy as np

import fakequant_cases as fc
from fakequant_cases import book, round16, widen16  # noqa: F401

DTYPES = ("bfloat16", "float16")
BOOKS_H = ("flint_b4_s", "int_b4_s", "flint_b4_u", "olive_flint")      # 4-bit: 16-bit-domain eligible (PlanHeader::hdom)
BOOK_WIDE = "int_b8_s"                                                  # no 16-bit-domain form, but the approximate quotient
BOOKS = BOOKS_H + (BOOK_WIDE,)
HDOM_BIT = dict(bfloat16=1, float16=2)

# magnitude patterns of the two formats
FMT = dict(bfloat16=dict(max=0x7f7f, min_normal=0x0080, max_sub=0x007f, min_sub=0x0001, inf=0x7f80, nan=0x7fc0, one=0x3f80,
                         awkward=0x3faf, low=0x02af),
           float16=dict(max=0x7bff, min_normal=0x0400, max_sub=0x03ff, min_sub=0x0001, inf=0x7c00, nan=0x7e00, one=0x3c00,
                        awkward=0x3d77, low=0x1577))
SEED = 1616


# ---------------------------------------------------------------------------------------------------------------------------
# 1: row lengths
# ---------------------------------------------------------------------------------------------------------------------------
def shape_of(vpr):
    """(wavefronts per row, vector steps per lane in use) of a row of vpr 16-byte vectors: csrc/antq_k_hrow.h hrow_dyn_shape
    restated (shorter rows: lane groups, one step)"""
    wpr = 1 if vpr <= 512 else 4 if vpr <= 2048 else 16
    return wpr, -(-vpr // (64 * wpr))


# label -> (row length in elements, elements by which x and out start off a 16-byte boundary)
GROUPS = dict(
    lane=(1, 2, 16, 64),
    w1=(128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512),
    w4=(513, 1024, 2047, 2048),
    w16=(2049, 4096, 8191, 8192),
)
VPRS = tuple(v for k in ("lane", "w1", "w4", "w16") for v in GROUPS[k])
FALLBACK = (("v8193", 8 * 8193, 0), ("ragged", 8 * 129 + 3, 0), ("lead", 8 * 128, 1))
GROUP_NAMES = tuple(GROUPS) + ("fallback",)


def shapes_of_group(name):
    """[(label, row length in elements, lead)]"""
    if name == "fallback":
        return list(FALLBACK)
    return [("v%d" % v, 8 * v, 0) for v in GROUPS[name]]


ALL_SHAPES = tuple(s for n in GROUP_NAMES for s in shapes_of_group(n))
ROW_COUNTS = (1, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# helpers on patterns
# ---------------------------------------------------------------------------------------------------------------------------
def value(oracle, p16, dtype_name):
    return widen16(oracle, np.asarray(p16, np.uint16), dtype_name)


def pattern_at_most(oracle, v, dtype_name):
    """largest magnitude pattern whose value is <= v (v >= 0, finite)"""
    with np.errstate(all="ignore"):
        p = int(round16(oracle, np.float32([v]), dtype_name)[0])
    if float(value(oracle, [p], dtype_name)[0]) > float(v):
        p -= 1
    return p


def filler(oracle, rng, dtype_name, shape, top16):
    """patterns of both signs, uniform in value, every magnitude <= value(top16) / 4"""
    tv = float(value(oracle, [top16], dtype_name)[0]) / 4.0
    cap = pattern_at_most(oracle, tv, dtype_name)
    with np.errstate(all="ignore"):
        f = round16(oracle, rng.uniform(-tv, tv, shape).astype(np.float32), dtype_name)
    return (f & 0x8000) | np.minimum(f & 0x7fff, cap).astype(np.uint16)


def vector_positions(vpr):
    """The vectors of a row of vpr at which a launch shape can lose one: per wavefront (the first, a middle and the last one in
    use) lane 0 and the last lane in use of the first and of the last vector step in use, i.e. also its first and last vector"""
    wpr, nv = shape_of(vpr)
    span = 64 * nv
    active = -(-vpr // span)
    vs = set()
    for g in sorted({0, active // 2, active - 1}):
        lo, hi = g * span, min(vpr, (g + 1) * span)
        for u in {0, (hi - lo - 1) // 64}:
            a = lo + 64 * u
            vs |= {a, min(hi, a + 64) - 1}
        vs |= {lo, hi - 1}
    return sorted(vs)


def planted_positions(row_len):
    """Element indices: element 0 and the last one, the low and the high half of the first, a middle and the last 32-bit word,
    and one element (the slot inside the vector rotates) of every vector of vector_positions"""
    vpr = -(-row_len // 8)
    mid = 8 * (vpr // 2)
    ps = {0, 1, row_len - 1, row_len - 2, min(mid + 2, row_len - 1), min(mid + 3, row_len - 1)}
    for k, v in enumerate(vector_positions(vpr)):
        ps.add(min(8 * v + (3 * k + 5) % 8, row_len - 1))
    return sorted(p for p in ps if p >= 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 2: where the abs-max sits
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _planted(dtype_name, row_len):
    from oracle import antq_oracle as oracle
    F = FMT[dtype_name]
    rng = np.random.default_rng(SEED + row_len + (0 if dtype_name == "bfloat16" else 7))
    pos = planted_positions(row_len)
    rows = len(pos) + 2
    x = filler(oracle, rng, dtype_name, (rows, row_len), F["awkward"])
    m16 = (F["awkward"] + (np.arange(rows) % 24)).astype(np.uint16)           # a different maximum (so a different scale) per row
    planted = []
    for r, p in enumerate(pos):
        x[r, p] = m16[r] | (0x8000 if r % 2 else 0)
        planted.append((p,))
    if row_len >= 2:
        a, b = pos[len(pos) // 3], pos[-1]
        if a == b:
            a = pos[0]
        x[rows - 2, a], x[rows - 2, b] = m16[rows - 2], m16[rows - 2] | 0x8000      # +M and -M
        planted.append((a, b))
    else:
        x[rows - 2, 0] = m16[rows - 2]
        planted.append((0,))
    p = pos[len(pos) // 2]
    x[rows - 1, p] = m16[rows - 1] | 0x8000                                           # only -M
    planted.append((p,))
    x.setflags(write=False)
    return dict(x=x, planted=planted, m16=m16)


def planted_case(dtype_name, row_len):
    """One row per planted position: every element of magnitude <= M / 4 except the planted +/-M (signs alternate by row), M a
    different awkward pattern per row; then a row with +M and -M at two positions, and one whose only maximum is -M.
    dict(x uint16 [rows, row_len] read-only, planted: per row the tuple of planted positions, m16: per row M's pattern)"""
    return _planted(dtype_name, row_len)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: what the abs-max is
# ---------------------------------------------------------------------------------------------------------------------------
MAG_VPRS = (16, 128, 512, 2048, 8192)
RATIOS = (1.0, 0.83, 0.25, 1.0625, 2.0 ** -20, 0.0, -0.5, 2.0 ** -140)
MAG_ROWS = ("awkward", "power of two", "largest finite", "smallest normal", "largest subnormal", "smallest subnormal", "zeros",
            "NaN", "+Inf", "-Inf", "NaN then Inf", "Inf then NaN", "order of the ratio")
ORDER_RATIO, ORDER_BOOK = 1.0625, "flint_b4_s"


@functools.lru_cache(maxsize=None)
def order_sensitive_top(dtype_name):
    """The first M in [1, 4) for which the scale fl(fl(M * ratio) / gmax) and the scale with the ratio applied last,
    fl(fl(M / gmax) * ratio), give the element M itself two different outputs (ORDER_RATIO, ORDER_BOOK): one fp32 ulp of the
    scale shows in a 16-bit output only where q * s falls next to a rounding boundary of the type"""
    from oracle import antq_oracle as oracle
    bk = book(ORDER_BOOK)
    gmax, r32 = np.float32(bk[2]), np.float32(ORDER_RATIO)
    one = FMT[dtype_name]["one"]
    pats = np.arange(one, one + 2 * (FMT[dtype_name]["min_normal"]), dtype=np.uint16)       # two binades
    m = value(oracle, pats, dtype_name)
    a = (m * r32).astype(np.float32)
    s_last = ((m / gmax).astype(np.float32) * r32).astype(np.float32)
    a_last = np.array([fc.alpha_for_scale(v, gmax) or np.nan for v in s_last], np.float32)
    usable = ~np.isnan(a_last)
    x = pats.reshape(-1, 1)
    differ = (forward16(oracle, x, dtype_name, bk, a) != forward16(oracle, x, dtype_name, bk, np.where(usable, a_last, a))).reshape(-1)
    return int(pats[np.flatnonzero(differ & usable)[0]])


@functools.lru_cache(maxsize=16)
def _magnitudes(dtype_name, vpr):
    from oracle import antq_oracle as oracle
    F = FMT[dtype_name]
    rl = 8 * vpr
    rng = np.random.default_rng(SEED + 31 * vpr + (0 if dtype_name == "bfloat16" else 7))
    vs = vector_positions(vpr)
    tops = [F["awkward"] + 9, F["one"] - (3 << (7 if dtype_name == "bfloat16" else 10)), F["max"], F["min_normal"], F["max_sub"], F["min_sub"]]
    x = np.zeros((len(MAG_ROWS), rl), np.uint16)
    m16 = np.zeros(len(MAG_ROWS), np.uint16)
    at = []
    for r, top in enumerate(tops):
        x[r] = filler(oracle, rng, dtype_name, rl, top)
        p = 8 * vs[(2 * r + 1) % len(vs)] + (5 * r + 1) % 8
        x[r, p] = top | (0x8000 if r % 2 else 0)
        m16[r] = top
        at.append((p,))
    r = len(tops)
    x[r] = np.where(rng.random(rl) < 0.5, 0x8000, 0).astype(np.uint16)          # +/-0 only
    at.append(())
    first, last = 8 * vs[0] + 3, 8 * vs[-1] + 6                                  # (first vector of the first, last of the last wavefront in use)
    for r, pats in ((r + 1, (F["nan"],)), (r + 2, (F["inf"],)), (r + 3, (F["inf"] | 0x8000,)), (r + 4, (F["nan"] | 0x8000, F["inf"])),
                    (r + 5, (F["inf"] | 0x8000, F["nan"] + 1))):
        x[r] = filler(oracle, rng, dtype_name, rl, F["awkward"])
        if len(pats) == 1:
            p = 8 * vs[(r + 2) % len(vs)] + r % 8
            x[r, p] = pats[0]
            at.append((p,))
        else:
            x[r, first], x[r, last] = pats
            at.append((first, last))
        m16[r] = max(p_ & 0x7fff for p_ in pats)
    r, top = len(MAG_ROWS) - 1, order_sensitive_top(dtype_name)
    x[r] = filler(oracle, rng, dtype_name, rl, top)
    p = 8 * vs[len(vs) // 2] + 4
    x[r, p], m16[r] = top, top
    at.append((p,))
    x.setflags(write=False)
    return dict(x=x, planted=at, m16=m16)


def magnitude_case(dtype_name, vpr):
    """One row per MAG_ROWS entry: the planted maximum is an awkward value, a power of two, the largest finite value, the
    smallest normal, the largest and the smallest subnormal (every other element <= M / 4: zeros for the last); a row of +/-0;
    NaN, +Inf, -Inf; NaN and Inf in the first vector of the first and the last vector of the last wavefront in use, both ways;
    and the M of order_sensitive_top, whose own output tells alpha = fl(M * ratio) from a ratio applied to the scale."""
    return _magnitudes(dtype_name, vpr)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: every pattern below the maximum
# ---------------------------------------------------------------------------------------------------------------------------
PATTERN_TOPS = ("max", "awkward", "low")
PATTERN_RATIOS = (1.0, 0.25)
PAIR_FAR_RATIO = 2.0 ** -5        # OliVe: 4 * gmax = 128 stays inside its table (xlim 768); at 2^-5 the row reaches 1024
OVERFLOW_RATIO = 1.0625           # largest finite M: with ratio <= 1 no output exceeds M (gmax * s <= M); here gmax * s does
DEAL_VPRS = (128, 512, 2048)


def pattern_ratios(top_name, pair):
    """1 and 0.25 for every row set; 2^-5 too where the pair rule is on, 1.0625 too for the largest finite M"""
    return PATTERN_RATIOS + ((PAIR_FAR_RATIO,) if pair else ()) + ((OVERFLOW_RATIO,) if top_name == "max" else ())


@functools.lru_cache(maxsize=8)
def _patterns(dtype_name, top_name):
    top = FMT[dtype_name][top_name]
    rng = np.random.default_rng(SEED + top)
    mags = np.arange(top + 1, dtype=np.uint16)
    pats = rng.permutation(np.concatenate([mags, mags | 0x8000]))
    n = pats.size
    vpr = -(-n // 8)
    assert vpr <= 8192
    one = np.zeros((1, 8 * vpr), np.uint16)
    one[0, :n] = pats
    out = [one]
    for v in DEAL_VPRS:
        cap = 8 * v - 2
        rows = -(-n // cap)
        x = np.zeros((rows, 8 * v), np.uint16)
        for r in range(rows):
            chunk = pats[r * cap:(r + 1) * cap]
            where = rng.permutation(8 * v)
            x[r, where[:chunk.size]] = chunk
            x[r, where[chunk.size]], x[r, where[chunk.size + 1]] = top, top | 0x8000
        out.append(x)
    for x in out:
        x.setflags(write=False)
    return tuple(out)


def pattern_case(dtype_name, top_name):
    """Every pattern of magnitude <= M, both signs (+/-0 among them), shuffled: as ONE zero-padded row, and dealt over rows of
    128, 512 and 2048 vectors each of which also holds +M and -M (so all rows share the alpha).  Tuple of four uint16 arrays."""
    return _patterns(dtype_name, top_name)


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def reference(oracle, x16, dtype_name, bk, ratio=1.0, pair=None):
    """(alpha_ref float32 [rows], out_ref uint16 like x16, oracle indices): alpha = oracle.absmax of the widened rows,
    out = the oracle's fp32 sequence on the widened rows with that alpha, rounded once to the type"""
    _, g, gmax, nn, ovp = bk
    xf = widen16(oracle, x16, dtype_name)
    with np.errstate(all="ignore"):
        alpha = oracle.absmax(xf, True, ratio)
        out, idx = oracle.forward(xf, alpha, g, gmax, ovp if pair is None else pair)
        return alpha, round16(oracle, out, dtype_name), idx


def forward16(oracle, x16, dtype_name, bk, alpha, pair=None):
    _, g, gmax, nn, ovp = bk
    with np.errstate(all="ignore"):
        out, _ = oracle.forward(widen16(oracle, x16, dtype_name), alpha, g, gmax, ovp if pair is None else pair)
        return round16(oracle, out, dtype_name)


def same16(oracle, a16, b16, dtype_name):
    """element-wise: equal patterns, or both NaN"""
    fa, fb = widen16(oracle, a16, dtype_name), widen16(oracle, b16, dtype_name)
    return (a16 == b16) | (np.isnan(fa) & np.isnan(fb))


def same32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------
# wrong ways to take the abs-max
# ---------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("skip last vector", "skip first step", "skip last step", "skip last wavefront", "signed max", "low halves", "high halves",
            "NaN dropped", "f16 subnormal as zero", "ratio on the scale")


def mistaken_alpha(oracle, kind, x16, dtype_name, ratio, gmax):
    """alpha per row under one wrong abs-max (float32 [rows]), or None where the mistake has no meaning for this tensor"""
    xf = widen16(oracle, x16, dtype_name)
    rl = x16.shape[1]
    vpr = -(-rl // 8)
    wpr, nv = shape_of(vpr)
    span = 64 * nv
    vec = np.arange(rl) // 8
    wave, step = vec // span, (vec % span) // 64
    active = -(-vpr // span)
    r32 = np.float32(ratio)

    def amax(keep):
        if not keep.any():
            return None
        with np.errstate(all="ignore"):
            return oracle.absmax(np.ascontiguousarray(xf[:, keep]), True, ratio)

    with np.errstate(all="ignore"):
        if kind == "skip last vector":
            return amax(vec != vpr - 1)
        if kind == "skip first step":
            return amax(step != 0)
        if kind == "skip last step":
            last = (np.minimum(vpr, (wave + 1) * span) - wave * span - 1) // 64
            return amax(step != last)
        if kind == "skip last wavefront":
            return amax(wave != active - 1) if active > 1 else None
        if kind == "signed max":
            return (np.max(xf, axis=1).astype(np.float32) * r32).astype(np.float32)
        if kind == "low halves":
            return amax(np.arange(rl) % 2 == 0)
        if kind == "high halves":
            return amax(np.arange(rl) % 2 == 1)
        if kind == "NaN dropped":
            return (np.fmax.reduce(np.abs(xf), axis=1).astype(np.float32) * r32).astype(np.float32)
        if kind == "f16 subnormal as zero":
            if dtype_name != "float16":
                return None
            z = np.where((x16 & 0x7fff) < 0x0400, np.float32(0), xf).astype(np.float32)
            return oracle.absmax(z, True, ratio)
        if kind == "ratio on the scale":
            m = oracle.absmax(xf, True, 1.0)
            s = ((m / np.float32(gmax)).astype(np.float32) * r32).astype(np.float32)
            right = oracle.absmax(xf, True, ratio)
            out = right.copy()
            for i, si in enumerate(s):
                a = fc.alpha_for_scale(si, gmax) if np.isfinite(si) and si != 0 else None
                if a is not None:
                    out[i] = a
            return out
    raise KeyError(kind)
