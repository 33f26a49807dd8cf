"""Input builders for the packed 4-bit encoder's edge tests (test_gpu_encode4_edges.py) and for the host test that holds the
builders themselves to their conditions with the CPU oracle alone (test_encode4_cases_host.py).  Nothing here touches the
HIP library: a builder takes numpy arrays and, where it has to classify a value, the oracle module."""
import os

import numpy as np

ULPS = 16                      # half width of a planted window, in fp32 ulps
WIN = 2 * ULPS + 1

BOOK_NAMES = ("flint_b4_s", "int_b4_s", "pot_b4_s", "flint_b4_u", "int_b3_u", "olive_flint", "olive_int")
ROW_SCALES = np.float32([1.0, 0.06, 0.0, -0.05, np.nan, np.inf, 1e-30, 1e30, 2.0 ** -60, 1e-41])


def golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), allow_pickle=False)


def books():
    """(name, grid as the kernel takes it, gmax, n_normal, pair rule): the books of test_gpu_packed._books()"""
    G, O = golden("ant_grids.npz"), golden("olive_grids.npz")
    out = [(k, np.ascontiguousarray(G[k], np.float32), float(G[k].max()), 0, False)
           for k in ("flint_b4_s", "int_b4_s", "pot_b4_s", "flint_b4_u", "int_b3_u")]
    for t in ("flint", "int"):
        gn, go = O["%s_b4_s" % t], O["outlier_b4_s"]
        out.append(("olive_" + t, np.ascontiguousarray(np.concatenate([gn, go]), np.float32), float(gn.max()), int(gn.size), True))
    return out


def book(name):
    return [b for b in books() if b[0] == name][0]


def zero_code(g, n_normal, ovp):
    z = np.flatnonzero((g[:n_normal] if ovp else g) == 0)
    return int(z[-1]) if z.size else 0


def codes_want(oracle, ridx, n_normal, ovp, zc):
    """The code of every element from the oracle's scan-order indices: an outlier is its index in the outlier list, a victim
    the identifier 15, no entry within the scan's horizon the code of the grid's zero."""
    want = ridx.astype(np.int64).copy()
    if ovp:
        want[ridx >= n_normal] -= n_normal
    want[ridx == oracle.IDX_VICTIM] = 15
    want[ridx == oracle.IDX_NONE] = zc
    return want


def oracle_codes(oracle, x, alpha, g, gmax, n_normal, ovp, pair_rule=None):
    """x: float32 [rows, row_len] as the encoder sees it (a 16-bit tensor widened exactly); alpha: one per row, or one."""
    pair_rule = ovp if pair_rule is None else pair_rule
    with np.errstate(all="ignore"):
        _, ridx = oracle.forward(np.ascontiguousarray(x, np.float32), alpha, g, gmax, pair_rule)
    return codes_want(oracle, ridx, n_normal, ovp, zero_code(g, n_normal, ovp))


def awkward_alpha(rng, n):
    return (np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n)) * rng.uniform(1.0, 2.0, n)).astype(np.float32)


def midpoints(g):
    """(midpoints of adjacent distinct grid values in float64, True where the two values differ in the pair rule's |v| > 32)"""
    gs = np.unique(np.asarray(g, np.float32) + np.float32(0))
    return (gs[:-1].astype(np.float64) + gs[1:]) / 2, (np.abs(gs[:-1]) > 32) != (np.abs(gs[1:]) > 32)


def ulp_window(c, k=ULPS):
    """The 2k + 1 floats from k ulps below to k ulps above |c| in magnitude, with c's sign; c is a normal, non-zero float32."""
    c = np.float32(c)
    bits = np.abs(c).view(np.uint32).astype(np.int64) + np.arange(-k, k + 1, dtype=np.int64)
    return bits.astype(np.uint32).view(np.float32) * np.sign(c)


def ulp_step(c, k):
    c = np.float32(c)
    return np.uint32(np.abs(c).view(np.uint32).astype(np.int64) + k).view(np.float32) * np.sign(c)


def centres(g, scale):
    """fl(midpoint * scale) of every pair of adjacent distinct values, those that round to 0 left out"""
    mids, edge = midpoints(g)
    c = (mids * float(scale)).astype(np.float32)
    keep = c != 0
    return c[keep], edge[keep]


def lay_out(rng, payloads, alpha, row_len, fill_sd, unsigned=False):
    """One payload (a flat float32 array) per scale -> x [rows, row_len] in which scale i owns as many consecutive rows as its
    payload needs, the payload at a random octet-aligned offset inside them and Gaussian data around it.  Returns
    (x, alpha per row, flat start of every payload)."""
    rps = max(1, max((p.size + row_len - 1) // row_len for p in payloads))
    n = len(payloads)
    a_rows = np.repeat(np.asarray(alpha, np.float32), rps)
    with np.errstate(all="ignore"):
        sd = np.nan_to_num(np.abs(np.asarray(fill_sd, np.float32)), nan=1.0, posinf=1.0)
    sd = np.where((sd > 1e-30) & (sd < 1e30), sd, np.float32(1.0)).astype(np.float32)
    x = (rng.standard_normal((n * rps, row_len)) * np.repeat(sd, rps)[:, None]).astype(np.float32)
    if unsigned:
        x = np.abs(x)
    flat = x.reshape(-1)
    starts = np.empty(n, np.int64)
    span = rps * row_len
    for i, p in enumerate(payloads):
        off = int(rng.integers(0, (span - p.size) // 8 + 1)) * 8
        starts[i] = i * span + off
        flat[starts[i]:starts[i] + p.size] = p
    return x, a_rows, starts


# ---------------------------------------------------------------------------------------------------------------------------
# 2a: windows around every threshold
# ---------------------------------------------------------------------------------------------------------------------------
def threshold_case(rng, g, gmax, row_len, n_scales=64, alpha=None):
    """+/-16 ulps around fl(midpoint * scale) of every pair of adjacent distinct grid values, for n_scales awkward scales.
    Returns dict(x, alpha, windows): windows is [n, 2] (flat start, length)."""
    alpha = awkward_alpha(rng, n_scales) if alpha is None else np.asarray(alpha, np.float32)
    scale = (alpha / np.float32(gmax)).astype(np.float32)
    payloads, counts = [], []
    for s in scale:
        c, _ = centres(g, s)
        order = rng.permutation(c.size)
        payloads.append(np.concatenate([ulp_window(c[k]) for k in order]).astype(np.float32))
        counts.append(c.size)
    x, a_rows, starts = lay_out(rng, payloads, alpha, row_len, alpha / 3, unsigned=bool(g.min() >= 0))
    windows = np.array([(starts[i] + WIN * k, WIN) for i in range(len(payloads)) for k in range(counts[i])], np.int64)
    return dict(x=x, alpha=a_rows, windows=windows)


def windows_straddle(oracle, case, g, gmax):
    """How many windows hold two different oracle indices (the pair rule off: the bare decisions), and how many there are."""
    with np.errstate(all="ignore"):
        _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, False)
    flat = ridx.reshape(-1)
    good = sum(1 for st, ln in case["windows"] if np.unique(flat[st:st + ln]).size >= 2)
    return good, len(case["windows"])


# ---------------------------------------------------------------------------------------------------------------------------
# 2a, second layout: the pair rule around the normal | outlier boundary
# ---------------------------------------------------------------------------------------------------------------------------
PAIR_FORMS = ("normal/normal", "outlier/normal", "normal/outlier", "outlier/outlier")
PAIR_STEPS = (1, 4, ULPS)


def pair_case(rng, g, gmax, n_normal, row_len, n_scales=64):
    """Octets in which one pair (position 0..3) is built from the windows around the two boundary midpoints (the positive one
    and its negative): each of the four forms at each position, the members k ulps inside / outside the boundary for k in
    PAIR_STEPS, and once more with one member far from it.  Returns dict(x, alpha, pairs): pairs is [n, 2] (flat index of
    the pair's even element, position in its octet); at least one member of every listed pair lies inside a window."""
    alpha = awkward_alpha(rng, n_scales)
    scale = (alpha / np.float32(gmax)).astype(np.float32)
    normal_far, outlier_far = np.float32(np.abs(g[:n_normal]).max() * 0.5), np.float32(np.abs(g[n_normal:]).min() * 1.4)
    payloads, where = [], []
    for s in scale:
        c, edge = centres(g, s)
        octs, poss = [], []
        for cen in c[edge]:
            for pos in range(4):
                for form in range(4):
                    for k in PAIR_STEPS + (-1,):
                        o = (rng.standard_normal(8) * float(gmax) * float(s) / 4).astype(np.float32)
                        out0, out1 = form in (1, 3), form in (2, 3)
                        kk = ULPS if k < 0 else k
                        e0 = ulp_step(cen, kk if out0 else -kk)
                        e1 = ulp_step(cen, kk if out1 else -kk)
                        if k < 0:          # one member far from the boundary, the other in the window
                            far = np.float32(np.sign(cen)) * np.float32(s) * (outlier_far if out1 else normal_far)
                            e1 = far
                        o[2 * pos], o[2 * pos + 1] = e0, e1
                        octs.append(o)
                        poss.append(pos)
        order = rng.permutation(len(octs))
        payloads.append(np.concatenate([octs[k] for k in order]).astype(np.float32))
        where.extend(poss[k] for k in order)
    x, a_rows, starts = lay_out(rng, payloads, alpha, row_len, alpha / 4)
    pairs, w = [], 0
    for i, p in enumerate(payloads):
        for k in range(p.size // 8):
            pairs.append((starts[i] + 8 * k + 2 * where[w], where[w]))
            w += 1
    return dict(x=x, alpha=a_rows, pairs=np.array(pairs, np.int64))


def pair_forms_present(oracle, case, g, gmax, n_normal):
    """The set of (form, position) over the listed pairs, from the oracle's bare decisions (pair rule off)."""
    with np.errstate(all="ignore"):
        _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, False)
    flat = ridx.reshape(-1)
    seen = set()
    for at, pos in case["pairs"]:
        assert at % 8 == 2 * pos
        seen.add((int(flat[at] >= n_normal) + 2 * int(flat[at + 1] >= n_normal), int(pos)))
    return seen


# ---------------------------------------------------------------------------------------------------------------------------
# 2b: magnitudes, specials, scales
# ---------------------------------------------------------------------------------------------------------------------------
MANTISSAS = (0x000000, 0x000001, 0x2aaaaa, 0x400000, 0x7fffff)
SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x00000001, 0x80000001,
                     0x007fffff, 0x807fffff], np.uint32).view(np.float32)


def none_edge(oracle, alpha, g, gmax, sign):
    """The magnitude at which the oracle's index of sign * x turns into IDX_NONE under this scale, by bisection on the bit
    pattern: (lo, hi) adjacent floats with different answers, or None when the answer is the same at both ends of the finite
    range (a scale of 0, NaN, Inf ... has no such edge)."""
    def is_none(bits):
        v = np.array([[np.uint32(bits).view(np.float32) * np.float32(sign)]], np.float32)
        with np.errstate(all="ignore"):
            _, j = oracle.forward(v, np.float32(alpha), g, gmax, False)
        return bool(j[0, 0] == oracle.IDX_NONE)
    lo, hi = 1, 0x7f7fffff
    f_lo, f_hi = is_none(lo), is_none(hi)
    if f_lo == f_hi:
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if is_none(mid) == f_lo:
            lo = mid
        else:
            hi = mid
    assert is_none(lo) == f_lo and is_none(hi) == f_hi and hi - lo == 1
    return np.uint32(lo).view(np.float32), np.uint32(hi).view(np.float32)


def magnitude_case(oracle, rng, g, gmax, row_len, alphas=ROW_SCALES):
    """Per scale: both signs of every fp32 exponent with the mantissas above (denormals are exponent 0), the specials, and
    +/-16 ulps around the magnitude where the index turns into IDX_NONE, for either sign.  Returns dict(x, alpha, edges,
    spans): edges[i] = {sign: (lo, hi) or None}; spans[i] = (flat start, length) of scale i's payload."""
    unsigned = bool(g.min() >= 0)
    e = np.arange(255, dtype=np.uint32)[:, None] << 23
    mag = (e | np.array(MANTISSAS, np.uint32)[None, :]).reshape(-1)
    sweep = np.concatenate([mag, mag | np.uint32(0x80000000)]).view(np.float32)
    payloads, edges = [], []
    for a in alphas:
        ed, parts = {}, [sweep, SPECIALS]
        for sign in (1, -1):
            ed[sign] = none_edge(oracle, a, g, gmax, sign)
            if ed[sign] is not None:
                parts.append(ulp_window(ed[sign][1] * np.float32(sign)))
        edges.append(ed)
        p = np.concatenate(parts).astype(np.float32)
        p = np.concatenate([p, np.zeros(-p.size % 8, np.float32)])
        payloads.append(p[rng.permutation(p.size)])
    x, a_rows, starts = lay_out(rng, payloads, alphas, row_len, alphas, unsigned=False)
    spans = np.array([(starts[i], payloads[i].size) for i in range(len(payloads))], np.int64)
    return dict(x=x, alpha=a_rows, edges=edges, spans=spans)


FAR = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7e000000, 0xfe000000, 0xffc00001], np.uint32).view(np.float32)


def split_octet_case(rng, g, gmax, row_len, n_scales=16):
    """Octets of which one half (4 elements) holds NaN / Inf / far-clipped values -- all four, or just one of them -- and the
    other half values of a threshold window: the two lanes that share an fp32 octet in the row encoder take different paths.
    Returns dict(x, alpha, halves): halves is [n, 2] (flat start of a window half, of a special half)."""
    alpha = awkward_alpha(rng, n_scales)
    scale = (alpha / np.float32(gmax)).astype(np.float32)
    payloads, marks = [], []
    for s in scale:
        c, _ = centres(g, s)
        octs, mk = [], []
        n = 0
        for cen in c:
            w = ulp_window(cen)
            w = np.concatenate([w, w[:3]])                     # 36 values: 9 halves
            for h in range(9):
                win = w[4 * h:4 * h + 4]
                sp = FAR[(n + np.arange(4)) % FAR.size].copy()
                if n % 3 == 2:                                 # a half with one special among window values
                    sp[:3] = w[(4 * h + 5 + np.arange(3)) % w.size]
                first = n % 2 == 0
                octs.append(np.concatenate([win, sp] if first else [sp, win]))
                mk.append((0, 4) if first else (4, 0))
                n += 1
        payloads.append(np.concatenate(octs).astype(np.float32))
        marks.append(mk)
    x, a_rows, starts = lay_out(rng, payloads, alpha, row_len, alpha / 3, unsigned=bool(g.min() >= 0))
    halves = np.array([(starts[i] + 8 * k + a, starts[i] + 8 * k + b) for i, mk in enumerate(marks) for k, (a, b) in enumerate(mk)], np.int64)
    return dict(x=x, alpha=a_rows, halves=halves)


# ---------------------------------------------------------------------------------------------------------------------------
# 2c / 2d: shapes
# ---------------------------------------------------------------------------------------------------------------------------
TASK = 4096                    # elements of one task of the element encoder (256 lanes x 2 octets)
SHAPES_F32 = [(3, 8), (5, 24), (7, 72), (64, 64), (33, 200),
              (3, 504), (3, 512), (3, 520), (2, 1016), (2, 1024), (2, 1032), (1, 2056),
              ((TASK - 8) // 8, 8), (TASK // 8, 8), ((TASK + 8) // 8, 8),
              # rows of 24: 4096 is no multiple of 24, so one octet over one task, one short of two, and three whole tasks
              ((TASK + 8) // 24, 24), ((2 * TASK - 8) // 24, 24), (3 * TASK // 24, 24)]
SHAPES_16 = SHAPES_F32 + [(3, 1016), (3, 1024), (3, 1032)]
PER_TENSOR_SHAPE = (8, 72)
LOOP_SHAPE = (441, 64)         # 6.9 tasks of the element encoder: 7 tasks, the last one partial
BIG_SHAPE = (131080, 64)       # 2049 tasks: with 2048 persistent workgroups exactly one of them loops
PARTIAL_SHAPES = [(5, 24), (7, 72), (33, 200), (3, 520), (2, 1016), (2, 1032), (1, 2056), ((TASK + 8) // 8, 8)]
PARTIAL_SHAPES_16 = PARTIAL_SHAPES + [(3, 1016), (3, 1032)]


def random_case(rng, rows, row_len, g, gmax, ovp, per_row=True):
    """Gaussian data on per-row scales, clipped to twice the outermost value; with the pair rule 5 % of the pairs hold an
    outlier, a third of those two."""
    a = np.exp(rng.uniform(-5, 1, rows if per_row else 1)).astype(np.float32)
    s = (a / np.float32(gmax)).astype(np.float32)
    lim = 1.9 * float(np.abs(g).max())
    d = rng.standard_normal((rows, row_len)).astype(np.float32) * np.float32(0.3 * gmax)
    if ovp:
        big = rng.random((rows, row_len // 2)) < 0.05
        both = big & (rng.random((rows, row_len // 2)) < 0.3)
        d2 = d.reshape(rows, row_len // 2, 2)
        side = rng.integers(0, 2, (rows, row_len // 2))
        mag = rng.uniform(1.2 * gmax, lim, (rows, row_len // 2, 2)).astype(np.float32)
        for k in (0, 1):
            m = (big & (side == k)) | both
            d2[..., k] = np.where(m, mag[..., k] * np.sign(d2[..., k] + 1e-9), d2[..., k])
    d = np.clip(np.abs(d) if g.min() >= 0 else d, -lim, lim)
    x = (d * (s[:, None] if per_row else s[0])).astype(np.float32)
    return dict(x=x, alpha=a)


def as_dtype(oracle, x, dtype_name):
    """(the tensor's bits as the kernels take them, the same values as float32 for the oracle)"""
    if dtype_name == "bfloat16":
        h = oracle.f32_to_bf16(x)
        return h, oracle.bf16_to_f32(h)
    if dtype_name == "float16":
        with np.errstate(all="ignore"):
            h = x.astype(np.float16)
        return h.view(np.uint16), h.astype(np.float32)
    return x, x


# ---------------------------------------------------------------------------------------------------------------------------
# 2e: arbitrary codebooks
# ---------------------------------------------------------------------------------------------------------------------------
def _values(rng, m, lo, hi, signed=True):
    """m values with lo <= |v| <= hi (lo may be 0): uniform, geometric, evenly spaced or quarter steps"""
    kind = int(rng.choice([0, 1, 2, 3, 4, 4, 4]))
    if kind == 4:
        # a ladder like the reference's own books: neighbouring magnitudes within a factor of two, both signs, zero(s)
        k = max(1, m // 2 if signed else m)
        mags = hi / rng.uniform(1.3, 1.9) ** np.arange(k)
        mags = mags[mags >= max(lo, 1e-3)]
        v = np.concatenate([-mags, mags] if signed else [mags])[:m]
        v = np.concatenate([v, np.full(m - v.size, 0.0 if lo == 0 else mags[0])])
        return np.sort(v).astype(np.float32)
    if kind == 0:
        v = rng.uniform(lo, hi, m)
    elif kind == 1:
        v = np.exp(rng.uniform(np.log(max(lo, 0.05)), np.log(hi), m))
    elif kind == 2:
        v = lo + (hi - lo) * (np.arange(m) + rng.uniform(0, 1)) / m
    else:
        v = np.clip(np.round(rng.uniform(lo, hi, m) * 4) / 4, lo, hi)
    if signed:
        v = v * np.where(rng.random(m) < 0.5, -1.0, 1.0)
    return v.astype(np.float32)


def _spice(rng, g, lo, hi):
    """order, duplicates, signed zeros, two entries one ulp apart"""
    m = g.size
    if rng.random() < 0.6:
        g = np.sort(g)
    if rng.random() < 0.4 and m > 3:
        g[rng.integers(0, m)] = g[rng.integers(0, m)]
    if rng.random() < 0.3 and m > 1:
        i, j = rng.choice(m, 2, replace=False)
        v = ulp_step(g[i], 1) if g[i] != 0 and np.abs(ulp_step(g[i], 1)) <= hi else g[i]
        if np.abs(v) >= lo:
            g[j] = v
    if lo == 0:
        if rng.random() < 0.4:
            g[rng.integers(0, m)] = -0.0
        if rng.random() < 0.4:
            g[rng.integers(0, m)] = 0.0
    return g.astype(np.float32)


def random_book(rng, ovp):
    """(grid, gmax, n_normal): a plain book of 2 .. 16 values, or n_normal in 1 .. 15 normal values (|v| <= 32) followed by
    1 .. 15 outliers (|v| > 32)."""
    if not ovp:
        m = int(rng.integers(2, 17))
        hi = float(rng.choice([1.0, 12.0, 40.0, 400.0]))
        g = _spice(rng, _values(rng, m, 0.0, hi, signed=bool(rng.random() < 0.8)), 0.0, hi)
        if not (g.max() > 0):
            g[-1] = np.float32(1.5)
        return g, float(g.max()), 0
    nn, no = int(rng.integers(1, 16)), int(rng.integers(1, 16))
    gn = _spice(rng, _values(rng, nn, 0.0, 32.0), 0.0, 32.0)
    if not (gn.max() > 0):
        gn[-1] = np.float32(rng.choice([32.0, 7.5]))
    go = _spice(rng, _values(rng, no, 32.5, float(rng.choice([64.0, 400.0]))), 32.5, 400.0)
    return np.concatenate([gn, go]).astype(np.float32), float(gn.max()), nn


def book_well_formed(g, gmax, n_normal, ovp):
    g = np.asarray(g)
    if g.dtype != np.float32 or not np.isfinite(g).all() or not gmax > 0:
        return False
    if not ovp:
        return 2 <= g.size <= 16 and n_normal == 0
    gn, go = g[:n_normal], g[n_normal:]
    return 1 <= gn.size <= 15 and 1 <= go.size <= 15 and bool((np.abs(gn) <= 32).all()) and bool((np.abs(go) > 32).all())


def fuzz_seeds(default=6):
    return int(os.environ.get("ANTQ_FUZZ_SEEDS", default))


FUZZ_BASE = 78300            # (with it the six default seeds meet every plan kind the builder has, see the GPU test)


def fuzz_books_rng(seed):
    """Per seed two plain and two pair-rule books, each from a generator of its own: [(pair rule, generator)].  The book is
    the generator's first draw (random_book), the data of FUZZ_SHAPES in order the following ones (fuzz_case)."""
    return [(ovp, np.random.default_rng(FUZZ_BASE + 10 * seed + k)) for k, ovp in enumerate((False, False, True, True))]


FUZZ_SHAPES = [((5, 40), "float32"), ((16, 200), "float32"), ((3, 520), "float32"), ((2, 1032), "float32"), ((3, 1032), "bfloat16")]


def fuzz_case(rng, g, gmax, rows, row_len):
    """make_x-style data (a few large elements, NaN, Inf, -3e30, signed zeros, a denormal) on random scales, and +/-16-ulp
    windows around as many of the book's midpoints as fit into each row behind the specials."""
    x = (rng.standard_normal((rows, row_len)) * 0.02).astype(np.float32)
    f = x.reshape(-1)
    f[::53] *= 9
    f[5], f[7], f[9], f[11], f[13], f[15] = np.nan, np.inf, -3e30, 0.0, -0.0, 1e-41
    am = np.abs(np.nan_to_num(x, nan=0, posinf=0, neginf=0))
    am[am > 1e10] = 0
    alpha = (am.max(1) * rng.uniform(0.1, 1.2, rows) + 1e-6).astype(np.float32)
    scale = (alpha / np.float32(gmax)).astype(np.float32)
    windows = []
    for r in range(rows):
        c, _ = centres(g, scale[r])
        c = c[np.abs(c) > 1e-30]
        n = min(c.size, (row_len - 16) // WIN)
        for k, ci in enumerate(rng.choice(c.size, n, replace=False) if n else []):
            at = 16 + k * WIN
            x[r, at:at + WIN] = ulp_window(c[ci])
            windows.append((r * row_len + at, WIN))
    return dict(x=x, alpha=alpha, windows=np.array(windows, np.int64).reshape(-1, 2))
