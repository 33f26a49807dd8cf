"""The inputs and expected outputs of test_gpu_linear_specials.py: NaN, Inf, overflowing and zero-valued weights, inputs and
biases for the five packed linears (antq_linear4, antq_linear8, antq_linear4_mm, antq_linear8_mm, antq_linear4_gemm), at the K
where a kernel pads its last load step, and exact sums planted on the edges of the one rounding to the output type.  Built here
with numpy alone so that test_linear_special_cases_host.py holds the very same arrays to their premises without a GPU.

The reference.  W[n, k] is the decoder's rule restated in numpy on the code bytes (test_gpu_linear4._yardstick for 4-bit codes,
byte_codes_cases.decode_ref for bytes): a NaN or Inf scale goes through it as IEEE says, 0 * Inf included.  The finite parts of
every case are built as the exact-sum tests build theirs -- dyadic weights, small-integer (or dyadic) x and bias -- so that every
finite partial sum is exact in any order; the expected y[m, n] then depends on no order and is made by class rules in float64:
    NaN   if a product is NaN (x NaN, W NaN, 0 * Inf either way) or the bias is NaN, or +Inf and -Inf both occur among the
          products and the bias;
    +-Inf if one sign of Inf occurs;
    else  the exact sum of the products, + 0.0 (the accumulators start at +0), + the bias, rounded once to the type.
NaN is compared by class, everything else by bits."""
import functools

import numpy as np

import byte_codes_cases as bc
from test_gpu_linear4 import _book, _round, _value, _yardstick

F32_MAX = float(np.finfo(np.float32).max)
SIG_BITS = {"float32": 24, "float16": 11, "bfloat16": 8}
BOOKS = {4: ("pot_b4_s", "olive_int"), 8: ("flint_b6_s", "olive_int_b8")}        # (plain, pair rule), all dyadic
# finite weights come from the codes whose grid value is a whole multiple of this: coarse enough that a row of K = 2080
# non-zero x stays below 2^24 units
QUANTUM = {"pot_b4_s": 0.625, "olive_int": 4.0, "flint_b6_s": 0.625, "olive_int_b8": 1.0}
# the rounding cases want weights that are powers of two: alpha = R_ALPHA 2^j.  The plain books hold 10 / 2^i or multiples of
# 5 / 128 on gmax = 10, and fl(g fl(2^j / 10)) = g 2^j / 10 for them (asserted where it is used)
R_ALPHA = {"pot_b4_s": 1.0, "olive_int": 28.0, "flint_b6_s": 1.0, "olive_int_b8": 31.75}

_ROW = dict(Ms=(1, 3, 8), NK=tuple((n, None) for n in (1, 5, 9)), knob=None, edges=(), pads=False,
            dtypes=("float32", "bfloat16", "float16"))
_MM = dict(Ms=(1, 16, 17, 33, 64), NK=tuple((n, t) for t in (1, 2, 4, 0) for n in (1, 17, 33)) + ((65, 4),), knob=22,
           edges=(15, 16, 63), pads=True, dtypes=("bfloat16", "float16"))
# unit: elements of one load unit of a lane, by code path (True: 16 bytes per lane); step: elements of K after which the
# kernel's lanes come round (row kernels: 64 lanes; mm: a chunk; gemm: a staged step); off: bytes that take the codes off a
# 16-byte boundary but keep the entry point's alignment; pads: lanes past the end of K run with clamped addresses
ENTRIES = {
    "linear4": dict(_ROW, width=4, narrow=(8, 520), wide=(32, 2080, 2048), unit={True: 32, False: 8}, step={True: 2048, False: 512}, off=4),
    "linear8": dict(_ROW, width=8, narrow=(8, 520), wide=(16, 1040, 1024), unit={True: 16, False: 8}, step={True: 1024, False: 512}, off=8),
    "linear4_mm": dict(_MM, width=4, narrow=(8, 40, 264), wide=(32, 160, 1056, 1024), unit={True: 32, False: 8}, step={True: 128, False: 32}, off=4),
    "linear8_mm": dict(_MM, width=8, narrow=(8, 40, 264), wide=(16, 80, 528, 512), unit={True: 16, False: 8}, step={True: 64, False: 32}, off=8),
    "linear4_gemm": dict(width=4, narrow=(8, 136, 264), wide=(32, 160, 256), unit={True: 32, False: 8}, step={True: 128, False: 128}, off=4,
                         Ms=(1, 65, 129, 257), NK=tuple((n, w) for w in (2, 4, 0) for n in (1, 63, 65)), knob=23,
                         edges=(63, 64, 127, 128), pads=True, dtypes=("bfloat16", "float16")),
}
SETS = tuple((e, d) for e in ENTRIES for d in ENTRIES[e]["dtypes"])
FAMILIES = ("weights", "inputs", "rounding")
DT_ALL = ("float32", "bfloat16", "float16")


def paths(entry):
    """[(K, vec)]: every K on the path it takes with aligned codes, the 16-byte-path K again with the codes offset"""
    e = ENTRIES[entry]
    wide_mod = 32 if e["width"] == 4 else 16
    assert all(k % wide_mod for k in e["narrow"]) and not any(k % wide_mod for k in e["wide"])
    return [(k, False) for k in e["narrow"]] + [(k, v) for k in e["wide"] for v in (True, False)]


def has_tail(entry, K, vec):
    return K % ENTRIES[entry]["step"][vec] != 0


def last_unit(entry, K, vec):
    """the k of the row's last load unit -- what a lane past the end of K repeats"""
    u = ENTRIES[entry]["unit"][vec]
    assert K % u == 0
    return slice(K - u, K)


class _Rounder:
    """byte_codes_cases.decode_ref asks its oracle for the bf16 rounding only"""
    f32_to_bf16 = staticmethod(lambda v: _round(v, "bfloat16"))


def book_of(width, name):
    return _book(name) if width == 4 else bc.book(name)


@functools.lru_cache(maxsize=None)
def code_classes(width, name):
    """codes of the book by the grid value they stand for: coarse positive / negative (whole multiples of the quantum), zero,
    and with the pair rule the outlier indices by sign and the identifier"""
    _, g, gmax, nn, ovp = book_of(width, name)
    normal = np.arange(nn if ovp else g.size)
    gv = g[normal].astype(np.float64)
    coarse = normal[np.round(gv / QUANTUM[name]) == gv / QUANTUM[name]]
    d = dict(pos=coarse[g[coarse] > 0], neg=coarse[g[coarse] < 0], zero=normal[gv == 0], normal=normal, ident=(15 if width == 4 else bc.IDENT))
    if ovp:
        go = g[nn:].astype(np.float64)
        assert np.array_equal(np.round(go / QUANTUM[name]), go / QUANTUM[name])
        d.update(opos=np.flatnonzero(go > 0), oneg=np.flatnonzero(go < 0))
    assert d["pos"].size and d["neg"].size and d["zero"].size
    return d


def pack(width, E):
    """code elements [N, K] -> the bytes the entry point takes (4-bit: element 2k in the low nibble)"""
    E = np.ascontiguousarray(E, np.uint8)
    return E if width == 8 else (E[:, 0::2] | (E[:, 1::2] << 4)).astype(np.uint8)


def weights(width, name, E, alpha, per_row, dtype_name):
    """the decoder's image of code elements E [N, K] as float64 (NaN and Inf as the rule gives them)"""
    bk = book_of(width, name)
    _, g, gmax, nn, ovp = bk
    N, K = E.shape
    rows, row_len = (N, K) if per_row else (1, N * K)
    if width == 4:
        b = _yardstick(pack(4, E), alpha, rows, row_len, per_row, g, gmax, nn, ovp, dtype_name)
    else:
        b = bc.decode_ref(_Rounder, E, alpha, bk, rows, row_len, dtype_name)
    return _value(np.ascontiguousarray(b).reshape(N, K), dtype_name)


def to_bits(v, dtype_name):
    """float64 values the type holds exactly -> its bits (asserted to go back to the same values)"""
    with np.errstate(all="ignore"):
        b = _round(np.asarray(v, np.float64).astype(np.float32), dtype_name)
    back = _value(b, dtype_name)
    assert np.array_equal(back, v, equal_nan=True) and np.array_equal(np.signbit(back), np.signbit(v)), "not a value of the type"
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# the expectation
# ---------------------------------------------------------------------------------------------------------------------------
def _lowbit(a):
    """exponent of the lowest set bit of every element (zero and non-finite: a large number)"""
    a = np.asarray(a, np.float64)
    ok = np.isfinite(a) & (a != 0)
    m, e = np.frexp(np.where(ok, a, 1.0))
    mi = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return np.where(ok, e - 53 + np.round(np.log2(low)), 10000.0)


def _half_up(total, dtype_name):
    """mistake (d): ties go away from zero"""
    with np.errstate(all="ignore"):
        b = _round(total.astype(np.float32), dtype_name)
        r = _value(b, dtype_name)
        if dtype_name == "float32":
            return b
        one = b.dtype.type(1)
        nxt = _value((b + one).astype(b.dtype), dtype_name)              # one step away from zero (sign-magnitude bits)
        tie = np.isfinite(r) & (np.abs(total) > np.abs(r)) & (np.abs(total) - np.abs(r) == np.abs(nxt) - np.abs(total))
    return np.where(tie, (b + one).astype(b.dtype), b)


def classes(x, W, bias=None):
    """(NaN, +Inf, -Inf) [M, N] among the products and the bias, the exact finite sum, and the sum of magnitudes"""
    f = np.float64
    xn, xp, xm, xz = np.isnan(x), x == np.inf, x == -np.inf, x == 0
    Wn, Wp, Wm, Wz = np.isnan(W), W == np.inf, W == -np.inf, W == 0
    xf, Wf = np.where(np.isfinite(x), x, 0.0), np.where(np.isfinite(W), W, 0.0)
    xpos, xneg, Wpos, Wneg = xf > 0, xf < 0, Wf > 0, Wf < 0
    mm = lambda a, b: a.astype(f) @ b.astype(f).T > 0
    ones_x, ones_w = np.ones_like(x, bool), np.ones_like(W, bool)
    nan = mm(xn, ones_w) | mm(ones_x, Wn) | mm(xp | xm, Wz) | mm(xz, Wp | Wm)
    pinf = mm(xp, Wpos | Wp) | mm(xm, Wneg | Wm) | mm(xpos, Wp) | mm(xneg, Wm)
    ninf = mm(xp, Wneg | Wm) | mm(xm, Wpos | Wp) | mm(xpos, Wm) | mm(xneg, Wp)
    total = xf @ Wf.T
    mass = np.abs(xf) @ np.abs(Wf).T
    if bias is not None:
        bf = np.where(np.isfinite(bias), bias, 0.0)
        mass = mass + np.abs(bf)[None, :]
    return nan, pinf, ninf, total, mass


def expect(x, W, bias, dtype_name, pad=None, half_up=False, saturate=False, bias_if_finite=False):
    """Expected bits [M, N] by the class rules.  pad: a slice of k whose weights are ALSO multiplied by a zero x (mistake (a));
    half_up, saturate, bias_if_finite: mistakes (d), (e), (f)."""
    nan, pinf, ninf, total, _ = classes(x, W, bias)
    if pad is not None:
        nan = nan | ~np.isfinite(W[:, pad]).all(1)[None, :]                # 0 * Inf, 0 * NaN
    total = total + 0.0                                                     # -0 products on a +0 accumulator
    if bias is not None:
        b = np.broadcast_to(bias[None, :], total.shape)
        use = ~(nan | pinf | ninf) if bias_if_finite else np.ones(total.shape, bool)
        nan, pinf, ninf = nan | (use & np.isnan(b)), pinf | (use & (b == np.inf)), ninf | (use & (b == -np.inf))
        total = total + np.where(np.isfinite(b), b, 0.0)                    # (+0) + (-0) = +0
    with np.errstate(all="ignore"):
        bits = _half_up(total, dtype_name) if half_up else _round(total.astype(np.float32), dtype_name)
    one = lambda v: _round(np.float32([v]), dtype_name)[0]
    if saturate and dtype_name == "float16":
        v = _value(bits, dtype_name)
        bits = np.where(v == np.inf, one(65504.0), np.where(v == -np.inf, one(-65504.0), bits))
    with np.errstate(all="ignore"):
        bits = np.where(pinf, one(np.inf), bits)
        bits = np.where(ninf, one(-np.inf), bits)
        bits = np.where(nan | (pinf & ninf), one(np.nan), bits)
    return bits.astype(_round(np.float32([0]), dtype_name).dtype)


def mismatches(got, want, dtype_name):
    """[M, N] bool: NaN against NaN passes, everything else is compared by bits"""
    g, w = _value(np.asarray(got), dtype_name), _value(np.asarray(want), dtype_name)
    return ~((np.isnan(g) & np.isnan(w)) | (~np.isnan(g) & ~np.isnan(w) & (np.asarray(got) == np.asarray(want))))


def assert_exact(x, W, bias, dtype_name):
    """The premise of the expectation, in float64.  No partial sum of the finite parts, in any order, exceeds the sum of their
    magnitudes, and that is at most the largest fp32: nothing overflows.  Where the class is finite, every product and the
    bias are whole multiples of one power of two (the lowest bit of the row of x times that of the row of W), and the sum of
    magnitudes is below 2^24 such units: every partial sum is exact in fp32."""
    nan, pinf, ninf, total, mass = classes(x, W, bias)
    assert mass.max() <= F32_MAX
    lx, lw = _lowbit(x).min(1), _lowbit(W).min(1)
    e = lx[:, None] + lw[None, :]
    if bias is not None:
        e = np.minimum(e, _lowbit(bias)[None, :])
    fin = ~(nan | pinf | ninf) & (mass > 0)
    units = np.where(fin, mass / np.exp2(np.where(fin, e, 0.0)), 0.0)
    assert units.max(initial=0.0) < 2.0 ** 24, units.max()
    return float(units.max(initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------------
# per-row scale kinds by n: non-finite rows interleaved with ordinary ones.  "mixed": products of both signs, so Inf - Inf;
# "ovf": float16 only, a finite scale at which the large grid values overflow the type (elsewhere: a coherent +Inf row)
PATTERN = ("+inf", "ord", "nan", "ord", "-inf", "ord", "mixed", "ovf", "ord")
BIAS_PATTERN = ("nan", None, "-inf", None, "+inf", "-0", None, None)
SPECIAL = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "-0": -0.0}


def _rng(entry, dtype_name, K, vec, family, v):
    return np.random.default_rng([list(ENTRIES).index(entry), DT_ALL.index(dtype_name), K, int(vec), FAMILIES.index(family), v, 4711])


def _shape(entry, ci):
    """(M, N, knob) of case number ci: the two lists turn at different rates, so every M meets every (N, knob)"""
    e = ENTRIES[entry]
    N, knob = e["NK"][(ci + ci // len(e["Ms"])) % len(e["NK"])]
    return e["Ms"][ci % len(e["Ms"])], N, knob


def _random_elements(rng, cc, N, K, ovp, zeros=True):
    """coarse codes; with the pair rule 2 % of the pairs hold an outlier and its victim"""
    pool = np.concatenate([cc["pos"], cc["neg"]] + ([cc["zero"]] if zeros else []))
    E = rng.choice(pool, (N, K)).astype(np.uint8)
    if ovp:
        P = E.reshape(N, K // 2, 2)
        hit = rng.random((N, K // 2)) < 0.02
        side = rng.integers(0, 2, (N, K // 2))
        out = rng.choice(np.concatenate([cc["opos"], cc["oneg"]]), (N, K // 2))
        for s in (0, 1):
            P[..., s] = np.where(hit & (side == s), cc["ident"], np.where(hit, out, P[..., s]))
    return E


def _signed(rng, cc, sign, outlier=False):
    """codes (or outlier indices) whose grid value has the sign of every element of `sign`"""
    p, n = (cc["opos"], cc["oneg"]) if outlier else (cc["pos"], cc["neg"])
    return np.where(sign > 0, rng.choice(p, sign.shape), rng.choice(n, sign.shape)).astype(np.uint8)


def _finish(entry, dtype_name, K, vec, family, ci, name, E, alpha, per_row, x, bias, knob, **meta):
    e = ENTRIES[entry]
    W = weights(e["width"], name, E, alpha, per_row, dtype_name)
    units = assert_exact(x, W, bias, dtype_name)
    _, g, gmax, nn, ovp = book_of(e["width"], name)
    c = dict(entry=entry, dtype=dtype_name, K=K, vec=vec, family=family, ci=ci, book=name, E=E, codes=pack(e["width"], E),
             alpha=np.asarray(alpha, np.float32), per_row=per_row, x=x, bias=bias, knob=knob, W=W, M=x.shape[0], N=E.shape[0],
             offset=(0 if vec or K in e["narrow"] else e["off"]), units=units,
             x_bits=to_bits(x, dtype_name), bias_bits=None if bias is None else to_bits(bias, dtype_name),
             want=expect(x, W, bias, dtype_name))
    c.update(meta)
    return c


def _ovf_exponent(width, name):
    """e: at s = 2^e the largest coarse grid values overflow float16 and the smallest stay finite"""
    _, g, gmax, nn, ovp = book_of(width, name)
    cc = code_classes(width, name)
    mags = np.abs(g[np.concatenate([cc["pos"], cc["neg"]])].astype(np.float64))
    e = int(np.ceil(np.log2(65520.0 / mags.max())))
    assert mags.max() * 2.0 ** e >= 65520 > mags.min() * 2.0 ** e
    return e


def weights_case(entry, dtype_name, K, vec, ci, v):
    """Non-finite weights.  v = 0 / 1: per-row scales by PATTERN on the plain / the pair-rule book, the last load unit of every
    non-finite row planted with non-zero grid values (set A); v = 2: the same with that unit holding zero-valued codes -- the
    duplicate zero, victims (set B); v = 3 / 4: ONE scale, +Inf / NaN.  x is non-zero everywhere, x[m, k] = tau[m] sigma[k] a, and
    a "coherent" row n holds codes of sign sigma[k] rho[n]: all its products have one sign."""
    e = ENTRIES[entry]
    width = e["width"]
    rng = _rng(entry, dtype_name, K, vec, "weights", v)
    name = BOOKS[width][v] if v < 2 else BOOKS[width][ci % 2]
    _, g, gmax, nn, ovp = book_of(width, name)
    cc = code_classes(width, name)
    M, N, knob = _shape(entry, ci)
    lu = last_unit(entry, K, vec)
    sigma = rng.choice([-1, 1], K)
    tau = 1 - 2 * (np.arange(M) % 2)
    rho = 1 - 2 * ((np.arange(N) // 3) % 2)
    x = (tau[:, None] * sigma[None, :] * rng.integers(1, 4, (M, K))).astype(np.float64)
    E = _random_elements(rng, cc, N, K, ovp)
    per_row = v < 3
    kinds = [PATTERN[n % len(PATTERN)] for n in range(N)] if per_row else [("+inf", "nan")[v - 3]] * N
    alpha = np.float32(gmax) * np.exp2(rng.integers(-2, 2, N)).astype(np.float32)
    special = []
    for n, kind in enumerate(kinds):
        if kind == "ord":
            continue
        special.append(n)
        if kind == "ovf" and dtype_name != "float16":
            kind, rho[n] = "+inf", -1
        coherent = _signed(rng, cc, sigma * rho[n])
        if kind == "ovf":
            ex = _ovf_exponent(width, name)
            mags = np.abs(g.astype(np.float64)) * 2.0 ** ex
            small = np.asarray([c for c in np.concatenate([cc["pos"], cc["neg"]]) if mags[c] < 65520])
            big_p = np.asarray([c for c in cc["pos"] if mags[c] >= 65520])
            big_n = np.asarray([c for c in cc["neg"] if mags[c] >= 65520])
            E[n] = rng.choice(small, K)
            s = sigma[lu] * rho[n]
            E[n, lu] = np.where(s > 0, rng.choice(big_p, s.size), rng.choice(big_n, s.size))
            alpha[n] = np.float32(gmax) * np.float32(2.0 ** ex)
        elif kind == "mixed":
            E[n] = _signed(rng, cc, rng.choice([-1, 1], K))
            E[n, :2] = _signed(rng, cc, sigma[:2] * np.array([1, -1]))
            E[n, lu] = _signed(rng, cc, sigma[lu] * (1 - 2 * (np.arange(lu.stop - lu.start) % 2)))
            alpha[n] = np.inf
        elif kind == "nan":
            E[n, lu] = coherent[lu]
            alpha[n] = np.nan
        else:
            E[n] = coherent
            alpha[n] = np.inf if kind == "+inf" else -np.inf
        if ovp and kind in ("nan", "ovf"):                     # an outlier and its victim in the last unit
            E[n, K - 2] = _signed(rng, cc, sigma[K - 2:K - 1] * rho[n], outlier=True)[0]
            E[n, K - 1] = cc["ident"]
        if v == 2:                                             # set B: zero-valued codes in the last unit
            z = cc["zero"][np.arange(lu.stop - lu.start) % cc["zero"].size]
            if ovp:
                z = z.copy()
                z[2::4] = cc["ident"]
                z[3::4] = _signed(rng, cc, sigma[lu][3::4] * rho[n], outlier=True)
            E[n, lu] = z
            if kind == "ovf" and K > z.size:                    # the overflowing weights at the row's start instead
                s = sigma[:z.size] * rho[n]
                E[n, :z.size] = np.where(s > 0, rng.choice(big_p, s.size), rng.choice(big_n, s.size))
    if not per_row:
        alpha = np.float32([np.inf if kinds[0] == "+inf" else np.nan])
    bias = None
    if ci % 3 != 0:
        bias = rng.integers(-8, 9, N).astype(np.float64)
        for n in range(N):
            k = BIAS_PATTERN[(n + ci) % len(BIAS_PATTERN)]
            if k is not None:
                bias[n] = SPECIAL[k]
    return _finish(entry, dtype_name, K, vec, "weights", ci, name, E, alpha, per_row, x, bias, knob,
                   special_rows=special, code_set=("B" if v == 2 else "A"), variant=v)


def boundary_positions(entry, K, vec):
    """first and last k (the last valid one before a padded tail) and both sides of every step boundary: the mm forms' chunk
    rounds (a wavefront's second chunk) start at a multiple of the step too"""
    step = ENTRIES[entry]["step"][vec]
    pos = {0, K - 1}
    for b in range(step, K, step):
        pos |= {b - 1, b}
    return sorted(pos)


def input_items(entry, K, vec):
    """[(k, kind)]: NaN, +Inf and -Inf at the first and the last k, the kinds in turn at the others"""
    pos = boundary_positions(entry, K, vec)
    kinds = ("nan", "+inf", "-inf")
    items = [(k, kinds[i % 3]) for i, k in enumerate(pos)]
    items += [(k, kind) for k in (0, K - 1) for kind in kinds if (k, kind) not in items]
    return items


def edge_rows(entry, M):
    """the rows that take a non-finite element in EVERY input case: the last one (rows m >= M are clamped onto it), the first,
    and those either side of a row-tile edge"""
    return list(dict.fromkeys([M - 1, 0] + [m for m in ENTRIES[entry]["edges"] if m < M]))


def special_rows(entry, M):
    """edge_rows first, then every third row -- so that most of them have a finite row after them in their tile"""
    return list(dict.fromkeys(edge_rows(entry, M) + list(range(2, M, 3))))


def input_cases(entry, dtype_name, K, vec, ci0):
    """Non-finite x: finite weights, small-integer x, and one NaN / +Inf / -Inf per row of special_rows at the k of input_items.
    One case per M of the entry point at least, and as many more as the items need; every case plants all of edge_rows (the
    items go round again for them once they are used up).  N >= 3, and at a planted k columns 0, 1, 2 hold a zero, a positive
    and a negative weight: an Inf x gives NaN, +Inf and -Inf there.  Every other row of x is finite."""
    e = ENTRIES[entry]
    width = e["width"]
    items = input_items(entry, K, vec)
    shapes = [nk for nk in e["NK"] if nk[0] >= 3]
    out, done, j = [], 0, 0
    while done < len(items) or j < len(e["Ms"]):
        ci = ci0 + j
        rng = _rng(entry, dtype_name, K, vec, "inputs", j)
        name = BOOKS[width][ci % 2]
        _, g, gmax, nn, ovp = book_of(width, name)
        cc = code_classes(width, name)
        M = e["Ms"][len(e["Ms"]) - 1 - j % len(e["Ms"])]            # the largest first: it takes the most items
        N, knob = shapes[(ci + j // len(e["Ms"])) % len(shapes)]
        per_row = ci % 2 == 1
        E = _random_elements(rng, cc, N, K, ovp)
        alpha = np.float32(gmax) * np.exp2(rng.integers(-2, 2, N if per_row else 1)).astype(np.float32)
        x = (rng.integers(-3, 4, (M, K)) * (rng.random((M, K)) < 0.7)).astype(np.float64)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        planted = []
        edges = edge_rows(entry, M)
        for m in special_rows(entry, M):
            if done >= len(items) and m not in edges:
                break
            k, kind = items[done % len(items)]
            done += 1
            x[m, k] = SPECIAL[kind]
            planted.append((m, k, kind))
            for n in range(3):
                E[n, k] = (cc["zero"][done % cc["zero"].size], rng.choice(cc["pos"]), rng.choice(cc["neg"]))[n]
                if ovp:                                        # (the partner of a planted k is never planted: steps are even)
                    E[n, k ^ 1] = rng.choice(cc["pos"])
        bias = rng.integers(-8, 9, N).astype(np.float64) if ci % 3 != 1 else None
        out.append(_finish(entry, dtype_name, K, vec, "inputs", ci, name, E, alpha, per_row, x, bias, knob, planted=planted))
        j += 1
    return out


def rounding_targets(dtype_name):
    """[(tag, terms)]: rows of x whose exact sum against a weight of 1 sits on an edge of the rounding.  terms: the non-zero
    x of the row; "-0": every x is -0.0."""
    t = [("zero", []), ("zero", [3.0, -3.0]), ("zero", "-0")]
    if dtype_name != "float32":
        h = 2.0 ** SIG_BITS[dtype_name]                        # ulp 2 from here: h + 1 and h + 3 are ties
        t += [("tie", [h, 1.0]), ("tie", [h, 2.0, 1.0]), ("tie", [-h, -1.0]), ("tie", [-h, -2.0, -1.0])]
    if dtype_name == "float16":                                # 65519 -> 65504, 65520 (a tie) -> Inf
        t += [("overflow", [65504.0, 15.0]), ("overflow", [65504.0, 16.0]), ("overflow", [-65504.0, -16.0])]
    return t


def bf16_overflow_targets():
    """against a weight of 2^64: 2^128 - 2^120 + 2^118 -> the largest bf16; + 2^119 instead (the tie) -> Inf.  Same-sign terms:
    every partial sum is at most the sum, which fp32 holds."""
    big = 255.0 * 2.0 ** 56
    return [("overflow", [big, 2.0 ** 54]), ("overflow", [big, 2.0 ** 55]), ("overflow", [-big, -2.0 ** 55]), ("overflow", [big, 2.0 ** 55, 2.0 ** 54])]


@functools.lru_cache(maxsize=None)
def _power_of_two_codes(width, name, dtype_name):
    """(codes whose weight at alpha = R_ALPHA is +2^i, those with -2^i, the exponents by code)"""
    cc = code_classes(width, name)
    E = np.repeat(cc["normal"].astype(np.uint8), 2)[None, :]
    W = weights(width, name, E, np.float32([R_ALPHA[name]]), True, dtype_name)[0, 0::2]
    m, ex = np.frexp(W)
    p2 = np.abs(m) == 0.5
    return cc["normal"][p2 & (W > 0)], cc["normal"][p2 & (W < 0)], dict(zip(cc["normal"].tolist(), (ex - 1).tolist()))


def rounding_cases(entry, dtype_name, K, vec, ci0):
    """Exact sums on the edges of the one rounding.  Every column holds ONE code at every k, of weight +-2^i or zero; column
    0's weight is exactly 1 (2^64 for the bf16 overflow rows), so y[m, 0] is the row's planted sum.  Each set of rows runs
    without a bias and with one whose element 0 is -0.0."""
    e = ENTRIES[entry]
    width = e["width"]
    sets = []
    t = rounding_targets(dtype_name)
    cap = max(e["Ms"])
    sets += [(t[i:i + cap], 0) for i in range(0, len(t), cap)]
    if dtype_name == "bfloat16":
        sets.append((bf16_overflow_targets(), 64))
    out, j = [], 0
    for targets, w0_exp in sets:
        for with_bias in (False, True):
            ci = ci0 + j
            rng = _rng(entry, dtype_name, K, vec, "rounding", j)
            name = BOOKS[width][ci % 2]
            cc = code_classes(width, name)
            pos, neg, ex = _power_of_two_codes(width, name, dtype_name)
            _, N, knob = _shape(entry, ci)
            per_row = w0_exp != 0 or ci % 2 == 0
            col = [pos[0]] + [(pos, neg, cc["zero"])[n % 3][n % (pos, neg, cc["zero"])[n % 3].size] for n in range(1, N)]
            E = np.repeat(np.asarray(col, np.uint8)[:, None], K, 1)
            j0 = w0_exp - ex[int(pos[0])]                      # column 0: 2^ex 2^j0 = 2^w0_exp
            jn = j0 + (rng.integers(-1, 2, N) if per_row and w0_exp == 0 else np.zeros(N, np.int64))
            jn[0] = j0
            if w0_exp:
                jn[1:] = rng.integers(-1, 2, N - 1)            # the other columns stay ordinary
            alpha = (np.float32(R_ALPHA[name]) * np.exp2(jn if per_row else jn[:1]).astype(np.float32)).astype(np.float32)
            x = np.zeros((len(targets), K))
            where = (0, K // 2, K - 1)
            for m, (tag, terms) in enumerate(targets):
                if isinstance(terms, str):
                    x[m] = -0.0
                else:
                    x[m, list(where[:len(terms)])] = terms
            bias = None
            if with_bias:
                bias = rng.integers(-8, 9, N).astype(np.float64) if w0_exp == 0 else np.zeros(N)     # (2^64 + 3 is no fp32)
                bias[0] = -0.0
            c = _finish(entry, dtype_name, K, vec, "rounding", ci, name, E, alpha, per_row, x, bias, knob, tags=[t[0] for t in targets])
            assert c["W"][0, 0] == 2.0 ** w0_exp and (c["W"][0] == c["W"][0, 0]).all()
            out.append(c)
            j += 1
    return out


@functools.lru_cache(maxsize=None)
def cases(entry, dtype_name):
    """every case of one (entry point, dtype) set, in a fixed order"""
    out = []
    for pi, (K, vec) in enumerate(paths(entry)):             # (+ pi: the shapes a path gets shift from path to path)
        ci = len(out) + 2 * pi
        out += [weights_case(entry, dtype_name, K, vec, ci + v, v) for v in range(5)]
        out += input_cases(entry, dtype_name, K, vec, len(out) + 2 * pi)
        out += rounding_cases(entry, dtype_name, K, vec, len(out) + 2 * pi)
    return out


def label(c):
    return "%s %s K=%d %s %s #%d M=%d N=%d %s %s%s%s" % (
        c["entry"], c["dtype"], c["K"], "16-byte" if c["vec"] else "narrow", c["family"], c["ci"], c["M"], c["N"], c["book"],
        "per-row" if c["per_row"] else "per-tensor", "" if c["bias"] is None else " bias", "" if c["knob"] is None else " knob=%d" % c["knob"])
