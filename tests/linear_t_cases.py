"""The tile rule of antq_linear4_t (include/antq.h, csrc/antq_k_linear_t.h) restated in numpy, and the inputs of its GPU tests
(test_gpu_linear4_t.py), built here so that test_linear_t_cases_host.py holds the very same arrays to their premises on the
CPU.  Nothing here touches the HIP library or torch.

The rule: 128 partial sums, partial sum P an fp32 fused-multiply-add chain over k = P, P + 128, ... < K from +0; one fixed
tree over the 128; the bias added in fp32; one rounding to the type.  `tile_rule` is that text and nothing else: the GPU test
compares bits with it, without a tolerance.  ORDERS also names other fixed orders a kernel could have, for the host test to
show that the cases tell them apart.

Also here, moved from test_gpu_linear4_t.py: the decode rule of include/antq.h on the code bytes (yardstick / image_bits),
the roundings to the three types, and the order-free exact-sum case."""
import numpy as np

import encode4_cases as ec

DTYPES = ("float32", "bfloat16", "float16")
PREC = {"float32": 23, "float16": 10, "bfloat16": 7}
PHASES = 128                             # partial sums of the rule
STAGED_K = 8192                          # the most scales the kernel stages in LDS (kLinTScales): beyond, a lane divides per step
RULE_K = (8, 72, 128, 136, 520, 1600, 8192, 8200)      # 8192: the last staged K, 8200 the first unstaged one
RULE_N = (8, 40)                         # a partial tile of 32 columns; one whole tile and a partial one
RULE_ROWS = 8
RULE_BOOKS = ("flint_b4_s", "olive_flint")
RULE_M = (1, 2, 3, 8)                    # rows 1 .. 2 and rows >= 3 keep different numbers of steps in flight

books, book = ec.books, ec.book


# ---------------------------------------------------------------------------------------------------------------------------
# the types, and the decoder's rule
# ---------------------------------------------------------------------------------------------------------------------------
def round_bits(v, dtype_name):
    """fp32 -> the output type's bits, round to nearest even"""
    v = np.ascontiguousarray(v, np.float32)
    if dtype_name == "float32":
        return v.view(np.uint32)
    if dtype_name == "float16":
        with np.errstate(all="ignore"):
            return v.astype(np.float16).view(np.uint16)
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def value(bits, dtype_name):
    """the output type's bits -> float64"""
    if dtype_name == "float32":
        return bits.view(np.float32).astype(np.float64)
    if dtype_name == "float16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def value32(bits, dtype_name):
    """the output type's bits -> float32 (exact for all three types)"""
    return value(np.ascontiguousarray(bits), dtype_name).astype(np.float32)


def yardstick(codes, alpha, rows, row_len, per_row, g, gmax, n_normal, ovp, dtype_name):
    """include/antq.h restated on the code bytes: element 2j in the low nibble; with the pair rule nibble 15 -> 0 and its
    partner read from the outlier list; value = fl((g[c] + 0) * (alpha / gmax)) rounded to the output type.  Returns bits."""
    gp = np.zeros(48, np.float32)
    gp[:g.size] = g
    gp = gp + np.float32(0)
    b = np.asarray(codes, np.uint8).reshape(-1).astype(np.int64)
    c0, c1 = b & 15, b >> 4
    if ovp:
        q0 = np.where(c0 == 15, np.float32(0), np.where(c1 == 15, gp[n_normal + c0], gp[c0]))
        q1 = np.where(c1 == 15, np.float32(0), np.where(c0 == 15, gp[n_normal + c1], gp[c1]))
    else:
        q0, q1 = gp[c0], gp[c1]
    q = np.stack([q0, q1], 1).astype(np.float32).reshape(rows, row_len)
    with np.errstate(all="ignore"):
        s = (np.asarray(alpha, np.float32).reshape(-1) / np.float32(gmax)).astype(np.float32)
        v = (q * (s.reshape(rows, 1) if per_row else s[0])).astype(np.float32)
    return round_bits(v, dtype_name).reshape(rows, row_len)


def image_bits(codes, alpha, K, N, per_row, book, dtype_name):
    """the yardstick's image of K rows of N codes as [K, N] bits"""
    name, g, gmax, nn, ovp = book
    return yardstick(codes, alpha, K if per_row else 1, N if per_row else K * N, per_row, g, gmax, nn, ovp, dtype_name).reshape(K, N)


def random_codes(rng, n_bytes, ovp):
    c = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    if ovp:
        c[rng.random(n_bytes) < 0.02] = 0xFF
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# order-free exact sums
# ---------------------------------------------------------------------------------------------------------------------------
def lowest_bit_exponent(t):
    """exponent of the lowest set bit of every nonzero float64 in t"""
    m, e = np.frexp(t[t != 0])
    mi = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)


def exact_case(rng, K, book, dtype_name, per_row, N):
    """Codes [K, N], power-of-two scales and small-integer x (8 rows) for which every product and every partial sum, in any
    order, is an integer below 2^24 in units of one power of two -- asserted here in float64 -- with the exact result.  A
    prefix of the columns is a narrower layer with the same property."""
    name, g, gmax, nn, ovp = book
    codes = random_codes(rng, K * N // 2, ovp)
    j = rng.integers(-2, 2, K if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = value(image_bits(codes, alpha, K, N, per_row, book, dtype_name), dtype_name)     # [K, N]
    bias = rng.integers(-8, 9, N).astype(np.float64)
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (8, K)).astype(np.float64) * (rng.random((8, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        terms = x[:, :, None] * W[None, :, :]                          # [8, K, N]
        nz = np.abs(terms[terms != 0])
        unit = 2.0 ** min(int(lowest_bit_exponent(terms).min()), 0)    # (the bias: whole numbers)
        mass = (np.abs(terms).sum(1) + np.abs(bias)[None, :]) / unit
        if mass.max() < 2.0 ** 24:
            break
        density *= 0.5
    # the premise, in float64: every term a whole multiple of the unit, and the sum of magnitudes below 2^24 units -- a
    # fortiori below 2^24 in units of the smallest nonzero |term|
    assert np.array_equal(terms / unit, np.round(terms / unit)) and mass.max() < 2.0 ** 24
    assert ((np.abs(terms).sum(1) + np.abs(bias)[None, :]) / nz.min()).max() < 2.0 ** 24
    y = terms.sum(1)                                                    # exact in float64: < 2^24 units
    return codes, alpha, x, bias, y, density


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------
def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def fma32(x, w, acc):
    """fl32(x * w + acc), correctly rounded, elementwise on float32 arrays.  The product of two fp32 numbers has 48
    significant bits and an exponent far inside float64's range: it is exact there.  The float64 sum of product and addend
    is rounded, so TwoSum recovers its residual and the sum is made round-to-odd from it (where the residual is not zero
    and the sum's last bit is even, the float64 neighbour on the residual's side is taken: it is odd).  A round-to-odd value
    of 53 bits rounds to 24 bits -- or to an fp32 subnormal's fewer -- as the exact sum does: one rounding."""
    p = _f32(x).astype(np.float64) * _f32(w).astype(np.float64)
    a = _f32(acc).astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + a
        t = s - p
        r = (p - (s - t)) + (a - t)                                     # s + r == p + a exactly (finite operands)
        fix = np.isfinite(s) & np.isfinite(r) & (r != 0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(r > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(np.float32)


def fma32_twice_rounded(x, w, acc):
    """What fma32 must NOT be: the float64 sum rounded to nearest, then to float32 -- wrong where the float64 rounding lands on
    an fp32 midpoint (test_linear_t_cases_host.py plants such triples)."""
    with np.errstate(all="ignore"):
        return (_f32(x).astype(np.float64) * _f32(w).astype(np.float64) + _f32(acc).astype(np.float64)).astype(np.float32)


def partial_sums(xv, Wv, dtype_name, phases=PHASES):
    """xv [M, K], Wv [K, N] float32 (the type's values widened) -> [M, N, phases] float32: partial sum P is the fma32 chain
    over k = P, P + phases, ... < K in rising order from +0; a phase with no k stays +0.  Vectorised over (m, n, P), a loop
    over the steps.  bfloat16 / float16 operands: their product is exact in fp32, so the fused multiply-add is a plain fp32
    add of it -- asserted at every step, not assumed."""
    xv, Wv = _f32(xv), _f32(Wv)
    (M, K), N = xv.shape, Wv.shape[1]
    assert Wv.shape[0] == K
    acc = np.zeros((M, N, phases), np.float32)
    for k0 in range(0, K, phases):
        n = min(phases, K - k0)
        xs = np.broadcast_to(xv[:, None, k0:k0 + n], (M, N, n))
        ws = np.broadcast_to(Wv[k0:k0 + n, :].T[None, :, :], (M, N, n))
        new = fma32(xs, ws, acc[:, :, :n])
        if dtype_name != "float32":
            p32 = xs * ws
            assert np.array_equal(p32.astype(np.float64), xs.astype(np.float64) * ws.astype(np.float64)), "a product inexact in fp32"
            assert np.array_equal((p32 + acc[:, :, :n]).view(np.uint32), new.view(np.uint32))
        acc[:, :, :n] = new
    return acc


def _tree_header(p):
    """include/antq.h: P = 16 w + p; the 16 of a wavefront as four groups of four, each (p0 + p2) + (p1 + p3); the groups as
    (g0 + g1) + (g2 + g3); the wavefronts as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))"""
    q = p.reshape(p.shape[:-1] + (8, 4, 4))
    g = (q[..., 0] + q[..., 2]) + (q[..., 1] + q[..., 3])
    w = (g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])
    return ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])) + ((w[..., 4] + w[..., 5]) + (w[..., 6] + w[..., 7]))


def _tree_groups_01_23(p):
    """the groups of four paired with their neighbours: (p0 + p1) + (p2 + p3) -- a DPP step pairing lanes 4 apart first"""
    q = p.reshape(p.shape[:-1] + (8, 4, 4))
    g = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    w = (g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])
    return ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])) + ((w[..., 4] + w[..., 5]) + (w[..., 6] + w[..., 7]))


def _tree_waves_left_to_right(p):
    """the eight wavefront sums added one after the other"""
    q = p.reshape(p.shape[:-1] + (8, 4, 4))
    g = (q[..., 0] + q[..., 2]) + (q[..., 1] + q[..., 3])
    w = (g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])
    v = w[..., 0]
    for i in range(1, 8):
        v = v + w[..., i]
    return v


# name -> (phases, tree over them); "header" is the rule, the others are orders a kernel must not have
ORDERS = {
    "header": (PHASES, _tree_header),
    "groups_01_23": (PHASES, _tree_groups_01_23),
    "waves_left_to_right": (PHASES, _tree_waves_left_to_right),
    "one_chain": (1, lambda p: p[..., 0]),                      # one fma chain over all k in rising order
}
ALTERNATIVES = tuple(o for o in ORDERS if o != "header")


def rule_sums(x, W, dtype_name, order="header", partials=None):
    """the fp32 sum [M, N] before the bias, of x [M, K] and W [K, N] given as the type's bits"""
    phases, tree = ORDERS[order]
    if partials is None:
        partials = partial_sums(value32(x, dtype_name), value32(W, dtype_name), dtype_name, phases)
    assert partials.shape[-1] == phases and partials.dtype == np.float32
    return np.ascontiguousarray(tree(partials), np.float32)


def finish(sums, bias, dtype_name):
    """the bias (the type's bits, or None) added in fp32, one rounding to the type: bits"""
    v = _f32(sums)
    if bias is not None:
        v = v + value32(bias, dtype_name)[None, :]
    return round_bits(v, dtype_name)


def tile_rule(x, W, bias, dtype_name, order="header"):
    """The bits of y = x . W (+ bias) by the tile rule.  x [M, K], W [K, N] (the yardstick's image) and bias [N] or None are
    the type's bits."""
    return finish(rule_sums(x, W, dtype_name, order), bias, dtype_name)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def encode_nearest(w, alpha, per_row, bk):
    """Code bytes [K, N / 2] of w [K, N]: the book's nearest value to w / (alpha / gmax); with the pair rule an element beyond
    the midpoint of the largest normal and the smallest outlier value takes the nearest outlier's index and makes its partner
    the victim (15) -- of two such elements in a pair the larger one.  A plain encoder for test data: the image the tests use
    is whatever the yardstick reads from these bytes."""
    name, g, gmax, nn, ovp = bk
    K, N = w.shape
    s = (np.asarray(alpha, np.float32).reshape(-1) / np.float32(gmax)).astype(np.float64)
    t = w.astype(np.float64) / (s.reshape(K, 1) if per_row else s[0])
    normal = g[:nn].astype(np.float64) if ovp else g.astype(np.float64)
    code = np.abs(t[:, :, None] - normal[None, None, :]).argmin(-1)
    if ovp:
        out = g[nn:].astype(np.float64)
        edge = (np.abs(normal).max() + np.abs(out).min()) / 2
        ocode = np.abs(t[:, :, None] - out[None, None, :]).argmin(-1)
        pair_t, pair_c, pair_o = t.reshape(K, N // 2, 2), code.reshape(K, N // 2, 2).copy(), ocode.reshape(K, N // 2, 2)
        big = np.abs(pair_t) > edge
        first = big[..., 0] & (~big[..., 1] | (np.abs(pair_t[..., 0]) >= np.abs(pair_t[..., 1])))
        second = big[..., 1] & ~first
        pair_c[..., 0] = np.where(first, pair_o[..., 0], np.where(second, 15, pair_c[..., 0]))
        pair_c[..., 1] = np.where(second, pair_o[..., 1], np.where(first, 15, pair_c[..., 1]))
        code = pair_c.reshape(K, N)
    code = code.reshape(K, N // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).astype(np.uint8)


def gauss_case(dtype_name, K, book_name, per_row, seed=0):
    """Gaussian weights [K, 40] encoded through the yardstick (codes -> image; the pair rule's book with 0.5 % planted
    outliers), one scale per k or one per tensor, Gaussian x (8 rows) and bias in the type.  Deterministic in its arguments.
    columns(case, 8) is the same layer's first eight columns: an output's bits depend on its own column alone."""
    bk = book(book_name)
    name, g, gmax, nn, ovp = bk
    N = max(RULE_N)
    rng = np.random.default_rng([DTYPES.index(dtype_name), K, RULE_BOOKS.index(book_name), int(per_row), seed, 4])
    w = rng.standard_normal((K, N)).astype(np.float32) * np.float32(0.05)
    if ovp:
        big = rng.random((K, N)) < 0.005
        big[0, :2], big[K - 1, -2:] = (False, True), (True, False)      # the outlier as the high and as the low nibble of its pair
        w = np.where(big, np.sign(w) * np.float32(0.05) * rng.uniform(8, 20, (K, N)).astype(np.float32), w)
        alpha = 3 * (w.std(1) if per_row else w.std(keepdims=True).reshape(1))
    else:
        alpha = np.float32(0.9) * (np.abs(w).max(1) if per_row else np.abs(w).max(keepdims=True).reshape(1))
    alpha = np.ascontiguousarray(alpha, np.float32)
    codes = encode_nearest(w, alpha, per_row, bk)
    W = image_bits(codes, alpha, K, N, per_row, bk, dtype_name)
    x = round_bits(rng.standard_normal((RULE_ROWS, K)).astype(np.float32), dtype_name)
    bias = round_bits(rng.standard_normal(N).astype(np.float32), dtype_name)
    return dict(dtype_name=dtype_name, K=K, N=N, book=bk, per_row=per_row, codes=codes, alpha=alpha, W=W, x=x, bias=bias)


def rule_cases(dtype_name, ks=RULE_K):
    """every case of a type: K x book x scale form, at N = 40"""
    return [gauss_case(dtype_name, K, b, per_row) for K in ks for b in RULE_BOOKS for per_row in (True, False)]


def case_id(c):
    return "%s K=%d %s %s" % (c["dtype_name"], c["K"], c["book"][0], "scale per k" if c["per_row"] else "one scale")


def columns(c, N):
    """the layer of the first N columns of a case (N % 8 == 0): its own contiguous codes, image and bias"""
    assert N % 8 == 0 and N <= c["N"]
    d = dict(c)
    d.update(N=N, codes=np.ascontiguousarray(c["codes"][:, :N // 2]), W=np.ascontiguousarray(c["W"][:, :N]), bias=np.ascontiguousarray(c["bias"][:N]))
    return d


def cancelling_bias(sums, row, dtype_name):
    """bias = -(the rule's own result of x's row `row` without bias, in the type), for a 16-bit type.  y[row, :] is then the
    residual of the fp32 sum against its own rounding: a few significant bits that are the LOW bits of the sum, which the
    type's 8 or 11 bits otherwise round away.  One vector per row of x (a bias belongs to a column, the sum to a row)."""
    assert dtype_name != "float32"
    return round_bits(sums[row], dtype_name) ^ np.uint16(0x8000)


def near_tie_bias(sums, dtype_name):
    """A small bias that puts one output per column next to a rounding tie of a 16-bit type.  For every column: over the
    rows of x, the two rounding midpoints next to the fp32 sum v and the three biases nearest to (midpoint - v) in the type,
    the one whose fl32(v + bias) comes closest to the midpoint.  Nothing cancels -- |bias| is below one unit in the last
    place of the output -- yet a sum that differs by an fp32 ulp on the far side of the tie rounds to another output."""
    assert dtype_name != "float32"
    step = np.uint16(1)
    r = round_bits(sums, dtype_name)
    v = sums.astype(np.float64)
    best, best_d = None, None
    for nb in (r + step, r - step):                                     # (the neighbour in magnitude: sign bit untouched)
        mid = (value(r, dtype_name) + value(nb, dtype_name)) / 2
        b0 = round_bits((mid - v).astype(np.float32), dtype_name)
        for b in (b0, b0 + step, b0 - step):
            land = (sums + value32(b, dtype_name)).astype(np.float32).astype(np.float64)
            with np.errstate(all="ignore"):
                d = np.abs(land - mid) / np.spacing(np.abs(sums)).astype(np.float64)
            d = np.where(np.isfinite(d), d, np.inf)
            if best is None:
                best, best_d = b.copy(), d
            else:
                best, best_d = np.where(d < best_d, b, best), np.minimum(d, best_d)
    row = best_d.argmin(0)
    cols = np.arange(sums.shape[1])
    return np.ascontiguousarray(best[row, cols]), row, best_d[row, cols]


def bias_variants(c, sums):
    """[(name, bias bits or None, rows of x the variant is about or None for all)] for a case and its header-rule sums:
    no bias and the Gaussian bias for every type; for the 16-bit types the cancelling bias of every row of x and the near-tie
    bias."""
    out = [("none", None, None), ("gauss", c["bias"], None)]
    if c["dtype_name"] != "float32":
        out += [("cancel%d" % r, cancelling_bias(sums, r, c["dtype_name"]), (r,)) for r in range(sums.shape[0])]
        out.append(("near_tie", near_tie_bias(sums, c["dtype_name"])[0], None))
    return out
