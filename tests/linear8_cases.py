"""The inputs of the byte-code linear's GPU tests (test_gpu_linear8.py), built here so that test_linear8_cases_host.py holds
the very same arrays to their premises with numpy and the CPU oracle alone.  Nothing here touches the HIP library.  Books and
the decoder's rule restated in numpy are byte_codes_cases' (book / decode_ref)."""
import numpy as np

import byte_codes_cases as bc

DTYPES = bc.DTYPES
PREC = {"float32": 23, "float16": 10, "bfloat16": 7}
SUBNORMAL_BELOW = {"float32": 2.0 ** -126, "bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}

# antq_linear8 reads 8 bytes of codes per lane (512 elements per step of a wavefront) unless K % 16 == 0 and the codes are
# 16-byte aligned: then 16 bytes per lane (1024 elements per step).
ONE_HOT_K = (520, 1040)                  # 8-byte path, one and a bit steps; 16-byte path, one and a bit steps
ONE_HOT_N = 5
ONE_HOT_BOOKS = bc.BOOK_NAMES
# Both sides of one and of two steps of each path.  The issue's list, plus 1008 / 1040 (either side of ONE 16-byte step: 1016 and
# 1032 are no multiples of 16 and take the 8-byte path), 2032 / 2048 / 2064 (two 16-byte steps).  The 8-byte path at exactly 512
# and 1024 elements is reached with codes that start 8 bytes off a 16-byte boundary (the GPU test runs those too).
EXACT_K = (8, 16, 504, 512, 520, 1008, 1016, 1024, 1032, 1040, 2032, 2048, 2056, 2064, 4096)
EXACT_N = (1, 2, 3, 4, 5, 7, 8, 9, 17, 33)
# int_b8_s is NOT dyadic here -- its values are k * 10 / 127 -- so in fp32 no power-of-two unit makes its sums exact, and in
# f16 (11 significant bits) the unit is so small that a handful of terms per row would be all that stays below 2^24 units.
# Rounded to bf16 (8 significant bits) its image is dyadic on a unit that leaves hundreds of terms per row: it is an exact-sum
# book for bfloat16 only.  olive_u4, whose values are halves and whole numbers, stands in for it in the other two types.
EXACT_BOOKS = ("flint_b6_s", "olive_int_b8", "olive_u4", "int_b8_s")
EXACT_CASES = tuple((b, d) for b in EXACT_BOOKS for d in DTYPES if b != "int_b8_s" or d == "bfloat16")
GENERAL_BOOKS = ("int_b8_s", "flint_b6_s", "olive_int_b8", "olive_u4")
GENERAL_K = (768, 4096)
GENERAL_N = 33


def tiny_scale(dtype_name):
    return 1.5e-4 if dtype_name == "float16" else 3.0e-38


def value(bits, dtype_name):
    """the output type's bits -> float64"""
    bits = np.asarray(bits)
    if dtype_name == "float32":
        return bits.view(np.float32).astype(np.float64)
    if dtype_name == "float16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows
# ---------------------------------------------------------------------------------------------------------------------------
def planted_pairs(name):
    """Pairs (low byte, high byte) every row of a pair-rule one-hot set holds: 255 as the low and as the high byte, outlier
    indices at both ends of the outlier list, an outlier index beyond the list, normal codes beyond the normal list, two victims."""
    _, g, gmax, nn, ovp = bc.book(name)
    if not ovp:
        return []
    no = g.size - nn
    pairs = [(255, 0), (0, 255), (255, no - 1), (no - 1, 255), (255, 255), (255, 254), (254, 255), (nn - 1, 0), (0, nn - 1)]
    if no < 255:
        pairs += [(255, no), (no, 255), (254, 255)]
    if nn < 255:
        pairs += [(nn, 3), (3, nn), (254, 254), (nn, nn)]
    return pairs


def one_hot_codes(name, K, N=ONE_HOT_N):
    """[N, K] bytes: every row holds all 256 byte values (at positions that shift from row to row by an odd amount, so that 255
    is the low byte of its pair in some rows and the high byte in others), then the planted pairs, then a filler."""
    rows = []
    for n in range(N):
        head = np.roll(np.arange(256), 37 * n)
        plant = np.asarray(planted_pairs(name), np.int64).reshape(-1)
        fill = (np.arange(K - 256 - plant.size) * 7 + 11 * n) % 256
        rows.append(np.concatenate([head, plant, fill]))
    c = np.stack(rows).astype(np.uint8)
    assert c.shape == (N, K)
    return c


def one_hot_scales(dtype_name):
    """(per_row, alpha) sets: ordinary and so small that weights are subnormal in the type"""
    t = np.float32(tiny_scale(dtype_name))
    return ((True, np.float32([1.0, 0.06, t, 20 * t, 0.37])), (False, np.float32([0.37])), (False, np.float32([t])))


def image_ref(oracle, codes, alpha, per_row, name, dtype_name):
    """bits [N, K] of the image antq_decode8 has to write for codes [N, K]"""
    N, K = codes.shape
    r, k = (N, K) if per_row else (1, N * K)
    return bc.decode_ref(oracle, codes, alpha, bc.book(name), r, k, dtype_name).reshape(N, K)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
def random_codes(rng, n, ovp):
    c = rng.integers(0, 256, n, dtype=np.uint8)
    if ovp:
        c[rng.random(n) < 0.02] = bc.IDENT
    return c


def lowest_bit_exponent(t):
    """exponent of the lowest set bit of every nonzero float64 in t"""
    m, e = np.frexp(t[t != 0])
    mi = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)


def unit_of(terms):
    """the power of two every term is a whole multiple of (at most 1: the bias holds whole numbers; all terms zero: 1)"""
    return 2.0 ** min(int(lowest_bit_exponent(terms).min()), 0) if (terms != 0).any() else 1.0


def exact_case(oracle, name, K, dtype_name, per_row, N=max(EXACT_N)):
    """Codes [N, K], power-of-two scales and small-integer x (8 rows) for which every product and every partial sum, in any
    order, is a whole number below 2^24 in units of one power of two -- asserted here in float64 -- with the exact result.
    Deterministic in its arguments."""
    _, g, gmax, nn, ovp = bc.book(name)
    rng = np.random.default_rng([EXACT_BOOKS.index(name), K, DTYPES.index(dtype_name), int(per_row), N, 81])
    codes = random_codes(rng, N * K, ovp).reshape(N, K)
    j = rng.integers(-2, 2, N if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = value(image_ref(oracle, codes, alpha, per_row, name, dtype_name), dtype_name)
    bias = rng.integers(-8, 9, N).astype(np.float64)
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (8, K)).astype(np.float64) * (rng.random((8, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        terms = x[:, None, :] * W[None, :, :]                          # [8, N, K]
        unit = unit_of(terms)
        mass = (np.abs(terms).sum(-1) + np.abs(bias)[None, :]) / unit
        if mass.max() < 2.0 ** 24:
            break
        density *= 0.5
        assert density > 2.0 ** -12, "no exact case for this book: its values share no power-of-two unit"
    assert_exact_premise(x, W, bias)
    y = terms.sum(-1)                                                   # exact in float64: < 2^24 units
    return dict(codes=codes, alpha=alpha, x=x, bias=bias, y=y, W=W, density=density)


def assert_exact_premise(x, W, bias):
    """the premise, in float64: every term a whole multiple of the unit, and the sum of magnitudes below 2^24 units -- a
    fortiori below 2^24 in units of the smallest nonzero |term|"""
    terms = x[:, None, :] * W[None, :, :]
    nz = np.abs(terms[terms != 0])
    unit = unit_of(terms)
    mass = (np.abs(terms).sum(-1) + np.abs(bias)[None, :]) / unit
    assert np.array_equal(terms / unit, np.round(terms / unit)) and mass.max() < 2.0 ** 24
    assert np.array_equal(bias, np.round(bias))
    if nz.size:
        assert ((np.abs(terms).sum(-1) + np.abs(bias)[None, :]) / min(nz.min(), 1.0)).max() < 2.0 ** 24


def exact_cases_of(oracle, name, K, dtype_name):
    """[(the N values a case serves, case)]: per-row scales -- the codes of a prefix of rows are that smaller layer's codes, one
    case serves every N; one scale per tensor -- the table is shared by a wavefront's rows: every N gets codes of its own."""
    per_row = EXACT_K.index(K) % 2 == 0
    if per_row:
        return per_row, [(EXACT_N, exact_case(oracle, name, K, dtype_name, True))]
    return per_row, [((N,), exact_case(oracle, name, K, dtype_name, False, N)) for N in EXACT_N]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data
# ---------------------------------------------------------------------------------------------------------------------------
def gauss_weights(name, dtype_name, K, N=GENERAL_N, M=8, seed=17):
    """Gaussian weights (pair rule: 0.1 % planted outliers), per-row scales, Gaussian x and bias, as float32"""
    _, g, gmax, nn, ovp = bc.book(name)
    rng = np.random.default_rng([seed, GENERAL_BOOKS.index(name), DTYPES.index(dtype_name), K, N])
    w = rng.standard_normal((N, K)).astype(np.float32) * np.float32(0.05)
    if ovp:
        big = rng.random((N, K)) < 0.001
        w = np.where(big, np.sign(w) * np.float32(0.05) * rng.uniform(8, 20, (N, K)).astype(np.float32), w)
        alpha = (3 * w.std(1)).astype(np.float32)
    else:
        alpha = (np.abs(w).max(1) * np.float32(0.9)).astype(np.float32)
    if g.min() >= 0:
        w = np.abs(w)
    x = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    return dict(w=w, alpha=alpha, x=x, bias=b)


def within_bound(y, y64, S, K, dtype_name):
    """|y - y64| <= K 2^-23 S + 2^-p |y64|: the bound of an fp32 sum of K exact-or-fused products in any order, doubled, plus
    the rounding to the output type (p = 23 / 10 / 7) -- the packed 4-bit linear's bound."""
    err = np.abs(y - y64)
    bound = K * 2.0 ** -23 * S + 2.0 ** -PREC[dtype_name] * np.abs(y64)
    return bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())
