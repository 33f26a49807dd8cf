"""The inputs of antq_linear4_t_mm's GPU tests (test_gpu_linear4_t_mm.py), built here so that test_linear_t_mm_cases_host.py holds
the very same arrays to their premises on the CPU.  Nothing here touches the HIP library or torch.  The decode rule, the
roundings, the books and the code generators are linear_t_cases' (the yardstick of antq_linear4_t).

The kernel (include/antq.h, csrc/antq_k_linear_t_mm.h): steps of 32 k dealt to eight wavefronts, tiles of 16 rows of x, a
workgroup per 64 output columns.  The grids below sit at its switch points -- and at those of a 32- or 128-column tile."""
import numpy as np

import linear_t_cases as lt

DTYPES = ("bfloat16", "float16")
MAX_M = 64
# 8, 24: a partial step, wavefronts without any step; 32: one step; 40: one plus a partial one; 256: one pass of the eight
# wavefronts; 264: a pass plus a partial step; 520, 1600: several passes, unequal step counts per wavefront
GRID_K = (8, 24, 32, 40, 256, 264, 520, 1600)
GRID_N = (8, 16, 32, 40, 64, 72, 128, 136)
GRID_M = (1, 9, 15, 16, 17, 32, 33, 48, 49, 64)
STAGED_K = lt.STAGED_K                    # the most scales staged in LDS (kLinTScales, shared with antq_linear4_t)
EXACT_BOOKS = ("pot_b4_s", "olive_int", "olive_flint")       # dyadic codebooks
ONE_HOT_K, ONE_HOT_N = 264, 72


def tiny_scale(dtype_name):
    """a scale at which the smallest nonzero weights are subnormal in the type"""
    return np.float32(1.5e-4 if dtype_name == "float16" else 3.0e-38)


def subnormal_limit(dtype_name):
    return {"float32": 2.0 ** -126, "bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype_name]


def all_byte_codes(K, N):
    """codes [K, N / 2] that hold every byte value"""
    c = np.concatenate([(np.arange(N // 2) + 37 * k) % 256 for k in range(K)]).astype(np.uint8)
    assert np.unique(c).size == 256
    return c


def one_hot_scales(dtype_name, K):
    """[(per_row, alpha, has tiny scales)]: one per k -- ordinary and tiny ones --, one per tensor, a tiny one per tensor"""
    tiny = tiny_scale(dtype_name)
    per_k = np.resize(np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37]), K).astype(np.float32)
    return [(True, per_k, True), (False, np.float32([0.37]), False), (False, np.float32([tiny]), True)]


def one_hot_x(K, k0, rows=MAX_M):
    """rows k0 .. k0 + rows of the identity [K, K], zero rows beyond K: float32"""
    x = np.zeros((rows, K), np.float32)
    n = min(rows, K - k0)
    x[np.arange(n), k0 + np.arange(n)] = 1.0
    return x


def exact_case(rng, K, book, dtype_name, per_row, N, rows=MAX_M, xmax=3):
    """Codes [K, N] of a dyadic codebook, power-of-two scales and small-integer x (`rows` rows, |x| <= xmax) for which every
    product and every partial sum, in any order, is an integer below 2^24 in units of one power of two -- asserted here in
    float64 -- with the exact result.  A prefix of the columns and a prefix of the rows are a smaller case with the same
    property.  Returns (codes, alpha, x, bias, y, density of x)."""
    name, g, gmax, nn, ovp = book
    codes = lt.random_codes(rng, K * N // 2, ovp)
    j = rng.integers(-2, 2, K if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = lt.value(lt.image_bits(codes, alpha, K, N, per_row, book, dtype_name), dtype_name)     # [K, N]
    assert np.isfinite(W).all() and (W != 0).any()
    bias = rng.integers(-8, 9, N).astype(np.float64)
    # every weight is a whole multiple of uw, every x and the bias a whole number: every product a whole multiple of uw
    uw = 2.0 ** min(int(lt.lowest_bit_exponent(W).min()), 0)
    density = 1.0
    while True:
        x = rng.integers(-xmax, xmax + 1, (rows, K)).astype(np.float64) * (rng.random((rows, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        mass = (np.abs(x) @ np.abs(W) + np.abs(bias)[None, :]) / uw     # (sums of whole numbers below 2^53: exact)
        if mass.max() < 2.0 ** 24:
            break
        density *= 0.5
    check_exact(x, W, bias, uw)
    return codes, alpha, x, bias, x @ W, density


def check_exact(x, W, bias, unit):
    """The premise of an order-free exact sum, in float64: x, W / unit and bias are whole numbers, so every product is a whole
    multiple of the unit; the sum of the magnitudes of a column's products and its bias is below 2^24 units, so every partial
    sum in any order is a whole number of units below 2^24 -- exact in fp32, and in the 48-bit products of the matrix cores."""
    assert np.array_equal(x, np.round(x)) and np.array_equal(bias, np.round(bias))
    assert np.array_equal(W / unit, np.round(W / unit))
    mass = (np.abs(x) @ np.abs(W) + np.abs(bias)[None, :]) / unit
    assert mass.max() < 2.0 ** 24, "a partial sum may reach 2^24 units: %g" % mass.max()


def gauss_case(dtype_name, K, N, book_name, rows=MAX_M, seed=0):
    """Gaussian weights [K, N] encoded to the nearest code (the pair rule's book with 0.5 % planted outliers, one of them as
    the high and one as the low nibble of its pair), one scale per k, Gaussian x and bias in the type; the yardstick's image,
    the float64 product with it and the float64 mass S = |x| |W| + |bias|.  Deterministic in its arguments."""
    bk = lt.book(book_name)
    name, g, gmax, nn, ovp = bk
    rng = np.random.default_rng([DTYPES.index(dtype_name), K, N, sum(map(ord, book_name)), seed, 7])
    w = rng.standard_normal((K, N)).astype(np.float32) * np.float32(0.05)
    if ovp:
        big = rng.random((K, N)) < 0.005
        big[0, :2], big[K - 1, -2:] = (False, True), (True, False)
        w = np.where(big, np.sign(w) * np.float32(0.05) * rng.uniform(8, 20, (K, N)).astype(np.float32), w)
        alpha = 3 * w.std(1)
    else:
        alpha = np.float32(0.9) * np.abs(w).max(1)
    alpha = np.ascontiguousarray(alpha, np.float32)
    codes = lt.encode_nearest(w, alpha, True, bk)
    W = lt.image_bits(codes, alpha, K, N, True, bk, dtype_name)
    x = lt.round_bits(rng.standard_normal((rows, K)).astype(np.float32), dtype_name)
    bias = lt.round_bits(rng.standard_normal(N).astype(np.float32), dtype_name)
    x64, W64, b64 = lt.value(x, dtype_name), lt.value(W, dtype_name), lt.value(bias, dtype_name)
    return dict(dtype_name=dtype_name, K=K, N=N, book=bk, per_row=True, codes=codes, alpha=alpha, W=W, x=x, bias=bias,
                y64=x64 @ W64 + b64[None, :], S=np.abs(x64) @ np.abs(W64) + np.abs(b64)[None, :])


def has_pair_identifier(codes):
    c = np.asarray(codes, np.uint8).reshape(-1)
    return bool((((c & 15) == 15) | ((c >> 4) == 15)).any())


def shifted(c, by=8):
    """the layer of columns by .. N of a case: the same columns `by` places further left in their tiles"""
    assert by % 8 == 0 and by < c["N"]
    d = dict(c)
    d.update(N=c["N"] - by, codes=np.ascontiguousarray(c["codes"][:, by // 2:]), W=np.ascontiguousarray(c["W"][:, by:]),
             bias=np.ascontiguousarray(c["bias"][by:]))
    return d
