"""The inputs of the tiled byte-code linear's GPU tests (test_gpu_linear8_gemm.py), built here so that
test_linear8_gemm_cases_host.py holds the very same arrays to their premises with numpy and the CPU oracle alone.  Nothing here
touches the HIP library.  Books, codes, the decoder's rule restated in numpy and the exact-sum premise are byte_codes_cases',
linear8_cases' and linear8_mm_cases'.

The kernel's own constants (csrc/antq_k_linear_gemm.h with Lin8Codec): a workgroup owns BN = 64 output rows and BM = 128 or 256
rows of x (2 or 4 wavefronts, antq_debug_set key 23); K is staged in steps of BK = 128 elements; a lane reads its 32 bytes of
codes per output tile and step as two 16-byte loads (K % 16 == 0 and 16-byte-aligned codes; with K % 32 == 16 the second load of
the row's last lane group lies past the row's end) or as four 8-byte loads; the tables of the 64 output rows are built by the
workgroup's own wavefronts, rows w, w + WAVES, ..."""
import numpy as np

import byte_codes_cases as bc
import linear8_cases as lc
import linear8_mm_cases as mc
from linear8_cases import gauss_weights, image_ref, one_hot_codes, one_hot_scales, random_codes, unit_of, within_bound  # noqa: F401
from linear8_mm_cases import assert_exact_premise, exact_mass, exact_offsets, scale_rows  # noqa: F401

DTYPES = ("bfloat16", "float16")
BN, BK = 64, 128
BMS = (128, 256)                         # rows of x per workgroup ...
TILES = (2, 4)                           # ... at this many wavefronts (antq_debug_set key 23; 0: the launcher's rule)
SHAPES = (0,) + TILES
CALL = 200                               # rows per call of the one-hot tests: crosses row tiles and ends inside one

ONE_HOT_K = (520, 528, 512)              # four 8-byte loads; two 16-byte loads with K % 32 == 16; the same without a tail
ONE_HOT_N = 37                           # ends inside the one tile of output rows
ONE_HOT_BOOKS = bc.BOOK_NAMES

# (160: the 16-byte path with a tail that ends on a whole lane group, K % 32 == 0)
EXACT_K = (8, 16, 24, 40, 120, 128, 136, 144, 160, 248, 256, 264, 272, 504, 512, 520, 528, 2056, 4096)
EXACT_N = (1, 15, 16, 17, 63, 64, 65, 129)
EXACT_M = (1, 9, 64, 65, 127, 128, 129, 255, 256, 257, 259, 515)
ROWS = max(EXACT_M)
EXACT_CASES = mc.MM_EXACT_CASES          # (book, dtype): the dyadic books of the other byte-code linears
MIN_DENSITY = 1.0 / 64                   # of x non-zero in every exact case

# int_b8_s (dyadic in bfloat16 only, on a fine unit) cannot keep 1 / 64 of 515 x 4096 elements of x non-zero below 2^24 units
# (1 / 64 as the draw's density leaves 0.0137 non-zero): at that K olive_u4 stands in for it, as it does in float16
STAND_IN = {("int_b8_s", 4096): "olive_u4"}

GENERAL_BOOKS = lc.GENERAL_BOOKS
GENERAL_K = (768, 4096)
GENERAL_N = 33
GENERAL_M = (65, 130, 300)


def vec_path(K, offset=0):
    """the 16-byte code path: K a multiple of 16 elements and the codes on a 16-byte boundary"""
    return K % 16 == 0 and offset % 16 == 0


def has_tail(K):
    return K % BK != 0


def exact_book(name, K):
    """the book an exact case of the set `name` uses at this K"""
    return STAND_IN.get((name, K), name)


def exact_case(oracle, name, K, dtype_name, per_row, N=max(EXACT_N), rows=ROWS):
    """linear8_mm_cases.exact_case for `rows` rows of x: codes [N, K], power-of-two scales and small-integer x for which every
    product and every partial sum, in any order, is a whole number below 2^24 in units of one power of two -- asserted here in
    float64, in matmul form -- with the exact result.  The density of x halves until that holds.  Deterministic in its arguments."""
    _, g, gmax, nn, ovp = bc.book(name)
    rng = np.random.default_rng([lc.EXACT_BOOKS.index(name), K, DTYPES.index(dtype_name), int(per_row), N, rows, 85])
    codes = random_codes(rng, N * K, ovp).reshape(N, K)
    j = rng.integers(-2, 2, N if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = lc.value(image_ref(oracle, codes, alpha, per_row, name, dtype_name), dtype_name)
    bias = rng.integers(-8, 9, N).astype(np.float64)
    unit = unit_of(W)                    # x and the bias hold whole numbers: every term is a whole multiple of W's unit
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (rows, K)).astype(np.float64) * (rng.random((rows, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        if exact_mass(x, W, bias, unit).max() < 2.0 ** 24:
            break
        density *= 0.5
        assert density >= 2.0 ** -12, "no exact case for this book: its values share no power-of-two unit"
    assert_exact_premise(x, W, bias)
    y = (x @ (W / unit).T) * unit                                       # exact: |partial sums| <= mass < 2^24 units
    return dict(codes=codes, alpha=alpha, x=x, bias=bias, y=y, W=W, density=density)


def exact_cases_of(oracle, name, K, dtype_name):
    """(per_row, [(the N values a case serves, case)]): per-row scales -- the codes of a prefix of rows are that smaller layer's
    codes, one case serves every N; one scale per tensor -- every N gets codes of its own."""
    per_row = EXACT_K.index(K) % 2 == 0
    if per_row:
        return per_row, [(EXACT_N, exact_case(oracle, name, K, dtype_name, True))]
    return per_row, [((N,), exact_case(oracle, name, K, dtype_name, False, N)) for N in EXACT_N]


def exact_runs(K):
    """[(ni, mi, offset, tile shape, bias forms)] one K's launches: the cross product N x M thinned by staggering -- a pair
    (N, M) runs where ni + mi + ki is even, the largest M with every N and the largest N with every M always -- the tile shape
    (both forced ones and the rule) and the bias rotated through it.  Every N, every M, every offset, every shape and both bias
    forms run at every K."""
    ki = EXACT_K.index(K)
    runs = []
    for ni in range(len(EXACT_N)):
        for oi, off in enumerate(exact_offsets(K)):
            for mi in range(len(EXACT_M)):
                if (ni + mi + ki + oi) % 2 and mi != len(EXACT_M) - 1 and ni != len(EXACT_N) - 1:
                    continue
                forms = (True, False) if (ni + mi) % 3 == 0 else ((ni + mi) % 2 == 0,)
                runs.append((ni, mi, off, SHAPES[(ni + mi + ki + oi) % 3], forms))
    return runs


# ---------------------------------------------------------------------------------------------------------------------------
# three mistakes restated in numpy (test_linear8_gemm_cases_host.py asserts that each would show)
# ---------------------------------------------------------------------------------------------------------------------------
def swap_16_byte_loads(W):
    """the weights a lane multiplies its x with when its two 16-byte loads of a step change places: inside every whole run of
    32 elements the two halves are exchanged (a row's last 16 elements, K % 32 == 16, stay: their partner is past the end)"""
    K = W.shape[1]
    k = np.arange(K)
    src = np.where(k < K - K % 32, k ^ 16, k)
    return W[:, src]


def rows_built_with_stride(waves, stride=8, rows=BN):
    """[rows] bool: the table rows of a tile that a workgroup of `waves` wavefronts builds when it strides them by `stride`"""
    built = np.zeros(rows, bool)
    for w in range(waves):
        built[w::stride] = True
    return built
