"""The inputs of the matrix-core byte-code linear's GPU tests (test_gpu_linear8_mm.py), built here so that
test_linear8_mm_cases_host.py holds the very same arrays to their premises with numpy and the CPU oracle alone.  Nothing here
touches the HIP library.  Books, codes and the decoder's rule restated in numpy are linear8_cases' and byte_codes_cases'.

The kernel's own constants (csrc/antq_k_linear_mm.h with Lin8Codec): K is cut into chunks of 64 elements (codes read 16 bytes per lane:
K % 16 == 0 and 16-byte-aligned codes) or of 32 (8 bytes per lane), dealt to eight wavefronts in turn, so w = 1 .. 8 wavefronts
have work up to K = 64 w and 32 w; a wavefront keeps a ring of D = 4 / 3 / 2 chunks (1 / 2 / 4 tiles of 16 rows of x) and
refills it for the first time when K holds more than 8 D chunks."""
import numpy as np

import byte_codes_cases as bc
import linear8_cases as lc
from linear8_cases import (EXACT_CASES, gauss_weights, image_ref, one_hot_codes, one_hot_scales, random_codes, unit_of,  # noqa: F401
                           within_bound)

DTYPES = ("bfloat16", "float16")
TILES = (1, 2, 4)                        # tiles of 16 output rows per workgroup (antq_debug_set key 22)
CHUNK = {8: 32, 16: 64}                  # bytes of codes per lane -> elements per chunk
RING_DEPTHS = (4, 3, 2)
WAVES = 8
ROWS = 64                                # rows of x a case holds

ONE_HOT_K = (520, 1040)                  # the 8-byte path, the 16-byte path
ONE_HOT_N = 37                           # two workgroups and a tail at every tile shape but the largest
ONE_HOT_BOOKS = bc.BOOK_NAMES

EXACT_K_SHARED = (8, 16, 24, 32, 40, 4096)
# the last K at which w wavefronts have work, and either side (multiples of 16 reach the 8-byte path with codes 8 bytes off a
# 16-byte boundary: EXACT_OFFSETS)
EXACT_K_8 = tuple(sorted({CHUNK[8] * w + d for w in range(1, WAVES + 1) for d in (-8, 0, 8)}))
EXACT_K_16 = tuple(sorted({CHUNK[16] * w + d for w in range(1, WAVES + 1) for d in (-16, 0, 16)}))
# the K at which a wavefront's ring holds exactly its 8 D chunks, one chunk fewer, and the first refill
EXACT_K_RING = {b: tuple(sorted({CHUNK[b] * (WAVES * D + d) for D in RING_DEPTHS for d in (-1, 0, 1)})) for b in (8, 16)}
EXACT_K = tuple(sorted(set(EXACT_K_SHARED) | set(EXACT_K_8) | set(EXACT_K_16) | set(EXACT_K_RING[8]) | set(EXACT_K_RING[16])))
EXACT_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
EXACT_M = (1, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)
MM_EXACT_CASES = tuple(c for c in EXACT_CASES if c[1] in DTYPES)

GENERAL_BOOKS = lc.GENERAL_BOOKS
GENERAL_K = (768, 4096)
GENERAL_N = 33
GENERAL_M = (9, 16, 40, 64)


def exact_offsets(K):
    """bytes past a 16-byte boundary the codes of an exact case start at: 0, and 8 where 0 would be the 16-byte path"""
    return (0, 8) if K % 16 == 0 else (0,)


def exact_case(oracle, name, K, dtype_name, per_row, N=max(EXACT_N)):
    """Codes [N, K], power-of-two scales and small-integer x (64 rows) for which every product and every partial sum, in any
    order, is a whole number below 2^24 in units of one power of two -- asserted here in float64, in matmul form -- with the
    exact result.  Deterministic in its arguments."""
    _, g, gmax, nn, ovp = bc.book(name)
    rng = np.random.default_rng([lc.EXACT_BOOKS.index(name), K, DTYPES.index(dtype_name), int(per_row), N, 83])
    codes = random_codes(rng, N * K, ovp).reshape(N, K)
    j = rng.integers(-2, 2, N if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = lc.value(image_ref(oracle, codes, alpha, per_row, name, dtype_name), dtype_name)
    bias = rng.integers(-8, 9, N).astype(np.float64)
    unit = unit_of(W)                    # x and the bias hold whole numbers: every term is a whole multiple of W's unit
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (ROWS, K)).astype(np.float64) * (rng.random((ROWS, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        if exact_mass(x, W, bias, unit).max() < 2.0 ** 24:
            break
        density *= 0.5
        assert density >= 2.0 ** -12, "no exact case for this book: its values share no power-of-two unit"
    assert_exact_premise(x, W, bias)
    y = (x @ (W / unit).T) * unit                                       # exact: |partial sums| <= mass < 2^24 units
    return dict(codes=codes, alpha=alpha, x=x, bias=bias, y=y, W=W, density=density)


def exact_mass(x, W, bias, unit):
    """sum of the terms' magnitudes plus |bias| in units, [M, N]: whole numbers below 2^53, so float64 holds them exactly"""
    return np.abs(x) @ np.abs(W / unit).T + np.abs(bias)[None, :] / unit


def assert_exact_premise(x, W, bias):
    """the premise, in float64 and in matmul form: x and the bias whole numbers, every weight a whole multiple of the unit (so
    every term and every partial sum is), and the sum of magnitudes plus |bias| below 2^24 units"""
    unit = unit_of(W)
    assert unit <= 1.0 and np.array_equal(W / unit, np.round(W / unit)) and np.abs(W / unit).max() < 2.0 ** 24
    assert np.array_equal(x, np.round(x)) and np.array_equal(bias, np.round(bias))
    assert exact_mass(x, W, bias, unit).max() < 2.0 ** 24


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
    and the bias rotated through it.  Every N, every M, every offset, both bias forms run at every K."""
    ki = EXACT_K.index(K)
    runs = []
    for ni in range(len(EXACT_N)):
        for oi, off in enumerate(exact_offsets(K)):
            for mi in range(len(EXACT_M)):
                if (ni + mi + ki + oi) % 2 and mi != len(EXACT_M) - 1 and ni != len(EXACT_N) - 1:
                    continue
                forms = (True, False) if (ni + mi) % 3 == 0 else ((ni + mi) % 2 == 0,)
                runs.append((ni, mi, off, TILES[(ni + mi + ki + oi) % 3], forms))
    return runs


def scale_rows(a, N):
    """N per-row scales cycling through a"""
    return np.float32([a[n % len(a)] for n in range(N)])
