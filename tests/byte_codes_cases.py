"""Books, expected codes, the decoder's rule in numpy and the input builders of the byte-code tests (test_gpu_byte_codes.py),
and what test_byte_codes_host.py holds those inputs to with the CPU oracle alone.  Nothing here touches the HIP library.
The builders for thresholds, pairs, magnitudes and random data are encode4_cases' (generic in the codebook)."""
import functools

import numpy as np

import encode4_cases as ec
import fakequant_cases as fc

IDENT = 255                    # the pair rule's identifier: this element is the victim, its partner an outlier
BOOK_NAMES = ("int_b8_s", "flint_b6_s", "float_b5_s", "olive_int_b8", "olive_u4", "ladder_plain", "ladder_pairs")
OLIVE_NAMES = ("olive_int_b8", "olive_u4", "ladder_pairs")
DTYPES = ("float32", "bfloat16", "float16")
ROW_LENS = (4, 12, 20, 60, 64, 252, 256, 260, 1024, 4100)
ROW_COUNTS = (1, 3, 257)


def _ladder(rng, n, hi, lo_floor):
    """n magnitudes from hi downwards, neighbours within a factor of two (the codec's condition for decode == fake-quant)"""
    r = rng.uniform(1.02, 1.0 + 6.0 / n, n)
    mags = hi / np.cumprod(r)
    assert mags.min() > lo_floor
    return mags.astype(np.float32)


def _ladder_book(ovp):
    """An arbitrary book of 100 .. 256 values in SCAN order that is not sorted: both signs of a ladder, a zero and a -0.0,
    shuffled, one duplicate.  With the pair rule: such a list within 32 (with both zeros) and one beyond it (the first outlier
    within twice the last normal value)."""
    rng = np.random.default_rng(8100 + int(ovp))
    if not ovp:
        k = int(rng.integers(50, 127))
        mags = _ladder(rng, k, 24.0, 1e-3)
        g = np.concatenate([mags, -mags, [0.0, -0.0, mags[3]]]).astype(np.float32)
        g = g[rng.permutation(g.size)]
        assert 100 <= g.size <= 256
        return g, float(g.max()), 0
    kn, ko = int(rng.integers(50, 127)), int(rng.integers(50, 127))
    mn, mo = _ladder(rng, kn, 32.0, 1e-3), _ladder(rng, ko, 500.0, 0.0)
    mo = mo * np.float32(33.0 / mo.min())
    gn = np.concatenate([mn, -mn, [0.0, -0.0]]).astype(np.float32)
    go = np.concatenate([mo, -mo]).astype(np.float32)
    gn, go = gn[rng.permutation(gn.size)], go[rng.permutation(go.size)]
    assert 100 <= gn.size <= 255 and 100 <= go.size <= 255 and np.abs(gn).max() <= 32 and np.abs(go).min() > 32
    return np.concatenate([gn, go]).astype(np.float32), float(gn.max()), int(gn.size)


@functools.lru_cache(maxsize=None)
def book(name):
    """(name, grid as the kernel takes it, gmax, n_normal, pair rule)"""
    if name == "olive_u4":         # OliVe's unsigned 4-bit book: 16 normal values (no nibble left for the identifier) + 15 outliers
        O = ec.golden("olive_grids.npz")
        gn, go = O["flint_b4_u"], O["outlier_b4_u"]
        return (name, np.ascontiguousarray(np.concatenate([gn, go]), np.float32), float(gn.max()), int(gn.size), True)
    if name.startswith("ladder_"):
        g, gmax, nn = _ladder_book(name == "ladder_pairs")
        return (name, g, gmax, nn, nn > 0)
    return fc.book(name)


def book_fits(g, n_normal, ovp):
    m = g.size
    return (1 <= n_normal <= 255 and 0 <= m - n_normal <= 255) if ovp else 1 <= m <= 256


def codes_want(oracle, ridx, n_normal, ovp, zc):
    """encode4_cases.codes_want with the byte identifier"""
    want = ridx.astype(np.int64).copy()
    if ovp:
        want[ridx >= n_normal] -= n_normal
    want[ridx == oracle.IDX_VICTIM] = IDENT
    want[ridx == oracle.IDX_NONE] = zc
    return want


def oracle_codes(oracle, x, alpha, bk):
    _, g, gmax, nn, ovp = bk
    with np.errstate(all="ignore"):
        _, ridx = oracle.forward(np.ascontiguousarray(x, np.float32), alpha, g, gmax, ovp)
    return codes_want(oracle, ridx, nn, ovp, ec.zero_code(g, nn, ovp))


def to_bits(oracle, v, dtype_name):
    """float32 values -> the bits of the output type, rounded to nearest even"""
    v = np.ascontiguousarray(v, np.float32)
    if dtype_name == "bfloat16":
        return oracle.f32_to_bf16(v)
    if dtype_name == "float16":
        with np.errstate(all="ignore"):
            return v.astype(np.float16).view(np.uint16)
    return v.view(np.uint32)


def decode_ref(oracle, codes, alpha, bk, rows, row_len, dtype_name):
    """The decoder's rule: fl((g[c] + 0.0f) * fl(alpha / gmax)) rounded to the type; pair rule on the flat pairs: a byte of
    255 is a victim (+0) and sends its partner to the outlier list; a code beyond its list decodes to +0.  -> bits [rows, row_len]"""
    _, g, gmax, nn, ovp = bk
    c = np.asarray(codes).reshape(-1).astype(np.int64)
    tab = np.zeros(512, np.float32)
    if ovp:
        tab[:nn] = g[:nn] + np.float32(0)
        tab[256:256 + g.size - nn] = g[nn:] + np.float32(0)
        tab[255] = tab[511] = 0
        partner = c.reshape(-1, 2)[:, ::-1].reshape(-1)
        v = tab[c + np.where(partner == IDENT, 256, 0)]
    else:
        tab[:g.size] = g + np.float32(0)
        v = tab[c]
    a = np.broadcast_to(np.asarray(alpha, np.float32).reshape(-1, 1), (rows, 1))
    with np.errstate(all="ignore"):
        s = (a / np.float32(gmax)).astype(np.float32)
        out = (v.reshape(rows, row_len) * s).astype(np.float32)
    return to_bits(oracle, out, dtype_name).reshape(rows, row_len)


def decoded_from_indices(oracle, ridx, alpha, bk, dtype_name):
    """fl((g[idx] + 0) * s) from the oracle's own indices (a victim: +0), as bits: what decode8(encode8(x)) has to give"""
    _, g, gmax, nn, ovp = bk
    idx = ridx.astype(np.int64)
    v = (g + np.float32(0))[np.clip(idx, 0, g.size - 1)]
    v = np.where(idx == oracle.IDX_VICTIM, np.float32(0), v)
    v = np.where(idx == oracle.IDX_NONE, np.float32(0), v).astype(np.float32)
    a = np.asarray(alpha, np.float32).reshape(-1, 1) if np.ndim(alpha) else np.float32(alpha)
    s = (a / np.float32(gmax)).astype(np.float32)
    return to_bits(oracle, (v * s).astype(np.float32), dtype_name)


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (built here so that the host test sees the same arrays)
# ---------------------------------------------------------------------------------------------------------------------------
THRESHOLD_ROW_LENS = (508, 1032)        # 4 mod 8 (quad units) and 0 mod 8 (octet units)
PAIR_ROW_LEN = 504


@functools.lru_cache(maxsize=None)
def threshold_input(name, row_len):
    _, g, gmax, nn, ovp = book(name)
    return ec.threshold_case(np.random.default_rng(99), g, gmax, row_len, n_scales=min(16, fc.n_scales_of(g)))


@functools.lru_cache(maxsize=None)
def pair_input(name):
    _, g, gmax, nn, ovp = book(name)
    return ec.pair_case(np.random.default_rng(17), g, gmax, nn, PAIR_ROW_LEN, n_scales=8)


def round_trip_input(name, dtype_name, rows, row_len, oracle):
    """Gaussian data clipped to 1.9 x the outermost grid value on finite positive scales (pair rule: 5 % of the pairs hold an
    outlier), rounded to the type.  -> (bits for the kernel, the same values as float32, alpha)"""
    _, g, gmax, nn, ovp = book(name)
    seed = 1000 * BOOK_NAMES.index(name) + 100 * DTYPES.index(dtype_name) + 10 * ROW_COUNTS.index(rows) + ROW_LENS.index(row_len)
    case = ec.random_case(np.random.default_rng(seed), rows, row_len, g, gmax, ovp)
    xk, xf = ec.as_dtype(oracle, case["x"], dtype_name)
    return xk, xf, case["alpha"]


def round_trip_ok(xf, alpha, bk):
    """the restriction the round trip is stated for: finite values within twice the outermost grid value, finite positive scales"""
    _, g, gmax, nn, ovp = bk
    s = (np.asarray(alpha, np.float32) / np.float32(gmax)).astype(np.float32)
    return bool(np.isfinite(xf).all() and np.isfinite(s).all() and (s > 0).all()
                and (np.abs(xf / s.reshape(-1, 1)) <= 2 * np.abs(g).max()).all())
