"""tests/linear_t_cases.py held to its premises on the CPU: the emulated fused multiply-add is correctly rounded (against exact
rationals, with planted ties where rounding twice goes wrong), the tile rule in numpy agrees with the float64 product inside
the fp32 bound and with the exact result on dyadic data, and the cases of the GPU test tell the rule of include/antq.h from
other fixed orders of the same sum.

What carries the bit-for-bit GPU test is float32: there every order named in linear_t_cases.ORDERS changes a quarter of
the outputs or more at K >= 128 (measured: 27 .. 99 %).  A 16-bit output keeps 8 or 11 bits of a 24-bit sum, so with no bias or
a Gaussian one at most 2 % of the float16 outputs and -- in all but one of the cases here -- no bfloat16 output at all depends
on the order; the cancelling bias (float16: 36 .. 98 % at K >= 520; bfloat16: 1.9 .. 28 % at K >= 1600) and, for a bias that
cancels nothing, the near-tie bias (bfloat16: 0.3 .. 7 % at K >= 1600) are there to make those types see the low bits at all."""
from fractions import Fraction

import numpy as np
import pytest

import linear_t_cases as lt


# ---------------------------------------------------------------------------------------------------------------------------
# fma32
# ---------------------------------------------------------------------------------------------------------------------------
def _round_fraction_to_f32(f):
    """an exact rational -> the nearest float32, ties to even, subnormals included (no overflow in the data here)"""
    if f == 0:
        return np.float32(0.0)
    a = abs(f)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)
    n = a / q
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    v = float(lo * q)                    # (24 bits times a power of two: exact in float64)
    assert v < 2.0 ** 128
    return np.float32(-v if f < 0 else v)


def _exact_fma(x, w, acc):
    out = np.empty(x.size, np.float32)
    for i in range(x.size):
        out[i] = _round_fraction_to_f32(Fraction(float(x[i])) * Fraction(float(w[i])) + Fraction(float(acc[i])))
    return out


def _random_f32(rng, n, lo_exp, hi_exp):
    return (rng.uniform(1, 2, n) * np.exp2(rng.integers(lo_exp, hi_exp + 1, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _planted_ties(rng, n):
    """Triples whose exact x * w + acc lies 2^-2u of an ulp off an fp32 midpoint (u = 15 .. 23): x * w = (1 + 2^-u)(1 - 2^-u) / 2
    = 1/2 - 2^-(2u+1) against an addend of 2^23 + j, all scaled by a power of two, either sign.  The float64 sum rounds ONTO
    the midpoint; rounding that to float32 goes to the even neighbour, which for odd j is the wrong one."""
    u = rng.integers(15, 24, n)
    s = rng.integers(-40, 41, n)
    j = rng.integers(0, 2 ** 23, n)
    sign_p, sign_a = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    x = (sign_p * np.exp2(s - 1.0) * (1 + np.exp2(-u.astype(np.float64)))).astype(np.float32)
    w = (1 - np.exp2(-u.astype(np.float64))).astype(np.float32)
    acc = (sign_a * (2.0 ** 23 + j) * np.exp2(s.astype(np.float64))).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), sign_p * np.exp2(s - 1.0) * (1 + np.exp2(-u.astype(np.float64))))
    return x, w, acc


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(7)
    n = 1200
    sets = {}
    # random triples of like magnitude: the sum cancels, or carries
    x, w = _random_f32(rng, n, -4, 4), _random_f32(rng, n, -4, 4)
    sets["random"] = (x, w, _random_f32(rng, n, -8, 8))
    # wide exponent gaps either way, down to subnormal results and up to where the addend swallows the product
    x, w = _random_f32(rng, n, -60, 40), _random_f32(rng, n, -60, 20)
    sets["gaps"] = (x, w, _random_f32(rng, n, -140, 60))
    # an fp32 partial sum and a product of 16-bit operands, as in the rule's chains
    x = lt.value32(lt.round_bits(_random_f32(rng, n, -3, 3), "bfloat16"), "bfloat16")
    w = lt.value32(lt.round_bits(_random_f32(rng, n, -6, 0), "float16"), "float16")
    sets["chain"] = (x, w, _random_f32(rng, n, -2, 6))
    # zeros and signs
    z = np.float32([0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 0.0, -0.0])
    sets["zeros"] = (z, np.float32([1.0, 1.0, -2.0, 0.0, 0.0, -0.0, 3.0, 3.0]), np.float32([0.0, 0.0, 0.0, 0.0, -0.0, 0.0, 2.0, -2.0]))
    sets["ties"] = _planted_ties(rng, 600)
    for name, (x, w, acc) in sets.items():
        got, want = lt.fma32(x, w, acc), _exact_fma(x, w, acc)
        assert np.array_equal(got.view(np.uint32) << 1, want.view(np.uint32) << 1) and np.isfinite(want).all(), name
        if name != "zeros":
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    # (the sign of a zero: +0 from the rule's +0 accumulator, as IEEE's round-to-nearest gives it)
    x, w, acc = sets["zeros"]
    assert np.array_equal(np.signbit(lt.fma32(x, w, acc)), [False, False, False, False, False, False, False, True])
    # the planted ties are what they claim: rounding twice fails on them, and on nothing else here
    x, w, acc = sets["ties"]
    wrong = lt.fma32_twice_rounded(x, w, acc).view(np.uint32) != _exact_fma(x, w, acc).view(np.uint32)
    assert wrong.sum() >= 100, int(wrong.sum())
    x, w, acc = sets["random"]
    assert np.array_equal(lt.fma32_twice_rounded(x, w, acc), _exact_fma(x, w, acc))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases are what they say
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", lt.DTYPES)
def test_cases_are_well_formed(dtype_name):
    assert lt.STAGED_K in lt.RULE_K and lt.STAGED_K + 8 in lt.RULE_K and max(lt.RULE_K) == lt.STAGED_K + 8
    assert {k % lt.PHASES == 0 for k in lt.RULE_K} == {True, False} and min(lt.RULE_K) < lt.PHASES < max(lt.RULE_K)
    seen = set()
    for c in lt.rule_cases(dtype_name, ks=(8, 136, 1600)):
        K, N, (name, g, gmax, nn, ovp) = c["K"], c["N"], c["book"]
        seen.add((name, c["per_row"]))
        assert c["codes"].shape == (K, N // 2) and c["codes"].dtype == np.uint8 and c["alpha"].dtype == np.float32
        assert c["alpha"].shape == ((K,) if c["per_row"] else (1,)) and (c["alpha"] > 0).all()
        assert c["x"].shape == (lt.RULE_ROWS, K) and c["bias"].shape == (N,) and c["W"].shape == (K, N)
        lo, hi = c["codes"] & 15, c["codes"] >> 4
        W = lt.value(c["W"], dtype_name)
        assert np.isfinite(W).all() and (W != 0).mean() > 0.5
        if ovp:     # planted outliers: the identifier on either side, its partner an index of the outlier list
            assert ((lo == 15) & (hi < g.size - nn)).any() and ((hi == 15) & (lo < g.size - nn)).any()
            assert not ((lo == 15) & (hi == 15)).any()
            assert (np.abs(W) > 1.2 * c["alpha"].reshape(-1, 1)).any()      # (normal values end at alpha, outliers start at 1.5 alpha)
        else:
            assert np.unique(np.concatenate([lo, hi])).size >= (12 if K > 8 else 6)
        # a prefix of the columns is the narrower layer: its own codes decode to the same columns
        d = lt.columns(c, 8)
        assert d["codes"].flags["C_CONTIGUOUS"] and d["codes"].shape == (K, 4)
        assert np.array_equal(lt.image_bits(d["codes"], d["alpha"], K, 8, c["per_row"], c["book"], dtype_name), c["W"][:, :8])
        again = lt.gauss_case(dtype_name, K, name, c["per_row"])
        assert all(np.array_equal(again[k], c[k]) for k in ("codes", "alpha", "x", "bias", "W"))
    assert seen == {(b, p) for b in lt.RULE_BOOKS for p in (True, False)}


# ---------------------------------------------------------------------------------------------------------------------------
# the rule against the yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def _within_bound(y, y64, S, K, dtype_name):
    """the bound of test_gpu_linear4_t.py: |y - y64| <= K 2^-23 S + 2^-p |y64|"""
    err = np.abs(y - y64)
    bound = K * 2.0 ** -23 * S + 2.0 ** -lt.PREC[dtype_name] * np.abs(y64)
    return bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype_name", lt.DTYPES)
def test_rule_agrees_with_the_float64_product(dtype_name):
    for c in lt.rule_cases(dtype_name, ks=(8, 72, 128, 136, 520, 1600)):
        x64, W64, b64 = (lt.value(c[k], dtype_name) for k in ("x", "W", "bias"))
        sums = lt.rule_sums(c["x"], c["W"], dtype_name)
        for bias, add in ((c["bias"], b64[None, :]), (None, 0.0)):
            y = lt.value(lt.finish(sums, bias, dtype_name), dtype_name)
            y64 = x64 @ W64 + add
            S = np.abs(x64) @ np.abs(W64) + np.abs(add)
            ok, worst = _within_bound(y, y64, S, c["K"], dtype_name)
            assert ok, (lt.case_id(c), bias is not None, worst)
        # a prefix of rows and of columns has the same bits: the rule knows one row and one column at a time
        d = lt.columns(c, 8)
        assert np.array_equal(lt.tile_rule(d["x"][:3], d["W"], d["bias"], dtype_name), lt.finish(sums, c["bias"], dtype_name)[:3, :8])


@pytest.mark.parametrize("dtype_name", lt.DTYPES)
def test_every_order_is_exact_on_dyadic_data(dtype_name):
    """the order-free case of the GPU test: every product and partial sum exact, so the rule and every alternative must give
    the exact result rounded once"""
    rng = np.random.default_rng(5)
    for bname, K, per_row in (("pot_b4_s", 136, True), ("olive_flint", 520, True), ("olive_int", 1600, True), ("pot_b4_s", 72, False)):
        bk = lt.book(bname)
        N = 40
        codes, alpha, x, bias, y, density = lt.exact_case(rng, K, bk, dtype_name, per_row, N)
        W = lt.image_bits(codes, alpha, K, N, per_row, bk, dtype_name)
        xb, bb = lt.round_bits(x.astype(np.float32), dtype_name), lt.round_bits(bias.astype(np.float32), dtype_name)
        assert np.array_equal(lt.value(xb, dtype_name), x) and np.array_equal(lt.value(bb, dtype_name), bias)
        for order in lt.ORDERS:
            assert np.array_equal(lt.tile_rule(xb, W, bb, dtype_name, order), lt.round_bits((y + bias[None, :]).astype(np.float32), dtype_name)), (bname, K, order)
            assert np.array_equal(lt.tile_rule(xb, W, None, dtype_name, order), lt.round_bits(y.astype(np.float32), dtype_name)), (bname, K, order)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases tell the orders apart
# ---------------------------------------------------------------------------------------------------------------------------
def shares(c):
    """{(bias variant, alternative order): (outputs whose bits the order changes, outputs)} of a case.  "cancel" gathers, for
    every row of x, that row of the output under its own cancelling bias."""
    dt = c["dtype_name"]
    xv, Wv = lt.value32(c["x"], dt), lt.value32(c["W"], dt)
    parts = {lt.PHASES: lt.partial_sums(xv, Wv, dt), 1: lt.partial_sums(xv, Wv, dt, 1)}
    sums = {o: lt.rule_sums(None, None, dt, o, parts[lt.ORDERS[o][0]]) for o in lt.ORDERS}
    out = {}
    for name, bias, rows in lt.bias_variants(c, sums["header"]):
        want = lt.finish(sums["header"], bias, dt)
        for o in lt.ALTERNATIVES:
            diff = want != lt.finish(sums[o], bias, dt)
            if rows is not None:
                diff = diff[list(rows)]
            key = ("cancel" if rows is not None else name, o)
            n, tot = out.get(key, (0, 0))
            out[key] = (n + int(diff.sum()), tot + diff.size)
    return out


@pytest.mark.parametrize("dtype_name", lt.DTYPES)
def test_cases_tell_the_orders_apart(dtype_name):
    """Conditions on the cases, not tolerances.  For every case (K x book x scale form, the 8 x 40 outputs; the launches of 8
    columns are a prefix of them) and every alternative order, the share of outputs whose bits differ from the rule's:
      float32, K >= 128, no bias and the Gaussian bias each     at least a quarter
      float16, K >= 520, the cancelling bias                    at least a tenth
      bfloat16, K >= 1600, the cancelling bias                  at least one output
      bfloat16, K >= 1600, without a cancelling bias            at least one output -- met by the near-tie bias: with no bias
                                                                or the Gaussian one no bfloat16 output changes in 11 of these
                                                                12 cases, whatever the seed of the data (the odds are about
                                                                three fp32 ulps in 2^16 per output)
    float32 carries the test (module docstring)."""
    lines = []
    for c in lt.rule_cases(dtype_name, ks=[k for k in lt.RULE_K if k >= 128]):
        K, sh = c["K"], shares(c)
        lines.append("%s: " % lt.case_id(c) + ", ".join("%s/%s %d/%d" % (v, o, n, tot) for (v, o), (n, tot) in sorted(sh.items())))
        for o in lt.ALTERNATIVES:
            share = lambda v: sh[(v, o)][0] / sh[(v, o)][1]
            if dtype_name == "float32":
                assert share("none") >= 0.25 and share("gauss") >= 0.25, (lt.case_id(c), o, sh[("none", o)], sh[("gauss", o)])
            if dtype_name == "float16" and K >= 520:
                assert share("cancel") >= 0.1, (lt.case_id(c), o, sh[("cancel", o)])
            if dtype_name == "bfloat16" and K >= 1600:
                assert sh[("cancel", o)][0] >= 1, (lt.case_id(c), o)
                assert sh[("none", o)][0] + sh[("gauss", o)][0] + sh[("near_tie", o)][0] >= 1, (lt.case_id(c), o)
                assert sh[("near_tie", o)][0] >= 1, (lt.case_id(c), o)
    print("\n".join(lines))


def test_near_tie_bias_cancels_nothing():
    """the near-tie bias stays below one unit in the last place of the output, and lands the chosen row within a few fp32
    ulps of a rounding midpoint"""
    for dtype_name in ("bfloat16", "float16"):
        c = lt.gauss_case(dtype_name, 1600, "flint_b4_s", True)
        sums = lt.rule_sums(c["x"], c["W"], dtype_name)
        bias, row, dist = lt.near_tie_bias(sums, dtype_name)
        cols = np.arange(c["N"])
        v = np.abs(sums[row, cols].astype(np.float64))
        assert (np.abs(lt.value(bias, dtype_name)) <= 2.0 ** -lt.PREC[dtype_name] * v).all()
        assert np.median(dist) <= 4 and np.isfinite(dist).all()
        y = lt.value(lt.finish(sums, bias, dtype_name), dtype_name)
        assert (np.abs(y[row, cols]) >= v * (1 - 2.0 ** -lt.PREC[dtype_name])).all()
