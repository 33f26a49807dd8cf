"""The packed 4-bit linear for [K, N] weights (GPT-2's Conv1D) on the GPU: antq_linear4_t (csrc/antq_k_linear_t.h) computes
y = x . W (+ bias) from the code bytes, W being the image antq_decode4 writes for K rows of N codes with one scale per row k.
The yardstick is that of tests/test_gpu_linear4.py -- include/antq.h's decode rule restated in numpy on the code bytes, and a
float64 product x64 @ W -- with the rows of the codes being k.  Exact tests compare bits; the general test holds the result
to the bound of an fp32 sum.

Shapes: the kernel's tile rule has two switch points only -- 128 phases of k (K = 8 ... 72 stay inside a partial pass, 128 is
exactly one pass, 136 one pass plus a partial one, 520 and 1600 are several passes -- at 1600 more than one group of steps in
flight -- plus a partial one) and 32 columns per workgroup (N = 8, 16 a partial tile, 32 exactly one, 40 ... 136 whole tiles plus
a partial one, 64 two whole tiles).  K = 128, 136 and N = 32, 40 are here for those switch points, beside the shapes the
kernel's issue named for a 64-phase, 64-column tile."""
import copy
import types

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16")
PREC = {"float32": 23, "float16": 10, "bfloat16": 7}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _books():
    """(name, grid as the kernel takes it, gmax, n_normal, pair rule)"""
    G, O = golden("ant_grids.npz"), golden("olive_grids.npz")
    out = [(k, np.ascontiguousarray(G[k], np.float32), float(G[k].max()), 0, False)
           for k in ("flint_b4_s", "int_b4_s", "pot_b4_s", "flint_b4_u", "int_b3_u")]
    for t in ("flint", "int"):
        gn, go = O["%s_b4_s" % t], O["outlier_b4_s"]
        out.append(("olive_" + t, np.ascontiguousarray(np.concatenate([gn, go]), np.float32), float(gn.max()), int(gn.size), True))
    return out


def _book(name):
    return [b for b in _books() if b[0] == name][0]


def _round(v, dtype_name):
    """fp32 -> the output type's bits, round to nearest even"""
    v = np.ascontiguousarray(v, np.float32)
    if dtype_name == "float32":
        return v.view(np.uint32)
    if dtype_name == "float16":
        with np.errstate(all="ignore"):
            return v.astype(np.float16).view(np.uint16)
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _value(bits, dtype_name):
    """the output type's bits -> float64"""
    if dtype_name == "float32":
        return bits.view(np.float32).astype(np.float64)
    if dtype_name == "float16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _yardstick(codes, alpha, rows, row_len, per_row, g, gmax, n_normal, ovp, dtype_name):
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
    return _round(v, dtype_name).reshape(rows, row_len)


def _image_bits(codes, alpha, K, N, per_row, book, dtype_name):
    """the yardstick's image of K rows of N codes as [K, N] bits"""
    name, g, gmax, nn, ovp = book
    return _yardstick(codes, alpha, K if per_row else 1, N if per_row else K * N, per_row, g, gmax, nn, ovp, dtype_name).reshape(K, N)


def _bits(t):
    import torch
    t = t.detach().contiguous()
    return (t.view(torch.int32).cpu().numpy().view(np.uint32) if t.dtype == torch.float32
            else t.view(torch.int16).cpu().numpy().view(np.uint16))


def _tensor(bits, dtype_name, dev):
    """bits (uint32 / uint16 array) -> a GPU tensor of the type"""
    import torch
    dt = getattr(torch, dtype_name)
    if dtype_name == "float32":
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.float32)).to(dev)
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(dt)


def _random_codes(rng, n_bytes, ovp):
    c = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    if ovp:
        c[rng.random(n_bytes) < 0.02] = 0xFF
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_one_hot_rows_read_the_image(antq_lib, dev, dtype_name):
    """x = e_k (and -2 e_k), 8 rows per call: y[m, :] is bit for bit row k of antq_decode4's image (times -2, exact) and of
    the numpy yardstick.  The codes hold every byte value; scales per row k, ordinary and so small that the smallest nonzero
    weights are subnormal in the output type, and per tensor."""
    import torch
    dt = getattr(torch, dtype_name)
    K, N = 136, 72
    tiny = 1.5e-4 if dtype_name == "float16" else 3.0e-38
    codes_np = np.concatenate([(np.arange(N // 2) + 37 * k) % 256 for k in range(K)]).astype(np.uint8)
    assert np.unique(codes_np).size == 256
    eye = torch.eye(K, device=dev, dtype=dt)
    eye_m2 = eye * -2
    codes = torch.from_numpy(codes_np).to(dev)
    per_k = np.resize(np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37]), K).astype(np.float32)
    for book in _books():
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for per_row, a_np in ((True, per_k), (False, np.float32([0.37])), (False, np.float32([tiny]))):
            a = torch.from_numpy(a_np).to(dev)
            want = _image_bits(codes_np, a_np, K, N, per_row, book, dtype_name)
            sub = np.abs(_value(want, dtype_name))
            lim = {"float32": 2.0 ** -126, "bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype_name]
            if a_np.min() <= tiny:
                assert ((sub > 0) & (sub < lim)).any(), "no subnormal weight in this case"
            image = antq_lib.decode4(codes, a, plan, gmax, K if per_row else 1, N if per_row else K * N, per_row, dt, n_normal=nn, ovp=ovp).view(K, N)
            assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode4 against the yardstick")
            # (exact: a doubling; + 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
            want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
            y1 = torch.empty(K, N, dtype=dt, device=dev)
            y2 = torch.empty(K, N, dtype=dt, device=dev)
            for k0 in range(0, K, 8):
                antq_lib.linear4_t(codes, eye[k0:k0 + 8], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + 8])
                antq_lib.linear4_t(codes, eye_m2[k0:k0 + 8], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + 8])
            torch.cuda.synchronize()
            assert np.array_equal(_bits(y1), want), (name, dtype_name, per_row, float(a_np.min()))
            assert np.array_equal(_bits(y2), want_m2), (name, dtype_name, per_row, float(a_np.min()), "-2 e_k")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_K = (8, 64, 72, 128, 136, 520, 1600)
EXACT_N = (8, 16, 32, 40, 56, 64, 72, 136)


def _lowest_bit_exponent(t):
    """exponent of the lowest set bit of every nonzero float64 in t"""
    m, e = np.frexp(t[t != 0])
    mi = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)


def _exact_case(rng, K, book, dtype_name, per_row, N=max(EXACT_N)):
    """Codes [K, N], power-of-two scales and small-integer x (8 rows) for which every product and every partial sum, in any
    order, is an integer below 2^24 in units of one power of two -- asserted here in float64 -- with the exact result.  A
    prefix of the columns is a narrower layer with the same property."""
    name, g, gmax, nn, ovp = book
    codes = _random_codes(rng, K * N // 2, ovp)
    j = rng.integers(-2, 2, K if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = _value(_image_bits(codes, alpha, K, N, per_row, book, dtype_name), dtype_name)    # [K, N]
    bias = rng.integers(-8, 9, N).astype(np.float64)
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (8, K)).astype(np.float64) * (rng.random((8, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        terms = x[:, :, None] * W[None, :, :]                          # [8, K, N]
        nz = np.abs(terms[terms != 0])
        unit = 2.0 ** min(int(_lowest_bit_exponent(terms).min()), 0)   # (the bias: whole numbers)
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


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_sums(antq_lib, dev, dtype_name):
    """Dyadic codebooks, power-of-two scales (per row k, and per tensor), small-integer activations: whatever the order of
    the sum, every partial sum is exact, so the result must be the exact one rounded to the type.  K and N on both sides of
    the tile rule's switch points (module docstring), M = 1..8, bias and none."""
    import torch
    rng = np.random.default_rng(5)
    for bname in ("pot_b4_s", "olive_int", "olive_flint"):
        book = _book(bname)
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for ki, K in enumerate(EXACT_K):
            per_row = ki % 2 == 0 or ovp
            NW = max(EXACT_N)
            codes_np, a_np, x_np, b_np, y_np, density = _exact_case(rng, K, book, dtype_name, per_row)
            x = _tensor(_round(x_np.astype(np.float32), dtype_name), dtype_name, dev)
            bias = _tensor(_round(b_np.astype(np.float32), dtype_name), dtype_name, dev)
            a = torch.from_numpy(a_np).to(dev)
            outs = []
            for ni, N in enumerate(EXACT_N):
                codes = torch.from_numpy(np.ascontiguousarray(codes_np.reshape(K, NW // 2)[:, :N // 2])).to(dev)
                for M in range(1, 9):
                    for with_bias in ((True, False) if (ni + M) % 3 == 0 else ((ni + M) % 2 == 0,)):
                        y = antq_lib.linear4_t(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N].clone() if with_bias else None,
                                               n_normal=nn, ovp=ovp)
                        outs.append((N, M, with_bias, y))
            torch.cuda.synchronize()
            assert {o[2] for o in outs} == {True, False} and {o[0] for o in outs} == set(EXACT_N)
            for N, M, with_bias, y in outs:
                want = y_np[:M, :N] + (b_np[None, :N] if with_bias else 0.0)
                assert y.shape == (M, N)
                assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, N, M, with_bias, density)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss_case(antq_lib, dev, rng, book, dtype_name, K, N, M=8):
    """Gaussian weights [K, N] encoded row by row k (0.1 % planted outliers for the pair rule), Gaussian x and bias in the
    type; the yardstick's weights, float64 result and float64 mass S = sum |x W| + |bias|."""
    import torch
    name, g, gmax, nn, ovp = book
    plan = antq_lib.plan_for(g)
    w = rng.standard_normal((K, N)).astype(np.float32) * np.float32(0.05)
    if ovp:
        big = rng.random((K, N)) < 0.001
        w = np.where(big, np.sign(w) * np.float32(0.05) * rng.uniform(8, 20, (K, N)).astype(np.float32), w)
        a_np = (3 * w.std(1)).astype(np.float32)
    else:
        a_np = (np.abs(w).max(1) * np.float32(0.9)).astype(np.float32)
    if g.min() >= 0:
        w = np.abs(w)
    wt = _tensor(_round(w, dtype_name), dtype_name, dev)
    a = torch.from_numpy(a_np).to(dev)
    codes = antq_lib.encode4(wt, a, plan, gmax, K, N, True, n_normal=nn, ovp=ovp)
    codes_np = codes.cpu().numpy()
    if ovp:
        assert ((codes_np & 15) == 15).any() or ((codes_np >> 4) == 15).any()
    W = _value(_image_bits(codes_np, a_np, K, N, True, book, dtype_name), dtype_name)
    xb = _round(rng.standard_normal((M, K)).astype(np.float32), dtype_name)
    bb = _round(rng.standard_normal(N).astype(np.float32), dtype_name)
    x64, b64 = _value(xb, dtype_name), _value(bb, dtype_name)
    y64 = x64 @ W + b64[None, :]
    S = np.abs(x64) @ np.abs(W) + np.abs(b64)[None, :]
    return dict(codes=codes, a=a, gd=plan.grid_dev(dev), x=_tensor(xb, dtype_name, dev), bias=_tensor(bb, dtype_name, dev), y64=y64, S=S,
                gmax=gmax, nn=nn, ovp=ovp, N=N, K=K)


def _run(antq_lib, c, x):
    return antq_lib.linear4_t(c["codes"], x, c["a"], c["gd"], c["gmax"], c["N"], c["K"], True, bias=c["bias"], n_normal=c["nn"], ovp=c["ovp"])


def _within_bound(y, y64, S, K, dtype_name):
    """|y - y64| <= K 2^-23 S + 2^-p |y64|: the bound of an fp32 sum of K exact-or-fused products in any order, doubled, plus
    the rounding to the output type (p = 23 / 10 / 7)."""
    err = np.abs(y - y64)
    bound = K * 2.0 ** -23 * S + 2.0 ** -PREC[dtype_name] * np.abs(y64)
    return bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, dev, dtype_name):
    rng = np.random.default_rng(17)
    for bname in ("flint_b4_s", "int_b4_s", "olive_flint", "olive_int"):
        for K, N in ((768, 136), (3072, 72)):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, K, N)
            for M in (1, 3, 8):
                y = _run(antq_lib, c, c["x"][:M])
                ok, worst = _within_bound(_value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d N=%d M=%d: worst error / bound %.3g" % (bname, dtype_name, K, N, M, worst))
                assert ok, (bname, dtype_name, K, N, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, dev, dtype_name):
    rng = np.random.default_rng(29)
    for bname in ("flint_b4_s", "olive_flint"):
        for K in (72, 1600):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, K, 72)
            run = lambda x: _bits(_run(antq_lib, c, x))
            y8 = run(c["x"])
            assert np.array_equal(y8, run(c["x"])), (bname, dtype_name, K, "two runs")
            for m in range(8):
                assert np.array_equal(run(c["x"][m:m + 1])[0], y8[m]), (bname, dtype_name, K, m, "a row alone")
            for M in (2, 3, 4, 5, 6, 7):
                assert np.array_equal(run(c["x"][:M]), y8[:M]), (bname, dtype_name, K, M)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, dtype_name):
    """y between poisoned guard bands; x, codes, alpha and bias are tensors of exactly their sizes and come back unchanged."""
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    book = _book("olive_flint")
    name, g, gmax, nn, ovp = book
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in (8, 72, 520):
        for N in (72, 8):
            codes = torch.from_numpy(_random_codes(rng, K * N // 2, ovp)).to(dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, K)).astype(np.float32)).to(dev)
            bias = torch.randn(N, device=dev).to(dt)
            for M in (1, 3, 5, 8):
                x = torch.randn(M, K, device=dev).to(dt)
                keep = (x.clone(), codes.clone(), a.clone(), bias.clone())
                full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                y = full[GUARD:GUARD + M * N]
                antq_lib.linear4_t(codes, x, a, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
                checks.append((K, N, M, full, (x, codes, a, bias), keep))
    torch.cuda.synchronize()
    for K, N, M, full, now, keep in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, "guard words")
        assert not (b[GUARD:GUARD + M * N] == guard).all(), (dtype_name, K, N, M, "y not written")
        for what, t, t0 in zip(("x", "codes", "alpha", "bias"), now, keep):
            assert torch.equal(t, t0), (dtype_name, K, N, M, what)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. padding and non-finite values
# ---------------------------------------------------------------------------------------------------------------------------
def _nonfinite_case(rng, dtype_name, K, N=72, M=4):
    book = _book("flint_b4_s")
    name, g, gmax, nn, ovp = book
    codes_np = _random_codes(rng, K * N // 2, ovp)
    a_np = np.exp(rng.uniform(-3, 0, K)).astype(np.float32)
    xb = _round(rng.integers(-3, 4, (M, K)).astype(np.float32), dtype_name)
    return book, codes_np, a_np, xb


def _product(xb, codes_np, a_np, K, N, book, dtype_name):
    """x64 @ (the yardstick's image) with IEEE non-finite values, as float64"""
    W = _value(_image_bits(codes_np, a_np, K, N, True, book, dtype_name), dtype_name)
    with np.errstate(all="ignore"):
        return _value(xb, dtype_name) @ W, W


@pytest.mark.parametrize("K", [72, 136])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_padding_and_non_finite_values(antq_lib, dev, dtype_name, K):
    """K = 72 leaves phases without any k, K = 136 is one pass over the 128 phases plus a partial one, and the last row of the
    codes has the Inf scale: the phases without that step must add +0, never a zero x against a weight (0 * Inf would be NaN).
    With a scale per k, a NaN or Inf alpha[k] makes ROW k of W non-finite -- that is the meaning of per-k scales: it reaches
    every row of y, also where x[m, k] == 0, exactly as x @ image does.  A NaN in x reaches its own row of y only."""
    import torch
    rng = np.random.default_rng(41)
    N, last = 72, K - 1
    book, codes_np, a_np, xb = _nonfinite_case(rng, dtype_name, K)
    name, g, gmax, nn, ovp = book
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)

    def run(codes_np, a_np, xb):
        y = antq_lib.linear4_t(torch.from_numpy(codes_np).to(dev), _tensor(xb, dtype_name, dev), torch.from_numpy(a_np).to(dev), gd, gmax,
                               N, K, True, n_normal=nn, ovp=ovp)
        return _value(_bits(y), dtype_name)

    one = _round(np.float32([1.0]), dtype_name)[0]
    # (a) alpha[K - 1] = +Inf, a positive code in column n0 of row K - 1, x[m, K - 1] = 1: +Inf, not NaN
    pos = int(np.argmax(g))
    n0 = 10
    c = codes_np.copy().reshape(K, N // 2)
    c[last, n0 // 2] = (c[last, n0 // 2] & 0xF0) | pos
    a = a_np.copy()
    a[last] = np.inf
    x = xb.copy()
    x[:, last] = one
    y = run(c.reshape(-1), a, x)
    want, W = _product(x, c.reshape(-1), a, K, N, book, dtype_name)
    assert W[last, n0] == np.inf and np.isfinite(W[:last]).all()
    assert (y[:, n0] == np.inf).all(), (dtype_name, y[:, n0])
    assert np.array_equal(np.isnan(y), np.isnan(want)) and np.array_equal(np.isinf(y), np.isinf(want))
    assert np.array_equal(y[np.isinf(want)], want[np.isinf(want)])
    # (b) a NaN in x[2, 5] reaches row 2 only
    x = xb.copy()
    x[2, 5] = _round(np.float32([np.nan]), dtype_name)[0]
    y = run(codes_np, a_np, x)
    assert np.isnan(y[2]).all() and np.isfinite(np.delete(y, 2, 0)).all()
    clean = run(codes_np, a_np, xb)
    assert np.array_equal(np.delete(y, 2, 0), np.delete(clean, 2, 0))
    # (c) a NaN alpha[3]: row 3 of W is NaN, so is every y[m, n] -- what x @ image gives
    a = a_np.copy()
    a[3] = np.nan
    x = xb.copy()
    x[1, 3] = 0
    y = run(codes_np, a, x)
    want, W = _product(x, codes_np, a, K, N, book, dtype_name)
    assert np.isnan(W[3]).all() and np.isnan(want).all() and np.isnan(y).all()
    image = antq_lib.decode4(torch.from_numpy(codes_np).to(dev), torch.from_numpy(a).to(dev), plan, gmax, K, N, True,
                             getattr(torch, dtype_name), n_normal=nn, ovp=ovp).view(K, N)
    ref = _tensor(x, dtype_name, dev).float() @ image.float()
    assert bool(torch.isnan(ref).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 7. module level
# ---------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _conv1d_model(dev, dt, K=136, N=72, seed=1):
    """nn.Sequential of one OliVe Conv1dQuantizer (4-bit, flint) built from a plain stand-in for HF's Conv1D"""
    import torch
    import torch.nn as nn
    from ant_quantization_amd.olive import quant_utils as qutil
    from ant_quantization_amd.olive.quant_modules import Conv1dQuantizer
    torch.manual_seed(seed)
    conv = types.SimpleNamespace(nf=N, weight=nn.Parameter(torch.randn(K, N) * 0.05), bias=nn.Parameter(torch.randn(N) * 0.1))
    layer = Conv1dQuantizer(mode="flint", wbit=4, abit=4, args=_args(mode="flint", wbit=4, abit=4))
    layer.set_param(conv)
    model = nn.Sequential(layer).to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    return model, qutil


def _layer_forward(model, x):
    """(output, the layer's own quantised input)"""
    seen = []
    h = model[0].quant_input.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    try:
        y = model(x)
    finally:
        h.remove()
    return y, seen[0]


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_packed_conv1d_layer(antq_lib, dev, dtype_name, capsys):
    import torch
    dt = getattr(torch, dtype_name)
    K, N = 136, 72
    base, qutil = _conv1d_model(dev, dt, K, N)
    gen = torch.Generator(device=dev).manual_seed(3)
    x1, x8, x9 = (torch.randn(r, K, device=dev, generator=gen).to(dt) for r in (1, 8, 9))
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        plain, twin, fused, lean = (copy.deepcopy(base) for _ in range(4))
        # without the option: today's path, every counter 0, with and without fused_linear
        pbank = qutil.pack_model(plain)
        tbank = qutil.pack_model(twin, fused_linear=True, keep_images=False)
        (pe,), (te,) = pbank.entries.values(), tbank.entries.values()
        assert pe["width"] == 4 and pe["shape"] == (K, N) and pe["per_row"] and pe["rows"] == K
        assert not te["fusable"] and te["out"] is not None             # a Conv1D entry keeps its image without fused_conv1d
        image = pe["out"]
        want = {}
        for x in (x1, x8, x9):
            want[x.shape[0]] = plain(x)
            assert torch.equal(twin(x), want[x.shape[0]])
            assert torch.equal(want[x.shape[0]], torch.addmm(plain[0].bias, plain[0].quant_input(x), image))
        for b in (pbank, tbank):
            assert (b.fused_t_calls, b.fused_calls, b.fused_mm_calls, b.fused_gemm_calls, b.fused_byte_calls) == (0, 0, 0, 0, 0)

        # fused_conv1d, image kept
        fbank = qutil.pack_model(fused, fused_linear=True, fused_conv1d=True)
        (fe,) = fbank.entries.values()
        assert fe["fusable"] and fe["kind"] == "conv1d" and fe["out"] is not None and fbank.nbytes() == pbank.nbytes()
        assert torch.equal(fe["out"], image)
        b64 = fused[0].bias.detach().double().cpu().numpy()
        W = image.double().cpu().numpy()
        for calls, x in enumerate((x1, x8), 1):
            y, xq = _layer_forward(fused, x)
            assert fbank.fused_t_calls == calls and y.shape == (x.shape[0], N) and y.dtype == dt
            x64 = xq.double().cpu().numpy()
            y64 = x64 @ W + b64[None, :]
            S = np.abs(x64) @ np.abs(W) + np.abs(b64)[None, :]
            ok, worst = _within_bound(y.double().cpu().numpy(), y64, S, K, dtype_name)
            assert ok, (dtype_name, x.shape[0], worst)
        assert torch.equal(fused(x9), want[9]) and fbank.fused_t_calls == 2      # 9 rows: the layer's addmm on the image
        assert fbank.fused_calls == 0

        # no image: codes + one scratch
        lbank = qutil.pack_model(lean, fused_linear=True, fused_conv1d=True, keep_images=False)
        (le,) = lbank.entries.values()
        assert le["out"] is None and le["kind"] == "conv1d"
        assert lbank.nbytes() == (pbank.nbytes()[0], image.numel() * image.element_size())   # (the scratch stands in)
        assert len(lbank._scratch) == 1
        assert torch.equal(lean(x9), want[9]) and lbank.fused_t_calls == 0
        assert torch.equal(lean(x8), fused(x8)) and torch.equal(lean(x1), fused(x1)) and lbank.fused_t_calls == 2
        assert torch.equal(lean(x9), want[9])
    # a forward that wants gradients: there is no float weight to train
    with pytest.raises(antq_lib.AntqError):
        fused(x1)
    capsys.readouterr()
