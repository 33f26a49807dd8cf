"""The packed 4-bit linear for [K, N] weights (GPT-2's Conv1D) on the GPU: antq_linear4_t (csrc/antq_k_linear_t.h) computes
y = x . W (+ bias) from the code bytes, W being the image antq_decode4 writes for K rows of N codes with one scale per row k.
The yardstick is that of tests/test_gpu_linear4.py -- include/antq.h's decode rule restated in numpy on the code bytes, and a
float64 product x64 @ W -- with the rows of the codes being k.  Exact tests compare bits; the general test holds the result
to the bound of an fp32 sum; the order of the sum that include/antq.h fixes (the tile rule) is held bit for bit against its
restatement in numpy (tests/linear_t_cases.py, proved on the CPU by tests/test_linear_t_cases_host.py), up to K = 8200 where
the scales are no longer staged in LDS.

Shapes: the kernel's tile rule has two switch points only -- 128 phases of k (K = 8 ... 72 stay inside a partial pass, 128 is
exactly one pass, 136 one pass plus a partial one, 520 and 1600 are several passes -- at 1600 more than one group of steps in
flight -- plus a partial one) and 32 columns per workgroup (N = 8, 16 a partial tile, 32 exactly one, 40 ... 136 whole tiles plus
a partial one, 64 two whole tiles).  K = 128, 136 and N = 32, 40 are here for those switch points, beside the shapes the
kernel's issue named for a 64-phase, 64-column tile."""
import copy
import types

import numpy as np
import pytest

import linear_t_cases as lt
from linear_t_cases import DTYPES, PREC
from linear_t_cases import books as _books, book as _book, round_bits as _round, value as _value, image_bits as _image_bits
from linear_t_cases import random_codes as _random_codes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


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
            codes_np, a_np, x_np, b_np, y_np, density = lt.exact_case(rng, K, book, dtype_name, per_row, max(EXACT_N))
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


def _check_guard_words(antq_lib, dev, dtype_name, Ks, Ns, Ms):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    book = _book("olive_flint")
    name, g, gmax, nn, ovp = book
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in Ks:
        for N in Ns:
            codes = torch.from_numpy(_random_codes(rng, K * N // 2, ovp)).to(dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, K)).astype(np.float32)).to(dev)
            bias = torch.randn(N, device=dev).to(dt)
            for M in Ms:
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


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, dtype_name):
    """y between poisoned guard bands; x, codes, alpha and bias are tensors of exactly their sizes and come back unchanged."""
    _check_guard_words(antq_lib, dev, dtype_name, (8, 72, 520), (72, 8), (1, 3, 5, 8))


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
# 7. the order of the sum: include/antq.h's tile rule, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_bits_follow_the_tile_rule(antq_lib, dev, dtype_name):
    """The kernel's bits are those of linear_t_cases.tile_rule -- the text of include/antq.h in numpy -- with no tolerance:
    Gaussian weights through two books (plain, pair rule with planted outliers), a scale per k and one per tensor, K on both
    sides of one pass over the 128 phases, of a group of steps in flight and of the staged scales (8192 | 8200), N = 8 and 40,
    1, 2, 3 and 8 rows; no bias, a Gaussian bias and, for the 16-bit types, the biases that bring the low bits of the fp32
    sum into the output (cancelling, near-tie).  test_linear_t_cases_host.py shows how many of these outputs another fixed
    order would change: float32 carries the test."""
    import torch
    dt = getattr(torch, dtype_name)
    for c in lt.rule_cases(dtype_name):
        name, g, gmax, nn, ovp = c["book"]
        K, per_row = c["K"], c["per_row"]
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        sums = lt.rule_sums(c["x"], c["W"], dtype_name)
        variants = lt.bias_variants(c, sums)
        a = torch.from_numpy(c["alpha"]).to(dev)
        x = _tensor(c["x"], dtype_name, dev)
        image = antq_lib.decode4(torch.from_numpy(c["codes"]).to(dev), a, plan, gmax, K if per_row else 1, c["N"] if per_row else K * c["N"],
                                 per_row, dt, n_normal=nn, ovp=ovp)
        runs = []
        for N in lt.RULE_N:
            d = lt.columns(c, N)
            codes = torch.from_numpy(d["codes"]).to(dev)
            for vname, bias, rows in variants:
                b = None if bias is None else _tensor(bias[:N], dtype_name, dev)
                want = lt.finish(sums[:, :N], None if bias is None else bias[:N], dtype_name)
                for M in lt.RULE_M:
                    if rows is not None and min(rows) >= M:      # (a row's cancelling bias: calls that hold the row)
                        continue
                    y = antq_lib.linear4_t(codes, x[:M], a, gd, gmax, N, K, per_row, bias=b, n_normal=nn, ovp=ovp)
                    runs.append((N, vname, M, y, want[:M]))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(image).reshape(K, c["N"]), c["W"]), (lt.case_id(c), "antq_decode4 against the yardstick")
        assert {r[1] for r in runs} >= {"none", "gauss"} and {r[2] for r in runs} == set(lt.RULE_M)
        for N, vname, M, y, want in runs:
            got = _bits(y)
            assert got.shape == want.shape == (M, N)
            assert np.array_equal(got, want), (lt.case_id(c), N, vname, M, "%d of %d outputs differ" % (int((got != want).sum()), got.size))


# ---------------------------------------------------------------------------------------------------------------------------
# 8. K > 8192: the scales divided per step instead of staged
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [lt.STAGED_K, lt.STAGED_K + 8])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_unstaged_scales_have_the_same_bits(antq_lib, dev, dtype_name, K):
    """The last K whose scales are staged in LDS and the first one beyond (a lane then divides alpha[k] / gmax per step): one-hot
    rows read the image, the order-free sums are exact, and nothing outside y is written.  (The order of the sum at these K
    is test_bits_follow_the_tile_rule's.)"""
    import torch
    dt = getattr(torch, dtype_name)
    N = 40
    # (a) one-hot rows e_k, 8 per call: the first and last k, both sides of the first pass, the last staged index, two mid ones
    tiny = 1.5e-4 if dtype_name == "float16" else 3.0e-38
    ks = [0, 127, 128, lt.STAGED_K - 1, K - 1, 4102, 6004, 127]
    assert len(ks) == 8 and max(ks) < K and {lt.STAGED_K - 1, K - 1} <= set(ks)
    codes_np = np.concatenate([(np.arange(N // 2) + 37 * k) % 256 for k in range(K)]).astype(np.uint8)
    assert np.unique(codes_np).size == 256
    per_k = np.resize(np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37]), K).astype(np.float32)
    assert {float(per_k[k]) for k in ks} == {float(v) for v in np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37])}
    xh = np.zeros((8, K), np.float32)
    xh[np.arange(8), ks] = 1.0
    x = _tensor(_round(xh, dtype_name), dtype_name, dev)
    codes, a = torch.from_numpy(codes_np).to(dev), torch.from_numpy(per_k).to(dev)
    lim = {"float32": 2.0 ** -126, "bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype_name]
    for book in _books():
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        want = _image_bits(codes_np, per_k, K, N, True, book, dtype_name)
        sub = np.abs(_value(want[ks], dtype_name))
        assert ((sub > 0) & (sub < lim)).any(), "no subnormal weight in these rows"
        image = antq_lib.decode4(codes, a, plan, gmax, K, N, True, dt, n_normal=nn, ovp=ovp).view(K, N)
        y = antq_lib.linear4_t(codes, x, a, plan.grid_dev(dev), gmax, N, K, True, n_normal=nn, ovp=ovp)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(image), want), (name, dtype_name, K, "antq_decode4 against the yardstick")
        assert np.array_equal(_bits(y), want[ks]), (name, dtype_name, K)
    # (b) order-free exact sums
    rng = np.random.default_rng(53)
    for bname in ("pot_b4_s", "olive_flint"):
        book = _book(bname)
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        codes_e, a_e, x_e, b_e, y_e, density = lt.exact_case(rng, K, book, dtype_name, True, N)
        xe = _tensor(_round(x_e.astype(np.float32), dtype_name), dtype_name, dev)
        be = _tensor(_round(b_e.astype(np.float32), dtype_name), dtype_name, dev)
        ce, ae = torch.from_numpy(codes_e).to(dev), torch.from_numpy(a_e).to(dev)
        outs = [(M, wb, antq_lib.linear4_t(ce, xe[:M], ae, plan.grid_dev(dev), gmax, N, K, True, bias=be if wb else None, n_normal=nn, ovp=ovp))
                for M in (1, 3, 8) for wb in (True, False)]
        torch.cuda.synchronize()
        for M, wb, y in outs:
            want = y_e[:M] + (b_e[None, :] if wb else 0.0)
            assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, M, wb, density)
    # (c) footprint
    if K > lt.STAGED_K:
        _check_guard_words(antq_lib, dev, dtype_name, (K,), (8, 40), (1, 8))


# ---------------------------------------------------------------------------------------------------------------------------
# 9. module level
# ---------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _conv1d_model(dev, dt, K=136, N=72, seed=1, eight_bit=False):
    """nn.Sequential of one OliVe Conv1dQuantizer (4-bit, flint; eight_bit: reset to 8 bits the way a mixed-precision model's
    layers are) built from a plain stand-in for HF's Conv1D"""
    import torch
    import torch.nn as nn
    from ant_quantization_amd.olive import quant_utils as qutil
    from ant_quantization_amd.olive.quant_modules import Conv1dQuantizer
    torch.manual_seed(seed)
    conv = types.SimpleNamespace(nf=N, weight=nn.Parameter(torch.randn(K, N) * 0.05), bias=nn.Parameter(torch.randn(N) * 0.1))
    layer = Conv1dQuantizer(mode="flint", wbit=4, abit=4, args=_args(mode="flint", wbit=4, abit=4))
    layer.set_param(conv)
    model = nn.Sequential(layer)
    if eight_bit:
        from ant_quantization_amd.olive import quant_model as qmod
        qmod.set_8_bit_layer_l(model, "0")
    model = model.to(dev).to(dt).eval()
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


COUNTERS = ("fused_t_calls", "fused_calls", "fused_mm_calls", "fused_gemm_calls", "fused_byte_calls", "fused_byte_mm_calls", "fused_byte_gemm_calls")


def _counters(bank):
    return tuple(getattr(bank, n) for n in COUNTERS)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_packed_conv1d_reload_capture_retype(antq_lib, dev, dtype_name, capsys):
    """What every sibling kernel's module test does, for the Conv1D path: a packed checkpoint loaded into a fresh model, a
    forward captured into a graph and replayed, the model retyped."""
    import torch
    dt = getattr(torch, dtype_name)
    K, N = 136, 72
    base, qutil = _conv1d_model(dev, dt, K, N)
    gen = torch.Generator(device=dev).manual_seed(3)
    x1, x3, x8, x9 = (torch.randn(r, K, device=dev, generator=gen).to(dt) for r in (1, 3, 8, 9))
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        lean = copy.deepcopy(base)
        lbank = qutil.pack_model(lean, fused_linear=True, fused_conv1d=True, keep_images=False)
        want = {x.shape[0]: lean(x) for x in (x1, x3, x8, x9)}
        assert _counters(lbank) == (3, 0, 0, 0, 0, 0, 0)               # 9 rows: the layer's addmm on the scratch decode

        # the checkpoint holds codes and no weight: into a differently seeded model with the same options
        sd = qutil.packed_state_dict(lean)
        assert "0.weight" not in sd and sd["0.quant_weight.codes"].dtype == torch.uint8 and sd["0.quant_weight.codes"].numel() == K * N // 2
        fresh, _ = _conv1d_model(dev, dt, K, N, seed=99)
        assert not torch.equal(fresh[0].bias, lean[0].bias)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, fused_conv1d=True, keep_images=False)
        (e2,) = bank2.entries.values()
        assert e2["fusable"] and e2["kind"] == "conv1d" and e2["out"] is None and e2["width"] == 4 and e2["shape"] == (K, N)
        assert torch.equal(e2["codes"], sd["0.quant_weight.codes"])
        for calls, x in ((1, x1), (2, x8), (2, x9)):
            assert torch.equal(fresh(x), want[x.shape[0]]), (dtype_name, x.shape[0])
            assert _counters(bank2) == (calls, 0, 0, 0, 0, 0, 0)

        # a captured 3-row forward replays to the same bits (one stream, no parallel branches)
        static_x = x3.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_calls = lbank.fused_t_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_t_calls == n_calls + 1
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, want[3]), (dtype_name, step)
        assert lbank.fused_t_calls == n_calls + 1

        # the model retyped: the bank rebuilds codes, scales and scratch from the shape it remembers (bf16 <-> fp32)
        other = torch.float32 if dt == torch.bfloat16 else torch.bfloat16
        fresh.to(other)
        before = _counters(bank2)
        for x in (x1, x9):
            y = fresh(x.to(other))
            assert y.dtype == other and y.shape == (x.shape[0], N) and bool(torch.isfinite(y.float()).all())
        assert _counters(bank2) == (before[0] + 1,) + before[1:]        # the 1-row call from the codes, the 9-row one not
        assert all(t.dtype == other for t in bank2._scratch.values()) and len(bank2._scratch) == 1
        assert e2["out"] is None and e2["codes"].dtype == torch.uint8 and e2["dtype"] == other
    capsys.readouterr()


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("what", ["K = 132", "byte codes"])
def test_conv1d_layers_the_kernel_does_not_take(antq_lib, dev, dtype_name, what, capsys):
    """A Conv1D layer whose K is no multiple of 8, and a byte-coded (8-bit) one, packed with fused_conv1d=True: the entry is
    not fusable, keeps its image whatever keep_images says, no call is counted, and the output is the layer's own addmm on the
    image, bit for bit -- the same as without the option."""
    import torch
    dt = getattr(torch, dtype_name)
    byte = what == "byte codes"
    K, N = (136, 72) if byte else (132, 72)
    base, qutil = _conv1d_model(dev, dt, K, N, eight_bit=byte)
    gen = torch.Generator(device=dev).manual_seed(3)
    xs = [torch.randn(r, K, device=dev, generator=gen).to(dt) for r in (1, 8, 9)]
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        plain, fused = copy.deepcopy(base), copy.deepcopy(base)
        pbank = qutil.pack_model(plain, byte_codes=byte)
        fbank = qutil.pack_model(fused, fused_linear=True, fused_conv1d=True, keep_images=False, byte_codes=byte, fused_bytes=byte)
        (pe,), (fe,) = pbank.entries.values(), fbank.entries.values()
        assert pe["width"] == fe["width"] == (8 if byte else 4) and fe["shape"] == (K, N) and fbank.skipped == []
        assert not fe["fusable"] and fe["kind"] == "linear" and fe["out"] is not None and torch.equal(fe["out"], pe["out"])
        assert len(fbank._scratch) == 0
        for x in xs:
            y = fused(x)
            assert y.shape == (x.shape[0], N) and y.dtype == dt
            assert torch.equal(y, torch.addmm(fused[0].bias, fused[0].quant_input(x), fe["out"])), (what, dtype_name, x.shape[0])
            assert torch.equal(y, plain(x)), (what, dtype_name, x.shape[0])
        assert _counters(fbank) == (0,) * len(COUNTERS) and _counters(pbank) == (0,) * len(COUNTERS)
    capsys.readouterr()
