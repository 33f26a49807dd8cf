"""The matrix-core packed 4-bit linear for [K, N] weights (GPT-2's Conv1D) on the GPU: antq_linear4_t_mm
(csrc/antq_k_linear_t_mm.h) computes y = x . W (+ bias) for 1 .. 64 rows of x from the code bytes, W being the image antq_decode4
writes for K rows of N codes with one scale per row k.  The yardstick is antq_linear4_t's (tests/linear_t_cases.py: include/antq.h's
decode rule restated in numpy on the code bytes, and a float64 product x64 @ W); the inputs are built in tests/linear_t_mm_cases.py
and held to their premises on the CPU by tests/test_linear_t_mm_cases_host.py.  Exact tests compare bits; the general test holds
the result to the bound of an fp32 sum.

Shapes, at the switch points of the kernel's rule: steps of 32 k dealt to eight wavefronts (K = 8, 24 a partial step and
wavefronts without any; 32 one step; 40 one plus a partial one; 256 one pass of the eight; 264 a pass plus a partial step; 520
and 1600 several passes with unequal step counts), the staged scales (8192 | 8200), tiles of 16 rows of x (M = 1 ... 64 on both
sides of 16, 32, 48) and N on both sides of a 32-, 64- and 128-column tile."""
import copy

import numpy as np
import pytest

import linear_t_cases as lt
import linear_t_mm_cases as mc
from linear_t_mm_cases import DTYPES
from test_gpu_linear4_t import _bits, _tensor, _within_bound, _conv1d_model, _layer_forward

pytestmark = pytest.mark.gpu

_round, _value = lt.round_bits, lt.value


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _call(antq_lib, dev, c, x, N=None, bias=True, out=None):
    """antq_linear4_t_mm on a case dict (codes / alpha as numpy, x a tensor)"""
    import torch
    name, g, gmax, nn, ovp = c["book"]
    key = "_dev"
    if key not in c:
        c[key] = (torch.from_numpy(np.ascontiguousarray(c["codes"]).reshape(-1)).to(dev), torch.from_numpy(c["alpha"]).to(dev),
                  antq_lib.plan_for(g).grid_dev(dev), None if c.get("bias") is None else _tensor(c["bias"], c["dtype_name"], dev))
    codes, a, gd, b = c[key]
    return antq_lib.linear4_t_mm(codes, x, a, gd, gmax, c["N"], c["K"], c["per_row"], bias=b if bias else None, n_normal=nn, ovp=ovp, out=out)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_one_hot_rows_read_the_image(antq_lib, dev, dtype_name):
    """x = e_k (and -2 e_k), 64 rows per call, over all k of a [264, 72] layer: y[m, :] is bit for bit row k of antq_decode4's
    image (times -2, exact) and of the numpy yardstick.  Every book; the codes hold every byte value; scales per row k --
    ordinary and so small that the smallest nonzero weights are subnormal in the type -- and per tensor."""
    import torch
    dt = getattr(torch, dtype_name)
    K, N = mc.ONE_HOT_K, mc.ONE_HOT_N
    codes_np = mc.all_byte_codes(K, N)
    eye = torch.eye(K, device=dev, dtype=dt)
    eye_m2 = eye * -2
    codes = torch.from_numpy(codes_np).to(dev)
    for book in lt.books():
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for per_row, a_np, has_tiny in mc.one_hot_scales(dtype_name, K):
            a = torch.from_numpy(a_np).to(dev)
            want = lt.image_bits(codes_np, a_np, K, N, per_row, book, dtype_name)
            if has_tiny:
                sub = np.abs(_value(want, dtype_name))
                assert ((sub > 0) & (sub < mc.subnormal_limit(dtype_name))).any(), "no subnormal weight in this case"
            image = antq_lib.decode4(codes, a, plan, gmax, K if per_row else 1, N if per_row else K * N, per_row, dt, n_normal=nn, ovp=ovp).view(K, N)
            want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
            y1 = torch.empty(K, N, dtype=dt, device=dev)
            y2 = torch.empty(K, N, dtype=dt, device=dev)
            for k0 in range(0, K, mc.MAX_M):
                antq_lib.linear4_t_mm(codes, eye[k0:k0 + mc.MAX_M], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + mc.MAX_M])
                antq_lib.linear4_t_mm(codes, eye_m2[k0:k0 + mc.MAX_M], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + mc.MAX_M])
            torch.cuda.synchronize()
            assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode4 against the yardstick")
            assert np.array_equal(_bits(y1), want), (name, dtype_name, per_row, float(a_np.min()))
            assert np.array_equal(_bits(y2), want_m2), (name, dtype_name, per_row, float(a_np.min()), "-2 e_k")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_sums(antq_lib, dev, dtype_name):
    """Dyadic codebooks, power-of-two scales (per row k, and per tensor), small-integer activations: whatever the order of
    the sum, every partial sum is exact, so the result must be the exact one rounded to the type.  The whole K x N x M grid of
    the module docstring; bias and none thinned as test_gpu_linear4_t.test_exact_sums thins them."""
    import torch
    rng = np.random.default_rng(5)
    NW = max(mc.GRID_N)
    for bname in mc.EXACT_BOOKS:
        book = lt.book(bname)
        name, g, gmax, nn, ovp = book
        gd = antq_lib.plan_for(g).grid_dev(dev)
        for ki, K in enumerate(mc.GRID_K):
            per_row = ki % 2 == 0 or ovp
            codes_np, a_np, x_np, b_np, y_np, density = mc.exact_case(rng, K, book, dtype_name, per_row, NW)
            x = _tensor(_round(x_np.astype(np.float32), dtype_name), dtype_name, dev)
            bias = _tensor(_round(b_np.astype(np.float32), dtype_name), dtype_name, dev)
            a = torch.from_numpy(a_np).to(dev)
            outs = []
            for ni, N in enumerate(mc.GRID_N):
                codes = torch.from_numpy(np.ascontiguousarray(codes_np.reshape(K, NW // 2)[:, :N // 2])).to(dev)
                for mi, M in enumerate(mc.GRID_M):
                    for with_bias in ((True, False) if (ni + mi) % 3 == 0 else ((ni + mi) % 2 == 0,)):
                        y = antq_lib.linear4_t_mm(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N].clone() if with_bias else None,
                                                  n_normal=nn, ovp=ovp)
                        outs.append((N, M, with_bias, y))
            torch.cuda.synchronize()
            assert {o[2] for o in outs} == {True, False} and {o[0] for o in outs} == set(mc.GRID_N) and {o[1] for o in outs} == set(mc.GRID_M)
            for N, M, with_bias, y in outs:
                want = y_np[:M, :N] + (b_np[None, :N] if with_bias else 0.0)
                assert y.shape == (M, N)
                assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, N, M, with_bias, density)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
_GAUSS = {}


def _gauss(dtype_name, K, N, bname):
    """a shared Gaussian case: built once, left unchanged"""
    key = (dtype_name, K, N, bname)
    if key not in _GAUSS:
        _GAUSS[key] = mc.gauss_case(dtype_name, K, N, bname)
    return _GAUSS[key]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, dev, dtype_name):
    """|y - y64| <= K 2^-23 S + 2^-p |y64| against the float64 product with the yardstick's image (the project's derived bound
    of an fp32 sum, test_gpu_linear4_t._within_bound); the pair rule's cases carry planted outliers."""
    for bname in ("flint_b4_s", "olive_flint"):
        for K, N in ((768, 136), (3072, 72)):
            c = _gauss(dtype_name, K, N, bname)
            if c["book"][4]:
                assert mc.has_pair_identifier(c["codes"])
            x = _tensor(c["x"], dtype_name, dev)
            for M in (9, 33, 64):
                y = _call(antq_lib, dev, c, x[:M])
                ok, worst = _within_bound(_value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d N=%d M=%d: worst error / bound %.3g" % (bname, dtype_name, K, N, M, worst))
                assert ok, (bname, dtype_name, K, N, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. invariance, by bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [40, 264, 1600])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_bits_depend_on_the_row_the_column_and_k_only(antq_lib, dev, dtype_name, K):
    """Two runs are equal; row m alone, and at every position 0 .. 15 of a tile and in each of the four M tiles, has the bits it
    has in the call of 64; a column computed as a layer of N = 8 has the bits it has inside N = 136; a layer shifted by 8
    columns -- every column at another place in its tile -- has the same bits."""
    import torch
    for bname in ("flint_b4_s", "olive_flint"):
        c = _gauss(dtype_name, K, 136, bname)
        x = _tensor(c["x"], dtype_name, dev)
        run = lambda case, xs: _bits(_call(antq_lib, dev, case, xs))
        y64 = run(c, x)
        assert np.array_equal(y64, run(c, x)), (bname, dtype_name, K, "two runs")
        # a row alone
        for m in (0, 5, 15, 16, 31, 32, 47, 48, 63):
            assert np.array_equal(run(c, x[m:m + 1])[0], y64[m]), (bname, dtype_name, K, m, "a row alone")
        # row m of the call at every position of a tile, in each of the four M tiles: a call whose row p is that row
        m = 21
        for tile in range(4):
            xs = x.clone()
            for p in range(16):
                xs[16 * tile + p] = x[m]
            got = run(c, xs)
            for p in range(16):
                assert np.array_equal(got[16 * tile + p], y64[m]), (bname, dtype_name, K, tile, p, "position in the tile")
            keep = [i for i in range(64) if not 16 * tile <= i < 16 * tile + 16]
            assert np.array_equal(got[keep], y64[keep]), (bname, dtype_name, K, tile, "the other rows")
        for M in (9, 16, 17, 33, 48, 49):
            assert np.array_equal(run(c, x[:M]), y64[:M]), (bname, dtype_name, K, M)
        # the first columns as a layer of their own
        d = lt.columns(c, 8)
        d.pop("_dev", None)
        assert np.array_equal(run(d, x), y64[:, :8]), (bname, dtype_name, K, "N = 8 against N = 136")
        # every column 8 places further left in its tile
        s = mc.shifted(c, 8)
        s.pop("_dev", None)
        assert np.array_equal(run(s, x), y64[:, 8:]), (bname, dtype_name, K, "shifted by 8 columns")
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _check_guard_words(antq_lib, dev, dtype_name, Ks, Ns, Ms):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    name, g, gmax, nn, ovp = lt.book("olive_flint")
    gd = antq_lib.plan_for(g).grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in Ks:
        for N in Ns:
            codes = torch.from_numpy(lt.random_codes(rng, K * N // 2, ovp)).to(dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, K)).astype(np.float32)).to(dev)
            bias = torch.randn(N, device=dev).to(dt)
            for M in Ms:
                x = torch.randn(M, K, device=dev).to(dt)
                keep = (x.clone(), codes.clone(), a.clone(), bias.clone())
                full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                y = full[GUARD:GUARD + M * N]
                antq_lib.linear4_t_mm(codes, x, a, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
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
    _check_guard_words(antq_lib, dev, dtype_name, (8, 40, 520), (8, 72), (9, 17, 64))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. padding and non-finite values
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [40, 264])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_padding_and_non_finite_values(antq_lib, dev, dtype_name, K):
    """K = 40 and 264 end in a partial step, and the last row of the codes has the Inf scale: the k groups past the end of K
    must add +0, never a zero x against a weight (0 * Inf would be NaN).  M = 9: padded rows of x exist beside the Inf weights
    and are not seen.  A NaN or Inf alpha[k] makes ROW k of W non-finite and reaches every row of y, as x @ image does; a NaN
    in x reaches its own row only."""
    import torch
    rng = np.random.default_rng(41)
    N, M, last = 72, 9, K - 1
    book = lt.book("flint_b4_s")
    name, g, gmax, nn, ovp = book
    codes_np = lt.random_codes(rng, K * N // 2, ovp)
    a_np = np.exp(rng.uniform(-3, 0, K)).astype(np.float32)
    xb = _round(rng.integers(-3, 4, (M, K)).astype(np.float32), dtype_name)
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)

    def run(codes_np, a_np, xb):
        y = antq_lib.linear4_t_mm(torch.from_numpy(codes_np).to(dev), _tensor(xb, dtype_name, dev), torch.from_numpy(a_np).to(dev), gd, gmax,
                                  N, K, True, n_normal=nn, ovp=ovp)
        return _value(_bits(y), dtype_name)

    def product(xb, codes_np, a_np):
        W = _value(lt.image_bits(codes_np, a_np, K, N, True, book, dtype_name), dtype_name)
        with np.errstate(all="ignore"):
            return _value(xb, dtype_name) @ W, W

    one = _round(np.float32([1.0]), dtype_name)[0]
    # (a) alpha[K - 1] = +Inf, a positive code in column n0 of row K - 1, x[m, K - 1] = 1: +Inf, not NaN
    pos, n0 = int(np.argmax(g)), 10
    c = codes_np.copy().reshape(K, N // 2)
    c[last, n0 // 2] = (c[last, n0 // 2] & 0xF0) | pos
    a = a_np.copy()
    a[last] = np.inf
    x = xb.copy()
    x[:, last] = one
    y = run(c.reshape(-1), a, x)
    want, W = product(x, c.reshape(-1), a)
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
    want, W = product(x, codes_np, a)
    assert np.isnan(W[3]).all() and np.isnan(want).all() and np.isnan(y).all()
    image = antq_lib.decode4(torch.from_numpy(codes_np).to(dev), torch.from_numpy(a).to(dev), plan, gmax, K, N, True,
                             getattr(torch, dtype_name), n_normal=nn, ovp=ovp).view(K, N)
    assert bool(torch.isnan(_tensor(x, dtype_name, dev).float() @ image.float()).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 7. K > 8192: the scales divided per use instead of staged
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [mc.STAGED_K, mc.STAGED_K + 8])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_unstaged_scales_have_the_same_bits(antq_lib, dev, dtype_name, K):
    """The last K whose scales are staged in LDS and the first one beyond (a lane then divides alpha[k] / gmax per use): one-hot
    rows read the image, the order-free sums are exact, and beyond the limit nothing outside y is written."""
    import torch
    dt = getattr(torch, dtype_name)
    N = 40
    tiny = mc.tiny_scale(dtype_name)
    # the first and last k, both sides of the first step and of the first pass, the last staged index, and every scale of per_k
    ks = [0, 31, 32, 255, 256, mc.STAGED_K - 1, K - 1, 4102, 6004, 8, 263]
    assert max(ks) < K and {mc.STAGED_K - 1, K - 1} <= set(ks)
    codes_np = mc.all_byte_codes(K, N)
    per_k = np.resize(np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37]), K).astype(np.float32)
    assert {float(per_k[k]) for k in ks} == {float(v) for v in np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37])}
    xh = np.zeros((len(ks), K), np.float32)
    xh[np.arange(len(ks)), ks] = 1.0
    x = _tensor(_round(xh, dtype_name), dtype_name, dev)
    codes, a = torch.from_numpy(codes_np).to(dev), torch.from_numpy(per_k).to(dev)
    for book in lt.books():
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        want = lt.image_bits(codes_np, per_k, K, N, True, book, dtype_name)
        sub = np.abs(_value(want[ks], dtype_name))
        assert ((sub > 0) & (sub < mc.subnormal_limit(dtype_name))).any(), "no subnormal weight in these rows"
        y = antq_lib.linear4_t_mm(codes, x, a, plan.grid_dev(dev), gmax, N, K, True, n_normal=nn, ovp=ovp)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(y), want[ks]), (name, dtype_name, K)
    rng = np.random.default_rng(53)
    for bname in ("pot_b4_s", "olive_flint"):
        book = lt.book(bname)
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        codes_e, a_e, x_e, b_e, y_e, density = mc.exact_case(rng, K, book, dtype_name, True, N)
        xe = _tensor(_round(x_e.astype(np.float32), dtype_name), dtype_name, dev)
        be = _tensor(_round(b_e.astype(np.float32), dtype_name), dtype_name, dev)
        ce, ae = torch.from_numpy(codes_e).to(dev), torch.from_numpy(a_e).to(dev)
        outs = [(M, wb, antq_lib.linear4_t_mm(ce, xe[:M], ae, plan.grid_dev(dev), gmax, N, K, True, bias=be if wb else None, n_normal=nn, ovp=ovp))
                for M in (9, 33, 64) for wb in (True, False)]
        torch.cuda.synchronize()
        for M, wb, y in outs:
            want = y_e[:M] + (b_e[None, :] if wb else 0.0)
            assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, M, wb, density)
    if K > mc.STAGED_K:
        _check_guard_words(antq_lib, dev, dtype_name, (K,), (8, 40), (9, 64))


# ---------------------------------------------------------------------------------------------------------------------------
# 8. module level
# ---------------------------------------------------------------------------------------------------------------------------
COUNTERS = ("fused_t_calls", "fused_t_mm_calls", "fused_calls", "fused_mm_calls", "fused_gemm_calls", "fused_byte_calls",
            "fused_byte_mm_calls", "fused_byte_gemm_calls")


def _counters(bank):
    return tuple(getattr(bank, n) for n in COUNTERS)


def _direct(antq_lib, bank, e, xq, bias):
    """_lib.linear4_t_mm called on the entry's own codes"""
    from ant_quantization_amd.packed import _codebook
    plan, gmax, n_normal, ovp = _codebook(e["q"])
    K, N = e["shape"]
    return antq_lib.linear4_t_mm(e["codes"], xq, e["alpha"], plan.grid_dev(e["device"]), gmax, N, K, e["per_row"], bias=bias.detach(),
                                 n_normal=n_normal, ovp=ovp)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_packed_conv1d_layer_with_the_flag(antq_lib, dev, dtype_name, capsys):
    import torch
    dt = getattr(torch, dtype_name)
    half = dtype_name != "float32"
    K, N = 136, 72
    base, qutil = _conv1d_model(dev, dt, K, N)
    gen = torch.Generator(device=dev).manual_seed(3)
    x8, x9, x64, x65 = (torch.randn(r, K, device=dev, generator=gen).to(dt) for r in (8, 9, 64, 65))
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        plain, off, on, lean = (copy.deepcopy(base) for _ in range(4))
        pbank = qutil.pack_model(plain)
        obank = qutil.pack_model(off, fused_linear=True, fused_conv1d=True)
        image = next(iter(pbank.entries.values()))["out"]
        want = {x.shape[0]: plain(x) for x in (x8, x9, x64, x65)}
        # flag off: every output and counter is as today
        y8_t = off(x8)
        for x in (x9, x64, x65):
            assert torch.equal(off(x), want[x.shape[0]])
        assert _counters(obank) == (1, 0, 0, 0, 0, 0, 0, 0) and obank.fused_conv1d_mm is False

        # flag on, images kept
        bank = qutil.pack_model(on, fused_linear=True, fused_conv1d=True, fused_conv1d_mm=True)
        (e,) = bank.entries.values()
        assert e["fusable"] and e["kind"] == "conv1d" and e["out"] is not None and torch.equal(e["out"], image)
        assert torch.equal(on(x8), y8_t) and _counters(bank) == (1, 0, 0, 0, 0, 0, 0, 0)          # 8 rows: the row kernel
        b64 = on[0].bias.detach().double().cpu().numpy()
        W = image.double().cpu().numpy()
        calls = 0
        for x in (x9, x64):
            y, xq = _layer_forward(on, x)
            if not half:                                               # fp32: the layer's addmm on the image, no counter
                assert torch.equal(y, want[x.shape[0]]) and _counters(bank) == (1, 0, 0, 0, 0, 0, 0, 0)
                continue
            calls += 1
            assert _counters(bank) == (1, calls, 0, 0, 0, 0, 0, 0) and y.shape == (x.shape[0], N) and y.dtype == dt
            x64_ = xq.double().cpu().numpy()
            y64 = x64_ @ W + b64[None, :]
            S = np.abs(x64_) @ np.abs(W) + np.abs(b64)[None, :]
            ok, worst = _within_bound(y.double().cpu().numpy(), y64, S, K, dtype_name)
            assert ok, (dtype_name, x.shape[0], worst)
            assert torch.equal(y, _direct(antq_lib, bank, e, xq, on[0].bias)), (dtype_name, x.shape[0], "against _lib.linear4_t_mm")
        before = _counters(bank)
        assert torch.equal(on(x65), want[65]) and _counters(bank) == before                       # 65 rows: addmm on the image

        # keep_images=False: a call the kernel serves leaves the scratch alone
        lbank = qutil.pack_model(lean, fused_linear=True, fused_conv1d=True, fused_conv1d_mm=True, keep_images=False)
        (le,) = lbank.entries.values()
        assert le["out"] is None and len(lbank._scratch) == 1
        (scratch,) = lbank._scratch.values()
        scratch.fill_(7.0)
        y9 = lean(x9)
        if half:
            assert bool((scratch == 7.0).all()) and _counters(lbank) == (0, 1, 0, 0, 0, 0, 0, 0)
            assert torch.equal(y9, on(x9))
        else:
            assert torch.equal(y9, want[9]) and _counters(lbank) == (0, 0, 0, 0, 0, 0, 0, 0)
        scratch.fill_(7.0)
        before = _counters(lbank)
        assert torch.equal(lean(x65), want[65]) and _counters(lbank) == before
        assert torch.equal(scratch[:K * N].view(K, N), image)                                      # decoded into the scratch
    capsys.readouterr()


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_packed_conv1d_mm_reload_capture_retype(antq_lib, dev, dtype_name, capsys):
    """A packed checkpoint loaded into a differently seeded model with the flag, a 9-row forward captured into a graph and
    replayed twice, the model retyped."""
    import torch
    dt = getattr(torch, dtype_name)
    half = dtype_name != "float32"
    K, N = 136, 72
    base, qutil = _conv1d_model(dev, dt, K, N)
    gen = torch.Generator(device=dev).manual_seed(3)
    x8, x9, x64 = (torch.randn(r, K, device=dev, generator=gen).to(dt) for r in (8, 9, 64))
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        lean = copy.deepcopy(base)
        opts = dict(fused_linear=True, fused_conv1d=True, fused_conv1d_mm=True, keep_images=False)
        lbank = qutil.pack_model(lean, **opts)
        want = {x.shape[0]: lean(x) for x in (x8, x9, x64)}
        assert _counters(lbank) == (1, 2 if half else 0, 0, 0, 0, 0, 0, 0)

        sd = qutil.packed_state_dict(lean)
        fresh, _ = _conv1d_model(dev, dt, K, N, seed=99)
        assert not torch.equal(fresh[0].bias, lean[0].bias)
        bank2 = qutil.load_packed_state_dict(fresh, sd, **opts)
        (e2,) = bank2.entries.values()
        assert e2["fusable"] and e2["kind"] == "conv1d" and e2["out"] is None and bank2.fused_conv1d_mm is True
        for x in (x8, x9, x64):
            assert torch.equal(fresh(x), want[x.shape[0]]), (dtype_name, x.shape[0])
        assert _counters(bank2) == _counters(lbank)

        # a captured 9-row forward replays to the same bits (one stream, no parallel branches)
        static_x = x9.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        before = _counters(lbank)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        after = _counters(lbank)
        assert after == (before[0], before[1] + (1 if half else 0)) + before[2:]
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, want[9]), (dtype_name, step)
        assert _counters(lbank) == after

        # the model retyped: bf16 -> fp32 routes the 9-row call to addmm and moves no counter; fp32 -> bf16 to the kernel
        other = torch.float32 if half else torch.bfloat16
        fresh.to(other)
        before = _counters(bank2)
        y = fresh(x9.to(other))
        assert y.dtype == other and y.shape == (9, N) and bool(torch.isfinite(y.float()).all())
        assert _counters(bank2) == ((before[0], before[1] + (0 if half else 1)) + before[2:])
        assert e2["out"] is None and e2["dtype"] == other
    capsys.readouterr()


@pytest.mark.parametrize("what", ["K = 132", "byte codes"])
def test_conv1d_layers_the_kernel_does_not_take(antq_lib, dev, what, capsys):
    """A Conv1D layer whose K is no multiple of 8, and a byte-coded one, stay unfusable with the flag on: the image is kept,
    no call is counted, the output is the layer's own addmm on the image."""
    import torch
    dt = torch.bfloat16
    byte = what == "byte codes"
    K, N = (136, 72) if byte else (132, 72)
    base, qutil = _conv1d_model(dev, dt, K, N, eight_bit=byte)
    gen = torch.Generator(device=dev).manual_seed(3)
    xs = [torch.randn(r, K, device=dev, generator=gen).to(dt) for r in (8, 9, 64)]
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        plain, fused = copy.deepcopy(base), copy.deepcopy(base)
        pbank = qutil.pack_model(plain, byte_codes=byte)
        fbank = qutil.pack_model(fused, fused_linear=True, fused_conv1d=True, fused_conv1d_mm=True, keep_images=False, byte_codes=byte,
                                 fused_bytes=byte)
        (fe,) = fbank.entries.values()
        assert not fe["fusable"] and fe["kind"] == "linear" and fe["out"] is not None and len(fbank._scratch) == 0
        for x in xs:
            assert torch.equal(fused(x), plain(x)), (what, x.shape[0])
        assert _counters(fbank) == (0,) * len(COUNTERS)
    capsys.readouterr()
