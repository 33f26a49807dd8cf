"""The tiled matrix-core packed 4-bit linear for [K, N] weights (GPT-2's Conv1D) on the GPU: antq_linear4_t_gemm
(csrc/antq_k_linear_t_gemm.h) computes y = x . W (+ bias) for 1 .. 4096 rows of x, W being the image antq_decode4 writes for K
rows of N codes.  The yardstick and the inputs are antq_linear4_t_mm's (tests/linear_t_cases.py, tests/linear_t_mm_cases.py).

Shapes, at the kernel's switch points: stages of 128 k made of four steps of 32 (K = 8 a partial step; 40 a step and a partial
one; 128 one stage; 136 a stage and a partial step; 264 two stages and one), tiles of 64 columns (N = 8, 72, 136), a wavefront's
64 rows and tiles of 128 / 256 rows (M = 1, 63, 64, 65, 129, 257), each with both tile heights forced (antq_debug_set key 23)."""
import copy

import numpy as np
import pytest

import linear_t_cases as lt
import linear_t_mm_cases as mc
from linear_t_mm_cases import DTYPES
from test_gpu_linear4_t import _bits, _tensor, _within_bound, _conv1d_model, _layer_forward

pytestmark = pytest.mark.gpu

_round, _value = lt.round_bits, lt.value
GRID_K, GRID_N, GRID_M = (8, 40, 128, 136, 264), (8, 72, 136), (1, 63, 64, 65, 129, 257)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def tiles(antq_lib):
    """set(w): force the tile height of the calling thread's later launches; the launcher's rule is restored afterwards"""
    knob = antq_lib.lib().antq_debug_set
    yield lambda w: knob(23, w)
    knob(23, 0)


def _call(antq_lib, dev, c, x, bias=True):
    """antq_linear4_t_gemm on a case dict (codes / alpha / bias as numpy, x a tensor)"""
    import torch
    name, g, gmax, nn, ovp = c["book"]
    codes = torch.from_numpy(np.ascontiguousarray(c["codes"]).reshape(-1)).to(dev)
    b = _tensor(c["bias"], c["dtype_name"], dev) if bias else None
    return antq_lib.linear4_t_gemm(codes, x, torch.from_numpy(c["alpha"]).to(dev), antq_lib.plan_for(g).grid_dev(dev), gmax, c["N"], c["K"],
                                   c["per_row"], bias=b, n_normal=nn, ovp=ovp)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_sums(antq_lib, dev, tiles, dtype_name):
    """Dyadic books, power-of-two scales (per k and per tensor), small-integer x: every partial sum is exact in any order, so y
    is the exact float64 result plus bias rounded once to the type, bit for bit, over the K x N x M grid with both tile heights."""
    import torch
    rng = np.random.default_rng(5)
    NW, rows = max(GRID_N), max(GRID_M)
    for bi, bname in enumerate(("pot_b4_s", "olive_flint")):
        book = lt.book(bname)
        name, g, gmax, nn, ovp = book
        gd = antq_lib.plan_for(g).grid_dev(dev)
        for ki, K in enumerate(GRID_K):
            per_row = (ki + bi) % 2 == 0
            codes_np, a_np, x_np, b_np, y_np, density = mc.exact_case(rng, K, book, dtype_name, per_row, NW, rows=rows)
            x = _tensor(_round(x_np.astype(np.float32), dtype_name), dtype_name, dev)
            bias = _tensor(_round(b_np.astype(np.float32), dtype_name), dtype_name, dev)
            a = torch.from_numpy(a_np).to(dev)
            outs = []
            for ni, N in enumerate(GRID_N):
                codes = torch.from_numpy(np.ascontiguousarray(codes_np.reshape(K, NW // 2)[:, :N // 2])).to(dev)
                for mi, M in enumerate(GRID_M):
                    for waves in (2, 4):
                        tiles(waves)
                        with_bias = (ni + mi + waves // 4) % 2 == 0
                        y = antq_lib.linear4_t_gemm(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N].clone() if with_bias else None,
                                                    n_normal=nn, ovp=ovp)
                        outs.append((N, M, waves, with_bias, y))
            torch.cuda.synchronize()
            for N, M, waves, with_bias, y in outs:
                want = y_np[:M, :N] + (b_np[None, :N] if with_bias else 0.0)
                assert y.shape == (M, N)
                assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, N, M, waves, with_bias, per_row, density)


_GAUSS = {}


def _gauss(dtype_name, K, N, bname, rows):
    """a shared Gaussian case: built once, left unchanged"""
    key = (dtype_name, K, N, bname, rows)
    if key not in _GAUSS:
        _GAUSS[key] = mc.gauss_case(dtype_name, K, N, bname, rows=rows)
    return _GAUSS[key]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, dev, dtype_name):
    """|y - y64| <= K 2^-23 S + 2^-p |y64| against the float64 product with the yardstick's image (the project's derived bound
    of an fp32 sum, test_gpu_linear4_t._within_bound); the pair rule's cases carry planted outliers."""
    for bname in ("flint_b4_s", "olive_flint"):
        for K, N in ((768, 136), (3072, 72)):
            c = _gauss(dtype_name, K, N, bname, 300)
            if c["book"][4]:
                assert mc.has_pair_identifier(c["codes"])
            x = _tensor(c["x"], dtype_name, dev)
            for M in (65, 300):
                y = _call(antq_lib, dev, c, x[:M])
                ok, worst = _within_bound(_value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d N=%d M=%d: worst error / bound %.3g" % (bname, dtype_name, K, N, M, worst))
                assert ok, (bname, dtype_name, K, N, M, worst)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_bits_depend_on_the_row_the_column_and_k_only(antq_lib, dev, tiles, dtype_name):
    """K = 264.  Two runs are equal; both tile heights give the same bits; a row computed alone -- one of each wavefront's block
    and one of the second tile -- has the bits it has in the call of 257; a column of a layer of N = 8 those it has inside N = 136."""
    for bname in ("flint_b4_s", "olive_flint"):
        c = _gauss(dtype_name, 264, 136, bname, 257)
        x = _tensor(c["x"], dtype_name, dev)
        run = lambda case, xs: _bits(_call(antq_lib, dev, case, xs))
        tiles(4)
        y4 = run(c, x)
        assert np.array_equal(y4, run(c, x)), (bname, dtype_name, "two runs")
        for m in (0, 70, 130, 255, 256):
            assert np.array_equal(run(c, x[m:m + 1])[0], y4[m]), (bname, dtype_name, m, "a row alone")
        assert np.array_equal(run(lt.columns(c, 8), x), y4[:, :8]), (bname, dtype_name, "N = 8 against N = 136")
        tiles(2)
        assert np.array_equal(run(c, x), y4), (bname, dtype_name, "128 rows against 256 rows per tile")
        assert np.array_equal(run(c, x[130:131])[0], y4[130]), (bname, dtype_name, "a row alone, tiles of 128 rows")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_padding_and_non_finite_values(antq_lib, dev, dtype_name):
    """K = 136 ends in a stage with one k group inside K and fifteen past it, and the last row of the codes has the Inf scale;
    M = 65 leaves 63 padded rows in the second wavefront, N = 72 padded columns.  The padding adds +0, never a zero x against a
    weight (0 * Inf would be NaN): finite rows and columns are as the float64 product says, a NaN in x reaches its own row only."""
    import torch
    rng = np.random.default_rng(41)
    K, N, M = 136, 72, 65
    book = lt.book("flint_b4_s")
    name, g, gmax, nn, ovp = book
    codes_np = lt.random_codes(rng, K * N // 2, ovp).reshape(K, N // 2)
    pos, n0 = int(np.argmax(g)), 10
    codes_np[K - 1, n0 // 2] = (codes_np[K - 1, n0 // 2] & 0xF0) | pos
    a_np = np.exp(rng.uniform(-3, 0, K)).astype(np.float32)
    a_np[K - 1] = np.inf
    xb = _round(rng.integers(-3, 4, (M, K)).astype(np.float32), dtype_name)
    xb[:, K - 1] = _round(np.float32([1.0]), dtype_name)[0]
    case = dict(book=book, codes=codes_np, alpha=a_np, N=N, K=K, per_row=True, dtype_name=dtype_name)
    run = lambda x: _value(_bits(_call(antq_lib, dev, case, _tensor(x, dtype_name, dev), bias=False)), dtype_name)
    W = _value(lt.image_bits(codes_np.reshape(-1), a_np, K, N, True, book, dtype_name), dtype_name)
    assert W[K - 1, n0] == np.inf and np.isfinite(W[:K - 1]).all()
    with np.errstate(all="ignore"):
        want = _value(xb, dtype_name) @ W
    y = run(xb)
    assert (y[:, n0] == np.inf).all(), (dtype_name, y[:, n0])
    assert np.array_equal(np.isnan(y), np.isnan(want)) and np.array_equal(np.isinf(y), np.isinf(want))
    assert np.array_equal(y[np.isinf(want)], want[np.isinf(want)])
    x = xb.copy()
    x[64, 5] = _round(np.float32([np.nan]), dtype_name)[0]         # the one real row of the second wavefront
    z = run(x)
    assert np.isnan(z[64]).all() and np.array_equal(z[:64], y[:64], equal_nan=True) and not np.isnan(y[64]).all()


def _t_gemm_calls(bank):
    return bank.fused_t_gemm_calls


def test_packed_conv1d_model_with_the_flag(antq_lib, dev, capsys):
    """Two Conv1D layers, K = 264, a call of 200 rows: with the flag both layers run antq_linear4_t_gemm from the codes -- no
    decode launch, the scratch untouched, the output that of the direct call -- and without it the counter stays 0."""
    import torch
    import torch.nn as nn
    dt = torch.bfloat16
    K, N = 264, 72
    first, qutil = _conv1d_model(dev, dt, K, K)
    second, _ = _conv1d_model(dev, dt, K, N, seed=2)
    base = nn.Sequential(first[0], second[0])
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(200, K, device=dev, generator=gen).to(dt)
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        off, on = copy.deepcopy(base), copy.deepcopy(base)
        obank = qutil.pack_model(off, fused_linear=True, fused_conv1d=True, keep_images=False)
        off(x)
        assert _t_gemm_calls(obank) == 0 and obank.fused_conv1d_gemm is False
        bank = qutil.pack_model(on, fused_linear=True, fused_conv1d=True, fused_conv1d_gemm=True, keep_images=False)
        assert all(e["fusable"] and e["kind"] == "conv1d" and e["out"] is None for e in bank.entries.values())
        (scratch,) = bank._scratch.values()
        scratch.fill_(7.0)
        launches = bank.launches
        y = on(x)
        assert _t_gemm_calls(bank) == 2 and bank.launches == launches and bool((scratch == 7.0).all())
        assert y.shape == (200, N) and y.dtype == dt
        # the second layer against the direct call on its own codes and quantised input
        from ant_quantization_amd.packed import _codebook
        y2, xq = _layer_forward(on[1:], on[:1](x))
        e = bank.entries[id(on[1].quant_weight)]
        plan, gmax, n_normal, ovp = _codebook(e["q"])
        direct = antq_lib.linear4_t_gemm(e["codes"], xq, e["alpha"], plan.grid_dev(e["device"]), gmax, N, K, e["per_row"],
                                         bias=on[1].bias.detach(), n_normal=n_normal, ovp=ovp)
        assert torch.equal(y2, y) and torch.equal(y2, direct) and _t_gemm_calls(bank) == 4
    capsys.readouterr()
