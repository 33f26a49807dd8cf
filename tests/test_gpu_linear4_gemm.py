"""The packed 4-bit linear as a tiled matrix-core product: antq_linear4_gemm (csrc/antq_k_linear_gemm.h) computes y = x . W^T
(+ bias) for 1 .. 4096 rows of bf16 / f16 x from the code bytes with v_mfma_f32_16x16x32, W being the image antq_decode4 writes.
The yardsticks are those of test_gpu_linear4.py: include/antq.h's decode rule restated in numpy on the code bytes, and float64.
Exact tests compare bits; the general test holds the result to the derived bound of an fp32 sum (test_gpu_linear4_mm.py's:
this kernel makes at most K + 1 additions per output).

The kernel's own boundaries: a workgroup owns BN = 64 output rows and BM = 128 or 256 rows of x (2 or 4 wavefronts of 64 rows
each; the launcher takes 128 while such tiles number at most 256, and antq_debug_set key 23 forces either so that both run at every M of a test -- no
result may depend on it); K is staged in steps of BK = 128 elements; codes are read 16 bytes per lane where K % 32 == 0 and
the codes are 16-byte aligned, 4 bytes per lane otherwise (another k permutation inside a step)."""
import copy

import numpy as np
import pytest

from test_gpu_linear4 import (GUARD, LINEARS, _bits, _book, _books, _check_layers, _gauss_case, _input, _lowest_bit_exponent,
                              _random_codes, _round, _tensor, _tiny, _traced_forward, _trees, _value, _yardstick)
from test_gpu_linear4_mm import _check_layers_mm, _lean_nbytes, _scale_rows, _within_bound

pytestmark = pytest.mark.gpu

DTYPES = ("bfloat16", "float16")
TILES = (2, 4)               # wavefronts (tiles of 64 rows of x) per workgroup: key 23
BMS = (128, 256)             # rows of x per workgroup at those
BN, BK = 64, 128
CALL = 200                   # rows per call of the one-hot tests: crosses row tiles and ends inside one


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def tiles(antq_lib):
    """set(w): force the tile shape of the calling thread's later launches; the rule is restored afterwards"""
    knob = antq_lib.lib().antq_debug_set
    yield lambda w: knob(23, w)
    knob(23, 0)


def _gemm(antq_lib, c, x, N=None, bias=True, out=None):
    N = c["N"] if N is None else N
    return antq_lib.linear4_gemm(c["codes"][:N * c["K"] // 2], x, c["a"], c["gd"], c["gmax"], N, c["K"], True,
                                 bias=c["bias"][:N] if bias else None, n_normal=c["nn"], ovp=c["ovp"], out=out)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
def _one_hot(antq_lib, dev, tiles, dtype_name, scales):
    """x = e_k and -2 e_k in calls of CALL rows: y[m, n] against antq_decode4's element [n, k] and the numpy yardstick.
    K = 520 runs the 4-byte code path, K = 512 the 16-byte one; N = 37 ends inside the one tile of output rows.
    Returns [(case, got bits, got bits of -2 e_k, image bits)]."""
    import torch
    dt = getattr(torch, dtype_name)
    N = 37
    out = []
    for K in (520, 512):
        codes_np = np.concatenate([(np.arange(K // 2) + 37 * n) % 256 for n in range(N)]).astype(np.uint8)
        for n in range(N):
            assert np.unique(codes_np[n * K // 2:(n + 1) * K // 2]).size == 256
        eye = torch.eye(K, device=dev, dtype=dt)
        eye_m2 = eye * -2
        codes = torch.from_numpy(codes_np).to(dev)
        for bi, (name, g, gmax, nn, ovp) in enumerate(_books()):
            plan = antq_lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for si, (per_row, a_np) in enumerate(scales):
                a = torch.from_numpy(a_np).to(dev)
                want = _yardstick(codes_np, a_np, N if per_row else 1, K if per_row else N * K, per_row, g, gmax, nn, ovp, dtype_name).reshape(N, K)
                image = antq_lib.decode4(codes, a, plan, gmax, N if per_row else 1, K if per_row else N * K, per_row, dt, n_normal=nn, ovp=ovp).view(N, K)
                assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode4 against the yardstick")
                y1 = torch.empty(K, N, dtype=dt, device=dev)
                y2 = torch.empty(K, N, dtype=dt, device=dev)
                for ci, k0 in enumerate(range(0, K, CALL)):
                    tiles(TILES[(ci + bi + si) % 2])
                    antq_lib.linear4_gemm(codes, eye[k0:k0 + CALL], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + CALL])
                    tiles(TILES[(ci + bi + si + 1) % 2])
                    antq_lib.linear4_gemm(codes, eye_m2[k0:k0 + CALL], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + CALL])
                torch.cuda.synchronize()
                out.append(((name, dtype_name, K, per_row, float(a_np.min())), _bits(y1.t()), _bits(y2.t()), want))
    return out


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_one_hot_rows_read_the_image(antq_lib, dev, tiles, dtype_name):
    """Ordinary magnitudes, per-row scales and one per tensor, every codebook: bit for bit the image (times -2: exact).  This
    is what catches a wrong lane map, k permutation, LDS swizzle or table stride."""
    scales = ((True, _scale_rows(37, (1.0, 0.06, 0.37, 3.0, 0.011))), (False, np.float32([0.37])))
    for case, y1, y2, want in _one_hot(antq_lib, dev, tiles, dtype_name, scales):
        # (+ 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
        want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
        assert np.array_equal(y1, want), case
        assert np.array_equal(y2, want_m2), case + ("-2 e_k",)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_subnormal_weights(antq_lib, dev, tiles, dtype_name):
    """The same with the scales of test_gpu_linear4_mm.py's test_subnormal_weights: the smallest nonzero weights (all of them,
    for the tiny per-tensor scale) are subnormal in the type, and the 16-bit MFMA keeps subnormal operands."""
    tiny = 1.5e-4 if dtype_name == "float16" else 3.0e-38
    lim = {"bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype_name]
    scales = ((True, _scale_rows(37, (1.0, 0.06, tiny, 20 * tiny, 0.37))), (False, np.float32([tiny])))
    for case, y1, y2, want in _one_hot(antq_lib, dev, tiles, dtype_name, scales):
        mag = np.abs(_value(want, dtype_name))
        assert ((mag > 0) & (mag < lim)).any(), "no subnormal weight in this case"
        want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
        assert np.array_equal(y1, want), case
        assert np.array_equal(y2, want_m2), case + ("-2 e_k",)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_K = tuple(sorted({8, 24, 32, 40, BK - 8, BK, BK + 8, 2 * BK - 8, 2 * BK, 2 * BK + 8, 504, 512, 520, 2056, 4096}))
EXACT_N = (1, 15, 16, 17, BN - 1, BN, BN + 1, 2 * BN + 1)
EXACT_M = tuple(sorted({1, 9, 64, 65} | {m for bm in BMS for m in (bm - 1, bm, bm + 1, 2 * bm + 3)}))


def _exact_case(rng, K, book, dtype_name, per_row, N, rows):
    """test_gpu_linear4_mm.py's construction for `rows` rows of x: codes, power-of-two scales and small-integer x for which
    every product and every partial sum, in any order, is a whole number below 2^24 of units of one power of two -- asserted
    here in float64 -- with the exact result.  The density of x shrinks until that holds."""
    name, g, gmax, nn, ovp = book
    codes = _random_codes(rng, N * K // 2, ovp)
    j = rng.integers(-2, 2, N if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = _value(_yardstick(codes, alpha, N if per_row else 1, K if per_row else N * K, per_row, g, gmax, nn, ovp, dtype_name).reshape(N, K), dtype_name)
    bias = rng.integers(-8, 9, N).astype(np.float64)
    unit = 2.0 ** min(int(_lowest_bit_exponent(W).min()), 0) if (W != 0).any() else 1.0
    assert np.array_equal(W / unit, np.round(W / unit)) and np.abs(W / unit).max() < 2.0 ** 24
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (rows, K)).astype(np.float64) * (rng.random((rows, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        mass = (np.abs(x) @ np.abs(W / unit).T + np.abs(bias)[None, :] / unit)           # exact in float64: whole numbers < 2^53
        if mass.max() < 2.0 ** 24:
            break
        density *= 0.5
    assert np.array_equal(x, np.round(x)) and mass.max() < 2.0 ** 24
    y = (x @ (W / unit).T) * unit                                                        # exact: |partial sums| <= mass
    return codes, alpha, x, bias, y, density


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_sums(antq_lib, dev, tiles, dtype_name):
    """Dyadic codebooks, power-of-two scales, small-integer activations: whatever the order of the sum inside an MFMA and along
    the chain, every partial sum is exact, so the result must be the exact one rounded to the type.  K around the staged step
    on both code paths, N around the tile of output rows, M around both tiles of x, both tile shapes and the rule, bias and
    none, per-row scales and one per tensor, codes 16- and 4-byte aligned."""
    import torch
    rng = np.random.default_rng(5)
    rows = max(EXACT_M)
    for bname in ("pot_b4_s", "olive_int", "olive_flint"):
        book = _book(bname)
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for ki, K in enumerate(EXACT_K):
            per_row = ki % 2 == 0 or ovp
            cases = [(EXACT_N, _exact_case(rng, K, book, dtype_name, True, max(EXACT_N), rows))] if per_row else \
                    [((N,), _exact_case(rng, K, book, dtype_name, False, N, rows)) for N in EXACT_N]
            outs = []
            for ns, (codes_np, a_np, x_np, b_np, y_np, density) in cases:
                x = _tensor(_round(x_np.astype(np.float32), dtype_name), dtype_name, dev)
                bias = _tensor(_round(b_np.astype(np.float32), dtype_name), dtype_name, dev)
                a = torch.from_numpy(a_np).to(dev)
                for N in ns:
                    ni = EXACT_N.index(N)
                    codes = torch.from_numpy(codes_np[:N * K // 2]).to(dev)
                    if (ni + ki) % 4 == 0:              # codes_dev 4-byte but not 16-byte aligned: the 4-byte path at every K
                        buf = torch.empty(codes.numel() + 16, dtype=torch.uint8, device=dev)
                        buf[4:4 + codes.numel()] = codes
                        codes = buf[4:4 + codes.numel()]
                        assert codes.data_ptr() % 16 == 4
                    for mi, M in enumerate(EXACT_M):
                        tiles(((0,) + TILES)[(ni + mi + ki) % 3])
                        for with_bias in ((True, False) if (ni + mi) % 3 == 0 else ((ni + mi) % 2 == 0,)):
                            y = antq_lib.linear4_gemm(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N] if with_bias else None, n_normal=nn, ovp=ovp)
                            outs.append((N, M, with_bias, y, y_np, b_np, density))
            torch.cuda.synchronize()
            assert {o[2] for o in outs} == {True, False} and {o[0] for o in outs} == set(EXACT_N) and {o[1] for o in outs} == set(EXACT_M)
            for N, M, with_bias, y, y_np, b_np, density in outs:
                want = y_np[:M, :N] + (b_np[None, :N] if with_bias else 0.0)
                assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, N, M, with_bias, density)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, dev, dtype_name):
    """_within_bound: (K + 8) 2^-23 S + 2^-p |y64|, derived for at most K + 8 additions; this kernel makes at most K + 1"""
    rng = np.random.default_rng(17)
    for bname in ("flint_b4_s", "int_b4_s", "olive_flint", "olive_int"):
        for K in (768, 4096):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, 33, K, M=300)
            for M in (65, 130, 300):
                y = _gemm(antq_lib, c, c["x"][:M])
                ok, worst = _within_bound(_value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d M=%d: worst error / bound %.3g" % (bname, dtype_name, K, M, worst))
                assert ok, (bname, dtype_name, K, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, dev, tiles, dtype_name):
    import torch
    rng = np.random.default_rng(29)
    rows = 2 * BMS[1] + 44
    for bname in ("flint_b4_s", "olive_flint"):
        for K in (520, 4096):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, 33, K, M=rows)
            run = lambda x, N=33: _bits(_gemm(antq_lib, c, x, N=N))
            tiles(0)
            y_all = run(c["x"])
            assert np.array_equal(y_all, run(c["x"])), (bname, dtype_name, K, "two runs")
            other = torch.randn(rows, K, device=dev, generator=torch.Generator(device=dev).manual_seed(K)).to(c["x"].dtype)
            for w in (0,) + TILES:
                tiles(w)
                assert np.array_equal(run(c["x"]), y_all), (bname, dtype_name, K, w, "tile shape")
                for M in (1, 9, 65, BMS[0], BMS[0] + 1, BMS[1] + 1):
                    assert np.array_equal(run(c["x"][:M]), y_all[:M]), (bname, dtype_name, K, w, M, "a prefix of the rows")
                for m in (0, 63, 64, BMS[0] - 1, BMS[0], BMS[1] - 1, BMS[1], rows - 1):
                    assert np.array_equal(run(c["x"][m:m + 1])[0], y_all[m]), (bname, dtype_name, K, w, m, "a row alone")
                    x2 = other.clone()
                    x2[m] = c["x"][m]
                    assert np.array_equal(run(x2)[m], y_all[m]), (bname, dtype_name, K, w, m, "a row in other company")
                assert np.array_equal(run(c["x"], N=17), y_all[:, :17]), (bname, dtype_name, K, w, "N = 17 against N = 33")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, tiles, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    name, g, gmax, nn, ovp = _book("olive_flint")
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in (8, 504, 520, 4096):
        for N in (1, 17, BN + 1):
            codes_np = _random_codes(rng, N * K // 2, ovp)
            codes = torch.from_numpy(codes_np).to(dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, N)).astype(np.float32)).to(dev)
            for M in sorted({65} | {m for bm in BMS for m in (bm + 1, 2 * bm - 1)}):
                x = torch.randn(M, K, device=dev).to(dt)
                x0, c0 = x.clone(), codes.clone()
                for w in TILES:
                    tiles(w)
                    full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                    y = full[GUARD:GUARD + M * N]
                    antq_lib.linear4_gemm(codes, x, a, gd, gmax, N, K, True, n_normal=nn, ovp=ovp, out=y)
                    checks.append((K, N, M, w, full, x, x0, codes, c0))
    torch.cuda.synchronize()
    for K, N, M, w, full, x, x0, codes, c0 in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, w, "guard words")
        assert torch.equal(x, x0), (dtype_name, K, N, M, w, "x")
        assert torch.equal(codes, c0), (dtype_name, K, N, M, w, "codes")


def test_binding_refuses_float32_and_4097_rows(antq_lib, dev):
    """_lib.linear4_gemm with every tensor on the GPU: float32 and more than LINEAR4_GEMM_MAX_M rows raise before any launch"""
    import torch
    name, g, gmax, nn, ovp = _book("flint_b4_s")
    gd = antq_lib.plan_for(g).grid_dev(dev)
    N, K = 16, 64
    codes = torch.zeros(N * K // 2, dtype=torch.uint8, device=dev)
    a = torch.ones(N, device=dev)
    call = lambda x: antq_lib.linear4_gemm(codes, x, a, gd, gmax, N, K, True)
    assert antq_lib.LINEAR4_GEMM_MAX_M == 4096
    y = call(torch.zeros(4096, K, dtype=torch.bfloat16, device=dev))
    assert y.shape == (4096, N) and bool((y == 0).all())
    with pytest.raises(antq_lib.AntqError, match="float32"):
        call(torch.zeros(9, K, dtype=torch.float32, device=dev))
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(antq_lib.AntqError, match="at most 4096 rows"):
            call(torch.zeros(4097, K, dtype=dt, device=dev))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. module level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_with_fused_gemm_rows(antq_lib, dev, tree, capsys, monkeypatch):
    import torch
    qmod, qutil = _trees(tree)
    dtype_name, dt = "bfloat16", torch.bfloat16
    L = len(LINEARS)
    base = _tiny(tree, dev, dt)
    xs = {r: _input(dev, dt, r, seed=r) for r in (3, 9, 40, 65, 130, 257)}
    decodes = []
    real_decode4 = antq_lib.decode4
    monkeypatch.setattr(antq_lib, "decode4", lambda *a, **kw: (decodes.append(1), real_decode4(*a, **kw))[1])
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, plain, gemm, both, lean = (copy.deepcopy(base) for _ in range(5))
        tbank = qutil.pack_model(twin)                  # no options: the images, and the bits of the calls past R
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        y_twin = {r: twin(x) for r, x in xs.items()}
        pbank = qutil.pack_model(plain, fused_linear=True)             # today's routing: the 3-row bits
        y3_plain = plain(xs[3])
        assert pbank.fused_calls == L and pbank.fused_gemm_calls == 0 and pbank.fused_gemm_rows is None
        assert torch.equal(plain(xs[130]), y_twin[130]) and (pbank.fused_calls, pbank.fused_mm_calls, pbank.fused_gemm_calls) == (L, 0, 0)
        mbank = qutil.pack_model(copy.deepcopy(base), fused_linear=True, fused_rows=64)
        y_mm = {r: mbank.model(xs[r]) for r in (9, 40)}                # antq_linear4_mm's bits
        assert mbank.fused_mm_calls == 2 * L

        gbank = qutil.pack_model(gemm, fused_linear=True, fused_gemm_rows=256)
        bbank = qutil.pack_model(both, fused_linear=True, fused_gemm_rows=256, fused_rows=64)
        lbank = qutil.pack_model(lean, fused_linear=True, keep_images=False, release_weights=True, fused_gemm_rows=256)
        y130 = {}
        for model, bank in ((gemm, gbank), (both, bbank), (lean, lbank)):
            nbytes = bank.nbytes()
            assert nbytes == (_lean_nbytes(tbank, images) if bank is lbank else tbank.nbytes())
            assert bank.fused_gemm_rows == 256
            # 3 rows: antq_linear4, the bits of a bank without the option
            assert torch.equal(model(xs[3]), y3_plain) and (bank.fused_calls, bank.fused_mm_calls, bank.fused_gemm_calls) == (L, 0, 0)
            for t in bank._scratch.values():
                t.fill_(7.0)
            n_dec, n_launch, n_mm, n_gemm = len(decodes), bank.launches, 0, 0
            # 9 and 40 rows: the gemm kernel without fused_rows, antq_linear4_mm (counter and bits) with it
            for r in (9, 40):
                y, seen = _traced_forward(model, xs[r])
                if bank is bbank:
                    n_mm += L
                    assert torch.equal(y, y_mm[r]), (tree, r)
                else:
                    n_gemm += L
                assert (bank.fused_calls, bank.fused_mm_calls, bank.fused_gemm_calls) == (L, n_mm, n_gemm), (tree, r)
                _check_layers_mm(seen, model, images, dtype_name)
            # 65 and 130 rows: the gemm kernel, within the bound layer by layer, nothing decoded, the scratch untouched
            for r in (65, 130):
                y, seen = _traced_forward(model, xs[r])
                n_gemm += L
                assert (bank.fused_calls, bank.fused_mm_calls, bank.fused_gemm_calls) == (L, n_mm, n_gemm), (tree, r)
                _check_layers_mm(seen, model, images, dtype_name)
                _check_layers(seen, model, images, dtype_name)
                assert y.shape == y_twin[r].shape and bool(torch.isfinite(y.float()).all())
                if r == 130:
                    y130[bank] = y
            assert len(decodes) == n_dec and bank.launches == n_launch and bank.nbytes() == nbytes
            assert all(bool((t == 7.0).all()) for t in bank._scratch.values())
            # 257 rows: the fallback, bit-equal to the unfused twin, no counter moves
            assert torch.equal(model(xs[257]), y_twin[257])
            assert (bank.fused_calls, bank.fused_mm_calls, bank.fused_gemm_calls) == (L, n_mm, n_gemm)
        assert torch.equal(y130[gbank], y130[lbank]) and torch.equal(y130[gbank], y130[bbank])   # the same kernel on the same codes
        assert len(decodes) > 0                         # (the lean bank's 257-row call did decode: the counter works)

        # float32: the option is accepted, such layers keep their present path
        f32 = _tiny(tree, dev, torch.float32)
        f32(_input(dev, torch.float32, 4))
        f32_twin = copy.deepcopy(f32)
        qutil.pack_model(f32_twin)
        b32 = qutil.pack_model(f32, fused_linear=True, fused_gemm_rows=256)
        x130f = _input(dev, torch.float32, 130, seed=130)
        assert torch.equal(f32(x130f), f32_twin(x130f)) and (b32.fused_calls, b32.fused_mm_calls, b32.fused_gemm_calls) == (0, 0, 0)

        # the checkpoint into a fresh model with the same options: the same 130-row bits
        sd = qutil.packed_state_dict(lean)
        fresh = _tiny(tree, dev, dt, seed=99)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, keep_images=False, fused_gemm_rows=256)
        assert bank2.fused_gemm_rows == 256 and all((e["out"] is None) == (e["name"] in LINEARS) for e in bank2.entries.values())
        assert torch.equal(fresh(xs[130]), y130[lbank]) and bank2.fused_gemm_calls == L

        # a captured 130-row forward replays twice to the eager bits
        static_x = xs[130].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_gemm = lbank.fused_gemm_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_gemm_calls == n_gemm + L
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, y130[lbank]), (tree, step)
    # a forward that wants gradients: there is no float weight to train
    for model in (gemm, lean):
        with pytest.raises(antq_lib.AntqError):
            model(xs[130])
    capsys.readouterr()
