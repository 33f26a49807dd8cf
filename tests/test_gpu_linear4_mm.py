"""The packed 4-bit linear on the matrix cores: antq_linear4_mm (csrc/antq_k_linear_mm.h with Lin4Codec) computes y = x . W^T (+ bias) for
1 .. 64 rows of bf16 / f16 x from the code bytes with v_mfma_f32_16x16x32, W being the image antq_decode4 writes.  The
yardsticks are those of test_gpu_linear4.py: include/antq.h's decode rule restated in numpy on the code bytes, and float64.
Exact tests compare bits; the general test holds the result to the derived bound of an fp32 sum.

The kernel's own boundaries: a workgroup owns 16 / 32 / 64 output rows (the launcher's choice, forced here through
antq_debug_set key 22 so that every tile shape runs at the small N of a test -- no result may depend on it); K is cut into
chunks of 128 elements (codes read 16 bytes per lane: K % 32 == 0 and aligned codes) or of 32 (4 bytes per lane) dealt to
eight wavefronts in turn, so w = 1 .. 8 wavefronts have work up to K = 128 w and 32 w."""
import copy

import numpy as np
import pytest

from test_gpu_linear4 import (GUARD, LINEARS, PREC, _bits, _book, _books, _check_layers, _gauss_case, _input, _lowest_bit_exponent,
                              _random_codes, _round, _tensor, _tiny, _traced_forward, _trees, _value, _yardstick)

pytestmark = pytest.mark.gpu

DTYPES = ("bfloat16", "float16")
TILES = (1, 2, 4)            # tiles of 16 output rows per workgroup


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def tiles(antq_lib):
    """set(nt): force the tile shape of the calling thread's later launches; the rule is restored afterwards"""
    knob = antq_lib.lib().antq_debug_set
    yield lambda nt: knob(22, nt)
    knob(22, 0)


def _mm(antq_lib, c, x, N=None, bias=True, out=None):
    N = c["N"] if N is None else N
    return antq_lib.linear4_mm(c["codes"][:N * c["K"] // 2], x, c["a"], c["gd"], c["gmax"], N, c["K"], True,
                               bias=c["bias"][:N] if bias else None, n_normal=c["nn"], ovp=c["ovp"], out=out)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. / 2. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
def _one_hot(antq_lib, dev, tiles, dtype_name, scales):
    """x = e_k and -2 e_k in calls of up to 64 rows: y[m, n] against antq_decode4's element [n, k] and the numpy yardstick.
    K = 520 runs the 4-byte code path, K = 512 the 16-byte one (another k permutation inside the MFMA steps); N = 37 is two
    workgroups and a tail at every tile shape but the largest.  Returns [(case, got bits, got bits of -2 e_k, image bits)]."""
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
                for ci, k0 in enumerate(range(0, K, 64)):
                    tiles(TILES[(ci + bi + si) % 3])
                    antq_lib.linear4_mm(codes, eye[k0:k0 + 64], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + 64])
                    antq_lib.linear4_mm(codes, eye_m2[k0:k0 + 64], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + 64])
                torch.cuda.synchronize()
                out.append(((name, dtype_name, K, per_row, float(a_np.min())), _bits(y1.t()), _bits(y2.t()), want))
    return out


def _scale_rows(N, values):
    """N per-row scales cycling through `values`"""
    return np.float32([values[n % len(values)] for n in range(N)])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_one_hot_rows_read_the_image(antq_lib, dev, tiles, dtype_name):
    """Ordinary magnitudes, per-row scales and one per tensor, every codebook: bit for bit the image (times -2: exact).  This
    is what catches a wrong lane map, k permutation or table stride."""
    scales = ((True, _scale_rows(37, (1.0, 0.06, 0.37, 3.0, 0.011))), (False, np.float32([0.37])))
    for case, y1, y2, want in _one_hot(antq_lib, dev, tiles, dtype_name, scales):
        # (+ 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
        want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
        assert np.array_equal(y1, want), case
        assert np.array_equal(y2, want_m2), case + ("-2 e_k",)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_subnormal_weights(antq_lib, dev, tiles, dtype_name):
    """The same with scales so small that the smallest nonzero weights (all of them, for the tiny per-tensor scale) are
    subnormal in the type.  Measured on an MI355X: v_mfma_f32_16x16x32_bf16 / _f16 keep subnormal operands (every one of the
    840 .. 12019 subnormal weights per case came back bit for bit, from e_k and from -2 e_k), so this is an equality test."""
    tiny = 1.5e-4 if dtype_name == "float16" else 3.0e-38
    lim = {"bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype_name]
    scales = ((True, _scale_rows(37, (1.0, 0.06, tiny, 20 * tiny, 0.37))), (False, np.float32([tiny])))
    for case, y1, y2, want in _one_hot(antq_lib, dev, tiles, dtype_name, scales):
        mag = np.abs(_value(want, dtype_name))
        assert ((mag > 0) & (mag < lim)).any(), "no subnormal weight in this case"
        want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
        print("%s: %d subnormal weights, %d of them kept by e_k, %d by -2 e_k" % (
            case, ((mag > 0) & (mag < lim)).sum(), (y1 == want)[(mag > 0) & (mag < lim)].sum(), (y2 == want_m2)[(mag > 0) & (mag < lim)].sum()))
        assert np.array_equal(y1, want), case
        assert np.array_equal(y2, want_m2), case + ("-2 e_k",)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
# the issue's list; the boundaries of the 4-byte path's split (32 w, w = 1 .. 8: the last K at which w wavefronts have work)
# with the multiples of 8 either side; those of the 16-byte path's (128 w) with the multiples of 8 either side (which run the
# 4-byte path) and the multiples of 32 either side (which stay on the 16-byte path)
EXACT_K = tuple(sorted({8, 24, 32, 40, 120, 128, 136, 504, 512, 520, 2056, 4096}
                       | {32 * w + d for w in range(1, 9) for d in (-8, 0, 8)}
                       | {128 * w + d for w in range(1, 9) for d in (-32, -8, 0, 8, 32)}))
EXACT_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)       # the issue's, and tile - 1, tile, tile + 1 for 16 / 32 / 64 rows
EXACT_M = (1, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)


def _exact_case(rng, K, book, dtype_name, per_row, N):
    """Codes, power-of-two scales and small-integer x (64 rows) for which every product and every partial sum, in any order,
    is a whole number below 2^24 of units of one power of two -- asserted here in float64 -- with the exact result."""
    name, g, gmax, nn, ovp = book
    codes = _random_codes(rng, N * K // 2, ovp)
    j = rng.integers(-2, 2, N if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    W = _value(_yardstick(codes, alpha, N if per_row else 1, K if per_row else N * K, per_row, g, gmax, nn, ovp, dtype_name).reshape(N, K), dtype_name)
    bias = rng.integers(-8, 9, N).astype(np.float64)
    # every weight a whole multiple of `unit` (a power of two <= 1), x and the bias whole numbers: every term is a whole
    # multiple of the unit, and so is every partial sum
    unit = 2.0 ** min(int(_lowest_bit_exponent(W).min()), 0) if (W != 0).any() else 1.0
    assert np.array_equal(W / unit, np.round(W / unit)) and np.abs(W / unit).max() < 2.0 ** 24
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (64, K)).astype(np.float64) * (rng.random((64, K)) < density)
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
    """Dyadic codebooks, power-of-two scales, small-integer activations: whatever the order of the sum -- inside an MFMA
    step, along a wavefront's chain, across the eight wavefronts -- every partial sum is exact, so the result must be the exact
    one rounded to the type.  Every K around the split's boundaries on both code paths, N around every tile shape, M around
    every tile of x, every tile shape, bias and none, per-row scales and one per tensor, codes 16- and 4-byte aligned."""
    import torch
    rng = np.random.default_rng(5)
    for bname in ("pot_b4_s", "olive_int", "olive_flint"):
        book = _book(bname)
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for ki, K in enumerate(EXACT_K):
            per_row = ki % 2 == 0 or ovp
            # (per-row scales: the codes of a prefix of rows are that smaller layer's codes; one scale per tensor: every N gets
            # codes of its own)
            cases = [(EXACT_N, _exact_case(rng, K, book, dtype_name, True, max(EXACT_N)))] if per_row else \
                    [((N,), _exact_case(rng, K, book, dtype_name, False, N)) for N in EXACT_N]
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
                        tiles(TILES[(ni + mi + ki) % 3])
                        for with_bias in ((True, False) if (ni + mi) % 3 == 0 else ((ni + mi) % 2 == 0,)):
                            y = antq_lib.linear4_mm(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N] if with_bias else None, n_normal=nn, ovp=ovp)
                            outs.append((N, M, with_bias, y, y_np, b_np, density))
            torch.cuda.synchronize()
            assert {o[2] for o in outs} == {True, False} and {o[0] for o in outs} == set(EXACT_N) and {o[1] for o in outs} == set(EXACT_M)
            for N, M, with_bias, y, y_np, b_np, density in outs:
                want = y_np[:M, :N] + (b_np[None, :N] if with_bias else 0.0)
                assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, N, M, with_bias, density)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
def _within_bound(y, y64, S, K, dtype_name):
    """|y - y64| <= (K + 8) 2^-23 S + 2^-p |y64|.  Derived, not measured: products of two bf16 or two f16 values are exact in
    fp32; there are at most K + 8 additions, counting the combination of the split and the bias, each allowed one full ulp of
    the running magnitude (<= S), so an internal adder that truncates is covered; then the rounding to the output type."""
    err = np.abs(y - y64)
    bound = (K + 8) * 2.0 ** -23 * S + 2.0 ** -PREC[dtype_name] * np.abs(y64)
    return bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, dev, dtype_name):
    rng = np.random.default_rng(17)
    for bname in ("flint_b4_s", "int_b4_s", "olive_flint", "olive_int"):
        for K in (768, 4096):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, 33, K, M=64)
            for M in (9, 16, 40, 64):
                y = _mm(antq_lib, c, c["x"][:M])
                ok, worst = _within_bound(_value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d M=%d: worst error / bound %.3g" % (bname, dtype_name, K, M, worst))
                assert ok, (bname, dtype_name, K, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, dev, tiles, dtype_name):
    import torch
    rng = np.random.default_rng(29)
    for bname in ("flint_b4_s", "olive_flint"):
        for K in (520, 4096):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, 33, K, M=64)
            run = lambda x, N=33: _bits(_mm(antq_lib, c, x, N=N))
            tiles(0)
            y64 = run(c["x"])
            assert np.array_equal(y64, run(c["x"])), (bname, dtype_name, K, "two runs")
            other = torch.randn(64, K, device=dev, generator=torch.Generator(device=dev).manual_seed(K)).to(c["x"].dtype)
            for nt in (0,) + TILES:
                tiles(nt)
                assert np.array_equal(run(c["x"]), y64), (bname, dtype_name, K, nt, "tile shape")
                for M in (1, 9, 16, 17, 33, 63):
                    assert np.array_equal(run(c["x"][:M]), y64[:M]), (bname, dtype_name, K, nt, M, "a prefix of the rows")
                for m in (0, 7, 16, 37, 63):
                    assert np.array_equal(run(c["x"][m:m + 1])[0], y64[m]), (bname, dtype_name, K, nt, m, "a row alone")
                    x2 = other.clone()
                    x2[m] = c["x"][m]
                    assert np.array_equal(run(x2)[m], y64[m]), (bname, dtype_name, K, nt, m, "a row in other company")
                assert np.array_equal(run(c["x"], N=17), y64[:, :17]), (bname, dtype_name, K, nt, "N = 17 against N = 33")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. footprint
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
        for N in (1, 15, 17, 33, 65):
            codes_np = _random_codes(rng, N * K // 2, ovp)
            codes = torch.from_numpy(codes_np).to(dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, N)).astype(np.float32)).to(dev)
            for M in (9, 17, 33, 63):
                x = torch.randn(M, K, device=dev).to(dt)
                x0, c0 = x.clone(), codes.clone()
                for nt in TILES:
                    tiles(nt)
                    full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                    y = full[GUARD:GUARD + M * N]
                    antq_lib.linear4_mm(codes, x, a, gd, gmax, N, K, True, n_normal=nn, ovp=ovp, out=y)
                    checks.append((K, N, M, nt, full, x, x0, codes, c0))
    torch.cuda.synchronize()
    for K, N, M, nt, full, x, x0, codes, c0 in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, nt, "guard words")
        assert torch.equal(x, x0), (dtype_name, K, N, M, nt, "x")
        assert torch.equal(codes, c0), (dtype_name, K, N, M, nt, "codes")


def test_binding_refuses_float32_and_65_rows(antq_lib, dev):
    """_lib.linear4_mm with every tensor on the GPU: float32 and more than LINEAR4_MM_MAX_M rows raise before any launch"""
    import torch
    name, g, gmax, nn, ovp = _book("flint_b4_s")
    gd = antq_lib.plan_for(g).grid_dev(dev)
    N, K = 16, 64
    codes = torch.zeros(N * K // 2, dtype=torch.uint8, device=dev)
    a = torch.ones(N, device=dev)
    call = lambda x: antq_lib.linear4_mm(codes, x, a, gd, gmax, N, K, True)
    assert call(torch.zeros(64, K, dtype=torch.bfloat16, device=dev)).shape == (64, N)
    with pytest.raises(antq_lib.AntqError, match="float32"):
        call(torch.zeros(9, K, dtype=torch.float32, device=dev))
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(antq_lib.AntqError, match="at most 64 rows"):
            call(torch.zeros(65, K, dtype=dt, device=dev))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. module level
# ---------------------------------------------------------------------------------------------------------------------------
def _check_layers_mm(seen, model, images, dtype_name):
    """the bound above, layer by layer: every Linear's output against float64 on its own quantised input and the twin's image"""
    for n in LINEARS:
        xq, y = seen[n]
        W = images[n].double().cpu().numpy()
        x64 = xq.double().cpu().numpy().reshape(-1, W.shape[1])
        b64 = model.get_submodule(n).bias.detach().double().cpu().numpy()
        y64 = x64 @ W.T + b64[None, :]
        S = np.abs(x64) @ np.abs(W).T + np.abs(b64)[None, :]
        ok, worst = _within_bound(y.double().cpu().numpy().reshape(y64.shape), y64, S, W.shape[1], dtype_name)
        assert ok, (n, dtype_name, worst)


def _lean_nbytes(tbank, images):
    """codes as the twin's; images: the twin's without the Linear layers' plus one scratch of the largest of them"""
    lin = [images[n].numel() * images[n].element_size() for n in LINEARS]
    return (tbank.nbytes()[0], tbank.nbytes()[1] - sum(lin) + max(lin))


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_with_fused_rows(antq_lib, dev, tree, capsys, monkeypatch):
    import torch
    qmod, qutil = _trees(tree)
    dtype_name, dt = "bfloat16", torch.bfloat16
    base = _tiny(tree, dev, dt)
    xs = {r: _input(dev, dt, r, seed=r) for r in (3, 9, 24, 40, 65)}
    decodes = []
    real_decode4 = antq_lib.decode4
    monkeypatch.setattr(antq_lib, "decode4", lambda *a, **kw: (decodes.append(1), real_decode4(*a, **kw))[1])
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, plain, fused, lean = (copy.deepcopy(base) for _ in range(4))
        tbank = qutil.pack_model(twin)
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        y_twin = {r: twin(x) for r, x in xs.items()}
        pbank = qutil.pack_model(plain, fused_linear=True)             # no fused_rows: today's routing
        y3_plain = plain(xs[3])
        assert pbank.fused_calls == len(LINEARS) and pbank.fused_mm_calls == 0 and pbank.fused_rows is None
        assert torch.equal(plain(xs[9]), y_twin[9]) and pbank.fused_calls == len(LINEARS) and pbank.fused_mm_calls == 0

        fbank = qutil.pack_model(fused, fused_linear=True, fused_rows=64)
        lbank = qutil.pack_model(lean, fused_linear=True, keep_images=False, release_weights=True, fused_rows=64)
        y9 = {}
        for model, bank in ((fused, fbank), (lean, lbank)):
            nbytes = bank.nbytes()
            assert nbytes == (tbank.nbytes() if bank is fbank else _lean_nbytes(tbank, images))
            # 3 rows: antq_linear4, the bits of a bank without fused_rows
            assert torch.equal(model(xs[3]), y3_plain) and (bank.fused_calls, bank.fused_mm_calls) == (len(LINEARS), 0)
            # 9 and 40 rows: antq_linear4_mm, within the bound layer by layer, nothing decoded, the scratch untouched
            for t in bank._scratch.values():
                t.fill_(7.0)
            n_dec, n_launch, n_mm = len(decodes), bank.launches, 0
            for r in (9, 40):
                y, seen = _traced_forward(model, xs[r])
                n_mm += len(LINEARS)
                assert (bank.fused_calls, bank.fused_mm_calls) == (len(LINEARS), n_mm), (tree, r)
                _check_layers_mm(seen, model, images, dtype_name)
                _check_layers(seen, model, images, dtype_name)
                assert y.shape == y_twin[r].shape and bool(torch.isfinite(y.float()).all())
                if r == 9:
                    y9[bank] = y
            assert len(decodes) == n_dec and bank.launches == n_launch and bank.nbytes() == nbytes
            assert all(bool((t == 7.0).all()) for t in bank._scratch.values())
            # 65 rows: the fallback, bit-equal to the unfused twin, neither counter moves
            assert torch.equal(model(xs[65]), y_twin[65]) and (bank.fused_calls, bank.fused_mm_calls) == (len(LINEARS), n_mm)
        assert torch.equal(y9[fbank], y9[lbank])       # the same kernel on the same codes
        assert len(decodes) > 0                         # (the lean bank's 65-row call did decode: the counter works)

        # float32: fused_rows is accepted, such layers keep their present path
        f32 = _tiny(tree, dev, torch.float32)
        f32(_input(dev, torch.float32, 4))
        f32_twin = copy.deepcopy(f32)
        qutil.pack_model(f32_twin)
        b32 = qutil.pack_model(f32, fused_linear=True, fused_rows=64)
        x9f = _input(dev, torch.float32, 9, seed=9)
        assert torch.equal(f32(x9f), f32_twin(x9f)) and b32.fused_mm_calls == 0 and b32.fused_calls == 0

        # the checkpoint into a fresh model with the same options: the same 9-row bits
        sd = qutil.packed_state_dict(lean)
        fresh = _tiny(tree, dev, dt, seed=99)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, keep_images=False, fused_rows=64)
        assert bank2.fused_rows == 64 and all((e["out"] is None) == (e["name"] in LINEARS) for e in bank2.entries.values())
        assert torch.equal(fresh(xs[9]), y9[lbank]) and bank2.fused_mm_calls == len(LINEARS)

        # a captured 24-row forward replays twice to the eager bits
        y24 = lean(xs[24])
        static_x = xs[24].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_mm = lbank.fused_mm_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_mm_calls == n_mm + len(LINEARS)
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, y24), (tree, step)
    # a forward that wants gradients: there is no float weight to train
    for model in (fused, lean):
        with pytest.raises(antq_lib.AntqError):
            model(xs[9])
    capsys.readouterr()
