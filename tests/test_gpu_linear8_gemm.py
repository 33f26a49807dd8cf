"""The byte-code linear as a tiled matrix-core product: antq_linear8_gemm (csrc/antq_k_linear_gemm.h with Lin8Codec) computes
y = x . W^T (+ bias) for 1 .. 4096 rows of bf16 / f16 x from the code bytes with v_mfma_f32_16x16x32, W being the image
antq_decode8 writes.  The yardstick is byte_codes_cases.decode_ref (include/antq.h restated in numpy) and float64.  Exact tests
compare bits; the general test holds the result to the derived bound of an fp32 sum (test_gpu_linear4_mm._within_bound: for at
most K + 8 additions; this kernel makes at most K + 1).  The inputs come from linear8_gemm_cases.py, which
test_linear8_gemm_cases_host.py holds to their premises without a GPU.

The kernel's own boundaries: a workgroup owns BN = 64 output rows and BM = 128 or 256 rows of x (2 or 4 wavefronts; the launcher
takes 128 while such tiles number at most 256, and antq_debug_set key 23 forces either so that both run at every M of a test --
no result may depend on it); K is staged in steps of BK = 128 elements; a lane reads its codes as two 16-byte loads per step
where K % 16 == 0 and the codes are 16-byte aligned, as four 8-byte loads otherwise (another k permutation inside a step).

Without the feature every test here fails: _lib has no linear8_gemm and pack_model no fused_byte_gemm_rows."""
import copy

import numpy as np
import pytest

import byte_codes_cases as bc
import encode4_cases as ec
import linear8_cases as lc
import linear8_gemm_cases as gc
from test_gpu_linear4_mm import _within_bound
from test_gpu_linear8 import GUARD, LINEARS, _bits, _codes, _input, _round, _tensor, _tiny, _traced_forward, _trees
from test_gpu_linear8_mm import _check_layers_mm

pytestmark = pytest.mark.gpu

TILES, BMS, BN = gc.TILES, gc.BMS, gc.BN


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


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", gc.DTYPES)
@pytest.mark.parametrize("K", gc.ONE_HOT_K)
def test_one_hot_rows_read_the_image(antq_lib, oracle, dev, tiles, K, dtype_name):
    """x = e_k (and -2 e_k) in calls of 200 rows, the forced tile shapes alternating: y[m, n] is bit for bit element [n, k] of
    antq_decode8's image (times -2, exact), which is first held to decode_ref.  Every byte value in every row at every position
    of a lane's bytes, every pair form, codes beyond the book; per-row scales and one per tensor, ordinary and so small that
    weights are subnormal in the type; N = 37 ends inside the tile of output rows.  K = 520: four 8-byte loads; 528: two 16-byte
    loads, the last lane group's second one past the row's end; 512: no tail.  This is what catches a wrong lane map, partner
    byte, load order, LDS swizzle, table stride or k permutation."""
    import torch
    dt = getattr(torch, dtype_name)
    N = gc.ONE_HOT_N
    eye = torch.eye(K, device=dev, dtype=dt)
    eye_m2 = eye * -2
    for bi, name in enumerate(gc.ONE_HOT_BOOKS):
        _, g, gmax, nn, ovp = bc.book(name)
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        codes_np = lc.one_hot_codes(name, K, N=N)
        codes = _codes(codes_np, dev)
        assert codes.data_ptr() % 16 == 0
        for si, (per_row, a5) in enumerate(lc.one_hot_scales(dtype_name)):
            a_np = gc.scale_rows(a5, N) if per_row else a5
            a = torch.from_numpy(a_np).to(dev)
            want = lc.image_ref(oracle, codes_np, a_np, per_row, name, dtype_name)
            image = antq_lib.decode8(codes, a, plan, gmax, N if per_row else 1, K if per_row else N * K, per_row, dt, n_normal=nn, ovp=ovp).view(N, K)
            assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode8 against the yardstick")
            # (exact: a doubling; + 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
            want_m2 = _round(oracle, (lc.value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
            y1 = torch.empty(K, N, dtype=dt, device=dev)
            y2 = torch.empty(K, N, dtype=dt, device=dev)
            for ci, k0 in enumerate(range(0, K, gc.CALL)):
                tiles(TILES[(ci + bi + si) % 2])
                antq_lib.linear8_gemm(codes, eye[k0:k0 + gc.CALL], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + gc.CALL])
                tiles(TILES[(ci + bi + si + 1) % 2])
                antq_lib.linear8_gemm(codes, eye_m2[k0:k0 + gc.CALL], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + gc.CALL])
            torch.cuda.synchronize()
            bad1, bad2 = int((_bits(y1.t()) != want).sum()), int((_bits(y2.t()) != want_m2).sum())
            assert bad1 == 0, (name, dtype_name, K, per_row, float(a_np.min()), "%d elements differ" % bad1)
            assert bad2 == 0, (name, dtype_name, K, per_row, float(a_np.min()), "-2 e_k", "%d elements differ" % bad2)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name,dtype_name", gc.EXACT_CASES)
def test_exact_sums(antq_lib, oracle, dev, tiles, set_name, dtype_name):
    """Dyadic codebooks, power-of-two scales, small-integer activations: whatever the order of the sum inside an MFMA and along
    the chain, every partial sum is exact, so the result must be the exact one rounded to the type.  K around the staged step
    on both code paths, N around the tile of output rows, M around both tiles of x, both forced tile shapes and the rule, bias
    and none, per-row scales and one per tensor, codes on and 8 bytes off a 16-byte boundary."""
    import torch
    failed = []
    for K in gc.EXACT_K:
        name = gc.exact_book(set_name, K)
        _, g, gmax, nn, ovp = bc.book(name)
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        per_row, cases = gc.exact_cases_of(oracle, name, K, dtype_name)
        by_n = {N: c for ns, c in cases for N in ns}
        dev_case = {}
        outs = []
        for ni, mi, off, w, forms in gc.exact_runs(K):
            N, M = gc.EXACT_N[ni], gc.EXACT_M[mi]
            c = by_n[N]
            if id(c) not in dev_case:
                dev_case[id(c)] = (_tensor(_round(oracle, c["x"], dtype_name), dtype_name, dev),
                                   _tensor(_round(oracle, c["bias"], dtype_name), dtype_name, dev), torch.from_numpy(c["alpha"]).to(dev), {})
            x, bias, a, code_cache = dev_case[id(c)]
            if (N, off) not in code_cache:
                code_cache[(N, off)] = _codes(c["codes"][:N], dev, off)
            codes = code_cache[(N, off)]
            assert codes.data_ptr() % 16 == off
            tiles(w)
            for with_bias in forms:
                y = antq_lib.linear8_gemm(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N] if with_bias else None, n_normal=nn, ovp=ovp)
                outs.append((N, M, off, w, with_bias, y, c))
        torch.cuda.synchronize()
        assert {o[4] for o in outs} == {True, False} and {o[0] for o in outs} == set(gc.EXACT_N) and {o[1] for o in outs} == set(gc.EXACT_M)
        assert {o[3] for o in outs} == set(gc.SHAPES) and {o[2] for o in outs} == set(gc.exact_offsets(K))
        for N, M, off, w, with_bias, y, c in outs:
            want = c["y"][:M, :N] + (c["bias"][None, :N] if with_bias else 0.0)
            if not np.array_equal(_bits(y), _round(oracle, want, dtype_name)):
                failed.append((K, N, M, off, w, with_bias, per_row, c["density"]))
    assert not failed, (set_name, dtype_name, "%d launches differ" % len(failed), failed[:8])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
_GAUSS = {}
ROWS = 2 * BMS[1] + 44


def _gauss_case(antq_lib, oracle, dev, name, dtype_name, K, seed=17):
    """Encoded Gaussian weights and ROWS rows of x; decode_ref's weights, the float64 result and the float64 mass
    S = sum |x W| + |bias|.  Built once per argument set and shared (nothing writes to it)."""
    import torch
    key = (name, dtype_name, K, seed)
    if key in _GAUSS:
        return _GAUSS[key]
    _, g, gmax, nn, ovp = bc.book(name)
    N = gc.GENERAL_N
    plan = antq_lib.plan_for(g)
    d = lc.gauss_weights(name, dtype_name, K, N=N, M=ROWS, seed=seed)
    wk, _ = ec.as_dtype(oracle, d["w"], dtype_name)
    wt = _tensor(np.asarray(wk).reshape(N, K), dtype_name, dev)
    a = torch.from_numpy(d["alpha"]).to(dev)
    codes = antq_lib.encode8(wt, a, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
    codes_np = codes.cpu().numpy().reshape(N, K)
    if ovp:
        assert (codes_np == bc.IDENT).any()
    W = lc.value(lc.image_ref(oracle, codes_np, d["alpha"], True, name, dtype_name), dtype_name)
    xb, bb = _round(oracle, d["x"], dtype_name), _round(oracle, d["bias"], dtype_name)
    x64, b64 = lc.value(xb, dtype_name), lc.value(bb, dtype_name)
    y64 = x64 @ W.T + b64[None, :]
    S = np.abs(x64) @ np.abs(W).T + np.abs(b64)[None, :]
    _GAUSS[key] = dict(codes=codes, a=a, gd=plan.grid_dev(dev), x=_tensor(xb, dtype_name, dev), bias=_tensor(bb, dtype_name, dev), y64=y64, S=S,
                       gmax=gmax, nn=nn, ovp=ovp, N=N, K=K)
    return _GAUSS[key]


def _gemm(antq_lib, c, x, N=None, bias=True, out=None):
    N = c["N"] if N is None else N
    return antq_lib.linear8_gemm(c["codes"][:N * c["K"]], x, c["a"], c["gd"], c["gmax"], N, c["K"], True,
                                 bias=c["bias"][:N] if bias else None, n_normal=c["nn"], ovp=c["ovp"], out=out)


@pytest.mark.parametrize("dtype_name", gc.DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, oracle, dev, dtype_name):
    """_within_bound: (K + 8) 2^-23 S + 2^-p |y64|, derived for at most K + 8 additions; this kernel makes at most K + 1"""
    for name in gc.GENERAL_BOOKS:
        for K in gc.GENERAL_K:
            c = _gauss_case(antq_lib, oracle, dev, name, dtype_name, K)
            assert c["x"].shape == (ROWS, K)
            for M in gc.GENERAL_M:
                y = _gemm(antq_lib, c, c["x"][:M])
                ok, worst = _within_bound(lc.value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d M=%d: worst error / bound %.3g" % (name, dtype_name, K, M, worst))
                assert ok, (name, dtype_name, K, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", gc.DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, oracle, dev, tiles, dtype_name):
    import torch
    for name in ("flint_b6_s", "olive_int_b8"):
        for K in (520, 4096):
            c = _gauss_case(antq_lib, oracle, dev, name, dtype_name, K)
            run = lambda x, N=gc.GENERAL_N: _bits(_gemm(antq_lib, c, x, N=N))   # noqa: E731
            tiles(0)
            y_all = run(c["x"])
            assert np.array_equal(y_all, run(c["x"])), (name, dtype_name, K, "two runs")
            other = torch.randn(ROWS, K, device=dev, generator=torch.Generator(device=dev).manual_seed(K)).to(c["x"].dtype)
            for w in (0,) + TILES:
                tiles(w)
                assert np.array_equal(run(c["x"]), y_all), (name, dtype_name, K, w, "tile shape")
                for M in (1, 9, 65, BMS[0], BMS[0] + 1, BMS[1] + 1):
                    assert np.array_equal(run(c["x"][:M]), y_all[:M]), (name, dtype_name, K, w, M, "a prefix of the rows")
                for m in (0, 63, 64, BMS[0] - 1, BMS[0], BMS[1] - 1, BMS[1], ROWS - 1):
                    assert np.array_equal(run(c["x"][m:m + 1])[0], y_all[m]), (name, dtype_name, K, w, m, "a row alone")
                    x2 = other.clone()
                    x2[m] = c["x"][m]
                    assert np.array_equal(run(x2)[m], y_all[m]), (name, dtype_name, K, w, m, "a row in other company")
                assert np.array_equal(run(c["x"], N=17), y_all[:, :17]), (name, dtype_name, K, w, "N = 17 against N = 33")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", gc.DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, tiles, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    _, g, gmax, nn, ovp = bc.book("olive_int_b8")
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in (8, 504, 520, 528, 4096):
        for N in (1, 17, BN + 1):
            codes = _codes(lc.random_codes(rng, N * K, ovp), dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, N)).astype(np.float32)).to(dev)
            for M in sorted({65} | {m for bm in BMS for m in (bm + 1, 2 * bm - 1)}):
                x = torch.randn(M, K, device=dev).to(dt)
                x0, c0 = x.clone(), codes.clone()
                for w in TILES:
                    tiles(w)
                    full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                    y = full[GUARD:GUARD + M * N]
                    antq_lib.linear8_gemm(codes, x, a, gd, gmax, N, K, True, n_normal=nn, ovp=ovp, out=y)
                    checks.append((K, N, M, w, full, x, x0, codes, c0))
    torch.cuda.synchronize()
    for K, N, M, w, full, x, x0, codes, c0 in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, w, "guard words")
        assert not (b[GUARD:GUARD + M * N] == guard).all(), (dtype_name, K, N, M, w, "nothing written")
        assert torch.equal(x, x0), (dtype_name, K, N, M, w, "x")
        assert torch.equal(codes, c0), (dtype_name, K, N, M, w, "codes")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. binding
# ---------------------------------------------------------------------------------------------------------------------------
def test_binding_refuses_float32_and_4097_rows(antq_lib, dev):
    """_lib.linear8_gemm with every tensor on the GPU: float32 and more than LINEAR8_GEMM_MAX_M rows raise before any launch"""
    import torch
    _, g, gmax, nn, ovp = bc.book("int_b8_s")
    gd = antq_lib.plan_for(g).grid_dev(dev)
    N, K = 16, 64
    codes = torch.zeros(N * K, dtype=torch.uint8, device=dev)
    a = torch.ones(N, device=dev)
    call = lambda x: antq_lib.linear8_gemm(codes, x, a, gd, gmax, N, K, True)   # noqa: E731
    assert antq_lib.LINEAR8_GEMM_MAX_M == 4096
    for dt in (torch.bfloat16, torch.float16):
        assert call(torch.zeros(4096, K, dtype=dt, device=dev)).shape == (4096, N)
    with pytest.raises(antq_lib.AntqError, match="float32"):
        call(torch.zeros(9, K, dtype=torch.float32, device=dev))
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(antq_lib.AntqError, match="at most 4096 rows"):
            call(torch.zeros(4097, K, dtype=dt, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. model level
# ---------------------------------------------------------------------------------------------------------------------------
WIDTHS = {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_with_fused_byte_gemm_rows(antq_lib, dev, tree, capsys, monkeypatch):
    """test_gpu_linear8.py's tiny model: layer "6" (64 -> 20, 8 bits) is the fusable byte-coded Linear; "0", "3", "5" hold 4-bit codes."""
    import torch
    qmod, qutil = _trees(tree)
    dtype_name, dt = "bfloat16", torch.bfloat16
    base = _tiny(tree, dev, dt)
    xs = {r: _input(dev, dt, r, seed=r) for r in (3, 9, 40, 65, 130, 257)}
    decodes = []
    real_decode8 = antq_lib.decode8
    monkeypatch.setattr(antq_lib, "decode8", lambda *a, **kw: (decodes.append(1), real_decode8(*a, **kw))[1])
    opts = dict(fused_linear=True, byte_codes=True, fused_bytes=True)
    counters = lambda b: (b.fused_byte_calls, b.fused_byte_mm_calls, b.fused_byte_gemm_calls)   # noqa: E731
    four_bit = lambda b: (b.fused_calls, b.fused_mm_calls, b.fused_gemm_calls)                  # noqa: E731
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, plain, gemm, both, lean = (copy.deepcopy(base) for _ in range(5))
        tbank = qutil.pack_model(twin, byte_codes=True)
        assert {e["name"]: e["width"] for e in tbank.entries.values()} == WIDTHS
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        y_twin = {r: twin(x) for r, x in xs.items()}

        # fused_bytes without the option: today's routing, and what the 4-bit layers count and compute
        pbank = qutil.pack_model(plain, **opts)
        y_plain, n4_plain = {}, {}
        for r in xs:
            before = four_bit(pbank)
            y_plain[r] = plain(xs[r])
            n4_plain[r] = tuple(a - b for a, b in zip(four_bit(pbank), before))
        assert pbank.fused_byte_gemm_rows is None and counters(pbank) == (1, 0, 0)
        assert all(torch.equal(y_plain[r], y_twin[r]) for r in (9, 40, 65, 130, 257))
        mbank = qutil.pack_model(copy.deepcopy(base), fused_byte_rows=64, **opts)
        y_mm = {r: mbank.model(xs[r]) for r in (9, 40)}                # antq_linear8_mm's bits
        assert counters(mbank) == (0, 2, 0)

        gbank = qutil.pack_model(gemm, fused_byte_gemm_rows=256, **opts)
        bbank = qutil.pack_model(both, fused_byte_gemm_rows=256, fused_byte_rows=64, **opts)
        lbank = qutil.pack_model(lean, fused_byte_gemm_rows=256, keep_images=False, release_weights=True, **opts)
        le = {e["name"]: e for e in lbank.entries.values()}
        assert le["6"]["out"] is None and le["6"]["fusable"] and le["6"]["width"] == 8
        y130 = {}
        for model, bank in ((gemm, gbank), (both, bbank), (lean, lbank)):
            assert bank.fused_byte_gemm_rows == 256 and bank.fused_gemm_rows is None
            assert bank.fused_byte_rows == (64 if bank is bbank else None)
            # 3 rows: antq_linear8, the bits of a bank without the option
            n4 = four_bit(bank)
            assert torch.equal(model(xs[3]), y_plain[3]) and counters(bank) == (1, 0, 0)
            assert tuple(a - b for a, b in zip(four_bit(bank), n4)) == n4_plain[3]
            for t in bank._scratch.values():
                t.fill_(7.0)
            n_mm, n_gemm = 0, 0
            # 9 and 40 rows: the tiled kernel without fused_byte_rows, antq_linear8_mm (counter and bits) with it
            for r in (9, 40):
                n4, n_dec, n_launch = four_bit(bank), len(decodes), bank.launches
                y, seen = _traced_forward(model, xs[r])
                if bank is bbank:
                    n_mm += 1
                    assert torch.equal(y, y_mm[r]), (tree, r)
                else:
                    n_gemm += 1
                assert counters(bank) == (1, n_mm, n_gemm), (tree, r)
                assert tuple(a - b for a, b in zip(four_bit(bank), n4)) == n4_plain[r], (tree, r)
                _check_layers_mm(seen, model, images, dtype_name)
                if bank is not lbank:                    # (the lean bank's 4-bit layers decode into the scratch at these rows)
                    assert len(decodes) == n_dec and bank.launches == n_launch
            # 65 and 130 rows: the tiled kernel, within the bound layer by layer; layer "6" decodes nothing
            for r in (65, 130):
                n4, n_dec, n_launch = four_bit(bank), len(decodes), bank.launches
                y, seen = _traced_forward(model, xs[r])
                n_gemm += 1
                assert counters(bank) == (1, n_mm, n_gemm), (tree, r)
                assert tuple(a - b for a, b in zip(four_bit(bank), n4)) == n4_plain[r], (tree, r)
                _check_layers_mm(seen, model, images, dtype_name)
                assert y.shape == y_twin[r].shape and bool(torch.isfinite(y.float()).all())
                assert len(decodes) == n_dec and bank.launches == n_launch, (tree, r, "antq_decode8 ran")
                if r == 130:
                    y130[bank] = y
                    y130[bank, "6"] = seen["6"][1]
            # the 4-bit layers of the same model ("3" and "5", upstream of "6"): their bits as without the option
            _, seen_plain = _traced_forward(plain, xs[130])
            for n in ("3", "5"):
                assert torch.equal(seen[n][0], seen_plain[n][0]) and torch.equal(seen[n][1], seen_plain[n][1]), (tree, n)
            # 257 rows: the fallback, bit-equal to the unfused twin, no counter moves
            assert torch.equal(model(xs[257]), y_twin[257]) and counters(bank) == (1, n_mm, n_gemm)
        assert torch.equal(y130[gbank], y130[lbank]) and torch.equal(y130[gbank], y130[bbank])   # the same kernel on the same codes
        assert torch.equal(y130[gbank, "6"], y130[lbank, "6"]) and torch.equal(y130[gbank, "6"], y130[bbank, "6"])

        # keep_images=False: 65- and 130-row calls of layer "6" decode nothing and leave the scratch alone
        mod6 = lean.get_submodule("6")
        for r in (65, 130):
            _, seen = _traced_forward(lean, xs[r])
            for t in lbank._scratch.values():
                t.fill_(7.0)
            n_dec, n_launch, n_gemm = len(decodes), lbank.launches, lbank.fused_byte_gemm_calls
            y6_again = mod6(seen["5"][1])               # (layer "6" quantises its own input: the output of "5")
            assert lbank.fused_byte_gemm_calls == n_gemm + 1 and len(decodes) == n_dec and lbank.launches == n_launch
            assert torch.equal(y6_again, seen["6"][1])
            assert lbank._scratch and all(bool((t == 7.0).all()) for t in lbank._scratch.values())
        # (the counter works: the 257-row call of the lean bank did decode layer "6" into the scratch)
        n_dec = len(decodes)
        lean(xs[257])
        assert len(decodes) > n_dec

        # float32: the option is accepted, such layers keep their present path
        f32 = _tiny(tree, dev, torch.float32)
        f32(_input(dev, torch.float32, 4))
        f32_twin = copy.deepcopy(f32)
        qutil.pack_model(f32_twin, byte_codes=True)
        b32 = qutil.pack_model(f32, fused_byte_gemm_rows=256, **opts)
        x130f = _input(dev, torch.float32, 130, seed=130)
        assert torch.equal(f32(x130f), f32_twin(x130f)) and counters(b32) == (0, 0, 0)

        # the checkpoint into a fresh model with the same options: the same 130-row bits
        sd = qutil.packed_state_dict(lean)
        fresh = _tiny(tree, dev, dt, seed=99)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, fused_bytes=True, keep_images=False, fused_byte_gemm_rows=256)
        assert bank2.fused_byte_gemm_rows == 256 and {e["name"]: e["width"] for e in bank2.entries.values()} == WIDTHS
        assert torch.equal(fresh(xs[130]), y130[lbank]) and bank2.fused_byte_gemm_calls == 1

        # a captured 130-row forward replays twice to the eager bits
        static_x = xs[130].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_gemm = lbank.fused_byte_gemm_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_byte_gemm_calls == n_gemm + 1
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
