"""The byte-code linear on the matrix cores: antq_linear8_mm (csrc/antq_k_linear_mm.h with Lin8Codec) computes y = x . W^T (+ bias) for
1 .. 64 rows of bf16 / f16 x from the code bytes with v_mfma_f32_16x16x32, W being the image antq_decode8 writes.  The
yardstick is byte_codes_cases.decode_ref (include/antq.h restated in numpy) and float64.  Exact tests compare bits; the general
test holds the result to the derived bound of an fp32 sum (test_gpu_linear4_mm._within_bound).  The inputs come from
linear8_mm_cases.py, which test_linear8_mm_cases_host.py holds to their premises without a GPU.

The kernel's own boundaries: a workgroup owns 16 / 32 / 64 output rows (the launcher's choice, forced here through
antq_debug_set key 22 so that every tile shape runs at the small N of a test -- no result may depend on it); K is cut into
chunks of 64 elements (codes read 16 bytes per lane: K % 16 == 0 and aligned codes) or of 32 (8 bytes per lane) dealt to eight
wavefronts in turn through a ring of 4 / 3 / 2 chunks.

Without the feature every test here fails: _lib has no linear8_mm and pack_model no fused_byte_rows."""
import copy

import numpy as np
import pytest

import byte_codes_cases as bc
import encode4_cases as ec
import linear8_cases as lc
import linear8_mm_cases as mc
from test_gpu_linear4_mm import _within_bound
from test_gpu_linear8 import GUARD, LINEARS, _bits, _codes, _input, _round, _tensor, _tiny, _traced_forward, _trees

pytestmark = pytest.mark.gpu

TILES = mc.TILES


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


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", mc.DTYPES)
@pytest.mark.parametrize("K", mc.ONE_HOT_K)
def test_one_hot_rows_read_the_image(antq_lib, oracle, dev, tiles, K, dtype_name):
    """x = e_k (and -2 e_k) in calls of 64 rows: y[m, n] is bit for bit element [n, k] of antq_decode8's image (times -2, exact)
    and of decode_ref.  Every byte value in every row at every position of a lane's bytes, every pair form, codes beyond the
    book; scales ordinary and so small that weights are subnormal in the type; N = 37 is two workgroups and a tail at every tile
    shape but the largest.  This is what catches a wrong lane map, partner byte, table stride or k permutation."""
    import torch
    dt = getattr(torch, dtype_name)
    N = mc.ONE_HOT_N
    eye = torch.eye(K, device=dev, dtype=dt)
    eye_m2 = eye * -2
    for bi, name in enumerate(mc.ONE_HOT_BOOKS):
        _, g, gmax, nn, ovp = bc.book(name)
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        codes_np = lc.one_hot_codes(name, K, N=N)
        codes = _codes(codes_np, dev)
        for si, (per_row, a5) in enumerate(lc.one_hot_scales(dtype_name)):
            a_np = mc.scale_rows(a5, N) if per_row else a5
            a = torch.from_numpy(a_np).to(dev)
            want = lc.image_ref(oracle, codes_np, a_np, per_row, name, dtype_name)
            image = antq_lib.decode8(codes, a, plan, gmax, N if per_row else 1, K if per_row else N * K, per_row, dt, n_normal=nn, ovp=ovp).view(N, K)
            assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode8 against the yardstick")
            # (exact: a doubling; + 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
            want_m2 = _round(oracle, (lc.value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
            y1 = torch.empty(K, N, dtype=dt, device=dev)
            y2 = torch.empty(K, N, dtype=dt, device=dev)
            for ci, k0 in enumerate(range(0, K, 64)):
                tiles(TILES[(ci + bi + si) % 3])
                antq_lib.linear8_mm(codes, eye[k0:k0 + 64], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + 64])
                antq_lib.linear8_mm(codes, eye_m2[k0:k0 + 64], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + 64])
            torch.cuda.synchronize()
            bad1, bad2 = int((_bits(y1.t()) != want).sum()), int((_bits(y2.t()) != want_m2).sum())
            assert bad1 == 0, (name, dtype_name, K, per_row, float(a_np.min()), "%d elements differ" % bad1)
            assert bad2 == 0, (name, dtype_name, K, per_row, float(a_np.min()), "-2 e_k", "%d elements differ" % bad2)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype_name", mc.MM_EXACT_CASES)
def test_exact_sums(antq_lib, oracle, dev, tiles, name, dtype_name):
    """Dyadic codebooks, power-of-two scales, small-integer activations: whatever the order of the sum -- inside an MFMA
    step, along a wavefront's chain, across the eight wavefronts -- every partial sum is exact, so the result must be the exact
    one rounded to the type.  Every K around the split's boundaries on both code paths and around the first refill of every
    ring depth, N around every tile shape, M around every tile of x, every tile shape, bias and none, per-row scales and one
    per tensor, codes on and 8 bytes off a 16-byte boundary."""
    import torch
    _, g, gmax, nn, ovp = bc.book(name)
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    failed = []
    for K in mc.EXACT_K:
        per_row, cases = mc.exact_cases_of(oracle, name, K, dtype_name)
        by_n = {N: c for ns, c in cases for N in ns}
        dev_case = {}
        outs = []
        for ni, mi, off, nt, forms in mc.exact_runs(K):
            N, M = mc.EXACT_N[ni], mc.EXACT_M[mi]
            c = by_n[N]
            if id(c) not in dev_case:
                dev_case[id(c)] = (_tensor(_round(oracle, c["x"], dtype_name), dtype_name, dev),
                                   _tensor(_round(oracle, c["bias"], dtype_name), dtype_name, dev), torch.from_numpy(c["alpha"]).to(dev), {})
            x, bias, a, code_cache = dev_case[id(c)]
            if (N, off) not in code_cache:
                code_cache[(N, off)] = _codes(c["codes"][:N], dev, off)
            codes = code_cache[(N, off)]
            assert codes.data_ptr() % 16 == off
            tiles(nt)
            for with_bias in forms:
                y = antq_lib.linear8_mm(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N] if with_bias else None, n_normal=nn, ovp=ovp)
                outs.append((N, M, off, nt, with_bias, y, c))
        torch.cuda.synchronize()
        assert {o[4] for o in outs} == {True, False} and {o[0] for o in outs} == set(mc.EXACT_N) and {o[1] for o in outs} == set(mc.EXACT_M)
        assert {o[3] for o in outs} == set(TILES) and {o[2] for o in outs} == set(mc.exact_offsets(K))
        for N, M, off, nt, with_bias, y, c in outs:
            want = c["y"][:M, :N] + (c["bias"][None, :N] if with_bias else 0.0)
            if not np.array_equal(_bits(y), _round(oracle, want, dtype_name)):
                failed.append((K, N, M, off, nt, with_bias, per_row, c["density"]))
    assert not failed, (name, dtype_name, "%d launches differ" % len(failed), failed[:8])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
_GAUSS = {}


def _gauss_case(antq_lib, oracle, dev, name, dtype_name, K, seed=17):
    """Encoded Gaussian weights and 64 rows of x; decode_ref's weights, the float64 result and the float64 mass
    S = sum |x W| + |bias|.  Built once per argument set and shared (nothing writes to it)."""
    import torch
    key = (name, dtype_name, K, seed)
    if key in _GAUSS:
        return _GAUSS[key]
    _, g, gmax, nn, ovp = bc.book(name)
    N = mc.GENERAL_N
    plan = antq_lib.plan_for(g)
    d = lc.gauss_weights(name, dtype_name, K, N=N, M=64, seed=seed)
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


def _mm(antq_lib, c, x, N=None, bias=True, out=None):
    N = c["N"] if N is None else N
    return antq_lib.linear8_mm(c["codes"][:N * c["K"]], x, c["a"], c["gd"], c["gmax"], N, c["K"], True,
                               bias=c["bias"][:N] if bias else None, n_normal=c["nn"], ovp=c["ovp"], out=out)


@pytest.mark.parametrize("dtype_name", mc.DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, oracle, dev, dtype_name):
    for name in mc.GENERAL_BOOKS:
        for K in mc.GENERAL_K:
            c = _gauss_case(antq_lib, oracle, dev, name, dtype_name, K)
            assert c["x"].shape == (64, K)
            for M in mc.GENERAL_M:
                y = _mm(antq_lib, c, c["x"][:M])
                ok, worst = _within_bound(lc.value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d M=%d: worst error / bound %.3g" % (name, dtype_name, K, M, worst))
                assert ok, (name, dtype_name, K, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", mc.DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, oracle, dev, tiles, dtype_name):
    import torch
    for name in ("flint_b6_s", "olive_int_b8"):
        for K in (520, 4096):
            c = _gauss_case(antq_lib, oracle, dev, name, dtype_name, K)
            run = lambda x, N=mc.GENERAL_N: _bits(_mm(antq_lib, c, x, N=N))   # noqa: E731
            tiles(0)
            y64 = run(c["x"])
            assert np.array_equal(y64, run(c["x"])), (name, dtype_name, K, "two runs")
            other = torch.randn(64, K, device=dev, generator=torch.Generator(device=dev).manual_seed(K)).to(c["x"].dtype)
            for nt in (0,) + TILES:
                tiles(nt)
                assert np.array_equal(run(c["x"]), y64), (name, dtype_name, K, nt, "tile shape")
                for M in (1, 9, 16, 17, 33, 63):
                    assert np.array_equal(run(c["x"][:M]), y64[:M]), (name, dtype_name, K, nt, M, "a prefix of the rows")
                for m in (0, 7, 16, 37, 63):
                    assert np.array_equal(run(c["x"][m:m + 1])[0], y64[m]), (name, dtype_name, K, nt, m, "a row alone")
                    x2 = other.clone()
                    x2[m] = c["x"][m]
                    assert np.array_equal(run(x2)[m], y64[m]), (name, dtype_name, K, nt, m, "a row in other company")
                assert np.array_equal(run(c["x"], N=17), y64[:, :17]), (name, dtype_name, K, nt, "N = 17 against N = 33")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", mc.DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, tiles, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    _, g, gmax, nn, ovp = bc.book("olive_int_b8")
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in (8, 504, 520, 4096):
        for N in (1, 15, 17, 33, 65):
            codes = _codes(lc.random_codes(rng, N * K, ovp), dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, N)).astype(np.float32)).to(dev)
            for M in (9, 17, 33, 63):
                x = torch.randn(M, K, device=dev).to(dt)
                x0, c0 = x.clone(), codes.clone()
                for nt in TILES:
                    tiles(nt)
                    full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                    y = full[GUARD:GUARD + M * N]
                    antq_lib.linear8_mm(codes, x, a, gd, gmax, N, K, True, n_normal=nn, ovp=ovp, out=y)
                    checks.append((K, N, M, nt, full, x, x0, codes, c0))
    torch.cuda.synchronize()
    for K, N, M, nt, full, x, x0, codes, c0 in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, nt, "guard words")
        assert not (b[GUARD:GUARD + M * N] == guard).all(), (dtype_name, K, N, M, nt, "nothing written")
        assert torch.equal(x, x0), (dtype_name, K, N, M, nt, "x")
        assert torch.equal(codes, c0), (dtype_name, K, N, M, nt, "codes")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. binding
# ---------------------------------------------------------------------------------------------------------------------------
def test_binding_refuses_float32_and_65_rows(antq_lib, dev):
    """_lib.linear8_mm with every tensor on the GPU: float32 and more than LINEAR8_MM_MAX_M rows raise before any launch"""
    import torch
    _, g, gmax, nn, ovp = bc.book("int_b8_s")
    gd = antq_lib.plan_for(g).grid_dev(dev)
    N, K = 16, 64
    codes = torch.zeros(N * K, dtype=torch.uint8, device=dev)
    a = torch.ones(N, device=dev)
    call = lambda x: antq_lib.linear8_mm(codes, x, a, gd, gmax, N, K, True)   # noqa: E731
    for dt in (torch.bfloat16, torch.float16):
        assert call(torch.zeros(64, K, dtype=dt, device=dev)).shape == (64, N)
    with pytest.raises(antq_lib.AntqError, match="float32"):
        call(torch.zeros(9, K, dtype=torch.float32, device=dev))
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(antq_lib.AntqError, match="at most 64 rows"):
            call(torch.zeros(65, K, dtype=dt, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. model level
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


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_with_fused_byte_rows(antq_lib, dev, tree, capsys, monkeypatch):
    """test_gpu_linear8.py's tiny model: layer "6" (64 -> 20, 8 bits) is the fusable byte-coded Linear."""
    import torch
    qmod, qutil = _trees(tree)
    dtype_name, dt = "bfloat16", torch.bfloat16
    base = _tiny(tree, dev, dt)
    xs = {r: _input(dev, dt, r, seed=r) for r in (3, 9, 64, 65)}
    decodes = []
    real_decode8 = antq_lib.decode8
    monkeypatch.setattr(antq_lib, "decode8", lambda *a, **kw: (decodes.append(1), real_decode8(*a, **kw))[1])
    opts = dict(fused_linear=True, byte_codes=True, fused_bytes=True)
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, plain, fused, lean = (copy.deepcopy(base) for _ in range(4))
        tbank = qutil.pack_model(twin, byte_codes=True)
        assert {e["name"]: e["width"] for e in tbank.entries.values()} == {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        y_twin = {r: twin(x) for r, x in xs.items()}

        # fused_bytes without the option: 9 rows are routed as today
        pbank = qutil.pack_model(plain, **opts)
        y3_plain = plain(xs[3])
        assert pbank.fused_byte_rows is None and (pbank.fused_byte_calls, pbank.fused_byte_mm_calls) == (1, 0)
        assert torch.equal(plain(xs[9]), y_twin[9]) and (pbank.fused_byte_calls, pbank.fused_byte_mm_calls) == (1, 0)

        fbank = qutil.pack_model(fused, fused_byte_rows=64, **opts)
        lbank = qutil.pack_model(lean, fused_byte_rows=64, keep_images=False, release_weights=True, **opts)
        assert fbank.fused_byte_rows == 64 and fbank.fused_rows is None
        le = {e["name"]: e for e in lbank.entries.values()}
        assert le["6"]["out"] is None and le["6"]["fusable"] and le["6"]["width"] == 8
        y9 = {}
        for model, bank in ((fused, fbank), (lean, lbank)):
            # 3 rows: antq_linear8, the bits of a bank without the option
            assert torch.equal(model(xs[3]), y3_plain) and (bank.fused_byte_calls, bank.fused_byte_mm_calls) == (1, 0)
            n_mm = 0
            for r in (9, 64):
                y, seen = _traced_forward(model, xs[r])
                n_mm += 1                               # layer "6"; the 4-bit layers have no fused_rows: their own path
                assert (bank.fused_byte_calls, bank.fused_byte_mm_calls, bank.fused_mm_calls) == (1, n_mm, 0), (tree, r)
                _check_layers_mm(seen, model, images, dtype_name)
                assert y.shape == y_twin[r].shape and bool(torch.isfinite(y.float()).all())
                if r == 9:
                    y9[bank] = y
            # 65 rows: the fallback, bit-equal to the unfused twin, no counter moves
            assert torch.equal(model(xs[65]), y_twin[65])
            assert (bank.fused_byte_calls, bank.fused_byte_mm_calls) == (1, n_mm)
        assert torch.equal(y9[fbank], y9[lbank])        # the same kernel on the same codes

        # keep_images=False: a 9-row call of layer "6" decodes nothing and leaves the scratch alone
        mod6 = lean.get_submodule("6")
        _, seen = _traced_forward(lean, xs[9])
        xq6, y6 = seen["6"]
        for t in lbank._scratch.values():
            t.fill_(7.0)
        n_dec, n_launch, n_mm = len(decodes), lbank.launches, lbank.fused_byte_mm_calls
        y6_again = mod6(seen["5"][1])                   # (layer "6" quantises its own input: the output of "5")
        assert lbank.fused_byte_mm_calls == n_mm + 1 and len(decodes) == n_dec and lbank.launches == n_launch
        assert torch.equal(y6_again, y6)
        assert lbank._scratch and all(bool((t == 7.0).all()) for t in lbank._scratch.values())
        # (the counter works: the 65-row call of the lean bank did decode layer "6" into the scratch)
        lean(xs[65])
        assert len(decodes) > n_dec

        # float32: the option is accepted, such layers keep their present path
        f32 = _tiny(tree, dev, torch.float32)
        f32(_input(dev, torch.float32, 4))
        f32_twin = copy.deepcopy(f32)
        qutil.pack_model(f32_twin, byte_codes=True)
        b32 = qutil.pack_model(f32, fused_byte_rows=64, **opts)
        x9f = _input(dev, torch.float32, 9, seed=9)
        assert torch.equal(f32(x9f), f32_twin(x9f)) and b32.fused_byte_mm_calls == 0 and b32.fused_byte_calls == 0

        # the checkpoint into a fresh model with the same options: the same 9-row bits
        sd = qutil.packed_state_dict(lean)
        fresh = _tiny(tree, dev, dt, seed=99)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, fused_bytes=True, keep_images=False, fused_byte_rows=64)
        assert bank2.fused_byte_rows == 64 and {e["name"]: e["width"] for e in bank2.entries.values()} == {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}
        assert torch.equal(fresh(xs[9]), y9[lbank]) and bank2.fused_byte_mm_calls == 1

        # a captured 9-row forward replays twice to the eager bits
        static_x = xs[9].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_mm = lbank.fused_byte_mm_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_byte_mm_calls == n_mm + 1
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, y9[lbank]), (tree, step)
    # a forward that wants gradients: there is no float weight to train
    for model in (fused, lean):
        with pytest.raises(antq_lib.AntqError):
            model(xs[9])
    capsys.readouterr()
