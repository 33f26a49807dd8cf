"""The byte-code linear on the GPU: antq_linear8 (csrc/antq_k_linear8.h) computes y = x . W^T (+ bias) from the code bytes, W
being the image antq_decode8 writes.  The yardstick is byte_codes_cases.decode_ref (include/antq.h restated in numpy) and a
float64 matmul.  Exact tests compare bits; the general test holds the result to the bound of an fp32 sum.  The inputs come
from linear8_cases.py, which test_linear8_cases_host.py holds to their premises without a GPU."""
import copy
import importlib
import types

import numpy as np
import pytest

import byte_codes_cases as bc
import encode4_cases as ec
import linear8_cases as lc

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


def _round(oracle, v, dtype_name):
    return bc.to_bits(oracle, np.ascontiguousarray(v, np.float32), dtype_name)


def _codes(codes_np, dev, off=0):
    """the codes on the device, `off` bytes past a 16-byte boundary (8: the 8-byte path whatever K is)"""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(codes_np).reshape(-1))
    full = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device=dev)
    assert full.data_ptr() % 16 == 0
    t = full[off:off + flat.numel()]
    t.copy_(flat)
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# 1. one-hot rows of x: the weight is the image
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", lc.DTYPES)
@pytest.mark.parametrize("K", lc.ONE_HOT_K)
def test_one_hot_rows_read_the_image(antq_lib, oracle, dev, K, dtype_name):
    """x = e_k (and -2 e_k), 8 rows per call: y[m, n] is bit for bit element [n, k] of antq_decode8's image (times -2, exact)
    and of decode_ref.  Every byte value in every row, every pair form, codes beyond the book; scales ordinary and so small
    that weights are subnormal in the type."""
    import torch
    dt = getattr(torch, dtype_name)
    N = lc.ONE_HOT_N
    eye = torch.eye(K, device=dev, dtype=dt)
    eye_m2 = eye * -2
    for name in lc.ONE_HOT_BOOKS:
        _, g, gmax, nn, ovp = bc.book(name)
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        codes_np = lc.one_hot_codes(name, K)
        codes = _codes(codes_np, dev)
        for per_row, a_np in lc.one_hot_scales(dtype_name):
            a = torch.from_numpy(a_np).to(dev)
            want = lc.image_ref(oracle, codes_np, a_np, per_row, name, dtype_name)
            image = antq_lib.decode8(codes, a, plan, gmax, N if per_row else 1, K if per_row else N * K, per_row, dt, n_normal=nn, ovp=ovp).view(N, K)
            assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode8 against the yardstick")
            # (exact: a doubling; + 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
            want_m2 = _round(oracle, (lc.value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
            y1 = torch.empty(K, N, dtype=dt, device=dev)
            y2 = torch.empty(K, N, dtype=dt, device=dev)
            for k0 in range(0, K, 8):
                antq_lib.linear8(codes, eye[k0:k0 + 8], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + 8])
                antq_lib.linear8(codes, eye_m2[k0:k0 + 8], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + 8])
            torch.cuda.synchronize()
            assert np.array_equal(_bits(y1.t()), want), (name, dtype_name, K, per_row, float(a_np.min()))
            assert np.array_equal(_bits(y2.t()), want_m2), (name, dtype_name, K, per_row, float(a_np.min()), "-2 e_k")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype_name", lc.EXACT_CASES)
def test_exact_sums(antq_lib, oracle, dev, name, dtype_name):
    """Dyadic codebooks, power-of-two scales, small-integer activations: whatever the order of the sum, every partial sum is
    exact, so the result must be the exact one rounded to the type.  K around the step sizes of both code paths (512 / 1024
    elements; where K % 16 == 0 also with the codes 8 bytes off a 16-byte boundary: the 8-byte path at exactly one and two
    steps), every N up to two workgroups' tails, M = 1..8, bias and none, per-row and per-tensor scales."""
    import torch
    _, g, gmax, nn, ovp = bc.book(name)
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    for K in lc.EXACT_K:
        per_row, cases = lc.exact_cases_of(oracle, name, K, dtype_name)
        outs = []
        for ns, c in cases:
            x = _tensor(_round(oracle, c["x"], dtype_name), dtype_name, dev)
            bias = _tensor(_round(oracle, c["bias"], dtype_name), dtype_name, dev)
            a = torch.from_numpy(c["alpha"]).to(dev)
            for N in ns:
                ni = lc.EXACT_N.index(N)
                for off in ((0, 8) if K % 16 == 0 else (0,)):
                    codes = _codes(c["codes"][:N], dev, off)
                    for M in (range(1, 9) if off == 0 else (1, 5, 8)):
                        for with_bias in ((True, False) if (ni + M) % 3 == 0 else ((ni + M) % 2 == 0,)):
                            y = antq_lib.linear8(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N] if with_bias else None, n_normal=nn, ovp=ovp)
                            outs.append((N, M, off, with_bias, y, c))
        torch.cuda.synchronize()
        assert {o[3] for o in outs} == {True, False} and {o[0] for o in outs} == set(lc.EXACT_N)
        for N, M, off, with_bias, y, c in outs:
            want = c["y"][:M, :N] + (c["bias"][None, :N] if with_bias else 0.0)
            assert np.array_equal(_bits(y), _round(oracle, want, dtype_name)), (name, dtype_name, K, N, M, off, with_bias, per_row, c["density"])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss_case(antq_lib, oracle, dev, name, dtype_name, K, seed=17):
    """Encoded Gaussian weights; decode_ref's weights, the float64 result and the float64 mass S = sum |x W| + |bias|."""
    import torch
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    N = lc.GENERAL_N
    plan = antq_lib.plan_for(g)
    d = lc.gauss_weights(name, dtype_name, K, seed=seed)
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
    return dict(codes=codes, a=a, gd=plan.grid_dev(dev), x=_tensor(xb, dtype_name, dev), bias=_tensor(bb, dtype_name, dev), y64=y64, S=S,
                gmax=gmax, nn=nn, ovp=ovp, N=N, K=K)


@pytest.mark.parametrize("dtype_name", lc.DTYPES)
def test_general_data_within_the_fp32_bound(antq_lib, oracle, dev, dtype_name):
    for name in lc.GENERAL_BOOKS:
        for K in lc.GENERAL_K:
            c = _gauss_case(antq_lib, oracle, dev, name, dtype_name, K)
            for M in (1, 3, 8):
                y = antq_lib.linear8(c["codes"], c["x"][:M], c["a"], c["gd"], c["gmax"], c["N"], K, True, bias=c["bias"], n_normal=c["nn"], ovp=c["ovp"])
                ok, worst = lc.within_bound(lc.value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d M=%d: worst error / bound %.3g" % (name, dtype_name, K, M, worst))
                assert ok, (name, dtype_name, K, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", lc.DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, oracle, dev, dtype_name):
    for name in ("flint_b6_s", "olive_int_b8"):
        for K in (520, 4096):
            c = _gauss_case(antq_lib, oracle, dev, name, dtype_name, K, seed=29)
            run = lambda x: _bits(antq_lib.linear8(c["codes"], x, c["a"], c["gd"], c["gmax"], c["N"], K, True, bias=c["bias"], n_normal=c["nn"], ovp=c["ovp"]))   # noqa: E731
            y8 = run(c["x"])
            assert np.array_equal(y8, run(c["x"])), (name, dtype_name, K, "two runs")
            for m in range(8):
                assert np.array_equal(run(c["x"][m:m + 1])[0], y8[m]), (name, dtype_name, K, m, "a row alone")
            for M in (2, 3, 4, 5, 6, 7):
                assert np.array_equal(run(c["x"][:M]), y8[:M]), (name, dtype_name, K, M)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64


@pytest.mark.parametrize("dtype_name", lc.DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    _, g, gmax, nn, ovp = bc.book("olive_int_b8")
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in (8, 504, 520, 2056, 4096):
        for N in (1, 3, 5, 7, 9, 17, 33):
            codes = _codes(lc.random_codes(rng, N * K, ovp), dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, N)).astype(np.float32)).to(dev)
            for M in (1, 3, 5, 7):
                x = torch.randn(M, K, device=dev).to(dt)
                x0, c0 = x.clone(), codes.clone()
                full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                y = full[GUARD:GUARD + M * N]
                antq_lib.linear8(codes, x, a, gd, gmax, N, K, True, n_normal=nn, ovp=ovp, out=y)
                checks.append((K, N, M, full, x, x0, codes, c0))
    torch.cuda.synchronize()
    for K, N, M, full, x, x0, codes, c0 in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, "guard words")
        assert not (b[GUARD:GUARD + M * N] == guard).all(), (dtype_name, K, N, M, "nothing written")
        assert torch.equal(x, x0), (dtype_name, K, N, M, "x")
        assert torch.equal(codes, c0), (dtype_name, K, N, M, "codes")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. module level
# ---------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _trees(tree):
    return (importlib.import_module("ant_quantization_amd.%s.quant_model" % tree),
            importlib.import_module("ant_quantization_amd.%s.quant_utils" % tree))


MODES = {"ant": "ant-int-pot-flint", "olive": "ant-int-flint"}
LINEARS = ("3", "5", "6", "7")


def _tiny(tree, dev, dt, seed=1):
    """tests/test_gpu_byte_codes.py's model.  Layers by name: "0" conv with K = 72, "3" linear 64 -> 48, "5" linear 48 -> 64,
    "6" linear 64 -> 20 set to 8 bits, "7" linear with 20 input features (row length 4 mod 8)."""
    import torch
    import torch.nn as nn
    qmod, qutil = _trees(tree)
    qutil.set_quantizer(_args(mode=MODES[tree], wbit=4, abit=4))
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(), nn.Flatten(), nn.Linear(64, 48), nn.ReLU(), nn.Linear(48, 64),
                        nn.Linear(64, 20), nn.Linear(20, 16))
    model = qmod.quantize_model(net)
    assert [n for n, m in model.named_children() if hasattr(m, "quant_weight")] == ["0", "3", "5", "6", "7"]
    qmod.set_8_bit_layer_l(model, "3")           # the fourth (weight, input) pair: layer "6"
    model = model.to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    return model


def _input(dev, dt, rows, seed=0):
    import torch
    return torch.randn(rows, 8, 2, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)).to(dt)


def _traced_forward(model, x):
    """(output, {linear layer: (its quantised input, its output)})"""
    seen, hooks = {}, []
    for n in LINEARS:
        mod = model.get_submodule(n)
        hooks.append(mod.quant_input.register_forward_hook(lambda m, i, o, n=n: seen.setdefault(n, [None, None]).__setitem__(0, o.detach().clone())))
        hooks.append(mod.register_forward_hook(lambda m, i, o, n=n: seen.setdefault(n, [None, None]).__setitem__(1, o.detach().clone())))
    try:
        y = model(x)
    finally:
        for h in hooks:
            h.remove()
    return y, seen


def _check_layers(seen, model, images, dtype_name):
    """bound 3, layer by layer: every Linear's output against float64 on its own quantised input and the twin's image"""
    for n in LINEARS:
        xq, y = seen[n]
        mod = model.get_submodule(n)
        W = images[n].double().cpu().numpy()
        x64 = xq.double().cpu().numpy().reshape(-1, W.shape[1])
        b64 = mod.bias.detach().double().cpu().numpy()
        y64 = x64 @ W.T + b64[None, :]
        S = np.abs(x64) @ np.abs(W).T + np.abs(b64)[None, :]
        ok, worst = lc.within_bound(y.double().cpu().numpy().reshape(y64.shape), y64, S, W.shape[1], dtype_name)
        assert ok, (n, dtype_name, worst)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_with_fused_bytes(antq_lib, dev, tree, dtype_name, capsys):
    import torch
    qmod, qutil = _trees(tree)
    dt = getattr(torch, dtype_name)
    base = _tiny(tree, dev, dt)
    x3, x9 = _input(dev, dt, 3, seed=3), _input(dev, dt, 9, seed=9)
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, plainf, fused, lean, bare = (copy.deepcopy(base) for _ in range(5))
        tbank = qutil.pack_model(twin, byte_codes=True)
        assert {e["name"]: e["width"] for e in tbank.entries.values()} == {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        y9_twin = twin(x9)

        # without fused_bytes: byte-coded layers keep their image and are not fusable, as test_packed_model_with_byte_codes says
        pbank = qutil.pack_model(plainf, fused_linear=True, keep_images=False, byte_codes=True)
        pe = {e["name"]: e for e in pbank.entries.values()}
        assert pe["6"]["out"] is not None and pe["7"]["out"] is not None and not pe["6"]["fusable"] and not pe["7"]["fusable"]
        assert pe["3"]["out"] is None and pe["3"]["fusable"] and not pbank.fused_bytes
        plainf(x3)
        assert pbank.fused_byte_calls == 0 and pbank.fused_calls == 2

        # fused_bytes, images kept
        fbank = qutil.pack_model(fused, fused_linear=True, byte_codes=True, fused_bytes=True)
        fe = {e["name"]: e for e in fbank.entries.values()}
        assert fe["6"]["fusable"] and fe["6"]["width"] == 8 and not fe["7"]["fusable"] and fe["7"]["width"] == 8
        assert fbank.nbytes() == tbank.nbytes()
        y3, seen = _traced_forward(fused, x3)
        assert fbank.fused_byte_calls == 1 and fbank.fused_calls == 2
        _check_layers(seen, fused, images, dtype_name)
        assert torch.equal(fused(x9), y9_twin) and fbank.fused_byte_calls == 1 and fbank.fused_calls == 2
        assert torch.equal(fused(x3), y3) and fbank.fused_byte_calls == 2

        # no images for the fusable layers: codes + one scratch
        lbank = qutil.pack_model(lean, fused_linear=True, byte_codes=True, fused_bytes=True, keep_images=False, release_weights=True)
        gone = ("3", "5", "6")
        for e in lbank.entries.values():
            assert (e["out"] is None) == (e["name"] in gone), e["name"]
            assert e["mod"].weight.numel() == (0 if e["name"] in gone else e["out"].numel())
        gone_bytes = [images[n].numel() * images[n].element_size() for n in gone]
        assert lbank.nbytes()[0] == tbank.nbytes()[0] and lbank.nbytes()[1] == tbank.nbytes()[1] - sum(gone_bytes) + max(gone_bytes)
        y3_lean, seen = _traced_forward(lean, x3)
        assert lbank.fused_byte_calls == 1 and lbank.fused_calls == 2
        _check_layers(seen, lean, images, dtype_name)
        assert torch.equal(y3_lean, y3)                 # the same kernels on the same codes
        assert torch.equal(lean(x9), y9_twin) and lbank.fused_byte_calls == 1      # decode8 into scratch, then F.linear
        assert torch.equal(lean(x3), y3) and torch.equal(lean(x9), y9_twin)

        # the checkpoint: into a fresh model with the same options
        sd = qutil.packed_state_dict(lean)
        assert sd["6.quant_weight.codes"].numel() == 64 * 20 and "6.weight" not in sd
        fresh = _tiny(tree, dev, dt, seed=99)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, fused_bytes=True, keep_images=False)
        assert all((e["out"] is None) == (e["name"] in gone) for e in bank2.entries.values())
        assert {e["name"]: e["width"] for e in bank2.entries.values()} == {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}
        assert torch.equal(fresh(x3), y3) and torch.equal(fresh(x9), y9_twin) and bank2.fused_byte_calls == 1

        # a captured 3-row forward replays to the same bits
        static_x = x3.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_calls = lbank.fused_byte_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_byte_calls == n_calls + 1
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, y3), (tree, dtype_name, step)

        # a disabled quantiser takes the float weight; after release_weights there is none: the existing error
        y3_on = fused(x3)
        calls = (fbank.fused_calls, fbank.fused_byte_calls)
        qutil.disable_quantization(twin)
        qutil.disable_quantization(fused)
        assert torch.equal(fused(x3), twin(x3)) and (fbank.fused_calls, fbank.fused_byte_calls) == calls
        qutil.enable_quantization(fused)
        assert torch.equal(fused(x3), y3_on)
        bbank = qutil.pack_model(bare, fused_linear=True, byte_codes=True, fused_bytes=True, keep_images=False, release_weights=True)
        qutil.disable_quantization(bare)
        for x in (x3, x9):
            with pytest.raises(antq_lib.AntqError, match="release_weights"):
                bare(x)
        qutil.enable_quantization(bare)
        assert torch.equal(bare(x3), y3) and bbank.fused_byte_calls == 1
    # a forward that wants gradients: there is no float weight to train
    for model in (fused, lean):
        with pytest.raises(antq_lib.AntqError):
            model(x3)
    # the model retyped: the bank rebuilds codes, scales and scratch from the shapes it remembers (bf16 <-> fp32)
    with torch.no_grad():
        other = torch.float32 if dt == torch.bfloat16 else torch.bfloat16
        fresh.to(other)
        n_calls = bank2.fused_byte_calls
        for x in (x3, x9):
            y = fresh(x.to(other))
            assert y.dtype == other and y.shape == (x.shape[0], 16) and bool(torch.isfinite(y.float()).all())
        assert bank2.fused_byte_calls == n_calls + 1
        assert all(t.dtype == other for t in bank2._scratch.values()) and len(bank2._scratch) == 1
    capsys.readouterr()
