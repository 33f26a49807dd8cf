"""The packed 4-bit linear on the GPU: antq_linear4 (csrc/antq_k_linear4.h) computes y = x . W^T (+ bias) from the code bytes,
W being the image antq_decode4 writes.  The independent yardstick is include/antq.h's decode rule restated in numpy on the
code bytes, and a float64 matmul.  Exact tests compare bits; the general test holds the result to the bound of an fp32 sum."""
import copy
import importlib
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
    """include/antq.h restated on the code bytes: element 2k in the low nibble; with the pair rule nibble 15 -> 0 and its
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
    """x = e_k (and -2 e_k), 8 rows per call: y[m, n] is bit for bit element [n, k] of antq_decode4's image (times -2, exact)
    and of the numpy yardstick.  Codes hold every byte value at varying positions; scales ordinary and so small that the
    smallest nonzero weights (all of them, for the tiny per-tensor scale) are subnormal in the output type."""
    import torch
    dt = getattr(torch, dtype_name)
    K, N = 520, 5
    tiny = 1.5e-4 if dtype_name == "float16" else 3.0e-38
    codes_np = np.concatenate([(np.arange(K // 2) + 37 * n) % 256 for n in range(N)]).astype(np.uint8)
    for n in range(N):
        assert np.unique(codes_np[n * K // 2:(n + 1) * K // 2]).size == 256
    eye = torch.eye(K, device=dev, dtype=dt)
    eye_m2 = eye * -2
    codes = torch.from_numpy(codes_np).to(dev)
    for name, g, gmax, nn, ovp in _books():
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for per_row, a_np in ((True, np.float32([1.0, 0.06, tiny, 20 * tiny, 0.37])), (False, np.float32([0.37])), (False, np.float32([tiny]))):
            a = torch.from_numpy(a_np).to(dev)
            want = _yardstick(codes_np, a_np, N if per_row else 1, K if per_row else N * K, per_row, g, gmax, nn, ovp, dtype_name).reshape(N, K)
            sub = np.abs(_value(want, dtype_name))
            lim = {"float32": 2.0 ** -126, "bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype_name]
            if a_np.min() <= tiny:
                assert ((sub > 0) & (sub < lim)).any(), "no subnormal weight in this case"
            image = antq_lib.decode4(codes, a, plan, gmax, N if per_row else 1, K if per_row else N * K, per_row, dt, n_normal=nn, ovp=ovp).view(N, K)
            assert np.array_equal(_bits(image), want), (name, dtype_name, per_row, "antq_decode4 against the yardstick")
            # (exact: a doubling; + 0.0: where the weight is zero the sum of +0 and the products' -0 is +0)
            want_m2 = _round((_value(want, dtype_name) * -2 + 0.0).astype(np.float32), dtype_name)
            y1 = torch.empty(K, N, dtype=dt, device=dev)
            y2 = torch.empty(K, N, dtype=dt, device=dev)
            for k0 in range(0, K, 8):
                antq_lib.linear4(codes, eye[k0:k0 + 8], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y1[k0:k0 + 8])
                antq_lib.linear4(codes, eye_m2[k0:k0 + 8], a, gd, gmax, N, K, per_row, n_normal=nn, ovp=ovp, out=y2[k0:k0 + 8])
            torch.cuda.synchronize()
            assert np.array_equal(_bits(y1.t()), want), (name, dtype_name, per_row, float(a_np.min()))
            assert np.array_equal(_bits(y2.t()), want_m2), (name, dtype_name, per_row, float(a_np.min()), "-2 e_k")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact sums
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_K = (8, 504, 512, 520, 2056, 4096)
EXACT_N = (1, 2, 3, 4, 5, 7, 8, 9, 17, 33)


def _lowest_bit_exponent(t):
    """exponent of the lowest set bit of every nonzero float64 in t"""
    m, e = np.frexp(t[t != 0])
    mi = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)


def _exact_case(rng, K, book, dtype_name, per_row, N=max(EXACT_N)):
    """Codes, power-of-two scales and small-integer x (8 rows) for which every product and every partial sum, in any order,
    is an integer below 2^24 in units of one power of two -- asserted here in float64 -- with the exact result."""
    name, g, gmax, nn, ovp = book
    codes = _random_codes(rng, N * K // 2, ovp)
    j = rng.integers(-2, 2, N if per_row else 1)
    alpha = (np.float32(gmax) * np.exp2(j).astype(np.float32)).astype(np.float32)        # alpha / gmax = 2^j exactly
    assert np.array_equal((alpha / np.float32(gmax)).astype(np.float32), np.exp2(j).astype(np.float32))
    Wb = _yardstick(codes, alpha, N if per_row else 1, K if per_row else N * K, per_row, g, gmax, nn, ovp, dtype_name).reshape(N, K)
    W = _value(Wb, dtype_name)
    bias = rng.integers(-8, 9, N).astype(np.float64)
    density = 1.0
    while True:
        x = rng.integers(-3, 4, (8, K)).astype(np.float64) * (rng.random((8, K)) < density)
        x[:, 0] = np.where(x[:, 0] == 0, 1.0, x[:, 0])
        terms = x[:, None, :] * W[None, :, :]                          # [8, N, K]
        nz = np.abs(terms[terms != 0])
        unit = 2.0 ** min(int(_lowest_bit_exponent(terms).min()), 0)   # (the bias: whole numbers)
        mass = (np.abs(terms).sum(-1) + np.abs(bias)[None, :]) / unit
        if mass.max() < 2.0 ** 24:
            break
        density *= 0.5
    # the premise, in float64: every term a whole multiple of the unit, and the sum of magnitudes below 2^24 units -- a
    # fortiori below 2^24 in units of the smallest nonzero |term|
    assert np.array_equal(terms / unit, np.round(terms / unit)) and mass.max() < 2.0 ** 24
    assert ((np.abs(terms).sum(-1) + np.abs(bias)[None, :]) / nz.min()).max() < 2.0 ** 24
    y = terms.sum(-1)                                                   # exact in float64: < 2^24 units
    return codes, alpha, x, bias, y, density


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_exact_sums(antq_lib, dev, dtype_name):
    """Dyadic codebooks, power-of-two scales, small-integer activations: whatever the order of the sum, every partial sum is
    exact, so the result must be the exact one rounded to the type.  K around the step sizes of both code paths (4 and 16
    bytes per lane: 504 / 520 / 2056 are no multiples of 32), every N up to two workgroups' tails, M = 1..8, bias and none."""
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(5)
    for bname in ("pot_b4_s", "olive_int", "olive_flint"):
        book = _book(bname)
        name, g, gmax, nn, ovp = book
        plan = antq_lib.plan_for(g)
        gd = plan.grid_dev(dev)
        for ki, K in enumerate(EXACT_K):
            per_row = ki % 2 == 0 or ovp
            # (per-row scales: the codes of a prefix of rows are that smaller layer's codes; one scale per tensor: the table is
            # shared by a wavefront's rows, so every N gets codes of its own and the row tails run with tstride = 0 too)
            cases = [(EXACT_N, _exact_case(rng, K, book, dtype_name, True))] if per_row else \
                    [((N,), _exact_case(rng, K, book, dtype_name, False, N)) for N in EXACT_N]
            outs = []
            for ns, (codes_np, a_np, x_np, b_np, y_np, density) in cases:
                x = _tensor(_round(x_np.astype(np.float32), dtype_name), dtype_name, dev)
                bias = _tensor(_round(b_np.astype(np.float32), dtype_name), dtype_name, dev)
                a = torch.from_numpy(a_np).to(dev)
                for N in ns:
                    ni = EXACT_N.index(N)
                    codes = torch.from_numpy(codes_np[:N * K // 2]).to(dev)
                    for M in range(1, 9):
                        for with_bias in ((True, False) if (ni + M) % 3 == 0 else ((ni + M) % 2 == 0,)):
                            y = antq_lib.linear4(codes, x[:M], a, gd, gmax, N, K, per_row, bias=bias[:N] if with_bias else None, n_normal=nn, ovp=ovp)
                            outs.append((N, M, with_bias, y, y_np, b_np, density))
            torch.cuda.synchronize()
            assert {o[2] for o in outs} == {True, False} and {o[0] for o in outs} == set(EXACT_N)
            for N, M, with_bias, y, y_np, b_np, density in outs:
                want = y_np[:M, :N] + (b_np[None, :N] if with_bias else 0.0)
                assert np.array_equal(_bits(y), _round(want.astype(np.float32), dtype_name)), (name, dtype_name, K, N, M, with_bias, density)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. general data against the bound of an fp32 sum
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss_case(antq_lib, dev, rng, book, dtype_name, N, K, M=8):
    """Encoded Gaussian weights (0.1 % planted outliers for the pair rule), Gaussian x and bias in the type; the yardstick's
    weights, float64 result and float64 mass S = sum |x W| + |bias|."""
    import torch
    name, g, gmax, nn, ovp = book
    plan = antq_lib.plan_for(g)
    w = rng.standard_normal((N, K)).astype(np.float32) * np.float32(0.05)
    if ovp:
        big = rng.random((N, K)) < 0.001
        w = np.where(big, np.sign(w) * np.float32(0.05) * rng.uniform(8, 20, (N, K)).astype(np.float32), w)
        a_np = (3 * w.std(1)).astype(np.float32)
    else:
        a_np = (np.abs(w).max(1) * np.float32(0.9)).astype(np.float32)
    if g.min() >= 0:
        w = np.abs(w)
    wt = _tensor(_round(w, dtype_name), dtype_name, dev)
    a = torch.from_numpy(a_np).to(dev)
    codes = antq_lib.encode4(wt, a, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
    codes_np = codes.cpu().numpy()
    if ovp:
        assert ((codes_np & 15) == 15).any() or ((codes_np >> 4) == 15).any()
    W = _value(_yardstick(codes_np, a_np, N, K, True, g, gmax, nn, ovp, dtype_name), dtype_name)
    xb = _round(rng.standard_normal((M, K)).astype(np.float32), dtype_name)
    bb = _round(rng.standard_normal(N).astype(np.float32), dtype_name)
    x64, b64 = _value(xb, dtype_name), _value(bb, dtype_name)
    y64 = x64 @ W.T + b64[None, :]
    S = np.abs(x64) @ np.abs(W).T + np.abs(b64)[None, :]
    return dict(codes=codes, a=a, gd=plan.grid_dev(dev), x=_tensor(xb, dtype_name, dev), bias=_tensor(bb, dtype_name, dev), y64=y64, S=S,
                gmax=gmax, nn=nn, ovp=ovp, N=N, K=K)


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
        for K in (768, 4096):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, 33, K)
            for M in (1, 3, 8):
                y = antq_lib.linear4(c["codes"], c["x"][:M], c["a"], c["gd"], c["gmax"], 33, K, True, bias=c["bias"], n_normal=c["nn"], ovp=c["ovp"])
                ok, worst = _within_bound(_value(_bits(y), dtype_name), c["y64"][:M], c["S"][:M], K, dtype_name)
                print("%s %s K=%d M=%d: worst error / bound %.3g" % (bname, dtype_name, K, M, worst))
                assert ok, (bname, dtype_name, K, M, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_same_bits_every_run_and_for_every_batch(antq_lib, dev, dtype_name):
    rng = np.random.default_rng(29)
    for bname in ("flint_b4_s", "olive_flint"):
        for K in (520, 4096):
            c = _gauss_case(antq_lib, dev, rng, _book(bname), dtype_name, 33, K)
            run = lambda x: _bits(antq_lib.linear4(c["codes"], x, c["a"], c["gd"], c["gmax"], 33, K, True, bias=c["bias"], n_normal=c["nn"], ovp=c["ovp"]))
            y8 = run(c["x"])
            assert np.array_equal(y8, run(c["x"])), (bname, dtype_name, K, "two runs")
            for m in range(8):
                assert np.array_equal(run(c["x"][m:m + 1])[0], y8[m]), (bname, dtype_name, K, m, "a row alone")
            assert np.array_equal(run(c["x"][:5]), y8[:5]), (bname, dtype_name, K, "5 rows against 8")
            for M in (2, 3, 4, 6, 7):
                assert np.array_equal(run(c["x"][:M]), y8[:M]), (bname, dtype_name, K, M)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. footprint
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_guard_words_and_inputs_untouched(antq_lib, dev, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(31)
    book = _book("olive_flint")
    name, g, gmax, nn, ovp = book
    plan = antq_lib.plan_for(g)
    gd = plan.grid_dev(dev)
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    checks = []
    for K in (8, 504, 520, 2056, 4096):
        for N in (1, 3, 5, 7, 9, 17, 33):
            codes_np = _random_codes(rng, N * K // 2, ovp)
            codes = torch.from_numpy(codes_np).to(dev)
            a = torch.from_numpy(np.exp(rng.uniform(-4, 0, N)).astype(np.float32)).to(dev)
            for M in (1, 3, 5, 7):
                x = torch.randn(M, K, device=dev).to(dt)
                x0, c0 = x.clone(), codes.clone()
                full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
                y = full[GUARD:GUARD + M * N]
                antq_lib.linear4(codes, x, a, gd, gmax, N, K, True, n_normal=nn, ovp=ovp, out=y)
                checks.append((K, N, M, full, x, x0, codes, c0))
    torch.cuda.synchronize()
    for K, N, M, full, x, x0, codes, c0 in checks:
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (dtype_name, K, N, M, "guard words")
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
LINEARS = ("3", "5")


def _tiny(tree, dev, dt, seed=1):
    """Layers by name: "0" conv with K = 72, "3" linear 64 -> 48, "5" linear 48 -> 64."""
    import torch
    import torch.nn as nn
    qmod, qutil = _trees(tree)
    qutil.set_quantizer(_args(mode=MODES[tree], wbit=4, abit=4))
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(), nn.Flatten(), nn.Linear(64, 48), nn.ReLU(), nn.Linear(48, 64))
    model = qmod.quantize_model(net)
    assert [n for n, m in model.named_children() if hasattr(m, "quant_weight")] == ["0", "3", "5"]
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
        ok, worst = _within_bound(y.double().cpu().numpy().reshape(y64.shape), y64, S, W.shape[1], dtype_name)
        assert ok, (n, dtype_name, worst)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_with_fused_linear(antq_lib, dev, tree, dtype_name, capsys):
    import torch
    qmod, qutil = _trees(tree)
    dt = getattr(torch, dtype_name)
    base = _tiny(tree, dev, dt)
    x3, x9 = _input(dev, dt, 3, seed=3), _input(dev, dt, 9, seed=9)
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, fused, lean = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
        tbank = qutil.pack_model(twin)
        assert sorted(e["name"] for e in tbank.entries.values()) == ["0", "3", "5"] and tbank.fused_calls == 0
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        y9_twin = twin(x9)
        twin(x3)
        assert tbank.fused_calls == 0                   # without the option nothing changes

        # fused_linear, images kept
        fbank = qutil.pack_model(fused, fused_linear=True)
        assert fbank.nbytes() == tbank.nbytes()
        y3, seen = _traced_forward(fused, x3)
        assert fbank.fused_calls == len(LINEARS)
        _check_layers(seen, fused, images, dtype_name)
        assert torch.equal(fused(x9), y9_twin) and fbank.fused_calls == len(LINEARS)
        assert torch.equal(fused(x3), y3) and fbank.fused_calls == 2 * len(LINEARS)

        # no images for the Linear layers: codes + one scratch
        lbank = qutil.pack_model(lean, fused_linear=True, keep_images=False, release_weights=True)
        for e in lbank.entries.values():
            assert (e["out"] is None) == (e["name"] in LINEARS)
            assert e["mod"].weight.numel() == (0 if e["name"] in LINEARS else e["out"].numel())
        lin_bytes = [images[n].numel() * images[n].element_size() for n in LINEARS]
        assert lbank.nbytes()[0] == tbank.nbytes()[0] and lbank.nbytes()[1] == tbank.nbytes()[1] - sum(lin_bytes) + max(lin_bytes)
        y3_lean, seen = _traced_forward(lean, x3)
        assert lbank.fused_calls == len(LINEARS)
        _check_layers(seen, lean, images, dtype_name)
        assert torch.equal(y3_lean, y3)                 # the same kernel on the same codes
        y9_lean = lean(x9)
        assert torch.equal(y9_lean, y9_twin) and lbank.fused_calls == len(LINEARS)
        assert torch.equal(lean(x3), y3) and torch.equal(lean(x9), y9_twin)

        # the checkpoint never holds images: into a fresh model with the same options
        sd = qutil.packed_state_dict(lean)
        for n in ("0",) + LINEARS:
            assert n + ".weight" not in sd and sd[n + ".quant_weight.codes"].dtype == torch.uint8
        fresh = _tiny(tree, dev, dt, seed=99)
        bank2 = qutil.load_packed_state_dict(fresh, sd, fused_linear=True, keep_images=False)
        assert all((e["out"] is None) == (e["name"] in LINEARS) for e in bank2.entries.values())
        assert torch.equal(fresh(x3), y3) and torch.equal(fresh(x9), y9_twin) and bank2.fused_calls == len(LINEARS)

        # a captured 3-row forward replays to the same bits
        static_x = x3.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lean(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n_calls = lbank.fused_calls
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = lean(static_x)
        assert lbank.fused_calls == n_calls + len(LINEARS)
        for step in range(2):
            static_y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, y3), (tree, dtype_name, step)
    # a forward that wants gradients: there is no float weight to train
    for model in (fused, lean):
        with pytest.raises(antq_lib.AntqError):
            model(x3)
    # the model retyped: the bank rebuilds codes, scales and scratch from the shapes it remembers (bf16 <-> fp32)
    with torch.no_grad():
        other = torch.float32 if dt == torch.bfloat16 else torch.bfloat16
        fresh.to(other)
        n_calls = bank2.fused_calls
        for x in (x3, x9):
            y = fresh(x.to(other))
            assert y.dtype == other and y.shape == (x.shape[0], 64) and bool(torch.isfinite(y.float()).all())
        assert bank2.fused_calls == n_calls + len(LINEARS)
        assert all(t.dtype == other for t in bank2._scratch.values()) and len(bank2._scratch) == 1
    capsys.readouterr()


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_disabled_quantiser_takes_the_float_weight(antq_lib, dev, tree, capsys):
    """disable_quantization(model) on a packed model: quant_weight hands back the float weight without asking the bank, so
    every option -- images kept or not -- must run F.linear on that weight like the unfused twin, and never the codes."""
    import torch
    qmod, qutil = _trees(tree)
    dt = torch.bfloat16
    base = _tiny(tree, dev, dt)
    x3, x9 = _input(dev, dt, 3, seed=3), _input(dev, dt, 9, seed=9)
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin, fused, lean, bare = (copy.deepcopy(base) for _ in range(4))
        qutil.pack_model(twin)
        banks = [qutil.pack_model(fused, fused_linear=True), qutil.pack_model(lean, fused_linear=True, keep_images=False)]
        bbank = qutil.pack_model(bare, fused_linear=True, keep_images=False, release_weights=True)
        y3_on, y9_on = lean(x3), lean(x9)
        assert torch.equal(fused(x3), y3_on) and torch.equal(twin(x9), y9_on)
        calls = [b.fused_calls for b in banks]
        for m in (twin, fused, lean, bare):
            qutil.disable_quantization(m)
        y3_off, y9_off = twin(x3), twin(x9)
        assert not torch.equal(y9_off, y9_on)           # (4-bit weights and inputs against none: the two paths do differ)
        for m in (fused, lean):
            assert torch.equal(m(x3), y3_off) and torch.equal(m(x9), y9_off)
        assert [b.fused_calls for b in banks] == calls  # nothing ran from the codes
        # a layer that gave its float weight away has nothing to compute with: an error that says so, not a shape mismatch
        for x in (x3, x9):
            with pytest.raises(antq_lib.AntqError, match="release_weights"):
                bare(x)
        # enabled again: the codes serve as before
        for m in (twin, fused, lean, bare):
            qutil.enable_quantization(m)
        for m in (fused, lean, bare):
            assert torch.equal(m(x3), y3_on) and torch.equal(m(x9), y9_on)
        assert [b.fused_calls for b in banks] == [c + len(LINEARS) for c in calls] and bbank.fused_calls == len(LINEARS)
        # load_state_dict re-arms every quantiser; a calibrated one settles before the bank is asked, empty weight or not
        bare.load_state_dict(bare.state_dict())
        assert torch.equal(bare(x3), y3_on) and torch.equal(bare(x9), y9_on)
    capsys.readouterr()
