"""The integer-domain 4-bit linear on the GPU: antq_quant_i8 against the image of antq_encode8's codes, antq_linear4_i8 bit for
bit against the formula of include/antq.h (S in int64, the epilogue in np.float32), its refusals, and the module surface
(pack_model(integer_linear=True))."""
import copy
import itertools

import numpy as np
import pytest

from test_gpu_linear8 import _args, _trees

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _book(name):
    """(full grid, gmax, n_normal, ovp) as the codec takes them"""
    from ant_quantization_amd import grids
    if name == "olive_int4":
        normal = grids.olive_grid("int", 4, True)
        return np.concatenate([normal, grids.olive_outliers(4, True)]), float(normal.max()), int(normal.size), True
    kind, signed = name.split("_")[1][:-1], name.endswith("s")
    g = grids.ant_grid(kind, 4, signed)
    return g, float(g.max()), 0, False


def _v_of_codes(codes, image, n_normal, ovp):
    """[rows, K] integers of packed 4-bit codes [rows, K/2]: the decoder's pair rule (dec_pair) on the image padded with zeros"""
    g = np.zeros(48, dtype=np.int64)
    g[:image.size] = image
    c0, c1 = (codes & 15).astype(np.int64), (codes >> 4).astype(np.int64)
    if ovp:
        v0 = np.where(c0 == 15, 0, np.where(c1 == 15, g[n_normal + c0], g[c0]))
        v1 = np.where(c1 == 15, 0, np.where(c0 == 15, g[n_normal + c1], g[c1]))
    else:
        v0, v1 = g[c0], g[c1]
    return np.stack([v0, v1], axis=-1).reshape(codes.shape[0], -1)


def _reference(xq, v, aw, I_w, ax, I_x, bias, dt):
    """the formula: exact S, then one rounding per operation in float32, then one to the output type; as raw bits"""
    import torch
    S = xq.astype(np.int64) @ v.T
    y = S.astype(np.float32) * (np.float32(ax) / np.float32(I_x))
    y = y * (aw.astype(np.float32) / np.float32(I_w))[None, :]
    if bias is not None:
        y = y + bias[None, :]
    return S, _bits(torch.from_numpy(y.astype(np.float32)).to(dt))


def _bits(t):
    import torch
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("book", ["ant_int4_s", "ant_flint4_u", "olive_int4"])
def test_quant_i8_is_the_image_of_the_byte_codes(antq_lib, dev, book, dtype_name):
    import torch
    grid, gmax, n_normal, ovp = _book(book)
    plan = antq_lib.plan_for(grid)
    I, image = plan.integer_image()
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(3, 64, device=dev, generator=gen) * (14.0 if ovp else 0.5)      # (OliVe: |x / s| > 32 makes outliers, pairs of them too)
    x[:, ::7] = 0.0
    x[1, 5:9] *= 40.0                                                                # far beyond the clip
    x = x.to(getattr(torch, dtype_name))
    alpha = torch.tensor([gmax if ovp else 1.0, 0.5 * gmax if ovp else 0.7, 2.0 * gmax if ovp else 1.3], device=dev)
    codes = antq_lib.encode8(x, alpha, plan, gmax, 3, 64, True, n_normal=n_normal, ovp=ovp).cpu().numpy().astype(np.int64).reshape(-1, 2)
    q = antq_lib.quant_i8(x, alpha, plan, gmax, 3, 64, True, plan.image_dev(dev), n_normal=n_normal, ovp=ovp)
    g = np.zeros(600, dtype=np.int64)
    g[:image.size] = image
    partner = codes[:, ::-1]
    want = np.where(codes == 255, 0, np.where(ovp & (partner == 255), g[n_normal + codes], g[codes]))
    if ovp:
        assert (codes == 255).any() and (np.abs(want) > 7).any()
    assert q.dtype == torch.int8 and q.shape == x.shape
    assert np.array_equal(q.cpu().numpy().reshape(-1, 2), want)


def _case(antq_lib, dev, book, dt, M, N, K, per_row, with_bias, seed, lo=None, or_mask=0, plant=False):
    """random codes (every byte is a defined code of these books; or_mask: bits set in every byte past the first 8) and random xq in -I_x .. I_x
    (lo: in lo .. I_x); plant: the book's first entry (int4: -8) and -I_x meet at [0, 0]"""
    import torch
    grid, gmax, n_normal, ovp = _book(book)
    plan = antq_lib.plan_for(grid)
    I, image = plan.integer_image()
    gen = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 256, (N, K // 2), device=dev, generator=gen, dtype=torch.uint8)
    codes[:, 8:] |= or_mask
    xq = torch.randint(-I if lo is None else lo, I + 1, (M, K), device=dev, generator=gen, dtype=torch.int8)
    if plant:
        xq[0, 0], codes[0, 0] = -I, 0
    aw = (torch.rand(N if per_row else 1, device=dev, generator=gen) + 0.5).float()
    ax = (torch.rand(1, device=dev, generator=gen) + 0.5).float()
    bias = torch.randn(N, device=dev, generator=gen).to(dt) if with_bias else None
    call = lambda xq_, out=None: antq_lib.int_linear4(codes, xq_, aw, plan.image_dev(dev), I, ax, I, N, K, per_row, dt, bias=bias,
                                                      n_normal=n_normal, ovp=ovp, out=out)
    v = _v_of_codes(codes.cpu().numpy(), image, n_normal, ovp)
    ref = lambda xq_: _reference(xq_.cpu().numpy(), v, np.broadcast_to(aw.cpu().numpy(), (N,)), I, float(ax), I,
                                 None if bias is None else bias.float().cpu().numpy(), dt)
    return xq, codes, call, ref


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("book", ["ant_flint4_s", "olive_int4", "ant_int4_s"])
def test_int_linear4_bit_for_bit(antq_lib, dev, book, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    for seed, (M, N, K, per_row, with_bias) in enumerate(itertools.product((1, 17, 129), (1, 63, 65), (32, 160, 384), (True, False), (True, False))):
        xq, codes, call, ref = _case(antq_lib, dev, book, dt, M, N, K, per_row, with_bias, seed, plant=book == "ant_int4_s")   # (-8 on both operands)
        assert np.array_equal(_bits(call(xq)), ref(xq)[1]), (M, N, K, per_row, with_bias)
    # (the last case: M = 129, N = 65, K = 384) a row computed alone has the bits it has inside the call; so has the 256-row tile
    y = _bits(call(xq))
    for row in (0, 64, 128):
        assert np.array_equal(_bits(call(xq[row:row + 1].clone()))[0], y[row])
    antq_lib.lib().antq_debug_set(23, 4)
    try:
        assert np.array_equal(_bits(call(xq)), y)
    finally:
        antq_lib.lib().antq_debug_set(23, 0)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_int_linear4_rounds_a_sum_beyond_2_24(antq_lib, dev, dtype_name):
    import torch
    xq, codes, call, ref = _case(antq_lib, dev, "ant_pot4_s", getattr(torch, dtype_name), 16, 16, 8192, True, True, 5, lo=48, or_mask=0xEE)       # xq in 48 .. 64, weights 32 or 64 but for 16 k
    S, want = ref(xq)
    assert np.abs(S).max() > 2 ** 24 and (S.astype(np.float32).astype(np.int64) != S).any()
    assert np.array_equal(_bits(call(xq)), want)


@pytest.mark.parametrize("what", ["k_not_32", "sum_overflow", "misaligned_xq"])
def test_int_linear4_refusals_leave_the_output_alone(antq_lib, dev, what):
    import torch
    grid, gmax, n_normal, ovp = _book("ant_flint4_s")
    plan = antq_lib.plan_for(grid)
    M, N, K, I_x, code = {"k_not_32": (2, 4, 48, 16, -2), "sum_overflow": (1, 1, 133152, 127, -2), "misaligned_xq": (2, 4, 64, 16, -5)}[what]
    assert what != "sum_overflow" or (I_x * I_x * K >= 2 ** 31 > I_x * I_x * (K - 32) and K % 32 == 0)
    codes = torch.zeros(N * K // 2, dtype=torch.uint8, device=dev)
    xq = torch.ones(M * K + 16, dtype=torch.int8, device=dev)[1 if what == "misaligned_xq" else 0:][:M * K].view(M, K)
    one = torch.ones(1, device=dev)
    out = torch.full((M, N), 7.0, device=dev)
    with pytest.raises(antq_lib.AntqError, match=r"\(%d\)" % code):
        antq_lib.int_linear4(codes, xq, one, plan.image_dev(dev), I_x, one, I_x, N, K, False, torch.float32, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _two_linears(tree, mode, dev, dt):
    import torch
    import torch.nn as nn
    qmod, qutil = _trees(tree)
    qutil.set_quantizer(_args(mode=mode, wbit=4, abit=4))
    torch.manual_seed(2)
    model = qmod.quantize_model(nn.Sequential(nn.Linear(64, 96), nn.ReLU(), nn.Linear(96, 64))).to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    x = torch.randn(33, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dt)
    with torch.no_grad():
        model(x)                                                           # calibration
    return model, qutil, x


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_packed_model_runs_the_integer_path(antq_lib, dev, dtype_name):
    import torch
    from ant_quantization_amd import packed
    dt = getattr(torch, dtype_name)
    base, qutil, x = _two_linears("ant", "ant-int-flint", dev, dt)
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    tbank = qutil.pack_model(twin, fused_linear=True)
    bank = qutil.pack_model(model, fused_linear=True, integer_linear=True)
    assert bank.integer_skipped == [] and all(e["integer"] for e in bank.entries.values())
    seen = {}
    hooks = [model.get_submodule(n).register_forward_hook(lambda m, i, o, n=n: seen.__setitem__(n, (i[0].detach(), o.detach()))) for n in ("0", "2")]
    with torch.no_grad():
        y = model(x)
    [h.remove() for h in hooks]
    assert bank.int_linear_calls == 2 and tbank.int_linear_calls == 0
    for n in ("0", "2"):
        mod, (xin, yout) = model.get_submodule(n), seen[n]
        e, qi = bank.entries[id(mod.quant_weight)], mod.quant_input
        (plan_w, gmax_w, nn_w, ovp_w), (plan_x, gmax_x, nn_x, ovp_x) = packed._codebook(mod.quant_weight), packed._codebook(qi)
        # the two library calls, on the layer's own input
        xq = antq_lib.quant_i8(xin, qi.alpha.detach().float().reshape(1), plan_x, gmax_x, 1, xin.numel(), False, plan_x.image_dev(dev))
        direct = antq_lib.int_linear4(e["codes"], xq, packed._unit_alpha(e["alpha"], plan_w, gmax_w), plan_w.image_dev(dev),
                                      plan_w.integer_image()[0], packed._unit_alpha(qi.alpha, plan_x, gmax_x), plan_x.integer_image()[0],
                                      e["shape"][0], e["shape"][1], e["per_row"], dt, bias=mod.bias.detach())
        assert np.array_equal(_bits(direct), _bits(yout)), n
        if dtype_name == "float32":
            # against the float64 product of the fake-quant images: at most 4 roundings per image factor (scale, value times
            # scale, on both operands) against 1 on the integer side, plus 3 in the epilogue -> 16 * 2^-24 covers it
            tmod = twin.get_submodule(n)
            with torch.no_grad():
                x64 = tmod.quant_input(xin, tmod.weight).double().cpu().numpy()
            W = tbank.entries[id(tmod.quant_weight)]["out"].double().cpu().numpy()
            b = mod.bias.detach().double().cpu().numpy()
            err = np.abs(yout.double().cpu().numpy() - (x64 @ W.T + b))
            assert (err <= 16 * 2.0 ** -24 * (np.abs(x64) @ np.abs(W).T + np.abs(b))).all(), (n, err.max())
    with torch.no_grad():
        assert np.array_equal(_bits(model.get_submodule("2")(torch.relu(seen["0"][1]))), _bits(y)) and bank.int_linear_calls == 3
    # a call that wants a gradient through the input takes today's path, with today's bits
    for p in itertools.chain(model.parameters(), twin.parameters()):
        p.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    assert np.array_equal(_bits(model(xg)), _bits(twin(xg))) and bank.int_linear_calls == 3


def test_a_book_without_an_image_keeps_todays_bits(antq_lib, dev):
    import torch
    base, qutil, x = _two_linears("olive", "ant-flint", dev, torch.bfloat16)
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    qutil.pack_model(twin, fused_linear=True)
    bank = qutil.pack_model(model, fused_linear=True, integer_linear=True)
    assert [n for n, _ in bank.integer_skipped] == ["0", "2"] and all("integer image" in why for _, why in bank.integer_skipped)
    with torch.no_grad():
        assert np.array_equal(_bits(model(x)), _bits(twin(x))) and bank.int_linear_calls == 0
