"""The integer-domain byte-code linear on the GPU: antq_linear8_i8 and antq_linear8_i8_sk bit for bit against the formula of
include/antq.h (test_gpu_int_linear4._reference: S in int64, the epilogue in np.float32, one rounding to the dtype) for the XOR
book and two TABLE books, a sum near the top of int32, antq_quant_i8 on the int8 book, the refusals, and the module surface
(pack_model(integer_bytes=True))."""
import copy
import ctypes
import functools
import itertools

import numpy as np
import pytest

from test_gpu_int_linear4 import _bits, _reference
from test_gpu_linear8 import _args, _trees

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")
BOOKS = {"int8": ("int", 8), "int6": ("int", 6), "flint5": ("flint", 5)}      # XOR (I = 128); TABLE, m = 64; TABLE, not monotone
# one partial stage, a 32-k tail, the double buffer's third stage, the row and column tile edges, the 64 / 65 tile switch
TILED = [(1, 1, 32), (17, 65, 160), (64, 63, 384), (65, 64, 128), (129, 130, 416), (257, 64, 256)]
SPLIT = list(itertools.product((1, 16, 17, 64), ((65, 160), (64, 1024))))


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def knob(antq_lib):
    """knob(key, value): antq_debug_set for this test (23: the tile, 24: the slices)"""
    yield antq_lib.lib().antq_debug_set
    antq_lib.lib().antq_debug_set(23, 0)
    antq_lib.lib().antq_debug_set(24, 0)


def _plan(antq_lib, book):
    from ant_quantization_amd import grids
    plan = antq_lib.plan_for(grids.ant_grid(BOOKS[book][0], BOOKS[book][1], True))
    I, image = plan.integer_image8()
    assert (I, image.size) == {"int8": (128, 256), "int6": (32, 64), "flint5": (64, 32)}[book]
    return plan, I, image


def _case(antq_lib, dev, book, dt, M, N, K, per_row, with_bias, seed, fill=None):
    """random codes -- int6: the whole byte range, so codes >= m are planted and must read 0 -- and random xq in -I .. min(I, 127)
    (fill: (xq value, code) everywhere).  Returns (xq, call(fn, **kw), reference bits on the device)."""
    import torch
    plan, I, image = _plan(antq_lib, book)
    gen = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 256 if book == "int6" else image.size, (N, K), device=dev, generator=gen, dtype=torch.uint8)
    xq = torch.randint(-I, min(I, 127) + 1, (M, K), device=dev, generator=gen, dtype=torch.int8)
    if fill is not None:
        xq.fill_(fill[0]), codes.fill_(fill[1])
    aw = (torch.rand(N if per_row else 1, device=dev, generator=gen) + 0.5).float()
    ax = (torch.rand(1, device=dev, generator=gen) + 0.5).float()
    bias = torch.randn(N, device=dev, generator=gen).to(dt) if with_bias else None
    call = lambda fn=antq_lib.int_linear8, **kw: fn(codes, xq, aw, plan.image_dev(dev, 128), image, I, ax, I, N, K, per_row, dt, bias=bias, **kw)
    g = np.zeros(256, dtype=np.int64)
    g[:image.size] = image
    S, want = _reference(xq.cpu().numpy(), g[codes.cpu().numpy()], np.broadcast_to(aw.cpu().numpy(), (N,)), I, float(ax), I,
                         None if bias is None else bias.float().cpu().numpy(), dt)
    return xq, call, torch.from_numpy(want).to(dev), S


def _raw(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("book", BOOKS)
def test_tiled_bit_for_bit(antq_lib, dev, knob, book, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    for seed, ((M, N, K), per_row, with_bias) in enumerate(itertools.product(TILED, (True, False), (True, False))):
        xq, call, want, _ = _case(antq_lib, dev, book, dt, M, N, K, per_row, with_bias, seed)
        assert torch.equal(_raw(call()), want), (M, N, K, per_row, with_bias)
        if (M, N, K) == (129, 130, 416):                  # both forced tiles: the sum is exact, the bits are the same
            for waves in (2, 4):
                knob(23, waves)
                assert torch.equal(_raw(call()), want), waves
            knob(23, 0)


@functools.lru_cache(maxsize=None)
def _split_cases(book, dtype_name):
    """the split-K cases of one (book, dtype) with their reference bits: computed once, shared by every S"""
    import torch
    from ant_quantization_amd import _lib
    return [_case(_lib, torch.device("cuda:0"), book, getattr(torch, dtype_name), M, N, K, seed % 2 == 0, seed % 3 != 0, seed)
            for seed, (M, (N, K)) in enumerate(SPLIT)]


@pytest.mark.parametrize("S", [0, 1, 2, 3, 16])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("book", BOOKS)
def test_split_k_bit_for_bit_whatever_the_split(antq_lib, dev, knob, book, dtype_name, S):
    import torch
    knob(24, S)
    for (M, (N, K)), (xq, call, want, _) in zip(SPLIT, _split_cases(book, dtype_name)):
        need = antq_lib.int_linear8_sk_workspace_bytes(M, N, K)
        slices = antq_lib.lib().antq_linear8_i8_sk_slices(M, N, K, 0)
        assert need == (0 if slices == 1 else (4 * slices * M * N + 15) // 16 * 16) and (S == 0 or slices == min(S, -(-K // 128)))
        buf = torch.full((need + 256,), 0x5a, dtype=torch.uint8, device=dev)      # a poisoned band behind the stated size
        assert torch.equal(_raw(call(antq_lib.int_linear8_sk, workspace=buf[:need])), want), (M, N, K)
        assert bool((buf[need:] == 0x5a).all()), (M, N, K)
    assert torch.equal(_raw(call()), want)                # (the last case) the tiled entry's bits


def test_a_sum_near_the_top_of_int32(antq_lib, dev):
    import torch
    xq, call, want, S = _case(antq_lib, dev, "int8", torch.float32, 1, 2, 131040, True, True, 7, fill=(-128, 0))
    assert (S == 2146959360).all() and 2146959360 < 2 ** 31
    assert torch.equal(_raw(call()), want) and torch.equal(_raw(call(antq_lib.int_linear8_sk)), want)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_quant_i8_on_the_int8_book(antq_lib, dev, dtype_name):
    import torch
    plan, I, image = _plan(antq_lib, "int8")
    gmax = float(plan.grid.max())
    x = torch.randn(3, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 0.5
    x[1, 5], x[1, 6] = -100.0, 100.0                      # far beyond the clip: -128 and 127
    x = x.to(getattr(torch, dtype_name))
    alpha = torch.tensor([1.0, 0.7, 1.3], device=dev)
    codes = antq_lib.encode8(x, alpha, plan, gmax, 3, 64, True).cpu().numpy().astype(np.int64)
    q = antq_lib.quant_i8(x, alpha, plan, gmax, 3, 64, True, plan.image_dev(dev, 128)).cpu().numpy()
    assert q.dtype == np.int8 and q.min() == -128 and q.max() == 127
    assert np.array_equal(q.reshape(-1), image[codes.reshape(-1)])


@pytest.mark.parametrize("what, code", [("k_not_32", -2), ("i_129", -2), ("sum_overflow", -2), ("ovp", -2), ("misaligned_xq", -5),
                                        ("small_workspace", -1)])
def test_refusals_leave_the_output_alone(antq_lib, dev, knob, what, code):
    import torch
    plan, I, image = _plan(antq_lib, "int8")
    M, N, K = {"k_not_32": (2, 4, 48), "sum_overflow": (1, 1, 131072)}.get(what, (2, 64, 512))
    I_x = 129 if what == "i_129" else 128
    codes = torch.zeros(N * K, dtype=torch.uint8, device=dev)
    xq = torch.ones(M * K + 16, dtype=torch.int8, device=dev)[1 if what == "misaligned_xq" else 0:][:M * K]
    one, out = torch.ones(1, device=dev), torch.full((M, N), 7.0, device=dev)
    ws = torch.zeros(4 * 4 * M * N, dtype=torch.uint8, device=dev)
    if what == "small_workspace":
        knob(24, 4)
        assert antq_lib.int_linear8_sk_workspace_bytes(M, N, K) == ws.numel()
    L, vp = antq_lib.lib(), ctypes.c_void_p
    head = (codes.data_ptr(), xq.data_ptr(), None, out.data_ptr(), M, N, K, one.data_ptr(), 0, 128, image.ctypes.data,
            plan.image_dev(dev, 128).data_ptr(), 256, one.data_ptr(), I_x)
    tail = (1 if what == "ovp" else 0, 0, None)
    assert L.antq_linear8_i8_sk(*head, ws.data_ptr(), ws.numel() - (1 if what == "small_workspace" else 0), *tail) == code
    if what != "small_workspace":
        assert L.antq_linear8_i8(*head, *tail) == code
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())


def _mlp(act, dev, dt):
    """Linear - act - Linear of ANT `int` quantisers, both (weight, input) pairs raised to 8 bit, calibrated"""
    import torch
    import torch.nn as nn
    qmod, qutil = _trees("ant")
    qutil.set_quantizer(_args(mode="ant-int", wbit=4, abit=4))
    torch.manual_seed(2)
    model = qmod.quantize_model(nn.Sequential(nn.Linear(64, 96), act, nn.Linear(96, 64)))
    qmod.set_8_bit_layer_l(model, "0,1")
    model = model.to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    x = torch.randn(33, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dt)
    with torch.no_grad():
        model(x)                                                           # calibration
    return model, qutil, x


OPTS = dict(byte_codes=True, fused_linear=True, fused_bytes=True, integer_linear=True, integer_bytes=True)


@pytest.mark.parametrize("split_k", [False, True])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_packed_model_runs_the_byte_integer_path(antq_lib, dev, dtype_name, split_k):
    import torch
    import torch.nn as nn
    from ant_quantization_amd import packed
    dt = getattr(torch, dtype_name)
    base, qutil, x = _mlp(nn.Tanh(), dev, dt)
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    tbank = qutil.pack_model(twin, byte_codes=True, fused_linear=True)
    bank = qutil.pack_model(model, integer_split_k=split_k, **OPTS)
    assert bank.integer_skipped == [] and [e["width"] for e in bank.entries.values()] == [8, 8] and all(e["integer"] == 128 for e in bank.entries.values())
    seen = {}
    hooks = [model.get_submodule(n).register_forward_hook(lambda m, i, o, n=n: seen.__setitem__(n, (i[0].detach(), o.detach()))) for n in ("0", "2")]
    with torch.no_grad():
        y = model(x)
    [h.remove() for h in hooks]
    sk = 2 if split_k else 0
    assert (bank.int_linear_calls, bank.int_linear_byte_calls, bank.int_linear_sk_calls, bank.int_linear_byte_sk_calls) == (2, 2, sk, sk)
    assert tbank.int_linear_calls == 0 and torch.equal(seen["2"][1], y)
    for n in ("0", "2"):
        mod, (xin, yout) = model.get_submodule(n), seen[n]
        e, qi = bank.entries[id(mod.quant_weight)], mod.quant_input
        (plan_w, gmax_w, _, _), (plan_x, gmax_x, _, _) = packed._codebook(mod.quant_weight), packed._codebook(qi)
        assert plan_x.integer_image8()[0] == 128           # an 8-bit signed int activation quantiser
        # the two library calls, on the layer's own input
        xq = antq_lib.quant_i8(xin, qi.alpha.detach().float().reshape(1), plan_x, gmax_x, 1, xin.numel(), False, plan_x.image_dev(dev, 128))
        direct = antq_lib.int_linear8(e["codes"], xq, packed._unit_alpha(e["alpha"], plan_w, gmax_w), plan_w.image_dev(dev, 128),
                                      plan_w.integer_image8()[1], 128, packed._unit_alpha(qi.alpha, plan_x, gmax_x), 128,
                                      e["shape"][0], e["shape"][1], e["per_row"], dt, bias=mod.bias.detach())
        assert np.array_equal(_bits(direct), _bits(yout)), n
        if dtype_name == "float32":
            # test_gpu_int_linear4's bound against the float64 product of the fake-quant images: 16 * 2^-24 (sum |x_q w_q| + |bias|)
            tmod = twin.get_submodule(n)
            with torch.no_grad():
                x64 = tmod.quant_input(xin, tmod.weight).double().cpu().numpy()
            W = tbank.entries[id(tmod.quant_weight)]["out"].double().cpu().numpy()
            b = mod.bias.detach().double().cpu().numpy()
            err = np.abs(yout.double().cpu().numpy() - (x64 @ W.T + b))
            assert (err <= 16 * 2.0 ** -24 * (np.abs(x64) @ np.abs(W).T + np.abs(b))).all(), (n, err.max())


def test_an_unsigned_8_bit_input_keeps_todays_bits(antq_lib, dev):
    import torch
    import torch.nn as nn
    base, qutil, x = _mlp(nn.ReLU(), dev, torch.bfloat16)
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    without = dict(OPTS, integer_bytes=False)
    qutil.pack_model(twin, **without)
    bank = qutil.pack_model(model, **OPTS)
    assert [n for n, _ in bank.integer_skipped] == ["2"] and "input" in bank.integer_skipped[0][1]
    with torch.no_grad():
        h = model.get_submodule("0")(x)
        assert bank.int_linear_byte_calls == 1
        assert np.array_equal(_bits(model.get_submodule("2")(h)), _bits(twin.get_submodule("2")(h))) and bank.int_linear_calls == 1


def test_capture_and_replay(antq_lib, dev):
    import torch
    import torch.nn as nn
    model, qutil, x = _mlp(nn.Tanh(), dev, torch.bfloat16)
    bank = qutil.pack_model(model, integer_split_k=True, **OPTS)
    with torch.no_grad():
        want = [_bits(model(torch.roll(x, s, dims=1).contiguous())) for s in (1, 5)]      # eager (code objects loaded before the capture)
        xs = x.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(xs)
        for s, w in zip((1, 5), want):
            xs.copy_(torch.roll(x, s, dims=1))
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out), w), s
    assert bank.int_linear_byte_sk_calls == 6
