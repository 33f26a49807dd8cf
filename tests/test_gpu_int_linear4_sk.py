"""The split-K integer-domain linear (antq_linear4_i8_sk, 1 .. 64 rows) on the GPU: bit for bit against the formula of
include/antq.h (test_gpu_int_linear4._reference: S in int64, the epilogue in np.float32) for every forced number of slices,
a sum beyond 2^24 across slices, the workspace's footprint, the refusals, capture, and pack_model(integer_split_k=True)."""
import copy
import functools
import itertools

import numpy as np
import pytest

from test_gpu_int_linear4 import _bits, _book, _reference, _two_linears, _v_of_codes

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")
SHAPES = list(itertools.product((1, 16, 17, 64), (1, 63, 65), (32, 160, 384, 1056), (True, False), (True, False)))


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def split(antq_lib):
    """force(S): antq_debug_set key 24 for this test"""
    yield lambda S: antq_lib.lib().antq_debug_set(24, S)
    antq_lib.lib().antq_debug_set(24, 0)


def _case(antq_lib, dev, book, dt, M, N, K, per_row, with_bias, seed, lo=None, or_mask=0, plant=False):
    """test_gpu_int_linear4._case's inputs; returns (xq, call(xq, fn, **kw), ref(xq) -> (S, bits))"""
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
    call = lambda xq_, fn=antq_lib.int_linear4_sk, **kw: fn(codes, xq_, aw, plan.image_dev(dev), I, ax, I, N, K, per_row, dt, bias=bias,
                                                            n_normal=n_normal, ovp=ovp, **kw)
    v = _v_of_codes(codes.cpu().numpy(), image, n_normal, ovp)
    ref = lambda xq_: _reference(xq_.cpu().numpy(), v, np.broadcast_to(aw.cpu().numpy(), (N,)), I, float(ax), I,
                                 None if bias is None else bias.float().cpu().numpy(), dt)
    return xq, call, ref


@functools.lru_cache(maxsize=None)
def _cases(book, dtype_name):
    """the cases of one (book, dtype) with their reference bits on the device: computed once, shared by every S"""
    import torch
    from ant_quantization_amd import _lib
    dev, dt, out = torch.device("cuda:0"), getattr(torch, dtype_name), []
    for seed, (M, N, K, per_row, with_bias) in enumerate(SHAPES):
        xq, call, ref = _case(_lib, dev, book, dt, M, N, K, per_row, with_bias, seed, plant=book == "ant_int4_s")      # (-8 on both operands)
        out.append((xq, call, torch.from_numpy(ref(xq)[1]).to(dev)))
    return out


def _raw(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("S", [0, 1, 2, 3, 16])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("book", ["ant_flint4_s", "olive_int4", "ant_int4_s"])
def test_bit_for_bit_whatever_the_split(antq_lib, dev, split, book, dtype_name, S):
    import torch
    ws = torch.empty(16 * 4 * 64 * 65 + 16, dtype=torch.uint8, device=dev)
    split(S)
    for shape, (xq, call, want) in zip(SHAPES, _cases(book, dtype_name)):
        ws.fill_(0x7f)
        assert torch.equal(_raw(call(xq, workspace=ws)), want), shape
    assert torch.equal(_raw(call(xq, antq_lib.int_linear4)), want)             # (the largest case) the bits of antq_linear4_i8


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_partials_beyond_2_24_are_added_as_integers(antq_lib, dev, split, dtype_name):
    import torch
    xq, call, ref = _case(antq_lib, dev, "ant_pot4_s", getattr(torch, dtype_name), 16, 16, 8192, True, True, 5, lo=48, or_mask=0xEE)
    S, want = ref(xq)
    assert np.abs(S).max() > 2 ** 24 and (S.astype(np.float32).astype(np.int64) != S).any()
    split(16)
    assert antq_lib.int_linear4_sk_workspace_bytes(16, 16, 8192) == 16 * 4 * 16 * 16
    assert np.array_equal(_bits(call(xq)), want)


def test_workspace_footprint(antq_lib, dev, split):
    import torch
    xq, call, ref = _case(antq_lib, dev, "olive_int4", torch.float32, 17, 63, 1056, True, True, 9)
    split(4)
    need = antq_lib.int_linear4_sk_workspace_bytes(17, 63, 1056)
    assert need == (3 * 4 * 17 * 63 + 15) // 16 * 16                          # 9 stages over 4 slices: 3 slices of 3 stages
    buf = torch.full((need + 4096,), 0x5a, dtype=torch.uint8, device=dev)
    assert np.array_equal(_bits(call(xq, workspace=buf[:need])), ref(xq)[1])
    assert bool((buf[need:] == 0x5a).all())


@pytest.mark.parametrize("what, code", [("rows", -2), ("short", -1), ("misaligned", -5)])
def test_refusals_leave_the_output_alone(antq_lib, dev, split, what, code):
    import torch
    M = 65 if what == "rows" else 8
    xq, call, _ = _case(antq_lib, dev, "ant_flint4_s", torch.float32, M, 64, 512, True, False, 1)
    split(4)
    need = antq_lib.int_linear4_sk_workspace_bytes(8, 64, 512)
    assert need == 4 * 4 * 8 * 64
    buf = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    ws = {"rows": buf, "short": buf[:need - 1], "misaligned": buf[4:]}[what]
    out = torch.full((M, 64), 7.0, device=dev)
    with pytest.raises(antq_lib.AntqError, match=r"\(%d\)" % code):
        call(xq, workspace=ws, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 0).all())


def test_capture_and_replay(antq_lib, dev, split):
    import torch
    xq, call, ref = _case(antq_lib, dev, "ant_flint4_s", torch.bfloat16, 17, 65, 1056, True, True, 4)
    split(4)
    ws = torch.empty(antq_lib.int_linear4_sk_workspace_bytes(17, 65, 1056), dtype=torch.uint8, device=dev)
    out = torch.empty(17, 65, dtype=torch.bfloat16, device=dev)
    call(xq, workspace=ws, out=out)                                            # (code objects loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(xq, workspace=ws, out=out)
    for shift in (1, 5):
        xq.copy_(torch.roll(xq, shift, dims=1).contiguous())
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), ref(xq)[1]), shift


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_packed_model_splits_its_small_calls(antq_lib, dev, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    base, qutil, x = _two_linears("ant", "ant-int-flint", dev, dt)
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    tbank = qutil.pack_model(twin, fused_linear=True, integer_linear=True)
    bank = qutil.pack_model(model, fused_linear=True, integer_linear=True, integer_split_k=True)
    with torch.no_grad():
        assert np.array_equal(_bits(model(x)), _bits(twin(x)))
        assert (bank.int_linear_sk_calls, bank.int_linear_calls, tbank.int_linear_sk_calls, tbank.int_linear_calls) == (2, 2, 0, 2)
        x65 = torch.cat([x, x])[:65].contiguous()
        assert np.array_equal(_bits(model(x65)), _bits(twin(x65)))
        assert (bank.int_linear_sk_calls, bank.int_linear_calls) == (2, 4)
