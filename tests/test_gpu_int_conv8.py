"""antq_conv2d8_i8 / antq_conv2d8_i8_sk on the GPU, bit for bit against the formula of include/antq.h (S from a float64 F.conv2d of
X = xq + x_offset and v, exact below 2^31; the epilogue step by step in np.float32): both offsets, tiles, slices, refusals, a packed CNN."""
import copy
import functools

import numpy as np
import pytest

from test_gpu_int_conv4 import GEOMETRIES, dev  # noqa: F401 (dev: the fixture)
from test_gpu_int_linear4 import _bits
from test_gpu_int_linear8 import _plan, knob  # noqa: F401 (knob: the fixture)
from test_gpu_linear8 import _args, _trees

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")
SPLIT = [c for c, (C, (R, S), st, pad, dil, (H, W), B, N) in enumerate(GEOMETRIES) if R * S * C >= 256]       # (all have M <= 1024)


@functools.lru_cache(maxsize=None)
def _case(case, dtype_name, x_offset):
    """One geometry's operands and, for (per row + bias) and (per tensor, no bias), (call(fn, **kw), reference bits); M, N, K."""
    import torch
    import torch.nn.functional as F
    from ant_quantization_amd import _lib, grids
    dev, dt = torch.device("cuda:0"), getattr(torch, dtype_name)
    C, (R, S), stride, padding, dilation, (H, W), B, N = GEOMETRIES[case]
    K = R * S * C
    # ANT's signed int8 book (XOR) on the even cases, the 6-bit table book with codes >= m drawn on the odd ones
    plan_w, I_w, image_w = _plan(_lib, "int8" if case % 2 == 0 else "int6")
    plan_x = _lib.plan_for(grids.ant_grid("int", 8, x_offset == 0))
    I_x, image_x = plan_x.offset_image() if x_offset else plan_x.integer_image8()
    assert I_x == (255 if x_offset else 128)
    gen = torch.Generator(device=dev).manual_seed(case)
    ax = (torch.rand(1, device=dev, generator=gen) + 0.5).float()
    if x_offset:                           # [0, 1.2 alpha]: both ends of the byte range occur
        x = torch.rand(B, C, H, W, device=dev, generator=gen) * 1.2 * ax
        x[0, 0, 0, 0], x[0, 1, 0, 0] = 0.0, 1.2 * ax.item()
    else:                                  # |x| in [0.5, 1] alpha: no byte is 0, so a wrong tap changes S
        x = (torch.rand(B, C, H, W, device=dev, generator=gen) * 0.5 + 0.5) * ax
        x = x * (torch.randint(0, 2, x.shape, device=dev, generator=gen) * 2 - 1)
    x = x.to(dt).contiguous(memory_format=torch.channels_last)
    xq = _lib.quant_i8(x.permute(0, 2, 3, 1), ax, plan_x, float(plan_x.grid.max()), 1, x.numel(), False,
                       plan_x.image_dev(dev, "offset" if x_offset else 128))
    assert (int(xq.min()) == -128 and int(xq.max()) == 127) if x_offset else bool((xq != 0).all())
    codes = torch.randint(0, 256, (N, K), device=dev, generator=gen, dtype=torch.uint8)
    g = np.zeros(256, dtype=np.int64)
    g[:image_w.size] = image_w
    v = g[codes.cpu().numpy()]
    wsum = torch.from_numpy(v.sum(axis=1).astype(np.int32)).to(dev)
    X = xq.permute(0, 3, 1, 2).double().cpu() + x_offset
    S64 = F.conv2d(X, torch.from_numpy(v.reshape(N, R, S, C).transpose(0, 3, 1, 2).astype(np.float64)), None, stride, padding, dilation)
    assert float(S64.abs().max()) < 2 ** 31
    S32 = S64.permute(0, 2, 3, 1).numpy().astype(np.float32)
    variants = []
    for per_row, with_bias in ((True, True), (False, False)):
        aw = (torch.rand(N if per_row else 1, device=dev, generator=gen) + 0.5).float()
        bias = torch.randn(N, device=dev, generator=gen).to(dt) if with_bias else None
        y = S32 * (np.float32(ax.item()) / np.float32(I_x))
        y = y * (np.broadcast_to(aw.cpu().numpy(), (N,)) / np.float32(I_w))
        if with_bias:
            y = y + bias.float().cpu().numpy()
        call = (lambda fn=_lib.int_conv2d8, aw=aw, bias=bias, per_row=per_row, **kw:
                fn(codes, xq, aw, plan_w.image_dev(dev, 128), image_w, I_w, ax, I_x, N, (R, S), stride, padding, dilation, per_row, dt,
                   bias=bias, x_offset=x_offset, wsum=wsum if x_offset else None, **kw))
        lin = None
        if (R, S) == (1, 1) and not x_offset:
            lin = _lib.int_linear8(codes, xq.view(-1, C), aw, plan_w.image_dev(dev, 128), image_w, I_w, ax, I_x, N, C, per_row, dt, bias=bias)
        variants.append((call, _bits(torch.from_numpy(y.astype(np.float32)).to(dt)), lin))
    return variants, S64.shape[0] * S64.shape[2] * S64.shape[3], N, K


@pytest.mark.parametrize("x_offset", [0, 128])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", range(len(GEOMETRIES)))
def test_int_conv2d8_bit_for_bit(antq_lib, dev, knob, case, dtype_name, x_offset):
    import torch
    for call, want, lin in _case(case, dtype_name, x_offset)[0]:
        out = call()
        assert out.is_contiguous(memory_format=torch.channels_last) and np.array_equal(_bits(out.permute(0, 2, 3, 1)), want)
        if case in (0, 4):
            for waves in (2, 4):
                knob(23, waves)
                assert np.array_equal(_bits(call().permute(0, 2, 3, 1)), want), waves
            knob(23, 0)
        if lin is not None:
            assert np.array_equal(_bits(lin).reshape(want.shape), want)


@pytest.mark.parametrize("slices", [1, 2, 16])
@pytest.mark.parametrize("x_offset", [0, 128])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_split_k_gives_the_same_bits_whatever_the_slices(antq_lib, dev, knob, dtype_name, x_offset, slices):
    import torch
    knob(24, slices)
    for case in SPLIT:
        variants, M, N, K = _case(case, dtype_name, x_offset)
        got = antq_lib.int_conv2d8_sk_slices(M, N, K)
        need = antq_lib.int_conv2d8_sk_workspace_bytes(M, N, K)
        assert got == min(slices, -(-K // 128)) and need == (0 if got == 1 else (4 * got * M * N + 15) // 16 * 16)
        buf = torch.full((256 + need + 256,), 0x5a, dtype=torch.uint8, device=dev)        # garbage inside, sentinels around
        for call, want, _ in variants:
            out = call(antq_lib.int_conv2d8_sk, workspace=buf[256:256 + need])
            assert np.array_equal(_bits(out.permute(0, 2, 3, 1)), want), case
        assert bool((buf[:256] == 0x5a).all()) and bool((buf[256 + need:] == 0x5a).all()), case


@pytest.mark.parametrize("what, code", [("c_48", -2), ("ovp", -2), ("m_257", -2), ("bad_offset", -1), ("null_wsum", -1), ("sum_offset_0", -2),
                                        ("sum_offset_128", -2), ("misaligned_xq", -5), ("misaligned_wsum", -5)])
def test_refusals_leave_the_output_alone(antq_lib, dev, what, code):
    import torch
    plan, _, image = _plan(antq_lib, "int8")
    # both sum bounds at their first refused K = C (H = W = R = S = 1), with K - 32 accepted
    C, I_x, off = {"c_48": (48, 128, 0), "sum_offset_0": (131072, 128, 0), "sum_offset_128": (65536, 255, 128)}.get(what, (64, 128, 128))
    if what == "bad_offset":
        off = 64
    HW = 1 if what.startswith("sum") else 4
    codes = torch.zeros(4 * C, dtype=torch.uint8, device=dev)
    xq = torch.ones(HW * HW * C + 16, dtype=torch.int8, device=dev)[1 if what == "misaligned_xq" else 0:][:HW * HW * C]
    wsum = torch.zeros(8, dtype=torch.int32, device=dev)
    wptr = None if what == "null_wsum" else wsum.data_ptr() + (2 if what == "misaligned_wsum" else 0)
    one, out = torch.ones(1, device=dev), torch.full((HW * HW * 4,), 7.0, device=dev)
    ws = torch.zeros(4 * 16 * HW * HW * 4, dtype=torch.uint8, device=dev)

    def both(C):
        head = (codes.data_ptr(), xq.data_ptr(), None, out.data_ptr(), 1, HW, HW, C, 4, 1, 1, 1, 1, 0, 0, 1, 1, one.data_ptr(), 0, 128,
                image.ctypes.data, plan.image_dev(dev, 128).data_ptr(), 257 if what == "m_257" else 256, one.data_ptr(), I_x, off, wptr)
        tail = (antq_lib.FLAG_OVP if what == "ovp" else 0, antq_lib.F32, None)
        L = antq_lib.lib()
        return L.antq_conv2d8_i8(*head, *tail), L.antq_conv2d8_i8_sk(*head, ws.data_ptr(), ws.numel(), *tail)

    assert both(C) == (code, code)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())
    if what.startswith("sum"):
        assert both(C - 32) == (0, 0)


@pytest.mark.parametrize("split_k", [False, True])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_packed_cnn_runs_the_byte_integer_convs(antq_lib, dev, dtype_name, split_k):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    dt = getattr(torch, dtype_name)
    qmod, qutil = _trees("ant")
    qutil.set_quantizer(_args(mode="ant-int-flint", wbit=4, abit=4))
    torch.manual_seed(4)
    net = nn.Sequential(nn.Conv2d(3, 32, 3), nn.ReLU(), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 1),
                        nn.Conv2d(64, 32, 3, stride=2, padding=1))
    base = qmod.quantize_model(net)
    qmod.set_8_bit_layer_l(base, "1,2,3")                                  # every conv after the first: both quantisers to 8 bit
    base = base.to(dev).to(dt).eval()
    qutil.enable_quantization(base)
    x = torch.randn(2, 3, 12, 12, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dt)
    with torch.no_grad():
        base(x)                                                            # calibration
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    opts = dict(byte_codes=True, fused_linear=True, fused_bytes=True, integer_linear=True, integer_bytes=True, integer_conv=True,
                integer_conv_split_k=split_k)
    tbank = qutil.pack_model(twin, **opts)
    bank = qutil.pack_model(model, integer_conv_bytes=True, **opts)
    assert [n for n, _ in bank.integer_skipped] == ["0"] and "C = 3" in bank.integer_skipped[0][1]
    assert [n for n, _ in tbank.integer_skipped] == ["0", "2", "4", "5"]
    seen = {}
    hooks = [model.get_submodule(n).register_forward_hook(lambda m, i, o, n=n: seen.__setitem__(n, (i[0].detach(), o.detach()))) for n in ("2", "5")]
    with torch.no_grad():
        y, today, plain = model(x), twin(x), base(x)
    [h.remove() for h in hooks]
    sk = 3                                 # (the measured rule: M <= 1024 takes the split-K entry with or without the flag)
    assert (bank.int_conv_calls, bank.int_conv_byte_calls, bank.int_conv_sk_calls, bank.int_conv_byte_sk_calls) == (3, 3, sk, sk)
    # the two post-ReLU inputs calibrate unsigned (8-bit: x_offset = 128), the input of "5" has negative values: signed, offset 0
    assert bank.int_conv_offset_calls == 2 and bank.int_conv_relayouts == 1
    assert (tbank.int_conv_calls, tbank.int_conv_byte_calls) == (0, 0)
    assert y.shape == today.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(_bits(today), _bits(plain))                      # without the flag: today's bits
    # "2" (offset 128: wsum and I_x = 255 from the bank) and "5" (offset 0) against the float64 product of the fake-quant images,
    # test_gpu_int_conv4's bound and derivation: at most 4 roundings per image factor, 3 in the epilogue -> 16 * 2^-24
    for n, stride in (("2", 1), ("5", 2)) if dtype_name == "float32" else ():
        (xin, yout), tmod = seen[n], twin.get_submodule(n)
        with torch.no_grad():
            x64 = tmod.quant_input(xin, tmod.weight).double().cpu()
        W64, b64 = tbank.entries[id(tmod.quant_weight)]["out"].double().cpu(), tmod.bias.detach().double().cpu()
        ref = F.conv2d(x64, W64, b64, stride=stride, padding=1)
        mag = F.conv2d(x64.abs(), W64.abs(), b64.abs(), stride=stride, padding=1)
        err = (yout.double().cpu() - ref).abs()
        assert bool((err <= 16 * 2.0 ** -24 * mag).all()), (n, float((err / mag).max()))
