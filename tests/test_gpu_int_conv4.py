"""The integer-domain conv2d on the GPU: antq_conv2d4_i8 bit for bit against the formula of include/antq.h (S from a float64
F.conv2d of the integer-valued operands, exact below 2^31; the epilogue step by step in np.float32), its refusals, and the module
surface (pack_model(integer_conv=True))."""
import copy

import numpy as np
import pytest

from test_gpu_int_linear4 import _bits, _book, _v_of_codes
from test_gpu_linear8 import _args, _trees

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")
# (C, (R, S), stride, padding, dilation, (H, W), B, N)
GEOMETRIES = [(32, (3, 3), 1, 1, 1, (7, 7), 3, 40),          # four taps per stage, K = 288: a partial last stage, a partial n tile, rows crossing images
              (64, (3, 3), 2, 1, 1, (9, 9), 2, 72),          # stride with an odd size, two n tiles
              (160, (1, 3), 1, (0, 1), 1, (5, 6), 2, 64),    # a tap boundary inside a stage, a non-square kernel, asymmetric padding
              (32, (3, 3), 1, 2, 2, (8, 8), 1, 16),          # dilation
              (64, (1, 1), 1, 0, 1, (10, 10), 3, 64),        # M = 300: two m tiles at the largest tile; equals antq_linear4_i8
              (32, (7, 7), 2, 3, 1, (12, 12), 1, 32)]        # many taps, most of them partly outside


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case", range(len(GEOMETRIES)))
def test_int_conv2d4_bit_for_bit(antq_lib, dev, case, dtype_name):
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype_name)
    C, (R, S), stride, padding, dilation, (H, W), B, N = GEOMETRIES[case]
    K = R * S * C
    # signed flint-4 weights with unsigned int-4 activations on the even cases, signed int-4 on both sides on the odd ones
    wbook, xbook = ("ant_flint4_s", "ant_int4_u") if case % 2 == 0 else ("ant_int4_s", "ant_int4_s")
    plan_w, (xgrid, xgmax, _, _) = antq_lib.plan_for(_book(wbook)[0]), _book(xbook)
    plan_x = antq_lib.plan_for(xgrid)
    (I_w, image_w), (I_x, image_x) = plan_w.integer_image(), plan_x.integer_image()
    gen = torch.Generator(device=dev).manual_seed(case)
    ax = (torch.rand(1, device=dev, generator=gen) + 0.5).float()
    # |x| in [0.5, 1] alpha: no element quantises to 0, so a tap read from outside the image that should be zero changes S
    x = (torch.rand(B, C, H, W, device=dev, generator=gen) * 0.5 + 0.5) * ax
    if xbook.endswith("s"):
        x = x * (torch.randint(0, 2, x.shape, device=dev, generator=gen) * 2 - 1)
    x = x.to(dt).contiguous(memory_format=torch.channels_last)
    xq = antq_lib.quant_i8(x.permute(0, 2, 3, 1), ax, plan_x, xgmax, 1, x.numel(), False, plan_x.image_dev(dev))
    assert tuple(xq.shape) == (B, H, W, C) and bool((xq != 0).all())
    codes = torch.randint(0, 256, (N, K // 2), device=dev, generator=gen, dtype=torch.uint8)      # [N][R][S][C]: every byte is two defined codes
    v = _v_of_codes(codes.cpu().numpy(), image_w, 0, False).reshape(N, R, S, C).transpose(0, 3, 1, 2)
    S64 = F.conv2d(xq.permute(0, 3, 1, 2).double().cpu(), torch.from_numpy(v.astype(np.float64)), None, stride, padding, dilation)
    assert float(S64.abs().max()) < 2 ** 31
    S32 = S64.permute(0, 2, 3, 1).numpy().astype(np.float32)                                     # NHWC, fl32(S)
    for per_row, with_bias in ((True, True), (False, False)):
        aw = (torch.rand(N if per_row else 1, device=dev, generator=gen) + 0.5).float()
        bias = torch.randn(N, device=dev, generator=gen).to(dt) if with_bias else None
        y = S32 * (np.float32(ax.item()) / np.float32(I_x))
        y = y * (np.broadcast_to(aw.cpu().numpy(), (N,)) / np.float32(I_w))
        if with_bias:
            y = y + bias.float().cpu().numpy()
        want = _bits(torch.from_numpy(y.astype(np.float32)).to(dt))
        call = lambda: antq_lib.int_conv2d4(codes, xq, aw, plan_w.image_dev(dev), I_w, ax, I_x, N, (R, S), stride, padding, dilation,
                                            per_row, dt, bias=bias)
        out = call()
        assert out.shape == S64.shape and out.is_contiguous(memory_format=torch.channels_last)
        assert np.array_equal(_bits(out.permute(0, 2, 3, 1)), want), (per_row, with_bias)
        if case in (0, 4):
            for waves in (2, 4):
                antq_lib.lib().antq_debug_set(23, waves)
                try:
                    assert np.array_equal(_bits(call().permute(0, 2, 3, 1)), want), waves
                finally:
                    antq_lib.lib().antq_debug_set(23, 0)
        if (R, S) == (1, 1):
            lin = antq_lib.int_linear4(codes, xq.view(-1, C), aw, plan_w.image_dev(dev), I_w, ax, I_x, N, C, per_row, dt, bias=bias)
            assert np.array_equal(_bits(lin).reshape(want.shape), want)


@pytest.mark.parametrize("what", ["c_48", "pair_rule", "sum_overflow", "misaligned_xq"])
def test_int_conv2d4_refusals_leave_the_output_alone(antq_lib, dev, what):
    import torch
    plan = antq_lib.plan_for(_book("ant_flint4_s")[0])
    C, I, flags, code = {"c_48": (48, 16, 0, -2), "pair_rule": (64, 16, antq_lib.FLAG_OVP, -2), "sum_overflow": (133152, 127, 0, -2),
                         "misaligned_xq": (64, 16, 0, -5)}[what]
    assert what != "sum_overflow" or (I * I * C >= 2 ** 31 > I * I * (C - 32) and C % 32 == 0)
    H = W = 1 if what == "sum_overflow" else 4
    codes = torch.zeros(4 * C // 2, dtype=torch.uint8, device=dev)
    xq = torch.ones(H * W * C + 16, dtype=torch.int8, device=dev)[1 if what == "misaligned_xq" else 0:][:H * W * C]
    one, image = torch.ones(1, device=dev), plan.image_dev(dev)
    out = torch.full((H * W * 4,), 7.0, device=dev)
    rc = antq_lib.lib().antq_conv2d4_i8(codes.data_ptr(), xq.data_ptr(), None, out.data_ptr(), 1, H, W, C, 4, 1, 1, 1, 1, 0, 0, 1, 1,
                                        one.data_ptr(), 0, I, image.data_ptr(), image.numel(), one.data_ptr(), I, flags, antq_lib.F32, None)
    torch.cuda.synchronize()
    assert rc == code and bool((out == 7.0).all())


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_packed_cnn_runs_the_integer_convs(antq_lib, dev, dtype_name):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    dt = getattr(torch, dtype_name)
    qmod, qutil = _trees("ant")
    qutil.set_quantizer(_args(mode="ant-int-flint", wbit=4, abit=4))
    torch.manual_seed(4)
    net = nn.Sequential(nn.Conv2d(3, 32, 3), nn.ReLU(), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 1),
                        nn.Conv2d(64, 32, 3, stride=2, padding=1))
    base = qmod.quantize_model(net).to(dev).to(dt).eval()
    qutil.enable_quantization(base)
    x = torch.randn(2, 3, 12, 12, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dt)
    with torch.no_grad():
        base(x)                                                            # calibration
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    tbank = qutil.pack_model(twin, fused_linear=True, integer_linear=True)
    bank = qutil.pack_model(model, fused_linear=True, integer_linear=True, integer_conv=True)
    assert [n for n, _ in bank.integer_skipped] == ["0"] and "C = 3" in bank.integer_skipped[0][1]
    seen = []
    hook = model.get_submodule("5").register_forward_hook(lambda m, i, o: seen.append((i[0].detach(), o.detach())))
    with torch.no_grad():
        y, today, plain = model(x), twin(x), base(x)
    hook.remove()
    assert bank.int_conv_calls == 3 and bank.int_conv_relayouts == 1 and tbank.int_conv_calls == 0
    assert y.shape == today.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(_bits(today), _bits(plain))                      # without the flag: today's bits
    if dtype_name == "float32":
        # the last conv against the float64 product of the fake-quant images, with the bound of the integer linear:
        # at most 4 roundings per image factor against 1 on the integer side, plus 3 in the epilogue -> 16 * 2^-24
        (xin, yout), tmod = seen[0], twin.get_submodule("5")
        with torch.no_grad():
            x64 = tmod.quant_input(xin, tmod.weight).double().cpu()
        W64 = tbank.entries[id(tmod.quant_weight)]["out"].double().cpu()
        b64 = tmod.bias.detach().double().cpu()
        ref = F.conv2d(x64, W64, b64, stride=2, padding=1)
        mag = F.conv2d(x64.abs(), W64.abs(), b64.abs(), stride=2, padding=1)
        err = (yout.double().cpu() - ref).abs()
        assert bool((err <= 16 * 2.0 ** -24 * mag).all()), float((err / mag).max())
