"""The split-K integer-domain conv2d (antq_conv2d4_i8_sk, outputs of up to 1024 rows) on the GPU: bit for bit against the formula
of include/antq.h as test_gpu_int_conv4.py forms it (S from a float64 F.conv2d of the integer-valued operands, the epilogue step
by step in np.float32) and against antq_conv2d4_i8, for forced slices and the rule; a sum beyond 2^24 across slices, the
workspace's footprint, the refusals, capture, and pack_model(integer_conv_split_k=True)."""
import copy
import functools

import numpy as np
import pytest

from test_gpu_int_linear4 import _bits, _book, _v_of_codes
from test_gpu_linear8 import _args, _trees

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")
# (C, (R, S), stride, padding, dilation, (H, W), B, N), the forced slices (0: the rule)
GEOMETRIES = [((32, (3, 3), 1, 1, 1, (7, 7), 1, 40), (1, 2, 3)),         # M = 49, K = 288: a partial last stage, four taps per stage, a partial n tile
              ((160, (1, 3), 1, (0, 1), 1, (5, 6), 2, 64), (2, 4)),      # K = 480: slices that begin inside a tap
              ((64, (3, 3), 2, 1, 1, (9, 9), 3, 72), (2,)),              # M = 75: two row tiles (64 + 11) that cross images, two n tiles
              ((32, (7, 7), 2, 3, 1, (12, 12), 1, 32), (16,)),           # 13 stages, most taps partly outside; 16 clamps to 13
              ((32, (3, 3), 1, 2, 2, (8, 8), 1, 16), (0,)),              # dilation
              ((64, (1, 1), 1, 0, 1, (10, 10), 3, 64), (0,))]            # M = 300: five row tiles; equals antq_linear4_i8
POINTS = [(case, S) for case, (_, forced) in enumerate(GEOMETRIES) for S in forced]


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


@functools.lru_cache(maxsize=None)
def _case(case, dtype_name):
    """One geometry's operands and fl32(S) in NHWC, formed once and shared by every number of slices.  Returns (geometry
    arguments of the _lib calls, call(fn, per_row, bias, **kw), S32, (aw per row, aw per tensor, bias, ax), I_x, I_w)."""
    import torch
    import torch.nn.functional as F
    from ant_quantization_amd import _lib
    dev, dt = torch.device("cuda:0"), getattr(torch, dtype_name)
    C, (R, S), stride, padding, dilation, (H, W), B, N = GEOMETRIES[case][0]
    K = R * S * C
    wbook, xbook = ("ant_flint4_s", "ant_int4_u") if case % 2 == 0 else ("ant_int4_s", "ant_int4_s")
    plan_w, (xgrid, xgmax, _, _) = _lib.plan_for(_book(wbook)[0]), _book(xbook)
    plan_x = _lib.plan_for(xgrid)
    (I_w, image_w), (I_x, _) = plan_w.integer_image(), plan_x.integer_image()
    gen = torch.Generator(device=dev).manual_seed(100 + case)
    ax = (torch.rand(1, device=dev, generator=gen) + 0.5).float()
    # |x| in [0.5, 1] alpha: no element quantises to 0, so a tap read from outside the image that should be zero changes S
    x = (torch.rand(B, C, H, W, device=dev, generator=gen) * 0.5 + 0.5) * ax
    if xbook.endswith("s"):
        x = x * (torch.randint(0, 2, x.shape, device=dev, generator=gen) * 2 - 1)
    x = x.to(dt).contiguous(memory_format=torch.channels_last)
    xq = _lib.quant_i8(x.permute(0, 2, 3, 1), ax, plan_x, xgmax, 1, x.numel(), False, plan_x.image_dev(dev))
    assert tuple(xq.shape) == (B, H, W, C) and bool((xq != 0).all())
    codes = torch.randint(0, 256, (N, K // 2), device=dev, generator=gen, dtype=torch.uint8)      # [N][R][S][C]
    v = _v_of_codes(codes.cpu().numpy(), image_w, 0, False).reshape(N, R, S, C).transpose(0, 3, 1, 2)
    S64 = F.conv2d(xq.permute(0, 3, 1, 2).double().cpu(), torch.from_numpy(v.astype(np.float64)), None, stride, padding, dilation)
    assert float(S64.abs().max()) < 2 ** 31
    S32 = S64.permute(0, 2, 3, 1).numpy().astype(np.float32)
    scales = ((torch.rand(N, device=dev, generator=gen) + 0.5).float(), (torch.rand(1, device=dev, generator=gen) + 0.5).float(),
              torch.randn(N, device=dev, generator=gen).to(dt), ax)
    image = plan_w.image_dev(dev)

    def call(fn, per_row, bias, **kw):
        return fn(codes, xq, scales[0] if per_row else scales[1], image, I_w, ax, I_x, N, (R, S), stride, padding, dilation, per_row, dt,
                  bias=bias, **kw)
    return (codes, xq, image), call, S32, scales, I_x, I_w


def _want(S32, scales, I_x, I_w, per_row, with_bias, dt):
    import torch
    y = S32 * (np.float32(scales[3].item()) / np.float32(I_x))
    y = y * (np.broadcast_to((scales[0] if per_row else scales[1]).cpu().numpy(), S32.shape[-1:]) / np.float32(I_w))
    if with_bias:
        y = y + scales[2].float().cpu().numpy()
    return _bits(torch.from_numpy(y.astype(np.float32)).to(dt))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("case, S", POINTS)
def test_bit_for_bit_whatever_the_split(antq_lib, dev, split, case, S, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    (codes, xq, image), call, S32, scales, I_x, I_w = _case(case, dtype_name)
    C, (R, Sk), _, _, _, _, _, N = GEOMETRIES[case][0]
    M = S32.size // N
    split(S)
    ws = torch.empty(antq_lib.int_conv2d4_sk_workspace_bytes(M, N, R * Sk * C), dtype=torch.uint8, device=dev)
    for per_row, with_bias in ((True, True), (False, False)):
        bias = scales[2] if with_bias else None
        want = _want(S32, scales, I_x, I_w, per_row, with_bias, dt)
        ws.fill_(0x7f)
        out = call(antq_lib.int_conv2d4_sk, per_row, bias, workspace=ws)
        assert out.shape == (S32.shape[0], N) + S32.shape[1:3] and out.is_contiguous(memory_format=torch.channels_last)
        assert np.array_equal(_bits(out.permute(0, 2, 3, 1)), want), (per_row, with_bias)
        assert np.array_equal(_bits(call(antq_lib.int_conv2d4, per_row, bias).permute(0, 2, 3, 1)), want)
        if (R, Sk) == (1, 1):
            lin = antq_lib.int_linear4(codes, xq.view(-1, C), scales[0] if per_row else scales[1], image, I_w, scales[3], I_x, N, C, per_row,
                                       dt, bias=bias)
            assert np.array_equal(_bits(lin).reshape(want.shape), want)


def _pixel(antq_lib, dev, dt, C, N, seed, H=1, W=1):
    """a 1 x 1 conv on an H x W image whose operands sit at their books' extremes but for 32 random k per row: (call, S, want)"""
    import torch
    plan = antq_lib.plan_for(_book("ant_int4_s")[0])
    I, image = plan.integer_image()
    top = int(np.argmax(np.abs(image)))
    gen = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.full((N, C // 2), top | (top << 4), dtype=torch.uint8, device=dev)
    codes[:, :16] = torch.randint(0, 256, (N, 16), device=dev, generator=gen, dtype=torch.uint8)
    xq = torch.full((1, H, W, C), int(image[top]), dtype=torch.int8, device=dev)
    xq[..., :32] = torch.randint(-I, I + 1, (1, H, W, 32), device=dev, generator=gen, dtype=torch.int8)
    aw, ax = (torch.rand(N, device=dev, generator=gen) + 0.5).float(), (torch.rand(1, device=dev, generator=gen) + 0.5).float()
    bias = torch.randn(N, device=dev, generator=gen).to(dt)
    S = xq.view(-1, C).cpu().numpy().astype(np.int64) @ _v_of_codes(codes.cpu().numpy(), image, 0, False).T
    y = S.astype(np.float32) * (np.float32(ax.item()) / np.float32(I))
    y = y * (aw.cpu().numpy() / np.float32(I))[None, :] + bias.float().cpu().numpy()[None, :]
    call = lambda **kw: antq_lib.int_conv2d4_sk(codes, xq, aw, plan.image_dev(dev), I, ax, I, N, 1, 1, 0, 1, True, dt, bias=bias, **kw)
    return call, S, _bits(torch.from_numpy(y.astype(np.float32)).to(dt)), I


@pytest.mark.parametrize("S", [1, 16])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_partials_beyond_2_24_are_added_as_integers(antq_lib, dev, split, dtype_name, S):
    import torch
    I = antq_lib.plan_for(_book("ant_int4_s")[0]).integer_image()[0]
    C = (2 ** 24 // (I * I) // 32 + 2) * 32                                    # extremes on all but 32 k: beyond 2^24
    assert I * I * (C - 32) > 2 ** 24 and I * I * C < 2 ** 31
    call, Sums, want, _ = _pixel(antq_lib, dev, getattr(torch, dtype_name), C, 16, 6)
    assert np.abs(Sums).max() > 2 ** 24 and (Sums.astype(np.float32).astype(np.int64) != Sums).any()
    split(S)
    assert np.array_equal(_bits(call().permute(0, 2, 3, 1)).reshape(want.shape), want)


def test_workspace_footprint(antq_lib, dev, split):
    import torch
    call, _, want, _ = _pixel(antq_lib, dev, torch.float32, 1056, 63, 9, H=3, W=7)         # M = 21, 9 stages
    split(4)
    need = antq_lib.int_conv2d4_sk_workspace_bytes(21, 63, 1056)
    assert need == (3 * 4 * 21 * 63 + 15) // 16 * 16                          # 9 stages over 4 slices: 3 slices of 3 stages
    buf = torch.full((need + 4096,), 0x5a, dtype=torch.uint8, device=dev)
    assert np.array_equal(_bits(call(workspace=buf[:need]).permute(0, 2, 3, 1)).reshape(want.shape), want)
    assert bool((buf[need:] == 0x5a).all())


@pytest.mark.parametrize("what, code", [("rows", -2), ("short", -1), ("misaligned", -5)])
def test_refusals_leave_output_and_workspace_alone(antq_lib, dev, split, what, code):
    import torch
    H, W = (25, 41) if what == "rows" else (2, 4)                              # M = 1025, or 8
    call, _, _, _ = _pixel(antq_lib, dev, torch.float32, 512, 64, 1, H=H, W=W)
    assert H * W == (antq_lib.CONV2D4_I8_SK_MAX_M + 1 if what == "rows" else 8)
    split(4)
    need = antq_lib.int_conv2d4_sk_workspace_bytes(8, 64, 512)
    assert need == 4 * 4 * 8 * 64
    buf = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    ws = {"rows": buf, "short": buf[:need - 1], "misaligned": buf[4:]}[what]
    out = torch.full((1, H, W, 64), 7.0, device=dev).permute(0, 3, 1, 2)
    with pytest.raises(antq_lib.AntqError, match=r"\(%d\)" % code):
        call(workspace=ws, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 0).all())


def test_capture_and_replay(antq_lib, dev, split):
    import torch
    (codes, xq, image), call, S32, scales, I_x, I_w = _case(0, "bfloat16")
    want = _want(S32, scales, I_x, I_w, True, True, torch.bfloat16)
    split(3)
    ws = torch.empty(antq_lib.int_conv2d4_sk_workspace_bytes(49, 40, 288), dtype=torch.uint8, device=dev)
    out = torch.empty(1, 7, 7, 40, dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2)
    call(antq_lib.int_conv2d4_sk, True, scales[2], workspace=ws, out=out)      # (code objects loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(antq_lib.int_conv2d4_sk, True, scales[2], workspace=ws, out=out)
    out.zero_()
    ws.fill_(0x7f)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.permute(0, 2, 3, 1)), want)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_packed_cnn_splits_its_small_convs(antq_lib, dev, dtype_name):
    import torch
    import torch.nn as nn
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
        base(x)                                                                # calibration
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    on = dict(fused_linear=True, integer_linear=True, integer_conv=True)
    tbank = qutil.pack_model(twin, integer_split_k=True, **on)
    bank = qutil.pack_model(model, integer_conv_split_k=True, **on)
    with torch.no_grad():
        assert np.array_equal(_bits(model(x)), _bits(twin(x)))
    assert bank.int_conv_sk_calls == bank.int_conv_calls == 3
    assert tbank.int_conv_sk_calls == 0 and tbank.int_conv_calls == 3
