"""antq_quant_i8_nhwc on the GPU: bit for bit the bytes antq_quant_i8 writes for a torch-made channels-last copy of the same
tensor (that path is held to the image of antq_encode8's codes by test_gpu_int_linear4 / 8), its footprint, and the module
surface (pack_model(integer_conv=True, integer_conv_nchw=True)).

All three books' plans take the encoder's `adom` branch (asserted from the plan's header); its other branch (quant_vec + the
code mapping) is reached for the same plans through antq_debug_set key 4 = 0, which clears pa.adom in every launcher."""
import copy

import numpy as np
import pytest

from test_gpu_int_linear4 import _bits
from test_gpu_linear8 import _args, _trees

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16")
BOOKS = {"flint4_s": ("flint", 4, True, 127), "int4_u": ("int", 4, False, 127), "int8_s": ("int", 8, True, 128)}
GEOMETRIES = [(1, 16, 1, 1),        # one piece
              (2, 32, 7, 7),        # P = 49: unaligned rows, position tail
              (1, 80, 3, 5),        # channel tail, P = 15
              (3, 64, 8, 8),        # full tiles, one contiguous run
              (1, 144, 14, 14),     # three channel slabs with a 16-channel tail; aligned in float32, not in 16-bit
              (2, 32, 9, 16)]       # P = 144: aligned, crosses a position tile with a tail
ADOM_WORD = 22                      # PlanHeader::adom, in 32-bit words (csrc/antq_internal.h)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _plan(antq_lib, dev, book):
    from ant_quantization_amd import grids
    kind, bits, signed, limit = BOOKS[book]
    grid = grids.ant_grid(kind, bits, signed)
    plan = antq_lib.plan_for(grid)
    return plan, float(grid.max()), plan.image_dev(dev, limit)


def _input(dev, dt, shape, seed, offset=0):
    """Seeded normal data covering the book at alpha = 1, with NaN, +Inf, -Inf, 0, a value beyond the range and the largest finite
    value planted at the first and last position of a vector, a thread's unit, a tile and the tensor, in the first and last
    channel of a thread, a piece, a slab and the tensor.  offset: elements between the allocation's start and x."""
    import torch
    B, C, H, W = shape
    n = B * C * H * W
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = (torch.randn(n + 8, device=dev, generator=gen) * 0.6).to(dt)[offset:offset + n].view(B, C, H * W)
    special = [float("nan"), float("inf"), float("-inf"), 0.0, 1.0e4, torch.finfo(dt).max]
    spots = [(c, p) for c in (0, 3, 4, 15, 16, 63, 64, C - 1) for p in (0, 3, 4, 7, 8, 63, 64, 127, 128, H * W - 1) if c < C and p < H * W]
    for i, (c, p) in enumerate(spots):
        x[i % B, c, p] = special[i % 6]
    return x.view(B, C, H, W)


def _yardstick(antq_lib, x, alpha, plan, gmax, image):
    import torch
    last = x.contiguous(memory_format=torch.channels_last)
    return antq_lib.quant_i8(last.permute(0, 2, 3, 1), alpha, plan, gmax, 1, x.numel(), False, image)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("book", list(BOOKS))
@pytest.mark.parametrize("case", range(len(GEOMETRIES)))
def test_the_bytes_are_quant_i8s(antq_lib, dev, case, book, dtype_name):
    import torch
    plan, gmax, image = _plan(antq_lib, dev, book)
    assert plan.host.view(np.uint32)[ADOM_WORD] == 1
    alpha = torch.ones(1, device=dev)
    x = _input(dev, getattr(torch, dtype_name), GEOMETRIES[case], case)
    for knob_a in (1, 0):                              # encode_unit_a; quant_vec + the code mapping
        antq_lib.lib().antq_debug_set(4, knob_a)
        try:
            want = _yardstick(antq_lib, x, alpha, plan, gmax, image)
            got = antq_lib.quant_i8_nhwc(x, alpha, plan, gmax, image)
        finally:
            antq_lib.lib().antq_debug_set(4, 1)
        assert got.shape == want.shape and torch.equal(got, want), knob_a
    assert int(want.min()) < 0 or book == "int4_u"
    assert int(want.max()) > 0


@pytest.mark.parametrize("dtype_name", ("float32", "bfloat16"))
@pytest.mark.parametrize("case", range(len(GEOMETRIES)))
def test_nothing_outside_q_is_written(antq_lib, dev, case, dtype_name):
    import torch
    plan, gmax, image = _plan(antq_lib, dev, "flint4_s")
    alpha = torch.full((1,), 0.75, device=dev)
    shape = GEOMETRIES[case]
    # one element off the allocation's start: the two geometries whose shape alone gives 16-byte loads take element loads
    x = _input(dev, getattr(torch, dtype_name), shape, 10 + case, offset=1 if case in (3, 5) else 0)
    assert (x.data_ptr() % 16 != 0) == (case in (3, 5))
    n = x.numel()
    buf = torch.full((n + 512,), 0x55, dtype=torch.int8, device=dev)
    got = antq_lib.quant_i8_nhwc(x, alpha, plan, gmax, image, out=buf[256:256 + n])
    assert bool((buf[:256] == 0x55).all()) and bool((buf[256 + n:] == 0x55).all())
    assert torch.equal(got, _yardstick(antq_lib, x, alpha, plan, gmax, image))


def test_packed_cnn_quantises_its_nchw_input_in_one_launch(antq_lib, dev):
    import torch
    import torch.nn as nn
    qmod, qutil = _trees("ant")
    qutil.set_quantizer(_args(mode="ant-int-flint", wbit=4, abit=4))
    torch.manual_seed(7)
    net = nn.Sequential(nn.Conv2d(32, 64, 3, padding=1), nn.Conv2d(64, 32, 1))
    base = qmod.quantize_model(net).to(dev).eval()
    qutil.enable_quantization(base)
    x = torch.randn(2, 32, 9, 9, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    with torch.no_grad():
        base(x)                                                            # calibration
    twin, model = copy.deepcopy(base), copy.deepcopy(base)
    opts = dict(fused_linear=True, integer_linear=True, integer_conv=True)
    tbank = qutil.pack_model(twin, **opts)
    bank = qutil.pack_model(model, integer_conv_nchw=True, **opts)
    with torch.no_grad():
        want = _bits(twin(x))
        assert (tbank.int_conv_calls, tbank.int_conv_relayouts, tbank.int_conv_nchw_calls) == (2, 1, 0)
        assert np.array_equal(_bits(model(x)), want)
        assert (bank.int_conv_calls, bank.int_conv_relayouts, bank.int_conv_nchw_calls) == (2, 0, 1)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(x)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), want)
