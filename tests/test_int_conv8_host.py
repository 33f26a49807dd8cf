"""antq_conv2d8_i8 / antq_conv2d8_i8_sk (the integer-domain conv2d from byte codes) on the host: the refusals in the order
include/antq.h states, the option's place in the table, the offset image, and the tap-major / wsum builders."""
import ctypes

import numpy as np
import pytest

vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
IMAGE = np.arange(-128, 128).astype(np.int8)           # ANT's signed int8 book: the host copy is read once the checks pass


def _call(L, sk, **kw):
    a = dict(codes=0x10000, xq=0x20000, bias=0, y=0x30000, B=1, H=4, W=4, C=256, N=16, R=1, S=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1,
             alpha_w=0x40000, per_row=1, I_w=128, host=IMAGE.ctypes.data, image=0x50000, m=256, alpha_x=0x60000, I_x=128, x_offset=0,
             wsum=0, ws=0, ws_bytes=0, flags=0, dtype=1)
    a.update(kw)
    head = [vp(a["codes"]), vp(a["xq"]), vp(a["bias"]), vp(a["y"])] + [sz(a[k]) for k in "BHWCN"]
    head += [ci(a[k]) for k in ("R", "S", "sh", "sw", "ph", "pw", "dh", "dw")]
    head += [vp(a["alpha_w"]), ci(a["per_row"]), ci(a["I_w"]), vp(a["host"]), vp(a["image"]), ci(a["m"]), vp(a["alpha_x"]), ci(a["I_x"]),
             ci(a["x_offset"]), vp(a["wsum"])]
    tail = [cu(a["flags"]), ci(a["dtype"]), vp(0)]
    return L.antq_conv2d8_i8_sk(*head, vp(a["ws"]), sz(a["ws_bytes"]), *tail) if sk else L.antq_conv2d8_i8(*head, *tail)


def test_refusals_come_in_the_stated_order(antq_lib):
    L = antq_lib.lib()
    assert len(L.antq_conv2d8_i8.argtypes) == 30 and len(L.antq_conv2d8_i8_sk.argtypes) == 32
    # each fault with every later one still present: the earliest decides (made-up addresses: nothing is launched)
    faults = [(dict(host=0), -1), (dict(x_offset=64), -1), (dict(x_offset=128, wsum=0), -1), (dict(dtype=9), -1),
              (dict(flags=antq_lib.FLAG_OVP << 1), -1), (dict(flags=antq_lib.FLAG_OVP), -2), (dict(m=257), -2), (dict(C=48), -2),
              (dict(I_x=129), -2), (dict(I_x=128, C=131072), -2), (dict(wsum=0x70002), -5)]
    sk_only = [(dict(B=100), -2), (dict(ws=0x80008), -5), (dict(ws=0, ws_bytes=0), -1)]
    L.antq_debug_set(24, 2)                # two slices: the last check has a workspace to ask for
    try:
        for sk, table in ((False, faults), (True, faults + sk_only)):
            for i, (_, code) in enumerate(table):
                merged = {}
                for f, _ in reversed(table[i:]):
                    merged.update(f)
                assert _call(L, sk, **merged) == code, (sk, i)
        assert _call(L, False, B=0, xq=0x20000) == 0          # an empty call: no launch
        # the offset form's own range and sum bound: I_x up to 255, 256 I_w K < 2^31
        assert _call(L, False, x_offset=128, wsum=0x70000, I_x=256) == -2
        assert _call(L, False, x_offset=128, wsum=0x70000, I_x=255, C=65536) == -2
    finally:
        L.antq_debug_set(24, 0)


def test_the_option_and_its_needs(antq_lib):
    from ant_quantization_amd import packed
    on = dict(fused_linear=True, fused_bytes=True, integer_linear=True, integer_bytes=True, integer_conv=True)
    row = [o for o in packed._OPTIONS if o.name == "integer_conv_bytes"]
    assert len(row) == 1 and row[0].default is False and row[0].limits is None and set(row[0].needs) == set(on)
    for missing in on:
        with pytest.raises(antq_lib.AntqError, match="needs %s=True" % missing):
            packed._check_options("pack_model", integer_conv_bytes=True, **{k: v for k, v in on.items() if k != missing})
    packed._check_options("pack_model", integer_conv_bytes=True, **on)
    assert antq_lib.CONV2D8_I8_SK_MAX_M == 1024 and callable(antq_lib.int_conv2d8) and callable(antq_lib.int_conv2d8_sk)


def test_the_offset_image(antq_lib):
    from ant_quantization_amd import grids
    unsigned = grids.ant_grid("int", 8, False)
    I, image = grids.offset_image(unsigned)
    assert I == 255 and image.dtype == np.int8
    assert np.array_equal(image.astype(np.int64) + 128, np.rint(unsigned / unsigned.max() * 255))       # bytes c - 128, in code order
    assert sorted(image.tolist()) == list(range(-128, 128))
    assert grids.offset_image(grids.ant_grid("int", 8, True)) is None and grids.offset_image(grids.ant_grid("flint", 4, True)) is None
    assert grids.integer_image(unsigned, limit=128) is None                # the 1 .. 128 limit is untouched
    plan = antq_lib.plan_for(unsigned)
    assert plan.offset_image()[0] == 255 and plan.integer_image8() is None


def test_tap_major_bytes_and_wsum_against_numpy():
    import torch
    from ant_quantization_amd import packed
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, size=(5, 32, 3, 3), dtype=np.uint8)       # encode8's layout of a [5, 32, 3, 3] weight
    image = rng.integers(-128, 128, size=200).astype(np.int8)              # a book of 200 values: codes past it count 0
    got = packed._tap_major_bytes(torch.from_numpy(codes.reshape(-1)), codes.shape)
    want = codes.transpose(0, 2, 3, 1).reshape(-1)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    table = np.zeros(256, dtype=np.int64)
    table[:200] = image
    wsum = packed._image_sums(got, image, 5)
    assert wsum.dtype == torch.int32 and np.array_equal(wsum.numpy(), table[want.reshape(5, -1)].sum(axis=1))
