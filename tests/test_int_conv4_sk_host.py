"""antq_conv2d4_i8_sk (the split-K integer-domain conv2d for outputs of up to 1024 rows) on the host: the option's place in the
option table, the launcher's rule for the slices of K restated, the workspace's size, and -- through ctypes with made-up
pointers, nothing is launched -- the refusals that precede any HIP call, in the header's order.  The launches:
tests/test_gpu_int_conv4_sk.py."""
import ctypes
import itertools

import pytest

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -5
vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def test_the_option_needs_its_prerequisites(antq_lib):
    from ant_quantization_amd import packed
    on = dict(fused_linear=True, integer_linear=True, integer_conv=True)
    for missing in on:
        given = {k: v for k, v in on.items() if k != missing}
        with pytest.raises(antq_lib.AntqError, match="needs %s=True" % missing):      # (named by the first option that lacks it)
            packed._check_options("pack_model", integer_conv_split_k=True, **given)
    packed._check_options("pack_model", integer_conv_split_k=True, **on)
    packed._check_options("pack_model", integer_conv_split_k=False, fused_linear=True)
    assert antq_lib.CONV2D4_I8_SK_MAX_M == 1024 and callable(antq_lib.int_conv2d4_sk)
    assert len(antq_lib.lib().antq_conv2d4_i8_sk.argtypes) == 29


def _rule(M, N, K, cus, forced=0):
    """csrc/antq_k_linear_i8.h, i8_sk_slices, restated with the conv's row tiles"""
    tiles, stages = -(-N // 64) * -(-M // 64), -(-K // 128)
    S = next((s for s in (1, 2, 4, 8, 16) if tiles * s >= 2 * cus), 16)
    S = min(S, max(K // (16 * min(M, 64)), 1))
    S = max(min(min(forced, 16) if forced >= 1 else S, stages), 1)
    return -(-stages // -(-stages // S))


def test_the_slice_rule_and_the_workspace(antq_lib):
    L = antq_lib.lib()
    # ResNet's 7 x 7 and 14 x 14 stages at batch 1 and 8, the edges of a row tile, one stage, uneven slices
    points = list(itertools.product((1, 49, 64, 65, 196, 392, 1024), (64, 512, 2048), (32, 288, 1152, 4608, 17 * 128)))
    try:
        for forced in (0, 1, 3, 16, 99):
            L.antq_debug_set(24, forced)
            for (M, N, K), cus in itertools.product(points, (256, 304, 32, 1)):
                assert L.antq_conv2d4_i8_sk_slices(M, N, K, cus) == _rule(M, N, K, cus, forced), (M, N, K, cus, forced)
            for M, N, K in points:
                S = L.antq_conv2d4_i8_sk_slices(M, N, K, 0)                    # (whatever the device, if there is one)
                assert antq_lib.int_conv2d4_sk_workspace_bytes(M, N, K) == (0 if S == 1 else (4 * S * M * N + 15) // 16 * 16)
    finally:
        L.antq_debug_set(24, 0)
    assert L.antq_conv2d4_i8_sk_slices(49, 512, 4608, 256) == 5 and L.antq_conv2d4_i8_sk_slices(196, 256, 2304, 256) == 2
    assert L.antq_conv2d4_i8_sk_slices(0, 64, 64, 256) == 0
    for M, N, K in ((1, 4096, 4096), (33, 64, 1056), (64, 16384, 16384)):     # at most 64 rows: the linear's answers
        assert L.antq_conv2d4_i8_sk_slices(M, N, K, 256) == L.antq_linear4_i8_sk_slices(M, N, K, 256)


def _call(L, **kw):
    a = dict(codes=0x10000, xq=0x20000, bias=0, y=0x30000, B=1, H=4, W=4, C=64, N=16, R=3, S=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             alpha_w=0x40000, per_row=1, I_w=16, image=0x50000, m=16, alpha_x=0x60000, I_x=16, ws=0, ws_bytes=0, flags=0, dtype=1)
    a.update(kw)
    return L.antq_conv2d4_i8_sk(vp(a["codes"]), vp(a["xq"]), vp(a["bias"]), vp(a["y"]), *(sz(a[k]) for k in "BHWCN"),
                                *(ci(a[k]) for k in ("R", "S", "sh", "sw", "ph", "pw", "dh", "dw")), vp(a["alpha_w"]), ci(a["per_row"]),
                                ci(a["I_w"]), vp(a["image"]), ci(a["m"]), vp(a["alpha_x"]), ci(a["I_x"]), vp(a["ws"]), sz(a["ws_bytes"]),
                                ctypes.c_uint(a["flags"]), ci(a["dtype"]), vp(0))


def test_refusals_in_the_stated_order(antq_lib):
    L = ctypes.CDLL(antq_lib.LIB_PATH)
    big = dict(H=7, W=7, C=512, N=512)                   # M = 49, K = 4608: split on every part of more than 4 CUs (256 without one)
    for name in ("codes", "xq", "y", "alpha_w", "image", "alpha_x"):
        assert _call(L, **{name: 0}) == ARG, name
    assert _call(L, m=0) == ARG and _call(L, dtype=3) == ARG and _call(L, flags=2) == ARG
    assert _call(L, xq=0, B=0) == ARG and _call(L, flags=4, C=48) == ARG                  # ... before everything else
    assert _call(L, B=0, C=48) == OK and _call(L, N=0, xq=0x20001) == OK                 # an empty call: before shape and alignment
    # antq_conv2d4_i8's own: the pair rule, the book, C, an empty output, the sum's range
    assert _call(L, flags=1) == UNSUPPORTED and _call(L, m=17) == UNSUPPORTED and _call(L, C=48) == UNSUPPORTED
    assert _call(L, R=7, ph=0) == UNSUPPORTED and _call(L, sh=0) == UNSUPPORTED and _call(L, I_x=128) == UNSUPPORTED
    assert _call(L, I_x=127, I_w=127, C=133152, R=1, S=1, ph=0, pw=0) == UNSUPPORTED
    for k, v in (("xq", 0x20008), ("codes", 0x10004), ("y", 0x30001), ("bias", 0x80001), ("alpha_w", 0x40002)):
        assert _call(L, **{k: v}) == ALIGN, k
    assert _call(L, H=33, W=32, xq=0x20004) == ALIGN                                     # ... those come before the row limit
    # then the row limit (M = 1025 > 1024 >= 1024), the workspace's alignment, the workspace's size
    assert _call(L, H=25, W=41, ws=0x70004) == UNSUPPORTED and _call(L, H=32, W=32, ws=0x70004) == ALIGN
    assert _call(L, ws=0x70004) == ALIGN and _call(L, ws=0x70008, ws_bytes=1 << 30, **big) == ALIGN
    need = L.antq_conv2d4_i8_sk_workspace_bytes
    need.restype, need.argtypes = sz, [sz, sz, sz]
    assert need(49, 512, 4608) >= 2 * 4 * 49 * 512
    assert _call(L, ws=0, ws_bytes=need(49, 512, 4608), **big) == ARG
    assert _call(L, ws=0x70000, ws_bytes=need(49, 512, 4608) - 1, **big) == ARG and _call(L, ws=0x70000, ws_bytes=0, **big) == ARG
