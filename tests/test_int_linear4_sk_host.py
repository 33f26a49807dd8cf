"""antq_linear4_i8_sk (the split-K integer-domain linear for 1 .. 64 rows) on the host: every refusal of include/antq.h in the
stated order, through ctypes with made-up pointers (nothing is launched: callable without a GPU), the launcher's rule for the
slices of K at the points where it switches, and the option's place in the option table.  The launches:
tests/test_gpu_int_linear4_sk.py."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -5
F32, BF16 = 0, 1
vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


@pytest.fixture(scope="module")
def L(antq_lib):
    L = ctypes.CDLL(antq_lib.LIB_PATH)
    L.antq_linear4_i8_sk_workspace_bytes.restype = sz
    L.antq_linear4_i8_sk_workspace_bytes.argtypes = [sz, sz, sz]
    L.antq_linear4_i8_sk_slices.argtypes = [sz, sz, sz, ci]
    return L


def _call(L, **kw):
    a = dict(codes=0x10000, xq=0x20000, bias=0, y=0x30000, M=1, N=16, K=64, alpha_w=0x40000, per_row=1, I_w=16, image=0x50000, m=16,
             n_normal=0, alpha_x=0x60000, I_x=16, ws=0, ws_bytes=0, flags=0, dtype=BF16)
    a.update(kw)
    return L.antq_linear4_i8_sk(vp(a["codes"]), vp(a["xq"]), vp(a["bias"]), vp(a["y"]), sz(a["M"]), sz(a["N"]), sz(a["K"]),
                                vp(a["alpha_w"]), ci(a["per_row"]), ci(a["I_w"]), vp(a["image"]), ci(a["m"]), ci(a["n_normal"]),
                                vp(a["alpha_x"]), ci(a["I_x"]), vp(a["ws"]), sz(a["ws_bytes"]), ctypes.c_uint(a["flags"]),
                                ci(a["dtype"]), vp(0))


def test_refusals_in_the_stated_order(L, antq_lib):
    assert L.antq_abi_version() == antq_lib.ABI_VERSION == 7
    big = dict(M=8, N=4096, K=4096)                      # a call that is split on every part of more than 32 CUs (256 without one)
    need = L.antq_linear4_i8_sk_workspace_bytes(8, 4096, 4096)
    assert need >= 2 * 4 * 8 * 4096
    for name in ("codes", "xq", "y", "alpha_w", "image", "alpha_x"):
        assert _call(L, **{name: 0}) == ARG, name
    assert _call(L, m=0) == ARG and _call(L, dtype=3) == ARG and _call(L, flags=2) == ARG
    assert _call(L, xq=0, M=0) == ARG and _call(L, flags=4, K=7, M=65) == ARG            # ... before everything else
    assert _call(L, M=0, K=7) == OK and _call(L, N=0, M=65, xq=0x20001) == OK           # an empty call: before shape and alignment
    assert _call(L, M=65) == UNSUPPORTED and _call(L, M=64, K=48) == UNSUPPORTED and _call(L, K=0) == UNSUPPORTED
    assert _call(L, m=17) == UNSUPPORTED and _call(L, I_x=128) == UNSUPPORTED and _call(L, N=1 << 31) == UNSUPPORTED
    assert _call(L, I_x=127, I_w=127, K=133152) == UNSUPPORTED
    assert _call(L, M=65, xq=0x20004, ws=0x70004) == UNSUPPORTED                        # ... before the alignment
    for k, v in (("xq", 0x20008), ("codes", 0x10004), ("y", 0x30001), ("bias", 0x80001), ("alpha_w", 0x40002), ("ws", 0x70004), ("ws", 0x70008)):
        assert _call(L, **{k: v}) == ALIGN, k
    assert _call(L, ws=0x70004, ws_bytes=0, **big) == ALIGN                             # ... before the workspace's size
    assert _call(L, ws=0, ws_bytes=need, **big) == ARG and _call(L, ws=0x70000, ws_bytes=need - 1, **big) == ARG
    assert _call(L, ws=0x70000, ws_bytes=0, **big) == ARG


def _rule(M, N, K, cus, forced=0):
    """csrc/antq_k_linear_i8.h, i8_sk_slices, restated"""
    tiles, stages = -(-N // 64), -(-K // 128)
    S = next((s for s in (1, 2, 4, 8, 16) if tiles * s >= 2 * cus), 16)
    S = min(S, max(K // (16 * M), 1))
    S = max(min(min(forced, 16) if forced >= 1 else S, stages), 1)
    return -(-stages // -(-stages // S))


def test_the_launcher_rule_where_it_switches(L):
    points = [(1, 4096, 4096), (64, 4096, 4096), (64, 4096, 4095 * 16), (1, 768, 3072), (8, 3072, 768), (64, 16384, 16384),
              (1, 64 * 511, 4096), (1, 64 * 512, 4096), (1, 64 * 255, 4096), (1, 64 * 256, 4096), (1, 64 * 63 + 1, 4096),    # tiles S against 2 cus
              (64, 64, 1024), (64, 64, 2047 * 32), (64, 64, 2048), (33, 64, 1056), (16, 64, 256 * 16), (17, 64, 256 * 16),    # the traffic cap
              (1, 64, 32), (1, 64, 128), (1, 64, 160), (1, 64, 384), (1, 64, 1152), (1, 64, 1056), (2, 1, 17 * 128)]          # stages, uneven slices
    for cus in (256, 304, 1, 32):
        for M, N, K in points:
            assert L.antq_linear4_i8_sk_slices(M, N, K, cus) == _rule(M, N, K, cus), (M, N, K, cus)
    assert [L.antq_linear4_i8_sk_slices(1, 4096, 4096, c) for c in (16, 32, 64, 128, 256)] == [1, 1, 2, 4, 8]
    assert [L.antq_linear4_i8_sk_slices(M, 4096, 4096, 256) for M in (16, 32, 33, 64)] == [8, 8, 7, 4]
    assert L.antq_linear4_i8_sk_slices(0, 64, 64, 256) == 0
    try:
        for forced in (1, 2, 3, 16, 99):
            L.antq_debug_set(24, forced)
            for M, N, K in points:
                assert L.antq_linear4_i8_sk_slices(M, N, K, 256) == _rule(M, N, K, 256, forced), (M, N, K, forced)
            S = L.antq_linear4_i8_sk_slices(5, 63, 1056, 0)                   # (forced: whatever the device, if there is one)
            assert L.antq_linear4_i8_sk_workspace_bytes(5, 63, 1056) == (0 if S == 1 else (4 * S * 5 * 63 + 15) // 16 * 16)
    finally:
        L.antq_debug_set(24, 0)
    S = L.antq_linear4_i8_sk_slices(8, 4096, 4096, 0)
    assert L.antq_linear4_i8_sk_workspace_bytes(8, 4096, 4096) // (4 * 8 * 4096) == S and S > 1


def test_surface(antq_lib):
    from ant_quantization_amd import packed
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    assert int(re.search(r"#define ANTQ_LINEAR4_I8_SK_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR4_I8_SK_MAX_M == 64
    assert antq_lib.lib().antq_linear4_i8_sk_workspace_bytes.restype is ctypes.c_size_t and len(antq_lib.lib().antq_linear4_i8_sk.argtypes) == 20
    for given in ({}, {"fused_linear": True}):
        with pytest.raises(antq_lib.AntqError, match="integer_split_k needs %s=True" % ("integer_linear" if given else "fused_linear")):
            packed._check_options("pack_model", integer_split_k=True, **given)
    packed._check_options("pack_model", fused_linear=True, integer_linear=True, integer_split_k=True)
