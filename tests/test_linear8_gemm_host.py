"""antq_linear8_gemm on the host: every refusal of include/antq.h in the stated order, through ctypes with null or made-up
pointers (the entry point validates before it touches HIP: callable on a CPU-only box), the constants shared by header and
binding, and the option check of fused_byte_gemm_rows through the three entry points of the module surface.  A call that has to
PASS a check is shown to by running into a later refusal (a misaligned x): nothing here launches."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -5
F32, BF16, F16 = 0, 1, 2
OVP = 1
BAD_X = 0x20004                # passes every check but the last one


def _call(L, **kw):
    a = dict(codes=0x10000, x=0x20000, bias=0, y=0x30000, M=130, N=16, K=64, alpha=0x40000, per_row=1, gmax=10.0, grid=0x50000,
             m=256, n_normal=0, flags=0, dtype=BF16)
    a.update(kw)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    f = L.antq_linear8_gemm
    f.restype = ci
    return f(vp(a["codes"]), vp(a["x"]), vp(a["bias"]), vp(a["y"]), sz(a["M"]), sz(a["N"]), sz(a["K"]), vp(a["alpha"]),
             ci(a["per_row"]), ctypes.c_float(a["gmax"]), vp(a["grid"]), ci(a["m"]), ci(a["n_normal"]), ctypes.c_uint(a["flags"]),
             ci(a["dtype"]), vp(0))


@pytest.fixture(scope="module")
def L(antq_lib):
    return ctypes.CDLL(antq_lib.LIB_PATH)


def test_argument_errors(L):
    for name in ("codes", "x", "y", "alpha", "grid"):
        assert _call(L, **{name: 0}) == ARG, name
    assert _call(L, dtype=3) == ARG and _call(L, dtype=-1) == ARG and _call(L, dtype=7) == ARG
    assert _call(L, flags=2) == ARG and _call(L, flags=OVP | 4) == ARG and _call(L, flags=0x80000000) == ARG
    assert _call(L, m=0) == ARG and _call(L, m=-3) == ARG
    # ... before the empty call, before float32 and with everything else wrong as well
    assert _call(L, x=0, M=0) == ARG and _call(L, dtype=9, N=0) == ARG and _call(L, flags=8, M=9999, K=7) == ARG
    assert _call(L, codes=0, x=0x20001) == ARG and _call(L, m=0, M=0) == ARG and _call(L, m=0, flags=OVP, K=7) == ARG
    assert _call(L, dtype=F32, grid=0) == ARG and _call(L, dtype=F32, flags=2) == ARG


def test_empty_calls_launch_nothing(L):
    assert _call(L, M=0) == OK and _call(L, N=0) == OK
    # before float32 and the refusals of the shape, of the book and of the alignment
    assert _call(L, M=0, dtype=F32) == OK and _call(L, N=0, dtype=F32) == OK
    assert _call(L, M=0, K=7) == OK and _call(L, N=0, K=0) == OK and _call(L, N=0, M=9999) == OK
    assert _call(L, M=0, x=BAD_X) == OK and _call(L, N=0, m=257) == OK and _call(L, M=0, codes=0x10001) == OK
    assert _call(L, N=0, flags=OVP, n_normal=0, m=5) == OK


def test_float32_is_unsupported(L):
    assert _call(L, dtype=F32) == UNSUPPORTED and _call(L, dtype=F32, M=1) == UNSUPPORTED
    # ... after the empty call (above) and before the alignment
    assert _call(L, dtype=F32, x=BAD_X) == UNSUPPORTED and _call(L, dtype=F32, codes=0x10001) == UNSUPPORTED
    for dtype in (BF16, F16):
        assert _call(L, dtype=dtype, x=BAD_X) == ALIGN


def test_unsupported(L, antq_lib):
    mx = antq_lib.LINEAR8_GEMM_MAX_M
    assert mx == 4096
    for M in (1, 8, 9, 64, 65, 128, 129, mx):
        assert _call(L, M=M, x=BAD_X) == ALIGN, M
    assert _call(L, M=mx + 1) == UNSUPPORTED and _call(L, M=100000) == UNSUPPORTED
    for K in (0, 4, 12, 20, 63):
        assert _call(L, K=K) == UNSUPPORTED, K
    for K in (8, 24, 72):
        assert _call(L, K=K, x=BAD_X) == ALIGN, K
    # plain books: up to 256 values
    assert _call(L, m=256, x=BAD_X) == ALIGN and _call(L, m=1, x=BAD_X) == ALIGN
    assert _call(L, m=257) == UNSUPPORTED and _call(L, m=100000) == UNSUPPORTED
    # pair rule: 1 .. 255 normal values, 0 .. 255 outliers
    for nn, m in ((255, 510), (1, 1), (1, 256), (255, 255), (15, 30)):
        assert _call(L, flags=OVP, n_normal=nn, m=m, x=BAD_X) == ALIGN, (nn, m)
    for nn, m in ((0, 20), (0, 0 + 255), (256, 300), (256, 511), (255, 511), (-1, 20), (8, 7), (200, 100), (1, 257)):
        assert _call(L, flags=OVP, n_normal=nn, m=m) == UNSUPPORTED, (nn, m)
    # rows and row length in 32 bits
    assert _call(L, N=2 ** 31) == UNSUPPORTED and _call(L, K=2 ** 31) == UNSUPPORTED and _call(L, K=2 ** 32 + 64) == UNSUPPORTED
    assert _call(L, N=2 ** 31 - 1, x=BAD_X) == ALIGN and _call(L, K=2 ** 31 - 8, x=BAD_X) == ALIGN
    # before the alignment
    assert _call(L, M=mx + 1, x=0x20008) == UNSUPPORTED and _call(L, K=12, codes=0x10001) == UNSUPPORTED
    assert _call(L, m=257, y=0x30001) == UNSUPPORTED and _call(L, flags=OVP, n_normal=0, m=4, x=BAD_X) == UNSUPPORTED


def test_alignment(L):
    for dtype in (BF16, F16):
        for off in (1, 2, 4, 8):
            assert _call(L, dtype=dtype, x=0x20000 + off) == ALIGN, (dtype, off)
        for off in range(1, 8):
            assert _call(L, dtype=dtype, codes=0x10000 + off) == ALIGN, (dtype, off)
            assert _call(L, dtype=dtype, codes=0x10008 + off, K=8) == ALIGN, (dtype, off)
        assert _call(L, dtype=dtype, y=0x30001) == ALIGN and _call(L, dtype=dtype, bias=0x60001) == ALIGN
    assert _call(L, flags=OVP, n_normal=255, m=510, y=0x30001) == ALIGN
    assert _call(L, M=4096, x=BAD_X) == ALIGN and _call(L, M=4097, x=BAD_X) == UNSUPPORTED


def test_constants_in_header_and_binding(antq_lib):
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    assert int(re.search(r"#define ANTQ_LINEAR8_GEMM_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR8_GEMM_MAX_M == 4096
    assert int(re.search(r"#define ANTQ_LINEAR8_MM_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR8_MM_MAX_M == 64
    assert int(re.search(r"#define ANTQ_LINEAR4_GEMM_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR4_GEMM_MAX_M == 4096
    assert int(re.search(r"#define ANTQ_ABI_VERSION (\d+)", hdr).group(1)) == antq_lib.ABI_VERSION == 7
    assert antq_lib.lib().antq_abi_version() == 7
    assert re.search(r"\bantq_linear8_gemm\s*\(", hdr)


def test_binding_has_the_entry(antq_lib):
    """(that linear8_gemm itself refuses float32 and 4097 rows needs tensors on a GPU: tests/test_gpu_linear8_gemm.py)"""
    assert callable(antq_lib.linear8_gemm)
    assert antq_lib.lib().antq_linear8_gemm.argtypes == antq_lib.lib().antq_linear8.argtypes


def test_fused_byte_gemm_rows_option(antq_lib):
    import torch.nn as nn
    from ant_quantization_amd import packed
    model = nn.Sequential(nn.Linear(8, 8))
    calls = (("pack_model", lambda **kw: packed.pack_model(model, **kw)), ("PackedBank", lambda **kw: packed.PackedBank(model, **kw)),
             ("load_packed_state_dict", lambda **kw: packed.load_packed_state_dict(model, {}, **kw)))
    for who, call in calls:
        who = "PackedBank" if who == "pack_model" else who          # (pack_model's checks are the bank's)
        # without fused_linear
        with pytest.raises(antq_lib.AntqError, match="%s: fused_byte_gemm_rows needs fused_linear=True" % who):
            call(fused_byte_gemm_rows=256)
        with pytest.raises(antq_lib.AntqError, match="fused_byte_gemm_rows needs fused_linear=True"):
            call(fused_byte_gemm_rows=128, fused_linear=False)
        # without fused_bytes
        with pytest.raises(antq_lib.AntqError, match="%s: fused_byte_gemm_rows needs fused_bytes=True" % who):
            call(fused_linear=True, fused_byte_gemm_rows=256)
        with pytest.raises(antq_lib.AntqError, match="fused_byte_gemm_rows needs fused_bytes=True"):
            call(fused_linear=True, fused_gemm_rows=256, fused_bytes=False, fused_byte_gemm_rows=128)
        # outside (64, 4096]
        for bad in (0, 8, 64, 4097, 128.0, "128", True, 1, 100000, -3):
            with pytest.raises(antq_lib.AntqError, match=r"fused_byte_gemm_rows must be an integer in \(64, 4096\]"):
                call(fused_linear=True, fused_bytes=True, fused_byte_gemm_rows=bad)
        # beside the other row options, whose own checks still hold
        with pytest.raises(antq_lib.AntqError, match="fused_byte_rows must be"):
            call(fused_linear=True, fused_bytes=True, fused_byte_rows=65, fused_byte_gemm_rows=256)
        with pytest.raises(antq_lib.AntqError, match="fused_gemm_rows must be"):
            call(fused_linear=True, fused_bytes=True, fused_gemm_rows=64, fused_byte_gemm_rows=256)
