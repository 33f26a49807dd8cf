"""antq_linear4_mm on the host: every refusal of include/antq.h in the stated order, through ctypes with null or made-up
pointers (the entry point validates before it touches HIP: callable on a CPU-only box), the constant shared by header and
binding, and the option checks of pack_model's fused_rows."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -5
F32, BF16, F16 = 0, 1, 2
OVP = 1


def _call(L, **kw):
    a = dict(codes=0x10000, x=0x20000, bias=0, y=0x30000, M=1, N=16, K=64, alpha=0x40000, per_row=1, gmax=10.0, grid=0x50000,
             m=16, n_normal=0, flags=0, dtype=BF16)
    a.update(kw)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    f = L.antq_linear4_mm
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
    # ... and they come first: with everything else wrong as well
    assert _call(L, x=0, M=0) == ARG and _call(L, dtype=9, N=0) == ARG and _call(L, flags=8, M=99, K=7) == ARG
    assert _call(L, codes=0, x=0x20001) == ARG
    # an empty codebook (m < 1) is an argument error as well, as the header says, and comes as early
    assert _call(L, m=0) == ARG and _call(L, m=-3) == ARG and _call(L, m=0, M=0) == ARG and _call(L, m=0, flags=OVP, K=7) == ARG


def test_empty_calls_launch_nothing(L):
    assert _call(L, M=0) == OK and _call(L, N=0) == OK
    # before the refusals of the shape and of the alignment
    assert _call(L, M=0, K=7) == OK and _call(L, N=0, K=0) == OK and _call(L, N=0, M=99) == OK
    assert _call(L, M=0, x=0x20004) == OK and _call(L, N=0, m=17) == OK


def test_unsupported(L, antq_lib):
    mx = antq_lib.LINEAR4_MM_MAX_M
    assert mx == 64
    assert _call(L, M=mx, x=0x20008) == ALIGN                   # (64 rows are taken: the next refusal is the alignment's)
    assert _call(L, M=65) == UNSUPPORTED and _call(L, M=mx + 1) == UNSUPPORTED and _call(L, M=1000) == UNSUPPORTED
    # float32 belongs to antq_linear4: refused here whatever else holds, after the argument errors and the empty calls
    assert _call(L, dtype=F32) == UNSUPPORTED and _call(L, dtype=F32, M=8) == UNSUPPORTED and _call(L, dtype=F32, x=0x20004) == UNSUPPORTED
    assert _call(L, dtype=F32, M=0) == OK and _call(L, dtype=F32, x=0) == ARG
    for K in (0, 1, 4, 12, 63, 65):
        assert _call(L, K=K) == UNSUPPORTED, K
    assert _call(L, m=17) == UNSUPPORTED
    for nn, m in ((0, 20), (16, 20), (-1, 20), (4, 20), (15, 31), (8, 7)):     # n_normal outside 1..15, > 15 outliers, m < n_normal
        assert _call(L, flags=OVP, n_normal=nn, m=m) == UNSUPPORTED, (nn, m)
    # before the alignment
    assert _call(L, M=mx + 1, x=0x20008) == UNSUPPORTED and _call(L, K=12, codes=0x10001) == UNSUPPORTED
    assert _call(L, m=17, y=0x30001) == UNSUPPORTED


def test_alignment(L):
    for dtype, esz in ((BF16, 2), (F16, 2)):
        for off in (1, 2, 4, 8):
            assert _call(L, dtype=dtype, x=0x20000 + off) == ALIGN, (dtype, off)
        for off in (1, 2, 3):
            assert _call(L, dtype=dtype, codes=0x10000 + off) == ALIGN, (dtype, off)
        for off in range(1, esz):
            assert _call(L, dtype=dtype, y=0x30000 + off) == ALIGN, (dtype, off)
            assert _call(L, dtype=dtype, bias=0x60000 + off) == ALIGN, (dtype, off)
    # OliVe's codebook of 15 + 15 values passes the checks of the shape and is then held to the same alignment
    assert _call(L, flags=OVP, n_normal=15, m=30, x=0x20004) == ALIGN
    assert _call(L, M=8, x=0x20004) == ALIGN and _call(L, M=64, x=0x20004) == ALIGN


def test_constant_in_header_and_binding(antq_lib):
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    assert int(re.search(r"#define ANTQ_LINEAR4_MM_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR4_MM_MAX_M == 64
    assert int(re.search(r"#define ANTQ_LINEAR4_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR4_MAX_M == 8
    assert int(re.search(r"#define ANTQ_ABI_VERSION (\d+)", hdr).group(1)) == antq_lib.ABI_VERSION == 7
    assert re.search(r"\bantq_linear4_mm\s*\(", hdr)


def test_fused_rows_option(antq_lib):
    import torch.nn as nn
    from ant_quantization_amd import packed
    model = nn.Sequential(nn.Linear(8, 8))
    calls = (lambda **kw: packed.pack_model(model, **kw), lambda **kw: packed.PackedBank(model, **kw),
             lambda **kw: packed.load_packed_state_dict(model, {}, **kw))
    for call in calls:
        # without fused_linear
        with pytest.raises(antq_lib.AntqError, match="fused_linear"):
            call(fused_rows=64)
        with pytest.raises(antq_lib.AntqError, match="fused_linear"):
            call(fused_rows=16, fused_linear=False)
        # outside (8, 64]
        for bad in (0, 1, 8, 65, 1000, -3, 16.0, "16", True):
            with pytest.raises(antq_lib.AntqError, match="fused_rows"):
                call(fused_linear=True, fused_rows=bad)


def test_binding_has_the_entry(antq_lib):
    """(that linear4_mm itself refuses float32 and 65 rows needs tensors on a GPU: tests/test_gpu_linear4_mm.py)"""
    assert callable(antq_lib.linear4_mm) and antq_lib.LINEAR4_MM_MAX_M == 64
    assert antq_lib.lib().antq_linear4_mm.argtypes == antq_lib.lib().antq_linear4.argtypes
