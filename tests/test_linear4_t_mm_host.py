"""antq_linear4_t_mm (the matrix-core packed 4-bit linear for [K, N] weights, GPT-2's Conv1D) on the host: every refusal of
include/antq.h in the stated order, through ctypes with null or made-up pointers (the entry point validates before it touches HIP:
callable on a CPU-only box), the constant shared by header and binding, the bound argument types, and the binding's own refusals."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -5
F32, BF16, F16 = 0, 1, 2
OVP = 1


def _call(L, **kw):
    a = dict(codes=0x10000, x=0x20000, bias=0, y=0x30000, M=9, N=16, K=64, alpha=0x40000, per_row=1, gmax=10.0, grid=0x50000,
             m=16, n_normal=0, flags=0, dtype=BF16)
    a.update(kw)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    f = L.antq_linear4_t_mm
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
    # ... and they come first: with an empty call, f32, an unsupported shape or a misaligned pointer as well
    assert _call(L, x=0, M=0) == ARG and _call(L, dtype=9, N=0) == ARG and _call(L, flags=8, M=99, K=7) == ARG
    assert _call(L, codes=0, x=0x20001) == ARG and _call(L, m=0, M=0) == ARG and _call(L, m=0, flags=OVP, N=12) == ARG
    assert _call(L, grid=0, N=12, y=0x30001) == ARG and _call(L, alpha=0, dtype=F32) == ARG


def test_empty_calls_launch_nothing(L):
    assert _call(L, M=0) == OK and _call(L, N=0) == OK
    # before the refusals of the dtype, of the shape and of the alignment
    assert _call(L, M=0, dtype=F32) == OK and _call(L, N=0, dtype=F32) == OK
    assert _call(L, M=0, K=7) == OK and _call(L, N=0, K=0) == OK and _call(L, N=0, M=99) == OK and _call(L, M=0, N=12) == OK
    assert _call(L, M=0, x=0x20004) == OK and _call(L, N=0, m=17) == OK and _call(L, M=0, N=1 << 31) == OK


def test_unsupported(L, antq_lib):
    mx = antq_lib.LINEAR4_T_MM_MAX_M
    assert mx == 64
    # f32, stated as for antq_linear4_mm: whatever else the call is
    assert _call(L, dtype=F32) == UNSUPPORTED and _call(L, dtype=F32, M=1) == UNSUPPORTED and _call(L, dtype=F32, x=0x20004) == UNSUPPORTED
    assert _call(L, M=mx + 1) == UNSUPPORTED and _call(L, M=1000) == UNSUPPORTED
    for K in (0, 1, 4, 12, 63, 65):
        assert _call(L, K=K) == UNSUPPORTED, K
    for N in (1, 2, 4, 12, 63, 65, 68):
        assert _call(L, N=N) == UNSUPPORTED, N
    assert _call(L, m=17) == UNSUPPORTED
    for nn, m in ((0, 20), (16, 20), (-1, 20), (4, 20), (15, 31), (8, 7)):     # n_normal outside 1..15, > 15 outliers, m < n_normal
        assert _call(L, flags=OVP, n_normal=nn, m=m) == UNSUPPORTED, (nn, m)
    assert _call(L, N=1 << 31) == UNSUPPORTED and _call(L, K=1 << 31) == UNSUPPORTED and _call(L, N=1 << 33, K=1 << 32) == UNSUPPORTED
    # before the alignment
    assert _call(L, M=mx + 1, x=0x20008) == UNSUPPORTED and _call(L, K=12, codes=0x10001) == UNSUPPORTED
    assert _call(L, m=17, y=0x30001) == UNSUPPORTED and _call(L, N=12, x=0x20002) == UNSUPPORTED
    assert _call(L, K=1 << 31, bias=0x60001) == UNSUPPORTED


def test_alignment(L, antq_lib):
    for dtype in (BF16, F16):
        for off in (1, 2, 4, 8):
            assert _call(L, dtype=dtype, x=0x20000 + off) == ALIGN, (dtype, off)
        for off in (1, 2, 3):
            assert _call(L, dtype=dtype, codes=0x10000 + off) == ALIGN, (dtype, off)
        assert _call(L, dtype=dtype, y=0x30001) == ALIGN and _call(L, dtype=dtype, bias=0x60001) == ALIGN
    # the most rows, every row count at a tile's edge and OliVe's codebook of 15 + 15 values pass the checks of the shape and are
    # then held to the same alignment: M = 64 is accepted up to here, 65 is not (test_unsupported)
    for M in (1, 8, 9, 16, 17, 32, 33, 48, 49, antq_lib.LINEAR4_T_MM_MAX_M):
        assert _call(L, M=M, x=0x20004) == ALIGN, M
    assert _call(L, flags=OVP, n_normal=15, m=30, x=0x20004) == ALIGN
    assert _call(L, N=8, K=8, codes=0x10002) == ALIGN and _call(L, N=136, K=8200, y=0x30001) == ALIGN


def test_constant_in_header_and_binding(antq_lib):
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    assert int(re.search(r"#define ANTQ_LINEAR4_T_MM_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR4_T_MM_MAX_M == 64
    assert re.search(r"\bint\s+antq_linear4_t_mm\s*\(", hdr)
    assert int(re.search(r"#define ANTQ_ABI_VERSION (\d+)", hdr).group(1)) == antq_lib.ABI_VERSION == 7       # an added entry point


def test_argtypes_are_bound(antq_lib):
    L = antq_lib.lib()
    assert L.antq_linear4_t_mm.restype is ctypes.c_int
    assert L.antq_linear4_t_mm.argtypes is not None and list(L.antq_linear4_t_mm.argtypes) == list(L.antq_linear4.argtypes)
    assert len(L.antq_linear4_t_mm.argtypes) == 16
    assert callable(antq_lib.linear4_t_mm)
    assert antq_lib._LINEARS["linear4_t_mm"] == antq_lib._Linear("antq_linear4_t_mm", antq_lib.LINEAR4_T_MM_MAX_M, False, 2, True)


class _Fake:
    """what _lib looks at before the library is called: a tensor that claims to live on the GPU"""

    def __init__(self, dtype, *shape, device="cuda:0"):
        import torch
        self.dtype, self.shape, self.is_cuda, self.device = dtype, tuple(shape), True, torch.device(device)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


def test_the_binding_refuses_before_the_library(antq_lib):
    """fp32, 65 rows and a wrong codes size raise AntqError in the binding: nothing is launched (there is no GPU here)."""
    import torch
    N, K = 16, 64
    good = dict(codes=_Fake(torch.uint8, N * K // 2), alpha=_Fake(torch.float32, K), grid=_Fake(torch.float32, 16))

    def call(x, codes=good["codes"], alpha=good["alpha"]):
        return antq_lib.linear4_t_mm(codes, x, alpha, good["grid"], 10.0, N, K, True)

    with pytest.raises(antq_lib.AntqError, match="unsupported dtype torch.float32"):
        call(_Fake(torch.float32, 9, K))
    with pytest.raises(antq_lib.AntqError, match="unsupported dtype torch.float64"):
        call(_Fake(torch.float64, 9, K))
    with pytest.raises(antq_lib.AntqError, match="antq_linear4_t_mm takes at most 64 rows of x \\(got 65\\)"):
        call(_Fake(torch.bfloat16, 65, K))
    with pytest.raises(antq_lib.AntqError, match="antq_linear4_t_mm takes at most 64 rows"):
        call(_Fake(torch.float16, 5, 13, K))
    with pytest.raises(antq_lib.AntqError, match="codes must be uint8 of N\\*K/2 bytes"):
        call(_Fake(torch.bfloat16, 9, K), codes=_Fake(torch.uint8, N * K))
    with pytest.raises(antq_lib.AntqError, match="codes must be uint8"):
        call(_Fake(torch.bfloat16, 9, K), codes=_Fake(torch.int8, N * K // 2))
    with pytest.raises(antq_lib.AntqError, match="x must be"):
        call(_Fake(torch.bfloat16, 9, K + 8))
    with pytest.raises(antq_lib.AntqError, match="alpha must be float32"):          # K scales, one per row k of the codes
        call(_Fake(torch.bfloat16, 9, K), alpha=_Fake(torch.float32, N))
