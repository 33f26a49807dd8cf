"""The tiled [K, N] packed linear (antq_linear4_t_gemm) on the host: the bank's option and its route, and the row limit the
binding and the header share.  The launches: tests/test_gpu_linear4_t_gemm.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("given, missing", [({}, "fused_linear"), ({"fused_linear": True}, "fused_conv1d")])
def test_the_option_needs_fused_linear_and_fused_conv1d(antq_lib, given, missing):
    import torch.nn as nn
    from ant_quantization_amd import packed
    want = "fused_conv1d_gemm needs %s=True" % missing
    with pytest.raises(antq_lib.AntqError, match=want):
        packed.PackedBank(nn.Linear(8, 8), fused_conv1d_gemm=True, **given)
    with pytest.raises(antq_lib.AntqError, match=want):
        packed.load_packed_state_dict(nn.Linear(8, 8), {}, fused_conv1d_gemm=True, **given)


def test_route(antq_lib):
    import torch
    from ant_quantization_amd import packed

    def fn(dtype, M, **flags):
        bank = object.__new__(packed.PackedBank)         # (a bank without a model: _route reads the options only)
        for k, v in flags.items():
            setattr(bank, k, v)
        r = bank._route(dict(kind="conv1d", width=4, dtype=dtype), M)
        return None if r is None else r.fn

    bf = torch.bfloat16
    assert [fn(bf, M, fused_conv1d_gemm=True) for M in (8, 9, 4096, 4097)] == ["linear4_t", "linear4_t_gemm", "linear4_t_gemm", None]
    both = dict(fused_conv1d_gemm=True, fused_conv1d_mm=True)
    assert [fn(bf, M, **both) for M in (9, 64, 65)] == ["linear4_t_mm", "linear4_t_mm", "linear4_t_gemm"]
    assert [fn(torch.float32, M, **both) for M in (8, 9, 65)] == ["linear4_t", None, None]
    assert [fn(bf, M, fused_conv1d_gemm=False) for M in (9, 65)] == [None, None]


def test_row_limit_is_the_header_s(antq_lib):
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    assert int(re.search(r"#define ANTQ_LINEAR4_T_GEMM_MAX_M (\d+)", hdr).group(1)) == antq_lib.LINEAR4_T_GEMM_MAX_M == 4096
    assert antq_lib._LINEARS["linear4_t_gemm"] == antq_lib._Linear("antq_linear4_t_gemm", 4096, False, 2, True)
