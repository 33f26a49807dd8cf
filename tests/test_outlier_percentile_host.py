"""ANT `outlier` mode without a device: np.percentile restated in float32, the forward's numpy reference, argument checks."""
import numpy as np
import pytest

from outlier_cases import F, STEP, inputs, reference


@pytest.mark.parametrize("n", [1, 2, 3, 5, 97, 2304, 10007, 65536, 100003])
def test_percentile_restatement_is_numpys(n):
    from ant_quantization_amd.ant.quant_modules import _percentile_lerp, _percentile_rank
    rng = np.random.default_rng(n)
    a = np.abs(rng.standard_normal(n)).astype(F)
    a[rng.integers(0, n, n // 3)] = a[0]                         # ties
    srt = np.sort(a)
    for q in (0, 12.5, 33.3, 50, 95, 99, 99.9, 99.99, 100):
        k, t = _percentile_rank(n, q)
        got, want = _percentile_lerp(srt[k], srt[min(k + 1, n - 1)], t), np.percentile(a, q)
        assert want.dtype == F and F(got).view(np.uint32) == want.view(np.uint32), (n, q)


def test_nan_in_gives_nan_out():
    from ant_quantization_amd.ant.quant_modules import _outlier_ends
    assert np.isnan(_outlier_ends(np.array([1.0, 3.0, 3.0, 1.0], F), F(0.5))).all()       # as np.percentile / Tensor.max
    assert _outlier_ends(np.array([1.0, 3.0, 4.0, 0.0], F), F(0.25)) == (F(1.5), F(4.0))


@pytest.mark.parametrize("signed", [True, False])
def test_forward_reference_is_defined(signed):
    """The numpy restatement on the GPU test's own inputs: the same bits twice, finite wherever x is."""
    from ant_quantization_amd import grids
    grid = np.asarray(grids.ant_int(4, signed), F)
    x = inputs(2304, F(1.5), F(1.5) / grid.max())
    level = 65535 if signed else 32767
    one, two = (reference(x, F(1.5), F(1.5) + F(level) * STEP, grid, level, True) for _ in range(2))
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))
    assert np.all(np.isfinite(one[np.isfinite(x)])) and np.isnan(x).any() and np.isinf(x).any()


def test_argument_checks_need_no_device(antq_lib):
    L, plan = antq_lib.lib(), antq_lib.plan_for(np.arange(-8, 8, dtype=F))
    ARG, UNSUPPORTED, PLAN, ALIGN = -1, -2, -3, -5
    p = 4096                                                     # (never dereferenced: every call below is refused first)
    def fq(x=p, out=p, n=8, p4=p, p16=p, plan_host=plan.host_addr, grid=None, m=16, level=65535, flags=8, dtype=antq_lib.F32):
        return L.antq_fakequant_outlier(x, out, n, p4, p16, 7.0, plan_host, p, grid, m, level, flags, dtype, None)

    assert [fq(x=None), fq(p16=None), fq(n=0), fq(level=0), fq(flags=1), fq(grid=p, m=15)] == [ARG] * 6
    assert [fq(dtype=antq_lib.BF16), fq(dtype=antq_lib.F16), fq(dtype=antq_lib.F64)] == [UNSUPPORTED] * 3
    assert [fq(x=p + 2), fq(out=p + 1), fq(p4=p + 2), fq(grid=p + 2)] == [ALIGN] * 4
    assert fq(plan_host=np.zeros(256, np.uint8).ctypes.data) == PLAN
    def os_(x=p, n=8, k=0, stats=p, ws=p, dtype=antq_lib.F32):
        return L.antq_abs_order_stats(x, n, k, stats, ws, dtype, None)

    assert [os_(x=None), os_(stats=None), os_(ws=None), os_(n=0), os_(k=8)] == [ARG] * 5
    assert [os_(dtype=antq_lib.BF16), os_(n=2 ** 32), os_(n=2 ** 32 + 5, k=7)] == [UNSUPPORTED] * 3
    assert [os_(x=p + 2), os_(stats=p + 1)] == [ALIGN] * 2
