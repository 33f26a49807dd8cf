"""antq_fakequant_outlier: the fused forward of ANT's `outlier` mode, bit for bit against the numpy restatement of
AQ:438-465 (outlier_cases.reference) and against the reference's own recorded outputs."""
import types

import numpy as np
import pytest

from conftest import golden
from outlier_cases import F, STEP, inputs, reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0") if torch.cuda.is_available() else pytest.skip("no GPU")


def f32_same(a, b):
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _check(antq_lib, dev, n, signed, tail, p4, p16, stale=False):
    """stale: the grid buffer holds flint while plan and gmax describe int -- the kernel must quantise to the buffer."""
    from ant_quantization_amd import grids
    grid = np.asarray(grids.ant_int(4, signed), F)
    held = np.asarray(grids.ant_flint(4, signed), F) if stale else grid
    level = 65535 if signed else 32767
    x = inputs(n, F(1.5), F(1.5) / held.max())
    want = reference(x, p4, p16, held, level, tail)
    plan, t4, t16 = antq_lib.plan_for(grid), torch.tensor([p4], device=dev), torch.tensor([p16], device=dev)
    gdev = torch.from_numpy(held.copy()).to(dev)
    for x_off, o_off in ((0, 0), (1, 1), (0, 1), (0, None)):          # aligned, base + 4 bytes, mixed, in place
        xt = torch.zeros(n + 1, device=dev)[x_off:x_off + n].copy_(torch.from_numpy(x))
        out = xt if o_off is None else torch.zeros(n + 1, device=dev)[o_off:o_off + n]
        got = antq_lib.fakequant_outlier(xt, t4, t16, plan, float(grid.max()), signed, tail, out=out, grid=gdev)
        assert got.data_ptr() == out.data_ptr()
        assert f32_same(got.cpu().numpy(), want), (x_off, o_off)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 2304])    # 1024 = 64 lanes * 4 * kOutlierU
@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("signed", [True, False])
def test_forward_bits(antq_lib, dev, n, signed, tail):
    _check(antq_lib, dev, n, signed, tail, F(1.5), F(1.5) + F(65535 if signed else 32767) * STEP)


@pytest.mark.parametrize("p4,p16,stale", [(0.0, 3.0, False), (np.nan, 3.0, False), (1.5, 1.5, False), (1.5, 65.0, True)],
                         ids=["p4_zero", "p4_nan", "step_zero", "stale_plan"])
@pytest.mark.parametrize("signed", [True, False])
def test_forward_scalar_cases(antq_lib, dev, signed, p4, p16, stale):
    for n in (5, 257, 2304):
        _check(antq_lib, dev, n, signed, True, F(p4), F(p16), stale)


def test_module_matches_reference_outputs(antq_lib, dev, monkeypatch, capsys):
    """TensorQuantizer(mode='outlier') on the reference's recorded tensors: bit for bit, every forward one fused launch."""
    from ant_quantization_amd.ant import quant_modules as qm
    calls, real = [], antq_lib.fakequant_outlier
    monkeypatch.setattr(antq_lib, "fakequant_outlier", lambda *a, **k: calls.append(1) or real(*a, **k))
    o = golden("ant_outlier.npz")
    x = torch.from_numpy(o["x"]).to(dev)
    for pct in (99, 95):
        for signed in (True, False):
            xx = x if signed else x.abs()
            args = types.SimpleNamespace(w_up=150, a_up=150, w_low=75, a_low=75, percent=float(pct), search=False, no_outlier=False)
            q = qm.TensorQuantizer(mode="outlier", bit=4, is_signed=signed, is_enable=True, is_input=not signed, args=args).to(dev)
            q.name = "golden"
            k = "p%d_%s" % (pct, "s" if signed else "u")
            assert f32_same(q(xx).cpu().numpy(), o[k + "_out"]), k
            assert f32_same(q(xx * 0.5).cpu().numpy(), o[k + "_out2"]), k
            assert q.percent_value_int4.item() == np.percentile(np.abs(xx.cpu().numpy()), q.percent * 100)
    assert len(calls) == 8
    capsys.readouterr()
