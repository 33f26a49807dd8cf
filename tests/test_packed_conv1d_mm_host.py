"""The option `fused_conv1d_mm` of the packed bank (ant_quantization_amd/packed.py) without a GPU: what it needs switched on, and
which kernel a Conv1D entry's call runs with and without it.  The rule, written here on its own: with the flag on, a fusable
Conv1D entry's bfloat16 / float16 call of 9 .. 64 rows runs `linear4_t_mm`; calls of at most 8 rows keep `linear4_t` in every
dtype; float32 calls beyond 8 rows and calls of more than 64 rows run the layer's own product.  Without the flag -- off, or absent
from a bank built before it existed -- every answer is the one tests/test_packed_routing_host.py states."""
import itertools

import pytest

from test_packed_routing_host import DTYPES, MS, ROWS_OPTIONS, _bare_bank, expected


def _entry(kind, width, dtype_name):
    import torch
    return dict(kind=kind, width=width, dtype=getattr(torch, dtype_name))


def _fn(bank, e, M):
    r = bank._route(e, M)
    return None if r is None else r.fn


def test_the_option_needs_fused_linear_and_fused_conv1d(antq_lib):
    import torch.nn as nn
    from ant_quantization_amd import packed
    model = nn.Sequential(nn.Linear(8, 8))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for who, call in (("pack_model", lambda **o: packed.pack_model(model, **o)),
                      ("PackedBank", lambda **o: packed.PackedBank(model, **o)),
                      ("load_packed_state_dict", lambda **o: packed.load_packed_state_dict(model, {}, **o))):
        with pytest.raises(antq_lib.AntqError, match="fused_conv1d_mm needs fused_linear=True"):
            call(fused_conv1d_mm=True)
        with pytest.raises(antq_lib.AntqError, match="fused_conv1d_mm needs fused_conv1d=True"):
            call(fused_conv1d_mm=True, fused_linear=True)
        with pytest.raises(antq_lib.AntqError, match="needs fused_linear=True"):
            call(fused_conv1d_mm=True, fused_conv1d=True)
        with pytest.raises(antq_lib.AntqError, match="fused_conv1d_mm needs fused_conv1d=True"):
            call(fused_conv1d_mm=1, fused_linear=True, fused_conv1d=False)
    # through load_packed_state_dict the error comes before the model is touched (an empty checkpoint would fail later, differently)
    assert set(model.state_dict()) == set(before) and all((model.state_dict()[k] == v).all() for k, v in before.items())
    assert not hasattr(model, "_antq_no_auto_bank")
    # off is the default and needs nothing
    packed._check_options("pack_model", fused_conv1d_mm=False)
    packed._check_options("pack_model")
    packed._check_options("pack_model", fused_linear=True, fused_conv1d=True, fused_conv1d_mm=True)


def test_the_option_is_a_flag_with_its_route(antq_lib):
    import inspect
    from ant_quantization_amd import packed
    (o,) = [o for o in packed._OPTIONS if o.name == "fused_conv1d_mm"]
    assert o.default is False and o.needs == ("fused_linear", "fused_conv1d") and o.limits is None
    assert inspect.signature(packed.PackedBank.__init__).parameters["fused_conv1d_mm"].default is False
    routes = packed._ROUTES[("conv1d", 4)]
    assert [r.fn for r in routes] == ["linear4_t", "linear4_t_mm"]
    assert routes[0].when is None and routes[1] == packed._Route("linear4_t_mm", "fused_t_mm_calls", "LINEAR4_T_MM_MAX_M", True, "fused_conv1d_mm")
    assert antq_lib.LINEAR4_T_MM_MAX_M == 64 and antq_lib.LINEAR4_T_MAX_M == 8
    # every other route exists unconditionally
    assert all(r.when is None for k, rs in packed._ROUTES.items() for r in rs if r.fn != "linear4_t_mm")


def test_conv1d_routes_with_the_flag_on():
    from ant_quantization_amd import packed
    bank = _bare_bank(packed, fused_conv1d_mm=True)
    for dtype_name in ("bfloat16", "float16"):
        e = _entry("conv1d", 4, dtype_name)
        for M in (9, 16, 33, 64):
            assert _fn(bank, e, M) == "linear4_t_mm", (dtype_name, M)
        assert bank._route(e, 9).counter == "fused_t_mm_calls"
        for M in (65, 256, 4096):
            assert _fn(bank, e, M) is None, (dtype_name, M)
    e32 = _entry("conv1d", 4, "float32")
    for M in (9, 16, 64, 65):
        assert _fn(bank, e32, M) is None, M
    for dtype_name in DTYPES:
        for M in (1, 2, 8):
            assert _fn(bank, _entry("conv1d", 4, dtype_name), M) == "linear4_t", (dtype_name, M)


def test_without_the_flag_the_answers_are_todays():
    from ant_quantization_amd import packed
    for flag in ("absent", False, True):
        for values in itertools.product(*ROWS_OPTIONS.values()):
            opts = dict(zip(ROWS_OPTIONS, values))
            bank = _bare_bank(packed, **opts) if flag == "absent" else _bare_bank(packed, fused_conv1d_mm=flag, **opts)
            for dtype_name, M in itertools.product(DTYPES, MS):
                # Linear entries of either width: unaffected by the flag, whatever it is
                for width in (4, 8):
                    assert _fn(bank, _entry("linear", width, dtype_name), M) == expected("linear", width, dtype_name, opts, M), \
                        (flag, width, dtype_name, opts, M)
                if flag is not True:
                    assert _fn(bank, _entry("conv1d", 4, dtype_name), M) == expected("conv1d", 4, dtype_name, opts, M), (flag, dtype_name, opts, M)
    # a byte-coded Conv1D entry has no route, flag or not
    bank = _bare_bank(packed, fused_conv1d_mm=True)
    assert all(_fn(bank, _entry("conv1d", 8, d), M) is None for d in DTYPES for M in (1, 9, 64))
