"""Which kernel a packed layer's call runs (ant_quantization_amd/packed.py: `_ROUTES`, `PackedBank._route`), without a GPU.

The rule, written here on its own and not read from the table: a fusable entry's call of M rows runs the first kernel, in the
order row kernel / matrix-core kernel / tiled kernel, whose row limit covers M -- the row kernel's is 8 and any dtype; the other
two exist only when their option is given, take what the option says, and serve bfloat16 / float16 only.  4-bit Linear entries
read `fused_rows` and `fused_gemm_rows`, byte-coded ones `fused_byte_rows` and `fused_byte_gemm_rows`, a Conv1D entry has its one
row kernel and reads none.  No kernel: the layer's own product on the image.  The launches: tests/test_gpu_packed_routing.py."""
import inspect
import itertools

import pytest

KINDS = (("linear", 4), ("linear", 8), ("conv1d", 4))
DTYPES = ("float32", "bfloat16", "float16")
ROWS_OPTIONS = {"fused_rows": (None, 9, 64), "fused_gemm_rows": (None, 65, 4096),                 # None, smallest legal, largest
                "fused_byte_rows": (None, 9, 64), "fused_byte_gemm_rows": (None, 65, 4096)}
MS = (1, 8, 9, 32, 33, 64, 65, 256, 257, 4096, 4097)


def expected(kind, width, dtype_name, opts, M):
    """the name of the _lib function, or None: the docstring's sentence"""
    if kind == "conv1d":
        return "linear4_t" if M <= 8 else None
    mm, gemm = ((opts["fused_rows"], opts["fused_gemm_rows"]) if width == 4
                else (opts["fused_byte_rows"], opts["fused_byte_gemm_rows"]))
    if M <= 8:
        return "linear%d" % width
    if dtype_name == "float32":
        return None
    if mm is not None and M <= mm:
        return "linear%d_mm" % width
    if gemm is not None and M <= gemm:
        return "linear%d_gemm" % width
    return None


def _bare_bank(packed, **opts):
    """a bank without a model: `_route` reads the options only"""
    bank = object.__new__(packed.PackedBank)
    for k, v in opts.items():
        setattr(bank, k, v)
    return bank


def test_route_is_the_stated_rule():
    import torch
    from ant_quantization_amd import packed
    points = 0
    for values in itertools.product(*ROWS_OPTIONS.values()):
        opts = dict(zip(ROWS_OPTIONS, values))
        bank = _bare_bank(packed, **opts)
        for (kind, width), dtype_name, M in itertools.product(KINDS, DTYPES, MS):
            e = dict(kind=kind, width=width, dtype=getattr(torch, dtype_name))
            r = bank._route(e, M)
            assert (None if r is None else r.fn) == expected(kind, width, dtype_name, opts, M), (kind, width, dtype_name, opts, M)
            points += 1
    assert points == 3 ** 4 * len(KINDS) * len(DTYPES) * len(MS)
    # the two cases that are easiest to get wrong
    e = dict(kind="linear", width=4, dtype=torch.bfloat16)
    only_mm = _bare_bank(packed, fused_rows=32, fused_gemm_rows=None)
    assert only_mm._route(e, 32).fn == "linear4_mm" and only_mm._route(e, 40) is None
    only_gemm = _bare_bank(packed, fused_rows=None, fused_gemm_rows=256)
    assert [only_gemm._route(e, M).fn for M in (8, 9, 256)] == ["linear4", "linear4_gemm", "linear4_gemm"]
    assert only_gemm._route(e, 257) is None


def test_tables_agree_with_the_bank_and_the_library(antq_lib):
    import torch.nn as nn
    from ant_quantization_amd import packed
    bank = object.__new__(packed.PackedBank)
    with pytest.raises(antq_lib.AntqError, match="no weight quantiser to pack"):
        bank.__init__(nn.Sequential())                 # (nothing to pack: the options and counters are set before that is known)
    routes = [r for rs in packed._ROUTES.values() for r in rs]
    assert sorted(r.fn for r in routes) == sorted(n for n in dir(antq_lib) if n.startswith("linear") and callable(getattr(antq_lib, n)))
    assert len({r.counter for r in routes}) == len(routes)
    for r in routes:
        assert getattr(bank, r.counter) == 0 and type(getattr(bank, r.counter)) is int, r
        assert callable(getattr(antq_lib, r.fn)), r
        # a limit is a constant of the library or an option of the bank
        assert isinstance(getattr(antq_lib, r.limit, None), int) or r.limit in ROWS_OPTIONS, r
    params = inspect.signature(packed.PackedBank.__init__).parameters
    assert set(ROWS_OPTIONS) == {o.name for o in packed._OPTIONS if o.limits}
    for o in packed._OPTIONS:
        assert params[o.name].default == o.default and getattr(bank, o.name) == o.default, o
        assert all(n in params and params[n].default is False for n in o.needs), o
        if o.limits:
            lo, hi = (getattr(antq_lib, c) for c in o.limits)
            assert (lo + 1, hi) == ROWS_OPTIONS[o.name][1:], o


def test_unknown_keywords_are_type_errors(antq_lib):
    import torch.nn as nn
    from ant_quantization_amd import packed
    model = nn.Linear(8, 8)
    with pytest.raises(TypeError, match="nonsense"):
        packed.pack_model(model, nonsense=1)
    with pytest.raises(TypeError, match="codes"):
        packed.pack_model(model, codes={})
    with pytest.raises(TypeError, match="byte_codes"):
        packed.load_packed_state_dict(model, {}, byte_codes=True)       # (the width comes from the stored size)
    with pytest.raises(TypeError, match="nonsense"):
        packed.load_packed_state_dict(model, {}, nonsense=1)
    assert all(p.requires_grad for p in model.parameters()) and set(model.state_dict()) == {"weight", "bias"}      # untouched
