"""Which kernel a packed layer's call launches, on the GPU: every `_lib.linear*` is wrapped by a recorder that calls the real
function, a tiny model is packed under each combination of the row options, and per layer and call the function that ran, the
counter that moved and the bits of the output are held to the rule tests/test_packed_routing_host.py states (its `expected`) --
the output is that of the same function called directly on the entry's codes, or of the layer's own product on the image."""
import copy

import pytest

from test_gpu_linear4_t import _conv1d_model, _layer_forward
from test_gpu_linear8 import LINEARS, _input, _tiny, _traced_forward, _trees
from test_packed_routing_host import ROWS_OPTIONS, expected

pytestmark = pytest.mark.gpu

COUNTER_OF = {"linear4": "fused_calls", "linear4_mm": "fused_mm_calls", "linear4_gemm": "fused_gemm_calls", "linear4_t": "fused_t_calls",
              "linear8": "fused_byte_calls", "linear8_mm": "fused_byte_mm_calls", "linear8_gemm": "fused_byte_gemm_calls"}
FOUR = ({}, dict(fused_rows=64), dict(fused_gemm_rows=256), dict(fused_rows=64, fused_gemm_rows=256))
BYTE = ({}, dict(fused_byte_rows=64), dict(fused_byte_gemm_rows=256), dict(fused_byte_rows=64, fused_byte_gemm_rows=256))
CONFIGS = (FOUR + tuple(dict(fused_bytes=True, **o) for o in BYTE)
           + (dict(fused_bytes=True, keep_images=False, **FOUR[3], **BYTE[3]),))
ROWS = (3, 9, 65, 257)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def recorded(antq_lib, monkeypatch):
    """(log of (function name, data_ptr of the codes), the real functions): every linear* of the library records its call"""
    log, real = [], {n: getattr(antq_lib, n) for n in COUNTER_OF}

    def recorder(name):
        def call(codes, *args, **kw):
            log.append((name, codes.data_ptr()))
            return real[name](codes, *args, **kw)
        return call
    for n in COUNTER_OF:
        monkeypatch.setattr(antq_lib, n, recorder(n))
    return log, real


def _direct(real, fn, e, xq, bias):
    """the function called on the entry's own codes, as the bank has to call it"""
    from ant_quantization_amd import packed
    plan, gmax, n_normal, ovp = packed._codebook(e["q"])
    N, K = e["shape"] if e["kind"] == "linear" else e["shape"][::-1]
    return real[fn](e["codes"], xq, e["alpha"], plan.grid_dev(e["device"]), gmax, N, K, e["per_row"], bias=bias, n_normal=n_normal, ovp=ovp)


def _counters(bank):
    return {c: getattr(bank, c) for c in COUNTER_OF.values()}


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float32"])
@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_linear_layers_run_the_kernel_the_rule_names(antq_lib, dev, recorded, tree, dtype_name, capsys):
    import torch
    import torch.nn.functional as F
    _, qutil = _trees(tree)
    log, real = recorded
    dt = getattr(torch, dtype_name)
    base = _tiny(tree, dev, dt)
    xs = {rows: _input(dev, dt, rows, seed=rows) for rows in ROWS}
    with torch.no_grad():
        base(_input(dev, dt, 4))                        # calibration
        twin = copy.deepcopy(base)
        tbank = qutil.pack_model(twin, byte_codes=True)
        images = {e["name"]: e["out"] for e in tbank.entries.values()}
        want = {rows: twin(x) for rows, x in xs.items()}          # F.linear on the images throughout
        assert log == [] and not any(_counters(tbank).values())
        for config in CONFIGS:
            model = copy.deepcopy(base)
            bank = qutil.pack_model(model, fused_linear=True, byte_codes=True, **config)
            opts = {name: config.get(name) for name in ROWS_OPTIONS}
            entries = {e["name"]: e for e in bank.entries.values()}
            assert {n: e["width"] for n, e in entries.items()} == {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}
            assert [n for n, e in entries.items() if e["fusable"]] == ["3", "5"] + (["6"] if config.get("fused_bytes") else [])
            for n, e in entries.items():
                assert (e["out"] is None) == (e["fusable"] and not config.get("keep_images", True)), (config, n)
            layer_of = {e["codes"].data_ptr(): n for n, e in entries.items()}
            for rows, x in xs.items():
                del log[:]
                before = _counters(bank)
                y, seen = _traced_forward(model, x)
                fns = {n: expected("linear", entries[n]["width"], dtype_name, opts, rows) if entries[n]["fusable"] else None for n in LINEARS}
                where = (tree, dtype_name, config, rows)
                # which function ran, per layer, in the model's order
                assert [(fn, layer_of[ptr]) for fn, ptr in log] == [(fns[n], n) for n in LINEARS if fns[n] is not None], where
                # the matching counter, and only it, moved
                moved = {c: v - before[c] for c, v in _counters(bank).items()}
                assert moved == {c: sum(fns[n] == fn for n in LINEARS) for fn, c in COUNTER_OF.items()}, where
                # the bits: the same function on the same codes, or the layer's product on the image
                for n in LINEARS:
                    xq, yn = seen[n]
                    bias = model.get_submodule(n).bias.detach()
                    ref = F.linear(xq, images[n], bias) if fns[n] is None else _direct(real, fns[n], entries[n], xq, bias)
                    assert torch.equal(yn, ref), where + (n,)
                if not any(fns.values()):
                    assert torch.equal(y, want[rows]), where
    capsys.readouterr()


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float32"])
def test_conv1d_layer_runs_its_one_kernel(antq_lib, dev, recorded, dtype_name, capsys):
    import torch
    log, real = recorded
    dt = getattr(torch, dtype_name)
    K, N = 64, 24
    base, qutil = _conv1d_model(dev, dt, K, N)
    gen = torch.Generator(device=dev).manual_seed(5)
    xs = {rows: torch.randn(rows, K, device=dev, generator=gen).to(dt) for rows in (3, 9)}
    with torch.no_grad():
        base(torch.randn(4, K, device=dev, generator=gen).to(dt))       # calibration
        twin = copy.deepcopy(base)
        (te,) = qutil.pack_model(twin).entries.values()
        # (the 4-bit row options do not apply to a conv1d entry: given or not, the same)
        for config in ({}, dict(fused_rows=64, fused_gemm_rows=256), dict(fused_rows=64, fused_gemm_rows=256, keep_images=False)):
            model = copy.deepcopy(base)
            bank = qutil.pack_model(model, fused_linear=True, fused_conv1d=True, **config)
            (e,) = bank.entries.values()
            assert e["kind"] == "conv1d" and e["fusable"] and e["shape"] == (K, N) and (e["out"] is None) == (not config.get("keep_images", True))
            for rows, x in xs.items():
                del log[:]
                before = _counters(bank)
                y, xq = _layer_forward(model, x)
                fn = expected("conv1d", 4, dtype_name, {}, rows)
                assert fn == ("linear4_t" if rows == 3 else None)
                assert log == ([(fn, e["codes"].data_ptr())] if fn else []), (dtype_name, config, rows)
                moved = {c: v - before[c] for c, v in _counters(bank).items()}
                assert moved == {c: int(f == fn) for f, c in COUNTER_OF.items()}, (dtype_name, config, rows)
                bias = model[0].bias.detach()
                ref = torch.addmm(bias, xq, te["out"]) if fn is None else _direct(real, fn, e, xq, bias)
                assert torch.equal(y, ref), (dtype_name, config, rows)
    capsys.readouterr()
