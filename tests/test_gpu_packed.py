"""Packed 4-bit weights on the GPU: the batched decoder (antq_decode4_batch, csrc/antq_k_decbatch.h) against a plain numpy
restatement of include/antq.h on the code bytes, the packed weight bank and the packed checkpoint
(ant_quantization_amd/packed.py).  Every comparison is a bit comparison; where the yardstick is NaN the output must be NaN."""
import copy
import importlib
import types

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


DTYPES = ("float32", "bfloat16", "float16")


def _books():
    """(name, grid as the kernel takes it, gmax, n_normal, pair rule)"""
    G, O = golden("ant_grids.npz"), golden("olive_grids.npz")
    out = [(k, np.ascontiguousarray(G[k], np.float32), float(G[k].max()), 0, False)
           for k in ("flint_b4_s", "int_b4_s", "pot_b4_s", "flint_b4_u", "int_b3_u")]
    for t in ("flint", "int"):
        gn, go = O["%s_b4_s" % t], O["outlier_b4_s"]
        out.append(("olive_" + t, np.ascontiguousarray(np.concatenate([gn, go]), np.float32), float(gn.max()), int(gn.size), True))
    return out


def _round(v, dtype_name):
    """fp32 -> the output type's bits, round to nearest even; NaN positions are compared as NaN."""
    v = np.ascontiguousarray(v, np.float32)
    if dtype_name == "float32":
        return v.view(np.uint32), np.isnan(v)
    if dtype_name == "float16":
        with np.errstate(all="ignore"):
            return v.astype(np.float16).view(np.uint16), np.isnan(v)
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16), np.isnan(v)


def _yardstick(codes, alpha, rows, row_len, per_row, g, gmax, n_normal, ovp, dtype_name):
    """include/antq.h restated on the code bytes: element 2k in the low nibble; with the pair rule nibble 15 -> 0 and its
    partner read from the outlier list; value = fl((g[c] + 0) * (alpha / gmax)) rounded to the output type."""
    gp = np.zeros(48, np.float32)
    gp[:g.size] = g
    gp = gp + np.float32(0)
    b = np.asarray(codes, np.uint8).reshape(-1).astype(np.int64)
    c0, c1 = b & 15, b >> 4
    if ovp:
        q0 = np.where(c0 == 15, np.float32(0), np.where(c1 == 15, gp[n_normal + c0], gp[c0]))
        q1 = np.where(c1 == 15, np.float32(0), np.where(c0 == 15, gp[n_normal + c1], gp[c1]))
    else:
        q0, q1 = gp[c0], gp[c1]
    q = np.stack([q0, q1], 1).astype(np.float32).reshape(rows, row_len)
    with np.errstate(all="ignore"):
        s = (np.asarray(alpha, np.float32).reshape(-1) / np.float32(gmax)).astype(np.float32)
        v = (q * (s.reshape(rows, 1) if per_row else s[0])).astype(np.float32)
    return _round(v, dtype_name)


def _bits(t):
    import torch
    t = t.detach().contiguous()
    return (t.view(torch.int32).cpu().numpy().view(np.uint32) if t.dtype == torch.float32
            else t.view(torch.int16).cpu().numpy().view(np.uint16)).reshape(-1)


def _same(got_bits, want, dtype_name):
    bits, nan = want
    bits, nan = bits.reshape(-1), nan.reshape(-1)
    if dtype_name == "float32":
        got_nan = (got_bits & 0x7fffffff) > 0x7f800000
    elif dtype_name == "bfloat16":
        got_nan = (got_bits & 0x7fff) > 0x7f80
    else:
        got_nan = (got_bits & 0x7fff) > 0x7c00
    return np.array_equal(got_nan, nan) and np.array_equal(got_bits[~nan], bits[~nan])


def test_every_code_byte_at_every_position(antq_lib, dev):
    """All 256 byte values at each of a lane's four code-byte positions (0xFF, 0x?F, 0xF? among them), as rows of 2048
    elements (row tasks: the byte table) and as rows of 64 (lane tasks: the 16-entry form) in one launch per dtype; scales
    ordinary, zero, negative, NaN, Inf, tiny and huge; against the numpy yardstick and antq_decode4 called per job."""
    import torch
    row = np.concatenate([np.roll(np.arange(256, dtype=np.uint8), p) for p in range(4)])          # 1024 bytes = 2048 elements
    alphas = np.float32([1.0, 0.06, 0.0, -0.05, np.nan, np.inf, 1e-30, 1e30, 0.37])
    R = alphas.size
    codes_np = np.ascontiguousarray(np.broadcast_to(row, (R, row.size)))
    for dtype_name in DTYPES:
        dt = getattr(torch, dtype_name)
        jobs, want = [], []
        for name, g, gmax, nn, ovp in _books():
            plan = antq_lib.plan_for(g)
            codes = torch.from_numpy(codes_np).to(dev).reshape(-1)
            a_long = torch.from_numpy(alphas).to(dev)
            a_short = torch.from_numpy(np.repeat(alphas, 32)).to(dev)
            for a, rows, rl in ((a_long, R, 2048), (a_short, R * 32, 64)):
                out = torch.full((rows * rl,), 7.0, dtype=dt, device=dev)
                jobs.append((ovp, (codes, out, a, plan, gmax, rows, rl, True, nn)))
                want.append((name, _yardstick(codes_np, a.cpu().numpy(), rows, rl, True, g, gmax, nn, ovp, dtype_name)))
        for flavour in (False, True):
            sel = [j for o, j in jobs if o == flavour]
            antq_lib.DecodeBatch(sel, ovp=flavour).run()
        torch.cuda.synchronize()
        for (ovp, (codes, out, a, plan, gmax, rows, rl, _, nn)), (name, w) in zip(jobs, want):
            got = _bits(out)
            assert _same(got, w, dtype_name), (name, dtype_name, rl)
            one = antq_lib.decode4(codes, a, plan, gmax, rows, rl, True, dt, n_normal=nn, ovp=ovp)
            assert np.array_equal(_bits(one), got), (name, dtype_name, rl, "antq_decode4")


GUARD = 64          # elements of guard band on either side of every output


def test_shapes_alignment_and_guard_words(antq_lib, dev):
    """The shapes at which the launch structure can go wrong, 61 jobs in one batch per dtype and flavour: one row shorter
    than a vector's lanes, ragged rows, rows of 2 / 3 / 4 vectors per lane with partial last tasks (rows of exactly 128 vectors -- 1024 bf16 / f16, 512 fp32
    elements -- are the ones that take 2), one very long row, a
    per-tensor scale, element counts one octet short of / over a whole task (row and lane tasks), and buffers that start at an
    odd code byte / 2 or 4 bytes off a 16-byte boundary (element-granular tasks).  Random code bytes (every pair form of the
    pair rule among them).  Outputs equal the yardstick; the guard words around every output are untouched."""
    import torch
    rng = np.random.default_rng(11)
    for dtype_name in DTYPES:
        dt = getattr(torch, dtype_name)
        epl = 4 if dtype_name == "float32" else 8
        T = 256 * epl                       # elements of a whole 4-vector task
        shapes = [(1, 8, True, 0), (3, 8, True, 0), (5, 24, True, 0), (64, 768, True, 0), (2, 1032, True, 0), (7, 4104, True, 0),
                  (1, 65544, True, 0), (9, 1024, False, 0), (1, 2 * T - 8, True, 0), (1, 2 * T + 8, True, 0),
                  ((T - 8) // 8, 8, True, 0), ((T + 8) // 8, 8, True, 0), (5, 1024, True, 0), (5, 512, True, 0), (5, 24, True, 1), (3, 2056, True, 1)]
        for name, g, gmax, nn, ovp in (_books()[0], _books()[-2]):
            plan = antq_lib.plan_for(g)
            jobs, checks = [], []
            for rep in range(4):
                for rows, rl, per_row, off in shapes[:15] if rep else shapes:
                    n = rows * rl
                    codes_np = rng.integers(0, 256, n // 2, dtype=np.uint8)
                    if ovp:
                        codes_np[rng.random(n // 2) < 0.1] = 0xFF
                    a_np = np.exp(rng.uniform(-6, 2, rows if per_row else 1)).astype(np.float32)
                    cfull = torch.zeros(n // 2 + 16, dtype=torch.uint8, device=dev)
                    codes = cfull[off:off + n // 2]
                    codes.copy_(torch.from_numpy(codes_np))
                    ofull = torch.full((n + 2 * GUARD + 8,), 3.0, dtype=dt, device=dev)
                    lo = GUARD + off                    # one element: 2 bytes (bf16 / f16) or 4 (fp32) off the 16-byte boundary
                    out = ofull[lo:lo + n]
                    assert (codes.data_ptr() % 4 != 0) == bool(off) and (out.data_ptr() % 16 != 0) == bool(off)
                    jobs.append((codes, out, torch.from_numpy(a_np).to(dev), plan, gmax, rows, rl, per_row, nn))
                    checks.append((ofull, lo, n, _yardstick(codes_np, a_np, rows, rl, per_row, g, gmax, nn, ovp, dtype_name), (rows, rl, off)))
            assert len(jobs) >= 40
            antq_lib.DecodeBatch(jobs, ovp=ovp).run()
            torch.cuda.synchronize()
            guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
            for ofull, lo, n, w, what in checks:
                b = _bits(ofull)
                assert _same(b[lo:lo + n], w, dtype_name), (name, dtype_name, what)
                assert (b[:lo] == guard).all() and (b[lo + n:] == guard).all(), (name, dtype_name, what, "guard words")


def _oracle_in(oracle, x_np, dtype_name):
    """(what the kernels see, the same as the oracle takes it)"""
    if dtype_name == "bfloat16":
        h = oracle.f32_to_bf16(x_np)
        return h, h
    if dtype_name == "float16":
        h = x_np.astype(np.float16)
        return h, h.astype(np.float32)
    return x_np, x_np


def test_round_trip_equals_fakequant_and_the_oracle(antq_lib, oracle, dev):
    """decode4_batch(encode4(x)) == antq_fakequant(x) == the oracle's forward, for x with finite, positive, normal scales and
    |x / scale| within twice the outermost grid value (what include/antq.h promises).  The inputs are first checked on the CPU
    with the oracle alone: g[idx] * s is the oracle's output everywhere, so a failure here is the kernels'."""
    import torch
    rng = np.random.default_rng(23)
    shapes = [(6, 4096), (40, 64), (3, 1032)]
    for dtype_name in DTYPES:
        dt = getattr(torch, dtype_name)
        for name, g, gmax, nn, ovp in _books():
            plan = antq_lib.plan_for(g)
            unsigned = g.min() >= 0
            jobs, refs = [], []
            for rows, rl in shapes:
                a_np = np.exp(rng.uniform(-5, 1, rows)).astype(np.float32)
                s = (a_np / np.float32(gmax)).astype(np.float32)
                lim = 1.9 * float(np.abs(g).max())
                d = rng.standard_normal((rows, rl)).astype(np.float32) * np.float32(0.3 * gmax)
                if ovp:           # planted outliers, both-outlier pairs among them
                    big = rng.random((rows, rl // 2)) < 0.05
                    both = big & (rng.random((rows, rl // 2)) < 0.3)
                    d2 = d.reshape(rows, rl // 2, 2)
                    side = rng.integers(0, 2, (rows, rl // 2))
                    mag = rng.uniform(1.2 * gmax, lim, (rows, rl // 2, 2)).astype(np.float32)
                    for k in (0, 1):
                        m = (big & (side == k)) | both
                        d2[..., k] = np.where(m, mag[..., k] * np.sign(d2[..., k] + 1e-9), d2[..., k])
                d = np.clip(np.abs(d) if unsigned else d, -lim, lim)
                x_np = (d * s[:, None]).astype(np.float32)
                xk, xo = _oracle_in(oracle, x_np, dtype_name)
                ref, ridx = oracle.forward(xo, a_np, g, gmax, ovp)
                if dtype_name == "float16":
                    ref = ref.astype(np.float16)
                # the oracle alone: its output is its own pick's value times the scale, rounded to the output type
                assert (ridx != oracle.IDX_NONE).all()
                q = np.where(ridx == oracle.IDX_VICTIM, np.float32(0), (g + np.float32(0))[np.maximum(ridx, 0)]).astype(np.float32)
                own, _ = _round(q * s[:, None], dtype_name)
                ref_bits = ref.view(np.uint32 if dtype_name == "float32" else np.uint16)
                assert np.array_equal(own, ref_bits), (name, dtype_name, rows, rl, "inputs outside the promised range")
                if ovp:
                    assert (ridx == oracle.IDX_VICTIM).any() and (ridx >= nn).any()
                x = torch.from_numpy(xk.view(np.int16) if xk.dtype != np.float32 else xk).to(dev)
                x = x.view(dt) if xk.dtype != np.float32 else x
                a = torch.from_numpy(a_np).to(dev)
                codes = antq_lib.encode4(x, a, plan, gmax, rows, rl, True, n_normal=nn, ovp=ovp)
                fq = antq_lib.fakequant(x, a, plan, gmax, rows, rl, True, ovp=ovp)
                out = torch.empty(rows * rl, dtype=dt, device=dev)
                jobs.append((codes, out, a, plan, gmax, rows, rl, True, nn))
                refs.append((ref_bits.reshape(-1), fq, (rows, rl)))
            antq_lib.DecodeBatch(jobs, ovp=ovp).run()
            torch.cuda.synchronize()
            for j, (ref_bits, fq, what) in zip(jobs, refs):
                got = _bits(j[1])
                assert np.array_equal(got, _bits(fq)), (name, dtype_name, what, "antq_fakequant")
                assert np.array_equal(got, ref_bits), (name, dtype_name, what, "oracle")


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _trees(tree):
    return (importlib.import_module("ant_quantization_amd.%s.quant_model" % tree),
            importlib.import_module("ant_quantization_amd.%s.quant_utils" % tree))


MODES = {"ant": "ant-int-pot-flint", "olive": "ant-int-flint"}


def _tiny(tree, dev, dt, seed=1):
    """Layers by name: "0" conv with K = 72, "3" linear 64 -> 48, "5" linear 48 -> 64, "6" linear 64 -> 20 set to 8 bits,
    "7" linear with 20 input features (row length no multiple of 8)."""
    import torch
    import torch.nn as nn
    qmod, qutil = _trees(tree)
    qutil.set_quantizer(_args(mode=MODES[tree], wbit=4, abit=4))
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(), nn.Flatten(), nn.Linear(64, 48), nn.ReLU(), nn.Linear(48, 64),
                        nn.Linear(64, 20), nn.Linear(20, 16))
    model = qmod.quantize_model(net)
    assert [n for n, m in model.named_children() if hasattr(m, "quant_weight")] == ["0", "3", "5", "6", "7"]
    qmod.set_8_bit_layer_l(model, "3")           # the fourth (weight, input) pair: layer "6"
    model = model.to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    return model


def _input(dev, dt, seed=0):
    import torch
    return torch.randn(4, 8, 2, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)).to(dt)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_packed_model_forward_schedule_and_checkpoint(antq_lib, dev, tree, dtype_name, tmp_path, capsys):
    import torch
    from ant_quantization_amd import packed
    from ant_quantization_amd.weight_bank import AutoBank
    qmod, qutil = _trees(tree)
    dt = getattr(torch, dtype_name)
    model = _tiny(tree, dev, dt)
    x = _input(dev, dt)
    with torch.no_grad():
        model(x)                                   # calibration
        ref_model = copy.deepcopy(model)
        qutil.set_weight_bank(ref_model, False)    # the fake-quant model: every layer quantises its own weight
        y_ref = ref_model(x)
        bank = qutil.pack_model(model)
        assert isinstance(bank, packed.PackedBank)
        # conv (K = 72), 64 -> 48 and 48 -> 64 are packed; the 8-bit layer and the 20-feature layer stay float, with reasons
        skipped = dict(bank.skipped)
        assert sorted(e["name"] for e in bank.entries.values()) == ["0", "3", "5"] and set(skipped) == {"6", "7"}, bank.skipped
        assert skipped["7"] == "row length 20 is not a multiple of 8"
        assert "values" in skipped["6"], skipped["6"]          # a codebook of 256 values (OliVe: too many normal values)
        assert model._antq_auto_bank.bank is None and not model._antq_auto_bank.enabled
        assert bank.launches == 1                  # one dtype group: one decode launch at construction
        y1 = model(x)
        y2 = model(x)
        assert bank.launches == 1                  # a forward on an unchanged model launches nothing for packed layers
        assert torch.equal(y1, y_ref) and torch.equal(y2, y_ref), (tree, dtype_name)
        bank.invalidate()
        y3 = model(x)
        assert bank.launches == 2 and torch.equal(y3, y_ref)
        for e in bank.entries.values():
            assert e["codes"].dtype == torch.uint8 and e["codes"].numel() == e["mod"].weight.numel() // 2
            assert torch.equal(e["out"], ref_model.get_submodule(e["name"]).quant_weight(ref_model.get_submodule(e["name"]).weight))
    # a forward that wants gradients through a packed quantiser: there is no float weight to train
    with pytest.raises(antq_lib.AntqError):
        model(x)
    # a copy does not silently get an automatic bank back (its forward hook would arm one)
    with torch.no_grad():
        twin = copy.deepcopy(model)
        assert all(m.quant_weight._bank is None for m in twin if hasattr(m, "quant_weight"))
        y_twin = twin(x)
        twin(x)
        assert not isinstance(twin.__dict__.get("_antq_auto_bank"), AutoBank) and torch.equal(y_twin, y_ref)
        assert all(m.quant_weight._bank is None and m.quant_weight._auto_bank is None for m in twin if hasattr(m, "quant_weight"))
        # checkpoint: through torch.save / torch.load into a freshly wrapped, uncalibrated model
        sd = qutil.packed_state_dict(model)
        for n in ("0", "3", "5"):
            assert n + ".weight" not in sd and sd[n + ".quant_weight.codes"].numel() == model.get_submodule(n).weight.numel() // 2
            assert sd[n + ".quant_weight.codes"].dtype == torch.uint8
        assert "6.weight" in sd and "7.weight" in sd and "0.quant_weight.quant_grid" in sd and "0.bias" in sd
        path = str(tmp_path / "packed.pth")
        torch.save(sd, path)
        fresh = _tiny(tree, dev, dt, seed=99)      # other weights: everything must come from the checkpoint
        bank2 = qutil.load_packed_state_dict(fresh, torch.load(path, map_location=dev))
        assert bank2.launches == 1 and sorted(e["name"] for e in bank2.entries.values()) == ["0", "3", "5"]
        assert torch.equal(fresh(x), y_ref), (tree, dtype_name, "checkpoint")
        assert bank2.launches == 1
        for e in bank2.entries.values():           # release_weights: the layer's weight IS the bank's decoded buffer
            assert e["mod"].weight.data_ptr() == e["out"].data_ptr()
        # release_weights on the packed model itself: same storage, same forward
        bank3 = qutil.pack_model(copy.deepcopy(ref_model), release_weights=True)
        m3 = bank3.model
        for e in bank3.entries.values():
            assert e["mod"].weight.data_ptr() == e["out"].data_ptr()
        assert torch.equal(m3(x), y_ref) and torch.equal(m3(x), y_ref) and bank3.launches == 1
    capsys.readouterr()


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_graph_capture_of_invalidate_and_forward(antq_lib, dev, tree):
    """One stream, no parallel branches: bank.invalidate() + a forward captured in a graph (the decode launch is part of it);
    two replays equal the eager forward."""
    import torch
    qmod, qutil = _trees(tree)
    model = _tiny(tree, dev, torch.float32)
    static_x = _input(dev, torch.float32)
    with torch.no_grad():
        model(static_x)                            # calibration
        bank = qutil.pack_model(model)
        y_eager = model(static_x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(static_x)
        torch.cuda.current_stream().wait_stream(side)
        n = bank.launches
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            bank.invalidate()
            static_y = model(static_x)
        assert bank.launches == n + 1              # the decode was captured
        for step in range(2):
            for e in bank.entries.values():
                e["out"].zero_()                   # the replay has to produce the images again
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, y_eager), (tree, step)
        assert bank.launches == n + 1
