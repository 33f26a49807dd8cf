"""Byte codes on the GPU: antq_encode8 against the CPU oracle's indices, antq_decode8 / antq_decode8_batch against the numpy
restatement of include/antq.h (byte_codes_cases.decode_ref), the round trip against antq_fakequant and the oracle, every launch
form, and the module surface (pack_model(byte_codes=True), checkpoints).  Every comparison is a bit comparison.  The inputs
come from byte_codes_cases.py, which test_byte_codes_host.py holds to their conditions without a GPU."""
import contextlib
import copy
import importlib
import types

import numpy as np
import pytest

import byte_codes_cases as bc
import encode4_cases as ec

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {1: 0, 4: 1}
GUARD = 64                     # elements / bytes of poison on either side of every output


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def knobs(antq_lib, **kv):
    keys = [int(k[1:]) for k in kv]
    try:
        for k, v in zip(keys, kv.values()):
            antq_lib.lib().antq_debug_set(k, v)
        yield
    finally:
        for k in keys:
            antq_lib.lib().antq_debug_set(k, KNOB_DEFAULTS[k])


def _tensor(xk, dtype_name, dev, lead=0):
    """The kernel's input on the device; lead: elements by which it starts off a 16-byte boundary."""
    import torch
    dt = getattr(torch, dtype_name)
    src = torch.from_numpy(np.ascontiguousarray(xk).reshape(-1).view(np.int32 if dtype_name == "float32" else np.int16))
    full = torch.zeros(src.numel() + 16, dtype=src.dtype, device=dev)
    assert full.data_ptr() % 16 == 0
    t = full[lead:lead + src.numel()]
    t.copy_(src)
    return t.view(dt)


def _bits(t):
    import torch
    t = t.detach().contiguous()
    return (t.view(torch.int32).cpu().numpy().view(np.uint32) if t.dtype == torch.float32
            else t.view(torch.int16).cpu().numpy().view(np.uint16)).reshape(-1)


def _alpha(a, dev):
    import torch
    return torch.from_numpy(np.atleast_1d(np.asarray(a, np.float32))).to(dev)


def _guarded(n, dt, dev, lead=0):
    """(buffer of poison, start, view of n elements `lead` elements off a 16-byte boundary)"""
    import torch
    full = torch.full((n + 2 * GUARD + 16,), 3.0, dtype=dt, device=dev)
    esz = full.element_size()
    lo = GUARD + (-(full.data_ptr() // esz + GUARD)) % (16 // esz) + lead
    out = full[lo:lo + n]
    assert (out.data_ptr() % 16) == lead * esz
    return full, lo, out


def _guards_intact(full, lo, n):
    import torch
    b = _bits(full)
    g = _bits(torch.full((1,), 3.0, dtype=full.dtype))[0]
    return bool((b[:lo] == g).all() and (b[lo + n:] == g).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 1: every byte
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", bc.DTYPES)
@pytest.mark.parametrize("name", ["int_b8_s", "flint_b6_s", "olive_int_b8", "olive_u4", "ladder_plain", "ladder_pairs"])
def test_every_byte_decodes_by_the_rule(antq_lib, oracle, dev, name, dtype_name):
    """All 256 byte values at every position of a code word (plain books) / all 65 536 ordered pairs (pair rule), as rows of
    4, 8 and 1024 elements, per-row and per-tensor awkward scales: antq_decode8 and ONE antq_decode8_batch launch over all
    layouts equal the numpy rule to the bit, between poisoned guard words."""
    import torch
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    dt = getattr(torch, dtype_name)
    if ovp:
        c = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(-1).astype(np.uint8)     # 131 072 elements
    else:
        c = np.concatenate([np.roll(np.arange(256, dtype=np.uint8), p) for p in range(8)])                            # 2048 elements
    assert c.size % 1024 == 0
    rng = np.random.default_rng(3)
    plan = antq_lib.plan_for(g)
    codes = torch.from_numpy(c).to(dev)
    jobs, checks = [], []
    for rl in (4, 8, 1024):
        rows = c.size // rl
        for per_row in (True, False):
            a_np = ec.awkward_alpha(rng, rows if per_row else 1)
            a = _alpha(a_np, dev)
            r, k = (rows, rl) if per_row else (1, c.size)
            want = bc.decode_ref(oracle, c, a_np, bk, r, k, dtype_name).reshape(-1)
            full, lo, out = _guarded(c.size, dt, dev)
            antq_lib.decode8(codes, a, plan, gmax, r, k, per_row, dt, n_normal=nn, ovp=ovp, out=out)
            assert np.array_equal(_bits(out), want), (name, dtype_name, rl, per_row, "antq_decode8")
            assert _guards_intact(full, lo, c.size), (name, dtype_name, rl, per_row, "guard words")
            fullb, lob, outb = _guarded(c.size, dt, dev)
            jobs.append((codes, outb, a, plan, gmax, r, k, per_row, nn))
            checks.append((fullb, lob, outb, want, (rl, per_row)))
    antq_lib.DecodeBatch(jobs, ovp=ovp, width=8).run()
    torch.cuda.synchronize()
    for full, lo, out, want, what in checks:
        assert np.array_equal(_bits(out), want), (name, dtype_name, what, "antq_decode8_batch")
        assert _guards_intact(full, lo, c.size), (name, dtype_name, what, "guard words")


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the encoder at its decision edges
# ---------------------------------------------------------------------------------------------------------------------------
FORMS = ((), (("k4", 0),))           # the plan's approximate-quotient table where it has one / the d-domain table with exact division


def _encode(antq_lib, dev, xt, alpha, bk, rows, rl, per_row=True, out=None):
    _, g, gmax, nn, ovp = bk
    return antq_lib.encode8(xt, _alpha(alpha, dev), antq_lib.plan_for(g), gmax, rows, rl, per_row, n_normal=nn, ovp=ovp, out=out)


def _codes_equal(antq_lib, oracle, dev, bk, x, alpha, dtype_name="float32", forms=FORMS, per_row=True, tag=()):
    rows, rl = x.shape
    xk, xf = ec.as_dtype(oracle, x, dtype_name)
    want = bc.oracle_codes(oracle, xf if per_row else xf.reshape(1, -1), alpha, bk).reshape(-1)
    xt = _tensor(xk, dtype_name, dev)
    for form in forms:
        with knobs(antq_lib, **dict(form)):
            got = _encode(antq_lib, dev, xt, alpha, bk, rows, rl, per_row).cpu().numpy().astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bk[0], dtype_name, rows, rl, form) + tuple(tag) + (
            "%d of %d codes differ" % (bad.size, got.size), "at", bad[:6].tolist(),
            "x bits", [hex(int(v)) for v in np.ascontiguousarray(xf, np.float32).reshape(-1).view(np.uint32)[bad[:6]]],
            "got", got[bad[:6]].tolist(), "want", want[bad[:6]].tolist())


@pytest.mark.parametrize("name", bc.BOOK_NAMES)
def test_codes_around_every_threshold(antq_lib, oracle, dev, name):
    """+/-16 ulps around fl(midpoint * scale) of every pair of adjacent distinct values, rows of 508 (units of four elements)
    and 1032 (octets): fp32 through both plan forms, and the same values rounded to bf16 / f16 (widened exactly)."""
    bk = bc.book(name)
    for rl in bc.THRESHOLD_ROW_LENS:
        case = bc.threshold_input(name, rl)
        _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"])
        for dtype_name in ("bfloat16", "float16"):
            _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"], dtype_name=dtype_name, forms=((),))


@pytest.mark.parametrize("name", bc.OLIVE_NAMES)
def test_pair_rule_at_the_outlier_boundary(antq_lib, oracle, dev, name):
    bk = bc.book(name)
    case = bc.pair_input(name)
    _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"])


@pytest.mark.parametrize("name", bc.BOOK_NAMES)
def test_magnitudes_specials_horizon_and_the_literal_scan(antq_lib, oracle, dev, name):
    """Both signs of every fp32 exponent, +/-0, +/-Inf, NaNs, subnormals, the magnitude at which the oracle's index turns into
    IDX_NONE (those encode as the zero code), odd scales -- and octets of which one half is NaN / Inf / far-clipped, which
    sends the whole unit through the literal scan."""
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    for rl in (500, 504):
        case = ec.magnitude_case(oracle, np.random.default_rng(3), g, gmax, rl)
        _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"], tag=("magnitudes",))
    case = ec.split_octet_case(np.random.default_rng(29), g, gmax, 504, n_scales=4)
    _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"], tag=("split octets",))
    for dtype_name in ("bfloat16", "float16"):
        _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"], dtype_name=dtype_name, forms=((),), tag=("split octets",))


# ---------------------------------------------------------------------------------------------------------------------------
# 3: round trip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", bc.DTYPES)
@pytest.mark.parametrize("name", bc.BOOK_NAMES)
def test_round_trip_equals_fakequant_and_the_oracle(antq_lib, oracle, dev, name, dtype_name):
    """decode8(encode8(w)) == antq_fakequant(w) == the oracle, as bit patterns: rows of 4 ... 4100 elements, 1 / 3 / 257 rows,
    and one scale per tensor on a single row."""
    import torch
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    dt = getattr(torch, dtype_name)
    plan = antq_lib.plan_for(g)
    for rows in bc.ROW_COUNTS:
        for rl in bc.ROW_LENS:
            xk, xf, a_np = bc.round_trip_input(name, dtype_name, rows, rl, oracle)
            for per_row in ((True, False) if rows == 1 else (True,)):
                al = a_np if per_row else a_np[:1]
                with np.errstate(all="ignore"):
                    ref, _ = oracle.forward(xf, al if per_row else al[0], g, gmax, ovp)
                want = bc.to_bits(oracle, ref, dtype_name).reshape(-1)
                x, a = _tensor(xk, dtype_name, dev), _alpha(al, dev)
                codes = antq_lib.encode8(x, a, plan, gmax, rows, rl, per_row, n_normal=nn, ovp=ovp)
                assert codes.dtype == torch.uint8 and codes.numel() == rows * rl
                got = _bits(antq_lib.decode8(codes, a, plan, gmax, rows, rl, per_row, dt, n_normal=nn, ovp=ovp))
                fq = _bits(antq_lib.fakequant(x, a, plan, gmax, rows, rl, per_row, ovp=ovp))
                tag = (name, dtype_name, rows, rl, per_row)
                assert np.array_equal(got, fq), tag + ("antq_fakequant", int((got != fq).sum()))
                assert np.array_equal(got, want), tag + ("oracle", int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# 4: launch forms
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_shapes(dtype_name):
    """(rows, row_len): both sides of every task size.  Decoder: 128 vectors (row tasks from there), 64 u vectors per row task,
    256 vectors / quads per task of the per-lane kinds.  Encoder: 512 units of 8 or 4 elements per task with vector loads, 256
    without."""
    epl = 4 if dtype_name == "float32" else 8
    shapes = [(2, v * epl) for v in (127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385)]
    shapes += [(u, epl) for u in (255, 256, 257)] + [(u, 4) for u in (255, 256, 257, 511, 512, 513)]
    shapes += [(u, 8) for u in (511, 512, 513)] + [(3, 20), (5, 12), (1, 4)]
    return shapes


@pytest.mark.parametrize("dtype_name", bc.DTYPES)
@pytest.mark.parametrize("name", ["int_b8_s", "olive_int_b8"])
def test_task_edges_unaligned_buffers_and_footprint(antq_lib, oracle, dev, name, dtype_name):
    """Every task-size edge (one below, at, one above); x on a 16-byte boundary and one element behind it; codes written and
    read at byte offsets 0 ... 3 inside a buffer of 0xA5; outputs on a 16-byte boundary and one element behind it between
    poisoned guard words.  Codes equal the oracle's, the decoded image equals the numpy rule, no guard changed."""
    import torch
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    dt = getattr(torch, dtype_name)
    plan = antq_lib.plan_for(g)
    rng = np.random.default_rng(53)
    for i, (rows, rl) in enumerate(_edge_shapes(dtype_name)):
        n = rows * rl
        case = ec.random_case(rng, rows, rl, g, gmax, ovp)
        xk, xf = ec.as_dtype(oracle, case["x"], dtype_name)
        want = bc.oracle_codes(oracle, xf, case["alpha"], bk).reshape(-1)
        want_img = bc.decode_ref(oracle, want, case["alpha"], bk, rows, rl, dtype_name).reshape(-1)
        a = _alpha(case["alpha"], dev)
        for lead, off in ((0, 0), (1, 1), (0, 2), (1, 3)) if i % 3 == 0 else ((0, 0), (i % 2, 1 + i % 3)):
            xt = _tensor(xk, dtype_name, dev, lead)
            cfull = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device=dev)
            lo = GUARD + (-(cfull.data_ptr() + GUARD)) % 16 + off
            cview = cfull[lo:lo + n]
            assert cview.data_ptr() % 4 == off
            got = antq_lib.encode8(xt, a, plan, gmax, rows, rl, True, n_normal=nn, ovp=ovp, out=cview)
            tag = (name, dtype_name, rows, rl, "x lead", lead, "codes offset", off)
            assert got.data_ptr() == cview.data_ptr()
            f = cfull.cpu().numpy()
            assert np.array_equal(f[lo:lo + n].astype(np.int64), want), tag
            assert (f[:lo] == 0xA5).all() and (f[lo + n:] == 0xA5).all(), tag + ("guard bytes",)
            full, olo, out = _guarded(n, dt, dev, lead)
            antq_lib.decode8(cview, a, plan, gmax, rows, rl, True, dt, n_normal=nn, ovp=ovp, out=out)
            assert np.array_equal(_bits(out), want_img), tag + ("decode",)
            assert _guards_intact(full, olo, n), tag + ("guard words",)


@pytest.mark.parametrize("name", ["flint_b6_s", "olive_int_b8"])
def test_persistent_encoder_workgroups_loop(antq_lib, oracle, dev, name):
    """A tensor of 6.9 tasks (octets) / 13.8 tasks (rows of 20: units of four) encoded by 1, 3 and 7 persistent workgroups."""
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    for rows, rl in (ec.LOOP_SHAPE, (1411, 20)):
        case = ec.random_case(np.random.default_rng(41), rows, rl, g, gmax, ovp)
        _codes_equal(antq_lib, oracle, dev, bk, case["x"], case["alpha"], forms=((("k1", 1),), (("k1", 3),), (("k1", 7),)))


# ---------------------------------------------------------------------------------------------------------------------------
# 5: batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", bc.DTYPES)
@pytest.mark.parametrize("ovp", [False, True])
def test_batch_equals_singles_twice_and_in_a_graph(antq_lib, oracle, dev, ovp, dtype_name):
    """One launch over 14 jobs -- row, short-row and unaligned kinds, per-row and per-tensor scales, two books -- equals
    antq_decode8 per job to the bit; a second launch of the same blob and one replay of it captured in a graph do too."""
    import torch
    dt = getattr(torch, dtype_name)
    epl = 4 if dtype_name == "float32" else 8
    rng = np.random.default_rng(71)
    names = ("olive_int_b8", "olive_u4") if ovp else ("int_b8_s", "flint_b6_s")
    shapes = [(3, 200 * epl, True, 0, 0), (2, 129 * epl, True, 0, 0), (5, 260, True, 0, 0), (40, 64, True, 0, 0), (7, 20, True, 0, 0),
              (4, 1024, False, 0, 0), (9, 64, False, 0, 0), (3, 2052, True, 1, 0), (6, 64, True, 3, 0), (3, 1024, True, 0, 1),
              (1, 4, True, 0, 0), (257, 12, True, 2, 1), (2, 4100, True, 0, 0), (1, 513 * epl, False, 0, 0)]
    jobs, singles, kinds = [], [], set()
    for i, (rows, rl, per_row, coff, lead) in enumerate(shapes):
        _, g, gmax, nn, _ = bk = bc.book(names[i % 2])
        plan = antq_lib.plan_for(g)
        n = rows * rl
        c_np = rng.integers(0, 256, n, dtype=np.uint8)
        if ovp:
            c_np[rng.random(n) < 0.1] = 255
        cfull = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
        codes = cfull[coff:coff + n]
        codes.copy_(torch.from_numpy(c_np))
        a_np = ec.awkward_alpha(rng, rows if per_row else 1)
        a = _alpha(a_np, dev)
        r, k = (rows, rl) if per_row else (1, n)
        full, lo, out = _guarded(n, dt, dev, lead)
        jobs.append((codes, out, a, plan, gmax, r, k, per_row, nn))
        one = antq_lib.decode8(codes, a, plan, gmax, r, k, per_row, dt, n_normal=nn, ovp=ovp)
        assert np.array_equal(_bits(one), bc.decode_ref(oracle, c_np, a_np, bk, r, k, dtype_name).reshape(-1)), (i, "single")
        singles.append((full, lo, n, _bits(one)))
        kinds.add(2 if (coff or lead or k % epl) else 0 if k // epl >= 128 else 1)
    assert len(jobs) >= 12 and kinds == {0, 1, 2}
    batch = antq_lib.DecodeBatch(jobs, ovp=ovp, width=8)

    def check(what):
        torch.cuda.synchronize()
        for i, ((full, lo, n, want), j) in enumerate(zip(singles, jobs)):
            assert np.array_equal(_bits(j[1]), want), (ovp, dtype_name, shapes[i], what)
            assert _guards_intact(full, lo, n), (ovp, dtype_name, shapes[i], what, "guard words")
            j[1].zero_()

    batch.run()
    check("first launch")
    batch.run()
    check("second launch")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.run()
    torch.cuda.current_stream().wait_stream(side)
    check("side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.run()
    torch.cuda.synchronize()
    for j in jobs:
        j[1].zero_()
    graph.replay()
    check("graph replay")


# ---------------------------------------------------------------------------------------------------------------------------
# 6: module
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
    "7" linear with 20 input features (row length 4 mod 8)."""
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
def test_packed_model_with_byte_codes(antq_lib, dev, tree, dtype_name, tmp_path, capsys):
    import torch
    from ant_quantization_amd import packed
    qmod, qutil = _trees(tree)
    dt = getattr(torch, dtype_name)
    model = _tiny(tree, dev, dt)
    x = _input(dev, dt)
    with torch.no_grad():
        model(x)                                   # calibration
        ref_model = copy.deepcopy(model)
        qutil.set_weight_bank(ref_model, False)    # the fake-quant model: every layer quantises its own weight
        y_ref = ref_model(x)
        # without the option: today's entries and reasons
        plain = qutil.pack_model(copy.deepcopy(ref_model))
        assert sorted(e["name"] for e in plain.entries.values()) == ["0", "3", "5"] and all(e["width"] == 4 for e in plain.entries.values())
        skipped = dict(plain.skipped)
        assert set(skipped) == {"6", "7"} and skipped["7"] == "row length 20 is not a multiple of 8" and "values" in skipped["6"]
        assert plain.launches == 1 and not plain.byte_codes and torch.equal(plain.model(x), y_ref)
        # with it
        bank = qutil.pack_model(model, byte_codes=True)
        assert isinstance(bank, packed.PackedBank) and bank.skipped == []
        width = {e["name"]: e["width"] for e in bank.entries.values()}
        assert width == {"0": 4, "3": 4, "5": 4, "6": 8, "7": 8}
        assert bank.launches == 2                  # one dtype, one pair rule, two code widths: two decode launches
        y1 = model(x)
        y2 = model(x)
        assert bank.launches == 2                  # a forward on an unchanged model launches nothing
        assert torch.equal(y1, y_ref) and torch.equal(y2, y_ref), (tree, dtype_name)
        bank.invalidate()
        assert torch.equal(model(x), y_ref) and bank.launches == 4          # one launch per group
        for e in bank.entries.values():
            n = e["mod"].weight.numel()
            assert e["codes"].dtype == torch.uint8 and e["codes"].numel() == (n if e["width"] == 8 else n // 2)
            assert not (e["width"] == 8 and e["fusable"]) and e["out"] is not None
            ref_layer = ref_model.get_submodule(e["name"])
            assert torch.equal(e["out"], ref_layer.quant_weight(ref_layer.weight)), e["name"]
        assert bank.nbytes()[0] == sum(e["codes"].numel() for e in bank.entries.values())
    with pytest.raises(antq_lib.AntqError, match="packed"):
        model(x)                                   # a gradient through a packed layer
    only8 = copy.deepcopy(ref_model)
    with torch.no_grad():
        b8 = qutil.pack_model(only8, byte_codes=True)
    for n in ("0", "3", "5"):                      # only the byte-coded layers may want gradients: still an error, and it names one
        only8.get_submodule(n).weight.requires_grad_(False)
        only8.get_submodule(n).quant_weight.alpha.requires_grad_(False)
    with pytest.raises(antq_lib.AntqError, match="byte codes"):
        only8(x)
    del b8
    with torch.no_grad():
        # checkpoint: numel-byte codes and no .weight for the byte-coded layers; the width comes from the stored size
        sd = qutil.packed_state_dict(model)
        for n, w in width.items():
            numel = model.get_submodule(n).weight.numel()
            assert n + ".weight" not in sd and sd[n + ".quant_weight.codes"].numel() == (numel if w == 8 else numel // 2)
            assert sd[n + ".quant_weight.codes"].dtype == torch.uint8
        path = str(tmp_path / "packed8.pth")
        torch.save(sd, path)
        fresh = _tiny(tree, dev, dt, seed=99)      # other weights: everything must come from the checkpoint
        bank2 = qutil.load_packed_state_dict(fresh, torch.load(path, map_location=dev))
        assert {e["name"]: e["width"] for e in bank2.entries.values()} == width and bank2.skipped == [] and bank2.launches == 2
        assert torch.equal(fresh(x), y_ref), (tree, dtype_name, "checkpoint")
        for e in bank2.entries.values():           # release_weights: the layer's weight IS the bank's decoded buffer
            assert e["mod"].weight.data_ptr() == e["out"].data_ptr()
        # a stored size that is neither numel nor numel / 2 names the layer
        bad = dict(torch.load(path, map_location=dev))
        bad["6.quant_weight.codes"] = bad["6.quant_weight.codes"][:-4]
        with pytest.raises(antq_lib.AntqError, match="layer 6"):
            qutil.load_packed_state_dict(_tiny(tree, dev, dt, seed=5), bad)
        # stored 4-bit codes for a layer whose book does not fit a nibble: refused as today
        bad = dict(torch.load(path, map_location=dev))
        bad["6.quant_weight.codes"] = bad["6.quant_weight.codes"][:bad["6.quant_weight.codes"].numel() // 2]
        with pytest.raises(antq_lib.AntqError, match="cannot be packed"):
            qutil.load_packed_state_dict(_tiny(tree, dev, dt, seed=5), bad)
        # release_weights frees the originals of byte-coded layers too
        bank3 = qutil.pack_model(copy.deepcopy(ref_model), release_weights=True, byte_codes=True)
        for e in bank3.entries.values():
            assert e["mod"].weight.data_ptr() == e["out"].data_ptr()
        assert torch.equal(bank3.model(x), y_ref) and torch.equal(bank3.model(x), y_ref) and bank3.launches == 2
        # fused_linear without images: the 8-bit Linear keeps its image and matches; the 4-bit Linears compute from their codes
        bank4 = qutil.pack_model(copy.deepcopy(ref_model), fused_linear=True, keep_images=False, byte_codes=True)
        e4 = {e["name"]: e for e in bank4.entries.values()}
        assert e4["6"]["out"] is not None and e4["7"]["out"] is not None and not e4["6"]["fusable"] and not e4["7"]["fusable"]
        assert e4["3"]["out"] is None and e4["3"]["fusable"]
        ref6 = ref_model.get_submodule("6")
        assert torch.equal(e4["6"]["out"], ref6.quant_weight(ref6.weight))
        assert torch.isfinite(bank4.model(x)).all()
        # the byte-coded Linear alone, on the same input: F.linear on the same image, so the same bits
        h = torch.randn(4, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(7)).to(dt)
        assert torch.equal(bank4.model.get_submodule("6")(h), ref6(h))
    capsys.readouterr()
