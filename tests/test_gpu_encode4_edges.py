"""antq_encode4 where its codes can be wrong without anything downstream noticing (the decoders and antq_linear4 are only
faithful to the codes): fp32 inputs within a few ulps of every decision point, the pair rule at the normal | outlier
boundary, magnitudes / specials / odd scales, every launch form (element encoder, aligned and not; row-table encoder with 2-,
4- and 8-vector tasks; exact division; persistent workgroups that loop), the write footprint, arbitrary codebooks.

The yardstick is always the CPU oracle: its scan-order indices mapped to codes (an outlier: its index in the outlier list, a
victim: 15, no entry within the scan's horizon: the code of the grid's zero).  Nothing on the reference side of an assert
comes from the HIP library.  The inputs are built by encode4_cases.py, which test_encode4_cases_host.py holds to their
conditions without a GPU.

Not covered: tensors of more than 2^32 octets (the 64-bit row-index branch of k_encode) -- too large for a test of seconds."""
import contextlib

import numpy as np
import pytest

import encode4_cases as ec

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {0: 0, 1: 0, 2: 1, 4: 1, 5: 1, 9: 1}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def knobs(antq_lib, **kv):
    """knobs(lib, k0=4, k2=0): set, run, restore the defaults"""
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


def _nibbles(codes):
    c = codes.cpu().numpy()
    return np.stack([c & 15, c >> 4], 1).reshape(-1).astype(np.int64)


def _encode(antq_lib, dev, xt, alpha, bk, rows, rl, per_row, out=None):
    import torch
    _, g, gmax, nn, ovp = bk
    a = torch.from_numpy(np.atleast_1d(np.asarray(alpha, np.float32))).to(dev)
    return antq_lib.encode4(xt, a, antq_lib.plan_for(g), gmax, rows, rl, per_row, n_normal=nn, ovp=ovp, out=out)


def _same(got, want, xf, tag):
    want = want.reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, "%d of %d codes differ" % (bad.size, got.size), "at", bad[:6].tolist(),
                           "x bits", [hex(int(v)) for v in np.ascontiguousarray(xf, np.float32).reshape(-1).view(np.uint32)[bad[:6]]],
                           "got", got[bad[:6]].tolist(), "want", want[bad[:6]].tolist())


def _run(antq_lib, oracle, dev, bk, x, alpha, per_row=True, dtype_name="float32", forms=((),), tag=()):
    """x [rows, row_len] float32 -> (rounded to the dtype) encoded under every form (a form: knob settings) == the oracle"""
    rows, rl = x.shape
    xk, xf = ec.as_dtype(oracle, x, dtype_name)
    _, g, gmax, nn, ovp = bk
    want = ec.oracle_codes(oracle, xf if per_row else xf.reshape(1, -1), alpha, g, gmax, nn, ovp)
    xt = _tensor(xk, dtype_name, dev)
    for form in forms:
        with knobs(antq_lib, **dict(form)):
            got = _nibbles(_encode(antq_lib, dev, xt, alpha, bk, rows, rl, per_row))
        _same(got, want, xf, (bk[0], dtype_name, rows, rl, per_row, form) + tuple(tag))


ELEMENT_FORMS = ((), (("k4", 0),))
ROW_FORMS = ((), (("k0", 2),), (("k0", 4),), (("k0", 8),), (("k2", 0),), (("k4", 0),), (("k2", 0), ("k4", 0)))


def _forms(row_len_elems):
    return ROW_FORMS if row_len_elems >= 512 else ELEMENT_FORMS


# ---------------------------------------------------------------------------------------------------------------------------
# 2a
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.BOOK_NAMES)
def test_fp32_codes_around_every_threshold(antq_lib, oracle, dev, name):
    """+/-16 ulps around fl(midpoint * scale) of every pair of adjacent distinct grid values, 64 awkward scales: rows of 504
    (element encoder), 520 (row-table encoder, 2-vector tasks, the second one partial) and 1032 elements (4-vector tasks,
    partial), and three tensors with one scale each (one row of 2080 elements); the long rows also with 2 / 4 / 8 vectors per
    task forced, through the element encoder (knob 2 = 0) and with exact division (knob 4 = 0).  Every form equals the
    oracle.  The OliVe books run with the pair rule."""
    bk = ec.book(name)
    _, g, gmax, nn, ovp = bk
    for rl in (504, 520, 1032):
        case = ec.threshold_case(np.random.default_rng(99), g, gmax, rl)
        good, total = ec.windows_straddle(oracle, case, g, gmax)
        assert good == total, (name, rl, good, total)
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], forms=_forms(rl))
    for a in ec.awkward_alpha(np.random.default_rng(5), 3):
        case = ec.threshold_case(np.random.default_rng(7), g, gmax, 2080, n_scales=1, alpha=[a])
        good, total = ec.windows_straddle(oracle, case, g, gmax)
        assert good == total
        _run(antq_lib, oracle, dev, bk, case["x"].reshape(4, 520), np.float32(a), per_row=False, forms=ROW_FORMS)


@pytest.mark.parametrize("name", ["olive_flint", "olive_int"])
def test_fp32_pair_rule_at_the_outlier_boundary(antq_lib, oracle, dev, name):
    """Pairs built from the windows around the normal | outlier midpoint and its negative: normal/normal, outlier/normal,
    normal/outlier and outlier/outlier at each of the four pair positions of an octet (all 16 present by the oracle's
    indices, asserted before the GPU is asked), members 1, 4 and 16 ulps from the boundary."""
    bk = ec.book(name)
    _, g, gmax, nn, ovp = bk
    for rl in (504, 520, 1032):
        case = ec.pair_case(np.random.default_rng(17), g, gmax, nn, rl)
        assert ec.pair_forms_present(oracle, case, g, gmax, nn) == {(f, p) for f in range(4) for p in range(4)}
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], forms=_forms(rl))


# ---------------------------------------------------------------------------------------------------------------------------
# 2b
# ---------------------------------------------------------------------------------------------------------------------------
def _plain_twin(bk):
    """An OliVe book's normal values alone, without the pair rule"""
    name, g, gmax, nn, ovp = bk
    return (name + "_normal_only", np.ascontiguousarray(g[:nn]), gmax, 0, False)


@pytest.mark.parametrize("name", ec.BOOK_NAMES)
def test_fp32_magnitudes_specials_and_scales(antq_lib, oracle, dev, name):
    """Both signs of every fp32 exponent (denormals among them) with five mantissas, +/-0, +/-Inf, NaNs, and +/-16 ulps around
    the magnitude at which the oracle's index turns into IDX_NONE, one group of rows per scale: 1, 0.06, 0, -0.05, NaN, Inf,
    1e-30, 1e30, 2^-60, 1e-41.  Rows of 504 and 1032 elements; the OliVe books with the pair rule and, their normal values
    alone, without."""
    bk = ec.book(name)
    for b in ((bk, _plain_twin(bk)) if bk[4] else (bk,)):
        _, g, gmax, nn, ovp = b
        for rl in (504, 1032):
            case = ec.magnitude_case(oracle, np.random.default_rng(3), g, gmax, rl)
            _run(antq_lib, oracle, dev, b, case["x"], case["alpha"], forms=_forms(rl))


@pytest.mark.parametrize("name", ec.BOOK_NAMES)
def test_fp32_octets_with_one_half_off_the_table_path(antq_lib, oracle, dev, name):
    """One half of an octet NaN / Inf / far-clipped (or one such value among ordinary ones), the other half threshold-window
    values: in the fp32 row-table encoder the two halves are two lanes that exchange their codes, one on the literal path
    and one on the table path."""
    bk = ec.book(name)
    _, g, gmax, nn, ovp = bk
    for rl in (504, 520, 1032):
        case = ec.split_octet_case(np.random.default_rng(29), g, gmax, rl)
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], forms=_forms(rl))


# ---------------------------------------------------------------------------------------------------------------------------
# 2c
# ---------------------------------------------------------------------------------------------------------------------------
DTYPES = ("float32", "bfloat16", "float16")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_shapes_row_index_forms_and_task_edges(antq_lib, oracle, dev, dtype_name):
    """The three row-index forms of the element encoder (shift, reciprocal, and -- per-tensor -- none), row lengths on both
    sides of the row encoders' 128- and 256-vector switches, element counts one octet short of / equal to / over whole tasks,
    a per-tensor scale; and a 7-task tensor encoded by 1, 3 and 7 persistent workgroups."""
    rng = np.random.default_rng(41)
    shapes = ec.SHAPES_F32 if dtype_name == "float32" else ec.SHAPES_16
    for bk in ec.books():
        _, g, gmax, nn, ovp = bk
        for rows, rl in shapes:
            case = ec.random_case(rng, rows, rl, g, gmax, ovp)
            _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], dtype_name=dtype_name)
        rows, rl = ec.PER_TENSOR_SHAPE
        case = ec.random_case(rng, rows, rl, g, gmax, ovp, per_row=False)
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"][0], per_row=False, dtype_name=dtype_name)
        rows, rl = ec.LOOP_SHAPE
        case = ec.random_case(rng, rows, rl, g, gmax, ovp)
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], dtype_name=dtype_name,
             forms=((("k1", 1),), (("k1", 3),), (("k1", 7),)))


@pytest.mark.parametrize("name", ["flint_b4_s", "olive_flint"])
def test_one_persistent_workgroup_loops_at_natural_size(antq_lib, oracle, dev, name):
    """(131080, 64) fp32, no knob: 2049 tasks of the element encoder on its 2048 workgroups, so exactly one of them takes a
    second task.  Every code against the oracle."""
    bk = ec.book(name)
    _, g, gmax, nn, ovp = bk
    rows, rl = ec.BIG_SHAPE
    case = ec.random_case(np.random.default_rng(13), rows, rl, g, gmax, ovp)
    _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"])


# ---------------------------------------------------------------------------------------------------------------------------
# 2d
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64 + 16


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_write_footprint_and_unaligned_buffers(antq_lib, oracle, dev, dtype_name):
    """codes is a view into a buffer of 0xA5 with at least 64 guard bytes on either side, starting 0, 4 and 12 bytes off a
    16-byte boundary; x starts on one or one element behind it (the element encoder without vector loads).  Shapes with partial
    last tasks.  The codes are the oracle's, every guard byte is still 0xA5, x is unchanged."""
    import torch
    rng = np.random.default_rng(53)
    shapes = ec.PARTIAL_SHAPES if dtype_name == "float32" else ec.PARTIAL_SHAPES_16
    for bk in (ec.book("flint_b4_s"), ec.book("olive_flint")):
        _, g, gmax, nn, ovp = bk
        for rows, rl in shapes:
            case = ec.random_case(rng, rows, rl, g, gmax, ovp)
            xk, xf = ec.as_dtype(oracle, case["x"], dtype_name)
            want = ec.oracle_codes(oracle, xf, case["alpha"], g, gmax, nn, ovp)
            nb = rows * rl // 2
            for lead in (0, 1):
                xt = _tensor(xk, dtype_name, dev, lead)
                assert (xt.data_ptr() % 16 != 0) == bool(lead)
                before = xt.clone()
                for off in (0, 4, 12):
                    full = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
                    lo = GUARD - (full.data_ptr() + GUARD) % 16 + off
                    assert lo >= 64 and (full.data_ptr() + lo) % 16 == off and full.numel() - lo - nb >= 64
                    out = full[lo:lo + nb]
                    got = _encode(antq_lib, dev, xt, case["alpha"], bk, rows, rl, True, out=out)
                    assert got.data_ptr() == out.data_ptr()
                    tag = (bk[0], dtype_name, rows, rl, "x lead", lead, "codes offset", off)
                    _same(_nibbles(out), want, xf, tag)
                    f = full.cpu().numpy()
                    assert (f[:lo] == 0xA5).all() and (f[lo + nb:] == 0xA5).all(), tag + ("guard bytes",)
                assert torch.equal(xt.view(torch.uint8), before.view(torch.uint8)), (bk[0], dtype_name, rows, rl, lead, "x changed")


def test_out_is_validated_and_odd_offsets_are_refused(antq_lib, dev):
    """out= takes a contiguous uint8 view of numel / 2 bytes on x's device and nothing else; codes at an odd byte offset are
    refused by antq_encode4 itself (ANTQ_ERR_ALIGN) before anything is launched: the buffer keeps its fill."""
    import torch
    bk = ec.book("flint_b4_s")
    x = torch.zeros(4 * 64, device=dev)
    full = torch.full((128 + 64,), 0xA5, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        with pytest.raises(antq_lib.AntqError):
            _encode(antq_lib, dev, x, np.ones(4, np.float32), bk, 4, 64, True, out=full[16 + off:16 + off + 128])
    torch.cuda.synchronize()
    assert (full == 0xA5).all()
    bad = [full[:127], full[:129], full[:256:2], torch.zeros(128, dtype=torch.int8, device=dev), torch.zeros(128, dtype=torch.uint8),
           torch.zeros(32, dtype=torch.int32, device=dev)]
    for out in bad:
        with pytest.raises(antq_lib.AntqError):
            _encode(antq_lib, dev, x, np.ones(4, np.float32), bk, 4, 64, True, out=out)
    ok = _encode(antq_lib, dev, x, np.ones(4, np.float32), bk, 4, 64, True, out=full[32:160])
    assert ok.data_ptr() == full[32:160].data_ptr() and (full[:32] == 0xA5).all() and (full[160:] == 0xA5).all()
    assert not (full[32:160] == 0xA5).any()            # zeros encode as the zero code 8 | 8 << 4
    assert _encode(antq_lib, dev, x, np.ones(4, np.float32), bk, 4, 64, True).numel() == 128


# ---------------------------------------------------------------------------------------------------------------------------
# 2e
# ---------------------------------------------------------------------------------------------------------------------------
def _plan_kind(antq_lib, g):
    """What the plan builder chose (antq_plan_kind and the plan header's eligibility words): a table whose thresholds move into
    the x domain per row (k_encode4_xrow on long rows, the approximate-quotient branch of k_encode on short ones), a table
    decided in the d domain with the approximate quotient (that branch on every row) or with the exact division only (the
    quant_vec branch), or no table at all (quant_vec's literal scan)."""
    plan = antq_lib.plan_for(g)
    if int(antq_lib.lib().antq_plan_kind(plan.host_ptr())) == 0:
        return "literal scan"
    h = plan.host[:128].view(np.uint32)
    return "x-domain table" if int(h[16]) else "d-domain table" if int(h[22]) else "d-domain table, exact division"


def _fuzz_seed(antq_lib, oracle, dev, seed, encode=True):
    """-> {plan kind: {"short", "long"}} of what was encoded"""
    done = {}
    for ovp, rng in ec.fuzz_books_rng(seed):
        g, gmax, nn = ec.random_book(rng, ovp)
        assert ec.book_well_formed(g, gmax, nn, ovp), (seed, ovp, g)
        bk = ("fuzz %d %s" % (seed, g.tolist()), g, gmax, nn, ovp)
        kind = _plan_kind(antq_lib, g)
        for (rows, rl), dtype_name in ec.FUZZ_SHAPES:
            case = ec.fuzz_case(rng, g, gmax, rows, rl)
            if encode:
                _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], dtype_name=dtype_name, forms=_forms(rl), tag=(kind,))
            done.setdefault(kind, set()).add("long" if rl >= 512 else "short")
    return done


@pytest.mark.parametrize("seed", range(ec.fuzz_seeds()))
def test_arbitrary_codebooks_fuzz(antq_lib, oracle, dev, seed):
    """Random well-formed books -- 2 .. 16 values, or 1 .. 15 normal values within 32 and 1 .. 15 outliers beyond it with the
    pair rule; sorted or not, duplicates, signed zeros, entries one ulp apart, uniform / geometric / even spacing -- on short
    and long fp32 rows and long bf16 rows, make_x-style data with specials and +/-16-ulp windows at the midpoints.  Codes
    against the oracle only (decoded values of arbitrary lists may differ from fake-quant by an ulp, include/antq.h).
    ANTQ_FUZZ_SEEDS widens it."""
    done = _fuzz_seed(antq_lib, oracle, dev, seed)
    assert all(v == {"short", "long"} for v in done.values()), done


def test_fuzz_reaches_every_plan_kind(antq_lib, oracle, dev):
    """Over the default seeds: every plan kind the builder chooses for some book was encoded on a short and on a long row (each
    book runs every shape), and all kinds occur with <= 16 (15 + 15) entries: x-domain table, d-domain table (rare: about one
    book in twenty), d-domain table with exact division, literal scan."""
    seen = {}
    for seed in range(6):
        for kind, where in _fuzz_seed(antq_lib, oracle, dev, seed, encode=False).items():
            seen.setdefault(kind, set()).update(where)
    assert all(v == {"short", "long"} for v in seen.values()), seen
    assert set(seen) == {"x-domain table", "d-domain table", "d-domain table, exact division", "literal scan"}, seen
