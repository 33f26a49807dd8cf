"""The fp32 fake-quant forward where a decision can flip, through every launch form: antq_fakequant ordered (with and without
the index output) and unordered, every dispatch knob, per-tensor / ragged / unaligned tensors, antq_fakequant_batch (job kinds
0 .. 3, alone and in the all-in-one launch), the in-kernel abs-max forms (antq_fakequant_dynamic, Batch(dynamic=True)), the
pair rule at the normal | outlier boundary, magnitudes / specials / odd scales, arbitrary codebooks; and the 65 536 bf16 / f16
patterns as short rows.

The yardstick is always oracle.forward on the same inputs: values compared as uint32 (NaN matches NaN), indices exactly.
Nothing on the reference side of an assert comes from the HIP library.  The inputs are built by fakequant_cases.py, which
test_fakequant_cases_host.py holds to their conditions without a GPU.  Every batched test asserts the kernels (and job kinds)
it meant to run, read off the descriptor the library built."""
import contextlib

import numpy as np
import pytest

import encode4_cases as ec
import fakequant_cases as fc

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {0: 0, 2: 1, 4: 1, 5: 1, 6: 0, 7: 0}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def knobs(antq_lib, kv):
    """knobs(lib, {5: 0, 0: 8}): set, run, restore the defaults"""
    try:
        for k, v in kv.items():
            antq_lib.lib().antq_debug_set(k, v)
        yield
    finally:
        for k in kv:
            antq_lib.lib().antq_debug_set(k, KNOB_DEFAULTS[k])


def _plan(antq_lib, g):
    plan = antq_lib.plan_for(g)
    return plan, fc.plan_header(plan.host)


def _dev_f32(x, dev, lead=0):
    """x on the device; lead: elements by which it starts off a 16-byte boundary"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1).view(np.int32))
    full = torch.zeros(src.numel() + 16, dtype=torch.int32, device=dev)
    assert full.data_ptr() % 16 == 0
    t = full[lead:lead + src.numel()]
    t.copy_(src)
    return t.view(torch.float32)


def _like(t, dev, lead=0):
    import torch
    full = torch.zeros(t.numel() + 16, dtype=torch.float32, device=dev)
    return full[lead:lead + t.numel()]


def _same(got_t, want, x, tag):
    got = got_t.detach().cpu().numpy().reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).reshape(-1)
    bad = np.flatnonzero((got != w.view(np.uint32)) & ~(np.isnan(got.view(np.float32)) & np.isnan(w)))
    assert bad.size == 0, (tag, "%d of %d values differ" % (bad.size, got.size), "at", bad[:6].tolist(), "x bits",
                           [hex(int(v)) for v in np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32)[bad[:6]]],
                           "got", [hex(int(v)) for v in got[bad[:6]]], "want", [hex(int(v)) for v in w.view(np.uint32)[bad[:6]]])


def _same_idx(idx_t, ridx, x, tag):
    got = idx_t.cpu().numpy().reshape(-1).astype(np.int32)
    w = ridx.reshape(-1)
    bad = np.flatnonzero(got != w)
    assert bad.size == 0, (tag, "%d of %d indices differ" % (bad.size, got.size), "at", bad[:6].tolist(), "x bits",
                           [hex(int(v)) for v in np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32)[bad[:6]]],
                           "got", got[bad[:6]].tolist(), "want", w[bad[:6]].tolist())


def _reference(oracle, x, alpha, bk, per_row=True):
    _, g, gmax, nn, ovp = bk
    with np.errstate(all="ignore"):
        return oracle.forward(x if per_row else x.reshape(1, -1), alpha, g, gmax, ovp)


def _alpha_dev(alpha, dev):
    import torch
    return torch.from_numpy(np.atleast_1d(np.asarray(alpha, np.float32)).copy()).to(dev)


PLAIN, IDX, UNORDERED = "plain", "idx", "unordered"
# (knobs, how): the launch forms of antq_fakequant.  Rows of fewer than 128 vectors always take the lane kernel: the knobs of
# the row kernels change nothing for them.
FORMS_SHORT = (({}, PLAIN), ({}, IDX), ({}, UNORDERED), ({4: 0}, PLAIN), ({4: 0}, IDX), ({7: 1}, PLAIN), ({7: 4}, PLAIN), ({6: 1}, PLAIN))
FORMS_LONG = FORMS_SHORT + (({5: 0}, PLAIN), ({5: 0}, IDX), ({5: 0}, UNORDERED), ({5: 2}, PLAIN), ({5: 2}, UNORDERED), ({2: 0}, PLAIN),
                            ({2: 0}, IDX), ({5: 0, 2: 0}, PLAIN), ({5: 0, 2: 0}, IDX), ({5: 0, 0: 1}, PLAIN), ({5: 0, 0: 8}, PLAIN),
                            ({5: 0, 0: 8}, IDX), ({5: 0, 0: 3}, UNORDERED), ({5: 0, 0: 2}, UNORDERED), ({5: 0, 2: 0, 0: 1}, PLAIN),
                            ({5: 0, 2: 0, 0: 8}, PLAIN), ({5: 0, 2: 0, 0: 3}, PLAIN), ({5: 0, 2: 0, 0: 3}, IDX), ({5: 0, 0: 5}, PLAIN), ({5: 0, 4: 0}, PLAIN), ({0: 1}, PLAIN), ({0: 8}, PLAIN))


def _run(antq_lib, oracle, dev, bk, x, alpha, per_row=True, forms=None, lead=0, tag=()):
    """x [rows, row_len] under every form == the oracle, values and (where the form has them) indices"""
    import torch
    _, g, gmax, nn, ovp = bk
    rows, rl = x.shape
    ref, ridx = _reference(oracle, x, alpha, bk, per_row)
    plan = antq_lib.plan_for(g)
    xt, at = _dev_f32(x, dev, lead), _alpha_dev(alpha, dev)
    assert (xt.data_ptr() % 16 != 0) == bool(lead)
    vpr = (rl if per_row else x.size) // 4
    aligned = not lead and (rl if per_row else x.size) % 4 == 0
    if forms is None:
        forms = FORMS_LONG if aligned and vpr >= 128 else FORMS_SHORT
    for kv, how in forms:
        t = (bk[0], rows, rl, per_row, kv, how, lead) + tuple(tag)
        with knobs(antq_lib, kv):
            if how == IDX:
                out, idx = antq_lib.fakequant(xt, at, plan, gmax, rows, rl, per_row, ovp=ovp, want_idx=True)
                _same_idx(idx, ridx, x, t)
            elif how == UNORDERED:
                out = _like(xt, dev, lead)
                torch.cuda.synchronize()                  # inputs at rest, nothing in flight touches the buffer
                got = antq_lib.fakequant(xt, at, plan, gmax, rows, rl, per_row, ovp=ovp, out=out, unordered=True)
                assert got.data_ptr() == out.data_ptr()
            else:
                out = antq_lib.fakequant(xt, at, plan, gmax, rows, rl, per_row, ovp=ovp, out=_like(xt, dev, lead) if lead else None)
        _same(out, ref, x, t)


# ---------------------------------------------------------------------------------------------------------------------------
# antq_fakequant: every row length, every knob
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rl", fc.ROW_LENS)
@pytest.mark.parametrize("name", fc.BOOK_NAMES)
def test_fp32_decision_edges_every_launch_form(antq_lib, oracle, dev, name, rl):
    """+/-16 ulps around every threshold, every bucket edge of the plan's table, fl(xlim * s), +/-2 * (outermost value) * s and
    the end of the exact straight-through step, 64 scales (16 / 8 for the 8-bit books) with short-mantissa ones and the
    floats around s = 2^-40 / 2^40 among them.  Rows of 16 (group-16), 12 and 20 (three and five vectors: the reciprocal row
    index), 72, 508, and 512 .. 4004 (whole and partial tasks of every size): ordered with and without indices, unordered,
    and under knobs 0 / 2 / 4 / 5 / 6 / 7 -- the lane kernel at every vectors-per-lane and workgroup size and on the exact
    division, the row-table kernel with 1 .. 8 vectors per lane in four- and one-wavefront workgroups, the d-domain row
    kernel (the 8-bit books' own, int-8's persistent loop; the 4-bit ones with knob 2 = 0)."""
    bk = fc.book(name)
    plan, h = _plan(antq_lib, bk[1])
    case = fc.static_case(oracle, name, h, rl)
    _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"])


@pytest.mark.parametrize("name", fc.BOOK_NAMES)
def test_fp32_per_tensor_ragged_and_unaligned(antq_lib, oracle, dev, name):
    """One scale for the tensor on (8, 72) -- as many tensors as hold a scale's windows, six at the most -- and on a flat
    tensor of 4099 elements a row (vector body + element tail); rows of 147 and 27 elements; the same rows with x and out
    4 bytes into a 16-byte line (the element kernel).  The OliVe books on an odd element count: the last element pairs
    with the first."""
    bk = fc.book(name)
    _, g, gmax, nn, ovp = bk
    plan, h = _plan(antq_lib, g)
    for a, c72, c4099 in fc.per_tensor_cases(oracle, name, h):
        flat = c72["x"].reshape(-1)
        for k in range(min(6, flat.size // 576)):
            _run(antq_lib, oracle, dev, bk, flat[576 * k:576 * (k + 1)].reshape(8, 72), np.float32(a), per_row=False)
        flat = c4099["x"].reshape(-1)
        flat = flat[:flat.size - (1 if flat.size % 4 == 0 else 0)]
        assert flat.size % 4
        _run(antq_lib, oracle, dev, bk, flat.reshape(1, -1), np.float32(a), per_row=False, forms=FORMS_LONG)
    for rl in fc.RAGGED_ROW_LENS:
        case = fc.static_case(oracle, name, h, rl)
        x, a = case["x"], case["alpha"]
        if (x.size % 2) == 0:                                     # an odd element count: rows and row length are both odd
            x, a = x[:-1], a[:-1]
        assert x.size % 2 == 1
        _run(antq_lib, oracle, dev, bk, x, a)
    for rl in (72, 1028) + fc.RAGGED_ROW_LENS:
        case = fc.static_case(oracle, name, h, rl)
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], lead=1, forms=(({}, PLAIN), ({}, UNORDERED), ({4: 0}, PLAIN)))


# ---------------------------------------------------------------------------------------------------------------------------
# antq_fakequant_batch
# ---------------------------------------------------------------------------------------------------------------------------
def _desc(b):
    """[(kind, vectors per lane, rotated map)] of a batch's jobs from its descriptor table (csrc/antq_k_batch.h BatchDesc: 192
    bytes each behind the 80-byte header; kind at byte 60, u at byte 148, rot at byte 152)"""
    n = int(b.host[:80].view(np.uint32)[1])
    d = [b.host[80 + 192 * k:80 + 192 * (k + 1)] for k in range(n)]
    return [tuple(int(v[at:at + 4].view(np.uint32)[0]) for at in (60, 148, 152)) for v in d]


def _job(antq_lib, oracle, dev, bk, x, alpha, lead=0):
    """(the Batch job, reference values, x)"""
    _, g, gmax, nn, ovp = bk
    ref, _ = _reference(oracle, x, alpha, bk)
    xt = _dev_f32(x, dev, lead)
    return (xt, _like(xt, dev, lead), _alpha_dev(alpha, dev), antq_lib.plan_for(g), gmax, x.shape[0], x.shape[1], True), ref, x


def _run_batch(antq_lib, jobs, ovp, kernels, kinds, tag, us=None, rots=None):
    """Build, check what the builder chose (kernels: what the descriptor's header says will be launched; None under knob 6,
    which picks the wavefronts per workgroup of k_fq_batch at the launch, whatever the header says), run, compare every job"""
    b = antq_lib.Batch([j[0] for j in jobs], ovp=ovp)
    assert not b.singles
    names = [k for k, _ in b.kernels()]
    assert kernels is None or names == kernels, (tag, names)
    assert [d[0] for d in _desc(b)] == kinds, (tag, _desc(b))
    if us is not None:
        assert [d[1] for d in _desc(b)] == us, (tag, _desc(b))
    if rots is not None:
        assert [d[2] for d in _desc(b)] == rots, (tag, _desc(b))
    for j in jobs:
        j[0][1].zero_()
    b.run()
    for n, (job, ref, x) in enumerate(jobs):
        _same(job[1], ref, x, tuple(tag) + ("job", n, job[5], job[6]))


def _static_kind(h, vpr, lane_rows=True):
    """The kind antq_batch_build files an aligned static fp32 job of vpr vectors per row under: rows of fewer than 128 vectors are
    lane jobs (1); longer ones too when the plan has the approximate-quotient form (unless knob 5 = 0: lane_rows False), else
    row-table jobs (2) with an x-domain plan, d-domain row jobs (0) without"""
    table = h["kind"] == fc.PLAN_TABLE
    if vpr < 128 or (lane_rows and table and h["adom"]):
        return 1
    return 2 if table and h["xdom"] else 0


def _o(ovp):
    return "true" if ovp else "false"


@pytest.mark.parametrize("family", ["ant", "olive"])
def test_fp32_batched_launch_every_job_kind(antq_lib, oracle, dev, family):
    """The decision-edge cases through antq_fakequant_batch.  As the builder files fp32 jobs: rows of >= 128 vectors are lane
    jobs (kind 1) by default and, with knob 5 = 0, row-table jobs (kind 2, k_fq_batch; a 4-bit book; rows of 128 vectors: whole tasks, the fixed
    map; of 400 and of 200: four 2-vector tasks, the last one partial, the rotated map -- asserted from the descriptor's rot
    word; workgroups of fewer than four wavefronts apply it, which rows of 400 vectors get by themselves and rows of 200 with
    knob 6 = 1 / 2) or d-domain row jobs (kind 0, an 8-bit book:
    k_fq_batch_d with the approximate quotient for int-8, with the exact division for flint-8); rows of 16 / 20 / 72 / 508 are
    kind 1; rows of 147 and an unaligned job kind 3.  Each alone, then all together (k_fq_batch_all); kind 1 with 2 and
    (knob 0 = 4) 4 vectors per lane, in a small batch and in one of the same job sixteen times over."""
    ovp = family == "olive"
    o = _o(ovp)
    b4 = fc.book("olive_flint" if ovp else "flint_b4_s")
    b8a = None if ovp else fc.book("int_b8_s")                 # (no 8-bit OliVe book has the approximate-quotient form)
    b8 = fc.book("olive_flint_b8" if ovp else "flint_b8_s")

    def job(bk, rl, lead=0, n_scales=None):
        _, h = _plan(antq_lib, bk[1])
        case = fc.edges_case(oracle, np.random.default_rng(fc.SEED + rl), bk, h, rl, n_scales=n_scales)
        return _job(antq_lib, oracle, dev, bk, case["x"], case["alpha"], lead)

    ka, kd = "antq::k_fq_batch_d<float,%s,true,false>" % o, "antq::k_fq_batch_d<float,%s,false,false>" % o
    # 128 vectors: one whole 2-vector task a row; 400 / 200 vectors: four 2-vector tasks, the last one 16 / 8 vectors: rotated
    long_full, long_part, long_part2 = job(b4, 512), job(b4, 1600), job(b4, 800)
    long8 = [job(b8, 576, n_scales=4)] + ([job(b8a, 576)] if b8a else [])
    short = [job(b4, rl) for rl in (16, 20, 72, 508)]
    ragged = [job(b4, 147), job(b4, 72, lead=1)]
    # (a) long rows, 4-bit: lane jobs by default, the row-table kernel with knob 5 = 0
    for jobs, waves, rots in (([long_full], 4, [0]), ([long_part], 1, [1]), ([long_part2], 4, [1]), ([long_full, long_part], 1, [0, 1]),
                              ([long_part, long_full, long_part2], 4, [1, 0, 1])):
        _run_batch(antq_lib, jobs, ovp, [ka], [1] * len(jobs), ("a, default", len(jobs)), us=[2] * len(jobs))
        with knobs(antq_lib, {5: 0}):
            # (one-wavefront workgroups when most of the launch sits in rows of >= 256 vectors; knob 6 forces 1 / 2 / 4 at the launch)
            kb = ["antq::k_fq_batch<float,%s,%d>" % (o, waves)]
            _run_batch(antq_lib, jobs, ovp, kb, [2] * len(jobs), ("a, knob 5 = 0", len(jobs)), us=[2] * len(jobs), rots=rots)
            for w in (1, 2, 4):
                with knobs(antq_lib, {6: w}):
                    _run_batch(antq_lib, jobs, ovp, None, [2] * len(jobs), ("a, knob 5 = 0, wavefronts", w, len(jobs)), rots=rots)
    # (b) long rows, 8-bit: d-domain row jobs with knob 5 = 0 (by default int-8 rows are lane jobs, flint-8 has no such form)
    for j in long8:
        adom = j is not long8[0]
        _run_batch(antq_lib, [j], ovp, [ka if adom else kd], [1 if adom else 0], ("b, default", adom))
        with knobs(antq_lib, {5: 0}):
            _run_batch(antq_lib, [j], ovp, [ka if adom else kd], [0], ("b, knob 5 = 0", adom))
    # (c) short rows: lane jobs, 2 vectors per lane (fp32 always) or 4 (knob 0 = 4); the same job sixteen times over
    for j in short:
        _run_batch(antq_lib, [j], ovp, [ka], [1], ("c", j[0][6]), us=[2])
    _run_batch(antq_lib, short, ovp, [ka], [1] * 4, ("c, together",), us=[2] * 4)
    with knobs(antq_lib, {0: 4}):
        _run_batch(antq_lib, short, ovp, [ka], [1] * 4, ("c, 4 vectors per lane",), us=[4] * 4)
    with knobs(antq_lib, {4: 0}):
        _run_batch(antq_lib, short, ovp, [kd], [1] * 4, ("c, exact division",))
    many = []
    for _ in range(16):
        (xt, out, at, plan, gmax, rows, rl, pr), ref, x = short[2]
        many.append(((xt, _like(xt, dev), at, plan, gmax, rows, rl, pr), ref, x))
    _run_batch(antq_lib, many, ovp, [ka], [1] * 16, ("c, sixteen times",), us=[2] * 16)
    with knobs(antq_lib, {0: 4}):
        _run_batch(antq_lib, many, ovp, [ka], [1] * 16, ("c, sixteen times, 4 vectors per lane",), us=[4] * 16)
    # (d) ragged rows and an unaligned job: element-granular jobs that ride with the d-domain launch
    for j in ragged:
        _run_batch(antq_lib, [j], ovp, [kd], [3], ("d", j[0][6]))
    _run_batch(antq_lib, ragged, ovp, [kd], [3, 3], ("d, together",))
    _run_batch(antq_lib, ragged + short[:1], ovp, [ka], [3, 3, 1], ("d, riding with a lane job",))
    # all together: more than one family -> the all-in-one kernel
    everything = [long_full, long_part] + long8 + short + ragged
    kinds8 = [0] + ([1] if b8a else [])
    _run_batch(antq_lib, everything, ovp, ["antq::k_fq_batch_all<float,%s>" % o], [1, 1] + kinds8 + [1] * 4 + [3, 3], ("all, default",))
    with knobs(antq_lib, {5: 0}):
        _run_batch(antq_lib, everything, ovp, ["antq::k_fq_batch_all<float,%s>" % o], [2, 2] + [0] * len(long8) + [1] * 4 + [3, 3],
                   ("all, knob 5 = 0",))
        _run_batch(antq_lib, [long_part, short[1], ragged[0]], ovp, ["antq::k_fq_batch_all<float,%s>" % o], [2, 1, 3], ("all, three kinds",))


# ---------------------------------------------------------------------------------------------------------------------------
# the in-kernel abs-max forms
# ---------------------------------------------------------------------------------------------------------------------------
DYN_BOOKS = ("flint_b4_s", "int_b4_s", "olive_flint", "int_b8_s", "flint_b8_s", "olive_int_b8")


def _dyn_batch_kernel(h, vpr, ovp):
    """What antq_batch_build files a dynamic fp32 job of vpr vectors per row under, or None where it refuses: groups of a
    power of two of <= 64 vectors and rows of up to 256 vectors in one wavefront's registers (the d-domain kernel); longer
    rows need the per-row table, in 1 / 4 wavefronts (k_fq_batch_dyn) or 16 (k_fq_batch_dyn16)."""
    d = "antq::k_fq_batch_d<float,%s,%s,true>" % (_o(ovp), "true" if h["adom"] else "false")
    if vpr < 128:
        return d if vpr & (vpr - 1) == 0 else None
    if h["xdom"] and not (h["adom"] and vpr <= 128):
        return ("antq::k_fq_batch_dyn<float,%s>" if vpr <= 2048 else "antq::k_fq_batch_dyn16<float,%s>") % _o(ovp) if vpr <= 8192 else None
    return d if vpr <= 256 else None


@pytest.mark.parametrize("vpr", fc.DYN_VPR)
@pytest.mark.parametrize("name", DYN_BOOKS)
def test_fp32_dynamic_scale_forms(antq_lib, oracle, dev, name, vpr):
    """Rows whose abs-max is planted (so the scales are known before the launch) around the decision edges that lie below
    it: antq_fakequant_dynamic with ratio 1 and an awkward one below 1, with and without indices, and Batch(dynamic=True)
    (ratio 1), at every row length where the kernels change shape -- groups in lanes, the small-row approximate path, the
    row in one, four and sixteen wavefronts, the two-pass fall-back of the books without a per-row table.  Values, indices and
    the returned scales against the oracle; a length the batch builder has no kernel for raises AntqError."""
    import torch
    bk = fc.book(name)
    _, g, gmax, nn, ovp = bk
    plan, h = _plan(antq_lib, g)
    for ratio in fc.DYN_RATIOS:
        case = fc.dynamic_case(oracle, name, h, vpr, ratio)
        x, alpha = case["x"], case["alpha"]
        rows, rl = x.shape
        assert np.array_equal(oracle.absmax(x, True, ratio), alpha)
        ref, ridx = _reference(oracle, x, alpha, bk)
        xt = _dev_f32(x, dev)
        t = (name, vpr, ratio, rows)
        out, a_dev, idx = antq_lib.fakequant_dynamic(xt, plan, gmax, rows, rl, ratio=ratio, ovp=ovp, want_idx=True)
        assert np.array_equal(a_dev.cpu().numpy(), alpha), t
        _same(out, ref, x, t + ("indices",))
        _same_idx(idx, ridx, x, t)
        out, a_dev, _ = antq_lib.fakequant_dynamic(xt, plan, gmax, rows, rl, ratio=ratio, ovp=ovp)
        assert np.array_equal(a_dev.cpu().numpy(), alpha), t
        _same(out, ref, x, t)
        with knobs(antq_lib, {4: 0}):
            out, a_dev, _ = antq_lib.fakequant_dynamic(xt, plan, gmax, rows, rl, ratio=ratio, ovp=ovp)
        assert np.array_equal(a_dev.cpu().numpy(), alpha), t
        _same(out, ref, x, t + ("exact division",))
        if ratio != 1.0:
            continue
        o_b, a_b = torch.zeros_like(xt), torch.zeros(rows, dtype=torch.float32, device=dev)
        want_kernel = _dyn_batch_kernel(h, vpr, ovp)
        if want_kernel is None:
            with pytest.raises(antq_lib.AntqError):
                antq_lib.Batch([(xt, o_b, a_b, plan, gmax, rows, rl, True)], ovp=ovp, dynamic=True)
            continue
        b = antq_lib.Batch([(xt, o_b, a_b, plan, gmax, rows, rl, True)], ovp=ovp, dynamic=True)
        assert [k for k, _ in b.kernels()] == [want_kernel] and not b.singles, (t, b.kernels())
        b.run()
        assert np.array_equal(a_b.cpu().numpy(), alpha), t + ("batch",)
        _same(o_b, ref, x, t + ("batch",))


# ---------------------------------------------------------------------------------------------------------------------------
# OliVe's pair rule at the normal | outlier boundary
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.OLIVE_NAMES)
def test_fp32_pair_rule_at_the_outlier_boundary(antq_lib, oracle, dev, name):
    """Pairs built around the normal | outlier midpoint and its negative: normal/normal, outlier/normal, normal/outlier and
    outlier/outlier at every pair position (all present by the oracle's indices, asserted before the GPU is asked), members
    1, 4 and 16 ulps from the boundary.  Through antq_fakequant (every form, indices with IDX_VICTIM), the batch as lane jobs
    (kind 1) and row-table / d-domain row jobs (kind 2 / 0), and the in-kernel abs-max forms with the row's maximum planted."""
    import torch
    bk = fc.book(name)
    _, g, gmax, nn, ovp = bk
    plan, h = _plan(antq_lib, g)
    for rl in fc.PAIR_ROW_LENS:
        case = fc.pair_case(np.random.default_rng(17), g, gmax, nn, rl, n_scales=16)
        assert ec.pair_forms_present(oracle, case, g, gmax, nn) == {(f, p) for f in range(4) for p in range(4)}
        x, alpha = case["x"], case["alpha"]
        _, ridx = _reference(oracle, x, alpha, bk)
        assert (ridx == oracle.IDX_VICTIM).any() and (ridx >= nn).any()
        _run(antq_lib, oracle, dev, bk, x, alpha)
        j = _job(antq_lib, oracle, dev, bk, x, alpha)
        d = "antq::k_fq_batch_d<float,true,%s,false>" % ("true" if h["adom"] else "false")
        _run_batch(antq_lib, [j], True, [d], [1 if rl < 512 or h["adom"] else 0], ("pairs", name, rl))
        if rl >= 512:
            with knobs(antq_lib, {5: 0}):
                _run_batch(antq_lib, [j], True, ["antq::k_fq_batch<float,true,%d>" % (4 if rl == 512 else 1)] if h["xdom"] else [d],
                           [2 if h["xdom"] else 0], ("pairs, knob 5 = 0", name, rl))
        # dynamic: the row's maximum m beyond every member (the far outlier members lie at 1.4 * the smallest outlier), alpha = fl(m * ratio)
        ratio = np.float32(fc.DYN_RATIOS[1])
        m = (alpha.astype(np.float64) / float(ratio)).astype(np.float32)
        xd = x.copy()
        assert (np.abs(xd) < m[:, None]).all()
        rng = np.random.default_rng(3)
        col = 2 * rng.integers(0, rl // 2, x.shape[0])            # an even position: its partner becomes the victim of an outlier
        xd[np.arange(x.shape[0]), col] = m
        a_dyn = (m * ratio).astype(np.float32)
        assert np.array_equal(oracle.absmax(xd, True, float(ratio)), a_dyn)
        present = dict(x=xd, alpha=a_dyn, pairs=case["pairs"])
        assert len(ec.pair_forms_present(oracle, present, g, gmax, nn)) == 16
        ref, ridx = _reference(oracle, xd, a_dyn, bk)
        xt = _dev_f32(xd, dev)
        out, a_dev, idx = antq_lib.fakequant_dynamic(xt, plan, gmax, x.shape[0], rl, ratio=float(ratio), ovp=True, want_idx=True)
        assert np.array_equal(a_dev.cpu().numpy(), a_dyn)
        _same(out, ref, xd, (name, rl, "dynamic"))
        _same_idx(idx, ridx, xd, (name, rl, "dynamic"))
        out, _, _ = antq_lib.fakequant_dynamic(xt, plan, gmax, x.shape[0], rl, ratio=float(ratio), ovp=True)
        _same(out, ref, xd, (name, rl, "dynamic, no indices"))
        # the batched form takes ratio 1: every member above gmax * s then is the row's maximum's business, so the oracle decides
        a_one = oracle.absmax(xd, True, 1.0)
        ref1, _ = _reference(oracle, xd, a_one, bk)
        kern = _dyn_batch_kernel(h, rl // 4, True)
        if kern is not None:
            o_b, a_b = torch.zeros_like(xt), torch.zeros(x.shape[0], dtype=torch.float32, device=dev)
            b = antq_lib.Batch([(xt, o_b, a_b, plan, gmax, x.shape[0], rl, True)], ovp=True, dynamic=True)
            assert [k for k, _ in b.kernels()] == [kern]
            b.run()
            assert np.array_equal(a_b.cpu().numpy(), a_one)
            _same(o_b, ref1, xd, (name, rl, "dynamic batch"))


# ---------------------------------------------------------------------------------------------------------------------------
# magnitudes, specials, scales
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flint_b4_s", "int_b4_s", "flint_b4_u", "olive_flint", "int_b8_s", "flint_b8_s", "olive_int_b8"])
def test_fp32_magnitudes_specials_and_scales(antq_lib, oracle, dev, name):
    """Both signs of every fp32 exponent (denormals among them) with five mantissas, +/-0, +/-Inf, NaNs, and +/-16 ulps around
    the magnitude at which the oracle's index turns into IDX_NONE, one group of rows per scale: 1, 0.06, 0, -0.05, NaN, Inf,
    1e-30, 1e30, 2^-60, 1e-41.  Through a representative of each mechanism: the lane kernel (rows of 72, and of 1024 by
    default), k_fq_uniform (knob 2 = 0, or the 8-bit books' own), the row-table kernel (knob 5 = 0), k_fq_scalar (rows of
    147), and the batch's job kinds 0 .. 3 in one all-in-one launch."""
    bk = fc.book(name)
    _, g, gmax, nn, ovp = bk
    plan, h = _plan(antq_lib, g)
    forms = (({}, PLAIN), ({}, IDX), ({}, UNORDERED), ({4: 0}, IDX), ({5: 0}, PLAIN), ({5: 0}, IDX), ({5: 0, 2: 0}, PLAIN), ({5: 0, 2: 0}, IDX))
    jobs = []
    for rl in (72, 1024, 147):
        case = ec.magnitude_case(oracle, np.random.default_rng(3), g, gmax, rl)
        _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"], forms=forms if rl == 1024 else forms[:4])
        jobs.append(_job(antq_lib, oracle, dev, bk, case["x"], case["alpha"]))
    # kind 1, kind 2 (an x-domain plan) or 0 (the others), kind 3; a second long job of the other long kind where there is one
    other = fc.book("int_b8_s" if h["xdom"] else "flint_b4_s") if not ovp else fc.book("olive_int_b8" if h["xdom"] else "olive_flint")
    case = ec.magnitude_case(oracle, np.random.default_rng(5), other[1], other[2], 1024)
    jobs.append(_job(antq_lib, oracle, dev, other, case["x"], case["alpha"]))
    with knobs(antq_lib, {5: 0}):
        kinds = [1, 2 if h["xdom"] else 0, 3, 0 if h["xdom"] else 2]
        _run_batch(antq_lib, jobs, ovp, ["antq::k_fq_batch_all<float,%s>" % _o(ovp)], kinds, ("magnitudes", name))


# ---------------------------------------------------------------------------------------------------------------------------
# arbitrary codebooks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(ec.fuzz_seeds()))
def test_fp32_arbitrary_codebooks_fuzz(antq_lib, oracle, dev, seed):
    """random_book + fuzz_case (make_x-style data with specials and +/-16-ulp windows at the midpoints) on the fp32 shapes of
    the encoder's fuzz, through antq_fakequant (values and indices, every form) and one batch of all the seed's tensors of a
    pair rule.  Arbitrary lists rarely have the approximate-quotient or x-domain form: this pins the plain quant_vec and the
    literal-scan plans in every kernel."""
    groups = {}
    for ovp, rng in ec.fuzz_books_rng(seed):
        g, gmax, nn = ec.random_book(rng, ovp)
        bk = ("fuzz %d %s" % (seed, g.tolist()), g, gmax, nn, ovp)
        for (rows, rl), dtype_name in ec.FUZZ_SHAPES:
            case = ec.fuzz_case(rng, g, gmax, rows, rl)
            if dtype_name != "float32":
                continue
            _run(antq_lib, oracle, dev, bk, case["x"], case["alpha"])
            groups.setdefault(ovp, []).append(_job(antq_lib, oracle, dev, bk, case["x"], case["alpha"]))
    for ovp, jobs in groups.items():
        for kv in ({}, {5: 0}):
            with knobs(antq_lib, kv):
                b = antq_lib.Batch([j[0] for j in jobs], ovp=ovp)
                assert not b.singles and all(k.startswith("antq::k_fq_batch") for k, _ in b.kernels()), b.kernels()
                want = [_static_kind(fc.plan_header(j[0][3].host), j[0][6] // 4, lane_rows=not kv) for j in jobs]
                assert [d[0] for d in _desc(b)] == want, (seed, ovp, kv, _desc(b), want)
                # families: row tables, d-domain jobs with / without the approximate quotient; more than one -> the all-in-one kernel
                hs = [fc.plan_header(j[0][3].host) for j in jobs]
                fams = {0 if k == 2 else 1 if h["kind"] == fc.PLAN_TABLE and h["adom"] else 2 for k, h in zip(want, hs)}
                one = {0: "antq::k_fq_batch<float,%s,", 1: "antq::k_fq_batch_d<float,%s,true,false>", 2: "antq::k_fq_batch_d<float,%s,false,false>"}
                name = "antq::k_fq_batch_all<float,%s>" % _o(ovp) if len(fams) > 1 else one[min(fams)] % _o(ovp)
                assert len(b.kernels()) == 1 and b.kernels()[0][0].startswith(name), (seed, ovp, kv, b.kernels(), name)
                for j in jobs:
                    j[0][1].zero_()
                b.run()
            for n, (job, ref, x) in enumerate(jobs):
                _same(job[1], ref, x, ("fuzz batch", seed, ovp, kv, n))


# ---------------------------------------------------------------------------------------------------------------------------
# the 16-bit types: every pattern as short rows, and with a book that has no 16-bit-domain form
# ---------------------------------------------------------------------------------------------------------------------------
def _dev_16(x16, dtype_name, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x16).view(np.int16)).to(dev).view(getattr(torch, dtype_name))


def _same16(oracle, got_t, want16, dtype_name, tag):
    import torch
    got = got_t.view(torch.int16).cpu().numpy().view(np.uint16).reshape(want16.shape)
    gf, wf = fc.widen16(oracle, got, dtype_name), fc.widen16(oracle, want16, dtype_name)
    bad = ~((got == want16) | (np.isnan(gf) & np.isnan(wf)))
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want16[bad][:4])


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float16"])
@pytest.mark.parametrize("name,rl", [("flint_b4_s", 16), ("flint_b4_s", 72), ("olive_flint", 16), ("olive_flint", 72), ("int_b8_s", 4096)])
def test_16bit_every_pattern_short_rows_and_wide_book(antq_lib, oracle, dev, name, rl, dtype_name):
    """The 65 536 bf16 / f16 patterns, in order and shuffled, as rows of 16 and of 72 elements (2 and 9 vectors: lane jobs, the
    approximate path with 8 elements per lane) and -- int-8, which has no 16-bit-domain form -- of 4096, per-row scales
    repeated from eight row scales: antq_fakequant (ordered, with indices, unordered) and the batch, against the oracle's fp32
    sequence rounded once."""
    import torch
    bk = fc.book(name)
    _, g, gmax, nn, ovp = bk
    plan, h = _plan(antq_lib, g)
    assert (h["hdom"] == 0) == (name == "int_b8_s")
    for shuffle in (None, np.random.default_rng(41)):
        x16, alpha = fc.pattern_rows(rl, shuffle)
        rows = x16.shape[0]
        xf = fc.widen16(oracle, x16, dtype_name)
        with np.errstate(all="ignore"):
            ref, ridx = oracle.forward(xf, alpha, g, gmax, ovp)
        want = fc.round16(oracle, ref, dtype_name)
        xt, at = _dev_16(x16, dtype_name, dev), _alpha_dev(alpha, dev)
        t = (name, rl, dtype_name, shuffle is not None)
        out, idx = antq_lib.fakequant(xt, at, plan, gmax, rows, rl, True, ovp=ovp, want_idx=True)
        _same16(oracle, out, want, dtype_name, t + ("indices",))
        assert np.array_equal(idx.cpu().numpy().reshape(ridx.shape).astype(np.int32), ridx), t
        _same16(oracle, antq_lib.fakequant(xt, at, plan, gmax, rows, rl, True, ovp=ovp), want, dtype_name, t)
        buf = torch.empty_like(xt)
        torch.cuda.synchronize()
        antq_lib.fakequant(xt, at, plan, gmax, rows, rl, True, ovp=ovp, out=buf, unordered=True)
        _same16(oracle, buf, want, dtype_name, t + ("unordered",))
        with knobs(antq_lib, {4: 0}):
            _same16(oracle, antq_lib.fakequant(xt, at, plan, gmax, rows, rl, True, ovp=ovp), want, dtype_name, t + ("exact division",))
        o_b = torch.zeros_like(xt)
        b = antq_lib.Batch([(xt, o_b, at, plan, gmax, rows, rl, True)], ovp=ovp)
        tn = {"bfloat16": "bf16", "float16": "f16"}[dtype_name]
        assert [k for k, _ in b.kernels()] == ["antq::k_fq_batch_d<%s,%s,true,false>" % (tn, _o(ovp))] and not b.singles, b.kernels()
        assert [d[0] for d in _desc(b)] == [1 if rl < 1024 else 0]
        b.run()
        _same16(oracle, o_b, want, dtype_name, t + ("batch",))
