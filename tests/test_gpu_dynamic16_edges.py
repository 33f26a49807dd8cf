"""The in-kernel abs-max forward (ANTQ_FLAG_DYNAMIC) of bf16 / f16 rows at its edges, through every launch form:
antq_fakequant_dynamic with and without an alpha buffer and with the index output, with knob 9 = 0, and Batch(dynamic=True) of
one job and of every row length at once.  Aimed at k_fq_hrow_dyn / k_fq_hbatch_dyn (hrow_wave_task_dyn, csrc/antq_k_hrow.h: the
row in 1, 4 or 16 wavefronts) and the 16-bit instantiations of the lane form (groups of <= 64 vectors, and the form whose
128-vector rows span two wavefronts): row lengths at every boundary of the launch shapes, the abs-max planted wherever a mask,
a half-word, a vector step or a wavefront can go missing, abs-max values from the smallest subnormal to NaN under eight ratios,
and every 16-bit pattern below a maximum.

The yardstick everywhere: alpha_ref = oracle.absmax(widened rows, True, ratio), out_ref = the oracle's fp32 sequence with that
alpha rounded once to the type; alpha compared as uint32, outputs as uint16 (NaN matches NaN), indices with the oracle's.
Nothing on the reference side of an assert comes from the HIP library.  The inputs are built by dynamic16_cases.py, which
test_dynamic16_cases_host.py holds to their conditions without a GPU.  Every batched run asserts the job kinds and kernels it
meant to run from the descriptor the library built; every out and alpha buffer lies between poisoned guard bands."""
import numpy as np
import pytest

import dynamic16_cases as dc
import fakequant_cases as fc
import operator_cases as oc

pytestmark = pytest.mark.gpu

ERR_ARG = -1                      # include/antq.h ANTQ_ERR_ARG
TYPE_TAG = {"bfloat16": "bf16", "float16": "f16"}
KIND_OF_WPR = {1: 14, 4: 15, 16: 16}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def knob9(antq_lib):
    """set knob 9 (0: the 16-bit-domain row kernels off); the default is back after the test whatever happens in it"""
    def set_(v):
        antq_lib.lib().antq_debug_set(9, v)
    yield set_
    antq_lib.lib().antq_debug_set(9, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
class Carved:
    """n elements inside a buffer filled with a poison pattern: oc.GUARD (+ lead) elements before them, oc.GUARD behind (128
    bytes a side for 16-bit elements, 256 for the scales)"""

    def __init__(self, n, dtype_name, dev, lead=0):
        import torch
        raw, self.poison = ("int32", oc.POISON32) if dtype_name == "float32" else ("int16", oc.POISON16)
        self.lo, self.n = oc.GUARD + lead, n
        self.buf = torch.full((self.lo + n + oc.GUARD,), self.poison, dtype=getattr(torch, raw), device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + n].view(getattr(torch, dtype_name))

    def bits(self, tag):
        """the n elements as unsigned integers, after checking that every guard element still holds the poison"""
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == self.poison).all() and (b[self.lo + self.n:] == self.poison).all(), (tag, "guard elements changed")
        v = b[self.lo:self.lo + self.n]
        return v.view(np.uint16 if v.itemsize == 2 else np.uint32)

    def untouched(self, tag):
        assert (self.buf == self.poison).all().item(), (tag, "a refused call wrote")

    def reset(self):
        self.buf.fill_(self.poison)


def _dev16(x16, dtype_name, dev, lead=0):
    """the patterns on the device, starting `lead` elements off a 16-byte boundary"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(x16).reshape(-1).view(np.int16).copy())
    full = torch.zeros(src.numel() + 16, dtype=torch.int16, device=dev)
    assert full.data_ptr() % 16 == 0
    t = full[lead:lead + src.numel()]
    t.copy_(src)
    return t.view(getattr(torch, dtype_name))


def _same_out(oracle, got16, want16, dtype_name, tag):
    got16 = got16.reshape(want16.shape)
    bad = ~dc.same16(oracle, got16, want16, dtype_name)
    assert not bad.any(), (tag, "%d of %d values differ" % (int(bad.sum()), bad.size), "at", np.argwhere(bad)[:4].tolist(),
                           "got", [hex(int(v)) for v in got16[bad][:4]], "want", [hex(int(v)) for v in want16[bad][:4]])


def _same_alpha(got32, want, tag):
    got = np.asarray(got32).view(np.float32).reshape(-1)
    bad = ~dc.same32(got, want)
    assert not bad.any(), (tag, "alpha differs in rows", np.flatnonzero(bad)[:6].tolist(), "got", [hex(int(v)) for v in got.view(np.uint32)[bad][:6]],
                           "want", [hex(int(v)) for v in np.asarray(want, np.float32).view(np.uint32)[bad][:6]])


def _o(b):
    return "true" if b else "false"


# ---------------------------------------------------------------------------------------------------------------------------
# what the batch builder files a dynamic 16-bit job under
# ---------------------------------------------------------------------------------------------------------------------------
def _desc(b):
    """[(kind, vectors per row, vshift, vectors per lane)] of a batch's jobs from its descriptor table (csrc/antq_k_batch.h
    BatchDesc: 192 bytes each behind the 80-byte header; vpr at byte 44, vshift at 52, kind at 60, u at 148)"""
    n = int(b.host[:80].view(np.uint32)[1])
    d = [b.host[80 + 192 * k:80 + 192 * (k + 1)] for k in range(n)]
    return [(int(v[60:64].view(np.uint32)[0]), int(v[44:48].view(np.uint32)[0]), int(v[52:56].view(np.int32)[0]), int(v[148:152].view(np.uint32)[0]))
            for v in d]


def _expect(h, dtype_name, rl, lead, ovp):
    """(kind, vshift or None, vectors per lane or None, kernel) antq_batch_build must file an ANTQ_FLAG_DYNAMIC job of this
    shape under, or None where it must refuse (ANTQ_ERR_UNSUPPORTED): ragged or unaligned jobs and rows beyond 8192 vectors;
    a plan without the 16-bit-domain form keeps rows of up to 256 vectors (128: the lane form over two wavefronts)."""
    t, o = TYPE_TAG[dtype_name], _o(ovp)
    lane = "antq::k_fq_batch_d<%s,%s,%s,true>" % (t, o, _o(h["adom"]))
    if lead or rl % 8:
        return None
    vpr = rl // 8
    if vpr < 128:
        sh = vpr.bit_length() - 1
        return (1, sh, None, lane) if vpr == 1 << sh else None
    if h["hdom"] & dc.HDOM_BIT[dtype_name]:
        if vpr > 8192:
            return None
        wpr, nv = dc.shape_of(vpr)
        return (KIND_OF_WPR[wpr], None, nv, "antq::k_fq_hbatch_dyn<%s,%s,%d>" % (t, o, wpr))
    assert not h["xdom"]                                   # (the wide book of this file: d-domain table only)
    if h["adom"] and vpr == 128:
        return (1, 7, 4, lane)
    return (0, None, None, lane) if vpr <= 256 else None


def _assert_filed(b, wants, tag):
    got = _desc(b)
    assert len(got) == len(wants) and not b.singles, (tag, got)
    for (kind, vpr, vshift, u), w in zip(got, wants):
        assert kind == w[0] and (w[1] is None or vshift == w[1]) and (w[2] is None or u == w[2]), (tag, (kind, vpr, vshift, u), w)
    names = [k for k, _ in b.kernels()]
    assert sorted(set(names)) == sorted({w[3] for w in wants}) and len(names) == len(set(names)), (tag, names)


# ---------------------------------------------------------------------------------------------------------------------------
# one case through every launch form
# ---------------------------------------------------------------------------------------------------------------------------
def _abi_dynamic(antq_lib, xt, out_t, alpha_t, plan, gmax, rows, rl, ratio, ovp):
    """antq_fakequant_dynamic as the bindings call it, with caller-owned out and alpha buffers (alpha_t None: no buffer)"""
    return antq_lib.lib().antq_fakequant_dynamic(xt.data_ptr(), out_t.data_ptr(), None, alpha_t.data_ptr() if alpha_t is not None else None,
                                                 rows, rl, ratio, gmax, plan.host_addr, plan.dev(xt.device).data_ptr(),
                                                 antq_lib.FLAG_OVP if ovp else 0, antq_lib._DTYPES[xt.dtype], antq_lib._stream_int(xt.device))


def _run_forms(antq_lib, oracle, dev, knob9, dtype_name, bk, x16, ref, ratio=1.0, lead=0, pair=None, tag=()):
    """x16 [rows, row_len] against ref = (alpha_ref, out_ref, idx_ref) of dynamic16_cases.reference, through every form"""
    name, g, gmax, nn, ovp = bk
    ovp = ovp if pair is None else pair
    rows, rl = x16.shape
    a_ref, o_ref, i_ref = ref
    plan = antq_lib.plan_for(g)
    h = fc.plan_header(plan.host)
    xt = _dev16(x16, dtype_name, dev, lead)
    assert (xt.data_ptr() % 16 != 0) == bool(lead)
    # abs-max pass + static pass: ragged or unaligned rows, rows beyond 8192 vectors, and -- a plan without the per-row table
    # (the 8-bit book) has the single-read kernel in one wavefront only -- its rows beyond 512 vectors (antq_fq.hip launch_uniform)
    two_pass = bool(lead) or rl % 8 != 0 or rl // 8 > (8192 if h["xdom"] else 512)
    tag = (name, dtype_name, rows, rl, lead, ratio, ovp) + tuple(tag)
    out, al = Carved(x16.size, dtype_name, dev, lead), Carved(rows, "float32", dev)

    def default_form(t):
        out.reset(), al.reset()
        assert _abi_dynamic(antq_lib, xt, out.view, al.view, plan, gmax, rows, rl, ratio, ovp) == 0, t
        _same_alpha(al.bits(t), a_ref, t)
        _same_out(oracle, out.bits(t), o_ref, dtype_name, t)

    default_form(tag + ("default",))
    # no alpha buffer: the single-read kernels skip the store; the two-pass fall-back needs the buffer and says so before it
    # launches anything, and the binding then retries with one
    out.reset()
    rc = _abi_dynamic(antq_lib, xt, out.view, None, plan, gmax, rows, rl, ratio, ovp)
    assert rc == (ERR_ARG if two_pass else 0), (tag, rc)
    if two_pass:
        out.untouched(tag + ("no alpha buffer, refused",))
    else:
        _same_out(oracle, out.bits(tag), o_ref, dtype_name, tag + ("no alpha buffer",))
    out.reset()
    o2, a2, _ = antq_lib.fakequant_dynamic(xt, plan, gmax, rows, rl, ratio=ratio, ovp=ovp, out=out.view, want_alpha=False)
    assert a2 is None and o2.data_ptr() == out.view.data_ptr()
    _same_out(oracle, out.bits(tag), o_ref, dtype_name, tag + ("want_alpha=False",))
    # with indices: the fp32-domain kernels
    out.reset()
    _, a3, idx = antq_lib.fakequant_dynamic(xt, plan, gmax, rows, rl, ratio=ratio, ovp=ovp, out=out.view, want_idx=True)
    _same_alpha(a3.cpu().numpy(), a_ref, tag + ("indices",))
    _same_out(oracle, out.bits(tag), o_ref, dtype_name, tag + ("indices",))
    got = idx.cpu().numpy().reshape(i_ref.shape).astype(np.int32)
    assert np.array_equal(got, i_ref), (tag, "indices differ at", np.argwhere(got != i_ref)[:4].tolist())
    # knob 9 = 0: the fp32-domain single-read kernels on the 16-bit data
    knob9(0)
    default_form(tag + ("knob 9 = 0",))
    knob9(1)
    if ratio != 1.0:
        return                                                     # (the batch form is ratio 1 by contract)
    want = _expect(h, dtype_name, rl, lead, ovp)
    job = (xt, out.view, al.view, plan, gmax, rows, rl, True)
    if want is None:
        with pytest.raises(antq_lib.AntqError):
            antq_lib.Batch([job], ovp=ovp, dynamic=True)
        return
    for with_alpha in (True, False):
        t = tag + ("batch", with_alpha)
        out.reset(), al.reset()
        b = antq_lib.Batch([job if with_alpha else job[:2] + (None,) + job[3:]], ovp=ovp, dynamic=True)
        _assert_filed(b, [want], t)
        b.run()
        if with_alpha:
            _same_alpha(al.bits(t), a_ref, t)
        else:
            al.untouched(t)
        _same_out(oracle, out.bits(t), o_ref, dtype_name, t)


def _rows(ref, n):
    return tuple(v[:n] for v in ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: every row length, the abs-max at every position
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", dc.GROUP_NAMES)
@pytest.mark.parametrize("name", dc.BOOKS)
@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_planted_abs_max_at_every_row_length_and_position(antq_lib, oracle, dev, knob9, dtype_name, name, group):
    """Row lengths (in 16-byte vectors) at every boundary of hrow_dyn_shape and of the launchers: lane groups of 1 / 2 / 16 / 64,
    one wavefront with 2 .. 8 vector steps at both ends of each (128, 129 | 192, ... 449 | 512), four wavefronts (513: the last
    one entirely past the row end; 1024, 2047, 2048), sixteen (2049: five idle; 4096, 8191, 8192), and the two-pass fall-back
    (8193 vectors, a ragged row of 8 * 129 + 3 elements, a tensor one element into a 16-byte line), which must report
    ANTQ_ERR_ARG without an alpha buffer and write nothing (so do the 8-bit book's rows beyond 512 vectors: without a per-row
    table the single-read kernel exists for one wavefront only).  One row per planted position of the maximum +/-M (element 0 and
    the last, both halves of a word, lane 0 and the last lane of the first and last vector step of the first, a middle and the
    last wavefront in use), a row with +M and -M, one with -M only; every other element <= M / 4.  The whole tensor, its first
    5 rows (the batched one-wavefront form: 8 tasks, 3 without a row) and its first row alone."""
    bk = dc.book(name)
    h = fc.plan_header(antq_lib.plan_for(bk[1]).host)
    assert bool(h["hdom"] & dc.HDOM_BIT[dtype_name]) == (name in dc.BOOKS_H) and h["adom"]
    for label, rl, lead in dc.shapes_of_group(group):
        x = dc.planted_case(dtype_name, rl)["x"]
        ref = dc.reference(oracle, x, dtype_name, bk)
        for n in (x.shape[0],) + dc.ROW_COUNTS[::-1]:
            _run_forms(antq_lib, oracle, dev, knob9, dtype_name, bk, x[:n], _rows(ref, n), lead=lead, tag=(label,))


@pytest.mark.parametrize("name", dc.BOOKS)
@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_one_batch_of_every_row_length(antq_lib, oracle, dev, dtype_name, name):
    """ONE Batch(dynamic=True) holding 5 rows of every row length the builder takes for the book: lane jobs (families 1 / 2)
    and the 16-bit-domain rows in 1, 4 and 16 wavefronts (families 6 / 7 / 8) share a launch sequence; for the 8-bit book the
    lane groups, the 128-vector rows over two wavefronts and the d-domain rows of up to 256 vectors.  Run twice, with the
    outputs poisoned again in between; with and without alpha buffers."""
    bk = dc.book(name)
    _, g, gmax, nn, ovp = bk
    plan = antq_lib.plan_for(g)
    h = fc.plan_header(plan.host)
    jobs, wants, refs = [], [], []
    for label, rl, lead in dc.ALL_SHAPES:
        want = _expect(h, dtype_name, rl, lead, ovp)
        if want is None:
            continue
        x = np.ascontiguousarray(dc.planted_case(dtype_name, rl)["x"][:5])
        refs.append(dc.reference(oracle, x, dtype_name, bk))
        out, al = Carved(x.size, dtype_name, dev), Carved(5, "float32", dev)
        jobs.append((_dev16(x, dtype_name, dev), out, al, rl))
        wants.append(want)
    kinds = {w[0] for w in wants}
    assert kinds == ({1, 14, 15, 16} if name in dc.BOOKS_H else {1, 0}) and (name in dc.BOOKS_H or (1, 7, 4) in {w[:3] for w in wants})
    assert len(jobs) == (len(dc.VPRS) if name in dc.BOOKS_H else 9)
    for with_alpha in (True, False):
        b = antq_lib.Batch([(xt, out.view, al.view if with_alpha else None, plan, gmax, 5, rl, True) for xt, out, al, rl in jobs], ovp=ovp, dynamic=True)
        _assert_filed(b, wants, (name, dtype_name, with_alpha))
        for again in (0, 1):
            for _, out, al, _ in jobs:
                out.reset(), al.reset()
            b.run()
            for (xt, out, al, rl), (a_ref, o_ref, _) in zip(jobs, refs):
                t = (name, dtype_name, rl, "alpha buffers" if with_alpha else "no alpha buffers", "run", again)
                if with_alpha:
                    _same_alpha(al.bits(t), a_ref, t)
                else:
                    al.untouched(t)
                _same_out(oracle, out.bits(t), o_ref, dtype_name, t)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: what the abs-max is
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vpr", dc.MAG_VPRS)
@pytest.mark.parametrize("name", dc.BOOKS)
@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_abs_max_values_specials_and_ratios(antq_lib, oracle, dev, knob9, dtype_name, name, vpr):
    """Rows whose maximum is an awkward value, a power of two, the largest finite value (f16 + OliVe: fl16(vout * s) overflows
    and the row loses its table), the smallest normal, the largest and the smallest subnormal (a denormal scale: the literal
    path), all +/-0 (alpha 0); NaN, +Inf, -Inf, NaN and Inf in different wavefronts (NaN wins, as in antq_absmax); and the
    value that tells alpha = fl(M * ratio) from a ratio applied to the scale.  Ratios 1, 0.83, 0.25, 1.0625, 2^-20, 0, -0.5
    and 2^-140 (M * ratio underflows) for the one-tensor forms, ratio 1 for the batch; a 16-vector group, and rows in one,
    four and sixteen wavefronts."""
    bk = dc.book(name)
    x = dc.magnitude_case(dtype_name, vpr)["x"]
    for ratio in dc.RATIOS:
        ref = dc.reference(oracle, x, dtype_name, bk, ratio)
        _run_forms(antq_lib, oracle, dev, knob9, dtype_name, bk, x, ref, ratio=ratio)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: every pattern below the maximum
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", dc.PATTERN_TOPS)
@pytest.mark.parametrize("name,pair", [(n, None) for n in dc.BOOKS] + [("olive_flint", False)])
@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_every_pattern_below_the_maximum(antq_lib, oracle, dev, knob9, dtype_name, name, pair, top):
    """Every 16-bit pattern of magnitude <= M, both signs and +/-0, shuffled, for M the largest finite value, an awkward value
    near 1 and one a few binades above the smallest normal: as one zero-padded row of up to 8192 vectors, and dealt over rows of
    128, 512 and 2048 vectors that each hold +/-M too.  Ratio 1 and 0.25 (the upper patterns go through the sentinel slot and
    hrow_vec_far), 2^-5 where the pair rule is on (OliVe's table ends at 24 * gmax) and 1.0625 for the largest finite M
    (outputs beyond it: Inf for f16); the OliVe book with and without the pair rule."""
    bk = dc.book(name)
    ovp = bk[4] if pair is None else pair
    for k, x in enumerate(dc.pattern_case(dtype_name, top)):
        for ratio in dc.pattern_ratios(top, ovp):
            ref = dc.reference(oracle, x, dtype_name, bk, ratio, pair)
            _run_forms(antq_lib, oracle, dev, knob9, dtype_name, bk, x, ref, ratio=ratio, pair=pair, tag=(top, k))
