"""The GIVEN-scale 16-bit-domain row kernels (csrc/antq_k_hrow.h "K1h": k_fq_hrow, k_fq_hbatch; csrc/antq_k_codec.h
k_encode4_hrow) where a row is cut into tasks: row lengths at every switch point of the host rules that pick a task size
(hrow_static_u, row_task_u, the encoder's 8 / 4 / 3 / 2 rule, the U = 8 promotion, rot), last tasks of 0, 1, 63 .. 65, ...
255 .. 257 vectors in use under every task size, 1 .. 9 tasks per row, one scale per row and one per tensor, bf16 and f16.
Rows whose scales differ so that a wrong row index shows in head and tail; +/-Inf, NaN, far-clipped and beyond-the-table
elements planted wherever a task, a vector step or a lane group ends; a row without a table in every tensor.

The yardstick everywhere: oracle.forward on the widened input rounded once to the type, compared as 16-bit patterns (NaN
matches NaN); for the encoder the oracle's scan-order indices mapped to codes.  Nothing on the expected side of an assert comes
from the HIP library, and there is no tolerance anywhere.  The inputs are built by static16_cases.py, which
test_static16_cases_host.py holds to their conditions without a GPU.  Every output lies between poisoned guard bands in one
arena per (type, book) that is compared whole after each launch form: a store one slot on, a vector left out or a task run on
the wrong row shows wherever it lands."""
import contextlib

import numpy as np
import pytest

import fakequant_cases as fc
import static16_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 64                        # poison elements on either side of every output; bytes on either side of every code buffer
KNOB_DEFAULTS = {0: 0, 6: 0, 8: 0, 9: 1, 10: -1, 13: 0}
TYPE_TAG = {"bfloat16": "bf16", "float16": "f16"}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def knobs(antq_lib, kv):
    """knobs(lib, {9: 2, 0: 3}): set, run, restore the defaults"""
    try:
        for k, v in kv.items():
            antq_lib.lib().antq_debug_set(k, v)
        yield
    finally:
        for k in kv:
            antq_lib.lib().antq_debug_set(k, KNOB_DEFAULTS[k])


def _plan(antq_lib, name):
    bk = sc.book(name)
    plan = antq_lib.plan_for(bk[1])
    h = fc.plan_header(plan.host)
    return bk, plan, h, sc.lims_of(h)


# ---------------------------------------------------------------------------------------------------------------------------
# every tensor of a case set in one device arena
# ---------------------------------------------------------------------------------------------------------------------------
class Arena:
    """x, alpha and the outputs of every tensor of a case set on the device.  The outputs share one buffer filled with the poison
    pattern, GUARD poison elements on either side of each: check() compares the WHOLE buffer with its expected image (the
    oracle's outputs, poison everywhere else) and poisons it again."""

    def __init__(self, cs, dtype_name, dev):
        import torch
        self.cs, self.dtype_name = cs, dtype_name
        tdt = getattr(torch, dtype_name)
        self.off, pos = [], 0
        for c in cs:
            self.off.append(pos + GUARD)
            pos += GUARD + c["x"].size + GUARD
        self.want = np.full(pos, sc.POISON16, np.uint16)
        self.x_host = np.zeros(pos, np.uint16)
        for c, o in zip(cs, self.off):
            self.want[o:o + c["x"].size] = c["out"].reshape(-1)
            self.x_host[o:o + c["x"].size] = c["x"].reshape(-1)
        self.x = torch.from_numpy(self.x_host.view(np.int16).copy()).to(dev)
        self.out = torch.full((pos,), sc.POISON16, dtype=torch.int16, device=dev)
        assert self.x.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and all(o % 8 == 0 for o in self.off)
        a_off = np.cumsum([0] + [4 * ((c["alpha"].size + 3) // 4) for c in cs])
        a_host = np.zeros(a_off[-1], np.float32)
        for c, o in zip(cs, a_off):
            a_host[o:o + c["alpha"].size] = c["alpha"]
        self.a_host = a_host
        self.alpha_all = torch.from_numpy(a_host.copy()).to(dev)
        self.xv = [self.x[o:o + c["x"].size].view(tdt) for c, o in zip(cs, self.off)]
        self.ov = [self.out[o:o + c["x"].size].view(tdt) for c, o in zip(cs, self.off)]
        self.av = [self.alpha_all[o:o + c["alpha"].size] for c, o in zip(cs, a_off)]

    def where(self, flat):
        i = int(np.searchsorted(np.asarray(self.off) - GUARD, flat, side="right")) - 1
        c, rel = self.cs[i], int(flat) - self.off[i]
        inside = 0 <= rel < c["x"].size
        return (c["rows"], c["rl"], c["per_row"]), ("row", rel // c["rl"], "vector", (rel % c["rl"]) // 8, "element", rel % 8) if inside else ("guard", rel)

    def check(self, oracle, tag, only=None):
        """the whole buffer against its image; only: the tensors that were run (the others must still be all poison)"""
        got = self.out.cpu().numpy().view(np.uint16)
        want = self.want
        if only is not None:
            want = np.full_like(self.want, sc.POISON16)
            for i in only:
                o, n = self.off[i], self.cs[i]["x"].size
                want[o:o + n] = self.want[o:o + n]
        bad = np.flatnonzero(~sc.same16(oracle, got, want, self.dtype_name))
        assert bad.size == 0, (tag, "%d of %d elements differ" % (bad.size, got.size), [self.where(b) for b in bad[:4]],
                               "got", [hex(int(v)) for v in got[bad[:4]]], "want", [hex(int(v)) for v in want[bad[:4]]])
        self.out.fill_(sc.POISON16)

    def inputs_unchanged(self, tag):
        assert np.array_equal(self.x.cpu().numpy().view(np.uint16), self.x_host), (tag, "x changed")
        assert np.array_equal(self.alpha_all.cpu().numpy().view(np.uint32), self.a_host.view(np.uint32)), (tag, "alpha changed")

    def job(self, i, plan, gmax):
        c = self.cs[i]
        return (self.xv[i], self.ov[i], self.av[i], plan, gmax, c["rows"], c["rl"], c["per_row"])


_ARENAS = {}


def _arena(dev, dtype_name, name, lims):
    """one arena per (type, book) and process: the oracle's work (static16_cases.cases) and the upload are done once"""
    key = (dtype_name, name)
    if key not in _ARENAS:
        _ARENAS[key] = Arena(sc.cases(dtype_name, name, lims), dtype_name, dev)
    return _ARENAS[key]


# ---------------------------------------------------------------------------------------------------------------------------
# 1: the forward, one tensor per launch
# ---------------------------------------------------------------------------------------------------------------------------
ORDERED, UNORDERED = "ordered", "unordered"
FORWARD_FORMS = (({}, ORDERED), ({9: 2}, ORDERED), ({9: 2, 0: 2}, ORDERED), ({9: 2, 0: 3}, ORDERED), ({9: 2, 0: 4}, ORDERED),
                 ({9: 2, 0: 8}, ORDERED), ({9: 2, 6: 4}, ORDERED), ({9: 2, 6: 4, 0: 8}, ORDERED), ({9: 2, 6: 4, 0: 3}, ORDERED),
                 ({}, UNORDERED), ({9: 2}, UNORDERED), ({9: 0}, ORDERED))


@pytest.mark.parametrize("name", sc.BOOKS_FWD)
@pytest.mark.parametrize("dtype_name", sc.DTYPES)
def test_forward_every_row_length_and_task_size(antq_lib, oracle, dev, dtype_name, name):
    """antq_fakequant on 5 rows of every length of static16_cases.VPRS and on the three per-tensor shapes: default routing
    (K1h where hrow_static_u keeps the row, the fp32-domain row table elsewhere), every row in K1h (knob 9 = 2) with the rule's
    task size and with 2 / 3 / 4 / 8 vectors per lane forced, the 4-wavefront form (knob 6 = 4; a forced 8 lowered to 4),
    unordered launches into the caller's buffer, and the fp32-domain kernels alone (knob 9 = 0), which must agree too.  The
    4-bit books of dynamic16_cases.BOOKS_H and the one reference codebook with the 16-bit-domain form but no fp32-domain row
    table (float4_b6_s).  Outputs == the oracle, every guard band intact, x and alpha unchanged."""
    import torch
    bk, plan, h, lims = _plan(antq_lib, name)
    _, g, gmax, nn, ovp = bk
    A = _arena(dev, dtype_name, name, lims)
    for kv, how in FORWARD_FORMS:
        tag = (name, dtype_name, kv, how)
        if how == UNORDERED:
            torch.cuda.synchronize()                  # inputs at rest, nothing in flight touches the buffer
        with knobs(antq_lib, kv):
            for i, c in enumerate(A.cs):
                got = antq_lib.fakequant(A.xv[i], A.av[i], plan, gmax, c["rows"], c["rl"], c["per_row"], ovp=ovp, out=A.ov[i],
                                         unordered=how == UNORDERED)
                assert got.data_ptr() == A.ov[i].data_ptr()
        A.check(oracle, tag)
    A.inputs_unchanged((name, dtype_name))


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the batched launch
# ---------------------------------------------------------------------------------------------------------------------------
def _desc(b):
    """[(kind, vectors per lane, rotated map, vectors per row, tasks per row, tasks)] of a batch's jobs from its descriptor table
    (csrc/antq_k_batch.h BatchDesc: 192 bytes each behind the 80-byte header; total_tasks at byte 40, vpr at 44, tpr at 48,
    kind at 60, u at 148, rot at 152)"""
    n = int(b.host[:80].view(np.uint32)[1])
    d = [b.host[80 + 192 * k:80 + 192 * (k + 1)] for k in range(n)]
    return [tuple(int(v[at:at + 4].view(np.uint32)[0]) for at in (60, 148, 152, 44, 48, 40)) for v in d]


def _want_desc(c, u):
    """what antq_batch_build must file a kind-13 job of u vectors per lane under"""
    vpr = sc.row_vpr(c["rows"], c["rl"], c["per_row"])
    tpr = sc.tpr_of(vpr, u)
    return (13, u, sc.rot_of(vpr, u), vpr, tpr, (c["rows"] if c["per_row"] else 1) * tpr)        # per tensor: ONE row


@pytest.mark.parametrize("name", sc.BOOKS_FWD)
@pytest.mark.parametrize("dtype_name", sc.DTYPES)
def test_batch_routing_and_block_map(antq_lib, oracle, dev, dtype_name, name):
    """antq_fakequant_batch.  (a) One job per batch, every shape: (kind, u, rot, tasks per row, tasks) read from the descriptor
    equal the restated hrow_static_u / rot -- kind 13 and k_fq_hbatch alone where the rule keeps the row, the fp32-domain row
    table (kind 2) where it hands it back; a tensor with one scale is ONE row.  (b) Every shape in ONE batch with knob 9 = 2:
    all kind 13 by row_task_u, task counts of every residue mod 4, mixed task sizes, rotated and fixed maps, a per-tensor job in
    the middle -- under knob 8 = 0 (per-job rotation), 1 (every whole group of eight workgroups) and 2 (none), with a workgroup
    count that is a multiple of 8 and, one job left out, one that is not (its last four workgroups are no whole group and stay
    unrotated); each run twice.  Outputs == the oracle (hence == the single launches of the test above, bit for bit), guard bands
    intact."""
    bk, plan, h, lims = _plan(antq_lib, name)
    _, g, gmax, nn, ovp = bk
    A = _arena(dev, dtype_name, name, lims)
    kname = "antq::k_fq_hbatch<%s,%s>" % (TYPE_TAG[dtype_name], "true" if ovp else "false")
    n13 = 0
    for i, c in enumerate(A.cs):
        b = antq_lib.Batch([A.job(i, plan, gmax)], ovp=ovp)
        assert not b.singles
        u = sc.hrow_static_u(sc.row_vpr(c["rows"], c["rl"], c["per_row"]), bool(h["xdom"]))
        tag = (name, dtype_name, c["rows"], c["rl"], c["per_row"], _desc(b))
        if u:
            want = _want_desc(c, u)
            assert _desc(b) == [want], tag
            assert b.kernels() == [(kname, 4 * ((want[5] + 3) // 4))], (tag, b.kernels())
            n13 += 1
        else:
            assert _desc(b)[0][0] == 2 and len(b.kernels()) == 1 and b.kernels()[0][0].startswith("antq::k_fq_batch<"), (tag, b.kernels())
        b.run()
    assert n13 == (len(A.cs) if not h["xdom"] else sum(1 for s in sc.SHAPES if sc.hrow_static_u(sc.row_vpr(*s), True))) and n13 >= 13
    A.check(oracle, (name, dtype_name, "one job per batch"))
    # (b) every shape in one launch: the per-tensor jobs moved into the middle
    order = list(range(len(sc.VPRS)))
    for k, i in enumerate(range(len(sc.VPRS), len(A.cs))):
        order.insert(5 + 9 * k, i)
    with knobs(antq_lib, {9: 2}):
        wants = {i: _want_desc(A.cs[i], sc.row_task_u(sc.row_vpr(A.cs[i]["rows"], A.cs[i]["rl"], A.cs[i]["per_row"]))) for i in order}
        blocks = {i: (wants[i][5] + 3) // 4 for i in order}
        drop = next(i for i in order[::-1] if blocks[i] % 2 == 1)
        sets = [order, [i for i in order if i != drop]]
        sets.sort(key=lambda s: sum(blocks[i] for i in s) % 2)                  # the multiple of 8 workgroups first
        for s in sets:
            b = antq_lib.Batch([A.job(i, plan, gmax) for i in s], ovp=ovp)
            assert _desc(b) == [wants[i] for i in s] and not b.singles, (name, dtype_name, _desc(b))
            wgs = 4 * sum(blocks[i] for i in s)
            assert b.kernels() == [(kname, wgs)] and wgs % 8 == (0 if s is sets[0] else 4), b.kernels()
            if s is order:
                assert {wants[i][5] % 4 for i in s} == {0, 1, 2, 3} and {wants[i][1] for i in s} == {2, 3, 4} and {wants[i][2] for i in s} == {0, 1}
            for rot in (0, 1, 2):
                with knobs(antq_lib, {8: rot}):
                    for again in (0, 1):
                        b.run()
                        A.check(oracle, (name, dtype_name, "one batch", wgs, "knob 8 =", rot, "run", again), only=s)
    A.inputs_unchanged((name, dtype_name))


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the promotion to 8-vector tasks, and the launches big enough for the occupancy cap
# ---------------------------------------------------------------------------------------------------------------------------
def _eight_rows(oracle, c, dtype_name, bk):
    """8 distinct rows from a 5-row tensor: its rows, and rows 0, 1 and 4 again under the scales of rows 1, 3 and 0.
    (x [8, rl], alpha [8], the oracle's outputs [8, rl])"""
    x = np.ascontiguousarray(np.concatenate([c["x"], c["x"][[0, 1, 4]]]))
    alpha = np.concatenate([c["alpha"], c["alpha"][[1, 3, 0]]]).astype(np.float32)
    return x, alpha, sc.forward16(oracle, x, dtype_name, bk, alpha)


@pytest.mark.parametrize("dtype_name", sc.DTYPES)
def test_promoted_and_large_launches(antq_lib, oracle, dev, dtype_name):
    """1024 rows of 512 vectors, ordered: the launcher's own promotion to 8-vector tasks (a whole row per wavefront); the same
    with the dynamic LDS forced (knob 10).  16384 rows of 129 vectors in 2-vector tasks (knobs 9 = 2, 0 = 2): 32768 tasks, the
    smallest launch that takes the occupancy pad by itself, every second task one vector.  References tiled from 8 distinct
    rows, compared on the device; guard bands on either side."""
    import torch
    tdt = getattr(torch, dtype_name)
    for name in ("flint_b4_s", "olive_flint"):
        bk, plan, h, lims = _plan(antq_lib, name)
        _, g, gmax, nn, ovp = bk
        for vpr, reps, forms in ((512, 128, ({}, {10: 8192})), (129, 2048, ({9: 2, 0: 2},))):
            x8, a8, o8 = _eight_rows(oracle, sc.case(dtype_name, name, lims, sc.ROWS, 8 * vpr, True), dtype_name, bk)
            rows, rl = 8 * reps, 8 * vpr
            xt = torch.from_numpy(x8.view(np.int16)).to(dev).repeat(reps, 1).contiguous().view(tdt)
            at = torch.from_numpy(a8).to(dev).repeat(reps).contiguous()
            want = torch.from_numpy(o8.view(np.int16)).to(dev).repeat(reps, 1).contiguous()
            nan = torch.isnan(want.view(tdt))
            buf = torch.full((GUARD + rows * rl + GUARD,), sc.POISON16, dtype=torch.int16, device=dev)
            out = buf[GUARD:GUARD + rows * rl]
            assert out.data_ptr() % 16 == 0
            for kv in forms:
                buf.fill_(sc.POISON16)
                with knobs(antq_lib, kv):
                    antq_lib.fakequant(xt, at, plan, gmax, rows, rl, True, ovp=ovp, out=out.view(tdt))
                got = out.view(rows, rl)
                bad = ~((got == want) | (nan & torch.isnan(got.view(tdt))))
                tag = (name, dtype_name, rows, vpr, kv)
                assert not bad.any().item(), (tag, int(bad.sum().item()), torch.nonzero(bad)[:4].tolist())
                assert (buf[:GUARD] == sc.POISON16).all().item() and (buf[GUARD + rows * rl:] == sc.POISON16).all().item(), (tag, "guard elements changed")


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the encoder
# ---------------------------------------------------------------------------------------------------------------------------
class CodeArena:
    """The code buffers of every tensor of a case set in one buffer of POISON_CODE bytes: each starts `lead` bytes into a
    16-byte line and has at least GUARD poison bytes on either side."""

    def __init__(self, A, lead, dev):
        import torch
        self.A, self.off, pos = A, [], GUARD
        for c in A.cs:
            self.off.append(pos + lead)
            pos = (pos + lead + c["x"].size // 2 + GUARD + 15) // 16 * 16
        self.want = np.full(pos, sc.POISON_CODE, np.uint8)
        for c, o in zip(A.cs, self.off):
            nib = c["codes"].reshape(-1).astype(np.uint8)
            self.want[o:o + nib.size // 2] = nib[0::2] | (nib[1::2] << 4)
        self.buf = torch.full((pos,), sc.POISON_CODE, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and all(o % 16 == lead for o in self.off)
        self.cv = [self.buf[o:o + c["x"].size // 2] for c, o in zip(A.cs, self.off)]

    def check(self, tag):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        if bad.size:
            i = int(np.searchsorted(np.asarray(self.off) - GUARD, bad[0], side="right")) - 1
            c, rel = self.A.cs[i], 2 * (int(bad[0]) - self.off[i])
            where = ("row", rel // c["rl"], "vector", (rel % c["rl"]) // 8) if 0 <= rel < c["x"].size else ("guard", rel // 2)
            assert False, (tag, "%d of %d code bytes differ" % (bad.size, got.size), (c["rows"], c["rl"], c["per_row"]), where,
                           "got", [hex(int(v)) for v in got[bad[:4]]], "want", [hex(int(v)) for v in self.want[bad[:4]]])
        self.buf.fill_(sc.POISON_CODE)


ENCODER_FORMS = ({}, {0: 2}, {0: 3}, {0: 4}, {0: 8}, {13: 1}, {13: 1, 0: 8}, {9: 0})


@pytest.mark.parametrize("name", sc.BOOKS_H)
@pytest.mark.parametrize("dtype_name", sc.DTYPES)
def test_encoder_every_row_length_and_task_size(antq_lib, oracle, dev, dtype_name, name):
    """antq_encode4 on the same tensors: the encoder's own 8 / 4 / 3 / 2 rule, every task size forced (knob 0), the other store
    form of the 8-vector tasks (knob 13 = 1: nontemporal instead of plain stores), and the fp32-domain row encoder (knob 9 = 0);
    one scale per row and one per tensor.  The codes go into buffers of 0xA5 bytes that start 0, 4 and 12 bytes into a 16-byte
    line with at least 64 guard bytes on either side.  Codes == the oracle's scan-order indices as codes (an outlier its index
    in the outlier list, a victim 15, nothing within the scan's horizon the code of the grid's zero); guards, x and alpha
    untouched.  (A NaN in a row's last vector is in every idle lane's duplicate of it: those lanes take the rare path with
    nothing to store.)"""
    bk, plan, h, lims = _plan(antq_lib, name)
    _, g, gmax, nn, ovp = bk
    A = _arena(dev, dtype_name, name, lims)
    assert any(w == "nan" and e // 8 == c["rl"] // 8 - 1 for c in A.cs for _, e, w in c["planted"])
    assert {sc.encoder_u(sc.row_vpr(*s)) for s in sc.SHAPES} == {8, 4, 3, 2}
    for lead in (0, 4, 12):
        C = CodeArena(A, lead, dev)
        for kv in ENCODER_FORMS:
            with knobs(antq_lib, kv):
                for i, c in enumerate(A.cs):
                    got = antq_lib.encode4(A.xv[i], A.av[i], plan, gmax, c["rows"], c["rl"], c["per_row"], n_normal=nn, ovp=ovp, out=C.cv[i])
                    assert got.data_ptr() == C.cv[i].data_ptr()
            C.check((name, dtype_name, "lead", lead, kv))
    A.inputs_unchanged((name, dtype_name))


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the encoder along the scale axis
# ---------------------------------------------------------------------------------------------------------------------------
def _scale_axis_rows(rng, plan, gmax, dtype, alphas, K):
    """One row of K patterns per scale, built as test_16bit_domain_row_kernels_along_the_scale_axis builds them -- every slot
    boundary of the row's key range +/- 1, every threshold's pattern +/- 3, the row limit +/- 3, zeros / Inf / NaN / denormals /
    the largest finite values, random patterns -- and, new here, the DECISION limit flim16 +/- 3, which is what the encoder's
    sentinel slot compares against"""
    from test_gpu_modules_r5 import _to16
    hdr = plan.host[:128].view(np.uint32)
    n_thr, hshift, tl_off = int(hdr[25]), (int(hdr[27]) >> (8 * (dtype - 1))) & 0xff, int(hdr[28])
    T = plan.host[tl_off:tl_off + 16 * n_thr].view(np.float32).reshape(n_thr, 4)[:, 0].copy()
    flim = float(plan.host[:128].view(np.float32)[13]) * 0.99999
    lim = min(flim, float(plan.host[:128].view(np.float32)[17]))
    inf16 = 0x7f80 if dtype == 1 else 0x7c00
    special = np.uint16([0, 0x8000, inf16, inf16 | 0x8000, inf16 + 1, 0xffff, inf16 - 1, (inf16 - 1) | 0x8000, 1, 0x8001, 2, 0x7fff,
                         inf16 >> 1, 0x3c00 if dtype == 2 else 0x3f80])
    x16 = np.empty((len(alphas), K), np.uint16)
    for r, a in enumerate(alphas):
        with np.errstate(all="ignore"):
            s = np.float32(a) / np.float32(gmax)
            u = np.abs(T).astype(np.float32) * s
            limx = np.float32(min(lim * float(s) * 0.999, 3.0e38))
            flimx = np.float32(min(flim * float(s) * 0.999, 3.0e38))
        pu = _to16(u[np.isfinite(u) & (u > 0)], dtype).astype(np.int64)
        pl = int(_to16(np.float32([limx]), dtype)[0]) if limx > 0 else 0
        pf = int(_to16(np.float32([flimx]), dtype)[0]) if flimx > 0 else 0
        cand = [special.astype(np.int64)]
        for d in range(-3, 4):
            cand += [pu + d, np.int64([max(pl + d, 0)]), np.int64([max(pf + d, 0)])]
        k0 = max((int(pu.min()) >> hshift) - 2, 0) if pu.size else 0
        k1 = min((pl >> hshift) + 2, (0x7fff >> hshift))
        if k1 - k0 <= 200:
            edges = (np.arange(k0, k1 + 1, dtype=np.int64) << hshift)
            cand += [edges, edges + 1, np.maximum(edges, 1) - 1]
        mag = np.unique(np.clip(np.concatenate(cand).astype(np.int64), 0, 0x7fff)).astype(np.uint16)
        both = np.concatenate([mag, mag | 0x8000, special])
        if both.size > K - K // 8:
            both = rng.choice(both, K - K // 8, replace=False)
        row = np.concatenate([both, rng.integers(0, 65536, K - both.size).astype(np.uint16)])
        x16[r] = rng.permutation(row)
    return x16


@pytest.mark.parametrize("name", ("flint_b4_s", "int_b4_s", "flint_b4_u", "olive_flint"))
@pytest.mark.parametrize("dtype_name", sc.DTYPES)
def test_encoder_along_the_scale_axis(antq_lib, oracle, dev, dtype_name, name):
    """The encoder's counterpart of test_16bit_domain_row_kernels_along_the_scale_axis: 256 log-uniform scales plus both float32
    neighbours of every scale at which the row's table appears or disappears by the library's host model of the path -- the
    flips without and with the pair rule's overflow condition, which hrow_build_codes does not have: nothing is asserted about
    which model the encoder follows, both sets of scales are run -- each row holding the patterns that can go wrong at its scale,
    among them the decision limit's pattern +/- 3.  Rows of 4096 elements (one 8-vector task) and of 1032 (129 vectors: two
    tasks, the second one vector), ANT and OliVe.  Codes == the oracle's."""
    import ctypes
    import torch
    from test_gpu_modules_r5 import _f32_bits, _flip_scales
    bk, plan, h, lims = _plan(antq_lib, name)
    _, g, gmax, nn, ovp = bk
    L = antq_lib.lib()
    L.antq_plan_eval_host_h.restype = ctypes.c_int
    dtype = sc.DTYPE_CODE[dtype_name]
    rng = np.random.default_rng([79, dtype] + [ord(ch) for ch in name])
    flips = _flip_scales(L, plan, gmax, dtype, False) + _flip_scales(L, plan, gmax, dtype, True)
    assert flips
    lo_e, hi_e = (-10.0, 10.0) if dtype == 1 else (-6.5, 5.5)
    alphas = list(np.float32(10.0) ** rng.uniform(lo_e, hi_e, 256).astype(np.float32))
    for a, b in flips[:48]:
        for v in (a, b):
            bits = int(_f32_bits(v))
            alphas += [v, np.uint32(max(bits - 1, 1)).view(np.float32), np.uint32(bits + 1).view(np.float32)]
    alphas = np.unique(np.float32(alphas))
    alphas = alphas[np.isfinite(alphas) & (alphas > 0)]
    assert alphas.size >= 256 + 6
    at = torch.from_numpy(alphas).to(dev)
    for K in (4096, 1032):
        x16 = _scale_axis_rows(rng, plan, gmax, dtype, alphas, K)
        want = sc.oracle_codes(oracle, sc.widen16(oracle, x16, dtype_name), alphas, g, gmax, nn, ovp)
        xt = torch.from_numpy(x16.view(np.int16)).to(dev).view(getattr(torch, dtype_name))
        codes = antq_lib.encode4(xt, at, plan, gmax, alphas.size, K, True, n_normal=nn, ovp=ovp)
        got = torch.stack([(codes & 15), (codes >> 4)], 1).reshape(alphas.size, K).cpu().numpy().astype(np.int64)
        bad = got != want
        assert not bad.any(), (name, dtype_name, K, int(bad.sum()), alphas[np.argwhere(bad)[:3, 0]].tolist(),
                               [hex(int(v)) for v in x16[bad][:3]], got[bad][:3], want[bad][:3])
