"""The input builders and restated host rules of the given-scale 16-bit edge tests (static16_cases.py) against the CPU oracle and
the library's host code alone, no GPU: the row lengths reach every tail and task count they are meant to, the restated rules
route them as the C++ does, every row's head and tail tell a neighbour's scale from its own, the planted specials reach all
three branches of the rare path, no reference output is the poison pattern, and every restated mistake in mapping tasks onto
rows changes a compared element.  A failure of test_gpu_static16_edges.py is then the kernels', not the inputs'."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import fakequant_cases as fc
import static16_cases as sc


def _header(antq_lib, name):
    return fc.plan_header(antq_lib.plan_for(sc.book(name)[1]).host)


def _paths(antq_lib, name, dtype_name, x_row, alpha):
    """antq_plan_eval_host_h's path per element of one row: 0 table, 1 far-clipped arithmetic, 2 literal sequence"""
    bk = sc.book(name)
    L = antq_lib.lib()
    L.antq_plan_eval_host_h.restype = ctypes.c_int
    x = np.ascontiguousarray(x_row, np.uint16)
    out, path = np.empty(x.size, np.uint16), np.empty(x.size, np.uint8)
    rc = L.antq_plan_eval_host_h(antq_lib.plan_for(bk[1]).host_ptr(), x.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(x.size),
                                 ctypes.c_float(float(alpha)), ctypes.c_float(bk[2]), ctypes.c_int(sc.DTYPE_CODE[dtype_name]),
                                 ctypes.c_uint(1 if bk[4] else 0), out.ctypes.data_as(ctypes.c_void_p), path.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return path, out


def test_row_lengths_reach_every_tail_and_task_count():
    """Forced to 2 / 3 / 4 / 8 vectors per lane, VPRS gives last tasks of 0, 1, 63 .. 65, 127 .. 129, 191 .. 193 and 255 .. 257
    vectors in use and 1 .. 9 tasks per row; 5 rows keep task counts off multiples of 4 unless the tasks per row are one; the
    per-tensor shapes are ONE row of 128, 513 and 1025 vectors; under knob 9 = 2 the jobs' task counts reach every residue mod 4
    with both values of `rot` and every task size."""
    tails = {sc.last_task_vectors(v, u) for v in sc.VPRS for u in sc.US}
    assert tails >= {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257}, sorted(tails)
    for u in sc.US:                                  # per task size: an empty, a one-vector and an all-but-one-vector last task
        mine = {sc.last_task_vectors(v, u) for v in sc.VPRS}
        assert {0, 1, 64 * u - 1} <= mine, (u, sorted(mine))
    assert {sc.tpr_of(v, u) for v in sc.VPRS for u in sc.US} >= set(range(1, 10))
    assert sc.ROWS % 2 == 1 and [sc.row_vpr(*s, False) for s in sc.PER_TENSOR_SHAPES] == [128, 513, 1025]
    jobs = [(sc.ROWS * sc.tpr_of(v, sc.row_task_u(v)), sc.row_task_u(v), sc.rot_of(v, sc.row_task_u(v))) for v in sc.VPRS]
    assert {t % 4 for t, _, _ in jobs} == {0, 1, 2, 3} and {u for _, u, _ in jobs} == {2, 3, 4} and {r for _, _, r in jobs} == {0, 1}
    # the planted vectors: both ends of the row, both sides of every 64-vector step, the head of every partial last task
    assert sc.planted_vectors(129) == [0, 63, 64, 127, 128]
    for v in sc.VPRS:
        vs = set(sc.planted_vectors(v))
        assert {0, v - 1} <= vs and max(vs) == v - 1 and all(64 * k - 1 in vs for k in range(1, v // 64 + 1))
        assert all((v // (64 * u)) * 64 * u in vs for u in sc.US if v % (64 * u))


def _exact_best(vpr, us, margin):
    """_best_u in exact rational arithmetic (the margins 0.02 and 1e-9 as the doubles the C++ adds)"""
    best_u, best = 0, Fraction(-1)
    for u in us:
        util = Fraction(vpr, sc.tpr_of(vpr, u) * 64 * u)
        if util > best + Fraction(margin):
            best, best_u = util, u
    return best_u, best


def test_restated_rules_route_the_row_lengths():
    """hrow_static_u, row_task_u, the encoder's rule and rot, restated in floating point as the C++ has them, agree with exact
    rational arithmetic on every length from 128 to 1200 vectors (no decision of the rules sits within rounding of its margin);
    the switch points the rule has below 520 vectors are those csrc/antq_k_hrow.h was tuned around; an x-domain-eligible plan keeps
    K1h only where a 3- or 4-vector task fills its lanes to 93 %."""
    for v in range(128, 1201):
        u, best = _exact_best(v, (4, 3, 2), 0.02)
        want = 0 if (v < 192 or best < Fraction(0.93) or u < 3) else u
        assert sc.hrow_static_u(v, True) == want and sc.hrow_static_u(v, False) == u, v
        assert sc.row_task_u(v) == _exact_best(v, (4, 3, 2), 1e-9)[0] and sc.encoder_u(v) == _exact_best(v, (8, 4, 3, 2), 0.02)[0], v
    switches = [v for v in range(129, 520) if sc.hrow_static_u(v, True) != sc.hrow_static_u(v - 1, True)]
    assert switches == [192, 193, 239, 257, 358, 385, 477, 513], switches
    table = sc.routing_table(True)
    print("vpr: u by default (0: the fp32-domain row table) / u under knob 9 = 2 / encoder's u / rot by default")
    for v, u, u2, ue in table:
        print("  %4d: %d / %d / %d / %d" % (v, u, u2, ue, sc.rot_of(v, u) if u else 0))
    k1h = {v: u for v, u, _, _ in table if u}
    for v, u in k1h.items():
        assert u in (3, 4) and v >= 192 and v / (sc.tpr_of(v, u) * 64.0 * u) >= 0.93, (v, u)
    # both sides of every switch point are in the list: a kept row next to a handed-back one, for 3- and for 4-vector tasks
    assert all(a in k1h and b not in k1h for a, b in ((192, 193), (256, 257), (384, 385), (512, 513), (768, 769), (1024, 1025)))
    assert all(a not in k1h and b in k1h for a, b in ((191, 192), (238, 239), (476, 477)))
    assert {u for u in k1h.values()} == {3, 4} and 1089 in k1h and 128 not in k1h
    assert all(u for _, u, _, _ in sc.routing_table(False))                  # without the x-domain form no row is handed back
    assert {ue for _, _, _, ue in table} == {8, 4, 3, 2}
    # rot: a partial last task and an even number of tasks per row
    assert sc.rot_of(257, 2) == 0 and sc.rot_of(385, 2) == 1 and sc.rot_of(384, 2) == 0 and sc.rot_of(129, 2) == 1


@pytest.mark.parametrize("dtype_name", sc.DTYPES)
@pytest.mark.parametrize("name", sc.BOOKS_FWD)
def test_cases_hold_their_conditions(antq_lib, oracle, name, dtype_name):
    """Every tensor of the case set: (1) each row's first and last vector quantised with either neighbour's scale differ from the
    same with its own in an output pattern and in a code; (2) the plain rows stay on the table, the special rows reach the
    far-clipped arithmetic and the literal sequence at the planted elements, the rows without a table take the literal sequence
    everywhere -- by the library's host model of the path; (3) no reference output is the poison pattern; the scales of
    neighbouring rows are >= 1.5 x apart; with the pair rule the first and the last word of every row with a table hold a victim."""
    bk = sc.book(name)
    h = _header(antq_lib, name)
    assert h["hdom"] == 3 and bool(h["xdom"]) == (name != sc.BOOK_NO_XDOM)
    lims = sc.lims_of(h)
    seen = set()
    n_el = 0
    top = float(sc.widen16(oracle, np.uint16([sc.FMT[dtype_name]["max"]]), dtype_name)[0])
    for c in sc.cases(dtype_name, name, lims):
        x, out, codes = sc.as_rows(c)
        n, rl = x.shape
        alpha, kinds = c["alpha"], c["kinds"]
        tag = (name, dtype_name, c["rows"], c["rl"], c["per_row"])
        n_el += x.size
        assert alpha.shape == (n,) and kinds == (sc.ROW_KINDS if n > 1 else ("special",)), tag
        assert not (out == sc.POISON16).any(), tag
        ref_out, ref_codes = sc.reference_of(oracle, x, alpha, dtype_name, bk)
        assert np.array_equal(ref_out, out) and np.array_equal(ref_codes, codes), tag
        for r, q, where, d_out, d_code in sc.head_tail_differ(oracle, x, alpha, dtype_name, bk):
            assert d_out and d_code, (tag, r, q, where)
        ok = [k != "none" for k in kinds]
        for r in range(n - 1):
            if ok[r] and ok[r + 1]:
                assert max(alpha[r] / alpha[r + 1], alpha[r + 1] / alpha[r]) >= 1.5, (tag, r)
        _, ridx = oracle.forward(sc.widen16(oracle, x, dtype_name), alpha, bk[1], bk[2], bk[4])
        planted, paths_b = {}, set()
        for r, e, what in c["planted"]:
            planted.setdefault(r, []).append((e, what))
        for r, kind in enumerate(kinds):
            path, model = _paths(antq_lib, name, dtype_name, x[r], alpha[r])
            assert sc.same16(oracle, model, out[r], dtype_name).all(), (tag, r)          # (the host model is the oracle's equal here)
            if kind == "none":
                assert (path == 2).all(), (tag, r)
                seen.add(("none", float(alpha[r]) if np.isfinite(alpha[r]) else "nan"))
                continue
            if bk[4]:
                assert ridx[r, 1] == oracle.IDX_VICTIM and ridx[r, rl - 2] == oracle.IDX_VICTIM and ridx[r, 0] >= bk[3] and ridx[r, rl - 1] >= bk[3], (tag, r)
            if kind == "plain":
                assert (path == 0).all(), (tag, r, np.flatnonzero(path)[:4])
                continue
            whats = dict(planted[r])
            assert {e // 8 for e in whats} == set(sc.planted_vectors(rl // 8)), (tag, r)
            for e, what in whats.items():
                if what != "pair":
                    want = sc.RARE_OF[what]
                    if what == "limit":
                        lim16, hs = int(sc.limit16(oracle, alpha[r:r + 1], bk[2], lims, dtype_name)[0]), sc.hshift_of(lims, dtype_name)
                        assert (x[r, e] & 0x7fff) == lim16 and lim16 % (1 << hs) == 0 and (x[r, e - e % 8:e - e % 8 + 8] & 0x7fff).max() == lim16, (tag, r, e)
                        below, _ = _paths(antq_lib, name, dtype_name, np.full(8, lim16 - 1, np.uint16), alpha[r])
                        assert (below == 0).all(), (tag, r, "lim16 - 1 is not on the table")
                    if what == "max":              # (f16 and a scale near 1: 65504 / s can lie inside flim -- far-clipped, not literal)
                        want = 2 if top * bk[2] / float(alpha[r]) > lims[1] else 1
                    assert path[e] == want, (tag, r, e, what, int(path[e]))
                    seen.add(what)
            paths_b |= {int(p) for p in np.unique(path)}
            # rare only where planted: every other vector of the row stays on the table
            rare_vec = np.unique(np.flatnonzero(path) // 8)
            assert set(rare_vec) <= {e // 8 for e in whats}, (tag, r)
        assert paths_b == {0, 1, 2}, (tag, paths_b)                      # class (b) of every tensor: table, far-clipped, literal
    no_far = dtype_name == "float16" and name in sc.F16_WIDE_RANGE
    assert seen >= set(sc.SPECIALS_ALIGNED) - ({"far"} if no_far else set()) and len([s for s in seen if isinstance(s, tuple)]) == 4, seen
    assert 500000 < n_el < 600000
    print("case set held to its conditions:", name, dtype_name, n_el, "elements")


@pytest.mark.parametrize("dtype_name", sc.DTYPES)
@pytest.mark.parametrize("name", ("flint_b4_s", "olive_flint"))
def test_every_restated_mistake_changes_a_compared_element(antq_lib, oracle, name, dtype_name):
    """Each mistake of static16_cases.MISTAKES, restated in numpy for 2 / 3 / 4 / 8 vectors per lane, changes at least one output
    pattern and -- where it says anything about the codes -- at least one code in EVERY tensor in which it has meaning, and has
    meaning in some tensor for every task size.  The far-clipped element sent through the literal sequence instead is no mistake:
    the literal sequence is the reference (that is the oracle itself), so nothing can differ."""
    bk = sc.book(name)
    lims = sc.lims_of(_header(antq_lib, name))
    caught = {(k, u): 0 for k in sc.MISTAKES for u in sc.US}
    for c in sc.cases(dtype_name, name, lims):
        _, out, codes = sc.as_rows(c)
        for kind in sc.MISTAKES:
            for u in sc.US:
                got = sc.mistaken(oracle, kind, c, dtype_name, bk, lims, u)
                if got is None:
                    continue
                tag = (name, dtype_name, c["rows"], c["rl"], c["per_row"], kind, u)
                assert (~sc.same16(oracle, got[0], out, dtype_name)).any(), tag
                assert got[1] is None or (got[1] != codes).any(), tag
                caught[(kind, u)] += 1
    print("tensors that tell each mistake from the right mapping:", name, dtype_name, caught)
    assert all(n > 0 for n in caught.values()), caught


def _built_descs(antq_lib, shapes, plan, gmax, dtype_name):
    """antq_batch_build (host code) on jobs of these shapes at made-up device addresses: [(kind, u, rot, vpr, tpr, tasks)]"""
    from ant_quantization_amd._lib import _Job
    L = antq_lib.lib()
    arr = (_Job * len(shapes))()
    for k, (rows, rl, per_row) in enumerate(shapes):
        arr[k] = _Job(0x10000000 + 0x1000000 * k, 0x50000000 + 0x1000000 * k, 0x90000000, rows, rl, 1 if per_row else 0, gmax,
                      plan.host_addr, 0xa0000000)
    cap = L.antq_batch_capacity(arr, len(shapes), sc.DTYPE_CODE[dtype_name])
    host = np.zeros(cap, np.uint8)
    n = L.antq_batch_build(arr, len(shapes), sc.DTYPE_CODE[dtype_name], 0, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap))
    assert n > 0, n
    d = [host[80 + 192 * k:80 + 192 * (k + 1)] for k in range(len(shapes))]
    return [tuple(int(v[at:at + 4].view(np.uint32)[0]) for at in (60, 148, 152, 44, 48, 40)) for v in d], host[:80].view(np.uint32)[8:17].tolist()


@pytest.mark.parametrize("dtype_name", sc.DTYPES)
@pytest.mark.parametrize("name", ("flint_b4_s", sc.BOOK_NO_XDOM))
def test_batch_builder_files_the_jobs_as_the_restated_rules_say(antq_lib, name, dtype_name):
    """antq_batch_build is host code: without a GPU, a job of every shape alone is kind 13 with hrow_static_u's task size, rot and
    task count (one row for a tensor with one scale) or, handed back, kind 2; with knob 9 = 2 all shapes in one batch are kind 13
    by row_task_u in ONE family-5 launch whose map has one entry per four tasks of each job."""
    bk = sc.book(name)
    plan = antq_lib.plan_for(bk[1])
    xdom = bool(fc.plan_header(plan.host)["xdom"])

    def want(s, u):
        vpr = sc.row_vpr(*s)
        return (13, u, sc.rot_of(vpr, u), vpr, sc.tpr_of(vpr, u), (s[0] if s[2] else 1) * sc.tpr_of(vpr, u))

    for s in sc.SHAPES:
        (d,), fam = _built_descs(antq_lib, [s], plan, bk[2], dtype_name)
        u = sc.hrow_static_u(sc.row_vpr(*s), xdom)
        assert (d == want(s, u) and fam[5] == (d[5] + 3) // 4) if u else (d[0] == 2 and fam[5] == 0 and xdom), (s, d, fam)
    try:
        antq_lib.lib().antq_debug_set(9, 2)
        ds, fam = _built_descs(antq_lib, list(sc.SHAPES), plan, bk[2], dtype_name)
    finally:
        antq_lib.lib().antq_debug_set(9, 1)
    assert ds == [want(s, sc.row_task_u(sc.row_vpr(*s))) for s in sc.SHAPES]
    assert fam[5] == sum((d[5] + 3) // 4 for d in ds) and sum(fam) == fam[5]
