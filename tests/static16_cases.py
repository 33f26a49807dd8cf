"""Input builders and restated host rules for the edge tests of the GIVEN-scale 16-bit-domain row kernels (k_fq_hrow, k_fq_hbatch
and k_encode4_hrow of csrc/antq_k_hrow.h / antq_k_codec.h: test_gpu_static16_edges.py) and for the host test that holds the
builders to their conditions with the CPU oracle alone (test_static16_cases_host.py).  numpy and the oracle only; books, widen16,
round16, forward16, same16, FMT, vector_positions and oracle_codes come from fakequant_cases, dynamic16_cases and encode4_cases.
New here: the row lengths at every switch point of the rules that cut a row into tasks, those rules restated in Python, rows
whose scales tell a wrong row index apart in head and tail, specials planted wherever a task, a vector step or a lane group ends,
and numpy restatements of the wrong ways to map tasks onto rows (which the case set must tell from the right one)."""
import functools

import numpy as np

from dynamic16_cases import BOOKS_H, DTYPES, FMT, forward16, same16, vector_positions  # noqa: F401
from encode4_cases import oracle_codes  # noqa: F401
from fakequant_cases import book, round16, widen16  # noqa: F401

# the one reference codebook whose plan has the 16-bit-domain form (PlanHeader::hdom) but not the fp32-domain row table (xdom):
# hrow_static_u then never hands a row back.  64 entries: no packed 4-bit form, the forward tests only.
BOOK_NO_XDOM = "float4_b6_s"
BOOKS_FWD = BOOKS_H + (BOOK_NO_XDOM,)
DTYPE_CODE = dict(bfloat16=1, float16=2)               # include/antq.h ANTQ_BF16 / ANTQ_F16
POISON16 = 0x5a5a                                      # a FINITE pattern in both formats: it differs from a NaN output too
POISON_CODE = 0xa5
SEED = 1613

# ---------------------------------------------------------------------------------------------------------------------------
# 1: shapes (row length = 8 x vectors per row)
# ---------------------------------------------------------------------------------------------------------------------------
VPRS = (128, 129, 191, 192, 193, 238, 239, 255, 256, 257, 320, 321, 383, 384, 385, 476, 477, 511, 512, 513, 577, 767, 768, 769,
        1023, 1024, 1025, 1089)
ROWS = 5                                               # odd: no job's task count is a multiple of 4 by the row count alone
PER_TENSOR_SHAPES = ((1, 8 * 128), (3, 8 * 171), (5, 8 * 205))        # alpha_per_row = 0: ONE row of 128 / 513 / 1025 vectors
US = (2, 3, 4, 8)                                      # vectors per lane and task the kernels are compiled for
SHAPES = tuple((ROWS, 8 * v, True) for v in VPRS) + tuple((r, rl, False) for r, rl in PER_TENSOR_SHAPES)


def row_vpr(rows, rl, per_row):
    """vectors of what the kernels take for a ROW: the row, or -- one scale for the tensor -- the whole tensor"""
    return (rl if per_row else rows * rl) // 8


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the host rules, restated
# ---------------------------------------------------------------------------------------------------------------------------
def tpr_of(vpr, u):
    return -(-vpr // (64 * u))


def _best_u(vpr, us, margin):
    """the first u of `us` whose lane utilisation beats the best one before it by more than `margin`: (u, utilisation)"""
    best_u, best = 0, -1.0
    for u in us:
        util = vpr / float(tpr_of(vpr, u) * 64 * u)
        if util > best + margin:
            best, best_u = util, u
    return best_u, best


def hrow_static_u(vpr, have_xdom):
    """csrc/antq_k_hrow.h hrow_static_u: 4 / 3 / 2 vectors per lane and task, or 0 where a plan with the fp32-domain row table
    keeps the row (short rows, rows that only split into tasks with many idle lanes, 2-vector tasks)"""
    u, best = _best_u(vpr, (4, 3, 2), 0.02)
    if have_xdom and (vpr < 192 or best < 0.93 or u < 3):
        return 0
    return u


def row_task_u(vpr):
    """csrc/antq_device.h row_task_u (knob 9 = 2: every row in the 16-bit domain): best utilisation, ties to the larger task"""
    return _best_u(vpr, (4, 3, 2), 1e-9)[0]


def encoder_u(vpr):
    """csrc/antq_k_codec.h launch_encode4: the largest of 8 / 4 / 3 / 2 that keeps the lanes of a row's tasks busy"""
    return _best_u(vpr, (8, 4, 3, 2), 0.02)[0]


def rot_of(vpr, u):
    """antq_batch_build: a partial last task and an even number of tasks per row -> the rotated workgroup -> task map"""
    return int(vpr % (64 * u) != 0 and tpr_of(vpr, u) % 2 == 0)


def last_task_vectors(vpr, u):
    """vectors in use in a row's last task (0: the row ends on a task boundary, the last task is whole)"""
    return vpr % (64 * u)


def routing_table(have_xdom=True):
    """[(vpr, u by default or 0, u under knob 9 = 2, encoder's u)] for VPRS"""
    return [(v, hrow_static_u(v, have_xdom), row_task_u(v), encoder_u(v)) for v in VPRS]


# ---------------------------------------------------------------------------------------------------------------------------
# 3: data
# ---------------------------------------------------------------------------------------------------------------------------
def lims_of(h):
    """(lim, flim, hshift word) of csrc/antq_k_hrow.h hargs_from_plan from a plan header (fakequant_cases.plan_header): |x / s|
    below lim -- the table is the whole story; below flim -- the table still decides; beyond -- the literal scan; a slot of the
    row's table holds the patterns that agree above bit hshift (byte 0 of the word: bf16, byte 1: f16)"""
    flim = np.float32(h["fastlim"]) * np.float32(0.99999)
    return float(min(flim, np.float32(h["xlim"]))), float(flim), int(h["hshift"])


def hshift_of(lims, dtype_name):
    return (lims[2] >> (8 * (DTYPE_CODE[dtype_name] - 1))) & 0xff


def limit16(oracle, alpha, gmax, lims, dtype_name):
    """hrow_build's lim16 for rows of these scales (array): the largest pattern whose value is <= fl(fl(lim * s) * 0.999), s the
    row's scale as row_scale forms it, fl32(alpha * (1 / gmax)) in double.  Patterns from lim16 on read the sentinel."""
    s = (np.asarray(alpha, np.float32).astype(np.float64) * (1.0 / np.float64(np.float32(gmax)))).astype(np.float32)
    with np.errstate(all="ignore"):
        limx = ((np.float32(lims[0]) * s).astype(np.float32) * np.float32(0.999)).astype(np.float32)
        p = round16(oracle, limx, dtype_name).astype(np.int64)
        return p - (widen16(oracle, p.astype(np.uint16), dtype_name) > limx)


def aligned_alpha(oracle, a0, gmax, lims, dtype_name):
    """the first scale from a0 upwards (steps of 2^-12, at most a factor 2) for which lim16 is the FIRST pattern of its slot: only
    then does the rare path's "is this vector's largest magnitude in the sentinel slot" decide on equality"""
    a = (np.float32(a0) * (1.0 + np.arange(1 << 12) * 2.0 ** -12)).astype(np.float32)
    ok = np.flatnonzero(limit16(oracle, a, gmax, lims, dtype_name) % (1 << hshift_of(lims, dtype_name)) == 0)
    return np.float32(a[ok[0]]) if ok.size else None


ROW_KINDS = ("plain", "special", "none", "special", "special")
SPECIALS = ("+inf", "mid", "nan", "far", "-inf", "max")
# the last special row of a tensor has a scale for which lim16 starts a slot, and "limit" among its specials: the pattern lim16
# itself, the largest magnitude of its vector
SPECIALS_ALIGNED = SPECIALS[:3] + ("limit",) + SPECIALS[3:]
RARE_OF = {"+inf": 2, "-inf": 2, "nan": 2, "far": 2, "max": 2, "mid": 1, "limit": 1}      # antq_plan_eval_host_h's path of the element


def none_alphas(dtype_name):
    """scales that leave a row without a table: zero, negative, NaN, and one below the table path's range"""
    return np.float32([0.0, -0.37, np.nan, 1e-30 if dtype_name == "bfloat16" else 6e-8])


def planted_vectors(vpr):
    """vector_positions(vpr), the row's first and last vector, vectors 64 k - 1 and 64 k, and the first vector of the partial
    last task for each of 2 / 3 / 4 / 8 vectors per lane"""
    vs = set(vector_positions(vpr)) | {0, vpr - 1}
    for k in range(1, vpr // 64 + 1):
        vs.add(64 * k - 1)
        if 64 * k < vpr:
            vs.add(64 * k)
    for u in US:
        if vpr % (64 * u):
            vs.add((vpr // (64 * u)) * 64 * u)
    return sorted(vs)


def special_pattern(oracle, kind, dtype_name, s, lims, negative):
    """the 16-bit pattern of one special for a row of scale s, or None where the format has no such value"""
    F = FMT[dtype_name]
    lim, flim = lims[:2]
    if kind in ("+inf", "-inf"):
        return F["inf"] | (0x8000 if kind == "-inf" else 0)
    if kind == "nan":
        return F["nan"] | (0x8000 if negative else 0)
    if kind == "max":
        return F["max"] | (0x8000 if negative else 0)
    v = float(np.sqrt(lim * flim)) * float(s) if kind == "mid" else 4.0 * flim * float(s)
    top = float(widen16(oracle, np.uint16([F["max"]]), dtype_name)[0])
    if not (np.isfinite(v) and 0 < v < top / 2) or (kind == "mid" and not flim > 1.5 * lim):
        return None
    with np.errstate(all="ignore"):
        p = int(round16(oracle, np.float32([v]), dtype_name)[0])
    return p | (0x8000 if negative else 0)


# f16 rows of the 6-bit float book have a table from alpha = 1 up (its smallest thresholds are 2e-5 of the largest: below, they
# fall among f16's subnormals); 4 * flim * s is then no finite f16, so these rows have no "far" special (the largest finite
# pattern stands in), and their "mid" one stays finite up to alpha = 200
F16_WIDE_RANGE = {BOOK_NO_XDOM: (1.0, 200.0)}


def _alphas(rng, dtype_name, name, gmax, lims, n):
    """n log-uniform scales, neighbours at least 1.5 x apart; for f16 small enough that 4 * flim * s is a finite f16"""
    hi = 30.0 if dtype_name == "bfloat16" else min(30.0, 65504.0 * gmax / (16.0 * lims[1]))
    lo = hi / 400.0               # (f16: a scale a few times smaller puts the thresholds among the subnormals and the row loses its table)
    if dtype_name == "float16" and name in F16_WIDE_RANGE:
        lo, hi = F16_WIDE_RANGE[name]
    while True:
        a = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)
        r = a[1:] / a[:-1]
        if n == 1 or (np.maximum(r, 1 / r) >= 1.5).all():
            return a


def _draw(oracle, rng, dtype_name, bk, lims, rows, rl, per_row, shape_no):
    name, g, gmax, nn, ovp = bk
    lim, flim = lims[:2]
    vpr = row_vpr(rows, rl, per_row)
    n_rows, row_len = (rows, rl) if per_row else (1, rows * rl)
    kinds = ROW_KINDS[:n_rows] if n_rows > 1 else ("special",)
    alpha = _alphas(rng, dtype_name, name, gmax, lims, n_rows)
    last_special = max(r for r, k in enumerate(kinds) if k == "special")
    a = aligned_alpha(oracle, alpha[last_special], gmax, lims, dtype_name)
    if a is None or (last_special and max(a / alpha[last_special - 1], alpha[last_special - 1] / a) < 1.5):
        return None
    alpha[last_special] = a
    # values uniform over about +/-2 alpha, kept inside the table (|x / s| < 0.9 lim) so that a plain row never leaves it; the row
    # without a table holds values between its neighbours' (their scales must tell on it, and its own on them)
    c = min(2.0, 0.9 * lim / gmax)
    mag = alpha.copy()
    if "none" in kinds:
        r = kinds.index("none")
        mag[r] = np.sqrt(alpha[r - 1] * alpha[r + 1])
        alpha[r] = none_alphas(dtype_name)[shape_no % 4]
    with np.errstate(all="ignore"):
        x = round16(oracle, (rng.uniform(-c, c, (n_rows, row_len)) * mag[:, None]).astype(np.float32), dtype_name)
    planted = []
    vs = planted_vectors(vpr)
    n_special = 0
    for r, kind in enumerate(kinds):
        if kind == "none":
            continue
        s = np.float32(alpha[r]) / np.float32(gmax)
        if ovp:
            # outlier / victim pairs in the row's first word (the odd element is the victim) and in its last (the even one)
            with np.errstate(all="ignore"):
                pats = round16(oracle, np.float32([3.1, 0.5, -0.4, -2.9]) * alpha[r], dtype_name)
            x[r, 0], x[r, 1], x[r, row_len - 2], x[r, row_len - 1] = pats
            planted += [(r, 0, "pair"), (r, row_len - 2, "pair")]
        if kind != "special":
            continue
        for k, v in enumerate(vs):
            pool = SPECIALS_ALIGNED if r == last_special else SPECIALS
            what = pool[(k + 2) % len(pool)] if r == last_special else pool[(k + 2 * n_special) % len(pool)]      # ("limit" second)
            if what == "limit":
                p = int(limit16(oracle, alpha[r:r + 1], gmax, lims, dtype_name)[0]) | (0x8000 if (k + r) % 2 else 0)
            else:
                p = special_pattern(oracle, what, dtype_name, s, lims, negative=bool((k + r) % 2))
            if p is None:
                what = "max"
                p = special_pattern(oracle, what, dtype_name, s, lims, negative=bool((k + r) % 2))
            e = 8 * v + 2 + (k + n_special) % 4                  # slots 2 .. 5 of the vector: its words 0 and 3 stay as drawn
            x[r, e] = p
            planted.append((r, e, what))
        n_special += 1
    return x, alpha, kinds, planted


def neighbour_rows(n_rows):
    return [(r, q) for r in range(n_rows) for q in (r - 1, r + 1) if 0 <= q < n_rows]


def head_tail_differ(oracle, x, alpha, dtype_name, bk):
    """Per (row r, neighbour q, 'head' | 'tail'): do the row's first / last vector quantised with row q's scale differ from
    the same with its own -- in an output pattern, and in a code?  [(r, q, where, outputs differ, codes differ)]"""
    name, g, gmax, nn, ovp = bk
    out = []
    for r, q in neighbour_rows(x.shape[0]):
        for where, sl in (("head", slice(0, 8)), ("tail", slice(x.shape[1] - 8, x.shape[1]))):
            v = np.ascontiguousarray(x[r:r + 1, sl])
            a_r, a_q = alpha[r:r + 1], alpha[q:q + 1]
            d_out = (~same16(oracle, forward16(oracle, v, dtype_name, bk, a_r), forward16(oracle, v, dtype_name, bk, a_q), dtype_name)).any()
            vf = widen16(oracle, v, dtype_name)
            d_code = (oracle_codes(oracle, vf, a_r, g, gmax, nn, ovp) != oracle_codes(oracle, vf, a_q, g, gmax, nn, ovp)).any()
            out.append((r, q, where, bool(d_out), bool(d_code)))
    return out


def reference_of(oracle, x, alpha, dtype_name, bk):
    """(output patterns, codes as one nibble per element) of the oracle for x [rows, row_len] with one scale per row"""
    name, g, gmax, nn, ovp = bk
    return forward16(oracle, x, dtype_name, bk, alpha), oracle_codes(oracle, widen16(oracle, x, dtype_name), alpha, g, gmax, nn, ovp)


@functools.lru_cache(maxsize=None)
def case(dtype_name, name, lims, rows, rl, per_row):
    """One tensor.  Rows by class: (a) a plain row (inside the table everywhere); (b) rows with the specials -- +/-Inf, NaN, a
    finite element between lim and flim, one beyond flim, the largest finite pattern -- planted at planted_vectors, the last of
    them at a scale for which the row limit's pattern starts a slot of the table, with that pattern among its specials; (c) a row
    whose scale leaves it without a table (0, negative, NaN, tiny: alternating over the shapes); for a book with the pair rule
    outlier / victim pairs in the first and in the last word of every row with a table.  Distinct log-uniform scales, neighbours
    at least 1.5 x apart, values uniform over +/-2 alpha.  Re-drawn until: every row's first and last vector quantise differently
    (outputs and codes) with either neighbour's scale; a row's last vector with its own scale differs from the next row's first
    vector (outputs and codes); no reference output is the poison pattern.
    dict(x uint16 [rows, rl], alpha float32 [rows or 1], kinds, planted [(row, element, what)], out, codes, rows, rl, per_row):
    out / codes the oracle's, shaped like x; everything read-only."""
    from oracle import antq_oracle as oracle
    bk = book(name)
    shape_no = SHAPES.index((rows, rl, per_row))
    for attempt in range(64):
        rng = np.random.default_rng([SEED, shape_no, DTYPE_CODE[dtype_name], attempt] + [ord(ch) for ch in name])
        drawn = _draw(oracle, rng, dtype_name, bk, lims, rows, rl, per_row, shape_no)
        if drawn is None:
            continue
        x, alpha, kinds, planted = drawn
        out, codes = reference_of(oracle, x, alpha, dtype_name, bk)
        if (out == POISON16).any():
            continue
        if not all(o and c for _, _, _, o, c in head_tail_differ(oracle, x, alpha, dtype_name, bk)):
            continue
        spill = duplicate_spill(oracle, x, alpha, dtype_name, bk)
        if spill is not None and not ((spill[0][1:, :8] != out[1:, :8]).any(axis=1).all() and (spill[1][1:, :8] != codes[1:, :8]).any(axis=1).all()):
            continue
        break
    else:
        raise AssertionError("no draw meets the conditions", dtype_name, name, rows, rl, per_row)
    shape = (rows, rl)
    res = dict(x=x.reshape(shape), alpha=alpha, kinds=kinds, planted=tuple(planted), out=out.reshape(shape), codes=codes.reshape(shape),
               rows=rows, rl=rl, per_row=per_row, attempt=attempt)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def cases(dtype_name, name, lims):
    """every tensor of SHAPES for one (type, book): about 0.55 M elements, the oracle's work done once per process"""
    return [case(dtype_name, name, lims, *s) for s in SHAPES]


def as_rows(c):
    """(x, out, codes) as the kernels see the rows: [rows, rl], or [1, rows * rl] for a tensor with one scale"""
    n = c["rows"] if c["per_row"] else 1
    return c["x"].reshape(n, -1), c["out"].reshape(n, -1), c["codes"].reshape(n, -1)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: wrong ways to map tasks onto rows, restated
# ---------------------------------------------------------------------------------------------------------------------------
# (An element between lim and flim sent through the literal sequence instead of the far-clipped arithmetic is no mistake: the
#  literal sequence IS the reference, nothing can differ.  The far-clipped arithmetic left out -- the table's fl16(q * s) alone --
#  is none for these books either: their extreme values are integers, and (q - d) + d == q for every |d| < flim < 2^24.)
MISTAKES = ("last vector not written", "duplicate lanes one slot on", "neighbour row's scale", "tpr of another U", "sentinel kept",
            "element beyond flim by the table's decision", "vector whose largest pattern starts the sentinel slot not redone")


def poison_codes(shape):
    """the nibbles of a buffer of POISON_CODE bytes, one per element (the low nibble is the even element's)"""
    out = np.empty(shape, np.int64)
    out[..., 0::2], out[..., 1::2] = POISON_CODE & 15, POISON_CODE >> 4
    return out


def duplicate_spill(oracle, x, alpha, dtype_name, bk):
    """(out, codes) when the idle lanes of a row's last task -- they hold a duplicate of the row's last vector -- store it one
    slot on: the next row's first vector becomes row r's last one, quantised with row r's scale.  None for a single row (the
    store then lands in the guard band)."""
    if x.shape[0] < 2:
        return None
    out, codes = reference_of(oracle, x, alpha, dtype_name, bk)
    o_t, c_t = reference_of(oracle, np.ascontiguousarray(x[:, -8:]), alpha, dtype_name, bk)
    out, codes = out.copy(), codes.copy()
    out[1:, :8], codes[1:, :8] = o_t[:-1], c_t[:-1]
    return out, codes


def mistaken(oracle, kind, c, dtype_name, bk, lims, u):
    """(out, codes) of tensor c under one mistake made with u vectors per lane and task, shaped [rows, row length] as
    as_rows(c); an entry is None where the mistake says nothing about it, the whole result where it has no meaning here"""
    name, g, gmax, nn, ovp = bk
    lim, flim = lims[:2]
    x, out, codes = as_rows(c)
    alpha = c["alpha"]
    n, rl = x.shape
    vpr = rl // 8
    out, codes = out.copy(), codes.copy()
    xf = widen16(oracle, x, dtype_name)
    with np.errstate(all="ignore"):
        s = (alpha.astype(np.float32) / np.float32(gmax)).astype(np.float32)[:, None]
        d = np.abs(xf / s)
        table = np.array([k != "none" for k in c["kinds"]])[:, None] & np.ones_like(x, bool)
    if kind == "last vector not written":
        out[:, -8:], codes[:, -8:] = POISON16, poison_codes((n, 8))
        return out, codes
    if kind == "duplicate lanes one slot on":
        return duplicate_spill(oracle, x, alpha, dtype_name, bk) if last_task_vectors(vpr, u) else None
    if kind == "neighbour row's scale":
        if n < 2:
            return None
        return reference_of(oracle, x, alpha[np.minimum(np.arange(n) + 1, n - 1)], dtype_name, bk)
    if kind == "tpr of another U":
        # the launcher cuts the rows for u + 1 vectors per lane, the kernel walks them with u: fewer tasks per row leave its tail
        # unwritten (more tasks per row only add tasks whose every lane is past the row end)
        t = tpr_of(vpr, u + 1)
        if t == tpr_of(vpr, u):
            return None
        out[:, 8 * 64 * u * t:], codes[:, 8 * 64 * u * t:] = POISON16, poison_codes((n, rl - 8 * 64 * u * t))
        return out, codes
    if kind == "sentinel kept":
        # the rare path never runs: an element at or beyond the row's limit keeps what the sentinel slot holds -- the output
        # 0xffff; the code byte 0x80 (encoder: from flim on), which the pair rule's masks turn into code 0 and which without them
        # leaks into the odd neighbour's nibble
        far_o, far_c = table & ~(d < lim), table & ~(d < flim)
        if not far_o.any():
            return None
        out[far_o] = 0xffff
        if ovp:
            codes[far_c] = 0
        else:
            a, b = np.where(far_c[:, 0::2], 0x80, codes[:, 0::2]), np.where(far_c[:, 1::2], 0x80, codes[:, 1::2])
            byte = (a | (b << 4)) & 0xff
            carry = np.zeros_like(byte)
            carry[:, 1:] = (b[:, :-1] << 4) >> 8                 # (B << 4 within the 32-bit word: bit 11 of byte i lands in byte i + 1)
            carry[:, 0::4] = 0
            byte |= carry
            codes[:, 0::2], codes[:, 1::2] = byte & 15, byte >> 4
        return out, codes
    if kind == "vector whose largest pattern starts the sentinel slot not redone":
        # the forward only: the encoder's sentinel sits at flim16, far above the slot's first pattern
        for r, e, what in c["planted"]:
            if what == "limit":
                out[r if c["per_row"] else 0, e] = 0xffff
        return out, None
    q_ext = np.where(xf > 0, np.float32(g.max()), np.float32(g.min())).astype(np.float32) + np.float32(0)
    if kind == "element beyond flim by the table's decision":
        m = table & np.isfinite(xf) & (d >= flim * 1.01)
        if not m.any():
            return None
        with np.errstate(all="ignore"):
            dd = (xf / s).astype(np.float32)
            out[m] = round16(oracle, (((q_ext - dd).astype(np.float32) + dd).astype(np.float32) * s).astype(np.float32), dtype_name)[m]
        ext = np.where(xf > 0, int(np.argmax(g)), int(np.argmin(g)))
        if not ovp:
            codes[m] = ext[m]
        return out, codes if not ovp else None
    raise KeyError(kind)
