"""The kernels that replace the reference's operators one for one, where a decision can flip: antq_nearest (fp32 and float64,
the per-workgroup grid analysis of k_nearest_fast and the literal scan), antq_nearest_plan / antq_nearest_hinted (fp32, bf16,
f16; table, big-table and scan plans; stale beliefs), antq_affine (vector and element kernel) and antq_fakequant_f64.

The yardstick is oracle.nearest / oracle.affine on the same inputs and, for the float64 forward, the numpy-float64 restatement
of the reference's sequence (operator_cases.f64_forward_ref).  Values compare as bit patterns (NaN matches NaN), indices
exactly; nothing on the expected side of an assert comes from the HIP library.  The inputs are built by operator_cases.py,
which test_operator_cases_host.py holds to their conditions without a GPU.  Every output is a view into a poisoned buffer
with 64 guard elements on either side, which must be unchanged after the launch; the entry points are called through the C
ABI so that the test owns those buffers."""
import contextlib
import ctypes

import numpy as np
import pytest

import operator_cases as oc

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {3: 1}
F32, BF16, F16, F64 = 0, 1, 2, 3
ERR_ARG, ERR_UNSUPPORTED = -1, -2
DT16 = {"bfloat16": BF16, "float16": F16}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def knobs(antq_lib, kv):
    """knobs(lib, {3: 0}): set, run, restore the defaults"""
    try:
        for k, v in kv.items():
            antq_lib.lib().antq_debug_set(k, v)
        yield
    finally:
        for k in kv:
            antq_lib.lib().antq_debug_set(k, KNOB_DEFAULTS[k])


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
class Out:
    """n elements inside a buffer filled with a poison pattern, oc.GUARD (+ lead) elements before them and oc.GUARD behind"""
    KINDS = dict(f32=("int32", oc.POISON32), f64=("int64", oc.POISON64), h16=("int16", oc.POISON16), idx=("int16", oc.POISON_IDX),
                 q=("int32", oc.POISON_Q))

    def __init__(self, n, kind, dev, lead=0):
        import torch
        dt, self.poison = self.KINDS[kind]
        self.lo, self.n = oc.GUARD + lead, n
        self.buf = torch.full((self.lo + n + oc.GUARD,), self.poison, dtype=getattr(torch, dt), device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + n]
        self.ptr = self.view.data_ptr()

    def bits(self, tag):
        """the n elements as unsigned integers, after checking that every guard element still holds the poison"""
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == self.poison).all() and (b[self.lo + self.n:] == self.poison).all(), (tag, "guard elements changed")
        v = b[self.lo:self.lo + self.n]
        return v.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[v.itemsize])


def _dev(a, dev, lead=0):
    """a numpy array's bytes on the device, starting `lead` elements off a 16-byte boundary"""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    it = {2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]
    full = torch.zeros(a.size + 16, dtype=getattr(torch, np.dtype(it).name), device=dev)
    t = full[lead:lead + a.size]
    t.copy_(torch.from_numpy(a.view(it).copy()))
    assert t.data_ptr() % 16 == lead * a.itemsize % 16
    return t


def _vp(t):
    return ctypes.c_void_p(0 if t is None else t if isinstance(t, int) else t.ptr if isinstance(t, Out) else t.data_ptr())


def _same(got, want, x, tag):
    """bit patterns equal, NaN matching NaN"""
    want = np.ascontiguousarray(want).reshape(-1)
    wb = want.view(got.dtype)
    ft = {2: None, 4: np.float32, 8: np.float64}[got.itemsize]
    nan = (np.isnan(got.view(ft)) & np.isnan(want)) if ft is not None and want.dtype.kind == "f" else np.zeros(got.size, bool)
    bad = np.flatnonzero((got != wb) & ~nan)
    xb = np.ascontiguousarray(x).reshape(-1)
    assert bad.size == 0, (tag, "%d of %d values differ" % (bad.size, got.size), "at", bad[:6].tolist(), "x", [repr(v) for v in xb[bad[:6]]],
                           "got", [hex(int(v)) for v in got[bad[:6]]], "want", [hex(int(v)) for v in wb[bad[:6]]])


def _same_idx(got, want, x, tag):
    got, want = got.view(np.int16).astype(np.int32), np.asarray(want).reshape(-1)
    bad = np.flatnonzero(got != want)
    xb = np.ascontiguousarray(x).reshape(-1)
    assert bad.size == 0, (tag, "%d of %d indices differ" % (bad.size, got.size), "at", bad[:6].tolist(), "x", [repr(v) for v in xb[bad[:6]]],
                           "got", got[bad[:6]].tolist(), "want", want[bad[:6]].tolist())


def _oracle_nearest(oracle, x, g):
    with np.errstate(all="ignore"):
        return oracle.nearest(x, g)


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: antq_nearest
# ---------------------------------------------------------------------------------------------------------------------------
def _nearest_rc(antq_lib, dev, xt, z, idx, n, gt, m, dt):
    return antq_lib.lib().antq_nearest(_vp(xt), _vp(z), _vp(idx), ctypes.c_size_t(n), _vp(gt), ctypes.c_int(m), ctypes.c_int(dt),
                                       antq_lib._stream(dev))


def _check_nearest(antq_lib, oracle, dev, x, g, tag):
    """x, g: both float32 or both float64.  Both settings of knob 3, with and without the index output."""
    f64 = x.dtype == np.float64
    assert g.dtype == x.dtype
    zr, jr = _oracle_nearest(oracle, x, g)
    assert zr.dtype == x.dtype
    xt, gt = _dev(x, dev), _dev(g, dev)
    for fast in (1, 0):
        for want_idx in (True, False):
            z = Out(x.size, "f64" if f64 else "f32", dev)
            idx = Out(x.size, "idx", dev) if want_idx else None
            with knobs(antq_lib, {3: fast}):
                rc = _nearest_rc(antq_lib, dev, xt, z, idx, x.size, gt, g.size, F64 if f64 else F32)
            assert rc == 0, (tag, rc)
            t = tag + (x.size, "fast" if fast else "scan", want_idx)
            _same(z.bits(t), zr, x, t)
            if want_idx:
                _same_idx(idx.bits(t), jr, x, t)


@pytest.mark.parametrize("name", sorted(oc.nearest_grids()))
def test_nearest_fp32_decision_edges(antq_lib, oracle, dev, name):
    """+/-16 ulps around every midpoint of the grid (the exact ones are ties: the later scan index), every grid value, +/-fastlim
    of the in-kernel grid analysis, +/-65536 and the scan's horizon, and every exponent / denormals / zeros / Inf / NaN."""
    g = oc.grid32(name)
    _check_nearest(antq_lib, oracle, dev, oc.nearest_case(g)["x"], g, (name,))


@pytest.mark.parametrize("name", oc.FORM_GRIDS)
def test_nearest_fp32_lengths(antq_lib, oracle, dev, name):
    """The workgroup spans of 2048 (k_nearest_fast) and 1024 (k_nearest) elements with a partial last span"""
    g = oc.grid32(name)
    x = oc.nearest_case(g)["x"]
    for n in oc.LENGTHS:
        _check_nearest(antq_lib, oracle, dev, oc.take(x, n), g, (name,))


def test_nearest_refuses_1025_entries(antq_lib, dev):
    g = np.arange(1025, dtype=np.float32)
    x = np.zeros(8, np.float32)
    z = Out(8, "f32", dev)
    assert _nearest_rc(antq_lib, dev, _dev(x, dev), z, None, 8, _dev(g, dev), 1025, F32) == ERR_UNSUPPORTED
    assert (z.bits("m = 1025") == oc.POISON32).all()
    assert _nearest_rc(antq_lib, dev, _dev(x, dev), z, None, 8, _dev(g, dev), 1024, F32) == 0


@pytest.mark.parametrize("name", sorted(oc.nearest_grids()))
def test_nearest_float64_narrows_inside(antq_lib, oracle, dev, name):
    """float64 x and grid: the kernel narrows both to float (the grid holds values float cannot hold), scans, and widens the
    chosen float.  The doubles halfway between a float midpoint and its float neighbours (where (float)x changes) with one
    double ulp on either side, +/-8 double ulps around the midpoint, doubles beyond FLT_MAX, double denormals, zeros, NaN, Inf."""
    g = oc.nearest_grids()[name]
    x = oc.nearest_case_f64(g)["x"]
    _check_nearest(antq_lib, oracle, dev, x, g, (name, "f64"))
    if name in oc.FORM_GRIDS:
        for n in oc.LENGTHS:
            _check_nearest(antq_lib, oracle, dev, oc.take(x, n), g, (name, "f64"))


# ---------------------------------------------------------------------------------------------------------------------------
# 3: antq_nearest_plan, antq_nearest_hinted
# ---------------------------------------------------------------------------------------------------------------------------
def _plan_rc(antq_lib, dev, xt, z, idx, n, plan, dt, gcheck=None, m=0, stale=None, hinted=False):
    L, st = antq_lib.lib(), antq_lib._stream(dev)
    host, pd = ctypes.c_void_p(plan.host_addr), _vp(plan.dev(dev))
    if hinted:
        return L.antq_nearest_hinted(_vp(xt), _vp(z), _vp(idx), ctypes.c_size_t(n), _vp(gcheck), ctypes.c_int(m), host, pd, _vp(stale),
                                     ctypes.c_int(dt), st)
    return L.antq_nearest_plan(_vp(xt), _vp(z), _vp(idx), ctypes.c_size_t(n), host, pd, ctypes.c_int(dt), st)


def _want_plan(oracle, x, g, dtype_name):
    """(expected bit patterns, expected indices) of x (float32, or uint16 patterns) on grid g"""
    if dtype_name == "float32":
        z, j = _oracle_nearest(oracle, x, g)
        return z, j
    z, j = _oracle_nearest(oracle, oc.widen16(oracle, x, dtype_name), g)
    return oc.round16(oracle, z, dtype_name), j


def _check_plan(antq_lib, oracle, dev, x, g, plan, dtype_name, tag, device_grid=None, stale=None, want_stale=None):
    """x through antq_nearest_plan, or antq_nearest_hinted when device_grid is given (the oracle then scans THAT grid)"""
    import torch
    dt = F32 if dtype_name == "float32" else DT16[dtype_name]
    hinted = device_grid is not None
    zr, jr = _want_plan(oracle, x, device_grid if hinted else g, dtype_name)
    xt = _dev(x, dev)
    gt = _dev(device_grid, dev) if hinted else None
    for want_idx in (True, False):
        z = Out(x.size, "f32" if dt == F32 else "h16", dev)
        idx = Out(x.size, "idx", dev) if want_idx else None
        if stale is not None:
            stale.zero_()
        rc = _plan_rc(antq_lib, dev, xt, z, idx, x.size, plan, dt, gt, g.size, stale, hinted)
        assert rc == 0, (tag, rc)
        t = tag + (dtype_name, x.size, want_idx)
        _same(z.bits(t), zr, x, t)
        if want_idx:
            _same_idx(idx.bits(t), jr, x, t)
        if stale is not None:
            torch.cuda.synchronize()
            assert int(stale[0]) == want_stale, (t, "stale")


def _plan_of(antq_lib, key):
    g = oc.grid32(oc.PLAN_GRIDS[key])
    plan = antq_lib.plan_for(g)
    h = oc.plan_header(plan.host)
    assert oc.plan_class(h) == dict(small="small", big_linear="big", big="big", scan="scan")[key], (key, h["kind"], oc.tab_units(h))
    return g, plan, h


def _patterns(rng=None):
    p = np.arange(65536, dtype=np.uint16)
    return p if rng is None else rng.permutation(p)


def _mixed16(oracle, g, h, dtype_name):
    """vectors of eight 16-bit elements, seven inside the table's domain and one at or beyond fastlim, as patterns"""
    lim = np.float32(h["fastlim"] if h["fastlim"] > 0 else oc.HORIZON)
    if dtype_name == "float16":
        lim = np.float32(65504.0)            # (float16 has nothing beyond fastlim but Inf and NaN)
    return oc.round16(oracle, oc.mixed_vectors(g, lim, 8), dtype_name)


@pytest.mark.parametrize("key", sorted(oc.PLAN_GRIDS))
def test_nearest_plan_fp32_edges(antq_lib, oracle, dev, key):
    """The windows of antq_nearest's test plus every bucket edge of the plan's table and +/-fastlim of the plan; vectors with one
    element beyond fastlim among three inside it (the whole vector takes the scan); every vector count around the workgroup
    spans of 512 and 1024 vectors; a ragged n and a pointer 4 bytes off a vector refuse."""
    g, plan, h = _plan_of(antq_lib, key)
    case = oc.plan_case(g, h)
    x = case["x"]
    assert case["edges"].shape[0] == oc.bucket_edges(h).size
    _check_plan(antq_lib, oracle, dev, x, g, plan, "float32", (key,))
    body = x[case["n_mixed"]:]
    for nv in oc.VECTOR_COUNTS:
        _check_plan(antq_lib, oracle, dev, oc.take(body, 4 * nv), g, plan, "float32", (key, nv))
    z, idx = Out(64, "f32", dev), Out(64, "idx", dev)
    assert _plan_rc(antq_lib, dev, _dev(x[:64], dev), z, idx, 63, plan, F32) == ERR_UNSUPPORTED
    assert _plan_rc(antq_lib, dev, _dev(x[:64], dev, lead=1), z, idx, 64, plan, F32) == ERR_UNSUPPORTED
    assert _plan_rc(antq_lib, dev, _dev(x[:64], dev), Out(64, "f32", dev, lead=1), idx, 64, plan, F32) == ERR_UNSUPPORTED
    assert (z.bits("refused") == oc.POISON32).all() and (idx.bits("refused") == oc.POISON_IDX).all()


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float16"])
@pytest.mark.parametrize("key", sorted(oc.PLAN_GRIDS))
def test_nearest_plan_all_16bit_patterns(antq_lib, oracle, dev, key, dtype_name):
    """All 65 536 patterns in order and shuffled == the oracle on the widened value, rounded once; vectors of eight with one
    element beyond the table's domain; the vector counts; a ragged n refuses."""
    g, plan, h = _plan_of(antq_lib, key)
    shuffled = _patterns(np.random.default_rng(16))
    for x in (_patterns(), shuffled, _mixed16(oracle, g, h, dtype_name)):
        _check_plan(antq_lib, oracle, dev, x, g, plan, dtype_name, (key,))
    for nv in oc.VECTOR_COUNTS:
        _check_plan(antq_lib, oracle, dev, shuffled[:8 * nv], g, plan, dtype_name, (key, nv))
    z = Out(64, "h16", dev)
    assert _plan_rc(antq_lib, dev, _dev(shuffled[:64], dev), z, None, 60, plan, DT16[dtype_name]) == ERR_UNSUPPORTED
    assert _plan_rc(antq_lib, dev, _dev(shuffled[:64], dev, lead=2), z, None, 64, plan, DT16[dtype_name]) == ERR_UNSUPPORTED
    assert (z.bits("refused") == oc.POISON16).all()


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("key", sorted(oc.PLAN_GRIDS))
def test_nearest_hinted_follows_the_device_grid(antq_lib, oracle, dev, key, dtype_name):
    """With the device grid equal to the plan's the results are the oracle's and `stale` stays 0.  With one entry of the device
    grid one ulp off (position 0, m - 1, and 255 / 256 of the 509-entry book), 0.0 replaced by -0.0, or an entry replaced by
    NaN, the results are the oracle's ON THE DEVICE GRID and `stale` is 1 after a synchronise.  A grid of another length is
    an argument error."""
    import torch
    g, plan, h = _plan_of(antq_lib, key)
    if dtype_name == "float32":
        x = oc.plan_case(g, h)["x"]
    else:
        x = np.concatenate([_mixed16(oracle, g, h, dtype_name), _patterns(np.random.default_rng(17))])
        x = x[:x.size - x.size % 8]
    stale = torch.zeros(1, dtype=torch.int32).pin_memory()
    epl = 4 if dtype_name == "float32" else 8
    _check_plan(antq_lib, oracle, dev, x, g, plan, dtype_name, (key, "same"), device_grid=g, stale=stale, want_stale=0)
    for nv in oc.VECTOR_COUNTS:
        _check_plan(antq_lib, oracle, dev, x[:epl * nv], g, plan, dtype_name, (key, "same", nv), device_grid=g, stale=stale, want_stale=0)
    # windows around the altered entry and its neighbours first (inputs on which the two grids give different answers: the host
    # test asserts it for fp32), then all of x for the 509-entry book, 1025 vectors of it for the others
    rest = x if g.size > 256 else x[:epl * 1025]
    for tag, a in oc.altered_grids(g):
        front = oc.altered_front(g, a)
        if dtype_name != "float32":
            front = oc.round16(oracle, front, dtype_name)
        _check_plan(antq_lib, oracle, dev, np.concatenate([front, rest]), g, plan, dtype_name, (key, tag), device_grid=a, stale=stale,
                    want_stale=1)
    z = Out(64, "f32" if epl == 4 else "h16", dev)
    dt = F32 if epl == 4 else DT16[dtype_name]
    for other in (g[:-1], np.concatenate([g, g[:1]])):
        if other.size:
            assert _plan_rc(antq_lib, dev, _dev(x[:64], dev), z, None, 64, plan, dt, _dev(other, dev), other.size, stale, True) == ERR_ARG
    assert (z.bits("refused") != z.poison).sum() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4: antq_affine
# ---------------------------------------------------------------------------------------------------------------------------
def _affine_rc(antq_lib, dev, xt, out, q, rows, row_len, k, mn_t, mx_t, per_row):
    return antq_lib.lib().antq_affine(_vp(xt), _vp(out), _vp(q), ctypes.c_size_t(rows), ctypes.c_size_t(row_len), ctypes.c_int(k), _vp(mn_t),
                                      _vp(mx_t), ctypes.c_int(1 if per_row else 0), antq_lib._stream(dev))


def _check_affine(antq_lib, oracle, dev, x, k, xmin, xmax, per_row, tag, leads=(0, 1)):
    """x [rows, row_len]; aligned (the vector kernel where the row length allows it) and the same data 4 bytes off (the element
    kernel), with and without q"""
    rows, rl = x.shape
    with np.errstate(all="ignore"):
        ref, rq = oracle.affine(x if per_row else x.reshape(1, -1), k, xmin, xmax)
    # q is an integer only where the level is a number: x finite and the row's scale and zero point not NaN (a NaN min / max)
    par = np.float32([oc.affine_params(k, a, b) for a, b in zip(np.atleast_1d(xmin), np.atleast_1d(xmax))])
    finite = np.isfinite(x.reshape(-1)) & np.repeat(np.isfinite(par).all(1), rl if per_row else x.size)
    mn_t, mx_t = _dev(np.float32(xmin), dev), _dev(np.float32(xmax), dev)
    for lead in leads:
        xt = _dev(x, dev, lead)
        for want_q in (True, False):
            out = Out(x.size, "f32", dev, lead)
            q = Out(x.size, "q", dev, lead) if want_q else None
            rc = _affine_rc(antq_lib, dev, xt, out, q, rows, rl, k, mn_t, mx_t, per_row)
            t = tag + (k, rows, rl, per_row, lead, want_q)
            assert rc == 0, (t, rc)
            _same(out.bits(t), ref, x, t)
            if want_q:
                got = q.bits(t).view(np.int32)
                bad = np.flatnonzero((got != rq.reshape(-1)) & finite)
                assert bad.size == 0, (t, "q differs", bad[:6].tolist(), x.reshape(-1)[bad[:6]].tolist(), got[bad[:6]].tolist(),
                                       rq.reshape(-1)[bad[:6]].tolist())


def _affine_ranges(k):
    return np.concatenate([oc.random_ranges(np.random.default_rng(40 + k), 6), oc.special_ranges(k)])


@pytest.mark.parametrize("row_len", oc.AFFINE_ROW_LENS + (13,))
@pytest.mark.parametrize("k", oc.AFFINE_K)
def test_affine_round_half_even_ties_per_row(antq_lib, oracle, dev, k, row_len):
    """Every row its own (min, max): awkward random ranges, max == min, max < min, a range below the clamp of 1e-8, NaN min / max,
    min = 0 (num == 0), scales within a few ulps of 2^40 and 2^-40 (the domain of the 5-FMA division), a range of 3e38, and
    min = 1e20 (|num| > 2^60: true division).  +/-16 ulps around x = (zp + j + 0.5) / scale, the round-half-even ties, for
    every level and both clamps (k <= 8) or the 40 levels at each end plus 150 drawn ones.  Row length 13 is ragged: the
    element kernel.  out is bit-equal to the oracle everywhere, NaN rows included.  q is compared wherever x is finite and the
    row's range is not NaN; q of NaN / Inf is not compared: the reference has no integer output, and what the conversion of a
    NaN level to int32 gives is not defined (the oracle's C cast gives INT32_MIN on x86, the device's conversion 0)."""
    case = oc.affine_case(np.random.default_rng(4000 + 31 * k + row_len), k, _affine_ranges(k), row_len)
    _check_affine(antq_lib, oracle, dev, case["x"], k, case["xmin"], case["xmax"], True, ("rows",))


@pytest.mark.parametrize("k", oc.AFFINE_K)
def test_affine_per_tensor_and_vector_counts(antq_lib, oracle, dev, k):
    """One (min, max) for the tensor, for every range of the per-row test; 511, 512 and 513 vectors (the vector kernel's span is
    512), and the same element counts plus one (ragged: the element kernel)."""
    rng = np.random.default_rng(4400 + k)
    for i, (mn, mx) in enumerate(_affine_ranges(k)):
        case = oc.affine_case(rng, k, [(mn, mx)], 1028)
        x = case["x"]
        _check_affine(antq_lib, oracle, dev, x, k, [mn], [mx], False, ("tensor", i), leads=(0, 1) if i % 4 == 0 else (0,))
        if i < 2:
            flat = x.reshape(-1)
            for nv in (511, 512, 513):
                _check_affine(antq_lib, oracle, dev, np.resize(flat, 4 * nv).reshape(1, -1), k, [mn], [mx], False, ("tensor", i, nv), leads=(0,))
                _check_affine(antq_lib, oracle, dev, np.resize(flat, 4 * nv + 1).reshape(1, -1), k, [mn], [mx], False, ("tensor", i, nv), leads=(0,))
            # the same counts per row: rows of 4 elements, a row of its own per vector
            for nv in (511, 513):
                r = np.float32([[mn, mx]]).repeat(nv, 0)
                _check_affine(antq_lib, oracle, dev, np.resize(flat, 4 * nv).reshape(nv, 4), k, r[:, 0], r[:, 1], True, ("rows of 4", i, nv), leads=(0,))


def test_affine_refuses_k_0_and_25(antq_lib, dev):
    x = _dev(np.zeros(16, np.float32), dev)
    out, q = Out(16, "f32", dev), Out(16, "q", dev)
    mn, mx = _dev(np.float32([0.0]), dev), _dev(np.float32([1.0]), dev)
    for k in (0, 25, -1):
        assert _affine_rc(antq_lib, dev, x, out, q, 1, 16, k, mn, mx, False) == ERR_ARG, k
    assert (out.bits("refused") == oc.POISON32).all() and (q.bits("refused") == oc.POISON_Q).all()
    assert _affine_rc(antq_lib, dev, x, out, q, 1, 16, 24, mn, mx, False) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 5: antq_fakequant_f64
# ---------------------------------------------------------------------------------------------------------------------------
def _check_f64(antq_lib, oracle, dev, bk, x, alpha, per_row, ovp, tag):
    _, g, gmax, nn, _ = bk
    plan = antq_lib.plan_for(g)
    rows, rl = x.shape
    alpha = np.atleast_1d(np.asarray(alpha, np.float64))
    ref = oc.f64_forward_ref(oracle, x, alpha, g, gmax, ovp, per_row)
    out = Out(x.size, "f64", dev)
    xt, at = _dev(x, dev), _dev(alpha, dev)
    rc = antq_lib.lib().antq_fakequant_f64(_vp(xt), _vp(out), ctypes.c_size_t(rows), ctypes.c_size_t(rl), _vp(at),
                                           ctypes.c_int(1 if per_row else 0), ctypes.c_double(float(gmax)), ctypes.c_void_p(plan.host_addr),
                                           _vp(plan.dev(dev)), ctypes.c_uint(antq_lib.FLAG_OVP if ovp else 0), antq_lib._stream(dev))
    t = tag + (bk[0], rows, rl, per_row, ovp)
    assert rc == 0, (t, rc)
    _same(out.bits(t), ref, x, t)


@pytest.mark.parametrize("name", oc.F64_BOOKS)
def test_float64_forward_decision_edges(antq_lib, oracle, dev, name):
    """Per scale (doubles that float cannot hold; 0, a negative one and NaN): x = d * s for the doubles d at which (float)d
    changes next to every threshold of the book and next to +/-fastlim of the plan, +/-8 double ulps of x around each, and the
    float64 specials -- per row, each row again as a tensor with one scale, and as (1, 4097).  OliVe: with and without the pair
    rule, pair_case's octets around the normal | outlier boundary, and the odd-sized (7, 33) and (33, 1) whose last element
    pairs with element 0: once an outlier there, once a normal value there and an outlier at the end."""
    bk = oc.f64_book(name)
    _, g, gmax, nn, ovp = bk
    h = oc.plan_header(antq_lib.plan_for(g).host)
    assert (oc.plan_class(h) == "scan") == (name == "scan_list")
    case = oc.f64_case(bk, h, oc.F64_ALPHAS_8BIT if g.size > 64 else oc.F64_ALPHAS)
    x, alpha = case["x"], case["alpha"]
    for pair_rule in ((False, True) if ovp else (False,)):
        _check_f64(antq_lib, oracle, dev, bk, x, alpha, True, pair_rule, ("rows",))
        for i in range(alpha.size):
            _check_f64(antq_lib, oracle, dev, bk, x[i:i + 1], alpha[i:i + 1], False, pair_rule, ("tensor", i))
        _check_f64(antq_lib, oracle, dev, bk, x[:1, :4097], alpha[:1], False, pair_rule, ("4097",))
        _check_f64(antq_lib, oracle, dev, bk, x[:, :x.shape[1] // 2 * 2 - 1], alpha, True, pair_rule, ("odd rows",))
    if not ovp:
        return
    pc = oc.f64_pair_case(bk)
    _check_f64(antq_lib, oracle, dev, bk, pc["x"], pc["alpha"], True, True, ("pairs",))
    _check_f64(antq_lib, oracle, dev, bk, pc["x"][:8], pc["alpha"][:1], False, True, ("pairs",))
    for shape, per_row in ((oc.ODD_SHAPES[0], True), (oc.ODD_SHAPES[1], False), (oc.ODD_SHAPES[1], True), (oc.ODD_SHAPES[0], False)):
        for first in (True, False):
            c = oc.f64_odd_case(bk, shape, first, per_row)
            _check_f64(antq_lib, oracle, dev, bk, c["x"], c["alpha"], per_row, True, ("odd", first))


def test_float64_forward_grid_stride_loop(antq_lib, oracle, dev):
    """One per-tensor OliVe tensor of 2 * 256 * 8192 * 2 + 513 elements: more pairs than the launch's cap of 8192 workgroups
    holds at once, so the grid-stride loop runs more than once, the last pass partial, the last element unpaired."""
    bk = oc.f64_book("olive_flint")
    _, g, gmax, nn, ovp = bk
    h = oc.plan_header(antq_lib.plan_for(g).host)
    alpha = oc.F64_ALPHAS[:1]
    row = oc.f64_case(bk, h, alpha)["x"][0]
    rng = np.random.default_rng(8192)
    d = rng.standard_normal(oc.BIG_F64) * 12
    d[rng.random(d.size) < 0.04] *= 5
    x = d * (alpha[0] / gmax)
    at = rng.integers(0, (x.size - row.size) // 2) * 2 + 1            # (odd: the windows' pairs are not the builder's own)
    x[at:at + row.size] = row
    x[0], x[-1] = 48.0 * alpha[0] / gmax, 3.0 * alpha[0] / gmax       # the last element is element 0's victim
    _check_f64(antq_lib, oracle, dev, bk, x.reshape(1, -1), alpha, False, True, ("big",))
