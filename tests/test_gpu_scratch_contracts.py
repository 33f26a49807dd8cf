"""The memory the calibration and reduction entry points use BESIDE their values: caller-owned workspaces, ticket blocks and
output buffers, held to what include/antq.h says about them ("contents are scratch (no initialisation)", "need not be
initialised", a stated size).

Every call goes through the C ABI on raw pointers (antq_lib.lib()), so the test owns every byte:
  * a Slab is GUARD + nbytes + GUARD bytes; the guards hold 0xC3 and must be byte-identical after the call;
  * a workspace is filled with 0x00 (the baseline), 0xFF (NaN as float / double, 2^32 - 1 as a counter or flag word), 0x7F (a
    huge finite double, a large count) or left exactly as calls of OTHER paths left it ("leftover": a whole-tensor moment sum,
    then a histogram search whose pair list overflowed -- its flag word set -- and the direct kernels behind it);
  * every output sits in a slab of its own, filled with 0xFF;
  * per case: the result bits under every pattern equal the baseline's, all guards are intact, the inputs are bit-identical,
    and the BASELINE is held to a yardstick that is no kernel of this library -- calib_check.exact_sse with the bars of
    calib_check for the searches (by path), exact integer sums for moments / alpha gradient, the numpy maximum and planted
    maxima for abs-max -- so that two equally wrong runs do not pass.
The cases and their premises: scratch_cases.py / test_scratch_cases_host.py.  The candidate-list split of the direct kernels
(knob 12) is forced in ONE case, "direct fp32 clamp binds": without it the clamp of the workgroup count to the workspace's
partial slots binds from ~7e8 element x candidate evaluations on, which the CPU yardstick cannot follow in a test's time.
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import calib_check
import scratch_cases as sc
from calib_check import exact_three_sigma
from test_gpu_reductions_exact import SIGMA_ULP, _int_data
from test_gpu_search_exact import _ant, _hold, _olive, _yard

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

vp, sz, ci, cf, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint
KNOB_DEFAULTS = {12: 0, 14: 1, 17: 0, 18: 0, 19: 1, 20: 1, 21: 1}


class Slab:
    """nbytes of device memory between two guards of GUARD bytes (scratch_cases.slab_layout); `pattern`: a byte, or None to
    leave the inner region to the caller"""

    def __init__(self, nbytes, pattern, dev):
        self.n = int(nbytes)
        assert self.n > 0
        self.raw = torch.empty(sc.GUARD + self.n + sc.GUARD, dtype=torch.uint8, device=dev)
        off, total = sc.slab_layout(self.raw.data_ptr(), self.n)
        assert total == self.raw.numel()
        self.raw.fill_(sc.GUARD_BYTE)
        self.inner = self.raw[off:off + self.n]
        if pattern is not None:
            self.inner.fill_(int(pattern))
        self.ptr = self.inner.data_ptr()
        assert self.ptr % 256 == 0

    def put(self, t):
        """copy the bytes of tensor t to the start of the inner region"""
        b = t.contiguous().view(-1).view(torch.uint8)
        self.inner[:b.numel()].copy_(b)
        return self

    def guards_ok(self):
        lo, hi = self.raw[:sc.GUARD], self.raw[sc.GUARD + self.n:]
        return hi.numel() == sc.GUARD and bool((lo == sc.GUARD_BYTE).all().item()) and bool((hi == sc.GUARD_BYTE).all().item())

    def bytes(self):
        return self.inner.cpu().numpy().copy()

    def as_np(self, dtype):
        return self.bytes().view(dtype)


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


class Env:
    """The entry points on raw pointers, the codebooks, and the donors of the "leftover" pattern"""

    def __init__(self, L, oracle, dev):
        from ant_quantization_amd import grids
        self.L, self.c, self.oracle, self.dev, self.grids = L, L.lib(), oracle, dev, grids
        self.st = L._stream_int(dev)
        self.yard_cache = {}
        self.alone_cache = {}
        over, xm = sc.flag_tensors()["overflow"]
        self.donor_over = (torch.from_numpy(over).to(dev).bfloat16(), torch.tensor([xm], dtype=torch.float32, device=dev))
        self.donor_sum = torch.from_numpy(sc.gauss(300001, 77)).to(dev)
        self.donor_out = torch.empty(4096, dtype=torch.float64, device=dev)
        self.flag_rt = torch.from_numpy(sc.FLAG_RATIOS).to(dev)

    # ---- codebooks: (cbs [(grid, gmax)], plans, gmaxs)
    def books(self, family):
        if family == "olive":
            return _olive(self.L, self.grids)
        return _ant(self.L, self.grids, types=sc.ANT_TYPES[family])

    def calib_books(self, ntypes):
        return _ant(self.L, self.grids, types=sc.CALIB_TYPES[:ntypes])

    @contextlib.contextmanager
    def knobs(self, settings):
        try:
            for k, v in settings.items():
                assert self.c.antq_debug_set(ci(k), ci(v)) == 0
            yield
        finally:
            for k in settings:
                self.c.antq_debug_set(ci(k), ci(KNOB_DEFAULTS[k]))

    def sync(self):
        torch.cuda.synchronize(self.dev)

    # ---- entry points
    def search_sse(self, x, rows, K, xm, per_row, rt, plan, gmax, ovp, code, sse_ptr, ws_ptr):
        return self.c.antq_search_sse(vp(x.data_ptr()), sz(rows), sz(K), vp(xm.data_ptr()), ci(per_row), vp(rt.data_ptr()), ci(rt.numel()),
                                      cf(gmax), plan.host_ptr(), vp(plan.dev(self.dev).data_ptr()), cu(sc.FLAG_OVP if ovp else 0), ci(code),
                                      vp(sse_ptr), vp(ws_ptr), vp(self.st))

    def plan_arrays(self, plans, gmaxs):
        nt = len(plans)
        return ((ctypes.c_void_p * nt)(*[p.host_addr for p in plans]), (ctypes.c_void_p * nt)(*[p.dev(self.dev).data_ptr() for p in plans]),
                (ctypes.c_float * nt)(*[float(g) for g in gmaxs]))

    def search_multi(self, x, rows, K, xm, per_row, rt, plans, gmaxs, ovp, code, sse_ptr, ws_ptr):
        ph, pd, gm = self.plan_arrays(plans, gmaxs)
        return self.c.antq_search_sse_multi(vp(x.data_ptr()), sz(rows), sz(K), vp(xm.data_ptr()), ci(per_row), vp(rt.data_ptr()),
                                            ci(rt.numel()), ci(len(plans)), gm, ph, pd, cu(sc.FLAG_OVP if ovp else 0), ci(code), vp(sse_ptr),
                                            vp(ws_ptr), vp(self.st))

    def moments(self, x, n, code, out_ptr, ws_ptr):
        return self.c.antq_moments(vp(x.data_ptr()), sz(1), sz(n), ci(0), ci(code), vp(out_ptr), vp(ws_ptr), vp(self.st))

    def alpha_grad(self, x, o, g, n, code, out_ptr, ws_ptr):
        return self.c.antq_alpha_grad(vp(x.data_ptr()), vp(o.data_ptr()), vp(g.data_ptr()), sz(1), sz(n), ci(0), vp(out_ptr), vp(ws_ptr),
                                      ci(code), vp(self.st))

    def calibrate(self, x, rows, K, per_row, code, mode, xmax_ptr, rng, plans, gmaxs, alpha_ptr, score_ptr, type_ptr, ws_ptr, ws_bytes, ovp=False):
        ph, pd, gm = self.plan_arrays(plans, gmaxs)
        return self.c.antq_calibrate(vp(x.data_ptr()), sz(rows), sz(K), ci(per_row), ci(code), ci(mode), vp(xmax_ptr), ci(rng[0]), ci(rng[1]),
                                     ci(rng[2]), ci(len(plans)), gm, ph, pd, cu(sc.FLAG_OVP if ovp else 0), vp(alpha_ptr), vp(score_ptr),
                                     vp(type_ptr), vp(ws_ptr), sz(ws_bytes), vp(self.st))

    # ---- the "leftover" pattern: what calls of other paths leave in a search workspace (nothing cleared afterwards)
    def dirty(self, ws_ptr):
        assert self.moments(self.donor_sum, self.donor_sum.numel(), 0, self.donor_out.data_ptr(), ws_ptr) == 0
        _, plans, gms = self.books("olive")
        x, xm = self.donor_over
        with self.knobs({14: 2}):
            assert self.search_sse(x, 1, x.numel(), xm, 0, self.flag_rt, plans[0], gms[0], True, 1, self.donor_out.data_ptr() + 64, ws_ptr) == 0

    def workspace(self, nbytes, pattern):
        """a workspace slab under `pattern`; "leftover": zero-filled, then the donors run on it"""
        ws = Slab(nbytes, 0x00 if pattern == "leftover" else pattern, self.dev)
        if pattern == "leftover":
            self.dirty(ws.ptr)
        return ws


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def env(antq_lib, oracle, dev):
    e = Env(antq_lib, oracle, dev)
    assert e.c.antq_search_workspace_bytes() == sc.SEARCH_WS_BYTES
    return e


@contextlib.contextmanager
def _timed(what):
    """(pytest -s: what each step of a case costs, the yardstick apart from the GPU side)"""
    t0 = time.perf_counter()
    yield
    print("SCRATCH CONTRACTS | %.2f s | %s" % (time.perf_counter() - t0, what), flush=True)


def _to_dev(env, x_np, dtype):
    return torch.from_numpy(np.ascontiguousarray(x_np)).to(env.dev).to(getattr(torch, dtype))


# ---------------------------------------------------------------------------------------------------------------------
# one-scale searches
# ---------------------------------------------------------------------------------------------------------------------
BARS = {"sorted": (0, calib_check.EXACT_RTOL), "sweep": (0, calib_check.EXACT_RTOL), "hist": (1, calib_check.HIST_RTOL),
        "direct": (1, calib_check.DIRECT_RTOL), "direct olive": (1, calib_check.DIRECT_RTOL_OLIVE)}
#        path -> (which sum of exact_sse: 0 `exact`, 1 `terms32`; the bar calib_check defines for the path)


def _search_run(env, c, x, xm, rt, plans, gms, pattern, knobs, multi, ws=None):
    """One search of case c under `knobs` on a workspace under `pattern` (or on the slab `ws` as it is): [ntypes, ncand, 1]
    float64.  Single-codebook calls run one after the other on the SAME workspace.  Asserts guards and inputs."""
    rows, K, per_row = sc.case_rows(c)
    nt, ncand, code = len(plans), rt.numel(), sc.DTYPE_CODE[c["dtype"]]
    ws = env.workspace(sc.SEARCH_WS_BYTES, pattern) if ws is None else ws
    out = Slab(nt * ncand * 8, sc.OUTPUT_FILL, env.dev)
    snap = (x.clone(), xm.clone(), rt.clone())
    with env.knobs(knobs):
        if multi:
            rc = env.search_multi(x, rows, K, xm, per_row, rt, plans, gms, c["ovp"], code, out.ptr, ws.ptr)
            assert rc == 0, (c["name"], "antq_search_sse_multi", rc)
        else:
            for t in range(nt):
                rc = env.search_sse(x, rows, K, xm, per_row, rt, plans[t], gms[t], c["ovp"], code, out.ptr + t * ncand * 8, ws.ptr)
                assert rc == 0, (c["name"], "antq_search_sse", rc)
    env.sync()
    assert ws.guards_ok(), (c["name"], pattern, "the workspace's guards")
    assert out.guards_ok(), (c["name"], pattern, "the guards of sse")
    assert _same_bytes(x, snap[0]) and _same_bytes(xm, snap[1]) and _same_bytes(rt, snap[2]), (c["name"], pattern, "an input changed")
    return out.as_np(np.float64).reshape(nt, ncand, 1)


def _search_inputs(env, c, family=None):
    x_np, xm_np = sc.case_data(c)
    x = _to_dev(env, x_np, c["dtype"])
    xm = torch.tensor([xm_np], dtype=torch.float32, device=env.dev)
    rt = torch.from_numpy(c["ratios"]).to(env.dev)
    return (x, xm, rt) + tuple(env.books(c["family"] if family is None else family))


def _search_yard(env, c, x, xm, cbs, key):
    """[2, ntypes, ncand, 1]: exact_sse's two sums for every codebook, computed once per (case, codebooks)"""
    if key not in env.yard_cache:
        with _timed("yardstick of " + str(key)):
            env.yard_cache[key] = _yard(env.oracle, x.reshape(1, -1), xm, c["ratios"], cbs, c["ovp"], False, slice(None)).transpose(1, 0, 2, 3)
    return env.yard_cache[key]


def _search_contract(env, c, family, multi):
    x, xm, rt, cbs, plans, gms = _search_inputs(env, c, family)
    label = "%s%s" % (c["name"], " multi %d" % len(plans) if multi else "")
    with _timed("search " + label):
        base = _search_run(env, c, x, xm, rt, plans, gms, 0x00, c["knobs"], multi)
        for p in sc.PATTERNS[1:]:
            got = _search_run(env, c, x, xm, rt, plans, gms, p, c["knobs"], multi)
            assert np.array_equal(got.view(np.uint64), base.view(np.uint64)), (label, "workspace pattern %r changes the result" % (p,),
                                                                               np.argwhere(got.view(np.uint64) != base.view(np.uint64))[:4].tolist())
        if c["path"] != "direct":           # the intended path ran: its bits differ from the direct kernels'
            d = _search_run(env, c, x, xm, rt, plans, gms, 0x00, sc.DIRECT_KNOBS, multi)
            assert not np.array_equal(d, base), (label, "the %s search did not run: the comparison would prove nothing" % c["path"])
    which, bar = BARS["direct olive" if (c["path"] == "direct" and c["family"] == "olive") else c["path"]]
    yard = _search_yard(env, c, x, xm, cbs, (c["name"], len(plans), family or c["family"]))
    _hold("scratch contracts, " + c["path"], label, c["dtype"], base, yard[which], bar)
    return base


@pytest.mark.parametrize("name", [c["name"] for c in sc.SEARCH_CASES])
def test_one_scale_search_workspace_is_scratch(env, name):
    _search_contract(env, sc.search_case(name), None, False)


@pytest.mark.parametrize("name,nt", sc.MULTI_CASES)
def test_one_scale_multi_search_workspace_is_scratch(env, name, nt):
    """antq_search_sse_multi with 2 and 4 codebooks on the one-scale paths: the call must take the launch (rc 0)"""
    _search_contract(env, sc.search_case(name), nt, True)


def test_histogram_flag_word_is_not_trusted_across_calls(env):
    """flags[] of the histogram search decides ON THE DEVICE whether the direct kernels behind it run.  A tensor whose pair
    list overflows (the flag set, the direct kernels answer) and a clean one (the histogram answers), back to back on ONE
    workspace in both orders and again: every result equals the same call on a fresh zeroed workspace.  The flag word is read
    back after each call to show that the device did decide differently for the two."""
    t = sc.flag_tensors()
    c = dict(name="flag", dtype="bfloat16", n=sc.FLAG_N, form="flat", ovp=True, ratios=sc.FLAG_RATIOS, path="hist", family="olive")
    cbs, plans, gms = env.books("olive")
    rt = env.flag_rt
    hist, direct = {19: 1, 20: 1, 14: 2}, {19: 1, 20: 1, 14: 0}
    x = {k: _to_dev(env, v[0], "bfloat16") for k, v in t.items()}
    xm = {k: torch.tensor([v[1]], dtype=torch.float32, device=env.dev) for k, v in t.items()}
    with _timed("histogram flag leftovers"):
        fresh = {k: _search_run(env, c, x[k], xm[k], rt, plans, gms, 0x00, hist, False) for k in x}
        off = {k: _search_run(env, c, x[k], xm[k], rt, plans, gms, 0x00, direct, False) for k in x}
        assert np.array_equal(fresh["overflow"].view(np.uint64), off["overflow"].view(np.uint64)), "the overflowing tensor was not answered by the direct kernels"
        assert not np.array_equal(fresh["clean"], off["clean"]), "the histogram search did not answer for the clean tensor"
        for order in (("overflow", "clean", "overflow", "clean"), ("clean", "overflow", "clean", "overflow")):
            for first in (0x00, 0xFF):
                ws = env.workspace(sc.SEARCH_WS_BYTES, first)
                for i, k in enumerate(order):
                    got = _search_run(env, c, x[k], xm[k], rt, plans, gms, None, hist, False, ws=ws)
                    assert np.array_equal(got.view(np.uint64), fresh[k].view(np.uint64)), (order, "workspace first %#x" % first, "call %d (%s)" % (i, k))
                    flag = int(ws.inner[sc.HIST_FLAGS_OFF:sc.HIST_FLAGS_OFF + 4].view(torch.int32).item())
                    assert (flag & 1) == (1 if k == "overflow" else 0), (order, i, k, "flag word %#x" % flag)
    for k in x:
        yard = _search_yard(env, c, x[k], xm[k], cbs, ("flag " + k, 2, "olive"))
        bar = calib_check.DIRECT_RTOL_OLIVE if k == "overflow" else calib_check.HIST_RTOL
        _hold("scratch contracts, flag " + k, "flag " + k, "bfloat16", fresh[k], yard[1], bar)


# ---------------------------------------------------------------------------------------------------------------------
# reductions with the shared workspace
# ---------------------------------------------------------------------------------------------------------------------
def _sum_run(env, op, ts, n, code, pattern, ws=None, sync=True):
    ws = env.workspace(sc.SEARCH_WS_BYTES, pattern) if ws is None else ws
    out = Slab(16 if op == "moments" else 8, sc.OUTPUT_FILL, env.dev)
    if op == "moments":
        rc = env.moments(ts[0], n, code, out.ptr, ws.ptr)
    else:
        rc = env.alpha_grad(ts[0], ts[1], ts[2], n, code, out.ptr, ws.ptr)
    assert rc == 0, (op, rc)
    if not sync:
        return out
    env.sync()
    assert ws.guards_ok() and out.guards_ok(), (op, n, pattern, "guards")
    return out.as_np(np.float64)


def _sum_want(op, xi, oi, gi):
    return [float(xi.sum()), float((xi * xi).sum())] if op == "moments" else [float((gi * (oi - xi)).sum())]


@pytest.mark.parametrize("op", ["moments", "alpha_grad"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_whole_tensor_sums_do_not_trust_the_workspace(env, op, dtype):
    """antq_moments / antq_alpha_grad with per_row = 0: one workgroup, and more workgroups than the 1024 partials the launcher
    caps at; integer data, so the sums must equal the int64 sums bit for bit under every workspace pattern"""
    code = sc.DTYPE_CODE[dtype]
    for n in sc.sum_sizes(op, dtype):
        (x, o, g), (xi, oi, gi) = _int_data(n, n + 17, dtype, env.dev)
        snap = [t.clone() for t in (x, o, g)]
        want = _sum_want(op, xi, oi, gi)
        with _timed("%s %s n=%d" % (op, dtype, n)):
            for p in sc.PATTERNS:
                got = _sum_run(env, op, (x, o, g), n, code, p)
                assert got.tolist() == want, (op, dtype, n, "workspace pattern %r" % (p,), got.tolist(), want)
        assert all(_same_bytes(a, b) for a, b in zip((x, o, g), snap)), (op, dtype, n, "an input changed")


def test_chain_on_one_workspace_without_synchronisation(env):
    """What _lib._workspace does in production: calls of different kinds share one stream's workspace.  Histogram search,
    antq_alpha_grad, antq_moments, direct search, sorted search enqueued on ONE workspace with nothing in between -- no
    synchronisation, nothing cleared; every link equals its stand-alone result (fresh zeroed workspace), which is itself held
    to its yardstick."""
    links = []
    for name in ("hist bf16 2^19", "direct fp32 8192", "sorted fp32 4096 forced"):
        c = sc.search_case(name)
        links.append(("search", c, _search_inputs(env, c)))
    sums = []
    for op, dtype in (("alpha_grad", "float32"), ("moments", "float16")):
        n = sc.sum_sizes(op, dtype)[1]
        ts, ints = _int_data(n, n + 17, dtype, env.dev)
        sums.append((op, dtype, n, ts, _sum_want(op, *ints)))
    order = [links[0], sums[0], sums[1], links[1], links[2]]
    with _timed("chain on one workspace"):
        alone = []
        for item in order:
            if item[0] == "search":
                _, c, (x, xm, rt, cbs, plans, gms) = item
                r = _search_run(env, c, x, xm, rt, plans, gms, 0x00, c["knobs"], False)
                which, bar = BARS[c["path"]]
                _hold("scratch contracts, chain", c["name"], c["dtype"], r, _search_yard(env, c, x, xm, cbs, (c["name"], len(plans), c["family"]))[which], bar)
                alone.append(r)
            else:
                op, dtype, n, ts, want = item
                r = _sum_run(env, op, ts, n, sc.DTYPE_CODE[dtype], 0x00)
                assert r.tolist() == want, (op, dtype, n, r.tolist(), want)
                alone.append(r)
        for first in (0x00, 0xFF, "leftover"):
            for rotate in (0, 2):
                seq = order[rotate:] + order[:rotate]
                want = alone[rotate:] + alone[:rotate]
                ws = env.workspace(sc.SEARCH_WS_BYTES, first)
                outs = []
                for item in seq:                                   # enqueue everything, look at nothing
                    if item[0] == "search":
                        _, c, (x, xm, rt, cbs, plans, gms) = item
                        rows, K, per_row = sc.case_rows(c)
                        out = Slab(len(plans) * rt.numel() * 8, sc.OUTPUT_FILL, env.dev)
                        with env.knobs(c["knobs"]):
                            for t in range(len(plans)):
                                assert env.search_sse(x, rows, K, xm, per_row, rt, plans[t], gms[t], c["ovp"], sc.DTYPE_CODE[c["dtype"]],
                                                      out.ptr + t * rt.numel() * 8, ws.ptr) == 0
                        outs.append(out)
                    else:
                        op, dtype, n, ts, _ = item
                        outs.append(_sum_run(env, op, ts, n, sc.DTYPE_CODE[dtype], None, ws=ws, sync=False))
                env.sync()
                assert ws.guards_ok(), (first, rotate)
                for i, (out, w) in enumerate(zip(outs, want)):
                    assert out.guards_ok(), (first, rotate, i)
                    got = out.as_np(np.float64).reshape(w.shape)
                    assert np.array_equal(got.view(np.uint64), w.view(np.uint64)), ("workspace first %r" % (first,), "rotation %d" % rotate,
                                                                                    "link %d (%s)" % (i, seq[i][1] if seq[i][0] != "search" else seq[i][1]["name"]))


# ---------------------------------------------------------------------------------------------------------------------
# abs-max: the outputs "need not be initialised"; antq_absmax_into honours the initial value
# ---------------------------------------------------------------------------------------------------------------------
INF_BITS, NAN_BITS = 0x7F800000, 0x7FC00000


def _planted(env, dtype, rows, K, pos):
    """values in [-1, 1] with +-2 planted at the flat positions `pos`: (device tensor, float32 image on the host)"""
    host = (torch.rand(rows * K, generator=torch.Generator().manual_seed(rows * 1000 + K)) * 2 - 1).to(getattr(torch, dtype))
    for i, p in enumerate(pos):
        host[p] = 2.0 if i % 2 == 0 else -2.0
    return host.to(env.dev), host.float().numpy().reshape(rows, K)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_absmax_outputs_need_no_initialisation(env, dtype):
    code = sc.DTYPE_CODE[dtype]
    with _timed("absmax " + dtype):
        for rows, K, per_row, pos in ((1, 5003, 0, [4001]), (3, 1001, 0, []), (3, 260, 1, [260 + 77]), (5, 1024, 1, [3 * 1024 + 1023]),
                                      (1, 300000, 0, [299999])):
            x, img = _planted(env, dtype, rows, K, pos)
            snap = x.clone()
            want = np.abs(img).max(axis=1) if per_row else np.abs(img).max(keepdims=True).reshape(1)
            if pos:
                assert want[pos[0] // K if per_row else 0] == 2.0
            for fill in (0xFF, INF_BITS):
                out = Slab(4 * want.size, None, env.dev)
                out.inner.view(torch.int32).fill_(-1 if fill == 0xFF else fill)
                assert env.c.antq_absmax(vp(x.data_ptr()), vp(out.ptr), sz(rows), sz(K), ci(per_row), ci(code), vp(env.st)) == 0
                env.sync()
                assert out.guards_ok() and _same_bytes(x, snap), (dtype, rows, K, per_row)
                got = out.as_np(np.float32)
                assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), (dtype, rows, K, per_row, "amax before %#x" % fill, got, want)
        # antq_absmax_into: max(initial, data) -- 0 gives the data's maximum, a value above it stays, a NaN stays (NaN wins)
        x, img = _planted(env, dtype, 1, 70001, [69999])
        snap = x.clone()
        for init, want in ((0.0, 2.0), (3.0, 3.0), (1.5, 2.0), (float("nan"), float("nan")), (float("inf"), float("inf"))):
            out = Slab(4, None, env.dev)
            out.inner.view(torch.float32).fill_(init)
            assert env.c.antq_absmax_into(vp(x.data_ptr()), vp(out.ptr), sz(x.numel()), ci(code), vp(env.st)) == 0
            env.sync()
            assert out.guards_ok() and _same_bytes(x, snap)
            got = float(out.as_np(np.float32)[0])
            assert (np.isnan(got) and np.isnan(want)) or got == want, (dtype, "initial %r" % init, got, want)
        assert float(np.abs(img).max()) == 2.0


# ---------------------------------------------------------------------------------------------------------------------
# the ticket block of the one-launch reductions
# ---------------------------------------------------------------------------------------------------------------------
TK_UNTOUCHED = [(sc.TK_COUNTER_BYTES, sc.TK_PARTIAL_OFF), (sc.TK_PARTIAL_OFF + 1024 * 16, sc.TK_GROUP_OFF),
                (sc.TK_GROUP_OFF + 64 * 16, sc.REDUCE_WS_BYTES)]        # bytes of the block no call may write


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_ticket_block_counters_zero_again_partials_are_scratch(env, dtype):
    """antq_absmax_t / antq_alpha_grad_t at n = 1, one workgroup, and the workgroup / group caps (knobs 18 / 17): with the
    counters zero and everything behind them 0xFF the results are the exact ones; after EVERY call the first
    TK_COUNTER_BYTES bytes -- the bytes include/antq.h promises -- are zero, and the bytes outside the counters and the two
    partial regions still hold what they held.  (The partial regions themselves keep the last call's partials: scratch.)"""
    code = sc.DTYPE_CODE[dtype]
    nmax = sc.TICKET_SIZES[-1]
    (x, o, g), (xi, oi, gi) = _int_data(nmax, 91, dtype, env.dev)
    snap = [t.clone() for t in (x, o, g)]
    term = gi * (oi - xi)
    partials_nonzero = 0
    with _timed("ticket block " + dtype):
        for setting in sc.TICKET_SETTINGS:
            knobs = {} if setting is None else {18: setting[0], 17: setting[1]}
            for n in sc.TICKET_SIZES:
                want_m, want_s = float(np.abs(xi[:n]).max()), float(term[:n].sum())
                for fill in (0x00, 0xFF):
                    blk = Slab(sc.REDUCE_WS_BYTES, 0x00, env.dev)
                    blk.inner[sc.TK_COUNTER_BYTES:].fill_(fill)
                    am, gs = Slab(4, sc.OUTPUT_FILL, env.dev), Slab(8, sc.OUTPUT_FILL, env.dev)
                    for rep in range(2):                            # twice on the same block: the second call meets the first's leavings
                        with env.knobs(knobs):
                            assert env.c.antq_absmax_t(vp(x.data_ptr()), vp(am.ptr), sz(n), ci(code), vp(blk.ptr), vp(env.st)) == 0
                        env.sync()
                        b = blk.bytes()
                        assert not b[:sc.TK_COUNTER_BYTES].any(), (dtype, setting, n, "counters after antq_absmax_t", np.flatnonzero(b[:sc.TK_COUNTER_BYTES])[:4])
                        with env.knobs(knobs):
                            assert env.c.antq_alpha_grad_t(vp(x.data_ptr()), vp(o.data_ptr()), vp(g.data_ptr()), sz(n), vp(gs.ptr), ci(code),
                                                           vp(blk.ptr), vp(env.st)) == 0
                        env.sync()
                        b = blk.bytes()
                        assert not b[:sc.TK_COUNTER_BYTES].any(), (dtype, setting, n, "counters after antq_alpha_grad_t", np.flatnonzero(b[:sc.TK_COUNTER_BYTES])[:4])
                        for lo, hi in TK_UNTOUCHED:
                            assert (b[lo:hi] == fill).all(), (dtype, setting, n, "bytes %d .. %d of the block were written" % (lo, hi))
                        assert blk.guards_ok() and am.guards_ok() and gs.guards_ok(), (dtype, setting, n)
                        got_m, got_s = float(am.as_np(np.float32)[0]), float(gs.as_np(np.float64)[0])
                        assert got_m == want_m and got_s == want_s, (dtype, setting, n, "block filled %#x" % fill, got_m, want_m, got_s, want_s)
                        if fill == 0x00:
                            partials_nonzero += int(b[sc.TK_PARTIAL_OFF:].any())
    assert all(_same_bytes(a, b) for a, b in zip((x, o, g), snap))
    # include/antq.h names the counters as the bytes left zeroed; that the partials stay behind is the reason it has to
    assert partials_nonzero > 0, "the partial regions were left zero too: the header may promise the whole block again"


# ---------------------------------------------------------------------------------------------------------------------
# antq_calibrate / antq_calibrate_batch on a workspace of EXACTLY the stated size
# ---------------------------------------------------------------------------------------------------------------------
class _CalibOut:
    def __init__(self, env, nt, na, given):
        self.alpha, self.score = Slab(nt * na * 4, sc.OUTPUT_FILL, env.dev), Slab(nt * 4, sc.OUTPUT_FILL, env.dev)
        self.type, self.xmax = Slab(4, sc.OUTPUT_FILL, env.dev), Slab(na * 4, sc.OUTPUT_FILL, env.dev)
        self.nt, self.na = nt, na
        if given is not None:
            self.xmax.put(given)
        self.slabs = (self.alpha, self.score, self.type, self.xmax)

    def guards_ok(self):
        return all(s.guards_ok() for s in self.slabs)

    def read(self):
        return dict(alpha=self.alpha.as_np(np.float32).reshape(self.nt, self.na), score=self.score.as_np(np.float32),
                    type=self.type.as_np(np.int32), xmax=self.xmax.as_np(np.float32))


def _calib_inputs(env, c):
    x_np, given = sc.calib_data(c)
    x = _to_dev(env, x_np, c["dtype"])
    return x, (None if given is None else torch.from_numpy(given).to(env.dev))


def _calib_workspace(env, c, nbytes, pattern):
    """`pattern`; "leftover": the donors of a search workspace on the search region, then the calibration of ANOTHER case on
    the whole workspace (its need is smaller or equal: every region is at least 256 bytes), nothing cleared"""
    ws = env.workspace(nbytes, pattern)
    if pattern == "leftover":
        small = sc.SMALLEST_CALIB
        d = sc.calib_case(small[1] if c["name"] == small[0] else small[0])
        assert sc.calibrate_workspace_bytes(d["rows"], d["per_row"], *d["rng"], d["ntypes"]) <= nbytes
        x, given = _calib_inputs(env, d)
        _, plans, gms = env.calib_books(d["ntypes"])
        out = _CalibOut(env, d["ntypes"], d["rows"] if d["per_row"] else 1, given)
        assert env.calibrate(x, d["rows"], d["row_len"], d["per_row"], sc.DTYPE_CODE[d["dtype"]], d["mode"], out.xmax.ptr, d["rng"], plans, gms,
                             out.alpha.ptr, out.score.ptr, out.type.ptr, ws.ptr, nbytes) == 0
        env.sync()
    return ws


def _calib_run(env, c, x, given, pattern):
    nt, na = c["ntypes"], (c["rows"] if c["per_row"] else 1)
    nbytes = sc.calibrate_workspace_bytes(c["rows"], c["per_row"], *c["rng"], nt)
    assert nbytes == env.c.antq_calibrate_workspace_bytes(sz(c["rows"]), ci(c["per_row"]), ci(c["rng"][0]), ci(c["rng"][1]), ci(c["rng"][2]), ci(nt))
    _, plans, gms = env.calib_books(nt)
    ws = _calib_workspace(env, c, nbytes, pattern)
    out = _CalibOut(env, nt, na, given)
    snap = x.clone()
    rc = env.calibrate(x, c["rows"], c["row_len"], c["per_row"], sc.DTYPE_CODE[c["dtype"]], c["mode"], out.xmax.ptr, c["rng"], plans, gms,
                       out.alpha.ptr, out.score.ptr, out.type.ptr, ws.ptr, nbytes)
    assert rc == 0, (c["name"], rc)
    env.sync()
    assert ws.guards_ok(), (c["name"], pattern, "the workspace's guards: a write beyond antq_calibrate_workspace_bytes")
    assert out.guards_ok(), (c["name"], pattern, "the guards of an output")
    assert _same_bytes(x, snap), (c["name"], pattern, "x changed")
    r = out.read()
    if given is not None:
        assert np.array_equal(r["xmax"].view(np.uint32), given.cpu().numpy().view(np.uint32)), (c["name"], pattern, "the given statistic changed")
    return r


def _check_calib(env, c, x, r):
    """antq_calibrate's outputs restated from yardsticks that are no kernel of this library, as include/antq.h defines them
    (the form of test_gpu_search_exact._check_calibration, for every statistic mode, one scale and an empty list):
      x_max   abs-max: the numpy maximum of the tensor's image, bit for bit; 3-sigma: calib_check.exact_three_sigma within
              one rounding step of the dtype (SIGMA_ULP, the floor of the bar of test_three_sigma_against_the_exact_statistic);
      alpha   per (type, row) x_max times a candidate whose yardstick score ties the minimum within the path's bar; x_max
              itself when the list is empty;
      score   the float of the double sum over rows of the best mean squared error, within the path's bar + 2^-22 (the
              float32 roundings of the scores, the figure _check_calibration uses); 1e10 per row when the list is empty;
      type    the first smallest of the returned scores."""
    nt, rows, K, per_row = c["ntypes"], c["rows"], c["row_len"], c["per_row"]
    na, n_per = (rows if per_row else 1), (K if per_row else rows * K)
    img = x.float().cpu().numpy().reshape(na, n_per)
    xm = r["xmax"]
    if c["mode"] == sc.XMAX_ABSMAX:
        assert np.array_equal(xm.view(np.uint32), np.abs(img).max(axis=1).astype(np.float32).view(np.uint32)), (c["name"], "abs-max")
    elif c["mode"] == sc.XMAX_3SIGMA:
        want = exact_three_sigma(img, True, c["dtype"]).astype(np.float64)
        assert (np.abs(xm.astype(np.float64) - want) <= SIGMA_ULP[c["dtype"]] * want).all(), (c["name"], "3-sigma statistic")
    assert np.isfinite(xm).all() and (xm > 0).all()
    ratios = calib_check.ratios_of(*c["rng"])
    score = r["score"]
    if ratios.size == 0:
        assert np.array_equal(r["alpha"].view(np.uint32), np.broadcast_to(xm, (nt, na)).view(np.uint32)), (c["name"], "empty list: alpha is x_max")
        assert np.array_equal(score, np.full(nt, np.float32(na * 1e10), dtype=np.float32)), (c["name"], "empty list: 1e10 per row", score)
        assert int(r["type"][0]) == 0
        return
    which, bar = BARS[c["path"]]
    key = ("calib", c["name"])
    if key not in env.yard_cache:
        cbs = env.calib_books(nt)[0]
        with _timed("yardstick of " + c["name"]):
            xt, xmt = torch.from_numpy(img), torch.from_numpy(xm.copy())
            env.yard_cache[key] = _yard(env.oracle, xt, xmt, ratios, cbs, False, True, which)          # [nt, ncand, na]
    ex = env.yard_cache[key]
    want_score = np.zeros(nt)
    for t in range(nt):
        mse = ex[t] / n_per
        best = mse.min(0)
        for row in range(na):
            cand = (xm[row] * ratios).astype(np.float32)
            hit = np.flatnonzero(cand == r["alpha"][t, row])
            assert hit.size, (c["name"], t, row, "alpha is not x_max times a candidate", r["alpha"][t, row], xm[row])
            assert min(mse[k, row] for k in hit) <= best[row] * (1 + bar), (c["name"], t, row, "picked", hit, "yardstick minimum at", int(mse[:, row].argmin()))
            want_score[t] += float(np.float32(best[row]))
        np.testing.assert_allclose(score[t], np.float32(want_score[t]), rtol=bar + 2.0 ** -22, err_msg=str((c["name"], "score", t)))
    assert int(r["type"][0]) == int(np.argmin(np.where(np.isnan(score), np.inf, score))), (c["name"], "type", r["type"], score)


def _calib_alone(env, name):
    """The case through antq_calibrate alone on a zeroed workspace, checked against its yardsticks ONCE"""
    if name not in env.alone_cache:
        c = sc.calib_case(name)
        x, given = _calib_inputs(env, c)
        r = _calib_run(env, c, x, given, 0x00)
        _check_calib(env, c, x, r)
        env.alone_cache[name] = (x, given, r)
    return env.alone_cache[name]


def _same_outputs(a, b):
    return [k for k in ("alpha", "score", "type", "xmax") if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]


@pytest.mark.parametrize("name", [c["name"] for c in sc.CALIB_CASES])
def test_calibrate_on_a_workspace_of_exactly_the_stated_size(env, name):
    c = sc.calib_case(name)
    with _timed("calibrate " + name):
        x, given, base = _calib_alone(env, name)
        for p in sc.PATTERNS[1:]:
            got = _calib_run(env, c, x, given, p)
            assert not _same_outputs(got, base), (name, "workspace pattern %r changes" % (p,), _same_outputs(got, base))
        # one byte short: ANTQ_ERR_ARG, and not a byte of the workspace or of an output written
        nt, na = c["ntypes"], (c["rows"] if c["per_row"] else 1)
        nbytes = sc.calibrate_workspace_bytes(c["rows"], c["per_row"], *c["rng"], nt)
        _, plans, gms = env.calib_books(nt)
        ws = Slab(nbytes, 0x7F, env.dev)
        out = _CalibOut(env, nt, na, given)
        before = [s.raw.clone() for s in (ws,) + out.slabs]
        rc = env.calibrate(x, c["rows"], c["row_len"], c["per_row"], sc.DTYPE_CODE[c["dtype"]], c["mode"], out.xmax.ptr, c["rng"], plans, gms,
                           out.alpha.ptr, out.score.ptr, out.type.ptr, ws.ptr, nbytes - 1)
        env.sync()
        assert rc == sc.ERR_ARG, (name, "workspace_bytes = total - 1", rc)
        assert all(torch.equal(s.raw, b) for s, b in zip((ws,) + out.slabs, before)), (name, "a refused call wrote something")


class _CalibJob(ctypes.Structure):           # include/antq.h: antq_calib_job
    _fields_ = [("x_dev", vp), ("rows", sz), ("row_len", sz), ("alpha_per_row", ci), ("xmax_mode", ci), ("xmax_dev", vp), ("lb", ci), ("ub", ci),
                ("step", ci), ("ntypes", ci), ("gmax_host", ctypes.POINTER(cf)), ("plan_host", ctypes.POINTER(vp)), ("plan_dev", ctypes.POINTER(vp)),
                ("alpha_dev", vp), ("score_dev", vp), ("type_dev", vp)]


def test_calibrate_batch_shares_one_workspace_between_its_jobs(env):
    """Six jobs of mixed shape, statistic mode, type count and candidate range on ONE workspace of
    antq_calibrate_batch_workspace_bytes (the largest job's need), in two orders, under every pattern: each job's outputs equal
    antq_calibrate of that job alone (which is held to its yardsticks)."""
    cases = [sc.calib_case(n) for n in sc.BATCH_JOBS]
    alone = [_calib_alone(env, n) for n in sc.BATCH_JOBS]
    env.c.antq_calibrate_batch_workspace_bytes.restype = ctypes.c_size_t
    with _timed("calibrate_batch"):
        for order in sc.BATCH_ORDERS:
            for p in sc.PATTERNS:
                arr, keep, outs = (_CalibJob * len(order))(), [], []
                for i, j in enumerate(order):
                    c, (x, given, _) = cases[j], alone[j]
                    nt, na = c["ntypes"], (c["rows"] if c["per_row"] else 1)
                    _, plans, gms = env.calib_books(nt)
                    ph, pd, gm = env.plan_arrays(plans, gms)
                    out = _CalibOut(env, nt, na, given)
                    keep.append((ph, pd, gm))
                    outs.append(out)
                    arr[i] = _CalibJob(x.data_ptr(), c["rows"], c["row_len"], c["per_row"], c["mode"], out.xmax.ptr, c["rng"][0], c["rng"][1], c["rng"][2],
                                       nt, gm, ph, pd, out.alpha.ptr, out.score.ptr, out.type.ptr)
                nbytes = env.c.antq_calibrate_batch_workspace_bytes(arr, ci(len(order)))
                assert nbytes == max(sc.calibrate_workspace_bytes(c["rows"], c["per_row"], *c["rng"], c["ntypes"]) for c in cases)
                ws = _calib_workspace(env, cases[order[0]], nbytes, p)
                snaps = [alone[j][0].clone() for j in order]
                rc = env.c.antq_calibrate_batch(arr, ci(len(order)), ci(sc.DTYPE_CODE[cases[0]["dtype"]]), cu(0), vp(ws.ptr), sz(nbytes), vp(env.st))
                assert rc == 0, (order, p, rc)
                env.sync()
                assert ws.guards_ok(), (order, p, "the shared workspace's guards")
                for i, j in enumerate(order):
                    assert outs[i].guards_ok(), (order, p, "job %d (%s): the guards of an output" % (i, cases[j]["name"]))
                    assert _same_bytes(alone[j][0], snaps[i]), (order, p, i, "x changed")
                    diff = _same_outputs(outs[i].read(), alone[j][2])
                    assert not diff, ("order %s" % (order,), "workspace pattern %r" % (p,), "job %d (%s) differs from antq_calibrate alone in" % (i, cases[j]["name"]), diff)
                # one byte short of the largest need: refused before anything is enqueued for the job that needs it
                if p == 0x00:
                    big = max(range(len(order)), key=lambda i: sc.calibrate_workspace_bytes(cases[order[i]]["rows"], cases[order[i]]["per_row"], *cases[order[i]]["rng"], cases[order[i]]["ntypes"]))
                    one = (_CalibJob * 1)(arr[big])
                    assert env.c.antq_calibrate_batch(one, ci(1), ci(0), cu(0), vp(ws.ptr), sz(nbytes - 1), vp(env.st)) == sc.ERR_ARG
                    env.sync()
