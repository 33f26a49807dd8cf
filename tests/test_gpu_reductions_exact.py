"""Every reduction kernel around the fake-quant hot path -- abs-max, the alpha gradient, OliVe's moments / 3-sigma statistic
(csrc/antq_k_aux.h, antq_k_reduce.h; launchers in antq_kernels.hip) -- with exact sums and planted maxima.

Sections 1-4 compare by EXACT EQUALITY:
  1. integer-valued data in [-128, 128] (exact in bf16 / f16 / fp32): every product, every fp32 partial over a lane's 4 / 8
     elements (< 2^24, also under fma contraction) and every float64 sum is exact in ANY order, so each sum must equal the
     int64 sum bit for bit -- a dropped or double-counted element, tail or half-chunk changes it;
  2. one planted element (|x| = 2 among [-1, 1], NaN, Inf; a single 1 among zeros) moved over the positions where kernels
     go wrong: vector / element tails, the edges of the unrolled loops, chunk and half-chunk edges, each workgroup's first and
     last stride, plus 32 random positions;
  3. sizes derived from the launch geometry (GEOM below mirrors the launchers, each entry names its source line);
  4. one ticket block shared by 200 back-to-back calls of the two one-launch reductions.
Section 5 holds antq_moments + antq_xmax_3sigma to calib_check.exact_three_sigma (math.fsum, two passes) with a bar
measured against the reference's own ops (torch mean / std on the CPU): profiles/reductions_exactness.md.

No case is filtered: every (entry point, dtype, size, position, variant) is asserted and counted, and the count must equal
the product of the table lengths.  The CPU tests at the top prove the yardsticks (`-m "not gpu"`).
"""
import ctypes
import math

import numpy as np
import pytest

import calib_check
from calib_check import exact_three_sigma

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# The launch geometry, restated ONCE from csrc/antq_kernels.hip (a retune of a launcher must show up here as an edit).
#   vec_per_wg : 16-byte vectors a workgroup is sized for (blocks = ceil(n / (vec_per_wg * EPL)), at least 1)
#   cap        : most workgroups of the launch (per element size where it differs)
#   group      : workgroups per ticket group of the one-launch reductions (antq_k_reduce.h)
#   unroll     : the unrolled block-strided loops of the kernel, widest first (vectors in flight per lane)
# ---------------------------------------------------------------------------------------------------------------------
GEOM = {
    # launch_absmax_t: blocks = (n + 64 * EPL * 4 * 4 - 1) / (64 * EPL * 4 * 4); cap 256; group 16; k_absmax_t: 8-way, 4-way
    "absmax_t": dict(vec_per_wg=64 * 4 * 4, cap={4: 256, 2: 256}, group=16, unroll=(8, 4)),
    # launch_alpha_grad_t: blocks = (n + 64 * EPL * 2 * 4 - 1) / (64 * EPL * 2 * 4) (4 chunks of 128 vectors); cap
    # sizeof(T) == 4 ? 256 : 512; group 32; k_alpha_grad_t walks chunks of 128 vectors, one per wavefront and pass
    "alpha_grad_t": dict(vec_per_wg=64 * 2 * 4, cap={4: 256, 2: 512}, group=32, unroll=()),
    # launch_absmax, per tensor: waves = ceil(n / (64 * EPL * 4)), blocks = ceil(waves / 4), cap 256; k_absmax: 8-way, 4-way
    "absmax": dict(vec_per_wg=64 * 4 * 4, cap={4: 256, 2: 256}, unroll=(8, 4)),
    "absmax_into": dict(vec_per_wg=64 * 4 * 4, cap={4: 256, 2: 256}, unroll=(8, 4)),
    # launch_alpha_grad, per tensor: waves = ceil(n / (64 * EPL * 2)), blocks = ceil(waves / 4), cap 1024; k_alpha_grad: 2-way
    "alpha_grad": dict(vec_per_wg=64 * 2 * 4, cap={4: 1024, 2: 1024}, unroll=(2,)),
    # launch_moments, per tensor: waves = ceil(n / (64 * EPL * 4)), blocks = ceil(waves / 4), cap 1024; k_moments: 4-way
    "moments": dict(vec_per_wg=64 * 4 * 4, cap={4: 1024, 2: 1024}, unroll=(4,)),
}
ROW_WAVES = 4 * 4096         # per row (launch_absmax / launch_alpha_grad / launch_moments): cap 4096 workgroups of 4 wavefronts
TK_COUNTER_BYTES = 8320      # antq_k_reduce.h kTkCounterBytes: the part of the ticket block every call must leave zeroed
MAX_ELEMS = 1 << 24          # no input of this module is larger

DT = {"float32": (torch.float32, 4, 4, 0), "bfloat16": (torch.bfloat16, 8, 2, 1), "float16": (torch.float16, 8, 2, 2)}
#       name -> (torch dtype, EPL = elements per 16-byte vector, element size, ANTQ_* dtype code)
GARBAGE = 0x7f7f7f7f         # what a result slot holds before an entry point that WRITES its result
N_RANDOM = 32                # random positions per (size, dtype); the boundary set is never thinned


def blocks_of(op, n, dtname):
    _, epl, esize, _ = DT[dtname]
    g = GEOM[op]
    per = g["vec_per_wg"] * epl
    return max(1, min((n + per - 1) // per, g["cap"][esize]))


def tensor_sizes(op, dtname):
    """[(n, storage offset in elements)] of the per-tensor forms of `op`: workgroup counts around one workgroup, a ticket
    group, the cap and several passes beyond it, with n % EPL cycling through 0, 1, EPL - 1, EPL + 3; the same through a view
    offset by one element (element path); n = 1 and n = EPL - 1."""
    _, epl, esize, _ = DT[dtname]
    g = GEOM[op]
    per, cap = g["vec_per_wg"] * epl, g["cap"][esize]
    if "group" in g:
        G = g["group"]
        counts = [1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, cap - 1, cap]
    else:
        counts = [1, 2, cap - 1, cap]
    tails = [0, 1, epl - 1, epl + 3]
    sizes = [(w * per - tails[i % 4], 0) for i, w in enumerate(counts)]
    stride = cap * 256 * epl                      # elements one block-strided pass of the capped grid covers
    if op == "alpha_grad_t":
        # within one size class: nv % 128 in {0, 1, 63, 64, 65, 127} x n % EPL in {0, 1, EPL - 1}, then several passes
        base = 3 * per
        sizes += [(base + v * epl + t, 0) for v in (0, 1, 63, 64, 65, 127) for t in (0, 1, epl - 1)]
        sizes += [(2 * cap * per + 64 * epl + 1, 0), (3 * cap * per + 129 * epl + epl - 1, 0), (5 * cap * per, 0)]
    else:
        u = g["unroll"][0]                        # 3 strides, widest loop + 1 stride, widest + next loop + 1 stride (8x+1 ...)
        sizes += [(3 * stride, 0), ((u + 1) * stride + 3 * epl + 1, 0), ((u + u // 2 + 1) * stride - epl, 0)]
    sizes += [(2 * per + 5, 1), (cap * per + epl + 1, 1), (1, 0), (epl - 1, 0), (1, 1)]
    assert all(0 < n and n + off <= MAX_ELEMS for n, off in sizes)
    return sizes


def _clip(P, n):
    return [min(max(int(p), 0), n - 1) for p in P]


def tensor_positions(op, n, dtname, seed):
    """The boundary set of one per-tensor launch + N_RANDOM random positions; a FIXED number of entries for a given op
    (out-of-range candidates are clipped into [0, n), never dropped, so that the tables multiply out)."""
    _, epl, _, _ = DT[dtname]
    B = blocks_of(op, n, dtname)
    nv, S = n // epl, B * 256
    P = [0, 1, epl - 1, epl] + list(range(n - epl - 1, n)) + [nv * epl - 1, nv * epl]
    wgs = [0, 1, B // 2, max(B - 2, 0), B - 1]
    if op == "alpha_grad_t":
        nch, nw = (nv + 127) // 128, B * 4
        last_pass = max(nch - 1, 0) // nw * nw                                   # first chunk of the last pass
        for c in (1, nch // 2, nch - 1, nw - 1, nw, last_pass, last_pass - 1):     # chunk edges +-1 vector, half-chunk edge
            for v in (c * 128 - 1, c * 128, c * 128 + 1, c * 128 + 63, c * 128 + 64, c * 128 + 65, c * 128 + 127):
                P += [v * epl, v * epl + epl - 1]
        for b in wgs:                       # first / last element of each workgroup's first and last pass (4 chunks each)
            c0 = min(b, B - 1) * 4
            P += [c0 * 128 * epl, (c0 + 4) * 128 * epl - 1, (last_pass + c0) * 128 * epl, (last_pass + c0 + 4) * 128 * epl - 1]
    else:
        for b in wgs:                       # first / last element of each workgroup's first and last stride
            first = min(b, B - 1) * 256
            k = max(nv - 1 - first, 0) // S
            P += [first * epl, (first + 256) * epl - 1, (k * S + first) * epl, (k * S + first + 256) * epl - 1]
        for tid in (0, S - 1):              # the first vector each unrolled loop leaves to the loops after it
            i = tid
            for u in GEOM[op]["unroll"]:
                while i + (u - 1) * S < nv:
                    i += u * S
                P += [i * epl - 1, i * epl, i * epl + epl - 1]
    rng = np.random.default_rng(seed)
    P += [int(p) for p in rng.integers(0, n, N_RANDOM)]
    return _clip(P, n)


def n_tensor_positions(op, dtname):
    return len(tensor_positions(op, 100003, dtname, 0))


# ---------------------------------------------------------------------------------------------------------------------
# per-row shapes and positions
# ---------------------------------------------------------------------------------------------------------------------
def row_shapes(op, dtname):
    """[(rows, K)]: abs-max through all three kernels (k_absmax_groups: a power of two of 1 .. 64 vectors; k_absmax_rows:
    128 / 256 / 512 / 1024 vectors; k_absmax: everything else incl. 65, 127, 1025 vectors and rows that are no multiple of
    EPL); sums with rows of every remainder of the 2-way / 4-way loops; rows = 1, 3, and more rows than the grid holds
    wavefronts (the row loop wraps)."""
    _, epl, _, _ = DT[dtname]
    if op == "absmax":
        vprs = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 3, 65, 127, 1025]
    else:
        vprs = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1025]
    shapes = [(3, v * epl) for v in vprs]
    shapes += [(1, 65 * epl), (1, 1), (3, 1), (3, epl - 1), (3, 65 * epl + 1), (5, 257 * epl + epl - 1)]
    shapes += [(1030, 2 * epl), (ROW_WAVES + 5, 3 * epl), (ROW_WAVES + 5, epl + 1)]
    assert all(r * k <= MAX_ELEMS for r, k in shapes)
    return shapes


def row_positions(rows, K, dtname, seed):
    """(row, column) pairs: rows 0, middle, the last one before / the first one after the row loop wraps, last; columns at
    the element / vector edges, the 64-lane strides and the unrolled loops' edges, + 8 random.  Fixed length, clipped."""
    _, epl, _, _ = DT[dtname]
    vpr = K // epl
    C = [0, 1, epl - 1, epl] + list(range(K - epl - 1, K)) + [vpr * epl - 1, vpr * epl]
    for v in (63, 64, 65, 127, 128, 191, 192, 255, 256, 257, vpr - vpr % 64 - 1, vpr - vpr % 64, vpr - vpr % 128, vpr - vpr % 256, vpr - 1):
        C += [v * epl, v * epl + epl - 1]
    rng = np.random.default_rng(seed)
    C += [int(c) for c in rng.integers(0, K, 8)]
    C = _clip(C, K)
    R = _clip([0, rows // 2, ROW_WAVES - 1, ROW_WAVES, rows - 1], rows)
    return [(R[i % len(R)], c) for i, c in enumerate(C)] + [(r, C[-1 - j]) for j, r in enumerate(R)]


def n_row_positions(dtname):
    return len(row_positions(3, 1000, dtname, 0))


# ---------------------------------------------------------------------------------------------------------------------
# CPU self-checks of the yardsticks (run under -m "not gpu")
# ---------------------------------------------------------------------------------------------------------------------
def _int_data(n, seed, dtname, dev="cpu"):
    """x, out, gout: random integers in [-128, 128] in the tensor's dtype, and the int64 images."""
    gen = torch.Generator().manual_seed(seed)
    ints = [torch.randint(-128, 129, (n,), generator=gen, dtype=torch.int64) for _ in range(3)]
    return [i.to(DT[dtname][0]).to(dev) for i in ints], [i.numpy() for i in ints]


def test_all_513_integers_survive_bf16_and_f16():
    v = torch.arange(-128, 129, dtype=torch.float32)
    w = torch.cat([v, v * 2.0 ** -10, v * 2.0 ** 8])
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(w.to(dt).float(), w), dt
    assert torch.equal((v * 2.0 ** 20).to(torch.bfloat16).float(), v * 2.0 ** 20)
    assert not torch.isfinite((v * 2.0 ** 20).to(torch.float16)).all()       # (why f16 is scaled by 2^8 instead, section 1)


def test_integer_sums_are_exact_in_the_kernels_arithmetic_and_one_element_shows():
    """numpy emulation of "fp32 over a lane's 8 elements, float64 beyond" on 2^20 elements: equal to the int64 sum whatever
    the order (two orders tried), every fp32 partial an integer below 2^24 (so fma contraction cannot change it); removing
    or doubling ONE element changes the expected value."""
    n = 1 << 20
    for dtname in DT:
        (x, o, g), (xi, oi, gi) = _int_data(n, 11, dtname)
        want = int((gi * (oi - xi)).sum())
        xf, of, gf = (t.float().numpy() for t in (x, o, g))
        term = (gf * (of - xf).astype(np.float32)).astype(np.float32)
        for order in (np.arange(n), np.random.default_rng(0).permutation(n)):
            part = np.zeros(n // 8, dtype=np.float32)
            for e in range(8):
                part = (part + term[order].reshape(-1, 8)[:, e]).astype(np.float32)
            assert np.abs(part).max() < 2 ** 24 and np.array_equal(part, np.rint(part))
            assert float(part.astype(np.float64).sum()) == float(want)
            assert float(part.astype(np.float64)[::-1].cumsum()[-1]) == float(want)          # a sequential float64 order
        assert abs(want) < 2 ** 53
        p = int(np.flatnonzero(gi * (oi - xi))[12345])
        t = int(gi[p] * (oi[p] - xi[p]))
        assert want - t != want and want + t != want and float(want - t) != float(want) and float(want + t) != float(want)
        s2 = int((xi * xi).sum())
        q = int(np.flatnonzero(xi)[777])
        assert float(s2 - int(xi[q]) ** 2) != float(s2) and float(int(xi.sum()) + int(xi[q])) != float(int(xi.sum()))
        assert 16384 * MAX_ELEMS < 2 ** 53 and 128 * 256 * MAX_ELEMS < 2 ** 53


def test_position_tables_are_in_range_and_multiply_out():
    """Every planted position is < n (asserted again on the host before any launch), the tables have one length per entry
    point, and the structural positions are really in them."""
    for op in GEOM:
        for dtname, (_, epl, _, _) in DT.items():
            for n, off in tensor_sizes(op, dtname):
                P = tensor_positions(op, n, dtname, n)
                assert len(P) == n_tensor_positions(op, dtname) and all(0 <= p < n for p in P), (op, dtname, n)
                nv = n // epl
                assert {0, n - 1, min(nv * epl, n - 1), max(nv * epl - 1, 0)} <= set(P)
    for op in ("absmax", "moments", "alpha_grad"):
        for dtname in DT:
            for rows, K in row_shapes(op, dtname):
                P = row_positions(rows, K, dtname, K)
                assert len(P) == n_row_positions(dtname) and all(0 <= r < rows and 0 <= c < K for r, c in P)
                assert (0, 0) in P and (rows - 1) in {r for r, _ in P} and (K - 1) in {c for _, c in P}
    # the workgroup counts the size tables are meant to reach
    for dtname, (_, epl, esize, _) in DT.items():
        got = sorted({blocks_of("absmax_t", n, dtname) for n, _ in tensor_sizes("absmax_t", dtname)})
        assert set([1, 2, 15, 16, 17, 31, 32, 33, 255, 256]) <= set(got), got
        cap = 256 if esize == 4 else 512
        got = sorted({blocks_of("alpha_grad_t", n, dtname) for n, _ in tensor_sizes("alpha_grad_t", dtname)})
        assert set([1, 2, 31, 32, 33, 63, 64, 65, cap - 1, cap]) <= set(got), got


def test_exact_three_sigma_agrees_with_the_oracle_on_the_existing_inputs(oracle):
    """The inputs and tolerances of test_olive_three_sigma_statistic_on_one_read (tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(31)
    for rows, K in ((64, 4096), (7, 33), (3, 8200), (1, 1), (5, 1), (128, 64)):
        x = (rng.standard_normal((rows, K)) * 0.05 + 0.01).astype(np.float32)
        x.reshape(-1)[::37] *= 12
        if rows > 2 and K > 1:
            x[2] = 0.75
        for bf16 in (False, True):
            xh = oracle.f32_to_bf16(x) if bf16 else x
            xf = oracle.bf16_to_f32(xh) if bf16 else xh
            for per_row in (True, False):
                want = oracle.three_sigma(xh, per_row)
                got = exact_three_sigma(xf, per_row, "bfloat16" if bf16 else "float32")
                nan = np.isnan(want)
                assert got.shape == want.shape and np.array_equal(np.isnan(got), nan)
                np.testing.assert_allclose(got[~nan], want[~nan], rtol=2.0 ** -7 if bf16 else 2e-6)
    assert exact_three_sigma(np.full((1, 1000), np.float32(0.1)), False)[0] == np.float32(0.1)        # std exactly 0
    assert np.array_equal(calib_check._round_bf16(np.float32([1.00390625, 1.01171875, -0.1])),
                          torch.tensor([1.00390625, 1.01171875, -0.1]).bfloat16().float().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Abi:
    """The seven entry points on raw device pointers (results land in slots of one device tensor: no synchronisation per
    call), one ticket block of its own, the stream's partials workspace."""

    def __init__(self, L, dev):
        self.c, self.L, self.dev = L.lib(), L, dev
        self.st = L._stream_int(dev)
        self.red = torch.zeros(L.REDUCE_WS_BYTES, dtype=torch.uint8, device=dev)
        self.ws = L._workspace(dev)

    @staticmethod
    def _ok(rc, what):
        assert rc == 0, (what, rc)

    def absmax_t(self, x, slot, n, dt):
        self._ok(self.c.antq_absmax_t(x, slot, n, dt, self.red.data_ptr(), self.st), "antq_absmax_t")

    def absmax(self, x, slot, rows, K, per_row, dt):
        self._ok(self.c.antq_absmax(x, slot, rows, K, per_row, dt, self.st), "antq_absmax")

    def absmax_into(self, x, slot, n, dt):
        self._ok(self.c.antq_absmax_into(x, slot, n, dt, self.st), "antq_absmax_into")

    def alpha_grad_t(self, x, o, g, n, slot, dt):
        self._ok(self.c.antq_alpha_grad_t(x, o, g, n, slot, dt, self.red.data_ptr(), self.st), "antq_alpha_grad_t")

    def alpha_grad(self, x, o, g, rows, K, per_row, slot, dt):
        self._ok(self.c.antq_alpha_grad(x, o, g, rows, K, per_row, slot, self.ws.data_ptr(), dt, self.st), "antq_alpha_grad")

    def moments(self, x, rows, K, per_row, dt, slot):
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self._ok(self.c.antq_moments(vp(x), sz(rows), sz(K), ci(per_row), ci(dt), vp(slot), vp(self.ws.data_ptr()), vp(self.st)),
                 "antq_moments")

    def counters_zero(self):
        return int(self.red[:TK_COUNTER_BYTES].count_nonzero().item()) == 0


@pytest.fixture(scope="module")
def abi(antq_lib, dev):
    return _Abi(antq_lib, dev)


def _view(t, off):
    """The tensor through a view `off` elements into its storage (off = 1: not 16-byte aligned, the element path)."""
    v = t[off:]
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


CELLS = {}


def _count(key, k):
    CELLS[key] = CELLS.get(key, 0) + k


# ---- sections 1-3, per tensor: abs-max ---------------------------------------------------------------------------------
# (planted value, what the slot holds before the call: None = garbage, expected result)
ABSMAX_VARIANTS = [(2.0, None, 2.0), (-2.0, None, 2.0), (float("nan"), None, float("nan")), (float("inf"), None, float("inf")),
                   (float("-inf"), None, float("inf"))]
INTO_VARIANTS = [(2.0, 0.0, 2.0), (-2.0, 0.0, 2.0), (float("nan"), 0.0, float("nan")), (float("inf"), 0.0, float("inf")),
                 (float("-inf"), 0.0, float("inf")), (2.0, 3.0, 3.0), (-2.0, 1.5, 2.0)]


def _absmax_call(abi, op, xp, slot, n, code):
    if op == "absmax_t":
        abi.absmax_t(xp, slot, n, code)
    elif op == "absmax":
        abi.absmax(xp, slot, 1, n, 0, code)
    else:
        abi.absmax_into(xp, slot, n, code)


@gpu
@pytest.mark.parametrize("op", ["absmax_t", "absmax", "absmax_into"])
def test_planted_maximum_whole_tensor(abi, dev, op):
    """All elements in [-1, 1], x[p] = +-2 / NaN / +-Inf at every position of the table: exactly 2.0 / NaN ("NaN wins") / Inf.
    antq_absmax_t and antq_absmax WRITE the slot (it holds garbage before); antq_absmax_into accumulates (a slot holding 3.0
    stays 3.0, one holding 1.5 becomes 2.0).  Without the planted element: the float64-free maximum of the data."""
    variants = INTO_VARIANTS if op == "absmax_into" else ABSMAX_VARIANTS
    for dtname, (tdt, epl, esize, code) in DT.items():
        npos = n_tensor_positions(op, dtname)
        sizes = tensor_sizes(op, dtname)
        for n, off in sizes:
            gen = torch.Generator().manual_seed(n * 7 + off)
            host = (torch.rand(n + off, generator=gen) * 2 - 1).to(tdt)
            xd = _view(host.to(dev), off)
            hostf = host[off:].float().numpy()
            P = tensor_positions(op, n, dtname, n + off)
            assert len(P) == npos and all(0 <= p < n for p in P) and xd.numel() == n
            res = torch.empty(len(variants) + 1, npos, dtype=torch.float32, device=dev)
            res.view(torch.int32).fill_(GARBAGE)
            if op == "absmax_into":
                res[-1].fill_(0.0)
            _absmax_call(abi, op, xd.data_ptr(), res[-1].data_ptr(), n, code)          # the plain maximum, nothing planted
            for vi, (val, pre, _) in enumerate(variants):
                if pre is not None:
                    res[vi].fill_(pre)
                base = res[vi].data_ptr()
                for k, p in enumerate(P):
                    cell = xd[p:p + 1]
                    cell.fill_(val)
                    _absmax_call(abi, op, xd.data_ptr(), base + 4 * k, n, code)
                    cell.fill_(float(hostf[p]))
            got = res.cpu().numpy()
            assert torch.equal(xd.cpu(), host[off:])                                   # every planted element was restored
            assert got[-1, 0] == np.abs(hostf).max(), (op, dtname, n, off, "plain", got[-1, 0], np.abs(hostf).max())
            for vi, (val, pre, want) in enumerate(variants):
                w = np.full(npos, want, dtype=np.float32)
                bad = np.flatnonzero(_bits(got[vi]) != _bits(w)) if not math.isnan(want) else np.flatnonzero(~np.isnan(got[vi]))
                assert bad.size == 0, (op, dtname, "n=%d off=%d blocks=%d" % (n, off, blocks_of(op, n, dtname)),
                                       "planted %r, slot before %r" % (val, pre), "positions", [P[i] for i in bad[:8]],
                                       "got", got[vi][bad[:8]], "want", want)
                _count(op, npos)
        assert abi.counters_zero()
    assert CELLS[op] == sum(len(tensor_sizes(op, d)) * n_tensor_positions(op, d) * len(variants) for d in DT), CELLS[op]
    print("REDUCTIONS | %s planted maximum | %d cells, all exact" % (op, CELLS[op]), flush=True)


# ---- sections 1-3, per tensor: sums -------------------------------------------------------------------------------------
def _sum_call(abi, op, ptrs, slot, n, code):
    if op == "alpha_grad_t":
        abi.alpha_grad_t(ptrs[0], ptrs[1], ptrs[2], n, slot, code)
    elif op == "alpha_grad":
        abi.alpha_grad(ptrs[0], ptrs[1], ptrs[2], 1, n, 0, slot, code)
    else:
        abi.moments(ptrs[0], 1, n, 0, code, slot)


def _scales(dtname):
    # (f16 cannot hold 128 * 2^20: its second power of two is 2^8, which keeps every value and square-free sum exact)
    return (1.0, 2.0 ** -10, 2.0 ** 8 if dtname == "float16" else 2.0 ** 20)


@gpu
@pytest.mark.parametrize("op", ["alpha_grad_t", "alpha_grad", "moments"])
def test_exact_sums_whole_tensor(abi, dev, op):
    """Integer data: gsum == the int64 sum of g * (out - x), sums == (sum x, sum x^2), also scaled by powers of two; one-hot
    at every position of the table: exactly 1.0 (moments: (1, 1)); all-ones: exactly n."""
    w = 2 if op == "moments" else 1                      # doubles per result
    for dtname, (tdt, epl, esize, code) in DT.items():
        npos = n_tensor_positions(op, dtname)
        for n, off in tensor_sizes(op, dtname):
            P = tensor_positions(op, n, dtname, n + off)
            assert len(P) == npos and all(0 <= p < n for p in P)
            key = "%s n=%d off=%d blocks=%d" % (dtname, n, off, blocks_of(op, n, dtname))
            # 1. integer data (and scaled by powers of two for the moments)
            (x, o, g), (xi, oi, gi) = _int_data(n + off, n + off, dtname, dev)
            xi, oi, gi = xi[off:], oi[off:], gi[off:]
            scales = _scales(dtname) if op == "moments" else (1.0,)
            res = torch.full((len(scales) + 1, w), float("nan"), dtype=torch.float64, device=dev)
            keep = []
            for si, s in enumerate(scales):
                t = [_view(v * s if s != 1.0 else v, off) for v in (x, o, g)]
                keep.append(t)
                _sum_call(abi, op, [v.data_ptr() for v in t], res[si].data_ptr(), n, code)
            # all-ones: g = 1, out = 1, x = 0 (moments: x = 1)
            ones, zeros = torch.ones(n + off, dtype=tdt, device=dev), torch.zeros(n + off, dtype=tdt, device=dev)
            t1 = [_view(ones if op == "moments" else zeros, off), _view(ones, off), _view(ones, off)]
            _sum_call(abi, op, [v.data_ptr() for v in t1], res[-1].data_ptr(), n, code)
            got = res.cpu().numpy()
            for si, s in enumerate(scales):
                want = [float(xi.sum()) * s, float((xi * xi).sum()) * s * s] if op == "moments" else [float((gi * (oi - xi)).sum())]
                assert got[si].tolist() == want, (op, key, "integer data x %g" % s, got[si].tolist(), want)
            assert got[-1].tolist() == [float(n)] * w, (op, key, "all ones", got[-1].tolist(), n)
            _count(op + " integer", len(scales) + 1)
            # 2. one-hot at every position: two one-element device writes to plant, two to clear
            zx, zo, zg = (torch.zeros(n + off, dtype=tdt, device=dev)[off:] for _ in range(3))
            ptrs = [zx.data_ptr(), zo.data_ptr(), zg.data_ptr()]
            hot = torch.full((npos, w), float("nan"), dtype=torch.float64, device=dev)
            base = hot.data_ptr()
            for k, p in enumerate(P):
                cells = (zx[p:p + 1],) if op == "moments" else (zo[p:p + 1], zg[p:p + 1])
                for c in cells:
                    c.fill_(1.0)
                _sum_call(abi, op, ptrs, base + 8 * w * k, n, code)
                for c in cells:
                    c.fill_(0.0)
            got = hot.cpu().numpy()
            bad = np.flatnonzero((got != 1.0).any(axis=1))
            assert bad.size == 0, (op, key, "one-hot", "positions", [P[i] for i in bad[:8]], "got", got[bad[:8]].tolist())
            _count(op, npos)
        assert abi.counters_zero()
    nsz = len(tensor_sizes(op, "float32"))
    assert CELLS[op] == sum(nsz * n_tensor_positions(op, d) for d in DT), CELLS[op]
    assert CELLS[op + " integer"] == len(DT) * nsz * (len(_scales("float32")) + 1 if op == "moments" else 2)
    print("REDUCTIONS | %s exact sums | %d one-hot cells + %d integer sums, all exact" % (op, CELLS[op], CELLS[op + " integer"]),
          flush=True)


# ---- sections 1-3, per row ----------------------------------------------------------------------------------------------
@gpu
def test_planted_maximum_per_row(abi, dev):
    """antq_absmax per row through k_absmax_groups, k_absmax_rows and k_absmax: the planted element decides ITS row and no
    other; every other row keeps the maximum of its data."""
    variants = [2.0, float("nan"), float("inf")]
    for dtname, (tdt, epl, esize, code) in DT.items():
        npos = n_row_positions(dtname)
        for rows, K in row_shapes("absmax", dtname):
            gen = torch.Generator().manual_seed(rows * 131 + K)
            host = (torch.rand(rows, K, generator=gen) * 2 - 1).to(tdt)
            xd = host.to(dev)
            flat = xd.view(-1)
            hostf = host.float().numpy()
            plain = np.abs(hostf).max(axis=1)
            P = row_positions(rows, K, dtname, K)
            assert len(P) == npos and all(0 <= r < rows and 0 <= c < K for r, c in P)
            res = torch.empty(len(variants), npos, rows, dtype=torch.float32, device=dev)
            res.view(torch.int32).fill_(GARBAGE)
            for vi, val in enumerate(variants):
                for k, (r, c) in enumerate(P):
                    cell = flat[r * K + c:r * K + c + 1]
                    cell.fill_(val if k % 2 == 0 else -val)
                    abi.absmax(xd.data_ptr(), res[vi, k].data_ptr(), rows, K, 1, code)
                    cell.fill_(float(hostf[r, c]))
            got = res.cpu().numpy()
            for vi, val in enumerate(variants):
                want = np.broadcast_to(plain, (npos, rows)).copy()
                for k, (r, c) in enumerate(P):
                    want[k, r] = abs(val)
                same = (_bits(got[vi]) == _bits(want)) | (np.isnan(got[vi]) & np.isnan(want))
                assert same.all(), ("absmax per row", dtname, rows, K, "planted %r" % val,
                                    [(P[k], int(r)) for k, r in zip(*np.nonzero(~same))][:8])
                _count("absmax rows", npos)
    assert CELLS["absmax rows"] == sum(len(row_shapes("absmax", d)) * n_row_positions(d) * len(variants) for d in DT)
    print("REDUCTIONS | absmax per row | %d cells (each a whole result vector), all exact" % CELLS["absmax rows"], flush=True)


@gpu
@pytest.mark.parametrize("op", ["alpha_grad", "moments"])
def test_exact_sums_per_row(abi, dev, op):
    """Per row: integer data == the int64 row sums; one-hot: exactly 1.0 in its row and 0.0 in every other; all-ones: K."""
    w = 2 if op == "moments" else 1

    def call(t, slot, rows, K, code):
        if op == "moments":
            abi.moments(t[0].data_ptr(), rows, K, 1, code, slot)
        else:
            abi.alpha_grad(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), rows, K, 1, slot, code)

    for dtname, (tdt, epl, esize, code) in DT.items():
        npos = n_row_positions(dtname)
        for rows, K in row_shapes(op, dtname):
            n = rows * K
            (x, o, g), (xi, oi, gi) = _int_data(n, n + 3, dtname, dev)
            xi, oi, gi = (a.reshape(rows, K) for a in (xi, oi, gi))
            res = torch.full((2, rows, w), float("nan"), dtype=torch.float64, device=dev)
            call((x, o, g), res[0].data_ptr(), rows, K, code)
            ones, zeros = torch.ones(n, dtype=tdt, device=dev), torch.zeros(n, dtype=tdt, device=dev)
            call((ones, ones, ones) if op == "moments" else (zeros, ones, ones), res[1].data_ptr(), rows, K, code)
            got = res.cpu().numpy()
            want = np.stack([xi.sum(1), (xi * xi).sum(1)], 1) if op == "moments" else (gi * (oi - xi)).sum(1)[:, None]
            assert np.array_equal(got[0], want.astype(np.float64)), (op, dtname, rows, K, "integer rows", np.flatnonzero((got[0] != want).any(1))[:8])
            assert np.array_equal(got[1], np.full((rows, w), float(K))), (op, dtname, rows, K, "all ones")
            _count(op + " rows integer", 2)
            zx, zo, zg = (torch.zeros(n, dtype=tdt, device=dev) for _ in range(3))
            P = row_positions(rows, K, dtname, K)
            assert len(P) == npos and all(0 <= r < rows and 0 <= c < K for r, c in P)
            hot = torch.full((npos, rows, w), float("nan"), dtype=torch.float64, device=dev)
            for k, (r, c) in enumerate(P):
                i = r * K + c
                cells = (zx[i:i + 1],) if op == "moments" else (zo[i:i + 1], zg[i:i + 1])
                for cc in cells:
                    cc.fill_(1.0)
                call((zx, zo, zg), hot[k].data_ptr(), rows, K, code)
                for cc in cells:
                    cc.fill_(0.0)
            got = hot.cpu().numpy()
            want = np.zeros((npos, rows, w))
            for k, (r, c) in enumerate(P):
                want[k, r] = 1.0
            assert np.array_equal(got, want), (op, dtname, rows, K, "one-hot", [P[k] for k in np.unique(np.nonzero(got != want)[0])[:8]])
            _count(op + " rows", npos)
    nsh = len(row_shapes(op, "float32"))
    assert CELLS[op + " rows"] == sum(nsh * n_row_positions(d) for d in DT) and CELLS[op + " rows integer"] == len(DT) * nsh * 2
    print("REDUCTIONS | %s per row | %d one-hot cells + %d integer cases, all exact" % (op, CELLS[op + " rows"], CELLS[op + " rows integer"]),
          flush=True)


# ---- section 3, the ticket-group / workgroup-count knobs --------------------------------------------------------------
# (workgroups, workgroups per group): every pair fits the ticket block's layout (<= 1024 workgroups, <= 64 groups, <= 64
# per group); the launchers clamp anything else (antq_kernels.hip: clamp_to_ticket_layout), which is read, not tried
KNOB_SETTINGS = [(3, 1), (64, 1), (100, 8), (512, 8), (1024, 16), (1024, 64)]


@gpu
def test_ticket_group_and_workgroup_knobs(abi, dev):
    """antq_debug_set keys 17 / 18 reach group sizes 1, 8, 16, 64 and 1024 workgroups at one n: same exact results."""
    n = (1 << 23) + 4099
    knob = abi.c.antq_debug_set
    cells = 0
    try:
        for dtname, (tdt, epl, esize, code) in DT.items():
            (x, o, g), (xi, oi, gi) = _int_data(n, 5, dtname, dev)
            want_sum, want_max = float((gi * (oi - xi)).sum()), float(np.abs(xi).max())
            P = _clip([0, n - 1, n // epl * epl, 4096 * epl - 1, 4096 * epl] + [int(p) for p in np.random.default_rng(3).integers(0, n, 8)], n)
            res = torch.empty(len(KNOB_SETTINGS), 2 + len(P), dtype=torch.float64, device=dev)
            amx = torch.empty(len(KNOB_SETTINGS), 2 + len(P), dtype=torch.float32, device=dev)
            amx.view(torch.int32).fill_(GARBAGE)
            for si, (blocks, group) in enumerate(KNOB_SETTINGS):
                assert blocks <= 1024 and group <= 64 and (blocks + group - 1) // group <= 64
                knob(18, blocks); knob(17, group)
                abi.alpha_grad_t(x.data_ptr(), o.data_ptr(), g.data_ptr(), n, res[si, 0].data_ptr(), code)
                abi.absmax_t(x.data_ptr(), amx[si, 0].data_ptr(), n, code)
                for k, p in enumerate(P):
                    cell = x[p:p + 1]
                    cell.fill_(-300.0)
                    abi.absmax_t(x.data_ptr(), amx[si, 2 + k].data_ptr(), n, code)
                    abi.alpha_grad_t(x.data_ptr(), o.data_ptr(), g.data_ptr(), n, res[si, 2 + k].data_ptr(), code)
                    cell.fill_(float(xi[p]))
            got_s, got_m = res.cpu().numpy(), amx.cpu().numpy()
            for si, st in enumerate(KNOB_SETTINGS):
                assert got_s[si, 0] == want_sum and got_m[si, 0] == want_max, (dtname, st, got_s[si, 0], want_sum, got_m[si, 0], want_max)
                for k, p in enumerate(P):
                    ws = want_sum - float(gi[p] * (oi[p] - xi[p])) + float(gi[p] * (oi[p] + 300))
                    assert got_m[si, 2 + k] == 300.0 and got_s[si, 2 + k] == ws, (dtname, st, p, got_m[si, 2 + k], got_s[si, 2 + k], ws)
                    cells += 1
            assert abi.counters_zero()
    finally:
        knob(17, 0); knob(18, 0)
    assert cells == len(DT) * len(KNOB_SETTINGS) * 13


# ---- section 4: the ticket block across calls ----------------------------------------------------------------------
@gpu
def test_ticket_block_shared_by_200_back_to_back_calls(abi, antq_lib, dev):
    """One ticket block, one stream, 200 calls alternating antq_absmax_t / antq_alpha_grad_t over the size tables in a seeded
    shuffle, no synchronisation in between: every result exact, the counter region zero afterwards, the replay gives the
    same bits.  Then the same sizes through _lib.absmax_t / _lib.alpha_grad(per_row=False) and the stream's own block."""
    for dtname, (tdt, epl, esize, code) in DT.items():
        sizes = sorted(set(tensor_sizes("absmax_t", dtname) + tensor_sizes("alpha_grad_t", dtname)))
        nmax = max(n + off for n, off in sizes)
        (x, o, g), (xi, oi, gi) = _int_data(nmax, 77, dtname, dev)
        term = gi * (oi - xi)
        order = np.random.default_rng(2026).permutation(200) % len(sizes)
        want_m, want_s = np.full(200, np.nan, dtype=np.float32), np.full(200, np.nan)
        for i, si in enumerate(order):
            n, off = sizes[si]
            if i % 2 == 0:
                want_m[i] = np.abs(xi[off:off + n]).max()
            else:
                want_s[i] = float(term[off:off + n].sum())
        runs = []
        for rep in range(2):
            am = torch.empty(200, dtype=torch.float32, device=dev)
            am.view(torch.int32).fill_(GARBAGE)
            gs = torch.full((200,), float("nan"), dtype=torch.float64, device=dev)
            for i, si in enumerate(order):
                n, off = sizes[si]
                ptr = [t.data_ptr() + off * esize for t in (x, o, g)]
                if i % 2 == 0:
                    abi.absmax_t(ptr[0], am[i].data_ptr(), n, code)
                else:
                    abi.alpha_grad_t(ptr[0], ptr[1], ptr[2], n, gs[i].data_ptr(), code)
            runs.append((am.cpu().numpy(), gs.cpu().numpy()))
            assert abi.counters_zero(), (dtname, "counter region not zero after the sequence", rep)
        for i, si in enumerate(order):
            got = runs[0][0][i] if i % 2 == 0 else runs[0][1][i]
            want = want_m[i] if i % 2 == 0 else want_s[i]
            assert got == want, (dtname, "call %d of the sequence" % i, "absmax_t" if i % 2 == 0 else "alpha_grad_t", sizes[si],
                                 "previous call", sizes[order[i - 1]] if i else None, got, want)
        ev, od = np.arange(0, 200, 2), np.arange(1, 200, 2)
        assert np.array_equal(_bits(runs[0][0][ev]), _bits(runs[1][0][ev])) and np.array_equal(_bits(runs[0][1][od]), _bits(runs[1][1][od]))
        # through the binding (the stream's own ticket block)
        outs = []
        for n, off in sizes:
            xv, ov, gv = (t[off:off + n] for t in (x, o, g))
            outs.append((antq_lib.absmax_t(xv), antq_lib.alpha_grad(xv, ov, gv, 1, n, per_row=False), n, off))
        for am, gs, n, off in outs:
            assert am.item() == np.abs(xi[off:off + n]).max() and gs.item() == float(term[off:off + n].sum()), (dtname, "_lib", n, off)
        assert int(antq_lib._reduce_ws(dev)[:TK_COUNTER_BYTES].count_nonzero().item()) == 0


# ---- section 5: the 3-sigma statistic -----------------------------------------------------------------------------
def _gauss(mean, std):
    return lambda rng, n: (rng.standard_normal(n, dtype=np.float32) * np.float32(std) + np.float32(mean)).astype(np.float32)


def _const(v):
    return lambda rng, n: np.full(n, np.float32(v), dtype=np.float32)


SIGMA_DISTS = [("mean 0.01 / std 0.05", _gauss(0.01, 0.05)), ("mean 100 / std 0.01", _gauss(100, 0.01)),
               ("mean 1e4 / std 1e-2", _gauss(1e4, 1e-2)), ("mean 1e6 / std 1", _gauss(1e6, 1.0)), ("mean 3e7 / std 4", _gauss(3e7, 4.0)),
               ("constant 0.1f", _const(0.1)), ("constant 1/3", _const(1.0 / 3.0)), ("constant 1e-30", _const(1e-30)),
               ("constant 3e38", _const(3e38)),
               ("all negative", lambda rng, n: (-np.abs(rng.standard_normal(n, dtype=np.float32)) - np.float32(0.5)).astype(np.float32))]
SIGMA_SHAPES = [("64 x 4096 per row", 64, 4096, True), ("2^16 per tensor", 1, 1 << 16, False), ("2^20 per tensor", 1, 1 << 20, False),
                ("2^24 per tensor", 1, 1 << 24, False)]
SIGMA_DTYPES = ("float32", "bfloat16")
SIGMA_ULP = {"float32": 2.0 ** -23, "bfloat16": 2.0 ** -8}       # one rounding step of the output's dtype: the last step rounds


def _torch_three_sigma(t, rows, per_row):
    """The reference's ops (olive quant_modules.py:193-197 / :213-218) on the CPU, in the tensor's dtype."""
    t2 = t.reshape(rows, -1) if per_row else t.reshape(1, -1)
    mean, std = t2.mean(dim=-1), t2.std(dim=-1)
    return torch.maximum((mean + 3 * std).abs(), (mean - 3 * std).abs()).float().numpy()


@gpu
def test_three_sigma_against_the_exact_statistic(antq_lib, dev):
    """antq_moments + antq_xmax_3sigma against calib_check.exact_three_sigma.  The bar per dtype: 4 x the worst relative error
    of torch's own mean() / std() composition on the CPU over the same cases (the factor covers the order difference of two
    correct summations, not a cancellation loss), never less than one rounding step of the dtype.
    Measured on the MI355X (profiles/reductions_exactness.md): the kernel returns the yardstick's bits in all 80 cases
    (worst 0 in both dtypes); torch's worst 6.0e-7 (fp32, a constant tensor of 0.1f) / 0 (bf16): bars 2.4e-6 / 2^-8."""
    rows_out = []
    for dtname in SIGMA_DTYPES:
        tdt = DT[dtname][0]
        for sname, rows, K, per_row in SIGMA_SHAPES:
            for dname, make in SIGMA_DISTS:
                rng = np.random.default_rng(len(rows_out) + 1)
                t = torch.from_numpy(make(rng, rows * K)).to(tdt)
                img = t.float().numpy().reshape(rows, K)
                want = exact_three_sigma(img, per_row, dtname).astype(np.float64)
                got = antq_lib.xmax_3sigma(t.to(dev).reshape(rows, K), rows, K, per_row).cpu().numpy().astype(np.float64)
                tor = _torch_three_sigma(t, rows, per_row).astype(np.float64)
                assert np.isfinite(want).all() and (want > 0).all(), (dtname, sname, dname)
                assert np.isfinite(got).all(), (dtname, sname, dname, "the kernel's x_max is not finite", got[~np.isfinite(got)][:4])
                ek = float((np.abs(got - want) / want).max())
                tf = np.isfinite(tor)                 # (torch's float32 sum of 2^16 and more values of 3e38 overflows)
                et = float((np.abs(tor[tf] - want[tf]) / want[tf]).max()) if tf.any() else float("nan")
                rows_out.append((dtname, sname, dname, ek, et, int((~tf).sum())))
                print("THREE_SIGMA | %s | %s | %s | kernel %.3g | torch %.3g | torch non-finite %d" % rows_out[-1], flush=True)
    failures = []
    for dtname in SIGMA_DTYPES:
        mine = [r for r in rows_out if r[0] == dtname]
        worst_torch = max(r[4] for r in mine if not math.isnan(r[4]))
        bar = max(4.0 * worst_torch, SIGMA_ULP[dtname])
        worst = max(mine, key=lambda r: r[3])
        print("THREE_SIGMA BAR | %s | torch worst %.3g | bar %.3g | kernel worst %.3g (%s, %s)" % (dtname, worst_torch, bar, worst[3], worst[1], worst[2]),
              flush=True)
        failures += [(r, bar) for r in mine if not r[3] <= bar]
    assert len(rows_out) == len(SIGMA_DTYPES) * len(SIGMA_SHAPES) * len(SIGMA_DISTS)
    assert not failures, failures
    # one element: the unbiased std is 0 / 0 -- NaN, like torch.std and the yardstick
    for dtname in SIGMA_DTYPES:
        for rows, per_row in ((5, True), (1, False)):
            t = torch.full((rows, 1), 0.75, dtype=DT[dtname][0])
            assert np.isnan(exact_three_sigma(t.float().numpy(), per_row, dtname)).all()
            assert np.isnan(antq_lib.xmax_3sigma(t.to(dev), rows, 1, per_row).cpu().numpy()).all()
