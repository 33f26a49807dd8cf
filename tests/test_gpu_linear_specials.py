"""Non-finite weights, inputs and biases, the padded tail of K and the edges of the one rounding, through the five packed linears
on the GPU: antq_linear4, antq_linear8, antq_linear4_mm, antq_linear8_mm and antq_linear4_gemm against the cases and the
order-independent expectation of linear_special_cases.py (which test_linear_special_cases_host.py holds to their premises).

What is planted: per-row scales of +Inf, NaN, -Inf and (float16) a finite one at which the weights overflow, on some output
rows between ordinary ones, with the row's last load unit -- the one a lane past the end of K repeats with a zero x -- holding
non-zero values, or zero-valued codes; one +Inf and one NaN scale per tensor; NaN, +Inf and -Inf at single k of single rows of
x, on both sides of every step of K and in the rows either side of a row tile; NaN, Inf and -0.0 in the bias; exact sums on
round-half-even ties, on the float16 and bfloat16 overflow thresholds and on zero.  Every K runs on the code path it takes and,
with the codes moved off a 16-byte boundary, on the narrow one; the forced tile shapes (antq_debug_set keys 22 and 23) run too.
NaN is compared by class, everything else by bits, and y sits between guard words that must stay as they were."""
import collections
import time

import numpy as np
import pytest

import linear_special_cases as sc
from test_gpu_linear4 import GUARD, _bits, _tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def knobs(antq_lib):
    """set(key, value): force a tile shape for the calling thread's later launches; both rules are restored afterwards"""
    knob = antq_lib.lib().antq_debug_set
    yield knob
    knob(22, 0)
    knob(23, 0)


def _upload(c, dev):
    import torch
    e = sc.ENTRIES[c["entry"]]
    flat = torch.from_numpy(np.ascontiguousarray(c["codes"]).reshape(-1)).to(dev)
    codes = flat
    if c["offset"]:                                     # off a 16-byte boundary: the narrow code path at every K
        buf = torch.empty(flat.numel() + 16, dtype=torch.uint8, device=dev)
        buf[c["offset"]:c["offset"] + flat.numel()] = flat
        codes = buf[c["offset"]:c["offset"] + flat.numel()]
    assert codes.data_ptr() % 16 == c["offset"]
    x = _tensor(c["x_bits"], c["dtype"], dev)
    bias = None if c["bias"] is None else _tensor(c["bias_bits"], c["dtype"], dev)
    return flat, codes, x, bias, torch.from_numpy(c["alpha"]).to(dev)


@pytest.mark.parametrize("entry,dtype_name", sc.SETS)
def test_special_values(antq_lib, dev, knobs, entry, dtype_name):
    """Every case of the set in one queue of launches and one synchronisation.  For the weight cases the decoder's own image of
    the codes is held to the numpy rule first, NaN and Inf scales included: the linear then has to return what that image and
    IEEE arithmetic give."""
    import torch
    dt = getattr(torch, dtype_name)
    e = sc.ENTRIES[entry]
    fn = getattr(antq_lib, entry)
    decode = antq_lib.decode4 if e["width"] == 4 else antq_lib.decode8
    guard = _bits(torch.full((1,), 3.0, dtype=dt))[0]
    t0 = time.time()
    runs = []
    for c in sc.cases(entry, dtype_name):
        _, g, gmax, nn, ovp = sc.book_of(e["width"], c["book"])
        plan = antq_lib.plan_for(g)
        M, N, K = c["M"], c["N"], c["K"]
        flat, codes, x, bias, a = _upload(c, dev)
        image = None
        if c["family"] == "weights":
            rows, row_len = (N, K) if c["per_row"] else (1, N * K)
            image = decode(flat, a, plan, gmax, rows, row_len, c["per_row"], dt, n_normal=nn, ovp=ovp)
        full = torch.full((M * N + 2 * GUARD,), 3.0, dtype=dt, device=dev)
        if e["knob"] is not None:
            knobs(e["knob"], c["knob"])
        fn(codes, x, a, plan.grid_dev(dev), gmax, N, K, c["per_row"], bias=bias, n_normal=nn, ovp=ovp, out=full[GUARD:GUARD + M * N])
        runs.append((c, full, image, (flat, codes, x, bias, a)))
    torch.cuda.synchronize()
    t1 = time.time()
    failed = collections.defaultdict(lambda: [0, 0, None])
    for c, full, image, _ in runs:
        M, N = c["M"], c["N"]
        if image is not None:
            assert np.array_equal(sc._value(_bits(image).reshape(N, c["K"]), dtype_name), c["W"], equal_nan=True), (sc.label(c), "the decoder's image")
        b = _bits(full)
        assert (b[:GUARD] == guard).all() and (b[GUARD + M * N:] == guard).all(), (sc.label(c), "guard words")
        bad = sc.mismatches(b[GUARD:GUARD + M * N].reshape(M, N), c["want"], dtype_name)
        if bad.any():
            f = failed[(c["K"], "16-byte" if c["vec"] else "narrow", c["family"])]
            f[0] += 1
            f[1] += int(bad.sum())
            if f[2] is None:
                m, n = np.argwhere(bad)[0]
                f[2] = "%s: y[%d, %d] = %r, expected %r" % (sc.label(c), m, n, sc._value(b[GUARD:GUARD + M * N].reshape(M, N), dtype_name)[m, n],
                                                            sc._value(c["want"], dtype_name)[m, n])
    print("%s %s: %d cases, %.2f s to queue and run, %.2f s to compare; %d failed" % (
        entry, dtype_name, len(runs), t1 - t0, time.time() - t1, sum(f[0] for f in failed.values())))
    for key in sorted(failed):
        print("    K = %d, %s path, %s: %d cases, %d elements; first: %s" % (key + tuple(failed[key])))
    assert not failed, "%d cases differ from the expectation (by K, code path and family: %s)" % (
        sum(f[0] for f in failed.values()), {k: v[0] for k, v in sorted(failed.items())})
