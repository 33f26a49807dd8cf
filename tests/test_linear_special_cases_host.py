"""The inputs of tests/test_gpu_linear_specials.py (tests/linear_special_cases.py) held to their premises with numpy alone: the
finite parts are exact in any order, every class of result occurs where it has meaning, the non-finite rows hold what they
claim in the load unit that padded lanes repeat, and each restated mistake changes at least one compared element."""
import collections

import numpy as np
import pytest

import linear_special_cases as sc

SETS = pytest.mark.parametrize("entry,dtype_name", sc.SETS)


def _unpack(width, codes, K):
    if width == 8:
        return codes
    E = np.empty((codes.shape[0], K), np.uint8)
    E[:, 0::2], E[:, 1::2] = codes & 15, codes >> 4
    return E


@SETS
def test_cases_are_exact_and_cover_what_they_claim(entry, dtype_name):
    e = sc.ENTRIES[entry]
    cases = sc.cases(entry, dtype_name)
    assert cases is sc.cases(entry, dtype_name)                          # the GPU test gets the same arrays
    seen = collections.defaultdict(set)
    worst = 0.0
    for c in cases:
        K, M, N = c["K"], c["M"], c["N"]
        assert c["x"].shape == (M, K) and c["codes"].shape == (N, K * e["width"] // 8) and c["want"].shape == (M, N)
        assert c["alpha"].size == (N if c["per_row"] else 1) and (c["bias"] is None or c["bias"].shape == (N,))
        # the weights are the decoder's rule on the very bytes the GPU test uploads, in this type
        W = sc.weights(e["width"], c["book"], _unpack(e["width"], c["codes"], K), c["alpha"], c["per_row"], dtype_name)
        assert np.array_equal(W, c["W"], equal_nan=True)
        # x and the bias are values of the type, and the finite parts are exact: mass below 2^24 units, no fp32 overflow
        assert np.array_equal(sc._value(c["x_bits"], dtype_name), c["x"], equal_nan=True)
        worst = max(worst, sc.assert_exact(c["x"], W, c["bias"], dtype_name))
        assert not sc.mismatches(sc.expect(c["x"], W, c["bias"], dtype_name), c["want"], dtype_name).any()
        # a row's expectation is that of the row alone: the finite rows among non-finite ones, bit for bit
        for m in range(M) if c["family"] == "inputs" else ():
            alone = sc.expect(c["x"][m:m + 1], W, c["bias"], dtype_name)
            assert np.array_equal(alone[0], c["want"][m]), (sc.label(c), m)
        # the code path: aligned codes take the 16-byte path exactly where the case says so
        wide = K % (32 if e["width"] == 4 else 16) == 0
        assert c["vec"] == (wide and c["offset"] == 0) and (c["offset"] == 0 or c["offset"] == e["off"])
        seen["path"].add((K, c["vec"]))
        seen["M"].add(M)
        seen["NK"].add((N, c["knob"]))
        seen["per_row"].add(c["per_row"])
        seen["bias"].add(c["bias"] is not None)
        seen["book"].add(c["book"])
        seen["family"].add(c["family"])
    assert seen["path"] == set(sc.paths(entry)) and seen["M"] >= set(e["Ms"]) and seen["NK"] == set(e["NK"])
    assert seen["per_row"] == {True, False} and seen["bias"] == {True, False} and seen["book"] == set(sc.BOOKS[e["width"]])
    assert seen["family"] == set(sc.FAMILIES)
    # every M meets every N (and forced tile shape) among the weight and the input cases
    met = {(c["M"], c["N"], c["knob"]) for c in cases if c["family"] != "rounding"}
    if entry in ("linear4", "linear8"):
        assert met >= {(M, N, k) for M in e["Ms"] for N, k in e["NK"]}
    assert {M for M, N, k in met} == set(e["Ms"])
    tails = [p for p in sc.paths(entry) if sc.has_tail(entry, *p)]
    assert {True, False} <= {v for _, v in tails} and any(not sc.has_tail(entry, *p) for p in sc.paths(entry))
    print("%s %s: %d cases, at most %.0f units of mass" % (entry, dtype_name, len(cases), worst))


@SETS
def test_every_class_of_result_occurs(entry, dtype_name):
    """NaN, +Inf and -Inf in the weight and in the input cases of every K; ties in both directions, the overflow threshold and
    zero results from -0 products and a -0.0 bias in the rounding cases.  A result of -0 cannot occur: the accumulators start at
    +0, and (+0) + (-0) = +0."""
    pz = sc.to_bits(np.float64([0.0]), dtype_name)[0]
    tie_dirs, over, zeros, neg_rows = set(), set(), 0, 0
    for path in sc.paths(entry):
        for fam in ("weights", "inputs"):
            v = np.concatenate([sc._value(c["want"], dtype_name).ravel() for c in sc.cases(entry, dtype_name)
                                if (c["K"], c["vec"]) == path and c["family"] == fam])
            assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any() and np.isfinite(v).any(), (path, fam)
    for c in sc.cases(entry, dtype_name):
        v = sc._value(c["want"], dtype_name)
        assert not (np.signbit(v) & (v == 0)).any(), "no sum of these cases is -0"
        if c["family"] != "rounding":
            continue
        assert np.isfinite(c["x"]).all() and np.isfinite(c["W"]).all()
        for m, tag in enumerate(c["tags"]):
            total = float(c["x"][m] @ c["W"][0])                         # exact: asserted by the builder
            r = v[m, 0]
            if tag == "tie":
                assert abs(r - total) == 1.0 and abs(r) % 4 == 0          # half an ulp of 2, to the even neighbour
                tie_dirs.add((np.sign(total), abs(r) > abs(total)))
            elif tag == "overflow":
                assert np.isinf(r) or abs(r) == {"float16": 65504.0, "bfloat16": (2.0 - 2.0 ** -7) * 2.0 ** 127}[dtype_name]
                over.add(r)
            else:
                assert total == 0 and c["want"][m, 0] == pz
                zeros += 1
        assert c["bias"] is None or (c["bias"][0] == 0 and np.signbit(c["bias"][0]))
        neg_rows += int(((c["x"] == 0) & np.signbit(c["x"])).all(1).sum())                    # rows of -0.0 only
    assert zeros and neg_rows
    if dtype_name != "float32":
        assert tie_dirs == {(s, up) for s in (1.0, -1.0) for up in (False, True)}
        assert len(over) == 3 and np.inf in over and -np.inf in over
    print("%s %s: ties %s, overflow results %s, %d planted zeros" % (entry, dtype_name, sorted(tie_dirs), sorted(over), zeros))


@SETS
def test_non_finite_rows_hold_their_plants(entry, dtype_name):
    """Set A: the last load unit of every non-finite row holds non-zero grid values (with the pair rule, in the NaN-scale and
    the overflowing rows, an outlier and its victim, whose value is zero) under non-zero finite x.  Set B: zero-valued codes
    there.  Per-tensor Inf and NaN scales occur.  The non-finite x stand alone in their rows."""
    e = sc.ENTRIES[entry]
    n_rows = collections.Counter()
    one_scale = set()
    used, input_ms = collections.defaultdict(set), collections.defaultdict(set)
    for c in sc.cases(entry, dtype_name):
        if c["family"] == "inputs":
            bad = ~np.isfinite(c["x"])
            assert bad.sum() == len(c["planted"]) >= 1 and (bad.sum(1) <= 1).all() and np.isfinite(c["W"]).all()
            assert c["N"] >= 3
            for m, k, kind in c["planted"]:
                assert np.array_equal(c["x"][m, k], sc.SPECIAL[kind], equal_nan=True)
                assert c["W"][0, k] == 0 and c["W"][1, k] > 0 and c["W"][2, k] < 0
                used[(c["K"], c["vec"])].add((k, kind))
            # every case plants the last row, the first and the rows either side of every row-tile edge it has
            rows = {m for m, k, kind in c["planted"]}
            assert rows >= {0, c["M"] - 1} | {m for m in e["edges"] if m < c["M"]}, (sc.label(c), sorted(rows))
            input_ms[(c["K"], c["vec"])].add(c["M"])
        if c["family"] != "weights":
            continue
        _, g, gmax, nn, ovp = sc.book_of(e["width"], c["book"])
        lu = sc.last_unit(entry, c["K"], c["vec"])
        assert np.isfinite(c["x"]).all() and (c["x"] != 0).all()
        if not c["per_row"]:
            one_scale.add("nan" if np.isnan(c["alpha"][0]) else "inf")
        assert c["special_rows"] and (c["N"] == 1 or not c["per_row"] or len(c["special_rows"]) < c["N"])
        for n in c["special_rows"]:
            a_n = c["alpha"][n if c["per_row"] else 0]
            # (set B at a K of one unit, finite overflowing scale: the zero codes are the whole row)
            assert not np.isfinite(c["W"][n]).all() or (c["code_set"] == "B" and np.isfinite(a_n) and lu.start == 0), (sc.label(c), n)
            # the codes' own values: the decoder's image of the row at a scale of one
            v = sc.weights(e["width"], c["book"], c["E"][n:n + 1], np.float32([gmax]), True, dtype_name)[0, lu]
            if c["code_set"] == "A":
                victims = int((c["E"][n, lu] == sc.code_classes(e["width"], c["book"])["ident"]).sum()) if ovp else 0
                assert (v != 0).sum() == v.size - victims and victims <= 1, (sc.label(c), n)
            else:
                assert (v == 0).sum() >= (v.size + 1) // 2 and ((v == 0).all() or ovp), (sc.label(c), n)
            n_rows[c["code_set"]] += 1
    assert one_scale == {"nan", "inf"} and n_rows["A"] and n_rows["B"]
    # on every path: every M of the entry point has input cases, and every promised (k, kind) is planted -- NaN, +Inf and -Inf
    # at the first and the last k, one of them on both sides of every step of K
    for path in sc.paths(entry):
        step = e["step"][path[1]]
        want_k = {0, path[0] - 1} | {b + d for b in range(step, path[0], step) for d in (-1, 0)}
        assert {k for k, kind in used[path]} == want_k == set(sc.boundary_positions(entry, *path)), path
        assert used[path] >= {(k, kind) for k in (0, path[0] - 1) for kind in ("nan", "+inf", "-inf")}, path
        assert used[path] == set(sc.input_items(entry, *path)) and input_ms[path] == set(e["Ms"]), path
    if e["edges"]:
        assert all(any(m in {r for r, k, kind in c["planted"]} for c in sc.cases(entry, dtype_name) if c["family"] == "inputs")
                   for m in e["edges"])
    print("%s %s: %d non-finite rows with set A, %d with set B" % (entry, dtype_name, n_rows["A"], n_rows["B"]))


@SETS
def test_restated_mistakes_show(entry, dtype_name):
    """(a) padded lanes multiply a zero x with the row's repeated last unit; (b) a non-finite x leaks into the next row of its
    16-row tile; (c) a non-finite scale lands on the neighbouring column; (d) ties round half-up; (e) float16 saturates; (f) the
    bias is added only to a finite sum; (g) a tail-skipping kernel also skips the last valid unit.  Each must change at least
    one compared element of this set where it has meaning; (a) and (g) at every K with a padded tail, (a) nowhere else."""
    e = sc.ENTRIES[entry]
    count = collections.Counter()
    by_path = {m: collections.Counter() for m in "ag"}
    for c in sc.cases(entry, dtype_name):
        x, W, bias, K = c["x"], c["W"], c["bias"], c["K"]
        diff = lambda want: int(sc.mismatches(want, c["want"], dtype_name).sum())
        path = (K, c["vec"])
        lu = sc.last_unit(entry, K, c["vec"])
        tail = sc.has_tail(entry, K, c["vec"])
        by_path["a"][path] += diff(sc.expect(x, W, bias, dtype_name, pad=lu if tail else None))
        if tail:
            by_path["g"][path] += diff(sc.expect(x[:, :lu.start], W[:, :lu.start], bias, dtype_name))
        if c["family"] == "inputs":
            x2 = x.copy()
            for m, k, kind in c["planted"]:
                if m + 1 < c["M"] and (m + 1) % 16:
                    x2[m + 1, k] = x[m, k]
            count["b"] += diff(sc.expect(x2, W, bias, dtype_name))
        if c["family"] == "weights" and c["per_row"] and c["N"] > 1:
            W2 = sc.weights(e["width"], c["book"], c["E"], np.roll(c["alpha"], 1), True, dtype_name)
            count["c"] += diff(sc.expect(x, W2, bias, dtype_name))
        count["d"] += diff(sc.expect(x, W, bias, dtype_name, half_up=True))
        count["e"] += diff(sc.expect(x, W, bias, dtype_name, saturate=True))
        if bias is not None:
            count["f"] += diff(sc.expect(x, W, bias, dtype_name, bias_if_finite=True))
    count["a"], count["g"] = sum(by_path["a"].values()), sum(by_path["g"].values())
    print("%s %s: elements changed by mistake " % (entry, dtype_name) + ", ".join("(%s) %d" % (m, count[m]) for m in "abcdefg"))
    for m in "ag":
        print("    (%s) by (K, 16-byte path): %s" % (m, sorted(by_path[m].items())))
    for path in sc.paths(entry):
        if sc.has_tail(entry, *path):
            assert by_path["a"][path] > 0 and by_path["g"][path] > 0, path
        else:
            assert by_path["a"][path] == 0, path
    assert count["b"] > 0 and count["c"] > 0 and count["f"] > 0
    assert (count["d"] > 0) == (dtype_name != "float32") and (count["e"] > 0) == (dtype_name == "float16")
