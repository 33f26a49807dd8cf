"""The builders of the scratch / output contract tests (scratch_cases.py) held to their premises without a GPU: every case
meets the eligibility rule it claims (and would not one step smaller, where the case sits on a threshold), the patterns read
as what the GPU tests say they are, the yardstick alone places the two tensors of the histogram flag test on either side of
the pair-list capacity, and the five-region sum is what antq_calibrate_workspace_bytes returns.  A failure of
test_gpu_scratch_contracts.py is then the kernels', not the cases'."""
import ctypes
import math
import os

import numpy as np
import pytest

import calib_check
import scratch_cases as sc


def test_slab_layout_and_guard():
    off, total = sc.slab_layout(512 * 7, 1000)
    assert off == sc.GUARD == 4096 and total == 4096 + 1000 + 4096
    assert (512 * 7 + off) % 256 == 0 and (512 * 7 + off) % 16 == 0
    with pytest.raises(AssertionError):
        sc.slab_layout(512 * 7 + 64, 1000)
    # wider than any single partial record: a workgroup's 128 doubles, a ticket partial, a histogram segment's counter
    assert sc.GUARD > sc.WIDEST_RECORD == sc.K_PT_CAND * 8 and sc.GUARD > 16
    assert sc.PATTERNS[0] == 0x00 and set(sc.PATTERNS) == {0x00, 0xFF, 0x7F, "leftover"}


def test_patterns_read_as_nan_huge_and_counters():
    f, d, u = sc.pattern_reads_as(0xFF)
    assert math.isnan(f) and math.isnan(d) and u == 2 ** 32 - 1
    f, d, u = sc.pattern_reads_as(0x7F)
    assert np.isfinite(f) and f > 3e38 and np.isfinite(d) and d > 1e306 and u == 0x7F7F7F7F and u > 2 ** 30
    f, d, u = sc.pattern_reads_as(0x00)
    assert f == 0.0 and d == 0.0 and u == 0
    f, d, u = sc.pattern_reads_as(sc.GUARD_BYTE)
    assert u == 0xC3C3C3C3 and f < 0 and d < 0            # (a guard that leaks into a sum or a counter would show)
    # the flag word of the histogram search: bit 0 set under both poison patterns, i.e. "a segment overflowed"
    assert sc.pattern_reads_as(0xFF)[2] & 1 and sc.pattern_reads_as(0x7F)[2] & 1
    # an output pre-filled with +Inf / 0xFF is above every finite maximum as the unsigned integer an atomicMax compares
    assert np.float32(np.inf).view(np.uint32) > np.float32(3e38).view(np.uint32) and 0xFFFFFFFF > np.float32(np.inf).view(np.uint32)


def test_workspace_layouts_restated():
    assert sc.SEARCH_WS_BYTES == sc.HIST_WS_BYTES == 50602240 and sc.K_WS_SLOTS * sc.K_PT_CAND * 8 == 8 << 20
    assert sc.HIST_FLAGS_OFF == sc.HIST_SLABS + 262144 + 8192 and sc.HIST_SEG_OFF == sc.HIST_FLAGS_OFF + 256
    assert sc.TK_COUNTER_BYTES == (1 + 64) * 32 * 4 <= sc.TK_PARTIAL_OFF
    assert sc.TK_PARTIAL_OFF + 1024 * 16 <= sc.TK_GROUP_OFF and sc.TK_GROUP_OFF + 64 * 16 <= sc.REDUCE_WS_BYTES
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ant_quantization_amd", "csrc")
    for fname, lines in (("antq_k_search.h", ["constexpr int kPtCand = 128;", "constexpr int kWsSlots = 8192;", "constexpr int kMaxTypes = 4;"]),
                         ("antq_k_hist.h", ["constexpr int kHistMaxG = 128;", "constexpr uint32_t kHistSegCap = 1024;"]),
                         ("antq_k_sweep.h", ["constexpr int kSweepMaxCand = 128;"]),
                         ("antq_k_reduce.h", ["constexpr uint32_t kTkPartialOffset = 16384;", "constexpr uint32_t kTkMaxGroups = 64;"])):
        text = open(os.path.join(src, fname)).read()
        for line in lines:
            assert line in text, (fname, line)


def test_every_search_case_takes_the_path_it_claims():
    names = [c["name"] for c in sc.SEARCH_CASES]
    assert len(set(names)) == len(names)
    for c in sc.SEARCH_CASES:
        takes, smaller = sc.eligible(c)
        assert takes, c["name"]
        rows, K, per_row = sc.case_rows(c)
        assert rows * K == c["n"] and (per_row == 0 or rows == 1)
        assert c["n"] % sc.EPL[c["dtype"]] == 0 and c["n"] * len(c["ratios"]) <= 70e6, c["name"]      # (the yardstick's cost)
        # the cases that sit ON a threshold would not take their path one vector smaller
        if c["name"] in ("sorted fp32 4096 forced", "sorted fp32 2^20 default", "sweep fp32 16384 forced", "sweep fp32 2^22 default",
                         "hist bf16 2^19", "hist f16 2^19"):
            assert not smaller, c["name"]
    paths = {(c["path"], c["dtype"]) for c in sc.SEARCH_CASES}
    assert {("direct", "float32"), ("direct", "bfloat16"), ("sorted", "float32"), ("sweep", "float32"), ("hist", "bfloat16"),
            ("hist", "float16")} <= paths
    assert {c["form"] for c in sc.SEARCH_CASES} == {"flat", "folded", "one_row"}
    # the pair-rule histogram cases: 2^20 elements, the default rule's size threshold (the rule also wants 1.5e8 evaluations,
    # which knob 14 = 2 waives for a short candidate list)
    for c in sc.SEARCH_CASES:
        if c["path"] == "hist" and c["ovp"]:
            assert c["n"] == 1 << 20 and c["knobs"][14] == 2 and c["n"] % 2 == 0
    for name, nt in sc.MULTI_CASES:
        c = sc.search_case(name)
        assert sc.eligible(c, ntypes=nt)[0] and c["n"] // sc.EPL[c["dtype"]] >= 64 and nt <= sc.K_MAX_TYPES


def test_the_clamp_case_asks_for_more_workgroups_than_slots():
    c = sc.search_case("direct fp32 clamp binds")
    chunks = c["knobs"][12]
    assert len(c["ratios"]) == chunks == sc.CLAMP_CHUNKS          # one candidate per chunk: blockIdx.y = 0 .. 63
    asked, clamped = sc.direct_blocks(c["dtype"], c["n"], chunks)
    assert asked > clamped == sc.K_WS_SLOTS // chunks == 128 and asked <= 1024, (asked, clamped)
    assert clamped * chunks == sc.K_WS_SLOTS                        # the last partial ends exactly at the end of the 8 MiB
    assert c["n"] // 4 >= 512 and c["n"] >= 1 << 20                 # fp32 rows of >= 512 vectors: 8 vectors per lane and task
    # the small direct cases stay far below the clamp
    for name in ("direct fp32 8192", "direct bf16 8192"):
        s = sc.search_case(name)
        asked, clamped = sc.direct_blocks(s["dtype"], s["n"], 1)
        assert asked == clamped <= 4


def test_yardstick_places_the_flag_tensors_on_either_side(oracle):
    books = [(np.concatenate([oracle.olive_grid(t, 4, True), oracle.olive_outlier_value(4, True)]), oracle.olive_grid(t, 4, True).size,
              float(oracle.olive_grid(t, 4, True).max())) for t in ("int", "flint")]
    cap = sc.segment_capacity_fraction(sc.FLAG_N)
    assert cap == 0.5                                     # 2^19 pair words over 16 x 16 wavefronts of 1024-word segments
    t = sc.flag_tensors()
    for g, n_normal, gmax in books:
        tmin = sc.outlier_threshold_over_gmax(g, n_normal, gmax)
        assert 1.0 < tmin < 2.0, tmin                     # between the largest normal value and the smallest outlier
        x, xm = t["overflow"]
        img = calib_check._round_bf16(x)
        f_over = sc.pair_fraction(img, xm, sc.FLAG_RATIOS, tmin)
        x, xm = t["clean"]
        img = calib_check._round_bf16(x)
        f_clean = sc.pair_fraction(img, xm, sc.FLAG_RATIOS, tmin)
        print("FLAG TENSORS | tmin/gmax %.4f | overflow %.3f | clean %.4f | capacity %.2f" % (tmin, f_over, f_clean, cap))
        assert f_over > sc.HEADER_PAIR_BOUND and f_over > 1.25 * cap, f_over      # every wavefront's segment overflows
        assert f_clean < sc.HEADER_PAIR_BOUND and f_clean < cap / 8, f_clean
        # and the clean tensor does hold victims: the pair rule has work to do (oracle, first candidate)
        alpha = np.float32(xm * sc.FLAG_RATIOS[0])
        _, idx = oracle.forward(img[:1 << 16].reshape(1, -1), np.float32([alpha]), g, gmax, True)
        assert (idx == oracle.IDX_VICTIM).sum() > 10
    # the pair-rule histogram cases of the search table are clean as well
    for c in sc.SEARCH_CASES:
        if c["path"] == "hist" and c["ovp"]:
            x, xm = sc.case_data(c)
            img = calib_check.ROUND_TO[c["dtype"]](x)
            for g, n_normal, gmax in books:
                assert sc.pair_fraction(img, xm, c["ratios"], sc.outlier_threshold_over_gmax(g, n_normal, gmax)) < cap / 8


def test_sum_sizes_cross_the_partial_cap():
    for op in ("moments", "alpha_grad"):
        for dt in sc.EPL:
            small, big = sc.sum_sizes(op, dt)
            assert sc.sum_blocks(op, dt, small) == 1 and sc.sum_blocks(op, dt, big) > sc.PARTIAL_CAP
            assert big % sc.EPL[dt] != 0 and big < 1 << 24          # a ragged tail; integer sums stay exact (2^7 * 2^8 * 2^24 < 2^53)
    assert sc.PARTIAL_CAP * sc.K_PT_CAND * 8 <= sc.SEARCH_WS_BYTES
    n = sc.TICKET_SIZES[-1]
    assert n >= 1024 * 64 * 4 * 4 * 4 and sc.TICKET_SIZES[0] == 1     # 1024 workgroups' worth for abs-max (fp32) and more for the gradient
    for s in sc.TICKET_SETTINGS[1:]:
        blocks, group = s
        assert blocks <= 1024 and group <= 64 and (blocks + group - 1) // group <= 64      # fits the block's layout unclamped


def test_calibrate_workspace_is_the_five_region_sum(antq_lib_host):
    fn = antq_lib_host.antq_calibrate_workspace_bytes
    fn.restype = ctypes.c_size_t
    seen = set()
    for c in sc.CALIB_CASES:
        lb, ub, step = c["rng"]
        want = sc.calibrate_workspace_bytes(c["rows"], c["per_row"], lb, ub, step, c["ntypes"])
        regions = sc.calibrate_regions(c["rows"] if c["per_row"] else 1, sc.calib_ncand(lb, ub, step), c["ntypes"])
        assert len(regions) == 5 and all(b % 256 == 0 and b > 0 for _, b in regions) and want == sum(b for _, b in regions)
        got = fn(ctypes.c_size_t(c["rows"]), ctypes.c_int(c["per_row"]), ctypes.c_int(lb), ctypes.c_int(ub), ctypes.c_int(step),
                 ctypes.c_int(c["ntypes"]))
        assert got == want, (c["name"], got, want)
        seen.add(want)
    assert len(seen) >= 12                                 # the cases do differ in their need
    w = antq_lib_host.antq_search_workspace_bytes
    w.restype = ctypes.c_size_t
    assert w() == sc.SEARCH_WS_BYTES


@pytest.fixture(scope="module")
def antq_lib_host(antq_lib):
    """libantq.so loaded for its host-only size functions (nothing here touches a device)"""
    return antq_lib.lib()


def test_calibrate_cases_cover_the_factors():
    cs = sc.CALIB_CASES
    assert len({c["name"] for c in cs}) == len(cs) == 2 * 3 * 3 * 3 * 3 + 1
    cross = {(c["dtype"], c["per_row"], c["rows"] if c["per_row"] else 0, c["mode"], c["ntypes"], sc.calib_ncand(*c["rng"])) for c in cs[:-1]}
    assert cross == {(dt, pr, rows, m, nt, nc) for dt in ("float32", "bfloat16") for pr, rows in ((1, 3), (1, 257), (0, 0))
                     for m in (sc.XMAX_GIVEN, sc.XMAX_ABSMAX, sc.XMAX_3SIGMA) for nt in (1, 3, 5) for nc in (0, 1, 75)}
    assert {(c["rows"], c["row_len"]) for c in cs if not c["per_row"]} == {(1, 4096), (4, 1024), (1, 1 << 19)}
    assert any(c["ntypes"] > sc.K_MAX_TYPES and c["per_row"] for c in cs) and any(c["ntypes"] > sc.K_MAX_TYPES and not c["per_row"] for c in cs)
    hist = [c for c in cs if sc.xmax_in_hist(c)]
    assert [c["name"] for c in hist] == ["bf16 one scale 2^19 absmax 3 types"] and hist[0]["path"] == "hist"
    assert all(sc.calib_case(n) for n in sc.SMALLEST_CALIB)
    least = min(sc.calibrate_workspace_bytes(c["rows"], c["per_row"], *c["rng"], c["ntypes"]) for c in cs)
    assert all(sc.calibrate_workspace_bytes(c["rows"], c["per_row"], *c["rng"], c["ntypes"]) == least for c in map(sc.calib_case, sc.SMALLEST_CALIB))
    for c in cs:
        x, given = sc.calib_data(c)
        assert x.shape == (c["rows"], c["row_len"]) and (given is not None) == (c["mode"] == sc.XMAX_GIVEN)
        if given is not None:
            assert given.size == (c["rows"] if c["per_row"] else 1) and (given > 0).all()
        n_per = c["row_len"] if c["per_row"] else c["rows"] * c["row_len"]
        # per row: the sorted-row search's entry (128 elements); one scale: below every front path unless the case says hist
        assert (c["per_row"] and n_per >= 128) or c["path"] in ("direct", "hist", "none"), c["name"]
        if c["path"] == "direct":
            assert n_per < 1 << 19
    jobs = [sc.calib_case(n) for n in sc.BATCH_JOBS]
    assert len(jobs) == 6 and len({j["dtype"] for j in jobs}) == 1 and len({(j["rows"], j["row_len"], j["ntypes"], j["rng"]) for j in jobs}) >= 5
    assert all(sorted(o) == list(range(6)) for o in sc.BATCH_ORDERS) and sc.BATCH_ORDERS[0] != sc.BATCH_ORDERS[1]
    needs = [sc.calibrate_workspace_bytes(j["rows"], j["per_row"], *j["rng"], j["ntypes"]) for j in jobs]
    assert max(needs) > min(needs)                         # ONE workspace of the largest need really is shared by smaller jobs
