"""Byte codes (antq_encode8 / antq_decode8 / antq_decode8_batch_*), the parts that need no device: the symbols, the pure-host
blob builder with its refusals and task counts, the same builder on its own under AddressSanitizer / UBSan, the layers
PackedBank takes with and without byte_codes, the checkpoint key sizes -- and the inputs of tests/test_gpu_byte_codes.py held
to their conditions with the CPU oracle alone."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import byte_codes_cases as bc
import encode4_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_PLAN, ERR_ALIGN = 0, -1, -2, -3, -5
F32, BF16, F16 = 0, 1, 2
FLAG_OVP = 1
FAKE = 0x7f0000000000            # the builder only looks at addresses: nothing is dereferenced
SYMBOLS = ("antq_encode8", "antq_decode8", "antq_decode8_batch_capacity", "antq_decode8_batch_build", "antq_decode8_batch")


def _job(antq_lib, rows=4, row_len=64, per_row=1, m=256, n_normal=0, codes=FAKE, out=FAKE + (1 << 20), alpha=FAKE + (2 << 20),
         grid=FAKE + (3 << 20)):
    return antq_lib._DecodeJob(codes, out, alpha, rows, row_len, per_row, 10.0, grid, m, n_normal)


def _build(antq_lib, jobs, dtype=BF16, flags=0, cap=None):
    L = antq_lib.lib()
    arr = (antq_lib._DecodeJob * len(jobs))(*jobs)
    need = L.antq_decode8_batch_capacity(arr, len(jobs), dtype)
    cap = need if cap is None else cap
    buf = np.zeros(max(cap, 1), np.uint8)
    n = L.antq_decode8_batch_build(arr, len(jobs), dtype, ctypes.c_uint(flags), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap))
    return n, need, buf


def _u32(d, at):
    return int(d[at:at + 4].copy().view(np.uint32)[0])


def test_symbols_are_declared_exported_and_bound(antq_lib):
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    names = set(re.findall(r"\b(antq_[a-z_0-9]+)\s*\(", hdr))
    L = ctypes.CDLL(antq_lib.LIB_PATH)
    for n in SYMBOLS:
        assert n in names and hasattr(L, n), n
    assert int(re.search(r"#define ANTQ_ABI_VERSION (\d+)", hdr).group(1)) == 7 == L.antq_abi_version() == antq_lib.ABI_VERSION
    B = antq_lib.lib()
    assert B.antq_decode8_batch_capacity.restype is ctypes.c_size_t
    for n in set(SYMBOLS) - {"antq_decode8_batch_capacity"}:
        assert getattr(B, n).restype is ctypes.c_int, n
    for n in ("encode8", "decode8"):
        assert callable(getattr(antq_lib, n))
    import inspect
    assert str(inspect.signature(antq_lib.encode8)) == str(inspect.signature(antq_lib.encode4))
    assert str(inspect.signature(antq_lib.decode8)) == str(inspect.signature(antq_lib.decode4))
    assert "width" in inspect.signature(antq_lib.DecodeBatch.__init__).parameters


def test_entry_points_refuse_before_touching_hip(antq_lib):
    """antq_encode8 / antq_decode8 / antq_decode8_batch: argument errors on a box without a GPU (made-up addresses)."""
    L = antq_lib.lib()
    vp, sz, ci, cf, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint
    plan = antq_lib.plan_for(np.arange(256, dtype=np.float32))
    plan257 = antq_lib.plan_for(np.arange(257, dtype=np.float32))
    for fn in (L.antq_encode8, L.antq_decode8):
        call = lambda a=FAKE, b=FAKE + 4096, rows=4, rl=64, al=FAKE + 8192, p=plan, pd=FAKE + 16384, nn=0, fl=0, dt=BF16: fn(   # noqa: E731
            vp(a), vp(b), sz(rows), sz(rl), vp(al), ci(1), cf(10.0), p.host_ptr() if p is not None else None, vp(pd), ci(nn), cu(fl), ci(dt), None)
        assert call(a=0) == ERR_ARG and call(b=0) == ERR_ARG and call(al=0) == ERR_ARG and call(p=None) == ERR_ARG and call(pd=0) == ERR_ARG
        assert call(rows=0) == ERR_ARG and call(rl=0) == ERR_ARG
        assert call(fl=2) == ERR_ARG and call(fl=5) == ERR_ARG
        assert call(rl=6) == ERR_UNSUPPORTED and call(rl=147) == ERR_UNSUPPORTED
        assert call(dt=3) == ERR_UNSUPPORTED
        assert call(p=plan257) == ERR_UNSUPPORTED
        assert call(fl=FLAG_OVP, nn=0) == ERR_UNSUPPORTED and call(fl=FLAG_OVP, nn=256) == ERR_UNSUPPORTED
    # an output / input that is not aligned to its element
    assert L.antq_decode8(vp(FAKE), vp(FAKE + 4097), sz(4), sz(64), vp(FAKE + 8192), ci(1), cf(10.0), plan.host_ptr(), vp(FAKE + 16384),
                          ci(0), cu(0), ci(BF16), None) == ERR_ALIGN
    assert L.antq_encode8(vp(FAKE + 1), vp(FAKE + 4096), sz(4), sz(64), vp(FAKE + 8192), ci(1), cf(10.0), plan.host_ptr(), vp(FAKE + 16384),
                          ci(0), cu(0), ci(BF16), None) == ERR_ALIGN
    buf = np.zeros(4096, np.uint8)
    assert L.antq_decode8_batch(None, None, None) == ERR_ARG
    assert L.antq_decode8_batch(buf.ctypes.data_as(vp), buf.ctypes.data_as(vp), None) == ERR_PLAN      # no magic
    n, _, blob4 = (lambda arr: (L.antq_decode4_batch_build(arr, 1, BF16, cu(0), buf.ctypes.data_as(vp), sz(4096)), 0, buf))(
        (antq_lib._DecodeJob * 1)(_job(antq_lib, m=16)))
    assert n > 0 and L.antq_decode8_batch(blob4.ctypes.data_as(vp), blob4.ctypes.data_as(vp), None) == ERR_PLAN   # a 4-bit blob is not a byte blob


def test_builder_refusals(antq_lib):
    L = antq_lib.lib()
    ok = _job(antq_lib)
    assert _build(antq_lib, [ok])[0] > 0
    assert _build(antq_lib, [ok, _job(antq_lib, row_len=6)])[0] == ERR_UNSUPPORTED               # row_len % 4 != 0
    assert _build(antq_lib, [_job(antq_lib, row_len=147)])[0] == ERR_UNSUPPORTED
    assert _build(antq_lib, [_job(antq_lib, row_len=20)])[0] > 0
    assert _build(antq_lib, [_job(antq_lib, m=257)])[0] == ERR_UNSUPPORTED                        # more than 256 plain values
    assert _build(antq_lib, [_job(antq_lib, m=1)])[0] > 0
    assert _build(antq_lib, [_job(antq_lib, m=0)])[0] == ERR_ARG
    assert _build(antq_lib, [_job(antq_lib, m=509, n_normal=255)], flags=FLAG_OVP)[0] > 0           # OliVe 8-bit signed: 255 + 254
    assert _build(antq_lib, [_job(antq_lib, m=510, n_normal=255)], flags=FLAG_OVP)[0] > 0
    assert _build(antq_lib, [_job(antq_lib, m=31, n_normal=16)], flags=FLAG_OVP)[0] > 0             # OliVe 4-bit unsigned: 16 + 15
    assert _build(antq_lib, [_job(antq_lib, m=511, n_normal=256)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED   # no code left for the identifier
    assert _build(antq_lib, [_job(antq_lib, m=511, n_normal=255)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED   # 256 outliers
    assert _build(antq_lib, [_job(antq_lib, m=20, n_normal=0)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED
    assert _build(antq_lib, [_job(antq_lib, m=20, n_normal=21)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED
    assert _build(antq_lib, [_job(antq_lib, m=300, n_normal=0)])[0] == ERR_UNSUPPORTED               # n_normal is read with the pair rule only
    assert _build(antq_lib, [_job(antq_lib)], dtype=3)[0] == ERR_UNSUPPORTED                        # float64
    assert _build(antq_lib, [ok], flags=2)[0] == ERR_ARG and _build(antq_lib, [ok], flags=FLAG_OVP | 4)[0] == ERR_ARG
    assert _build(antq_lib, [_job(antq_lib, rows=0)])[0] == ERR_ARG and _build(antq_lib, [_job(antq_lib, row_len=0)])[0] == ERR_ARG
    for kw in ("codes", "out", "alpha", "grid"):
        assert _build(antq_lib, [ok, _job(antq_lib, **{kw: 0})])[0] == ERR_ARG, kw
    buf = np.zeros(4096, np.uint8)
    arr = (antq_lib._DecodeJob * 1)(ok)
    vp = ctypes.c_void_p
    assert L.antq_decode8_batch_build(None, 1, BF16, ctypes.c_uint(0), buf.ctypes.data_as(vp), ctypes.c_size_t(4096)) == ERR_ARG
    assert L.antq_decode8_batch_build(arr, 1, BF16, ctypes.c_uint(0), None, ctypes.c_size_t(4096)) == ERR_ARG
    assert L.antq_decode8_batch_build(arr, 0, BF16, ctypes.c_uint(0), buf.ctypes.data_as(vp), ctypes.c_size_t(4096)) == ERR_ARG
    assert L.antq_decode8_batch_capacity(None, 1, BF16) == 0
    assert _build(antq_lib, [_job(antq_lib, out=FAKE + (1 << 20) + 1)])[0] == ERR_ALIGN
    assert _build(antq_lib, [_job(antq_lib, out=FAKE + (1 << 20) + 2)], dtype=F32)[0] == ERR_ALIGN
    n, need, _ = _build(antq_lib, [ok, _job(antq_lib, 257, 4100)])
    assert 0 < n <= need
    assert _build(antq_lib, [ok, _job(antq_lib, 257, 4100)], cap=n - 1)[0] == ERR_PLAN and _build(antq_lib, [ok], cap=0)[0] == ERR_PLAN


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_builder_task_counts_kinds_and_map(antq_lib, dtype):
    """Rows of 4, 252, 256, 260 and both sides of every task size: 128 vectors (row tasks from there), 64 u vectors per row
    task (u = 2, 3, 4), 256 vectors / 256 quads per task of the per-lane kinds; the unaligned kinds."""
    epl = 4 if dtype == F32 else 8
    lens = [4, 12, 20, 60, 64, 252, 256, 260, 1024, 4100] + [v * epl for v in (127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513)]
    jobs, want = [], []
    for rows in (1, 3, 257):
        for rl in lens:
            for per_row, codes, out in ((1, FAKE, FAKE + (1 << 20)), (0, FAKE, FAKE + (1 << 20)), (1, FAKE + 1 + rl % 3, FAKE + (1 << 20)),
                                        (1, FAKE, FAKE + (1 << 20) + epl), (0, FAKE + 2, FAKE + (1 << 20))):
                jobs.append(_job(antq_lib, rows, rl, per_row, codes=codes, out=out))
                n = rows * rl
                r, k = (rows, rl) if per_row else (1, n)
                if codes % 4 or out % 16 or k % epl:
                    want.append((2, -(-(n // 4) // 256), k // 4))
                elif k // epl >= 128:
                    want.append((0, None, k // epl))
                else:
                    want.append((1, -(-(n // epl) // 256), k // epl))
    for units in (255, 256, 257, 511, 512, 513):
        jobs += [_job(antq_lib, units, epl), _job(antq_lib, units, 4, codes=FAKE + 2)]
        want += [(1, -(-units // 256), 1), (2, -(-units // 256), 1)]
    n1, need, b1 = _build(antq_lib, jobs, dtype)
    n2, _, b2 = _build(antq_lib, jobs, dtype)
    assert 0 < n1 == n2 <= need and np.array_equal(b1[:n1], b2[:n2])
    h = b1[:32].view(np.uint32)
    assert int(h[0]) == 0x38444E41 and int(h[1]) == len(jobs) and int(h[2]) == dtype and int(h[5]) == n1
    descs = b1[32:32 + 88 * len(jobs)].reshape(len(jobs), 88)
    tasks = np.array([_u32(d, 40) for d in descs])
    first = np.array([_u32(d, 52) for d in descs])
    blk_map = b1[int(h[4]):n1].view(np.uint32)
    assert blk_map.size == int(h[6]) == int(((tasks + 3) // 4).sum())
    assert np.array_equal(blk_map, np.repeat(np.arange(len(jobs), dtype=np.uint32), (tasks + 3) // 4))
    assert np.array_equal(first, np.concatenate([[0], np.cumsum((tasks + 3) // 4)[:-1]]))
    kinds = set()
    for J, d, (kind, t, vpr) in zip(jobs, descs, want):
        tag = (J.rows, J.row_len, J.alpha_per_row, dtype)
        assert _u32(d, 56) == kind and _u32(d, 44) == vpr, tag
        if kind == 0:
            u, tpr = _u32(d, 60), _u32(d, 48)
            rows = J.rows if J.alpha_per_row else 1
            assert u in (2, 3, 4) and tpr == -(-vpr // (64 * u)) and _u32(d, 40) == rows * tpr, tag
            # no other u leaves fewer idle lanes
            assert all(tpr * u <= -(-vpr // (64 * v)) * v for v in (2, 3, 4)), tag
        else:
            assert _u32(d, 40) == t, tag
        kinds.add(kind)
    assert kinds == {0, 1, 2}
    if dtype != F32:       # a 16-bit row of 4 mod 8 elements has no whole vectors: element-granular although everything is aligned
        d = descs[[i for i, J in enumerate(jobs) if J.row_len == 20 and J.alpha_per_row and J.codes_dev == FAKE and J.out_dev == FAKE + (1 << 20)][0]]
        assert _u32(d, 56) == 2


def test_builder_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cabi/decbatch8_check.cpp: the header-only builder in a stand-alone program (its own main, no library, no Python),
    compiled here with -fsanitize=address,undefined, fed the refusals and the edge jobs into exact-size heap buffers."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "decbatch8_check")
    src = os.path.join(ROOT, "tests", "cabi", "decbatch8_check.cpp")
    # (the sanitizer runtimes are linked into the program itself: it needs nothing of the environment it starts in)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-o", exe, src], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests' inputs, by the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------
def test_books_fit_a_byte_and_not_a_nibble():
    for name in bc.BOOK_NAMES:
        _, g, gmax, nn, ovp = bc.book(name)
        assert bc.book_fits(g, nn, ovp) and g.dtype == np.float32 and gmax > 0, name
        assert (nn > 15 or g.size - nn > 15) if ovp else g.size > 16, name          # the 4-bit codec refuses every one of them
        assert ovp == (name in bc.OLIVE_NAMES)
    assert bc.book("olive_int_b8")[1].size == 509 and bc.book("olive_u4")[1].size == 31 and bc.book("int_b8_s")[1].size == 256
    for name in ("ladder_plain", "ladder_pairs"):
        g = bc.book(name)[1]
        assert 100 <= g.size - bc.book(name)[3] <= 256 and not np.array_equal(g, np.sort(g))      # arbitrary: not in sorted order


@pytest.mark.parametrize("name", bc.BOOK_NAMES)
def test_threshold_windows_straddle_their_thresholds(oracle, name):
    _, g, gmax, nn, ovp = bc.book(name)
    for rl in bc.THRESHOLD_ROW_LENS:
        case = bc.threshold_input(name, rl)
        good, total = ec.windows_straddle(oracle, case, g, gmax)
        assert good == total > 0, (name, rl, good, total)
        assert case["x"].shape[1] == rl


@pytest.mark.parametrize("name", bc.OLIVE_NAMES)
def test_every_pair_form_is_present(oracle, name):
    _, g, gmax, nn, ovp = bc.book(name)
    case = bc.pair_input(name)
    assert ec.pair_forms_present(oracle, case, g, gmax, nn) == {(f, p) for f in range(4) for p in range(4)}
    # the byte codes of those pairs: a victim is 255, its partner an index into the outlier list
    want = bc.oracle_codes(oracle, case["x"], case["alpha"], bc.book(name)).reshape(-1, 2)
    with np.errstate(all="ignore"):
        _, bare = oracle.forward(case["x"], case["alpha"], g, gmax, False)
    out = bare.reshape(-1, 2) >= nn
    assert ((want == bc.IDENT).sum(1) == out.any(1)).all() and (want[out.any(1)].min(1) < g.size - nn).all()


@pytest.mark.parametrize("dtype_name", bc.DTYPES)
@pytest.mark.parametrize("name", bc.BOOK_NAMES)
def test_round_trip_inputs_decode_to_the_oracle_output(oracle, name, dtype_name):
    """For every round-trip input of the GPU test: inside the stated restriction, and fl((g[idx] + 0) * s) -- rounded to the type --
    equals the oracle's fake-quant output in every element, 0 exceptions."""
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    n = 0
    for rows in bc.ROW_COUNTS:
        for rl in bc.ROW_LENS:
            _, xf, alpha = bc.round_trip_input(name, dtype_name, rows, rl, oracle)
            assert bc.round_trip_ok(xf, alpha, bk), (name, dtype_name, rows, rl)
            with np.errstate(all="ignore"):
                ref, ridx = oracle.forward(xf, alpha, g, gmax, ovp)
            assert (ridx != oracle.IDX_NONE).all()
            want = bc.to_bits(oracle, ref, dtype_name)
            got = bc.decoded_from_indices(oracle, ridx, alpha, bk, dtype_name)
            bad = int((got != want).sum())
            assert bad == 0, (name, dtype_name, rows, rl, "%d of %d differ" % (bad, got.size))
            # the same through the codes and the decoder's rule (what the GPU has to reproduce)
            codes = bc.codes_want(oracle, ridx, nn, ovp, ec.zero_code(g, nn, ovp))
            assert codes.min() >= 0 and codes.max() <= 255
            assert np.array_equal(bc.decode_ref(oracle, codes, alpha, bk, rows, rl, dtype_name), want)
            n += got.size
    assert n == sum(bc.ROW_LENS) * sum(bc.ROW_COUNTS)


# ---------------------------------------------------------------------------------------------------------------------------
# PackedBank: which layers, which width
# ---------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _calibrated_like(q, tree, bits=4, signed=True):
    """The state a calibration leaves on a weight quantiser, written by hand (the searches need the GPU)."""
    import torch
    from ant_quantization_amd import grids
    q.is_signed = signed
    q.bit.data = torch.tensor(bits)
    q._hm_known("bit", bits)
    if tree == "ant":
        q.mode = "int" if bits > 6 else "flint"
        q._install_grid(grids.ant_grid(q.mode, bits, signed))
    else:
        q.mode = "flint"
        q._install(grids.olive_flint(bits, signed), grids.olive_outliers(bits, signed))
    q.has_inited_quant_para.data = torch.ones_like(q.has_inited_quant_para)
    q._hm_known("has_inited_quant_para", 1.0)
    q._steady = True


class _Resident:
    """A weight as _width sees one that lives on the GPU (it only asks where the tensor is, never what it holds)."""

    def __init__(self, w):
        self._w = w
        self.is_cuda = True

    def __getattr__(self, k):
        return getattr(self._w, k)


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_layers_packed_with_and_without_the_option(antq_lib, tree):
    import torch.nn as nn
    from ant_quantization_amd import packed
    qmod = importlib.import_module("ant_quantization_amd.%s.quant_model" % tree)
    qutil = importlib.import_module("ant_quantization_amd.%s.quant_utils" % tree)
    qutil.set_quantizer(_args(mode="flint", wbit=4, abit=4))
    net = nn.Sequential(nn.Linear(64, 48), nn.ReLU(), nn.Linear(48, 64), nn.Linear(64, 20), nn.Linear(20, 16), nn.Linear(16, 8),
                        nn.Linear(8, 8), nn.Linear(147, 8), nn.Linear(8, 8), nn.Linear(8, 8), nn.Linear(32, 8))
    model = qmod.quantize_model(net)
    qutil.enable_quantization(model)
    layers = [m for m in model if hasattr(m, "quant_weight")]
    for m in layers:
        _calibrated_like(m.quant_weight, tree)
    _calibrated_like(layers[4].quant_weight, tree, bits=8)
    _calibrated_like(layers[5].quant_weight, tree, signed=False)
    _calibrated_like(layers[9].quant_weight, tree, bits=6)
    layers[7].quant_weight.mode = "outlier"
    W = packed.PackedBank._width
    why = packed.PackedBank._unsuitable
    host = "weight not resident / not contiguous"
    res = lambda m: _Resident(m.weight)      # noqa: E731
    # without the option: today's answers, to the letter
    assert why(layers[0].quant_weight, layers[0].weight) == host and W(layers[0].quant_weight, res(layers[0])) == (4, None)
    assert why(layers[3].quant_weight, layers[3].weight) == "row length 20 is not a multiple of 8"
    assert re.match(r"(codebook of 256 values \(the 4-bit codec holds 16\)|\d+ (normal|outlier) values)", why(layers[4].quant_weight, layers[4].weight))
    assert why(layers[6].quant_weight, layers[6].weight) == "row length 147 is not a multiple of 8"
    for m in layers:
        assert W(m.quant_weight, m.weight) == (None, why(m.quant_weight, m.weight)) and W(m.quant_weight, m.weight, byte_codes=False)[0] is None
    # with it: 4-bit stays 4-bit, int-8 / 6-bit / row length 20 become width 8
    assert W(layers[0].quant_weight, res(layers[0]), byte_codes=True) == (4, None)
    assert W(layers[1].quant_weight, res(layers[1]), byte_codes=True) == (4, None)
    assert W(layers[3].quant_weight, res(layers[3]), byte_codes=True) == (8, None)          # row length 20
    assert W(layers[4].quant_weight, res(layers[4]), byte_codes=True) == (8, None)          # 8 bit
    assert W(layers[9].quant_weight, res(layers[9]), byte_codes=True) == (8, None)          # 6 bit
    assert W(layers[5].quant_weight, res(layers[5]), byte_codes=True) == ((8 if tree == "olive" else 4), None)   # OliVe's unsigned 16 + 15
    assert why(layers[3].quant_weight, layers[3].weight, byte_codes=True) == host            # where the weight lives comes last
    # what stays skipped, with reasons worded for the byte codec
    assert W(layers[6].quant_weight, res(layers[6]), byte_codes=True) == (None, "row length 147 is not a multiple of 4")
    assert W(layers[7].quant_weight, res(layers[7]), byte_codes=True) == (None, "mode outlier")
    assert W(layers[8].quant_weight, _Resident(model[9].double().weight), byte_codes=True) == (None, "dtype torch.float64")
    # stored codes name their width: a 4-bit layer takes byte codes too, an 8-bit layer no nibbles
    assert W(layers[0].quant_weight, res(layers[0]), byte_codes=True, only=8) == (8, None)
    assert W(layers[4].quant_weight, res(layers[4]), only=4)[0] is None
    with pytest.raises(antq_lib.AntqError):
        packed.PackedBank(model, byte_codes=True)          # nothing resident to pack on the host: an error, not a fall-back


def test_packed_keys_sizes():
    import torch
    import torch.nn as nn
    from ant_quantization_amd import packed
    net = nn.Sequential(nn.Linear(64, 48), nn.Linear(48, 20))
    sd = net.state_dict()
    codes = {"0": torch.zeros(64 * 48 // 2, dtype=torch.uint8), "1": torch.zeros(48 * 20, dtype=torch.uint8)}
    psd = packed._packed_keys(sd, codes)
    assert set(psd) == (set(sd) - {"0.weight", "1.weight"}) | {"0.quant_weight.codes", "1.quant_weight.codes"}
    assert psd["0.quant_weight.codes"].numel() * 2 == net[0].weight.numel()          # 4-bit layer: numel / 2 bytes
    assert psd["1.quant_weight.codes"].numel() == net[1].weight.numel()              # byte-coded layer: numel bytes
    assert all(v.dtype == torch.uint8 for k, v in psd.items() if k.endswith("codes"))
