"""Packed 4-bit weights, the parts that need no device: the pure-host builder of the batched decoder's descriptor blob
(antq_decode4_batch_capacity / antq_decode4_batch_build, include/antq.h), the exports, the key layout of a packed checkpoint
and the reasons a layer stays float (ant_quantization_amd/packed.py).  The launches: tests/test_gpu_packed.py."""
import ctypes
import importlib
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_PLAN, ERR_ALIGN = 0, -1, -2, -3, -5
F32, BF16, F16 = 0, 1, 2
FLAG_OVP = 1
FAKE = 0x7f0000000000            # the builder only looks at addresses: nothing is dereferenced


def _job(antq_lib, rows=4, row_len=64, per_row=1, m=16, n_normal=0, codes=FAKE, out=FAKE + (1 << 20), alpha=FAKE + (2 << 20),
         grid=FAKE + (3 << 20)):
    return antq_lib._DecodeJob(codes, out, alpha, rows, row_len, per_row, 10.0, grid, m, n_normal)


def _build(antq_lib, jobs, dtype=BF16, flags=0, cap=None):
    L = antq_lib.lib()
    arr = (antq_lib._DecodeJob * len(jobs))(*jobs)
    need = L.antq_decode4_batch_capacity(arr, len(jobs), dtype)
    cap = need if cap is None else cap
    buf = np.zeros(max(cap, 1), np.uint8)
    n = L.antq_decode4_batch_build(arr, len(jobs), dtype, ctypes.c_uint(flags), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(cap))
    return n, need, buf


def test_decode_batch_symbols_are_declared_and_exported(antq_lib):
    hdr = open(os.path.join(ROOT, "include", "antq.h")).read()
    names = set(re.findall(r"\b(antq_[a-z_0-9]+)\s*\(", hdr))
    L = ctypes.CDLL(antq_lib.LIB_PATH)
    for n in ("antq_decode4_batch_capacity", "antq_decode4_batch_build", "antq_decode4_batch"):
        assert n in names and hasattr(L, n), n
    assert int(re.search(r"#define ANTQ_ABI_VERSION (\d+)", hdr).group(1)) == 7 == L.antq_abi_version()
    # the binding's struct is the header's
    body = re.search(r"typedef struct antq_decode_job \{(.*?)\} antq_decode_job;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in re.sub(r"^.*?([\w*]+\s*,.*|[\w*]+)$", r"\1", decl.strip()).split(",")]
    assert [f.lstrip("*") for f in fields] == [n for n, _ in antq_lib._DecodeJob._fields_]


def test_builder_sizes_and_is_stable(antq_lib):
    shapes = [(1, 8), (3, 8), (5, 24), (64, 768), (2, 1032), (7, 4104), (1, 65544), (9, 1024)]
    for dtype in (F32, BF16, F16):
        jobs = [_job(antq_lib, r, k, per_row=int((r, k) != (9, 1024))) for r, k in shapes]
        jobs += [_job(antq_lib, 2, 64, codes=FAKE + 1), _job(antq_lib, 2, 64, out=FAKE + (1 << 20) + 4)]      # element-granular
        n1, need, b1 = _build(antq_lib, jobs, dtype)
        n2, _, b2 = _build(antq_lib, jobs, dtype)
        assert 0 < n1 == n2 <= need and np.array_equal(b1[:n1], b2[:n2])
        h = b1[:32].view(np.uint32)
        assert int(h[1]) == len(jobs) and int(h[2]) == dtype and int(h[5]) == n1
        descs = b1[32:32 + 88 * len(jobs)].reshape(len(jobs), 88)
        tasks = descs[:, 40:44].copy().view(np.uint32).reshape(-1)
        first = descs[:, 52:56].copy().view(np.uint32).reshape(-1)
        blk_map = b1[int(h[4]):n1].view(np.uint32)
        assert blk_map.size == int(h[6]) == int(((tasks + 3) // 4).sum())
        # every map entry names its job, in order; a job's entries cover its tasks and nothing else
        want = np.repeat(np.arange(len(jobs), dtype=np.uint32), (tasks + 3) // 4)
        assert np.array_equal(blk_map, want) and np.array_equal(first, np.concatenate([[0], np.cumsum((tasks + 3) // 4)[:-1]]))
        # tasks cover every output vector / octet once: rows x ceil(vpr / (64 u)) for rows of >= 128 vectors, else flat
        epl = 4 if dtype == F32 else 8
        for (r, k), t, d in zip(shapes, tasks, descs):
            kind, u = int(d[56:60].copy().view(np.uint32)[0]), int(d[60:64].copy().view(np.uint32)[0])
            rows, rl = (r, k) if (r, k) != (9, 1024) else (1, r * k)
            vpr = rl // epl
            if vpr >= 128:
                assert kind == 0 and u in (2, 3, 4) and t == rows * -(-vpr // (64 * u)), (r, k, dtype)
            else:
                assert kind == 1 and t == -(-(r * k // epl) // 256), (r, k, dtype)
        assert [int(d[56:60].copy().view(np.uint32)[0]) for d in descs[-2:]] == [2, 2]
        # a capacity of 0 or one byte short: refused, nothing launched can come of it
        assert _build(antq_lib, jobs, dtype, cap=0)[0] == ERR_PLAN
        assert _build(antq_lib, jobs, dtype, cap=n1 - 1)[0] == ERR_PLAN


def test_builder_refusals(antq_lib):
    L = antq_lib.lib()
    ok = _job(antq_lib)
    assert _build(antq_lib, [ok])[0] > 0
    # what launch_codec refuses (antq_k_codec.h), reported by the builder
    assert _build(antq_lib, [ok, _job(antq_lib, row_len=12)])[0] == ERR_UNSUPPORTED            # row_len % 8 != 0
    assert _build(antq_lib, [_job(antq_lib, m=17)])[0] == ERR_UNSUPPORTED                        # more than 16 plain values
    assert _build(antq_lib, [_job(antq_lib, m=16)])[0] > 0
    assert _build(antq_lib, [_job(antq_lib, m=29, n_normal=15)], flags=FLAG_OVP)[0] > 0          # OliVe 4-bit signed: 15 + 14
    assert _build(antq_lib, [_job(antq_lib, m=30, n_normal=16)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED   # no code left for the identifier
    assert _build(antq_lib, [_job(antq_lib, m=20, n_normal=0)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED
    assert _build(antq_lib, [_job(antq_lib, m=31, n_normal=15)], flags=FLAG_OVP)[0] == ERR_UNSUPPORTED   # 16 outliers
    assert _build(antq_lib, [_job(antq_lib)], dtype=3)[0] == ERR_UNSUPPORTED                     # float64
    # null pointers
    for kw in ("codes", "out", "alpha", "grid"):
        assert _build(antq_lib, [ok, _job(antq_lib, **{kw: 0})])[0] == ERR_ARG, kw
    buf = np.zeros(4096, np.uint8)
    arr = (antq_lib._DecodeJob * 1)(ok)
    assert L.antq_decode4_batch_build(None, 1, BF16, ctypes.c_uint(0), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(4096)) == ERR_ARG
    assert L.antq_decode4_batch_build(arr, 1, BF16, ctypes.c_uint(0), None, ctypes.c_size_t(4096)) == ERR_ARG
    assert L.antq_decode4_batch_build(arr, 0, BF16, ctypes.c_uint(0), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(4096)) == ERR_ARG
    assert L.antq_decode4_batch_capacity(None, 1, BF16) == 0
    assert L.antq_decode4_batch(None, None, None) == ERR_ARG
    assert L.antq_decode4_batch(buf.ctypes.data_as(ctypes.c_void_p), buf.ctypes.data_as(ctypes.c_void_p), None) == ERR_PLAN    # no magic
    # an output that is not aligned to its element
    assert _build(antq_lib, [_job(antq_lib, out=FAKE + 1)])[0] == ERR_ALIGN


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


@pytest.mark.parametrize("tree", ["ant", "olive"])
def test_skip_reasons_and_packed_key_layout(antq_lib, tree):
    import torch
    import torch.nn as nn
    from ant_quantization_amd import packed
    qmod = importlib.import_module("ant_quantization_amd.%s.quant_model" % tree)
    qutil = importlib.import_module("ant_quantization_amd.%s.quant_utils" % tree)
    for name in ("pack_model", "packed_state_dict", "load_packed_state_dict", "set_weights_at_rest"):
        assert hasattr(qutil, name)
    qutil.set_quantizer(_args(mode="flint", wbit=4, abit=4))
    net = nn.Sequential(nn.Linear(64, 48), nn.ReLU(), nn.Linear(48, 64), nn.Linear(64, 20), nn.Linear(20, 16), nn.Linear(16, 8),
                        nn.Linear(8, 8))
    model = qmod.quantize_model(net)
    qutil.enable_quantization(model)
    layers = [m for m in model if hasattr(m, "quant_weight")]
    why = lambda m: packed.PackedBank._unsuitable(m.quant_weight, m.weight)      # noqa: E731
    assert why(layers[0]) == "not calibrated yet"
    for m in layers:
        _calibrated_like(m.quant_weight, tree)
    _calibrated_like(layers[4].quant_weight, tree, bits=8)
    _calibrated_like(layers[5].quant_weight, tree, signed=False)
    # suitable layers: only where the weight lives is left to object to on a host model
    assert why(layers[0]) == why(layers[1]) == why(layers[2]) == "weight not resident / not contiguous"
    assert why(layers[3]) == "row length 20 is not a multiple of 8"
    assert re.match(r"(codebook of 256 values|\d+ (normal|outlier) values)", why(layers[4])), why(layers[4])     # an 8-bit layer
    if tree == "olive":
        assert why(layers[5]) == "16 normal values leave no code for the pair identifier"     # OliVe's unsigned 4-bit codebook
    else:
        assert why(layers[5]) == "weight not resident / not contiguous"                       # ANT's unsigned 4-bit flint packs
    layers[0].quant_weight.mode = "base"
    assert why(layers[0]) == "mode base"
    layers[0].quant_weight.mode = "flint"
    assert why(model[0].double()) == "dtype torch.float64"
    with pytest.raises(antq_lib.AntqError):
        packed.PackedBank(model)                      # nothing to pack on the host: an error, not a fall-back
    assert all(m.quant_weight._bank is None for m in layers)
    with pytest.raises(antq_lib.AntqError):
        packed.packed_state_dict(model)
    # the key layout: weights of packed layers leave, their codes come, everything else is the reference's state dict
    sd = model.state_dict()
    codes = {"0": torch.zeros(64 * 48 // 2, dtype=torch.uint8), "2": torch.zeros(48 * 64 // 2, dtype=torch.uint8)}
    psd = packed._packed_keys(sd, codes)
    assert set(psd) == (set(sd) - {"0.weight", "2.weight"}) | {"0.quant_weight.codes", "2.quant_weight.codes"}
    assert "0.weight" in sd and "3.weight" in psd and "0.bias" in psd and "0.quant_weight.alpha" in psd
    assert psd["0.quant_weight.codes"].dtype == torch.uint8 and psd["0.quant_weight.codes"].numel() == model[0].weight.numel() // 2
