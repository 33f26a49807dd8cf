#!/usr/bin/env python3
"""A/B/C of a byte-coded Linear layer with few input rows, the method of tools/probe_linear4.py: same process, the arms
alternated, event-timed, replayed from one captured graph of `--iters` calls (the kernels alone).

    A  F.linear on the kept image
    C  antq_decode8 into one scratch buffer, then F.linear on it (what a layer without an image did before antq_linear8)
    B  antq_linear8 on the byte codes
    4  antq_linear4 on a 4-bit book of the same shape: the reference for the element rate

Layers: OPT-6.7B's three Linear shapes and BERT-base's two; M in {1, 2, 4, 8}; bf16, f16 and fp32; ANT int-8 (`int_b8_s`) and
OliVe int-8 + outliers (`olive_int_b8`: 255 + 254 values).  Each arm rotates over enough distinct weight buffers that the
rotation exceeds the 256 MB Infinity Cache (every call streams its weights from HBM).  `--rounds` rounds of A, C, B, 4 in turn;
the median over the rounds is reported, and the largest spread (max - min) / median of any arm over the rounds.
Then the resident bytes of a mixed model (counts, not timings): tools/probe_decode8.py's stack of BERT-base's 74 Linear layers
with set_8_bit_layer_n(model, 8), `pack_model(byte_codes=True)` against `fused_linear=True, fused_bytes=True, keep_images=False`
(both with release_weights=True).

This process never opens the GPU: every step -- one (dtype, book) of the timing, one tree of the model part -- runs in a child
process of its own under its own time limit (`--step-timeout` seconds), and the first step that fails or runs out of time ends
the run (nothing more is started on a GPU that may have faulted).  Run the whole tool under `timeout` as well.

    timeout 1500 python tools/probe_linear8.py [--quick] [--out profiles/packed_linear8]      (writes <out>.json and <out>.md)
"""
import argparse
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids  # noqa: E402

SHAPES = [(4096, 4096), (16384, 4096), (4096, 16384), (3072, 768), (768, 3072)]
ROTATE_BYTES = 1 << 29       # per arm: twice the Infinity Cache


def books():
    """name -> (8-bit grid, gmax, n_normal, pair rule, the 4-bit grid of the family, its gmax, its n_normal)"""
    g8, g4 = np.asarray(grids.ant_grid("int", 8, True), np.float32), np.asarray(grids.ant_grid("int", 4, True), np.float32)
    gn, go = grids.olive_int(8, True), grids.olive_outliers(8, True)
    gn4, go4 = grids.olive_int(4, True), grids.olive_outliers(4, True)
    return {"int_b8_s": (g8, float(g8.max()), 0, False, g4, float(g4.max()), 0),
            "olive_int_b8": (np.concatenate([gn, go]).astype(np.float32), float(np.max(gn)), int(len(gn)), True,
                             np.concatenate([gn4, go4]).astype(np.float32), float(np.max(gn4)), int(len(gn4)))}


DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}


def graph_of(fn, n_buf, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(min(20, iters)):
            fn(i % n_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            fn(i % n_buf)
    g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def time_step(dtype_name, bname, quick, iters, rounds):
    """one (dtype, book): every shape and M; prints one JSON line per point"""
    dev = torch.device("cuda:0")
    dt = DTYPES[dtype_name]
    esz = 4 if dt == torch.float32 else 2
    g, gmax, nn, ovp, g4, gmax4, nn4 = books()[bname]
    plan, plan4 = _lib.plan_for(g), _lib.plan_for(g4)
    gd, gd4 = plan.grid_dev(dev), plan4.grid_dev(dev)
    for N, K in (SHAPES[:2] if quick else SHAPES):
        n_img = max(2, -(-ROTATE_BYTES // (N * K * esz)))
        n_c8 = max(2, -(-ROTATE_BYTES // (N * K)))
        n_c4 = max(2, -(-ROTATE_BYTES // (N * K // 2)))
        w = (torch.randn(N, K, device=dev) * 0.05).to(dt)
        if ovp:
            w.view(-1)[::997] *= 12
        alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
        c8 = _lib.encode8(w, alpha, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
        c4 = _lib.encode4(w, alpha, plan4, gmax4, N, K, True, n_normal=nn4, ovp=ovp)
        img = _lib.decode8(c8, alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp).view(N, K)
        del w
        images = [img.clone() for _ in range(n_img)]
        codes8 = [c8.clone() for _ in range(n_c8)]
        codes4 = [c4.clone() for _ in range(n_c4)]
        scratch = torch.empty(N * K, dtype=dt, device=dev)
        bias = torch.randn(N, device=dev).to(dt)
        for M in (1, 2, 4, 8):
            x = torch.randn(M, K, device=dev).to(dt)
            y = torch.empty(M, N, dtype=dt, device=dev)

            def arm_c(i):
                _lib.decode8(codes8[i], alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                return F.linear(x, scratch.view(N, K), bias)
            arms = {"A": (lambda i: F.linear(x, images[i], bias), n_img), "C": (arm_c, n_c8),
                    "B": (lambda i: _lib.linear8(codes8[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y), n_c8),
                    "4": (lambda i: _lib.linear4(codes4[i], x, alpha, gd4, gmax4, N, K, True, bias=bias, n_normal=nn4, ovp=ovp, out=y), n_c4)}
            graphs = {k: graph_of(fn, n, iters) for k, (fn, n) in arms.items()}
            t = {k: [] for k in arms}
            for _ in range(rounds):
                for k in arms:
                    t[k].append(time_us(graphs[k], iters))
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = max((max(v) - min(v)) / med[k] for k, v in t.items())
            r = dict(dtype=dtype_name, book=bname, N=N, K=K, M=M, rounds=rounds, iters=iters,
                     us_A=round(med["A"], 2), us_C=round(med["C"], 2), us_B=round(med["B"], 2), us_linear4=round(med["4"], 2),
                     B_codes_frac_8TBs=round(N * K / (med["B"] * 1e-6) / 8e12, 4), B_over_A=round(med["A"] / med["B"], 3),
                     B_over_C=round(med["C"] / med["B"], 3), linear4_over_B=round(med["4"] / med["B"], 3), worst_spread=round(spread, 3))
            print("ROW " + json.dumps(r), flush=True)
            del graphs
        del images, codes8, codes4, scratch
        torch.cuda.empty_cache()


def model_step(tree):
    """resident bytes of probe_decode8's BERT-base stack with 8 pairs at 8 bits, with images and without"""
    import copy
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from probe_decode8 import BertStack
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    qmod = importlib.import_module("ant_quantization_amd.%s.quant_model" % tree)
    qutil = importlib.import_module("ant_quantization_amd.%s.quant_utils" % tree)
    qutil.set_quantizer(types.SimpleNamespace(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False,
                                              mode={"ant": "ant-int-pot-flint", "olive": "ant-int-flint"}[tree], wbit=4, abit=4))
    torch.manual_seed(0)
    model = qmod.quantize_model(BertStack()).to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    x = torch.randn(4, 768, device=dev).to(dt)
    with torch.no_grad():
        model(x)
        qmod.set_8_bit_layer_n(model, 8)
        model(x)                           # calibrates again with the 8-bit layers
        for label, kw in (("byte_codes", dict(byte_codes=True)),
                          ("fused_bytes, no images", dict(byte_codes=True, fused_linear=True, fused_bytes=True, keep_images=False))):
            m = copy.deepcopy(model)
            bank = qutil.pack_model(m, release_weights=True, **kw)
            y = m(x)
            skipped = {n for n, _ in bank.skipped}
            w_float = sum(p.numel() * p.element_size() for n, p in m.named_parameters() if n.endswith(".weight") and n[:-7] in skipped)
            codes, images = bank.nbytes()
            r = dict(tree=tree, dtype="bfloat16", options=label, packed_layers=len(bank.entries),
                     byte_coded_layers=sum(e["width"] == 8 for e in bank.entries.values()),
                     layers_without_image=sum(e["out"] is None for e in bank.entries.values()), skipped_layers=len(bank.skipped),
                     fused_calls=bank.fused_calls, fused_byte_calls=bank.fused_byte_calls, finite=bool(torch.isfinite(y.float()).all()),
                     codes_bytes=int(codes), image_and_scratch_bytes=int(images), float_weight_bytes=int(w_float),
                     resident_weight_bytes=int(codes + images + w_float))
            print("MODEL " + json.dumps(r), flush=True)


def write_out(prefix, rows, model_rows, rounds, iters, note):
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    with open(prefix + ".json", "w") as f:
        json.dump(dict(rounds=rounds, iters=iters, note=note, timing=rows, model=model_rows), f, indent=1)
    with open(prefix + ".md", "w") as f:
        f.write("# antq_linear8 (B) against F.linear on the image (A) and antq_decode8 + F.linear (C)\n\n"
                "One MI355X, ONE run of the tool; one process per (dtype, book), arms alternated at every point, %d rounds of a graph of %d calls each, medians;\n"
                "times in us per call (kernels alone, replayed from a graph).  `B/8TB/s`: code bytes of B per second as a share of 8 TB/s.\n"
                "`xA`, `xC`: A / B and C / B (above 1: B is faster).  `x4`: antq_linear4's time on the family's 4-bit book over B's.\n"
                "`spread`: the largest (max - min) / median of any arm over the rounds.  No hardware counters were collected.\n%s\n\n" % (rounds, iters, note))
        f.write("| dtype | book | N | K | M | A | C | B | linear4 | B/8TB/s | xA | xC | x4 | spread |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s | %d | %d | %d | %.2f | %.2f | %.2f | %.2f | %.1f %% | %.2f | %.2f | %.2f | %.1f %% |\n" % (
                r["dtype"], r["book"], r["N"], r["K"], r["M"], r["us_A"], r["us_C"], r["us_B"], r["us_linear4"],
                100 * r["B_codes_frac_8TBs"], r["B_over_A"], r["B_over_C"], r["linear4_over_B"], 100 * r["worst_spread"]))
        f.write("\n## Largest M at which B beats A / beats C (0: at none; M in 1, 2, 4, 8)\n\n"
                "| dtype | book | N | K | beats A up to | beats C up to |\n|---|---|---|---|---|---|\n")
        for k in sorted({(r["dtype"], r["book"], r["N"], r["K"]) for r in rows}):
            rs = [r for r in rows if (r["dtype"], r["book"], r["N"], r["K"]) == k]
            f.write("| %s | %s | %d | %d | %d | %d |\n" % (k + (max([r["M"] for r in rs if r["B_over_A"] > 1] or [0]),
                                                             max([r["M"] for r in rs if r["B_over_C"] > 1] or [0]))))
        f.write("\n## Resident weight bytes: BERT-base's 74 Linear layers, 8 pairs at 8 bits, bf16, release_weights=True\n\n"
                "| tree | options | packed | byte-coded | without image | codes MB | images + scratch MB | float MB | resident MB |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in model_rows:
            f.write("| %s | %s | %d | %d | %d | %.1f | %.1f | %.1f | %.1f |\n" % (
                r["tree"], r["options"], r["packed_layers"], r["byte_coded_layers"], r["layers_without_image"], r["codes_bytes"] / 1e6,
                r["image_and_scratch_bytes"] / 1e6, r["float_weight_bytes"] / 1e6, r["resident_weight_bytes"] / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, two shapes, the plain book, one tree")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "time":
            time_step(a.child[1], a.child[2], a.quick, a.iters, a.rounds)
        else:
            model_step(a.child[1])
        return
    steps = [["time", d, b] for d in (("bfloat16",) if a.quick else DTYPES) for b in (("int_b8_s",) if a.quick else books())]
    steps += [["model", t] for t in (("ant",) if a.quick else ("ant", "olive"))]
    rows, model_rows, note = [], [], ""
    for st in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--rounds", str(a.rounds)] + (["--quick"] if a.quick else []) + ["--child"] + st
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            rc, out, err = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            rc, out, err = 124, (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), "time limit"
        for line in out.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
            elif line.startswith("MODEL "):
                model_rows.append(json.loads(line[6:]))
        print("step %s: rc %d, %d timing rows, %d model rows so far" % (" ".join(st), rc, len(rows), len(model_rows)), flush=True)
        if rc != 0:
            note = "INCOMPLETE: step `%s` ended with status %d; nothing was started after it." % (" ".join(st), rc)
            print(err[-2000:], flush=True)
            break
    if a.out:
        write_out(a.out, rows, model_rows, a.rounds, a.iters, note)
    sys.exit(1 if note else 0)


if __name__ == "__main__":
    main()
