#!/usr/bin/env python3
"""A/B of a packed GPT-2 Conv1D layer (weight [K, N], y = x @ W + b) with 1 .. 8 input rows, the protocol of
profiles/packed_linear.md: same process, each arm rotating over enough distinct weight buffers to exceed the 256 MiB Infinity
Cache so that every call streams its weights from HBM, per point `--reps` measurements of one captured graph of calls per arm,
the arms ALTERNATED inside every repetition; the median and the spread (max - min) / median are reported.

    A  torch.addmm on the decoded image                         (a packed model that keeps its images: today's path)
    C  antq_decode4 into one scratch buffer, then torch.addmm   (the keep_images=False path for calls that do not qualify)
    B  antq_linear4_t on the codes

Layers: GPT-2 small's and GPT-2 XL's four Conv1D shapes, bf16 / f16 / fp32, ANT flint-4 and OliVe flint + outliers, one scale
per row k of the codes, M in {1, 2, 4, 8}.  The number of calls per graph follows the layer: at least `--iters`, and as many as
it takes for the codes touched by one replay to exceed the cache (capped at `--max-iters`).

    python tools/probe_linear4_t.py [--quick] [--out profiles/packed_linear_t]      (writes .json and .md)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids  # noqa: E402

SHAPES = [("gpt2 c_attn", 768, 2304), ("gpt2 attn.c_proj", 768, 768), ("gpt2 c_fc", 768, 3072), ("gpt2 mlp.c_proj", 3072, 768),
          ("gpt2-xl c_attn", 1600, 4800), ("gpt2-xl attn.c_proj", 1600, 1600), ("gpt2-xl c_fc", 1600, 6400), ("gpt2-xl mlp.c_proj", 6400, 1600)]
ROTATE_BYTES = 320 << 20     # per arm and replay: more than the Infinity Cache
MS = (1, 2, 4, 8)
HBM_BYTES_PER_S = 8.0e12

# `make -C ant_quantization_amd/csrc asm UNIT=antq_batch` (-Rpass-analysis=kernel-resource-usage), the 24 instantiations of
# k_linear_t<T, OVP, M> (--resources takes the remarks): the pair rule changes one SGPR and at most four VGPRs
RESOURCES = """| T | M | VGPRs | AGPRs | SGPRs | LDS bytes | scratch | spills | waves / SIMD (by registers) |
|---|---|---|---|---|---|---|---|---|
%s
"""


# What the run does not say: counted in the ISA of the same build, and the first tile shape, measured by the same tool in an
# earlier run on the same day (same protocol, one run).
NOTES = """## The K loop, counted in the ISA (not from a run)

The loop body is one group of steps of a lane -- 8 steps = 64 weights for M <= 2, 4 steps = 32 weights beyond -- and holds, in
the pair-rule instantiations:

| T | M | instructions per weight | of them vector ALU | LDS reads per weight | vector-memory loads per weight |
|---|---|---|---|---|---|
LOOP_ROWS

Per pair of weights: one byte extract, one `ds_read_b64` of the unscaled pair, two multiplies by the scale, the rounding to the
type (`DecOut<T>::make`), the widening (`Lin4W<T>::get`), 2 M `fmaf`; per step one more LDS read (the scale), one code word and M
elements of x.  About a hundred instructions of every loop body are scalar bookkeeping of its predicated steps.

## The tile: 32 columns and 128 phases against 64 columns and 64 phases

The kernel was first built as suggested -- a workgroup per 64 output columns, 64 phases of k, 4 steps in flight -- and measured
with this tool (192 points, same protocol, one run).  Its time followed K and not N ([768, 768] and [768, 3072] within 6 %;
8 / 13 / 20 / 37 us at K = 768 / 1600 / 3072 / 6400, M = 1, bf16): bound by the chain of a lane's own loads (K / 64 dependent
steps, one group of four per memory latency), with 12 ... 100 workgroups on 256 CUs, not by bandwidth (0.2 ... 4.7 % of 8 TB/s).
Half the tile and twice the phases (this build; 8 steps in flight for M <= 2) halves the chain and doubles the workgroups.
B's time, first shape over this one, min ... max over the six (dtype, codebook) runs:

| layer [K, N] | M = 1 | M = 2 | M = 4 | M = 8 |
|---|---|---|---|---|
| [768, 2304] | 0.84 ... 0.90 | 0.96 ... 1.15 | 1.06 ... 1.30 | 1.09 ... 1.25 |
| [768, 768] | 0.85 ... 0.91 | 0.97 ... 1.15 | 1.06 ... 1.30 | 1.09 ... 1.26 |
| [768, 3072] | 0.86 ... 0.92 | 0.96 ... 1.13 | 1.06 ... 1.29 | 1.08 ... 1.25 |
| [3072, 768] | 1.10 ... 1.25 | 1.06 ... 1.36 | 1.24 ... 1.55 | 1.28 ... 1.54 |
| [1600, 4800] | 0.92 ... 1.02 | 0.93 ... 1.17 | 1.11 ... 1.41 | 1.16 ... 1.37 |
| [1600, 1600] | 0.97 ... 1.08 | 0.99 ... 1.24 | 1.15 ... 1.45 | 1.19 ... 1.40 |
| [1600, 6400] | 0.91 ... 1.00 | 0.92 ... 1.14 | 1.08 ... 1.37 | 1.13 ... 1.35 |
| [6400, 1600] | 1.26 ... 1.48 | 1.21 ... 1.51 | 1.35 ... 1.66 | 1.41 ... 1.65 |

(Above 1: this build is faster.  Arm A agreed between the two runs within 4.2 % at every point, within 2 % on average.)  The smaller tile is kept: it
loses 8 ... 16 % at M = 1 on the K = 768 layers and wins 6 ... 66 % at M >= 4 and on the long-K layers.  Its 16-byte row
segments are a quarter of a 64-byte line; what that costs in fetched bytes was not measured.

## Not measured

Hardware counters (fetched bytes, LDS bank conflicts, occupancy on the device); other M; per-tensor scales; K > 8192 (scales
divided per step); a whole GPT-2's decode step; more than one run per point; tiles of 16 or 8 columns; a choice of tile by N.
The first shape's run is not kept as a file: the table above is all of it that is recorded.
"""


def loop_table(path):
    """rows of the table of NOTES from a file of lines `T M instructions valu lds vmem weights` (None: not available)"""
    if not path or not os.path.exists(path):
        return None
    out = []
    for line in open(path):
        f = line.split()
        if len(f) == 7:
            w = float(f[6])
            out.append("| %s | %s | %.1f | %.1f | %.2f | %.2f |" % (f[0], f[1], int(f[2]) / w, int(f[3]) / w, int(f[4]) / w, int(f[5]) / w))
    return "\n".join(out)


def books():
    g = grids.ant_flint(4, True)
    gn, go = grids.olive_flint(4, True), grids.olive_outliers(4, True)
    return [("ant flint-4", g, float(g.max()), 0, False), ("olive flint+outliers", np.concatenate([gn, go]), float(gn.max()), int(gn.size), True)]


def capture(fn, n_buf, iters, warm):
    """one graph of `iters` calls of fn, warmed up and replayed once"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(warm):
            fn(i % n_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            fn(i % n_buf)
    graph.replay()
    torch.cuda.synchronize()
    return graph


def alternate(graphs, iters, reps):
    """{arm: (median us per call, spread)}: every repetition replays every arm's graph once, in turn"""
    t = {k: [] for k in graphs}
    for _ in range(reps):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (float(np.median(v)), float((max(v) - min(v)) / np.median(v))) for k, v in t.items()}


def resources_table(path):
    """the table of the kernel's instantiations from the compiler's remarks saved in `path` (None: not available)"""
    if not path or not os.path.exists(path):
        return None
    import re
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: _ZN4antq10k_linear_tI(\S+?)Lb([01])ELi(\d)EEE", line)
        if m:
            cur = dict(T={"f": "fp32", "NS_8bf16_tagE": "bf16", "NS_7f16_tagE": "f16"}.get(m.group(1), m.group(1)), ovp=int(m.group(2)), M=int(m.group(3)))
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def write_md(rows, path, args, static):
    out = ["# antq_linear4_t against addmm on the image and against decode + addmm", "",
           "Written by `tools/probe_linear4_t.py%s`: one MI355X, one process, one run; every arm rotates over distinct weight buffers "
           "(more than 256 MiB touched per replay where %d calls reach that, see `calls`); per point %d repetitions of one "
           "graph-replayed batch of calls per arm, the arms alternated inside a repetition; medians in us per call, `spread` = the "
           "largest (max - min) / median of the point's arms." % (" --quick" if args.quick else "", args.max_iters, args.reps), "",
           "A = torch.addmm on the kept image, C = antq_decode4 into scratch + torch.addmm (the `keep_images=False` path of a call "
           "that does not qualify), B = antq_linear4_t on the codes.  One scale per row k, bias.  `% of 8 TB/s` = K N / 2 bytes of "
           "codes over B's time.", ""]
    keys = []
    for r in rows:
        k = (r["dtype"], r["book"])
        if k not in keys:
            keys.append(k)
    for dt, book in keys:
        out += ["## %s, %s" % (dt, book), "", "| layer [K, N] | M | calls | A | C | B | A / B | C / B | % of 8 TB/s | spread |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            if (r["dtype"], r["book"]) == (dt, book):
                out.append("| %s [%d, %d] | %d | %d | %.1f | %.1f | %.1f | %.2f | %.2f | %.1f | %.1f %% |" % (
                    r["layer"], r["K"], r["N"], r["M"], r["calls"], r["us_image"], r["us_decode_addmm"], r["us_linear4_t"], r["image_over_t"],
                    r["decode_addmm_over_t"], 100 * r["codes_fraction_of_hbm"], 100 * r["spread"]))
        out.append("")
    if rows:
        out += ["## Per layer and M: A / B and C / B over all %d runs (dtype x codebook), min ... max" % len(keys), "",
                "| layer [K, N] | M | A / B | C / B | B wins against A in | B wins against C in |", "|---|---|---|---|---|---|"]
        seen = []
        for r in rows:
            k = (r["layer"], r["K"], r["N"], r["M"])
            if k in seen:
                continue
            seen.append(k)
            pts = [q for q in rows if (q["layer"], q["K"], q["N"], q["M"]) == k]
            ab, cb = [q["image_over_t"] for q in pts], [q["decode_addmm_over_t"] for q in pts]
            out.append("| %s [%d, %d] | %d | %.2f ... %.2f | %.2f ... %.2f | %d of %d | %d of %d |" % (
                k[0], k[1], k[2], k[3], min(ab), max(ab), min(cb), max(cb), sum(v > 1 for v in ab), len(ab), sum(v > 1 for v in cb), len(cb)))
        out.append("")
    if static:
        body = "\n".join("| %s%s | %d | %d | %d | %d | %d | %d | %d | %d |" % (
            s["T"], ", pair rule" if s["ovp"] else "", s["M"], s.get("vgpr", -1), s.get("agpr", -1), s.get("sgpr", -1), s.get("lds", -1),
            s.get("scratch", -1), s.get("sspill", 0) + s.get("vspill", 0), s.get("occ", -1)) for s in sorted(static, key=lambda s: (s["T"], s["ovp"], s["M"])))
        out += ["## Resources of every instantiation (from the compiler, not from a run)", "", RESOURCES % body]
    loops = loop_table(args.loop_counts)
    if loops:
        out += [NOTES.replace("LOOP_ROWS", loops)]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, OliVe, GPT-2 small only")
    ap.add_argument("--iters", type=int, default=200, help="the fewest calls per graph")
    ap.add_argument("--max-iters", type=int, default=1200, help="the most calls per graph")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None, help="file with the compiler's kernel-resource-usage remarks of k_linear_t")
    ap.add_argument("--loop-counts", default=None, help="file of `T M instructions valu lds vmem weights` lines counted in the ISA of the K loop")
    ap.add_argument("--rewrite", default=None, help="a .json of an earlier run: write its .md again (no GPU needed) and stop")
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    a = ap.parse_args()
    static = resources_table(a.resources)
    if a.rewrite:
        write_md(json.load(open(a.rewrite)), (a.out or os.path.splitext(a.rewrite)[0]) + ".md", a, static)
        return
    if not torch.cuda.is_available():
        raise SystemExit("probe_linear4_t: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.bfloat16, torch.float16, torch.float32)):
        esz = torch.empty(0, dtype=dt).element_size()
        for bname, g, gmax, nn, ovp in (books()[1:] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, K, N in (SHAPES[:4] if a.quick else SHAPES):
                cbytes = K * N // 2
                iters = int(min(a.max_iters, max(a.iters, -(-ROTATE_BYTES // cbytes))))
                n_cod = iters
                n_img = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N * esz)))))
                w = (torch.randn(K, N, device=dev) * 0.05).to(dt)
                if ovp:
                    w.view(-1)[::997] *= 12
                alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
                codes0 = _lib.encode4(w, alpha, plan, gmax, K, N, True, n_normal=nn, ovp=ovp)
                image0 = _lib.decode4(codes0, alpha, plan, gmax, K, N, True, dt, n_normal=nn, ovp=ovp).view(K, N)
                del w
                images = [image0.clone() for _ in range(n_img)]
                codes = [codes0.clone() for _ in range(n_cod)]
                scratch = torch.empty(K * N, dtype=dt, device=dev)
                bias = torch.randn(N, device=dev).to(dt)

                def arm_c(i):
                    _lib.decode4(codes[i], alpha, plan, gmax, K, N, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                    return torch.addmm(bias, x, scratch.view(K, N))

                for M in MS:
                    x = torch.randn(M, K, device=dev).to(dt)
                    y = torch.empty(M, N, dtype=dt, device=dev)
                    lin = lambda i: _lib.linear4_t(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
                    graphs = {"A": capture(lambda i: torch.addmm(bias, x, images[i]), n_img, iters, 20), "C": capture(arm_c, n_cod, iters, 20),
                              "B": capture(lin, n_cod, iters, 20)}
                    t = alternate(graphs, iters, a.reps)
                    ta, tc, tb = t["A"][0], t["C"][0], t["B"][0]
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, K=K, N=N, M=M, calls=iters, image_buffers=n_img, code_buffers=n_cod,
                             us_image=round(ta, 2), us_decode_addmm=round(tc, 2), us_linear4_t=round(tb, 2), image_over_t=round(ta / tb, 3),
                             decode_addmm_over_t=round(tc / tb, 3), codes_fraction_of_hbm=round(cbytes / (tb * 1e-6) / HBM_BYTES_PER_S, 4),
                             spread=round(max(v[1] for v in t.values()), 4))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del graphs
                del images, codes, scratch
                torch.cuda.empty_cache()
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out + ".json", "w") as f:
                        json.dump(rows, f, indent=1)
                    write_md(rows, a.out + ".md", a, static)


if __name__ == "__main__":
    main()
