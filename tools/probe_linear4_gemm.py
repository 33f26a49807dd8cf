#!/usr/bin/env python3
"""A/B of a packed Linear layer with 64 .. 4096 input rows, the protocol of profiles/packed_linear.md (same process, each arm
rotating over 1 GiB of distinct weight buffers so that every call streams its weights from HBM, per point `--reps` measurements
of `--iters` calls replayed from one captured graph per arm, the arms ALTERNATED inside every repetition; the median and the
spread (max - min) / median are reported):

    A  F.linear on the decoded image                         (a packed model that keeps its images)
    C  antq_decode4 into one scratch buffer, then F.linear   (today's keep_images=False path beyond 64 rows)
    B  antq_linear4_gemm on the codes
    L  antq_linear4_mm on the codes, at M = 64 only

Layers: OPT-6.7B's three Linear shapes and BERT-base's two, bf16 and f16, ANT flint-4 and OliVe flint + outliers, per-row
scales, M in {64, 128, 256, 512, 1024, 4096}.  B is also timed with either tile shape forced (antq_debug_set key 23 = 2 / 4
wavefronts, i.e. 128 / 256 rows of x per workgroup); the results of the kernel do not depend on it.

    python tools/probe_linear4_gemm.py [--quick] [--out profiles/packed_linear4_gemm]      (writes .json and .md)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids  # noqa: E402

SHAPES = [("opt6.7b qkv/out", 4096, 4096), ("opt6.7b fc1", 16384, 4096), ("opt6.7b fc2", 4096, 16384),
          ("bert fc1", 3072, 768), ("bert fc2", 768, 3072)]
ROTATE_BYTES = 1 << 30       # per arm: four times the Infinity Cache
MS = (64, 128, 256, 512, 1024, 4096)

# `make -C ant_quantization_amd/csrc asm UNIT=antq_batch` (-Rpass-analysis=kernel-resource-usage), all 16 instantiations of
# k_linear4_gemm<T, OVP, WAVES, VEC>: the lines do not differ between bf16 and f16 or with OVP
RESOURCES = """| WAVES (rows of x per workgroup) | codes per lane | VGPRs | AGPRs | SGPRs | LDS bytes | scratch | spills | waves / SIMD |
|---|---|---|---|---|---|---|---|---|
| 4 (256) | 16 B | 242 | 64 | 62 | 131456 | 0 | 0 | 1 |
| 4 (256) | 4 B | 238 | 64 | 62 | 131456 | 0 | 0 | 1 |
| 2 (128) | 16 B | 250 | 64 | 62 | 98688 | 0 | 0 | 1 |
| 2 (128) | 4 B | 246 | 64 | 62 | 98688 | 0 | 0 | 1 |
"""


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


def write_md(rows, path, args):
    out = ["# antq_linear4_gemm against F.linear on the image and against decode + F.linear", "",
           "Written by `tools/probe_linear4_gemm.py%s`: one MI355X, one process; every arm rotates over 1 GiB of distinct weights; per "
           "point %d repetitions of %d graph-replayed calls per arm, the arms alternated inside a repetition; medians in us, "
           "`spread` = the largest (max - min) / median of the point's arms." % (" --quick" if args.quick else "", args.reps, args.iters), "",
           "A = F.linear on the kept image, C = antq_decode4 into scratch + F.linear (the `keep_images=False` path the option "
           "replaces), B = antq_linear4_gemm with the launcher's tile rule, B128 / B256 = B with 128 / 256 rows of x per workgroup "
           "forced (key 23 = 2 / 4), L = antq_linear4_mm (M = 64 only).  Per-row scales, bias.", ""]
    keys = []
    for r in rows:
        k = (r["dtype"], r["book"])
        if k not in keys:
            keys.append(k)
    for dt, book in keys:
        out += ["## %s, %s" % (dt, book), "", "| layer [N, K] | M | A | C | B | B128 | B256 | L | C / B | A / B | B TFLOP/s | spread |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            if (r["dtype"], r["book"]) == (dt, book):
                out.append("| %s [%d, %d] | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %s | %.2f | %.2f | %.0f | %.1f %% |" % (
                    r["layer"], r["N"], r["K"], r["M"], r["us_image"], r["us_decode_linear"], r["us_gemm"], r["us_gemm_w2"], r["us_gemm_w4"],
                    "%.1f" % r["us_mm"] if "us_mm" in r else "", r["decode_linear_over_gemm"], r["image_over_gemm"], r["gemm_tflops"], 100 * r["spread"]))
        out.append("")
    out += ["## Per layer: the M at which B wins in all %d runs (dtype x codebook)" % len(keys), "",
            "| layer [N, K] | B beats C at M = | largest M up to which B beats C | B beats A at M = | largest M up to which B beats A |", "|---|---|---|---|---|"]
    layers = []
    for r in rows:
        if (r["layer"], r["N"], r["K"]) not in layers:
            layers.append((r["layer"], r["N"], r["K"]))
    for name, N, K in layers:
        cell = []
        for ratio in ("decode_linear_over_gemm", "image_over_gemm"):
            wins = [M for M in MS if all(r[ratio] > 1.0 for r in rows if r["N"] == N and r["K"] == K and r["M"] == M)]
            upto = 0
            for M in MS:
                if M not in wins:
                    break
                upto = M
            cell += [", ".join(map(str, wins)) or "none", str(upto) if upto else "none (loses at M = 64)"]
        out.append("| %s [%d, %d] | %s |" % (name, N, K, " | ".join(cell)))
    out += ["", "## Resources of every instantiation", "", RESOURCES]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, ANT only")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    knob = _lib.lib().antq_debug_set
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.bfloat16, torch.float16)):
        for bname, g, gmax, nn, ovp in (books()[:1] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, N, K in SHAPES:
                n_img = max(2, -(-ROTATE_BYTES // (N * K * 2)))
                n_cod = max(2, -(-ROTATE_BYTES // (N * K // 2)))
                w = (torch.randn(N, K, device=dev) * 0.05).to(dt)
                if ovp:
                    w.view(-1)[::997] *= 12
                alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
                codes0 = _lib.encode4(w, alpha, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
                image0 = _lib.decode4(codes0, alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp).view(N, K)
                del w
                images = [image0.clone() for _ in range(n_img)]
                codes = [codes0.clone() for _ in range(n_cod)]
                scratch = torch.empty(N * K, dtype=dt, device=dev)
                bias = torch.randn(N, device=dev).to(dt)

                def arm_c(i):
                    _lib.decode4(codes[i], alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                    return F.linear(x, scratch.view(N, K), bias)

                for M in MS:
                    x = torch.randn(M, K, device=dev).to(dt)
                    y = torch.empty(M, N, dtype=dt, device=dev)
                    gemm = lambda i: _lib.linear4_gemm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
                    graphs = {"A": capture(lambda i: F.linear(x, images[i], bias), n_img, a.iters, 20), "C": capture(arm_c, n_cod, a.iters, 20),
                              "B": capture(gemm, n_cod, a.iters, 20)}
                    for wv in (2, 4):                   # (the knob is read at capture: the graph keeps the kernel it chose)
                        knob(23, wv)
                        graphs["B%d" % wv] = capture(gemm, n_cod, a.iters, 20)
                    knob(23, 0)
                    if M <= _lib.LINEAR4_MM_MAX_M:
                        graphs["L"] = capture(lambda i: _lib.linear4_mm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn,
                                                                        ovp=ovp, out=y), n_cod, a.iters, 20)
                    t = alternate(graphs, a.iters, a.reps)
                    ta, tc, tb = t["A"][0], t["C"][0], t["B"][0]
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, N=N, K=K, M=M, us_image=round(ta, 2),
                             us_decode_linear=round(tc, 2), us_gemm=round(tb, 2), us_gemm_w2=round(t["B2"][0], 2), us_gemm_w4=round(t["B4"][0], 2),
                             gemm_tflops=round(2.0 * M * N * K / (tb * 1e-6) / 1e12, 1), image_over_gemm=round(ta / tb, 3),
                             decode_linear_over_gemm=round(tc / tb, 3), spread=round(max(v[1] for v in t.values()), 4))
                    if "L" in t:
                        r["us_mm"] = round(t["L"][0], 2)
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del graphs
                del images, codes, scratch
                torch.cuda.empty_cache()
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out + ".json", "w") as f:
                        json.dump(rows, f, indent=1)
                    write_md(rows, a.out + ".md", a)


if __name__ == "__main__":
    main()
