#!/usr/bin/env python3
"""A/B of a byte-coded packed Linear layer with 64 .. 4096 input rows: tools/probe_linear4_gemm.py's protocol for the byte form
of the tiled kernel (same process, each arm rotating over 1 GiB of distinct weight buffers so that every call streams its
weights from HBM, per point `--reps` measurements of graph-replayed calls per arm, the arms ALTERNATED inside every
repetition; the median and the spread (max - min) / median are reported):

    A  F.linear on the decoded image                         (a packed model that keeps its images)
    C  antq_decode8 into one scratch buffer, then F.linear   (today's keep_images=False path beyond 64 rows)
    B  antq_linear8_gemm on the byte codes
    L  antq_linear8_mm on the byte codes, at M = 64 only

Layers: OPT-6.7B's three Linear shapes and BERT-base's two, bf16 and f16, ANT int-8 and OliVe int-8 + outliers, per-row
scales, M in {64, 128, 256, 512, 1024, 4096}.  B is also timed with either tile shape forced (antq_debug_set key 23 = 2 / 4
wavefronts, i.e. 128 / 256 rows of x per workgroup); the results of the kernel do not depend on it.  A graph holds `--iters`
calls up to M = 512 and a quarter of that beyond (the calls are long there).

    python tools/probe_linear8_gemm.py [--dtypes bfloat16,float16] [--books 0,1] [--out profiles/packed_linear8_gemm]
    python tools/probe_linear8_gemm.py --merge a.json b.json --out profiles/packed_linear8_gemm     (joins runs, writes .json and .md)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ant_quantization_amd import _lib, grids  # noqa: E402
from probe_linear4_gemm import MS, ROTATE_BYTES, SHAPES, alternate, capture  # noqa: E402

# `make -C ant_quantization_amd/csrc asm UNIT=antq_batch` (-Rpass-analysis=kernel-resource-usage), all 16 instantiations of
# k_linear_gemm<Lin8Codec<T, OVP>, WAVES, VEC>: the lines do not differ between bf16 and f16
RESOURCES = """| pair rule | WAVES (rows of x per workgroup) | code loads per lane, output tile and step | VGPRs | AGPRs | SGPRs | LDS bytes | scratch | spills | waves / SIMD |
|---|---|---|---|---|---|---|---|---|---|
%s
"""


def books():
    g8 = np.asarray(grids.ant_grid("int", 8, True), np.float32)
    gn, go = grids.olive_int(8, True), grids.olive_outliers(8, True)
    return [("ant int-8", g8, float(g8.max()), 0, False),
            ("olive int-8+outliers", np.concatenate([gn, go]).astype(np.float32), float(np.max(gn)), int(len(gn)), True)]


def resources_table(path=None):
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "packed_linear8_gemm_resources.json")
    if not os.path.exists(path):
        return RESOURCES % "| (not recorded) |"
    rows = json.load(open(path))
    return RESOURCES % "\n".join("| %s | %d (%d) | %s | %d | %d | %d | %d | %d | %d | %d |" % (
        "yes" if r["pair"] else "no", r["waves"], 64 * r["waves"], "2 x 16 B" if r["vec"] else "4 x 8 B", r["vgprs"], r["agprs"], r["sgprs"], r["lds"],
        r["scratch"], r["spills"], r["occupancy"]) for r in rows)


def write_md(rows, path, args, notes=()):
    out = ["# antq_linear8_gemm against F.linear on the image and against decode + F.linear", "",
           "Written by `tools/probe_linear8_gemm.py`: one MI355X, one process per dtype; every arm rotates over 1 GiB of distinct "
           "weights; per point %d repetitions of graph-replayed calls per arm (%d calls per graph up to M = 512, %d beyond), the arms "
           "alternated inside a repetition; medians in us, `spread` = the largest (max - min) / median of the point's arms." % (
               args.reps, args.iters, max(1, args.iters // 4)), "",
           "A = F.linear on the kept image, C = antq_decode8 into scratch + F.linear (the `keep_images=False` path the option "
           "replaces), B = antq_linear8_gemm with the launcher's tile rule, B128 / B256 = B with 128 / 256 rows of x per workgroup "
           "forced (key 23 = 2 / 4), L = antq_linear8_mm (M = 64 only).  Per-row scales, bias, the 16-byte code path.", ""]
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
            "| layer [N, K] | B beats C at M = | C / B, all runs | B beats A at M = | A / B, all runs |", "|---|---|---|---|---|"]
    layers = []
    for r in rows:
        if (r["layer"], r["N"], r["K"]) not in layers:
            layers.append((r["layer"], r["N"], r["K"]))
    for name, N, K in layers:
        cell = []
        for ratio in ("decode_linear_over_gemm", "image_over_gemm"):
            mine = [r for r in rows if r["N"] == N and r["K"] == K]
            wins = [M for M in MS if [r for r in mine if r["M"] == M] and all(r[ratio] > 1.0 for r in mine if r["M"] == M)]
            cell += [", ".join(map(str, wins)) or "none", "%.2f ... %.2f" % (min(r[ratio] for r in mine), max(r[ratio] for r in mine))]
        out.append("| %s [%d, %d] | %s |" % (name, N, K, " | ".join(cell)))
    out += ["", "## Resources of every instantiation", "", resources_table()]
    out += list(notes)
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bfloat16,float16")
    ap.add_argument("--books", default="0,1", help="indices into books()")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    ap.add_argument("--merge", nargs="*", default=None, help="join the .json files of earlier runs instead of measuring")
    ap.add_argument("--notes", default=None, help="a text file appended to the .md")
    a = ap.parse_args()
    if a.merge is not None:
        rows = [r for p in a.merge for r in json.load(open(p))]
        with open(a.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)
        write_md(rows, a.out + ".md", a, notes=open(a.notes).read().split("\n") if a.notes else ())
        return
    dev = torch.device("cuda:0")
    knob = _lib.lib().antq_debug_set
    rows = []
    for dt in [getattr(torch, d) for d in a.dtypes.split(",")]:
        for bname, g, gmax, nn, ovp in [books()[int(i)] for i in a.books.split(",")]:
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, N, K in SHAPES:
                n_img = max(2, -(-ROTATE_BYTES // (N * K * 2)))
                n_cod = max(2, -(-ROTATE_BYTES // (N * K)))
                w = (torch.randn(N, K, device=dev) * 0.05).to(dt)
                if ovp:
                    w.view(-1)[::997] *= 12
                alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
                codes0 = _lib.encode8(w, alpha, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
                image0 = _lib.decode8(codes0, alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp).view(N, K)
                del w
                images = [image0.clone() for _ in range(n_img)]
                codes = [codes0.clone() for _ in range(n_cod)]
                scratch = torch.empty(N * K, dtype=dt, device=dev)
                bias = torch.randn(N, device=dev).to(dt)

                def arm_c(i):
                    _lib.decode8(codes[i], alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                    return F.linear(x, scratch.view(N, K), bias)

                for M in MS:
                    iters = a.iters if M <= 512 else max(1, a.iters // 4)
                    x = torch.randn(M, K, device=dev).to(dt)
                    y = torch.empty(M, N, dtype=dt, device=dev)
                    gemm = lambda i: _lib.linear8_gemm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)   # noqa: E731
                    graphs = {"A": capture(lambda i: F.linear(x, images[i], bias), n_img, iters, 20), "C": capture(arm_c, n_cod, iters, 20),
                              "B": capture(gemm, n_cod, iters, 20)}
                    for wv in (2, 4):                   # (the knob is read at capture: the graph keeps the kernel it chose)
                        knob(23, wv)
                        graphs["B%d" % wv] = capture(gemm, n_cod, iters, 20)
                    knob(23, 0)
                    if M <= _lib.LINEAR8_MM_MAX_M:
                        graphs["L"] = capture(lambda i: _lib.linear8_mm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn,
                                                                        ovp=ovp, out=y), n_cod, iters, 20)
                    t = alternate(graphs, iters, a.reps)
                    ta, tc, tb = t["A"][0], t["C"][0], t["B"][0]
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, N=N, K=K, M=M, iters=iters, us_image=round(ta, 2),
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
