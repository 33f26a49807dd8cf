#!/usr/bin/env python3
"""A/B of a packed Linear layer with 8 .. 64 input rows, the protocol of tools/probe_linear4.py (same process, each arm
rotating over 1 GiB of distinct weight buffers so that every call streams its weights from HBM, the median of `--reps`
measurements of `--iters` calls replayed from one captured graph):

    A  F.linear on the decoded image                         (a packed model that keeps its images)
    C  antq_decode4 into one scratch buffer, then F.linear   (today's keep_images=False path beyond 8 rows)
    B  antq_linear4_mm on the codes
    L  antq_linear4 on the codes, at M = 8 only

Layers: OPT-6.7B's three Linear shapes and BERT-base's two, bf16 and f16, ANT flint-4 and OliVe flint + outliers,
M in {8, 16, 32, 64}.  `--tiles` also times B with the launcher's tile rule overridden (antq_debug_set key 22 = 1 / 2 / 4
tiles of 16 output rows per workgroup); the results of the kernel do not depend on it.

    python tools/probe_linear4_mm.py [--quick] [--tiles] [--out profiles/packed_linear_mm.json]
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
MS = (8, 16, 32, 64)


def books():
    g = grids.ant_flint(4, True)
    gn, go = grids.olive_flint(4, True), grids.olive_outliers(4, True)
    return [("ant flint-4", g, float(g.max()), 0, False), ("olive flint+outliers", np.concatenate([gn, go]), float(gn.max()), int(gn.size), True)]


def timed(fn, n_buf, iters, reps, warm):
    """us per call: the median of `reps` replays of one captured graph of `iters` calls"""
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
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, the OPT shapes, ANT only")
    ap.add_argument("--tiles", action="store_true", help="also time B with 1 / 2 / 4 tiles of output rows per workgroup forced")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    knob = _lib.lib().antq_debug_set
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.bfloat16, torch.float16)):
        for bname, g, gmax, nn, ovp in (books()[:1] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, N, K in (SHAPES[:3] if a.quick else SHAPES):
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
                    mm = lambda i: _lib.linear4_mm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
                    ta = timed(lambda i: F.linear(x, images[i], bias), n_img, a.iters, a.reps, 20)
                    tc = timed(arm_c, n_cod, a.iters, a.reps, 20)
                    tb = timed(mm, n_cod, a.iters, a.reps, 20)
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, N=N, K=K, M=M, us_image=round(ta, 2),
                             us_decode_linear=round(tc, 2), us_mm=round(tb, 2), mm_codes_frac_8TBs=round(N * K / 2 / (tb * 1e-6) / 8e12, 4),
                             image_over_mm=round(ta / tb, 3), decode_linear_over_mm=round(tc / tb, 3))
                    if M <= _lib.LINEAR4_MAX_M:
                        r["us_linear4"] = round(timed(lambda i: _lib.linear4(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn,
                                                                            ovp=ovp, out=y), n_cod, a.iters, a.reps, 20), 2)
                    if a.tiles:
                        for nt in (1, 2, 4):
                            knob(22, nt)
                            r["us_mm_tiles%d" % nt] = round(timed(mm, n_cod, a.iters, a.reps, 20), 2)
                        knob(22, 0)
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                del images, codes, scratch
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
