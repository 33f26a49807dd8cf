#!/usr/bin/env python3
"""A/B of a packed Linear layer with few input rows: F.linear on the decoded image (arm A, what a packed model did before)
against antq_linear4 on the codes (arm B), same process, event-timed.

Layers: OPT-6.7B's three Linear shapes and BERT-base's two, bf16 and fp32, M in {1, 2, 4, 8}, ANT flint-4 and OliVe flint +
outliers.  Each arm rotates over enough distinct weight buffers that the rotation exceeds the 256 MB Infinity Cache several
times (so every call streams its weights from HBM), warms up, then times `--iters` calls between two events; the median of
`--reps` such measurements is reported.  The calls are timed twice: replayed from one captured graph of `--iters` calls
(`us_*`: the kernels alone -- antq_linear4's Python wrapper checks a dozen tensor properties per call, which at a few
microseconds of kernel would be what an eager loop measures) and issued eagerly (`us_*_eager`: what a Python caller sees).
Bytes per second -- of the image for arm A, of the codes for arm B -- are given as a fraction of 8 TB/s, from the graph times.

    python tools/probe_linear4.py [--quick] [--out profiles/packed_linear.json]
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


def books():
    g = grids.ant_flint(4, True)
    gn, go = grids.olive_flint(4, True), grids.olive_outliers(4, True)
    return [("ant flint-4", g, float(g.max()), 0, False), ("olive flint+outliers", np.concatenate([gn, go]), float(gn.max()), int(gn.size), True)]


def _median_us(run, iters, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return float(np.median(out))


def timed(fn, n_buf, iters, reps, warm):
    """(us per call replayed from a graph of `iters` calls, us per call issued eagerly)"""
    def loop():
        for i in range(iters):
            fn(i % n_buf)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(warm):
            fn(i % n_buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = _median_us(loop, iters, reps)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop()
    graph.replay()
    torch.cuda.synchronize()
    return _median_us(graph.replay, iters, reps), eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, the OPT shapes, ANT only")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.bfloat16, torch.float32)):
        for bname, g, gmax, nn, ovp in (books()[:1] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, N, K in (SHAPES[:3] if a.quick else SHAPES):
                esz = 2 if dt == torch.bfloat16 else 4
                n_img = max(2, -(-ROTATE_BYTES // (N * K * esz)))
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
                bias = torch.randn(N, device=dev).to(dt)
                for M in (1, 2, 4, 8):
                    x = torch.randn(M, K, device=dev).to(dt)
                    y = torch.empty(M, N, dtype=dt, device=dev)
                    ta = timed(lambda i: F.linear(x, images[i], bias), n_img, a.iters, a.reps, 20)
                    tb = timed(lambda i: _lib.linear4(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y),
                               n_cod, a.iters, a.reps, 20)
                    (ta, ta_eager), (tb, tb_eager) = ta, tb
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, N=N, K=K, M=M, us_image=round(ta, 2), us_codes=round(tb, 2),
                             us_image_eager=round(ta_eager, 2), us_codes_eager=round(tb_eager, 2),
                             image_frac_8TBs=round(N * K * esz / (ta * 1e-6) / 8e12, 4), codes_frac_8TBs=round(N * K / 2 / (tb * 1e-6) / 8e12, 4),
                             speedup=round(ta / tb, 3))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                del images, codes
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
