#!/usr/bin/env python3
"""A/B of a packed GPT-2 Conv1D layer (weight [K, N], y = x @ W + b) with 64 .. 4096 input rows, the protocol of
profiles/packed_linear_t_mm.md: same process, each arm rotating over distinct weight buffers, per point `--reps` measurements of one
captured graph of calls per arm, the arms ALTERNATED inside every repetition; the median and the spread (max - min) / median
are reported.

    A  torch.addmm on the decoded image                         (a packed model that keeps its images)
    C  antq_decode4 into one scratch buffer, then torch.addmm   (the keep_images=False path of a call no kernel serves)
    B  antq_linear4_t_gemm on the codes                         (the launcher's tile rule)
    T  antq_linear4_t_mm on the codes, at M = 64 only
    B2 / B4  B with 2 / 4 wavefronts per workgroup forced (antq_debug_set key 23), at M = 256 and 1024 only

Layers: GPT-2 small's and GPT-2 XL's four Conv1D shapes, bf16 / f16, ANT flint-4 and OliVe flint + outliers, one scale per row k
of the codes, M in {64, 65, 128, 256, 1024, 4096}.  A graph holds as many calls as make about `--flop` floating-point
operations, between `--min-iters` and `--max-iters`.

    python tools/probe_linear4_t_gemm.py [--quick] [--out profiles/packed_linear_t_gemm]      (writes .json and .md)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib  # noqa: E402
from probe_linear4_t import SHAPES, ROTATE_BYTES, books, capture, alternate  # noqa: E402

MS = (64, 65, 128, 256, 1024, 4096)
TILE_MS = (256, 1024)


def _range(v):
    return "%.2f ... %.2f" % (min(v), max(v))


def write_md(rows, path, args):
    out = ["# antq_linear4_t_gemm against addmm on the image and against decode + addmm", "",
           "Written by `tools/probe_linear4_t_gemm.py%s`: one MI355X, one process, one run; every arm rotates over distinct weight "
           "buffers; per point %d repetitions of one graph-replayed batch of calls per arm, the arms alternated inside a "
           "repetition; medians in us per call, `spread` = the largest (max - min) / median of the point's arms." % (
               " --quick" if args.quick else "", args.reps), "",
           "A = torch.addmm on the kept image, C = antq_decode4 into scratch + torch.addmm, B = antq_linear4_t_gemm on the codes, "
           "T = antq_linear4_t_mm on the codes (M = 64 only).  One scale per row k, bias.  B / C and B / A are TIMES: below 1, B is "
           "faster.  TFLOP/s = 2 M N K over B's time.", ""]
    if rows:
        n = len(rows)
        out += ["## Verdict in counts", "",
                "B is faster than C at %d of %d points (B / C %s), faster than A at %d of %d (B / A %s)." % (
                    sum(r["b_over_c"] < 1 for r in rows), n, _range([r["b_over_c"] for r in rows]),
                    sum(r["b_over_a"] < 1 for r in rows), n, _range([r["b_over_a"] for r in rows])),
                "Per M, B / C and B / A: " + "; ".join("M = %d: %s and %s" % (
                    M, _range([r["b_over_c"] for r in rows if r["M"] == M]), _range([r["b_over_a"] for r in rows if r["M"] == M]))
                    for M in MS if any(r["M"] == M for r in rows)) + ".",
                "B reaches %s TFLOP/s.  The largest spread of a point is %.1f %%." % (
                    _range([r["tflops"] for r in rows]), 100 * max(r["spread"] for r in rows)), ""]
        t = [r for r in rows if r.get("us_t_mm") is not None]
        if t:
            out += ["At M = 64, B / T (antq_linear4_t_mm) is %s: B is faster at %d of %d points." % (
                _range([r["b_over_t"] for r in t]), sum(r["b_over_t"] < 1 for r in t), len(t)), ""]
        tl = [r for r in rows if r.get("us_b2") is not None]
        if tl:
            agree = sum((r["us_b2"] <= r["us_b4"]) == (r["rule_waves"] == 2) for r in tl)
            out += ["## The tile height: 2 against 4 wavefronts per workgroup, forced, against the rule", "",
                    "The rule (`gemm_waves`) picked the faster forced shape at %d of %d points; B4 / B2 is %s." % (
                        agree, len(tl), _range([r["us_b4"] / r["us_b2"] for r in tl])), "",
                    "| dtype, book | layer [K, N] | M | B2 | B4 | rule | B (rule) |", "|---|---|---|---|---|---|---|"]
            out += ["| %s, %s | %s [%d, %d] | %d | %.1f | %.1f | %d | %.1f |" % (
                r["dtype"], r["book"], r["layer"], r["K"], r["N"], r["M"], r["us_b2"], r["us_b4"], r["rule_waves"], r["us_b"]) for r in tl] + [""]
    keys = []
    for r in rows:
        if (r["dtype"], r["book"]) not in keys:
            keys.append((r["dtype"], r["book"]))
    for dt, book in keys:
        out += ["## %s, %s" % (dt, book), "", "| layer [K, N] | M | calls | A | C | B | T | B / C | B / A | TFLOP/s | spread |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            if (r["dtype"], r["book"]) == (dt, book):
                out.append("| %s [%d, %d] | %d | %d | %.1f | %.1f | %.1f | %s | %.2f | %.2f | %.0f | %.1f %% |" % (
                    r["layer"], r["K"], r["N"], r["M"], r["calls"], r["us_a"], r["us_c"], r["us_b"],
                    "" if r.get("us_t_mm") is None else "%.1f" % r["us_t_mm"], r["b_over_c"], r["b_over_a"], r["tflops"], 100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, OliVe, GPT-2 small only")
    ap.add_argument("--flop", type=float, default=1.5e12, help="floating-point operations per graph, about")
    ap.add_argument("--min-iters", type=int, default=8)
    ap.add_argument("--max-iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--notes", default=None, help="a markdown file appended to the .md: what the run does not say")
    ap.add_argument("--rewrite", default=None, help="a .json of an earlier run: write its .md again (no GPU needed) and stop")
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    a = ap.parse_args()
    if a.rewrite:
        write_md(json.load(open(a.rewrite)), (a.out or os.path.splitext(a.rewrite)[0]) + ".md", a)
        return
    if not torch.cuda.is_available():
        raise SystemExit("probe_linear4_t_gemm: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    knob = _lib.lib().antq_debug_set
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.bfloat16, torch.float16)):
        esz = torch.empty(0, dtype=dt).element_size()
        for bname, g, gmax, nn, ovp in (books()[1:] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, K, N in (SHAPES[:4] if a.quick else SHAPES):
                w = (torch.randn(K, N, device=dev) * 0.05).to(dt)
                if ovp:
                    w.view(-1)[::997] *= 12
                alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
                codes0 = _lib.encode4(w, alpha, plan, gmax, K, N, True, n_normal=nn, ovp=ovp)
                image0 = _lib.decode4(codes0, alpha, plan, gmax, K, N, True, dt, n_normal=nn, ovp=ovp).view(K, N)
                del w
                scratch = torch.empty(K * N, dtype=dt, device=dev)
                bias = torch.randn(N, device=dev).to(dt)
                for M in MS:
                    iters = int(min(a.max_iters, max(a.min_iters, a.flop / (2.0 * M * N * K))))
                    n_img = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N * esz)))))
                    images = [image0.clone() for _ in range(n_img)]
                    codes = [codes0.clone() for _ in range(iters)]
                    x = torch.randn(M, K, device=dev).to(dt)
                    y = torch.empty(M, N, dtype=dt, device=dev)

                    def arm_c(i):
                        _lib.decode4(codes[i], alpha, plan, gmax, K, N, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                        return torch.addmm(bias, x, scratch.view(K, N))

                    gemm = lambda i: _lib.linear4_t_gemm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
                    graphs = {"A": capture(lambda i: torch.addmm(bias, x, images[i]), n_img, iters, 3), "C": capture(arm_c, iters, iters, 3),
                              "B": capture(gemm, iters, iters, 3)}
                    if M <= _lib.LINEAR4_T_MM_MAX_M:
                        graphs["T"] = capture(lambda i: _lib.linear4_t_mm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y),
                                              iters, iters, 3)
                    if M in TILE_MS:
                        for wv in (2, 4):       # (a captured launch keeps the kernel it was captured with)
                            knob(23, wv)
                            try:
                                graphs["B%d" % wv] = capture(gemm, iters, iters, 3)
                            finally:
                                knob(23, 0)
                    t = alternate(graphs, iters, a.reps)
                    us = {k: v[0] for k, v in t.items()}
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, K=K, N=N, M=M, calls=iters, image_buffers=n_img,
                             us_a=round(us["A"], 2), us_c=round(us["C"], 2), us_b=round(us["B"], 2),
                             us_t_mm=round(us["T"], 2) if "T" in us else None, us_b2=round(us["B2"], 2) if "B2" in us else None,
                             us_b4=round(us["B4"], 2) if "B4" in us else None,
                             rule_waves=2 if -(-N // 64) * -(-M // 128) <= 256 else 4,
                             b_over_c=round(us["B"] / us["C"], 3), b_over_a=round(us["B"] / us["A"], 3),
                             b_over_t=round(us["B"] / us["T"], 3) if "T" in us else None,
                             tflops=round(2.0 * M * N * K / (us["B"] * 1e-6) / 1e12, 1), spread=round(max(v[1] for v in t.values()), 4))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del graphs, images, codes
                del scratch
                torch.cuda.empty_cache()
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out + ".json", "w") as f:
                        json.dump(rows, f, indent=1)
                    write_md(rows, a.out + ".md", a)


if __name__ == "__main__":
    main()
