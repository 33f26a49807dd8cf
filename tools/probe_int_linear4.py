#!/usr/bin/env python3
"""A/B of a packed 4-bit Linear layer's whole forward from a RAW input -- activation quantiser and product -- with 1 .. 4096 input
rows, the protocol of profiles/packed_linear_t_mm.md: same process, each arm rotating over distinct weight buffers (more than 256 MiB
where the shape allows), per point `--reps` measurements of one captured graph of calls per arm, the arms ALTERNATED inside every
repetition; the median and the spread (max - min) / median are reported.

    I  antq_quant_i8 + antq_linear4_i8 on the codes                          (pack_model(integer_linear=True))
    R  antq_fakequant + today's route on the codes: antq_linear4 (M <= 8), antq_linear4_mm (M <= 64, 16-bit), antq_linear4_gemm
       (M <= 4096, 16-bit); float32 beyond 8 rows has none
    C  antq_fakequant + antq_decode4 into one scratch buffer + F.linear      (keep_images=False, a call no kernel serves)
    A  antq_fakequant + F.linear on the kept image
    K  (--split-k) antq_quant_i8 + antq_linear4_i8_sk: K split across workgroups, at most 64 rows.  The rows are then 1, 8, 16, 64,
       the tables compare K with every other arm, and --force 1,2,4,8,16 adds one arm per forced number of slices (knob 24)

Layers [N, K]: 4096 x 4096, 16384 x 4096, 4096 x 16384, 3072 x 768, 768 x 3072; float32 and bfloat16; ANT flint-4 (signed) and OliVe
int-4 with its outlier list, the same book on both operands, one scale per output row, one per input tensor, bias.

    python tools/probe_int_linear4.py [--quick] [--out profiles/int_linear4]      (writes .json and .md)
    python tools/probe_int_linear4.py --split-k [--force 1,2,4,8,16] [--quick] --out profiles/int_linear4_sk
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids, packed  # noqa: E402
from probe_linear4_t import ROTATE_BYTES, capture, alternate  # noqa: E402

SHAPES = ((4096, 4096), (16384, 4096), (4096, 16384), (3072, 768), (768, 3072))
MS = (1, 8, 64, 512, 4096)
MS_SK = (1, 8, 16, 64)


def books():
    g = grids.ant_flint(4, True)
    gn, go = grids.olive_int(4, True), grids.olive_outliers(4, True)
    return [("ant flint-4", g, float(g.max()), 0, False), ("olive int-4 + outliers", np.concatenate([gn, go]), float(gn.max()), int(gn.size), True)]


def _range(v):
    return "%.2f ... %.2f" % (min(v), max(v))


def write_md(rows, path, args):
    out = ["# antq_quant_i8 + antq_linear4_i8 against today's forwards of a packed 4-bit Linear layer", "",
           "Written by `tools/probe_int_linear4.py%s`: one MI355X, one process, one run; every arm starts from the RAW input and rotates "
           "over distinct weight buffers; per point %d repetitions of one graph-replayed batch of calls per arm, the arms alternated "
           "inside a repetition; medians in us per call, `spread` = the largest (max - min) / median of the point's arms." % (
               " --quick" if args.quick else "", args.reps), "",
           "I = antq_quant_i8 + antq_linear4_i8, R = antq_fakequant + today's route on the codes (blank: none), C = antq_fakequant + "
           "antq_decode4 into scratch + F.linear, A = antq_fakequant + F.linear on the kept image.  I / R, I / C and I / A are TIMES: "
           "below 1, I is faster.  TOP/s = 2 M N K over I's time (quantiser included).", ""]
    if rows:
        for dt in sorted({r["dtype"] for r in rows}):
            rs = [r for r in rows if r["dtype"] == dt]
            rr = [r for r in rs if r["us_r"] is not None]
            out += ["## Verdict in counts, %s" % dt, "",
                    "I is faster than A at %d of %d points (I / A %s), than C at %d of %d (I / C %s)%s." % (
                        sum(r["i_over_a"] < 1 for r in rs), len(rs), _range([r["i_over_a"] for r in rs]),
                        sum(r["i_over_c"] < 1 for r in rs), len(rs), _range([r["i_over_c"] for r in rs]),
                        ", than R at %d of %d (I / R %s)" % (sum(r["i_over_r"] < 1 for r in rr), len(rr), _range([r["i_over_r"] for r in rr])) if rr else ""),
                    "Per M, I / A: " + "; ".join("M = %d: %s" % (M, _range([r["i_over_a"] for r in rs if r["M"] == M]))
                                                 for M in MS if any(r["M"] == M for r in rs)) + ".",
                    "I reaches %s TOP/s.  The largest spread of a point is %.1f %%." % (
                        _range([r["tops"] for r in rs]), 100 * max(r["spread"] for r in rs)), ""]
    keys = []
    for r in rows:
        if (r["dtype"], r["book"]) not in keys:
            keys.append((r["dtype"], r["book"]))
    for dt, book in keys:
        out += ["## %s, %s" % (dt, book), "", "| layer [N, K] | M | calls | I | R | C | A | I / R | I / C | I / A | TOP/s | spread |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            if (r["dtype"], r["book"]) == (dt, book):
                out.append("| [%d, %d] | %d | %d | %.1f | %s | %.1f | %.1f | %s | %.2f | %.2f | %.0f | %.1f %% |" % (
                    r["N"], r["K"], r["M"], r["calls"], r["us_i"], "" if r["us_r"] is None else "%.1f (%s)" % (r["us_r"], r["route"]),
                    r["us_c"], r["us_a"], "" if r["us_r"] is None else "%.2f" % r["i_over_r"], r["i_over_c"], r["i_over_a"], r["tops"],
                    100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def write_md_sk(rows, path, args):
    """the --split-k form: K against I, R, C and A (times of K over the other arm's: below 1, K is faster)"""
    others = ("i", "r", "c", "a")
    out = ["# antq_quant_i8 + antq_linear4_i8_sk (K split across workgroups) at 1 ... 64 rows", "",
           "Written by `tools/probe_int_linear4.py --split-k%s%s`: the protocol of profiles/int_linear4.md (one MI355X, one process, every "
           "arm from the RAW input, rotating weight buffers, %d repetitions of one graph-replayed batch of calls per arm, the arms "
           "alternated inside a repetition; medians in us per call, `spread` = the largest (max - min) / median of the point's arms)." % (
               " --quick" if args.quick else "", " --force " + args.force if args.force else "", args.reps), "",
           "K = antq_quant_i8 + antq_linear4_i8_sk with S slices by the launcher's rule; I, R, C, A as in profiles/int_linear4.md.  "
           "K / X are TIMES: below 1, K is faster.  `won` counts the points where K is faster by more than the point's spread, "
           "`lost` those where it is slower by more than it.", ""]
    for dt in sorted({r["dtype"] for r in rows}):
        rs = [r for r in rows if r["dtype"] == dt]
        out += ["## Verdict in counts, %s" % dt, "", "| against | points | won | lost | K / X |", "|---|---|---|---|---|"]
        for o in others:
            rr = [r for r in rs if r.get("k_over_" + o) is not None]
            if rr:
                out.append("| %s | %d | %d | %d | %s |" % (o.upper(), len(rr), sum(r["k_over_" + o] < 1 - r["spread"] for r in rr),
                                                         sum(r["k_over_" + o] > 1 + r["spread"] for r in rr), _range([r["k_over_" + o] for r in rr])))
        out += ["", "Per M, K / I: " + "; ".join("M = %d: %s" % (M, _range([r["k_over_i"] for r in rs if r["M"] == M]))
                                                  for M in MS_SK if any(r["M"] == M for r in rs)) + ".", ""]
    forced = sorted({int(k[5:]) for r in rows for k in r if k.startswith("us_k_")})
    keys = []
    for r in rows:
        if (r["dtype"], r["book"]) not in keys:
            keys.append((r["dtype"], r["book"]))
    for dt, book in keys:
        out += ["## %s, %s" % (dt, book), "",
                "| layer [N, K] | M | S | K | I | R | C | A | K / I | K / R | K / C | K / A |%s spread |" % "".join(" S = %d |" % f for f in forced),
                "|---|---|---|---|---|---|---|---|---|---|---|---|%s---|" % ("---|" * len(forced))]
        for r in rows:
            if (r["dtype"], r["book"]) == (dt, book):
                out.append("| [%d, %d] | %d | %d | %.1f | %.1f | %s | %.1f | %.1f | %.2f | %s | %.2f | %.2f |%s %.1f %% |" % (
                    r["N"], r["K"], r["M"], r["slices"], r["us_k"], r["us_i"], "" if r["us_r"] is None else "%.1f" % r["us_r"], r["us_c"],
                    r["us_a"], r["k_over_i"], "" if r["us_r"] is None else "%.2f" % r["k_over_r"], r["k_over_c"], r["k_over_a"],
                    "".join(" %.1f |" % r["us_k_%d" % f] for f in forced), 100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split-k", action="store_true", help="add arm K (antq_linear4_i8_sk) at 1, 8, 16, 64 rows; K's tables")
    ap.add_argument("--force", default="", help="(--split-k) numbers of slices to force as arms of their own, e.g. 1,2,4,8,16")
    ap.add_argument("--quick", action="store_true", help="bfloat16, ANT flint-4, the first and the fourth layer only")
    ap.add_argument("--flop", type=float, default=3e11, help="operations per graph, about")
    ap.add_argument("--min-iters", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--notes", default=None, help="a markdown file appended to the .md: what the run does not say")
    ap.add_argument("--rewrite", default=None, help="a .json of an earlier run: write its .md again (no GPU needed) and stop")
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    a = ap.parse_args()
    md = write_md_sk if a.split_k else write_md
    forced = [int(v) for v in a.force.split(",") if v]
    if a.rewrite:
        md(json.load(open(a.rewrite)), (a.out or os.path.splitext(a.rewrite)[0]) + ".md", a)
        return
    if not torch.cuda.is_available():
        raise SystemExit("probe_int_linear4: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.float32, torch.bfloat16)):
        esz = torch.empty(0, dtype=dt).element_size()
        for bname, g, gmax, nn, ovp in (books()[:1] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd, img = plan.grid_dev(dev), plan.image_dev(dev)
            I = plan.integer_image()[0]
            for N, K in (SHAPES[::3] if a.quick else SHAPES):
                w = (torch.randn(N, K, device=dev) * 0.05).to(dt)
                if ovp:
                    w.view(-1)[::997] *= 12
                alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
                codes0 = _lib.encode4(w, alpha, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
                image0 = _lib.decode4(codes0, alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp).view(N, K)
                del w
                unit_w = packed._unit_alpha(alpha, plan, gmax)
                scratch = torch.empty(N * K, dtype=dt, device=dev)
                bias = torch.randn(N, device=dev).to(dt)
                for M in (MS_SK if a.split_k else MS):
                    iters = int(min(a.max_iters, max(a.min_iters, a.flop / (2.0 * M * N * K))))
                    n_img = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N * esz)))))
                    n_cod = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N // 2)))))
                    images = [image0.clone() for _ in range(n_img)]
                    codes = [codes0.clone() for _ in range(n_cod)]
                    x = torch.randn(M, K, device=dev).to(dt)
                    if ovp:
                        x.view(-1)[::499] *= 12
                    ax = (x.float().abs().max() * 0.9 if not ovp else 3 * x.float().std()).reshape(1).contiguous()
                    unit_x = packed._unit_alpha(ax, plan, gmax)
                    xq, xf = torch.empty(M, K, dtype=torch.int8, device=dev), torch.empty_like(x)
                    y = torch.empty(M, N, dtype=dt, device=dev)
                    half = dt != torch.float32
                    route = ("linear4" if M <= _lib.LINEAR4_MAX_M else "linear4_mm" if half and M <= _lib.LINEAR4_MM_MAX_M
                             else "linear4_gemm" if half and M <= _lib.LINEAR4_GEMM_MAX_M else None)
                    fq = lambda: _lib.fakequant(x, ax, plan, gmax, 1, M * K, False, ovp=ovp, out=xf)

                    def arm_i(i):
                        _lib.quant_i8(x, ax, plan, gmax, 1, M * K, False, img, n_normal=nn, ovp=ovp, out=xq)
                        return _lib.int_linear4(codes[i], xq, unit_w, img, I, unit_x, I, N, K, True, dt, bias=bias, n_normal=nn, ovp=ovp, out=y)

                    def arm_r(i):
                        fq()
                        return getattr(_lib, route)(codes[i], xf, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)

                    def arm_c(i):
                        fq()
                        _lib.decode4(codes[i], alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                        return F.linear(xf, scratch.view(N, K), bias)

                    def arm_a(i):
                        fq()
                        return F.linear(xf, images[i], bias)

                    def arm_k(i, S=0):
                        _lib.quant_i8(x, ax, plan, gmax, 1, M * K, False, img, n_normal=nn, ovp=ovp, out=xq)
                        _lib.lib().antq_debug_set(24, S)
                        try:
                            return _lib.int_linear4_sk(codes[i], xq, unit_w, img, I, unit_x, I, N, K, True, dt, bias=bias, n_normal=nn, ovp=ovp,
                                                       out=y, workspace=ws)
                        finally:
                            _lib.lib().antq_debug_set(24, 0)

                    graphs = {"I": capture(arm_i, n_cod, iters, 3), "C": capture(arm_c, n_cod, iters, 3), "A": capture(arm_a, n_img, iters, 3)}
                    if route:
                        graphs["R"] = capture(arm_r, n_cod, iters, 3)
                    if a.split_k:
                        ws = torch.empty(16 * 4 * M * N, dtype=torch.uint8, device=dev)
                        graphs["K"] = capture(arm_k, n_cod, iters, 3)
                        for S in forced:
                            graphs["K%d" % S] = capture(lambda i, S=S: arm_k(i, S), n_cod, iters, 3)
                    t = alternate(graphs, iters, a.reps)
                    us = {k: v[0] for k, v in t.items()}
                    r = dict(dtype=str(dt).split(".")[1], book=bname, N=N, K=K, M=M, calls=iters, image_buffers=n_img, code_buffers=n_cod,
                             route=route, us_i=round(us["I"], 2), us_r=round(us["R"], 2) if route else None, us_c=round(us["C"], 2),
                             us_a=round(us["A"], 2), i_over_r=round(us["I"] / us["R"], 3) if route else None,
                             i_over_c=round(us["I"] / us["C"], 3), i_over_a=round(us["I"] / us["A"], 3),
                             tops=round(2.0 * M * N * K / (us["I"] * 1e-6) / 1e12, 1), spread=round(max(v[1] for v in t.values()), 4))
                    if a.split_k:
                        r.update(slices=_lib.lib().antq_linear4_i8_sk_slices(M, N, K, 0), us_k=round(us["K"], 2),
                                 **{"k_over_" + o.lower(): round(us["K"] / us[o], 3) if o in us else None for o in "IRCA"},
                                 **{"us_k_%d" % S: round(us["K%d" % S], 2) for S in forced})
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del graphs, images, codes
                del scratch
                torch.cuda.empty_cache()
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out + ".json", "w") as f:
                        json.dump(rows, f, indent=1)
                    md(rows, a.out + ".md", a)


if __name__ == "__main__":
    main()
