#!/usr/bin/env python3
"""A/B of a byte-coded (8-bit) Linear layer's whole forward from a RAW input -- activation quantiser and product -- with 1 .. 4096
input rows: the protocol of tools/probe_int_linear4.py (same process, each arm rotating over distinct weight buffers, per point
`--reps` measurements of one captured graph of calls per arm, the arms ALTERNATED inside every repetition; the median and the
spread (max - min) / median are reported).

    I  antq_quant_i8 + antq_linear8_i8 on the byte codes                     (pack_model(integer_bytes=True))
    K  antq_quant_i8 + antq_linear8_i8_sk, at most 64 rows                   (... with integer_split_k); --force 1,2,4 adds one arm
       per forced number of slices (knob 24)
    R  antq_fakequant + today's byte route: antq_linear8 (M <= 8), antq_linear8_mm (M <= 64, 16-bit), antq_linear8_gemm (M <= 4096,
       16-bit); float32 beyond 8 rows has none
    C  antq_fakequant + antq_decode8 into one scratch buffer + F.linear
    A  antq_fakequant + F.linear on the kept image
    4  antq_quant_i8 + antq_linear4_i8 on 4-bit codes of the same shape (ANT int-4): the cost of the decode the byte form removes

Layers [N, K]: 4096 x 4096, 16384 x 4096, 4096 x 16384, 3072 x 768, 768 x 3072; float32 and bfloat16.  Books: ANT int-8 signed (the
XOR decode) and, with --table, ANT int-6 signed (the LDS table) on the first and fourth layer; the same book on both operands, one
scale per output row, one per input tensor, bias.

    python tools/probe_int_linear8.py [--table] [--force 1,2,4,8,16] [--layers 0,3] [--ms 1,64] --out profiles/int_linear8
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids, packed  # noqa: E402
from probe_linear4_t import ROTATE_BYTES, capture, alternate  # noqa: E402
from probe_int_linear4 import SHAPES, MS, _range  # noqa: E402

ARMS = (("K", "k"), ("R", "r"), ("C", "c"), ("A", "a"), ("4", "4"))


def write_md(rows, path, args):
    forced = sorted({int(k[5:]) for r in rows for k in r if k.startswith("us_k_")})
    out = ["# antq_quant_i8 + antq_linear8_i8 / antq_linear8_i8_sk against today's forwards of a byte-coded Linear layer", "",
           "Written by `tools/probe_int_linear8.py`: one MI355X, one process; every arm starts from the RAW input and rotates over "
           "distinct weight buffers; per point %d repetitions of one graph-replayed batch of calls per arm, the arms alternated inside a "
           "repetition; medians in us per call, `spread` = the largest (max - min) / median of the point's arms." % args.reps, "",
           "I = antq_quant_i8 + antq_linear8_i8, K = ... + antq_linear8_i8_sk with S slices by the launcher's rule (M <= 64), R = "
           "antq_fakequant + today's byte route (blank: none), C = antq_fakequant + antq_decode8 into scratch + F.linear, A = "
           "antq_fakequant + F.linear on the kept image, 4 = antq_quant_i8 + antq_linear4_i8 on 4-bit codes of the same shape.  B = the "
           "better of I and K.  B / X are TIMES: below 1, the byte-code integer path is faster.  TOP/s = 2 M N K over B's time.", ""]
    for dt, book in sorted({(r["dtype"], r["book"]) for r in rows}):
        rs = [r for r in rows if (r["dtype"], r["book"]) == (dt, book)]
        out += ["## Verdict in counts, %s, %s" % (dt, book), "", "| against | points | won | lost | B / X |", "|---|---|---|---|---|"]
        for o in "rca4":
            rr = [r for r in rs if r.get("b_over_" + o) is not None]
            if rr:
                out.append("| %s | %d | %d | %d | %s |" % (o.upper(), len(rr), sum(r["b_over_" + o] < 1 - r["spread"] for r in rr),
                                                         sum(r["b_over_" + o] > 1 + r["spread"] for r in rr), _range([r["b_over_" + o] for r in rr])))
        out += ["", "Per M, B / A: " + "; ".join("M = %d: %s" % (M, _range([r["b_over_a"] for r in rs if r["M"] == M]))
                                                  for M in sorted({r["M"] for r in rs})) + ".  B reaches %s TOP/s." % _range([r["tops"] for r in rs]), ""]
        out += ["| layer [N, K] | M | calls | I | K (S) | R | C | A | 4 | B / R | B / C | B / A | B / 4 | TOP/s |%s spread |" % "".join(" S = %d |" % f for f in forced),
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|%s---|" % ("---|" * len(forced))]
        f2 = lambda v, fmt="%.1f": "" if v is None else fmt % v
        for r in rs:
            out.append("| [%d, %d] | %d | %d | %.1f | %s | %s | %.1f | %.1f | %.1f | %s | %.2f | %.2f | %.2f | %.0f |%s %.1f %% |" % (
                r["N"], r["K"], r["M"], r["calls"], r["us_i"], "" if r["us_k"] is None else "%.1f (%d)" % (r["us_k"], r["slices"]),
                "" if r["us_r"] is None else "%.1f (%s)" % (r["us_r"], r["route"]), r["us_c"], r["us_a"], r["us_4"], f2(r["b_over_r"], "%.2f"),
                r["b_over_c"], r["b_over_a"], r["b_over_4"], r["tops"], "".join(" %s |" % f2(r.get("us_k_%d" % f)) for f in forced), 100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", action="store_true", help="the TABLE book (ANT int-6 signed) instead of the XOR book")
    ap.add_argument("--force", default="", help="numbers of slices to force as arms of their own at M <= 64, e.g. 1,2,4,8,16")
    ap.add_argument("--layers", default="0,1,2,3,4", help="indices into the five layers")
    ap.add_argument("--ms", default=",".join(str(m) for m in MS))
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--flop", type=float, default=3e11, help="operations per graph, about")
    ap.add_argument("--min-iters", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--notes", default=None, help="a markdown file appended to the .md: what the run does not say")
    ap.add_argument("--rewrite", default=None, help=".json files of earlier runs, comma separated: write their .md (no GPU needed) and stop")
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    a = ap.parse_args()
    if a.rewrite:
        rows = [r for p in a.rewrite.split(",") for r in json.load(open(p))]
        write_md(rows, (a.out or os.path.splitext(a.rewrite.split(",")[0])[0]) + ".md", a)
        return
    if not torch.cuda.is_available():
        raise SystemExit("probe_int_linear8: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    forced = [int(v) for v in a.force.split(",") if v]
    bname, g = ("ant int-6 (TABLE)", grids.ant_grid("int", 6, True)) if a.table else ("ant int-8 (XOR)", grids.ant_grid("int", 8, True))
    plan, gmax = _lib.plan_for(g), float(g.max())
    (I, image), img, gd = plan.integer_image8(), plan.image_dev(dev, 128), plan.grid_dev(dev)
    g4 = grids.ant_grid("int", 4, True)
    plan4, gmax4 = _lib.plan_for(g4), float(g4.max())
    I4, img4 = plan4.integer_image()[0], plan4.image_dev(dev)
    rows = []
    for dt in [getattr(torch, n) for n in a.dtypes.split(",")]:
        esz = torch.empty(0, dtype=dt).element_size()
        for N, K in [SHAPES[int(i)] for i in a.layers.split(",")]:
            w = (torch.randn(N, K, device=dev) * 0.05).to(dt)
            alpha = (w.float().abs().amax(1) * 0.9).contiguous()
            codes0 = _lib.encode8(w, alpha, plan, gmax, N, K, True)
            codes40 = _lib.encode4(w, alpha, plan4, gmax4, N, K, True)
            image0 = _lib.decode8(codes0, alpha, plan, gmax, N, K, True, dt).view(N, K)
            del w
            unit_w, unit_w4 = packed._unit_alpha(alpha, plan, gmax), packed._unit_alpha(alpha, plan4, gmax4)
            scratch = torch.empty(N * K, dtype=dt, device=dev)
            bias = torch.randn(N, device=dev).to(dt)
            for M in [int(m) for m in a.ms.split(",")]:
                iters = int(min(a.max_iters, max(a.min_iters, a.flop / (2.0 * M * N * K))))
                n_img = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N * esz)))))
                n_cod = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N)))))
                images = [image0.clone() for _ in range(n_img)]
                codes = [codes0.clone() for _ in range(n_cod)]
                codes4 = [codes40.clone() for _ in range(n_cod)]
                x = torch.randn(M, K, device=dev).to(dt)
                ax = (x.float().abs().max() * 0.9).reshape(1).contiguous()
                unit_x, unit_x4 = packed._unit_alpha(ax, plan, gmax), packed._unit_alpha(ax, plan4, gmax4)
                xq, xf = torch.empty(M, K, dtype=torch.int8, device=dev), torch.empty_like(x)
                y = torch.empty(M, N, dtype=dt, device=dev)
                ws = torch.empty(16 * 4 * min(M, 64) * N, dtype=torch.uint8, device=dev)
                half = dt != torch.float32
                route = ("linear8" if M <= _lib.LINEAR8_MAX_M else "linear8_mm" if half and M <= _lib.LINEAR8_MM_MAX_M
                         else "linear8_gemm" if half and M <= _lib.LINEAR8_GEMM_MAX_M else None)
                fq = lambda: _lib.fakequant(x, ax, plan, gmax, 1, M * K, False, out=xf)
                q8 = lambda: _lib.quant_i8(x, ax, plan, gmax, 1, M * K, False, img, out=xq)

                def arm_i(i):
                    q8()
                    return _lib.int_linear8(codes[i], xq, unit_w, img, image, I, unit_x, I, N, K, True, dt, bias=bias, out=y)

                def arm_k(i, S=0):
                    q8()
                    _lib.lib().antq_debug_set(24, S)
                    try:
                        return _lib.int_linear8_sk(codes[i], xq, unit_w, img, image, I, unit_x, I, N, K, True, dt, bias=bias, out=y, workspace=ws)
                    finally:
                        _lib.lib().antq_debug_set(24, 0)

                def arm_r(i):
                    fq()
                    return getattr(_lib, route)(codes[i], xf, alpha, gd, gmax, N, K, True, bias=bias, out=y)

                def arm_c(i):
                    fq()
                    _lib.decode8(codes[i], alpha, plan, gmax, N, K, True, dt, out=scratch)
                    return F.linear(xf, scratch.view(N, K), bias)

                def arm_a(i):
                    fq()
                    return F.linear(xf, images[i], bias)

                def arm_4(i):
                    _lib.quant_i8(x, ax, plan4, gmax4, 1, M * K, False, img4, out=xq)
                    return _lib.int_linear4(codes4[i], xq, unit_w4, img4, I4, unit_x4, I4, N, K, True, dt, bias=bias, out=y)

                graphs = {"I": capture(arm_i, n_cod, iters, 3), "C": capture(arm_c, n_cod, iters, 3), "A": capture(arm_a, n_img, iters, 3),
                          "4": capture(arm_4, n_cod, iters, 3)}
                if route:
                    graphs["R"] = capture(arm_r, n_cod, iters, 3)
                if M <= _lib.LINEAR8_I8_SK_MAX_M:
                    graphs["K"] = capture(arm_k, n_cod, iters, 3)
                    for S in forced:
                        graphs["K%d" % S] = capture(lambda i, S=S: arm_k(i, S), n_cod, iters, 3)
                t = alternate(graphs, iters, a.reps)
                us = {k: v[0] for k, v in t.items()}
                best = min(us["I"], us.get("K", us["I"]))
                r = dict(dtype=str(dt).split(".")[1], book=bname, N=N, K=K, M=M, calls=iters, image_buffers=n_img, code_buffers=n_cod, route=route,
                         us_i=round(us["I"], 2), slices=_lib.lib().antq_linear8_i8_sk_slices(M, N, K, 0) if "K" in us else None,
                         **{"us_" + lo: round(us[up], 2) if up in us else None for up, lo in ARMS},
                         **{"b_over_" + lo: round(best / us[up], 3) if up in us else None for up, lo in ARMS[1:]},
                         **{"us_k_%d" % S: round(us["K%d" % S], 2) for S in forced if "K%d" % S in us},
                         tops=round(2.0 * M * N * K / (best * 1e-6) / 1e12, 1), spread=round(max(v[1] for v in t.values()), 4))
                rows.append(r)
                print(json.dumps(r), flush=True)
                del graphs, images, codes, codes4
            del scratch
            torch.cuda.empty_cache()
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out + ".json", "w") as f:
                    json.dump(rows, f, indent=1)
                write_md(rows, a.out + ".md", a)


if __name__ == "__main__":
    main()
