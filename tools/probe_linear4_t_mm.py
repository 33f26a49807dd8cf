#!/usr/bin/env python3
"""A/B of a packed GPT-2 Conv1D layer (weight [K, N], y = x @ W + b) with 8 .. 64 input rows, the protocol of
profiles/packed_linear_t.md: same process, each arm rotating over enough distinct weight buffers to exceed the 256 MiB Infinity
Cache so that every call streams its weights from HBM, per point `--reps` measurements of one captured graph of calls per arm,
the arms ALTERNATED inside every repetition; the median and the spread (max - min) / median are reported.

    A  torch.addmm on the decoded image                         (a packed model that keeps its images: today's path)
    C  antq_decode4 into one scratch buffer, then torch.addmm   (the keep_images=False path for calls that do not qualify)
    B  antq_linear4_t_mm on the codes
    T  antq_linear4_t on the codes, at M = 8 only               (the row kernel that keeps the calls of at most 8 rows)

Layers: GPT-2 small's and GPT-2 XL's four Conv1D shapes, bf16 / f16, ANT flint-4 and OliVe flint + outliers, one scale per row k
of the codes, M in {8, 9, 16, 32, 64}.  The number of calls per graph follows the layer: at least `--iters`, and as many as it
takes for the codes touched by one replay to exceed the cache (capped at `--max-iters`).

    python tools/probe_linear4_t_mm.py [--quick] [--out profiles/packed_linear_t_mm]      (writes .json and .md)
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib  # noqa: E402
from probe_linear4_t import SHAPES, ROTATE_BYTES, HBM_BYTES_PER_S, books, capture, alternate  # noqa: E402

MS = (8, 9, 16, 32, 64)

RESOURCES = """| T | M tiles | VGPRs | AGPRs | SGPRs | LDS bytes | scratch | spills | waves / SIMD (by registers) |
|---|---|---|---|---|---|---|---|---|
%s
"""


def resources_table(path):
    """the table of the kernel's instantiations from the compiler's remarks saved in `path` (None: not available)"""
    if not path or not os.path.exists(path):
        return None
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: _ZN4antq13k_linear_t_mmI(\S+?)Lb([01])ELi(\d)ELi(\d)EEE", line)
        if m:
            cur = dict(T={"NS_8bf16_tagE": "bf16", "NS_7f16_tagE": "f16"}.get(m.group(1), m.group(1)), ovp=int(m.group(2)), MT=int(m.group(3)),
                       pairs=int(m.group(4)))
            rows.append(cur)
            continue
        if "Function Name:" in line:
            cur = None
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def _ratio_rows(rows, over, title):
    """per layer and M: min ... max of `over` (a key of the rows: an arm's time over B's) and B's wins, over all runs"""
    out = [title, "", "| layer [K, N] | " + " | ".join("M = %d" % M for M in MS) + " |", "|---|" + "---|" * len(MS)]
    seen = []
    for r in rows:
        k = (r["layer"], r["K"], r["N"])
        if k in seen:
            continue
        seen.append(k)
        cells = []
        for M in MS:
            v = [q[over] for q in rows if (q["layer"], q["K"], q["N"]) == k and q["M"] == M and q.get(over) is not None]
            cells.append("%.2f ... %.2f (%d of %d)" % (min(v), max(v), sum(x > 1 for x in v), len(v)) if v else "")
        out.append("| %s [%d, %d] | %s |" % (k[0], k[1], k[2], " | ".join(cells)))
    out.append("")
    return out


def write_md(rows, path, args, static):
    out = ["# antq_linear4_t_mm against addmm on the image, against decode + addmm and against antq_linear4_t", "",
           "Written by `tools/probe_linear4_t_mm.py%s`: one MI355X, one process, one run; every arm rotates over distinct weight "
           "buffers (more than 256 MiB touched per replay where %d calls reach that, see `calls`); per point %d repetitions of one "
           "graph-replayed batch of calls per arm, the arms alternated inside a repetition; medians in us per call, `spread` = the "
           "largest (max - min) / median of the point's arms." % ((" --quick" if args.quick else "") + (" --all-shapes" if args.all_shapes else ""), args.max_iters, args.reps), "",
           "A = torch.addmm on the kept image, C = antq_decode4 into scratch + torch.addmm (the `keep_images=False` path of a call "
           "that does not qualify), B = antq_linear4_t_mm on the codes, T = antq_linear4_t on the codes (M = 8 only).  One scale per "
           "row k, bias.  `% of 8 TB/s` = K N / 2 bytes of codes over B's time.", ""]
    keys = []
    for r in rows:
        k = (r["dtype"], r["book"])
        if k not in keys:
            keys.append(k)
    if rows:
        n = len(rows)
        wa, wc = sum(r["image_over_mm"] > 1 for r in rows), sum(r["decode_addmm_over_mm"] > 1 for r in rows)
        t8 = [r for r in rows if r.get("t_over_mm") is not None]
        out += ["## Verdict in counts", "",
                "B is faster than A at %d of %d points (A / B %.2f ... %.2f), faster than C at %d of %d (C / B %.2f ... %.2f)%s." % (
                    wa, n, min(r["image_over_mm"] for r in rows), max(r["image_over_mm"] for r in rows), wc, n,
                    min(r["decode_addmm_over_mm"] for r in rows), max(r["decode_addmm_over_mm"] for r in rows),
                    "; at M = 8 faster than T at %d of %d (T / B %.2f ... %.2f)" % (
                        sum(r["t_over_mm"] > 1 for r in t8), len(t8), min(r["t_over_mm"] for r in t8), max(r["t_over_mm"] for r in t8)) if t8 else ""),
                "Per M, B's wins against A / against C: " + "; ".join("M = %d: %d / %d of %d" % (
                    M, sum(r["image_over_mm"] > 1 for r in rows if r["M"] == M), sum(r["decode_addmm_over_mm"] > 1 for r in rows if r["M"] == M),
                    sum(1 for r in rows if r["M"] == M)) for M in MS) + ".",
                "B's own time from M = 9 to M = 64, same layer and run: %.2f ... %.2f times." % (
                    min(b["us_linear4_t_mm"] / a["us_linear4_t_mm"] for a in rows if a["M"] == 9 for b in rows
                        if b["M"] == 64 and (b["dtype"], b["book"], b["layer"]) == (a["dtype"], a["book"], a["layer"])),
                    max(b["us_linear4_t_mm"] / a["us_linear4_t_mm"] for a in rows if a["M"] == 9 for b in rows
                        if b["M"] == 64 and (b["dtype"], b["book"], b["layer"]) == (a["dtype"], a["book"], a["layer"])))
                if any(r["M"] == 64 for r in rows) and any(r["M"] == 9 for r in rows) else "", ""]
        out += _ratio_rows(rows, "image_over_mm", "## A / B per layer and M over all %d runs (dtype x codebook): min ... max (B's wins)" % len(keys))
        out += _ratio_rows(rows, "decode_addmm_over_mm", "## C / B per layer and M: min ... max (B's wins)")
    for dt, book in keys:
        out += ["## %s, %s" % (dt, book), "", "| layer [K, N] | M | calls | A | C | B | T | A / B | C / B | T / B | % of 8 TB/s | spread |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            if (r["dtype"], r["book"]) == (dt, book):
                t = r.get("us_linear4_t")
                out.append("| %s [%d, %d] | %d | %d | %.1f | %.1f | %.1f | %s | %.2f | %.2f | %s | %.1f | %.1f %% |" % (
                    r["layer"], r["K"], r["N"], r["M"], r["calls"], r["us_image"], r["us_decode_addmm"], r["us_linear4_t_mm"],
                    "" if t is None else "%.1f" % t, r["image_over_mm"], r["decode_addmm_over_mm"],
                    "" if t is None else "%.2f" % r["t_over_mm"], 100 * r["codes_fraction_of_hbm"], 100 * r["spread"]))
        out.append("")
    if static:
        body = "\n".join("| %s%s | %d | %d | %d | %d | %d | %d | %d | %d |" % (
            s["T"], ", pair rule" if s["ovp"] else "", s["MT"], s.get("vgpr", -1), s.get("agpr", -1), s.get("sgpr", -1), s.get("lds", -1),
            s.get("scratch", -1), s.get("sspill", 0) + s.get("vspill", 0), s.get("occ", -1)) for s in sorted(static, key=lambda s: (s["T"], s["ovp"], s["MT"])))
        out += ["## Resources of every instantiation (from the compiler, not from a run)", "", RESOURCES % body]
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, OliVe, GPT-2 small only")
    ap.add_argument("--all-shapes", action="store_true", help="with --quick: GPT-2 XL's shapes as well")
    ap.add_argument("--iters", type=int, default=200, help="the fewest calls per graph")
    ap.add_argument("--max-iters", type=int, default=1200, help="the most calls per graph")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=None, help="file with the compiler's kernel-resource-usage remarks of k_linear_t_mm")
    ap.add_argument("--notes", default=None, help="a markdown file appended to the .md: what the run does not say")
    ap.add_argument("--rewrite", default=None, help="a .json of an earlier run: write its .md again (no GPU needed) and stop")
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every layer)")
    a = ap.parse_args()
    static = resources_table(a.resources)
    if a.rewrite:
        write_md(json.load(open(a.rewrite)), (a.out or os.path.splitext(a.rewrite)[0]) + ".md", a, static)
        return
    if not torch.cuda.is_available():
        raise SystemExit("probe_linear4_t_mm: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []
    for dt in ((torch.bfloat16,) if a.quick else (torch.bfloat16, torch.float16)):
        esz = torch.empty(0, dtype=dt).element_size()
        for bname, g, gmax, nn, ovp in (books()[1:] if a.quick else books()):
            plan = _lib.plan_for(g)
            gd = plan.grid_dev(dev)
            for sname, K, N in (SHAPES[:4] if a.quick and not a.all_shapes else SHAPES):
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
                    mm = lambda i: _lib.linear4_t_mm(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)
                    graphs = {"A": capture(lambda i: torch.addmm(bias, x, images[i]), n_img, iters, 20), "C": capture(arm_c, n_cod, iters, 20),
                              "B": capture(mm, n_cod, iters, 20)}
                    if M <= _lib.LINEAR4_T_MAX_M:
                        graphs["T"] = capture(lambda i: _lib.linear4_t(codes[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y),
                                              n_cod, iters, 20)
                    t = alternate(graphs, iters, a.reps)
                    ta, tc, tb = t["A"][0], t["C"][0], t["B"][0]
                    tt = t["T"][0] if "T" in t else None
                    r = dict(dtype=str(dt).split(".")[1], book=bname, layer=sname, K=K, N=N, M=M, calls=iters, image_buffers=n_img, code_buffers=n_cod,
                             us_image=round(ta, 2), us_decode_addmm=round(tc, 2), us_linear4_t_mm=round(tb, 2),
                             us_linear4_t=None if tt is None else round(tt, 2), image_over_mm=round(ta / tb, 3),
                             decode_addmm_over_mm=round(tc / tb, 3), t_over_mm=None if tt is None else round(tt / tb, 3),
                             codes_fraction_of_hbm=round(cbytes / (tb * 1e-6) / HBM_BYTES_PER_S, 4),
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
