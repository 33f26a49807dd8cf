#!/usr/bin/env python3
"""A/B of a byte-coded packed Linear layer with 8 .. 64 input rows, the protocol of tools/probe_linear8.py (one process per
(dtype, book); each arm rotating over 512 MB of distinct weight buffers so that every call streams its weights from HBM; one
captured graph of `--iters` calls per arm; `--rounds` rounds in which the arms take turns; the median over the rounds is
reported, and the largest spread (max - min) / median of any arm over the rounds):

    A   F.linear on the decoded image                         (a packed model that keeps its images)
    C   antq_decode8 into one scratch buffer, then F.linear   (keep_images=False beyond 8 rows without fused_byte_rows)
    B   antq_linear8_mm on the codes, with the launcher's tile rule
    B1 / B2 / B4   the same with 1 / 2 / 4 tiles of 16 output rows per workgroup forced (antq_debug_set key 22; no result
        depends on it)
    L   antq_linear8 on the codes, at M = 8 only

Layers: OPT-6.7B's three Linear shapes and BERT-base's two, bf16 and f16, ANT int-8 (a plain book of 256 values) and OliVe
int-8 (the pair rule), per-row scales, M in {8, 16, 32, 64}.

    python tools/probe_linear8_mm.py [--quick] [--out profiles/packed_linear8_mm]      (writes <out>.json and <out>.md)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids  # noqa: E402

SHAPES = [(4096, 4096), (16384, 4096), (4096, 16384), (3072, 768), (768, 3072)]
MS = (8, 16, 32, 64)
ROTATE_BYTES = 1 << 29       # per arm: twice the Infinity Cache
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def books():
    """name -> (grid, gmax, n_normal, pair rule)"""
    g8 = np.asarray(grids.ant_grid("int", 8, True), np.float32)
    gn, go = grids.olive_int(8, True), grids.olive_outliers(8, True)
    return {"int_b8_s": (g8, float(g8.max()), 0, False),
            "olive_int_b8": (np.concatenate([gn, go]).astype(np.float32), float(np.max(gn)), int(len(gn)), True)}


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
    g, gmax, nn, ovp = books()[bname]
    plan = _lib.plan_for(g)
    gd = plan.grid_dev(dev)
    knob = _lib.lib().antq_debug_set
    for N, K in (SHAPES[:2] if quick else SHAPES):
        n_img = max(2, -(-ROTATE_BYTES // (N * K * 2)))
        n_c8 = max(2, -(-ROTATE_BYTES // (N * K)))
        w = (torch.randn(N, K, device=dev) * 0.05).to(dt)
        if ovp:
            w.view(-1)[::997] *= 12
        alpha = (w.float().abs().amax(1) * 0.9 if not ovp else 3 * w.float().std(1)).contiguous()
        c8 = _lib.encode8(w, alpha, plan, gmax, N, K, True, n_normal=nn, ovp=ovp)
        img = _lib.decode8(c8, alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp).view(N, K)
        del w
        images = [img.clone() for _ in range(n_img)]
        codes8 = [c8.clone() for _ in range(n_c8)]
        scratch = torch.empty(N * K, dtype=dt, device=dev)
        bias = torch.randn(N, device=dev).to(dt)
        for M in ((8, 64) if quick else MS):
            x = torch.randn(M, K, device=dev).to(dt)
            y = torch.empty(M, N, dtype=dt, device=dev)

            def arm_c(i):
                _lib.decode8(codes8[i], alpha, plan, gmax, N, K, True, dt, n_normal=nn, ovp=ovp, out=scratch)
                return F.linear(x, scratch.view(N, K), bias)
            mm = lambda i: _lib.linear8_mm(codes8[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y)   # noqa: E731
            arms = {"A": (lambda i: F.linear(x, images[i], bias), n_img, 0), "C": (arm_c, n_c8, 0), "B": (mm, n_c8, 0),
                    "B1": (mm, n_c8, 1), "B2": (mm, n_c8, 2), "B4": (mm, n_c8, 4)}
            if M <= _lib.LINEAR8_MAX_M:
                arms["L"] = (lambda i: _lib.linear8(codes8[i], x, alpha, gd, gmax, N, K, True, bias=bias, n_normal=nn, ovp=ovp, out=y), n_c8, 0)
            graphs = {}
            for k, (fn, n, nt) in arms.items():     # (the tile shape is the launcher's choice at capture: a graph keeps it)
                knob(22, nt)
                graphs[k] = graph_of(fn, n, iters)
            knob(22, 0)
            t = {k: [] for k in arms}
            for _ in range(rounds):
                for k in arms:
                    t[k].append(time_us(graphs[k], iters))
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = max((max(v) - min(v)) / med[k] for k, v in t.items())
            r = dict(dtype=dtype_name, book=bname, N=N, K=K, M=M, rounds=rounds, iters=iters,
                     us_A=round(med["A"], 2), us_C=round(med["C"], 2), us_B=round(med["B"], 2), us_B1=round(med["B1"], 2),
                     us_B2=round(med["B2"], 2), us_B4=round(med["B4"], 2), us_linear8=round(med["L"], 2) if "L" in med else None,
                     B_codes_frac_8TBs=round(N * K / (med["B"] * 1e-6) / 8e12, 4), B_over_A=round(med["A"] / med["B"], 3),
                     B_over_C=round(med["C"] / med["B"], 3), linear8_over_B=round(med["L"] / med["B"], 3) if "L" in med else None,
                     worst_spread=round(spread, 3))
            print("ROW " + json.dumps(r), flush=True)
            del graphs
        del images, codes8, scratch
        torch.cuda.empty_cache()


def largest_m(rows, key):
    """per layer: the largest M up to which B beats the arm at every smaller M too, in every (dtype, book) run (0: at none)"""
    out = {}
    for N, K in sorted({(r["N"], r["K"]) for r in rows}, key=lambda s: [(n, k) for n, k in SHAPES].index(s)):
        best = 0
        for M in sorted({r["M"] for r in rows}):
            pts = [r for r in rows if (r["N"], r["K"], r["M"]) == (N, K, M)]
            if all(r[key] > 1.0 for r in pts):
                best = M
            else:
                break
        out[(N, K)] = best
    return out


def write_out(prefix, rows, rounds, iters, note):
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    with open(prefix + ".json", "w") as f:
        json.dump(dict(rounds=rounds, iters=iters, note=note, timing=rows), f, indent=1)
    opt = lambda v, fmt="%.2f": "" if v is None else fmt % v   # noqa: E731
    with open(prefix + ".md", "w") as f:
        f.write("# antq_linear8_mm (B) against F.linear on the image (A) and antq_decode8 + F.linear (C)\n\n"
                "One MI355X, ONE run of the tool; one process per (dtype, book), arms alternated at every point, %d rounds of a graph of %d\n"
                "calls each, medians; times in us per call (kernels alone, replayed from a graph); per-row scales.  `B`: the launcher's tile\n"
                "rule, `B1` / `B2` / `B4`: 1 / 2 / 4 tiles of 16 output rows per workgroup forced.  `L`: antq_linear8 (M = 8 only).\n"
                "`B/8TB/s`: code bytes of B per second as a share of 8 TB/s.  `xA`, `xC`, `xL`: A / B, C / B and L / B (above 1: B is faster).\n"
                "`spread`: the largest (max - min) / median of any arm over the rounds.  No hardware counters were collected.\n%s\n\n" % (rounds, iters, note))
        f.write("| dtype | book | N | K | M | A | C | B | B1 | B2 | B4 | L | B/8TB/s | xA | xC | xL | spread |\n" + "|---" * 17 + "|\n")
        for r in rows:
            f.write("| %s | %s | %d | %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %s | %.1f %% | %.2f | %.2f | %s | %.1f %% |\n" % (
                r["dtype"], r["book"], r["N"], r["K"], r["M"], r["us_A"], r["us_C"], r["us_B"], r["us_B1"], r["us_B2"], r["us_B4"],
                opt(r["us_linear8"]), 100 * r["B_codes_frac_8TBs"], r["B_over_A"], r["B_over_C"], opt(r["linear8_over_B"]), 100 * r["worst_spread"]))
        f.write("\n## Largest M up to which B beats A / beats C in every (dtype, book) run (0: not even at M = 8; M in 8, 16, 32, 64)\n\n"
                "`every M where`: the M at which B wins in every run, whatever the smaller M did (M = 8 is not routed to B: the option\n"
                "serves 9 .. R rows).\n\n"
                "| N | K | beats A up to | beats C up to | every M where B beats A | every M where B beats C |\n|---|---|---|---|---|---|\n")
        la, lc = largest_m(rows, "B_over_A"), largest_m(rows, "B_over_C")
        where = lambda N, K, key: ", ".join(str(M) for M in sorted({r["M"] for r in rows}) if all(   # noqa: E731
            r[key] > 1.0 for r in rows if (r["N"], r["K"], r["M"]) == (N, K, M))) or "none"
        for (N, K) in la:
            f.write("| %d | %d | %d | %d | %s | %s |\n" % (N, K, la[(N, K)], lc[(N, K)], where(N, K, "B_over_A"), where(N, K, "B_over_C")))
        m8 = [r for r in rows if r["linear8_over_B"] is not None]
        if m8:
            wins = [r for r in m8 if r["linear8_over_B"] > 1.0]
            f.write("\nAt M = 8 B is faster than antq_linear8 in %d of %d rows (L / B from %.2f to %.2f).\n"
                    % (len(wins), len(m8), min(r["linear8_over_B"] for r in m8), max(r["linear8_over_B"] for r in m8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="the first two shapes, M = 8 and 64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        time_step(a.child[0], a.child[1], a.quick, a.iters, a.rounds)
        return
    rows, note = [], ""
    for st in [[d, b] for d in DTYPES for b in books()]:
        cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--rounds", str(a.rounds)] + (["--quick"] if a.quick else []) + ["--child"] + st
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            rc, out, err = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            rc, out, err = 124, (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), "timeout"
        for line in out.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
        if rc != 0:                                  # a step that failed: nothing more is started on the GPU
            note = "INCOMPLETE: step %s ended with status %d (%s)" % (st, rc, err.strip().splitlines()[-1] if err.strip() else "")
            print(note, flush=True)
            break
    if a.out:
        write_out(a.out, rows, a.rounds, a.iters, note)
    sys.exit(1 if note else 0)


if __name__ == "__main__":
    main()
