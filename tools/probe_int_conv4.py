#!/usr/bin/env python3
"""A/B of a packed 4-bit Conv2d layer's whole forward from a RAW input -- activation quantiser and convolution -- on ResNet-50's
distinct conv shapes with C % 32 == 0 (224 x 224 images), at batch 1, 8 and 64, float32 and bfloat16; the protocol of
profiles/int_linear4.md: same process, each arm rotating over distinct weight buffers, per point `--reps` measurements of one
captured graph of calls per arm, the arms ALTERNATED inside every repetition; the median and the spread (max - min) / median.

    I   antq_quant_i8 + antq_conv2d4_i8 on the tap-major codes, the input channels-last   (pack_model(integer_conv=True))
    IN  the same from an NCHW-contiguous input: the copy to channels-last memory is paid
    A   antq_fakequant + F.conv2d on the kept image; measured with the NCHW-contiguous and with the channels-last input, the
        faster of the two per point is A (`a_layout` says which)

Signed flint-4 weights with one scale per output channel, unsigned int-4 activations (post-ReLU) with one scale, bias.

    K   (--sk) antq_quant_i8 + antq_conv2d4_i8_sk, the input channels-last   (pack_model(integer_conv_split_k=True)); measured
        against I and A at the points whose output has at most CONV2D4_I8_SK_MAX_M rows, `--force S` with forced slices

    Q0 / Q1 / Q2, IN2   (--nchw) the quantiser alone -- antq_quant_i8 on a channels-last input, today's copy + antq_quant_i8 on an
        NCHW input, antq_quant_i8_nhwc on it -- and IN2 = Q2 + antq_conv2d4_i8 against IN and A   (pack_model(integer_conv_nchw=True))

    python tools/probe_int_conv4.py [--quick] [--out profiles/int_conv4]      (writes .json and .md)
    python tools/probe_int_conv4.py --nchw [--dtype bfloat16] --out profiles/quant_i8_nhwc
    python tools/probe_int_conv4.py --sk [--force S] [--every n] [--dtype bfloat16] --out profiles/int_conv4_sk
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

# (C, N, kernel, stride, padding, H = W of the input): torchvision's ResNet-50 (stride on the 3 x 3), conv1 (C = 3) left out
SHAPES = ((64, 64, 1, 1, 0, 56), (64, 64, 3, 1, 1, 56), (64, 256, 1, 1, 0, 56), (256, 64, 1, 1, 0, 56), (256, 128, 1, 1, 0, 56),
          (128, 128, 3, 2, 1, 56), (128, 512, 1, 1, 0, 28), (256, 512, 1, 2, 0, 56), (512, 128, 1, 1, 0, 28), (128, 128, 3, 1, 1, 28),
          (512, 256, 1, 1, 0, 28), (256, 256, 3, 2, 1, 28), (256, 1024, 1, 1, 0, 14), (512, 1024, 1, 2, 0, 28), (1024, 256, 1, 1, 0, 14),
          (256, 256, 3, 1, 1, 14), (1024, 512, 1, 1, 0, 14), (512, 512, 3, 2, 1, 14), (512, 2048, 1, 1, 0, 7), (1024, 2048, 1, 2, 0, 14),
          (2048, 512, 1, 1, 0, 7), (512, 512, 3, 1, 1, 7))
BATCHES = (1, 8, 64)


def _range(v):
    return "%.2f ... %.2f" % (min(v), max(v))


def write_md(rows, path, args):
    out = ["# antq_quant_i8 + antq_conv2d4_i8 against today's forward of a packed 4-bit Conv2d layer", "",
           "Written by `tools/probe_int_conv4.py%s`: one MI355X, one process, one run; every arm starts from the RAW input and rotates "
           "over distinct weight buffers; per point %d repetitions of one graph-replayed batch of calls per arm, the arms alternated "
           "inside a repetition; medians in us per call, `spread` = the largest (max - min) / median of the point's arms." % (
               " --quick" if args.quick else "", args.reps), "",
           "I = antq_quant_i8 + antq_conv2d4_i8 from a channels-last input, IN = the same from an NCHW input (relayout paid), A = "
           "antq_fakequant + F.conv2d on the kept image with the faster of the two input layouts (`A in`).  I / A and IN / A are TIMES: "
           "below 1, the integer path is faster.  `won` / `lost`: faster / slower than A by more than the point's spread.  TOP/s = "
           "2 M N K over I's time (quantiser included).", ""]
    for dt in sorted({r["dtype"] for r in rows}):
        rs = [r for r in rows if r["dtype"] == dt]
        out += ["## Verdict in counts, %s" % dt, "", "| arm | points | won | lost | arm / A |", "|---|---|---|---|---|"]
        for arm in ("i", "in"):
            k = arm + "_over_a"
            out.append("| %s | %d | %d | %d | %s |" % (arm.upper(), len(rs), sum(r[k] < 1 - r["spread"] for r in rs),
                                                     sum(r[k] > 1 + r["spread"] for r in rs), _range([r[k] for r in rs])))
        out += ["", "Per batch, I / A: " + "; ".join("B = %d: %s" % (B, _range([r["i_over_a"] for r in rs if r["B"] == B]))
                                                     for B in BATCHES if any(r["B"] == B for r in rs)) + ".",
                "I reaches %s TOP/s.  The largest spread of a point is %.1f %%." % (_range([r["tops"] for r in rs]), 100 * max(r["spread"] for r in rs)), "",
                "| C -> N, k / stride, input | B | M | K | calls | I | IN | A | A in | I / A | IN / A | TOP/s | spread |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rs:
            out.append("| %d -> %d, %d / %d, %d x %d | %d | %d | %d | %d | %.1f | %.1f | %.1f | %s | %.2f | %.2f | %.0f | %.1f %% |" % (
                r["C"], r["N"], r["k"], r["stride"], r["H"], r["H"], r["B"], r["M"], r["K"], r["calls"], r["us_i"], r["us_in"], r["us_a"],
                r["a_layout"], r["i_over_a"], r["in_over_a"], r["tops"], 100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def write_md_sk(rows, path, args):
    """--sk: K = antq_quant_i8 + antq_conv2d4_i8_sk against I and A, the points where the rule gives one slice apart"""
    out = ["# antq_conv2d4_i8_sk (split-K) against antq_conv2d4_i8 and today's forward, outputs of up to 1024 rows", "",
           "Written by `tools/probe_int_conv4.py --sk`: one MI355X, one process; the protocol of profiles/int_conv4.md (every arm from "
           "the RAW channels-last input, distinct weight buffers in rotation, per point %d repetitions of one graph-replayed batch of "
           "calls per arm, the arms alternated inside a repetition; medians in us per call, `spread` = the largest (max - min) / median "
           "of the point's arms).  K = antq_quant_i8 + antq_conv2d4_i8_sk, I = antq_quant_i8 + antq_conv2d4_i8 (the parent's kernel), "
           "A = antq_fakequant + F.conv2d on the kept image, the faster input layout.  K / I and K / A are TIMES: below 1, K is "
           "faster.  `won` / `lost`: by more than the point's spread.  `forced`: slices set with antq_debug_set key 24 (0: the rule)." % args.reps, ""]
    for dt in sorted({r["dtype"] for r in rows}):
        for title, rs in (("the rule splits K", [r for r in rows if r["dtype"] == dt and r["slices"] > 1 and not r["forced"]]),
                          ("the rule gives one slice", [r for r in rows if r["dtype"] == dt and r["slices"] == 1 and not r["forced"]]),
                          ("forced slices", [r for r in rows if r["dtype"] == dt and r["forced"]])):
            if not rs:
                continue
            out += ["## %s, %s" % (dt, title), ""]
            for k, name in (("k_over_i", "K / I"), ("k_over_a", "K / A")):
                out.append("%s: %d points, won %d, lost %d, %s.  " % (name, len(rs), sum(r[k] < 1 - r["spread"] for r in rs),
                                                                     sum(r[k] > 1 + r["spread"] for r in rs), _range([r[k] for r in rs])))
            out += ["", "| C -> N, k / stride, input | B | M | K | slices | calls | K | I | A | K / I | K / A | spread |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
            for r in rs:
                out.append("| %d -> %d, %d / %d, %d x %d | %d | %d | %d | %d | %d | %.1f | %.1f | %.1f | %.2f | %.2f | %.1f %% |" % (
                    r["C"], r["N"], r["k"], r["stride"], r["H"], r["H"], r["B"], r["M"], r["K"], r["slices"], r["calls"], r["us_k"], r["us_i"],
                    r["us_a"], r["k_over_i"], r["k_over_a"], 100 * r["spread"]))
            out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def write_md_nchw(rows, path, args):
    """--nchw: the quantiser alone (Q0, Q1, Q2) and the whole call from an NCHW input (IN, IN2, A)"""
    out = ["# antq_quant_i8_nhwc against the channels-last copy + antq_quant_i8, NCHW inputs", "",
           "Written by `tools/probe_int_conv4.py --nchw`: one MI355X, one process; the protocol of profiles/int_conv4.md (per point %d "
           "repetitions of one graph-replayed batch of calls per arm, the arms alternated inside a repetition; medians in us per call, "
           "`spread` = the largest (max - min) / median of the point's arms).  Q0 = antq_quant_i8 on a channels-last input, Q1 = "
           "contiguous(channels_last) + antq_quant_i8 (today's NCHW path), Q2 = antq_quant_i8_nhwc, COPY = the copy alone; IN = Q1 + "
           "antq_conv2d4_i8, IN2 = Q2 + antq_conv2d4_i8, A = antq_fakequant + F.conv2d on the kept image, the faster input layout.  "
           "Ratios are TIMES: below 1, the first is faster.  `won` / `lost`: by more than the point's spread.  GB/s: bytes read + "
           "written (Q2: element + 1, COPY: 2 elements) over the time; every call of an arm reads the same input, so small inputs "
           "come from the caches." % args.reps, ""]
    for dt in sorted({r["dtype"] for r in rows}):
        rs = [r for r in rows if r["dtype"] == dt]
        out += ["## %s" % dt, "", "| ratio | points | won | lost | range |", "|---|---|---|---|---|"]
        for k, name in (("q2_over_q1", "Q2 / Q1"), ("in2_over_in", "IN2 / IN"), ("in_over_a", "IN / A"), ("in2_over_a", "IN2 / A")):
            out.append("| %s | %d | %d | %d | %s |" % (name, len(rs), sum(r[k] < 1 - r["spread"] for r in rs),
                                                     sum(r[k] > 1 + r["spread"] for r in rs), _range([r[k] for r in rs])))
        big = sorted(rs, key=lambda r: -r["B"] * r["C"] * r["H"] * r["H"])[:3]
        out += ["", "The three largest inputs: " + "; ".join("%d x %d x %d x %d: Q2 %.0f GB/s, COPY %.0f GB/s" % (
            r["B"], r["C"], r["H"], r["H"], r["q2_gbs"], r["copy_gbs"]) for r in big) + ".", "",
                "| C -> N, k / stride, input | B | Q0 | Q1 | Q2 | COPY | IN | IN2 | A | Q2 / Q1 | IN2 / IN | IN2 / A | Q2 GB/s | spread |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rs:
            out.append("| %d -> %d, %d / %d, %d x %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.2f | %.2f | %.0f | %.1f %% |" % (
                r["C"], r["N"], r["k"], r["stride"], r["H"], r["H"], r["B"], r["us_q0"], r["us_q1"], r["us_q2"], r["us_copy"], r["us_in"],
                r["us_in2"], r["us_a"], r["q2_over_q1"], r["in2_over_in"], r["in2_over_a"], r["q2_gbs"], 100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def write_md_bytes(rows, path, args):
    """--bytes: I8 and K8 (offset form) against A on the kept 8-bit image, I4 for scale"""
    out = ["# antq_conv2d8_i8 / antq_conv2d8_i8_sk (W8A8, unsigned 8-bit activations) against today's forward of a byte-coded Conv2d layer", "",
           "Written by `tools/probe_int_conv4.py --bytes`: one MI355X, one process; the protocol of profiles/int_conv4.md (every arm from "
           "the RAW input, distinct weight buffers in rotation, per point %d repetitions of one graph-replayed batch of calls per arm, "
           "the arms alternated inside a repetition; medians in us per call, `spread` = the largest (max - min) / median of the point's "
           "arms).  Signed int8 weights (XOR kind), unsigned int8 activations (x_offset = 128), bias.  I8 = antq_quant_i8 + "
           "antq_conv2d8_i8 from a channels-last input, K8 = the same through antq_conv2d8_i8_sk (M <= 1024; `S` = its slices), A = "
           "antq_fakequant + F.conv2d on the kept 8-bit image with the faster input layout, I4 = antq_quant_i8 + antq_conv2d4_i8 at "
           "the same shape.  Ratios are TIMES: below 1, the first is faster.  `won` / `lost`: by more than the point's spread." % args.reps, ""]
    for dt in sorted({r["dtype"] for r in rows}):
        rs = [r for r in rows if r["dtype"] == dt]
        out += ["## %s" % dt, "", "| ratio | points | won | lost | range |", "|---|---|---|---|---|"]
        for k, name, sel in (("i8_over_a", "I8 / A", rs), ("k8_over_a", "K8 / A", [r for r in rs if r["slices"]]),
                             ("k8_over_i8", "K8 / I8, the rule splits", [r for r in rs if r["slices"] > 1]),
                             ("k8_over_i8", "K8 / I8, one slice", [r for r in rs if r["slices"] == 1]), ("i8_over_i4", "I8 / I4", rs)):
            if sel:
                out.append("| %s | %d | %d | %d | %s |" % (name, len(sel), sum(r[k] < 1 - r["spread"] for r in sel),
                                                         sum(r[k] > 1 + r["spread"] for r in sel), _range([r[k] for r in sel])))
        out += ["", "I8 reaches %s TOP/s.  The largest spread of a point is %.1f %%." % (_range([r["tops"] for r in rs]), 100 * max(r["spread"] for r in rs)), "",
                "| C -> N, k / stride, input | B | M | K | S | I8 | K8 | A | A in | I4 | I8 / A | K8 / A | K8 / I8 | I8 / I4 | spread |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        f = lambda v, p: "-" if v is None else p % v
        for r in rs:
            out.append("| %d -> %d, %d / %d, %d x %d | %d | %d | %d | %d | %.1f | %s | %.1f | %s | %.1f | %.2f | %s | %s | %.2f | %.1f %% |" % (
                r["C"], r["N"], r["k"], r["stride"], r["H"], r["H"], r["B"], r["M"], r["K"], r["slices"], r["us_i8"], f(r["us_k8"], "%.1f"),
                r["us_a"], r["a_layout"], r["us_i4"], r["i8_over_a"], f(r["k8_over_a"], "%.2f"), f(r["k8_over_i8"], "%.2f"), r["i8_over_i4"],
                100 * r["spread"]))
        out.append("")
    if args.notes and os.path.exists(args.notes):
        out += [open(args.notes).read()]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchw", action="store_true", help="the quantiser arms Q0 / Q1 / Q2 and the whole call IN / IN2 / A from an NCHW input")
    ap.add_argument("--bytes", action="store_true", help="W8A8: I8 / K8 (antq_conv2d8_i8 / _sk, offset form) against A on the 8-bit image and I4")
    ap.add_argument("--sk", action="store_true", help="the split-K arm K against I and A, at the points of at most CONV2D4_I8_SK_MAX_M rows")
    ap.add_argument("--force", type=int, default=0, help="(--sk) slices forced with antq_debug_set key 24")
    ap.add_argument("--every", type=int, default=1, help="(--sk) every n-th shape only")
    ap.add_argument("--quick", action="store_true", help="bfloat16, batch 8, every fourth shape")
    ap.add_argument("--dtype", default=None, help="float32 or bfloat16 alone (a run split in two; merge with --rewrite)")
    ap.add_argument("--flop", type=float, default=1e11, help="operations per graph, about")
    ap.add_argument("--min-iters", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--notes", default=None, help="a markdown file appended to the .md: what the run does not say")
    ap.add_argument("--rewrite", default=None, help="the .json of an earlier run, or several with commas: write the .md (and the merged .json) again (no GPU needed) and stop")
    ap.add_argument("--out", default=None, help="path without extension: .json and .md are written (and rewritten after every shape)")
    a = ap.parse_args()
    if a.rewrite:
        rows = [r for f in a.rewrite.split(",") for r in json.load(open(f))]          # (several files: the parts of a split run)
        if a.out:
            with open(a.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)
        (write_md_bytes if a.bytes else write_md_nchw if a.nchw else write_md_sk if a.sk else write_md)(rows, (a.out or os.path.splitext(a.rewrite)[0]) + ".md", a)
        return
    if not torch.cuda.is_available():
        raise SystemExit("probe_int_conv4: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    gw, gx = grids.ant_flint(4, True), grids.ant_grid("int", 4, False)
    plan_w, plan_x = _lib.plan_for(gw), _lib.plan_for(gx)
    gmax_w, gmax_x = float(gw.max()), float(gx.max())
    (I_w, _), (I_x, _) = plan_w.integer_image(), plan_x.integer_image()
    img_w, img_x = plan_w.image_dev(dev), plan_x.image_dev(dev)
    if a.bytes:
        gw8, gx8 = grids.ant_grid("int", 8, True), grids.ant_grid("int", 8, False)
        plan_w8, plan_x8 = _lib.plan_for(gw8), _lib.plan_for(gx8)
        gmax_w8, gmax_x8 = float(gw8.max()), float(gx8.max())
        (I_w8, host8), I_x8 = plan_w8.integer_image8(), plan_x8.offset_image()[0]
        img_w8, img_x8 = plan_w8.image_dev(dev, 128), plan_x8.image_dev(dev, "offset")
    rows = []
    for dt in ((getattr(torch, a.dtype),) if a.dtype else (torch.bfloat16,) if a.quick else (torch.float32, torch.bfloat16)):
        esz = torch.empty(0, dtype=dt).element_size()
        for C, N, k, stride, pad, H in (SHAPES[::4] if a.quick else SHAPES[::a.every] if a.sk else SHAPES):
            K = C * k * k
            w = (torch.randn(N, C, k, k, device=dev) * 0.05).to(dt)
            alpha = (w.float().abs().amax((1, 2, 3)) * 0.9).contiguous()
            codes0 = _lib.encode4(w, alpha, plan_w, gmax_w, N, K, True)
            image0 = _lib.decode4(codes0, alpha, plan_w, gmax_w, N, K, True, dt).view(N, C, k, k)
            taps0 = packed._tap_major(codes0, (N, C, k, k))
            unit_w = packed._unit_alpha(alpha, plan_w, gmax_w)
            bias = torch.randn(N, device=dev).to(dt)
            del w
            for B in ((8,) if a.quick else BATCHES):
                Ho = (H + 2 * pad - k) // stride + 1
                M = B * Ho * Ho
                if a.sk and M > _lib.CONV2D4_I8_SK_MAX_M:
                    continue
                iters = int(min(a.max_iters, max(a.min_iters, a.flop / (2.0 * M * N * K))))
                n_buf = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N * esz)))))
                images, taps = [image0.clone() for _ in range(n_buf)], [taps0.clone() for _ in range(n_buf)]
                x = torch.rand(B, C, H, H, device=dev).to(dt)                      # post-ReLU: no negative value
                x_cl = x.contiguous(memory_format=torch.channels_last)
                ax = (x.float().max() * 0.9).reshape(1).contiguous()
                unit_x = packed._unit_alpha(ax, plan_x, gmax_x)
                xq = torch.empty(B, H, H, C, dtype=torch.int8, device=dev)
                xf, xf_cl = torch.empty_like(x), torch.empty_like(x_cl)
                y = torch.empty(B, Ho, Ho, N, dtype=dt, device=dev).permute(0, 3, 1, 2)

                def integer(src, i):
                    _lib.quant_i8(src.permute(0, 2, 3, 1), ax, plan_x, gmax_x, 1, src.numel(), False, img_x, out=xq)
                    return _lib.int_conv2d4(taps[i], xq, unit_w, img_w, I_w, unit_x, I_x, N, k, stride, pad, 1, True, dt, bias=bias, out=y)

                def image(src, dst, i):
                    last = not src.is_contiguous()            # (the quantiser takes the memory as it lies: NHWC views of both)
                    _lib.fakequant(src.permute(0, 2, 3, 1) if last else src, ax, plan_x, gmax_x, 1, src.numel(), False,
                                   out=dst.permute(0, 2, 3, 1) if last else dst)
                    return F.conv2d(dst, images[i], bias, stride, pad)

                if a.bytes:
                    # W8A8: signed int8 weights (the XOR kind), unsigned int8 activations -- the offset form, x_offset = 128
                    if B == (8 if a.quick else BATCHES[0]):       # (the shape's first batch: its byte-coded weight)
                        w8 = (torch.randn(N, C, k, k, device=dev) * 0.05).to(dt)
                        alpha8 = (w8.float().abs().amax((1, 2, 3)) * 0.9).contiguous()
                        codes8 = _lib.encode8(w8, alpha8, plan_w8, gmax_w8, N, K, True)
                        image8 = _lib.decode8(codes8, alpha8, plan_w8, gmax_w8, N, K, True, dt).view(N, C, k, k)
                        taps8 = packed._tap_major_bytes(codes8, (N, C, k, k))
                        wsum = packed._image_sums(taps8, host8, N)
                        unit_w8 = packed._unit_alpha(alpha8, plan_w8, gmax_w8)
                    n_buf8 = int(min(iters, max(2, -(-ROTATE_BYTES // (K * N)))))
                    images8, tap8s = [image8.clone() for _ in range(n_buf)], [taps8.clone() for _ in range(n_buf8)]
                    unit_x8 = packed._unit_alpha(ax, plan_x8, gmax_x8)
                    use_sk = M <= _lib.CONV2D8_I8_SK_MAX_M
                    ws = torch.empty(max(_lib.int_conv2d8_sk_workspace_bytes(M, N, K), 16) if use_sk else 16, dtype=torch.uint8, device=dev)

                    def bytes8(fn, i, **kw):
                        _lib.quant_i8(x_cl.permute(0, 2, 3, 1), ax, plan_x8, gmax_x8, 1, x_cl.numel(), False, img_x8, out=xq)
                        return fn(tap8s[i % n_buf8], xq, unit_w8, img_w8, host8, I_w8, unit_x8, I_x8, N, k, stride, pad, 1, True, dt, bias=bias,
                                  out=y, x_offset=128, wsum=wsum, **kw)

                    def image8bit(src, dst, i):
                        last = not src.is_contiguous()
                        _lib.fakequant(src.permute(0, 2, 3, 1) if last else src, ax, plan_x8, gmax_x8, 1, src.numel(), False,
                                       out=dst.permute(0, 2, 3, 1) if last else dst)
                        return F.conv2d(dst, images8[i], bias, stride, pad)

                    graphs = {"I8": capture(lambda i: bytes8(_lib.int_conv2d8, i), n_buf, iters, 3),
                              "A": capture(lambda i: image8bit(x, xf, i), n_buf, iters, 3),
                              "ACL": capture(lambda i: image8bit(x_cl, xf_cl, i), n_buf, iters, 3),
                              "I4": capture(lambda i: integer(x_cl, i), n_buf, iters, 3)}
                    if use_sk:
                        graphs["K8"] = capture(lambda i: bytes8(_lib.int_conv2d8_sk, i, workspace=ws), n_buf, iters, 3)
                    t = alternate(graphs, iters, a.reps)
                    us = {key: v[0] for key, v in t.items()}
                    us_a = min(us["A"], us["ACL"])
                    r = dict(dtype=str(dt).split(".")[1], C=C, N=N, k=k, stride=stride, H=H, B=B, M=M, K=K, calls=iters,
                             slices=_lib.int_conv2d8_sk_slices(M, N, K) if use_sk else 0, us_i8=round(us["I8"], 2),
                             us_k8=round(us["K8"], 2) if use_sk else None, us_a=round(us_a, 2), us_i4=round(us["I4"], 2),
                             a_layout="NCHW" if us["A"] <= us["ACL"] else "channels-last", i8_over_a=round(us["I8"] / us_a, 3),
                             k8_over_a=round(us["K8"] / us_a, 3) if use_sk else None, k8_over_i8=round(us["K8"] / us["I8"], 3) if use_sk else None,
                             i8_over_i4=round(us["I8"] / us["I4"], 3), tops=round(2.0 * M * N * K / (us["I8"] * 1e-6) / 1e12, 1),
                             spread=round(max(v[1] for v in t.values()), 4))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del graphs, t, images, taps, images8, tap8s
                    continue
                if a.sk:
                    _lib.lib().antq_debug_set(24, a.force)
                    slices = _lib.lib().antq_conv2d4_i8_sk_slices(M, N, K, 0)
                    ws = torch.empty(max(_lib.int_conv2d4_sk_workspace_bytes(M, N, K), 16), dtype=torch.uint8, device=dev)

                    def split(i):
                        _lib.quant_i8(x_cl.permute(0, 2, 3, 1), ax, plan_x, gmax_x, 1, x_cl.numel(), False, img_x, out=xq)
                        return _lib.int_conv2d4_sk(taps[i], xq, unit_w, img_w, I_w, unit_x, I_x, N, k, stride, pad, 1, True, dt, bias=bias,
                                                   out=y, workspace=ws)

                    t = alternate({"K": capture(split, n_buf, iters, 3), "I": capture(lambda i: integer(x_cl, i), n_buf, iters, 3),
                                   "A": capture(lambda i: image(x, xf, i), n_buf, iters, 3),
                                   "ACL": capture(lambda i: image(x_cl, xf_cl, i), n_buf, iters, 3)}, iters, a.reps)
                    _lib.lib().antq_debug_set(24, 0)
                    us = {key: v[0] for key, v in t.items()}
                    us_a = min(us["A"], us["ACL"])
                    r = dict(dtype=str(dt).split(".")[1], C=C, N=N, k=k, stride=stride, H=H, B=B, M=M, K=K, calls=iters, buffers=n_buf,
                             forced=a.force, slices=slices, us_k=round(us["K"], 2), us_i=round(us["I"], 2), us_a=round(us_a, 2),
                             k_over_i=round(us["K"] / us["I"], 3), k_over_a=round(us["K"] / us_a, 3),
                             spread=round(max(v[1] for v in t.values()), 4))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del t, images, taps
                    continue
                if a.nchw:
                    def q1(i):
                        src = x.contiguous(memory_format=torch.channels_last)
                        _lib.quant_i8(src.permute(0, 2, 3, 1), ax, plan_x, gmax_x, 1, src.numel(), False, img_x, out=xq)

                    def in2(i):
                        _lib.quant_i8_nhwc(x, ax, plan_x, gmax_x, img_x, out=xq)
                        return _lib.int_conv2d4(taps[i], xq, unit_w, img_w, I_w, unit_x, I_x, N, k, stride, pad, 1, True, dt, bias=bias, out=y)

                    t = alternate({"Q0": capture(lambda i: _lib.quant_i8(x_cl.permute(0, 2, 3, 1), ax, plan_x, gmax_x, 1, x.numel(), False,
                                                                         img_x, out=xq), n_buf, iters, 3),
                                   "Q1": capture(q1, n_buf, iters, 3),
                                   "Q2": capture(lambda i: _lib.quant_i8_nhwc(x, ax, plan_x, gmax_x, img_x, out=xq), n_buf, iters, 3),
                                   "COPY": capture(lambda i: x.contiguous(memory_format=torch.channels_last), n_buf, iters, 3),
                                   "IN": capture(lambda i: integer(x.contiguous(memory_format=torch.channels_last), i), n_buf, iters, 3),
                                   "IN2": capture(in2, n_buf, iters, 3),
                                   "A": capture(lambda i: image(x, xf, i), n_buf, iters, 3),
                                   "ACL": capture(lambda i: image(x_cl, xf_cl, i), n_buf, iters, 3)}, iters, a.reps)
                    us = {key: v[0] for key, v in t.items()}
                    us_a, n = min(us["A"], us["ACL"]), x.numel()
                    r = dict(dtype=str(dt).split(".")[1], C=C, N=N, k=k, stride=stride, H=H, B=B, M=M, K=K, calls=iters,
                             us_q0=round(us["Q0"], 2), us_q1=round(us["Q1"], 2), us_q2=round(us["Q2"], 2), us_copy=round(us["COPY"], 2),
                             us_in=round(us["IN"], 2), us_in2=round(us["IN2"], 2), us_a=round(us_a, 2),
                             q2_over_q1=round(us["Q2"] / us["Q1"], 3), in2_over_in=round(us["IN2"] / us["IN"], 3),
                             in_over_a=round(us["IN"] / us_a, 3), in2_over_a=round(us["IN2"] / us_a, 3),
                             q2_gbs=round(n * (esz + 1) / us["Q2"] / 1e3, 1), copy_gbs=round(n * 2 * esz / us["COPY"] / 1e3, 1),
                             spread=round(max(v[1] for v in t.values()), 4))
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    del t, images, taps
                    continue
                graphs = {"I": capture(lambda i: integer(x_cl, i), n_buf, iters, 3),
                          "IN": capture(lambda i: integer(x.contiguous(memory_format=torch.channels_last), i), n_buf, iters, 3),
                          "A": capture(lambda i: image(x, xf, i), n_buf, iters, 3),
                          "ACL": capture(lambda i: image(x_cl, xf_cl, i), n_buf, iters, 3)}
                t = alternate(graphs, iters, a.reps)
                us = {key: v[0] for key, v in t.items()}
                best = "ACL" if us["ACL"] < us["A"] else "A"
                r = dict(dtype=str(dt).split(".")[1], C=C, N=N, k=k, stride=stride, H=H, B=B, M=M, K=K, calls=iters, buffers=n_buf,
                         us_i=round(us["I"], 2), us_in=round(us["IN"], 2), us_a_nchw=round(us["A"], 2), us_a_cl=round(us["ACL"], 2),
                         us_a=round(us[best], 2), a_layout="NCHW" if best == "A" else "channels-last",
                         i_over_a=round(us["I"] / us[best], 3), in_over_a=round(us["IN"] / us[best], 3),
                         tops=round(2.0 * M * N * K / (us["I"] * 1e-6) / 1e12, 1), spread=round(max(v[1] for v in t.values()), 4))
                rows.append(r)
                print(json.dumps(r), flush=True)
                del graphs, images, taps
            torch.cuda.empty_cache()
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out + ".json", "w") as f:
                    json.dump(rows, f, indent=1)
                (write_md_bytes if a.bytes else write_md_nchw if a.nchw else write_md_sk if a.sk else write_md)(rows, a.out + ".md", a)


if __name__ == "__main__":
    main()
