"""One batched decode (antq_decode4_batch) against the loop of per-tensor antq_decode4 launches over the same buffers and
against antq_copy of the output bytes: ResNet-50's weight shapes (53 of the 54: conv1's K = 147 has no packed form),
BERT-base's 74, 32 x 4096^2; bf16, OliVe pairs off.
Buffers are rotated past the Infinity Cache (sets of >= 512 MiB in turn); times from device events over whole passes.
    python tools/probe_packed.py [--out profiles/packed_decode.md]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids  # noqa: E402


def resnet50():
    s = [(64, 147)]
    cin = 64
    for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            s += [(width, cin), (width, width * 9), (width * 4, width)]
            if b == 0:
                s.append((width * 4, cin))
            cin = width * 4
    return s + [(1000, 2048)]


def bert_base():
    s = []
    for _ in range(12):
        s += [(768, 768)] * 4 + [(3072, 768), (768, 3072)]
    return s + [(768, 768), (2, 768)]


def timed(fn, passes):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(passes):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    plan = _lib.plan_for(grids.ant_flint(4, True))
    L = _lib.ctypes.CDLL(_lib.LIB_PATH)          # a handle of its own: the declared signature stays out of the binding's
    L.antq_decode4.restype = _lib.ctypes.c_int
    L.antq_decode4.argtypes = [_lib.ctypes.c_void_p, _lib.ctypes.c_void_p, _lib.ctypes.c_size_t, _lib.ctypes.c_size_t, _lib.ctypes.c_void_p,
                   _lib.ctypes.c_int, _lib.ctypes.c_float, _lib.ctypes.c_void_p, _lib.ctypes.c_void_p, _lib.ctypes.c_int,
                   _lib.ctypes.c_uint, _lib.ctypes.c_int, _lib.ctypes.c_void_p]
    lines = ["| workload | tensors | output MB | batched us | per-tensor loop us | copy us | loop / batched | batched / copy |",
             "|---|---|---|---|---|---|---|---|"]
    for name, shapes in (("ResNet-50", resnet50()), ("BERT-base", bert_base()), ("32 x 4096^2", [(4096, 4096)] * 32)):
        shapes = [(r, k) for r, k in shapes if k % 8 == 0]          # (conv1's K = 147 has no packed form)
        out_bytes = sum(r * k * 2 for r, k in shapes)
        nsets = max(2, -(-(640 << 20) // int(out_bytes * 1.25)))     # rotate past the 256 MiB Infinity Cache
        nsets = min(nsets, 48)
        sets, batches = [], []
        for _ in range(nsets):
            jobs = []
            for r, k in shapes:
                codes = torch.randint(0, 256, (r * k // 2,), dtype=torch.uint8, device=dev)
                jobs.append((codes, torch.empty(r * k, dtype=torch.bfloat16, device=dev), torch.rand(r, device=dev) + 0.5, plan, 10.0, r, k, True, 0))
            sets.append(jobs)
            batches.append(_lib.DecodeBatch(jobs))
        src = [torch.empty(out_bytes, dtype=torch.uint8, device=dev) for _ in range(nsets)]
        dst = [torch.empty(out_bytes, dtype=torch.uint8, device=dev) for _ in range(nsets)]

        def loop(k=0):
            for c, o, a, p, gm, r, kk, pr, nn in sets[k % nsets]:
                L.antq_decode4(c.data_ptr(), o.data_ptr(), r, kk, a.data_ptr(), 1, _lib.ctypes.c_float(gm), p.host_ptr(),
                                        p.dev(dev).data_ptr(), 0, 0, _lib.BF16, None)
        passes = max(20, min(400, int(2e9 / max(out_bytes, 1))))
        for w in range(3):                                            # clocks settle, code objects load: all three paths
            timed(lambda k=0: batches[k % nsets].run(), 10)
            timed(loop, 10)
            timed(lambda k=0: _lib.copy(src[k % nsets], dst[k % nsets]), 10)
        res = []
        for rnd in range(3):                                          # alternate the three, keep the best of each
            res.append((timed(lambda k=0: batches[k % nsets].run(), passes), timed(loop, passes),
                        timed(lambda k=0: _lib.copy(src[k % nsets], dst[k % nsets]), passes)))
        tb, tl, tc = (min(r[i] for r in res) for i in range(3))
        lines.append("| %s | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.2f |" % (name, len(shapes), out_bytes / 1e6, tb, tl, tc, tl / tb, tb / tc))
        print(lines[-1], flush=True)
        del sets, batches, src, dst
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
