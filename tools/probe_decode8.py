"""The byte-code decoder against its yardsticks, in one process (profiles/packed_bytes.md):
    A  antq_decode8_batch on byte codes
    B  antq_decode4_batch on 4-bit codes of the same shapes (the same number of output bytes; the 4-bit book of the same family)
    C  antq_fakequant_batch on the float weights with the 8-bit book: what those layers cost per refresh without byte codes
for ANT int-8 and OliVe int-8 (+ outliers), bf16 and fp32, on BERT-base's 74 weight shapes, [4096, 4096] and [16384, 4096].
Every arm rotates over buffer sets of at least 1 GiB in all; one pass over the sets is captured in a graph and replayed; the
figure is the median of 5 measurements (device events around the replays), the arms taken in turn within each measurement.
Then one whole-model line: a stack of BERT-base's 74 Linear layers with set_8_bit_layer_n(model, 8), packed with and without
byte_codes: weight launches per forward, resident bytes, checkpoint bytes (counts, not timings).
    python tools/probe_decode8.py [--out profiles/packed_bytes] [--quick]"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ant_quantization_amd import _lib, grids  # noqa: E402

PEAK = 8.0e12          # bytes / s


def bert_base():
    s = []
    for _ in range(12):
        s += [(768, 768)] * 4 + [(3072, 768), (768, 3072)]
    return s + [(768, 768), (2, 768)]


def books():
    """family -> (8-bit grid, gmax, n_normal, pair rule), (4-bit grid of the family, gmax, n_normal)"""
    o8n, o8o = grids.olive_int(8, True), grids.olive_outliers(8, True)
    o4n, o4o = grids.olive_int(4, True), grids.olive_outliers(4, True)
    return {"ant int-8": ((np.asarray(grids.ant_grid("int", 8, True), np.float32), 0, False), (np.asarray(grids.ant_grid("int", 4, True), np.float32), 0)),
            "olive int-8": ((np.concatenate([o8n, o8o]).astype(np.float32), int(len(o8n)), True),
                            (np.concatenate([o4n, o4o]).astype(np.float32), int(len(o4n))))}


def build_arms(shapes, dt, dev, book8, book4, ovp, gib):
    """-> {arm: (list of batches, one per buffer set; bytes moved per pass over ONE set)}"""
    g8, nn8, _ = book8
    g4, nn4 = book4
    p8, p4 = _lib.plan_for(g8), _lib.plan_for(g4)
    gmax8, gmax4 = float(g8[:nn8].max() if ovp else g8.max()), float(g4[:nn4].max() if ovp else g4.max())
    esz = torch.empty(0, dtype=dt).element_size()
    n = sum(r * k for r, k in shapes)
    per_set = {"A": n * (1 + esz), "B": n * 0.5 + n * esz, "C": 2 * n * esz}
    arms = {}
    for arm in ("A", "B", "C"):
        nsets = max(2, -(-int(gib * (1 << 30)) // int(per_set[arm])))
        sets = []
        for _ in range(nsets):
            jobs = []
            for r, k in shapes:
                alpha = torch.rand(r, device=dev) * 0.05 + 0.02
                out = torch.empty(r * k, dtype=dt, device=dev)
                if arm == "A":
                    codes = torch.randint(0, 255 if ovp else 256, (r * k,), dtype=torch.uint8, device=dev)
                    jobs.append((codes, out, alpha, p8, gmax8, r, k, True, nn8))
                elif arm == "B":
                    codes = torch.randint(0, 256, (r * k // 2,), dtype=torch.uint8, device=dev)
                    jobs.append((codes, out, alpha, p4, gmax4, r, k, True, nn4))
                else:
                    x = (torch.randn(r, k, device=dev) * 0.02).to(dt)
                    jobs.append((x, out.view(r, k), alpha, p8, gmax8, r, k, True))
            sets.append(_lib.DecodeBatch(jobs, ovp=ovp, width=8) if arm == "A" else _lib.DecodeBatch(jobs, ovp=ovp) if arm == "B"
                        else _lib.Batch(jobs, ovp=ovp))
        arms[arm] = (sets, per_set[arm])
    return arms


def graph_of(sets):
    def one_pass():
        for b in sets:
            b.run()
    for _ in range(3):
        one_pass()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_pass()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one_pass()
    torch.cuda.synchronize()
    return g


def measure(arms, target_s, rounds=5):
    graphs = {a: graph_of(s) for a, (s, _) in arms.items()}
    reps = {}
    for a, g in graphs.items():            # size the window: replays until a measurement lasts about target_s
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        reps[a] = max(5, int(target_s / max(e0.elapsed_time(e1) / 5e3, 1e-6)))
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a, g in graphs.items():        # the arms in turn within every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[a]):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[a].append(e0.elapsed_time(e1) * 1e-3 / (reps[a] * len(arms[a][0])))      # seconds per pass over ONE set
    return {a: dict(us=float(np.median(t)) * 1e6, spread=float((max(t) - min(t)) / np.median(t)), replays=reps[a], sets=len(arms[a][0]),
                    bytes=arms[a][1], tbs=arms[a][1] / float(np.median(t)) / 1e12) for a, t in times.items()}


class BertStack(torch.nn.Module):
    """BERT-base's 74 Linear layers chained (q + k + v summed, out, fc1, GELU, fc2 with residuals; pooler, classifier): the
    weights and their order are the model's, attention scores / softmax / LayerNorm are left out -- they hold no weights."""

    def __init__(self):
        super().__init__()
        L = torch.nn.Linear
        self.blocks = torch.nn.ModuleList([torch.nn.ModuleList([L(768, 768), L(768, 768), L(768, 768), L(768, 768), L(768, 3072), L(3072, 768)])
                                           for _ in range(12)])
        self.pooler, self.classifier = L(768, 768), L(768, 2)

    def forward(self, x):
        for q, k, v, o, f1, f2 in self.blocks:
            x = x + o(q(x) + k(x) + v(x)) * 0.3
            x = x + f2(torch.nn.functional.gelu(f1(x))) * 0.3
            x = x / x.std()
        return self.classifier(torch.tanh(self.pooler(x)))


def whole_model(dev, dt, tree):
    import copy
    import importlib
    qmod = importlib.import_module("ant_quantization_amd.%s.quant_model" % tree)
    qutil = importlib.import_module("ant_quantization_amd.%s.quant_utils" % tree)
    qutil.set_quantizer(types.SimpleNamespace(w_up=150, a_up=150, w_low=75, a_low=75, percent=100, search=False, no_outlier=False,
                                              mode={"ant": "ant-int-pot-flint", "olive": "ant-int-flint"}[tree], wbit=4, abit=4))
    torch.manual_seed(0)
    model = qmod.quantize_model(BertStack()).to(dev).to(dt).eval()
    qutil.enable_quantization(model)
    x = torch.randn(16, 768, device=dev).to(dt)
    rows = []
    with torch.no_grad():
        model(x)
        qmod.set_8_bit_layer_n(model, 8)
        model(x)                           # calibrates again with the 8-bit layers
        for byte_codes in (False, True):
            m = copy.deepcopy(model)
            bank = qutil.pack_model(m, release_weights=True, byte_codes=byte_codes)
            m(x)
            before = bank.launches
            m(x)
            skipped = {n for n, _ in bank.skipped}
            w_float = sum(p.numel() * p.element_size() for n, p in m.named_parameters() if n.endswith(".weight") and n[:-7] in skipped)
            codes, images = bank.nbytes()
            sd = qutil.packed_state_dict(m)
            rows.append(dict(tree=tree, dtype=str(dt), byte_codes=byte_codes, packed_layers=len(bank.entries),
                             byte_coded_layers=sum(e["width"] == 8 for e in bank.entries.values()), skipped_layers=len(bank.skipped),
                             weight_launches_per_forward=len(bank.skipped) + (bank.launches - before),
                             resident_weight_bytes=int(codes + images + w_float), codes_bytes=int(codes), image_bytes=int(images),
                             float_weight_bytes=int(w_float),
                             transient_fakequant_bytes_per_forward=int(w_float),
                             checkpoint_bytes=int(sum(v.numel() * v.element_size() for v in sd.values() if torch.is_tensor(v)))))
            print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="prefix: writes <prefix>.json and <prefix>_tables.md")
    ap.add_argument("--quick", action="store_true", help="small rotation and short windows (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU fall-back for a measurement"
    dev = torch.device("cuda:0")
    gib, target = (0.05, 0.01) if args.quick else (1.0, 0.15)
    work = (("BERT-base 74 W", bert_base()), ("[4096, 4096]", [(4096, 4096)]), ("[16384, 4096]", [(16384, 4096)]))
    if args.quick:
        work = (("BERT-base 74 W", bert_base()[:8] + [(2, 768)]), ("[512, 4096]", [(512, 4096)]))
    rows, lines = [], ["| workload | book | dtype | A us | B us | C us | A TB/s (of 8) | B TB/s (of 8) | C TB/s (of 8) | A / B bytes per s | spread A / B / C |",
                       "|---|---|---|---|---|---|---|---|---|---|---|"]
    for wname, shapes in work:
        for family, (book8, book4) in books().items():
            for dt in (torch.bfloat16, torch.float32):
                arms = build_arms(shapes, dt, dev, book8, book4, book8[2], gib)
                r = measure(arms, target)
                rows.append(dict(workload=wname, book=family, dtype=str(dt), **{a: r[a] for a in r}))
                f = lambda a: "%.2f (%.0f %%)" % (r[a]["tbs"], 100 * r[a]["tbs"] * 1e12 / PEAK)      # noqa: E731
                lines.append("| %s | %s | %s | %.1f | %.1f | %.1f | %s | %s | %s | %.2f | %.1f %% / %.1f %% / %.1f %% |" % (
                    wname, family, str(dt).replace("torch.", ""), r["A"]["us"], r["B"]["us"], r["C"]["us"], f("A"), f("B"), f("C"),
                    r["A"]["tbs"] / r["B"]["tbs"], 100 * r["A"]["spread"], 100 * r["B"]["spread"], 100 * r["C"]["spread"]))
                print(lines[-1], flush=True)
                del arms
                torch.cuda.empty_cache()
    model_rows = []
    for tree in ("ant", "olive"):
        model_rows += whole_model(dev, torch.bfloat16, tree)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out + ".json", "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), quick=bool(args.quick), rotation_gib=gib, window_s=target, rounds=5,
                           decode=rows, model=model_rows), f, indent=1)
        with open(args.out + "_tables.md", "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
