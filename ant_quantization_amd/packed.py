"""Packed 4-bit weights: a calibrated model whose weights exist as codes (SURVEY 8f N4 at the module surface).

`antq_encode4` turns a calibrated weight into the quantised tensor itself -- two codes per byte, OliVe's identifier 15 for
the victim of a pair -- and `decode4(encode4(w))` is bit-identical to the fake-quantised weight the layer computes on every
forward under the condition include/antq.h states for the codec: finite, positive scales and |w / scale| within twice the
outermost grid value (elements beyond the scan's range encode as 0).  Calibration gives that: alpha is a clip ratio of at
least 0.5 times the row's abs-max (w_low / a_low are 75 by default).  A channel whose alpha is 0 or not finite, or a clip
window below 50 %, can make a packed layer differ from its fake-quant twin in the clipped elements.  `PackedBank(model)` keeps those codes instead of re-quantising: it takes the place of `weight_bank.WeightBank`
behind the same `q._bank` / `lookup()` protocol of `tensor_forward`, encodes every suitable weight once, and produces the
decoded images with ONE `antq_decode4_batch` launch per (device, dtype, pair rule) group.  Codes are frozen weights by
definition, so the schedule is resident: the images are decoded at construction, again after `.to()` / `.half()` moved or
retyped the buffers, and on `invalidate()`; a forward on an unchanged model launches nothing for packed layers.

Suitable = a steady-state quantiser whose codebook and row length the 4-bit codec accepts.  Everything else -- 8-bit layers
(`set_8_bit_layer_n/_l`), rows that are no multiple of 8 elements (conv1: K = 147), OliVe's unsigned codebook of 16 normal
values (no code left for the identifier), `base` / `outlier` modes, float64 -- keeps its float weight and its per-layer
fake-quant launch, and is listed in `.skipped` with the reason, as WeightBank does.

A forward that wants gradients through a packed quantiser raises AntqError: there is no float weight to train.

`release_weights=True` points each packed layer's `weight.data` at the bank's decoded buffer, so the float original is
freed: a packed layer then holds codes + one quantised copy instead of weight + quantised copy.  `state_dict()` of such a
model holds FAKE-QUANTISED weights, not the originals; `packed_state_dict(model)` is the checkpoint to write.

The scale a layer is decoded with is the quantiser's `alpha` as it is when the images are decoded (read as float32).

Checkpoint: `packed_state_dict(model)` = the quantiser state the reference's checkpoints already carry (same keys) plus
`<layer>.quant_weight.codes` (uint8, numel / 2 bytes) for packed layers and `<layer>.weight` only for skipped ones;
`load_packed_state_dict(model, sd)` loads it into a freshly wrapped, uncalibrated model without re-encoding.

`fused_linear=True` lets the packed Linear layers compute with the codes: a no-grad call whose quantised input has at most
`_lib.LINEAR4_MAX_M` rows (LLM decode, batch 1) and is a contiguous, 16-byte-aligned GPU tensor of the layer's dtype runs
`antq_linear4` -- y = x . W^T + bias straight from the codes, W being bit for bit the decoded image, the sum in fp32 in the
kernel's own fixed order (so the result is that of F.linear on the image up to the rounding of an fp32 sum, not its bits).
Every other call runs F.linear on the image as before.  `.fused_calls` counts the calls the kernel served.
`keep_images=False` (with fused_linear only) drops the decoded images of those layers: a call with more rows decodes that
one layer with `antq_decode4` into ONE scratch buffer owned by the bank -- sized to the largest such layer per (device,
dtype) -- and runs F.linear on it.  The scratch is valid only until the next such layer's call on the same stream: nothing
may keep a reference to it (a captured graph is fine, a side stream or autograd through the input is not).  With
`release_weights=True` such a layer's `weight.data` becomes an empty tensor (the bank remembers the shape): a deep copy
of such a model has no weights to fall back on, and a forward with the layer's quantiser disabled raises AntqError.  Conv layers and skipped layers behave as without the options.

`fused_rows=R` (with fused_linear; LINEAR4_MAX_M < R <= LINEAR4_MM_MAX_M = 64) extends that to calls of 9 .. R rows of bfloat16 /
float16 layers: they run `antq_linear4_mm`, the same product on the matrix cores (`.fused_mm_calls` counts them), and with
`keep_images=False` decode nothing and leave the scratch buffer alone.  Calls of at most 8 rows still run `antq_linear4`,
float32 layers and every other call keep the path described above.  The two kernels sum in different orders: the same row of x
has different low bits from a 3-row and from a 9-row call (each within the bound of an fp32 sum, each independent of the other
rows).  Subnormal weights are kept by the MFMA (measured), so W is the image there too.  Without `fused_rows` nothing changes.
What the A/B found (profiles/packed_linear_mm.md): one MI355X, one run, M = 8 / 16 / 32 / 64, bf16 and f16, ANT flint-4 and
OliVe; A = F.linear on the image, C = antq_decode4 into scratch + F.linear, B = antq_linear4_mm.  Largest M up to which B
beats A / beats C in all four runs, per layer [N, K]: [4096, 4096] A 32, C 64; [16384, 4096] A 64, C 64; [4096, 16384] A 16, C
64; [3072, 768] A 64, C 64; [768, 3072] A 16, C 32.  At M = 8 B is faster than antq_linear4 in 20 of 20 rows (1.27-1.82x), so
M = 5 ... 8 would be better served by it (only M = 8 was timed; the routing keeps antq_linear4 up to 8 rows).  B never streams
the codes at more than 21 % of 8 TB/s; its time grows with M (x is re-read from L2 by every workgroup) and with fewer, larger
workgroups, and did not change with a deeper load ring: it appears bound by the x stream from L2 at M >= 32 and by parallelism
and the table look-ups below -- inferred from the scaling, no hardware counters were collected.  Not measured: other M, the
4-byte code path, per-tensor scales, a whole model, more than one run per point.  The 16-bit MFMA keeps subnormal operands
(measured): W is the image there too.

`fused_gemm_rows=R` (with fused_linear; LINEAR4_MM_MAX_M = 64 < R <= LINEAR4_GEMM_MAX_M = 4096; off by default -- without it
everything above is unchanged) extends the same to calls with more rows than the other kernels take -- more than 8, or more than
`fused_rows` when that is given -- and at most R rows of bfloat16 / float16 4-bit layers: they run `antq_linear4_gemm`, a tiled
matrix-core product straight from the codes (`.fused_gemm_calls` counts them; one fp32 accumulator chain per output, its own
order of the sum), and with `keep_images=False` decode nothing and leave the scratch buffer alone, so the scratch's lifetime rule
does not apply to them.  Calls of more than R rows, float32 layers and byte-coded entries keep the paths above.
Measured (profiles/packed_linear4_gemm.md; one MI355X, one run, 5 repetitions of 200 graph-replayed calls per point with the
arms alternated, medians, spread below 8 %; M = 64 / 128 / 256 / 512 / 1024 / 4096, the five layer shapes above, bf16 and f16,
ANT flint-4 and OliVe, per-row scales; A = F.linear on the kept image, C = antq_decode4 into scratch + F.linear, B =
antq_linear4_gemm): B LOSES to C and to A at all 120 points, so there is no M up to which the option is worth choosing for
speed on any layer measured.  Closest to C: [16384, 4096] at M = 128 / 256 (C / B 0.83 ... 0.92) and [3072, 768] at M = 512 /
1024 (0.65 ... 0.84); elsewhere B takes 1.3 ... 5 times C's time (3.6 ... 3.9 times at M = 4096 on the wide layers), and at M =
64 it takes 2.9 ... 4.7 times antq_linear4_mm's, so give fused_rows=64 beside it.  The kernel tops out at 356 ... 404 TFLOP/s,
a quarter of F.linear's rate: one workgroup per CU, and by the count of LDS instructions per step the table look-ups (every
wavefront decodes all 64 output rows of the tile itself) and the two barriers per step bound it -- inferred from arithmetic
and scaling, no hardware counters.  What the option buys is the memory (no decoded image, a quarter of the weight bytes) and
the free scratch buffer, at those prices.  Not measured: other M, the 4-byte code path, per-tensor scales, a whole model's
forward, more than one run.

`byte_codes=True` (pack_model, PackedBank; off by default -- without it everything above is unchanged): a layer the 4-bit codec
refuses for its codebook (the 5- to 8-bit layers of `set_8_bit_layer_n/_l`, OliVe's unsigned 16 + 15 values) or for its row
length (4 mod 8, such as 20) and that the byte codec accepts -- at most 256 values, with OliVe at most 255 normal and 255 outlier
values, rows of a multiple of 4 elements -- is encoded with `antq_encode8`, one code per byte, 255 the pair identifier: an entry
with `width == 8`.  Layers the 4-bit codec accepts keep 4-bit codes.  What stays in `.skipped`: rows that are no multiple of 4
(conv1: K = 147), `base` / `outlier` modes, float64, quantisers that are disabled or not calibrated.  Byte-coded layers are decoded
by `antq_decode8_batch`, one more launch per (device, dtype, pair rule) group (`.launches` counts it).  `antq_linear4` and
`antq_linear4_mm` do not take byte codes: without `fused_bytes` (below) such a layer is never fusable, always keeps its decoded
image (also under `keep_images=False`) and runs F.linear on it.  `release_weights`, `nbytes()` and the gradient error work on it as on
any image-keeping layer.  `packed_state_dict` writes its codes as numel bytes; `load_packed_state_dict` takes the width from the
stored size (numel / 2: 4-bit, numel: bytes; anything else raises AntqError naming the layer).  Measured
(profiles/packed_bytes.md): BERT-base's 74 Linear layers with 8 pairs at 8 bit -- 0 instead of 8 weight launches per forward,
checkpoint 48.9 instead of 60.1 MB, resident bytes 219.4 instead of 208.2 MB (codes are added, the image replaces the float weight).

`fused_bytes=True` (with fused_linear, else AntqError; off by default -- without it everything above is unchanged): a byte-coded
entry that is a 2-D Linear weight with in_features = K and K % 8 == 0 is fusable.  Its no-grad calls of at most
`_lib.LINEAR8_MAX_M` = 8 rows, under the input conditions of the 4-bit path, run `antq_linear8` -- the same product from the byte
codes, W bit for bit the image `antq_decode8` writes (`.fused_byte_calls` counts them; `.fused_calls` stays antq_linear4's).
`fused_rows` does not apply to byte entries (their matrix-core form has an option of its own, `fused_byte_rows` below): without
that one, calls of more rows run F.linear on the image or, with `keep_images=False`, on the scratch decode (`antq_decode8` into
the bank's one scratch buffer, which is sized to the largest image-less layer of either width).  `release_weights`, the "float weight is gone" error, the disabled-quantiser path and `.to()`
/ `.half()` behave as for the 4-bit layers.  Other byte-coded layers (K = 20, conv layers) keep their image as before.
Measured (profiles/packed_linear8.md; one MI355X, one run, 5 rounds per point, medians; OPT-6.7B's and BERT-base's shapes, M = 1,
2, 4, 8, bf16 / f16 / fp32, ANT int-8 and OliVe int-8): antq_linear8 beats decode8 + F.linear at all 120 points (1.2-6.5x); against
F.linear on the kept image it wins everywhere at M = 1 (1.3-3.2x) and M = 2 (1.07-2.0x), at M = 4 everywhere but four 16-bit
points (0.80-0.99x), and at M = 8 it LOSES on most 16-bit shapes (down to 0.61x) and on the wide fp32 layers (0.86-0.92x).
BERT-base with 8 pairs at 8 bits, bf16: 216.8 MB resident with byte_codes=True, 50.4 MB with fused_linear, fused_bytes and
keep_images=False.

`fused_byte_rows=R` (with fused_linear and fused_bytes, else AntqError naming the missing one; LINEAR8_MAX_M < R <=
LINEAR8_MM_MAX_M = 64; off by default -- without it everything above is unchanged): no-grad calls of 9 .. R rows of a fusable
byte-coded bfloat16 / float16 layer, under the same input conditions, run `antq_linear8_mm` -- the product on the matrix cores
from the byte codes, W bit for bit the image `antq_decode8` writes (`.fused_byte_mm_calls` counts them) -- and with
`keep_images=False` decode nothing and leave the scratch buffer alone.  Calls of at most 8 rows still run `antq_linear8`; float32
layers, calls of more than R rows and banks without the option keep the paths above.  `fused_rows` keeps meaning 4-bit entries
only.  The two byte kernels sum in different orders: the same row of x has different low bits from a 3-row and from a 9-row call
(each within the bound of an fp32 sum, each independent of the other rows).
Measured (profiles/packed_linear8_mm.md; one MI355X, one run, 5 rounds per point with the arms alternated, medians, spread below
6 %; M = 8 / 16 / 32 / 64, bf16 and f16, ANT int-8 and OliVe int-8, per-row scales; A = F.linear on the kept image, C =
antq_decode8 into scratch + F.linear, B = antq_linear8_mm).  Largest M up to which B beats A / beats C in all four runs, counted
from M = 8, per layer [N, K]: [4096, 4096] A 0, C 64; [16384, 4096] A 0, C 64; [4096, 16384] A 0, C 64; [3072, 768] A 64, C 64;
[768, 3072] A 0, C 32.  The zeros are M = 8 (which the option does not route: B loses to A there in at least one of the four runs); the M at
which B beats A in all four runs are [4096, 4096] 16; [16384, 4096] 16, 32; [4096, 16384] 16; [3072, 768] 8 ... 64; [768, 3072]
none (M = 16: 0.995 ... 1.29x).  So: against the scratch decode (keep_images=False) the option is worth turning on for every
layer measured up to R = 64 except [768, 3072], where R = 32 is the limit (M = 64: 0.78 ... 1.01x); against kept images it pays at
M = 16 (1.0 ... 1.3x) and, beyond that, only on [16384, 4096] at 32 (1.05x) and [3072, 768] up to 64 (1.16 ... 1.53x) -- at M = 64
B takes up to twice A's time on the other layers (0.51 ... 0.83x), and what the option buys there is the memory and the free
scratch.  At M = 8 B beats antq_linear8 in 12 of 20 rows only (0.81 ... 1.41x): the routing up to 8 rows stays.  The tile rule of
the 4-bit kernel (mm_ntiles) was within 7.5 % of the best forced shape in every row and is kept.  Not measured: other M, per-tensor
scales, the 8-byte code path, a whole model's forward time, more than one run; no hardware counters were collected.

`fused_byte_gemm_rows=R` (with fused_linear and fused_bytes, else AntqError naming the missing one; LINEAR8_MM_MAX_M = 64 < R <=
LINEAR8_GEMM_MAX_M = 4096; off by default -- without it everything above is unchanged) is `fused_gemm_rows` for the byte-coded
entries: no-grad calls of a fusable byte-coded bfloat16 / float16 layer with more rows than the other byte kernels take -- more
than 8, or more than `fused_byte_rows` when that is given -- and at most R rows run `antq_linear8_gemm`, the same tiled
matrix-core kernel instantiated for byte codes (W bit for bit the image `antq_decode8` writes, one fp32 accumulator chain per
output, its own order of the sum; `.fused_byte_gemm_calls` counts them), and with `keep_images=False` decode nothing and leave
the scratch buffer alone.  Calls of more than R rows, float32 layers and non-fusable byte entries keep the paths above;
`fused_gemm_rows` keeps meaning 4-bit entries only.  A mixed-precision model packed with both options, `keep_images=False` and
R at least its largest call needs no scratch decode at all: the scratch's lifetime rule then binds no layer.
Measured (profiles/packed_linear8_gemm.md; one MI355X, one run, 5 repetitions of graph-replayed calls per point -- 200 per graph
up to M = 512, 50 beyond -- with the arms alternated, medians, spread below 11 %; M = 64 / 128 / 256 / 512 / 1024 / 4096, the five
layer shapes above, bf16 and f16, ANT int-8 and OliVe int-8, per-row scales; A = F.linear on the kept image, C = antq_decode8
into scratch + F.linear, B = antq_linear8_gemm): B LOSES to C and to A at all 120 points (C / B 0.17 ... 0.78, A / B 0.09 ... 0.46),
so no R is worth choosing for speed on any layer measured.  Closest to C: [16384, 4096] at M = 64 ... 256 (0.61 ... 0.78) and
[3072, 768] up to M = 1024 (0.50 ... 0.69); elsewhere B takes 2.2 ... 6 times C's time (4.3 ... 5 times at M = 4096 on the wide
layers), and at M = 64 it takes 2.8 ... 6.1 times antq_linear8_mm's, so give fused_byte_rows=64 beside it.  The kernel tops out at
255 ... 304 TFLOP/s against the 4-bit form's 356 ... 404: it makes 128 table look-ups per wavefront and step, twice as many.
With the plain book the launcher's shared tile rule chose 256 rows per workgroup at 18 points where 128 were 8 ... 20 % faster
(two 64 KB workgroups fit a CU); the rule was left alone.  What the option buys is the memory (no decoded image, half the weight
bytes) and the free scratch buffer, at those prices.  Not measured: other M, the 8-byte code path, per-tensor scales, a whole
model's forward, more than one run; no hardware counters.  Not built: one decode of a B fragment shared by the workgroup's
wavefronts.

`fused_conv1d=True` (with fused_linear, else AntqError; off by default -- without it everything above is unchanged) is for GPT-2,
whose projections are all HF `Conv1D` layers behind OliVe's `Conv1dQuantizer`: weight [in, out] = [K, N], y = x @ W + b, one scale
per INPUT feature k, the pairs of the pair rule adjacent output columns.  Such a layer is packed with or without the option (the
codec does not care about orientation), but no other kernel can sum across the rows of its codes: without the option it always
keeps its decoded image, also under `keep_images=False`, and runs its `addmm` on it.  With the option a 4-bit entry whose module is
a Conv1dQuantizer with a 2-D weight, `w.shape[1] == nf` and `w.shape[0] % 8 == 0` is fusable with kind `conv1d`: its no-grad calls
of at most `_lib.LINEAR4_T_MAX_M` = 8 rows, under the input conditions of the 4-bit path, run `antq_linear4_t` -- the product from
the codes, W[k, n] bit for bit the image `antq_decode4` writes, the sum in fp32 in the kernel's own fixed order, a function of K
alone (`.fused_t_calls` counts them).  Every other call runs the layer's own `addmm` (`_conv_forward`, so the bits are today's) on
the image or, with `keep_images=False`, on the scratch decode; the scratch's lifetime rule is the same.  `fused_rows` and
`fused_gemm_rows` do not apply to `conv1d` entries (there is no matrix-core form for this layout); byte-coded Conv1D entries keep
their image as byte entries did before `fused_bytes`.  `release_weights` and the "float weight is gone" error behave as for Linear
entries.
Measured (profiles/packed_linear_t.md; one MI355X, one run, 5 repetitions of graph-replayed calls per point -- 200 ... 1200 per
graph, each arm rotating over more than 256 MiB of distinct weights where 1200 calls reach that -- with the arms alternated,
medians, spread below 4.3 %; M = 1 / 2 / 4 / 8, GPT-2 small's and GPT-2 XL's four Conv1D shapes [K, N], bf16 / f16 / fp32, ANT
flint-4 and OliVe flint with the pair rule, one scale per k; A = addmm on the kept image, C = antq_decode4 into scratch + addmm,
B = antq_linear4_t; 192 points).  Against C, the path `keep_images=False` would otherwise take: B wins at all 48 points of M = 1
(1.02 ... 2.26x), at 40 of 48 at M = 2 (0.73 ... 1.89x), 32 of 48 at M = 4 (0.59 ... 1.92x) and 21 of 48 at M = 8 (0.52 ... 1.56x);
it loses on the long-K layers [3072, 768] and [6400, 1600] in f16 / bf16 from M = 2 on.  Against A: B wins only at M = 1 -- at 30
of 48 points, 0.72 ... 1.28x: on GPT-2 XL's [1600, 4800], [1600, 1600] and [1600, 6400] in every run (1.03 ... 1.19x) and in fp32 on
every layer (1.06 ... 1.28x) -- and LOSES at every point of M = 2 (0.48 ... 1.00x), M = 4 (0.38 ... 0.93x) and M = 8 (0.34 ... 0.76x).
The codes stream at 0.2 ... 4.5 % of 8 TB/s: the kernel is nowhere near a stream.  Its time follows K, not N -- it is bound by
each lane's chain of dependent steps and by 10 ... 20 instructions per weight (every pair is scaled and rounded per use), with
24 ... 200 workgroups on 256 CUs; inferred from the scaling and the ISA, no hardware counters were collected.  The tile is half
the first one built (64 columns, 64 phases), which was 1.06 ... 1.66x slower at M >= 4 and K >= 3072 and 8 ... 16 % faster at M = 1
with K = 768.  So the option buys a GPT-2 the memory (no decoded image: a quarter of the bf16 bytes) and, at batch 1, roughly the
speed of the image; with kept images it is not worth turning on beyond one row.  Not measured: other M, per-tensor scales,
K > 8192, a whole model's decode step, more than one run, smaller tiles or a tile chosen by N.
"""
import torch
import torch.nn.functional as F

from . import _lib
from ._model import load_ant_state_dict
from .weight_bank import _weight_layers

__all__ = ["PackedBank", "pack_model", "packed_state_dict", "load_packed_state_dict"]

CODES_KEY = "quant_weight.codes"


def _codebook(q):
    """(plan, gmax, n_normal, ovp) of a steady-state quantiser as the codec takes them."""
    plan = q._ensure_plan()
    ovp = getattr(q, "_no_outlier", True) is False
    return plan, float(q._gmax), (int(q.quant_grid.numel()) if ovp else 0), ovp


def _settle(q):
    """A quantiser whose state came from a checkpoint: learn on the host what its first forward would (one read-back)."""
    q._hm_get('bit')
    if q._hm_get('has_inited_quant_para') != 0:
        q._ensure_plan()
        q._steady = True


class PackedBank:
    def __init__(self, model, release_weights=False, codes=None, fused_linear=False, keep_images=True, fused_rows=None,
                 byte_codes=False, fused_bytes=False, fused_byte_rows=None, fused_gemm_rows=None, fused_byte_gemm_rows=None,
                 fused_conv1d=False):
        """codes: {layer name: uint8 tensor} -- stored codes to attach instead of encoding the weights (load_packed_state_dict);
        a layer's code width is then the one its stored size says (numel / 2 bytes: 4-bit, numel bytes: byte codes).
        byte_codes: layers the 4-bit codec refuses and the byte codec accepts are packed one code per byte (width 8).
        fused_bytes (with fused_linear): byte-coded Linear layers of K % 8 == 0 compute from their codes too (antq_linear8).
        fused_byte_rows=R (with fused_linear and fused_bytes): their bf16 / f16 calls of 9 .. R rows too (antq_linear8_mm).
        fused_gemm_rows=R (with fused_linear): bf16 / f16 calls of the 4-bit layers with more rows than the other kernels take
        and at most R rows run antq_linear4_gemm.
        fused_byte_gemm_rows=R (with fused_linear and fused_bytes): the same for the byte-coded layers (antq_linear8_gemm).
        fused_conv1d (with fused_linear): 4-bit Conv1dQuantizer layers (weight [K, N]) of K % 8 == 0 compute calls of at most
        _lib.LINEAR4_T_MAX_M rows from their codes (antq_linear4_t); fused_rows / fused_gemm_rows do not apply to them."""
        self.byte_codes = bool(byte_codes)
        if fused_conv1d and not fused_linear:
            raise _lib.AntqError("PackedBank: fused_conv1d needs fused_linear=True")
        self.fused_conv1d = bool(fused_conv1d)   # 4-bit Conv1D layers ([K, N] weights) with few input rows compute from the codes (antq_linear4_t)
        self.fused_t_calls = 0     # forwards antq_linear4_t served
        if fused_bytes and not fused_linear:
            raise _lib.AntqError("PackedBank: fused_bytes needs fused_linear=True")
        _check_fused_byte_rows("PackedBank", fused_linear, fused_bytes, fused_byte_rows)
        self.fused_bytes = bool(fused_bytes)     # byte-coded Linear layers with few input rows compute from the codes (antq_linear8)
        self.fused_byte_calls = 0  # forwards antq_linear8 served
        self.fused_byte_rows = None if fused_byte_rows is None else int(fused_byte_rows)   # bf16 / f16 calls of 9 .. R rows: antq_linear8_mm
        self.fused_byte_mm_calls = 0   # forwards antq_linear8_mm served
        _check_fused_byte_gemm_rows("PackedBank", fused_linear, fused_bytes, fused_byte_gemm_rows)
        self.fused_byte_gemm_rows = None if fused_byte_gemm_rows is None else int(fused_byte_gemm_rows)   # bf16 / f16 calls of more rows, up to this many: antq_linear8_gemm
        self.fused_byte_gemm_calls = 0     # forwards antq_linear8_gemm served
        if not keep_images and not fused_linear:
            raise _lib.AntqError("PackedBank: keep_images=False needs fused_linear=True (nothing else computes from the codes)")
        _check_fused_rows("PackedBank", fused_linear, fused_rows)
        self.fused_rows = None if fused_rows is None else int(fused_rows)   # bf16 / f16 calls of 9 .. fused_rows rows: antq_linear4_mm
        self.fused_mm_calls = 0    # forwards antq_linear4_mm served
        _check_fused_gemm_rows("PackedBank", fused_linear, fused_gemm_rows)
        self.fused_gemm_rows = None if fused_gemm_rows is None else int(fused_gemm_rows)   # bf16 / f16 calls of more rows, up to this many: antq_linear4_gemm
        self.fused_gemm_calls = 0  # forwards antq_linear4_gemm served
        self.model = model
        self.release_weights = bool(release_weights)
        self.fused_linear = bool(fused_linear)   # Linear layers with few input rows compute from the codes (antq_linear4)
        self.keep_images = bool(keep_images)
        self.fused_calls = 0       # forwards antq_linear4 served
        self._scratch = {}         # (device, dtype) -> the one decode buffer of the layers without an image
        self.entries = {}          # id(quantiser) -> dict
        self.skipped = []          # (layer name, reason): layers that keep their float weight and per-layer launch
        self.launches = 0          # decode launches so far (one per (device, dtype, pair rule, code width) group and refresh)
        self.dirty = True
        self._batches = []
        self._ptr_key = None
        try:
            for name, mod, q, w in _weight_layers(model):
                if codes is not None and name in codes:
                    # stored codes say their own width; the layer has to be packable at that width
                    nc = int(codes[name].numel())
                    if codes[name].dtype != torch.uint8 or (nc * 2 != w.numel() and nc != w.numel()):
                        raise _lib.AntqError("PackedBank: codes of layer %s must be uint8 of numel/2 bytes (4-bit) or numel bytes "
                                             "(byte codes); got %d %s values for %d elements" % (name, nc, codes[name].dtype, w.numel()))
                    width, reason = self._width(q, w, only=8 if nc == w.numel() else 4)
                else:
                    width, reason = self._width(q, w, byte_codes=self.byte_codes)
                if reason is None and codes is not None and name not in codes:
                    reason = "no codes in the checkpoint"
                if reason:
                    if codes is not None and name in codes:
                        raise _lib.AntqError("PackedBank: stored codes for layer %s, which cannot be packed (%s)" % (name, reason))
                    self.skipped.append((name, reason))
                    continue
                per_row = bool(q.is_perchannel)
                rows, row_len = (w.shape[0], w.numel() // w.shape[0]) if per_row else (1, w.numel())
                plan, gmax, n_normal, ovp = _codebook(q)
                if codes is not None:
                    c = codes[name].to(w.device).contiguous()
                else:
                    with torch.no_grad():
                        alpha = q.alpha.detach().reshape(-1).to(torch.float32).contiguous()
                        enc = _lib.encode4 if width == 4 else _lib.encode8
                        c = enc(w.detach(), alpha, plan, gmax, rows, row_len, per_row, n_normal=n_normal, ovp=ovp)
                # (byte codes: only with fused_bytes -- without it a byte-coded layer always keeps its image)
                fusable = ((width == 4 or self.fused_bytes) and self.fused_linear and w.dim() == 2
                           and getattr(mod, "in_features", None) == w.shape[1] and w.shape[1] % 8 == 0)
                kind = "linear"
                if (self.fused_conv1d and width == 4 and _is_conv1d(mod) and w.dim() == 2 and getattr(mod, "nf", None) == w.shape[1]
                        and w.shape[0] % 8 == 0):
                    fusable, kind = True, "conv1d"     # weight [K, N]: the codes' rows are k (antq_linear4_t)
                image = self.keep_images or not fusable
                self.entries[id(q)] = dict(name=name, q=q, mod=mod, rows=rows, row_len=row_len, per_row=per_row, codes=c, width=width,
                                           fusable=fusable, kind=kind, shape=tuple(w.shape), dtype=w.dtype, device=w.device,
                                           out=torch.empty_like(w, memory_format=torch.contiguous_format) if image else None)
            if not self.entries:
                raise _lib.AntqError("PackedBank: no weight quantiser to pack (run one forward to calibrate first): %r" % (self.skipped,))
            for e in self.entries.values():
                old = e["q"]._bank
                if old is not None and old is not self:
                    old.detach()
                e["q"]._bank = self
            self.refresh()
        except BaseException:      # (out of memory half way through: leave nothing attached)
            self.detach()
            raise
        _no_auto_bank(model)

    def __deepcopy__(self, memo):       # (a copy of the model starts without a bank, like WeightBank's)
        return None

    def __reduce__(self):
        return (type(None), ())

    @staticmethod
    def _unsuitable(q, w, byte_codes=False):
        """Why this layer stays float (None: it can be packed).  What the codec refuses comes first, where the weight lives
        last: the answer for a model's layers is the same before and after it moved to the GPU."""
        return PackedBank._width(q, w, byte_codes=byte_codes)[1]

    @staticmethod
    def _width(q, w, byte_codes=False, only=None):
        """(code width, None) of a layer that can be packed -- 4 where the 4-bit codec takes it, 8 (byte_codes only) where
        that one refuses the codebook or the row length and the byte codec does not -- or (None, why it stays float).
        only: the width stored codes have; the layer has to be packable at exactly that one."""
        if q.mode in ("base", "outlier"):
            return None, "mode %s" % q.mode
        if not (q.is_enable and q.is_enable_weight):
            return None, "quantisation disabled"
        if not q._steady:
            return None, "not calibrated yet"
        if w.dtype not in _lib._DTYPES or w.dtype == torch.float64:
            return None, "dtype %s" % w.dtype
        row_len = w.numel() // w.shape[0] if q.is_perchannel else w.numel()

        def refusal(nibble):
            if row_len == 0 or row_len % (8 if nibble else 4) != 0:
                return "row length %d is not a multiple of %d" % (row_len, 8 if nibble else 4)
            plan, _, n_normal, ovp = _codebook(q)
            m = int(plan.grid.size)
            if nibble:
                if ovp:
                    if n_normal > 15:
                        return "%d normal values leave no code for the pair identifier" % n_normal
                    if m - n_normal > 15:
                        return "%d outlier values (the 4-bit codec holds 15)" % (m - n_normal)
                elif m > 16:
                    return "codebook of %d values (the 4-bit codec holds 16)" % m
            elif ovp:
                if n_normal > 255:
                    return "%d normal values leave no byte code for the pair identifier" % n_normal
                if m - n_normal > 255:
                    return "%d outlier values (the byte codec holds 255)" % (m - n_normal)
            elif m > 256:
                return "codebook of %d values (the byte codec holds 256)" % m
            return None

        if only == 8:
            width, reason = 8, refusal(False)
        else:
            width, reason = 4, refusal(True)
            if reason is not None and byte_codes and only is None:
                width, reason = 8, refusal(False)
        if reason is not None:
            return None, reason
        if not w.is_cuda or not w.is_contiguous():
            return None, "weight not resident / not contiguous"
        return width, None

    # ------------------------------------------------------------------ bookkeeping
    def invalidate(self):
        """The next lookup decodes every packed weight again (one launch per group)."""
        self.dirty = True

    mark_dirty = invalidate

    def nbytes(self):
        """(bytes of codes, bytes of decoded images and of the scratch buffers that stand in for dropped ones)"""
        return (sum(e["codes"].numel() for e in self.entries.values()),
                sum(t.numel() * t.element_size() for t in [e["out"] for e in self.entries.values() if e["out"] is not None]
                    + list(self._scratch.values())))

    def detach(self):
        for e in self.entries.values():
            if e["q"]._bank is self:
                e["q"]._bank = None
        self.entries.clear()
        self._batches = []

    def _pointers(self):
        return tuple((e["mod"].weight.dtype, e["mod"].weight.device, e["out"].data_ptr() if e["out"] is not None else 0, e["q"].alpha.data_ptr(), e["q"].alpha.dtype,
                      id(e["q"]._ensure_plan()), e["q"]._gmax) for e in self.entries.values())

    def _build(self):
        """(Re)build the descriptor tables: one batch per (device, dtype, pair rule, code width)."""
        groups, need = {}, {}
        for e in self.entries.values():
            q, w = e["q"], e["mod"].weight
            if e["dtype"] != w.dtype or e["device"] != w.device:      # .half() / .to(device) since
                if e["out"] is not None:
                    e["out"] = torch.empty(e["shape"], dtype=w.dtype, device=w.device)
                e["codes"] = e["codes"].to(w.device)
                e["dtype"], e["device"] = w.dtype, w.device
            plan, gmax, n_normal, ovp = _codebook(q)
            alpha = q.alpha.detach().reshape(-1)
            e["alpha32"] = None
            if alpha.dtype != torch.float32 or not alpha.is_contiguous() or alpha.device != w.device:
                # (a 16-bit model's alpha: the kernel reads a float32 copy, brought up to date in place at every refresh)
                alpha = e["alpha32"] = alpha.to(device=w.device, dtype=torch.float32).contiguous()
            e["alpha"] = alpha
            if e["out"] is None:           # no image: the codes are the weight (linear); one scratch per (device, dtype) stands in
                need[(w.device, w.dtype)] = max(need.get((w.device, w.dtype), 0), e["rows"] * e["row_len"])
                continue
            groups.setdefault((w.device, w.dtype, ovp, e["width"]), []).append(
                (e["codes"], e["out"], alpha, plan, gmax, e["rows"], e["row_len"], e["per_row"], n_normal))
        self._batches = [_lib.DecodeBatch(jobs, ovp=ovp, width=width) for (_, _, ovp, width), jobs in groups.items()]
        self._scratch = {k: (self._scratch[k] if k in self._scratch and self._scratch[k].numel() == n
                             else torch.empty(n, dtype=k[1], device=k[0])) for k, n in need.items()}
        self._ptr_key = self._pointers()

    # ------------------------------------------------------------------ the one launch
    @torch.no_grad()
    def refresh(self):
        if self._ptr_key is None or self._ptr_key != self._pointers():
            self._build()
        else:
            for e in self.entries.values():
                if e["alpha32"] is not None:
                    e["alpha32"].copy_(e["q"].alpha.detach().reshape(-1))
        for b in self._batches:
            b.run()
            self.launches += 1
        self.dirty = False
        if self.release_weights:
            for e in self.entries.values():
                w = e["mod"].weight
                if e["out"] is None:
                    if w.numel():
                        w.data = torch.empty(0, dtype=w.dtype, device=w.device)     # the codes are all there is
                elif w.data_ptr() != e["out"].data_ptr():
                    w.data = e["out"]        # the float original is freed; weight now IS the fake-quantised image

    def lookup(self, q, tensor, training=None):
        """Called from tensor_forward in steady state (the WeightBank protocol): the decoded image of this quantiser's
        weight, or None when the call has to take the per-layer path (not this layer's weight, quantiser re-armed)."""
        e = self.entries.get(id(q))
        if e is None or tensor is not e["mod"].weight:
            return None
        if training is None:
            training = torch.is_grad_enabled() and (tensor.requires_grad or q.alpha.requires_grad)
        if training:
            raise _lib.AntqError("layer %s is packed: its weight exists as %s codes, there is no float weight to train "
                                 "(run the forward under torch.no_grad())" % (e["name"], "4-bit" if e["width"] == 4 else "byte"))
        if not q._steady or not (q.is_enable and q.is_enable_weight):
            return None
        if self.dirty or e["dtype"] != tensor.dtype or e["device"] != tensor.device:
            self.refresh()
        if e["out"] is None:
            # (a layer without an image: the weight itself stands in until linear() below, which every call of such a layer
            # reaches; the mark tells it that this call was served here -- a disabled quantiser hands back the same tensor)
            e["served"] = True
            return tensor
        return e["out"]

    def _image(self, e):
        """The decoded image of a layer that keeps none, in the bank's scratch buffer (valid until the next such call)."""
        q = e["q"]
        plan, gmax, n_normal, ovp = _codebook(q)
        buf = self._scratch[(e["device"], e["dtype"])][:e["rows"] * e["row_len"]]
        dec = _lib.decode4 if e["width"] == 4 else _lib.decode8
        dec(e["codes"], e["alpha"], plan, gmax, e["rows"], e["row_len"], e["per_row"], e["dtype"], n_normal=n_normal, ovp=ovp, out=buf)
        return buf.view(e["shape"])

    def _fits(self, e, input, bias, K, max_rows):
        """Whether a call may run from the codes: a contiguous, 16-byte-aligned no-grad input [..., K] of at most max_rows rows
        in the layer's dtype on its device, the bias (if any) alike."""
        return (input.is_cuda and input.dtype == e["dtype"] and input.device == e["device"] and input.dim() >= 1 and input.shape[-1] == K
                and 0 < input.numel() <= max_rows * K and input.is_contiguous() and input.data_ptr() % 16 == 0
                and not (torch.is_grad_enabled() and (input.requires_grad or (bias is not None and bias.requires_grad)))
                and (bias is None or (bias.dtype == input.dtype and bias.is_contiguous() and bias.device == input.device)))

    def linear(self, mod, input, weight):
        """The output of a LinearQuantizer or Conv1dQuantizer whose weight quantiser this bank serves (fused_linear): `input`
        after quant_input, `weight` what quant_weight returned.  From the codes when the call qualifies, otherwise the layer's
        own product on the image: F.linear, or a Conv1dQuantizer's addmm (`_conv_forward`)."""
        conv = _is_conv1d(mod)
        q = mod.quant_weight
        e = self.entries.get(id(q))
        if e is not None and e["out"] is None:     # (lookup()'s own conditions again: a mark left by a call that failed is stale)
            served = e.pop("served", False) and weight is mod.weight and q._steady and q.is_enable and q.is_enable_weight
        else:
            served = e is not None and weight is e["out"]
        if not served or not e["fusable"]:         # not served by lookup(): the per-layer path's tensor, or the float weight
            if e is not None and e["out"] is None and mod.weight.numel() == 0:
                raise _lib.AntqError("layer %s was packed with keep_images=False and release_weights=True: its float weight is "
                                     "gone, so it cannot run with its quantiser disabled or re-calibrating (only from its "
                                     "codes)" % e["name"])
            return mod._conv_forward(input, weight) if conv else F.linear(input, weight, mod.bias)
        bias = mod.bias
        if e["kind"] == "conv1d":                  # weight [K, N]; fused_rows / fused_gemm_rows do not apply
            K, N = e["shape"]
            if self._fits(e, input, bias, K, _lib.LINEAR4_T_MAX_M):
                plan, gmax, n_normal, ovp = _codebook(e["q"])
                self.fused_t_calls += 1
                return _lib.linear4_t(e["codes"], input, e["alpha"], plan.grid_dev(e["device"]), gmax, N, K, e["per_row"],
                                      bias=None if bias is None else bias.detach(), n_normal=n_normal, ovp=ovp)
            return mod._conv_forward(input, weight if e["out"] is not None else self._image(e))
        K = e["shape"][1]
        byte = e["width"] == 8                     # (fused_rows is antq_linear4_mm's, fused_byte_rows antq_linear8_mm's)
        max_rows = _lib.LINEAR8_MAX_M if byte else _lib.LINEAR4_MAX_M
        more_rows = self.fused_byte_rows if byte else self.fused_rows
        gemm_rows = self.fused_byte_gemm_rows if byte else self.fused_gemm_rows     # (fused_gemm_rows is antq_linear4_gemm's)
        if e["dtype"] in (torch.bfloat16, torch.float16):
            if more_rows is not None:
                max_rows = more_rows
            if gemm_rows is not None:
                max_rows = gemm_rows               # (> LINEAR4_MM_MAX_M = LINEAR8_MM_MAX_M >= fused_rows, fused_byte_rows)
        if self._fits(e, input, bias, K, max_rows) and not (byte and e["codes"].data_ptr() % 8):
            plan, gmax, n_normal, ovp = _codebook(e["q"])
            if byte and input.numel() <= _lib.LINEAR8_MAX_M * K:
                self.fused_byte_calls += 1
                fn = _lib.linear8
            elif byte and self.fused_byte_rows is not None and input.numel() <= self.fused_byte_rows * K:
                self.fused_byte_mm_calls += 1
                fn = _lib.linear8_mm
            elif byte:                             # more rows than the other kernels take, at most fused_byte_gemm_rows
                self.fused_byte_gemm_calls += 1
                fn = _lib.linear8_gemm
            elif input.numel() <= _lib.LINEAR4_MAX_M * K:
                self.fused_calls += 1
                fn = _lib.linear4
            elif self.fused_rows is not None and input.numel() <= self.fused_rows * K:
                self.fused_mm_calls += 1
                fn = _lib.linear4_mm
            else:                                  # more rows than the other kernels take, at most fused_gemm_rows
                self.fused_gemm_calls += 1
                fn = _lib.linear4_gemm
            return fn(e["codes"], input, e["alpha"], plan.grid_dev(e["device"]), gmax, e["shape"][0], K, e["per_row"],
                      bias=None if bias is None else bias.detach(), n_normal=n_normal, ovp=ovp)
        return F.linear(input, weight if e["out"] is not None else self._image(e), bias)


def _check_rows_option(who, name, rows, needs, lo, hi):
    """rows is None, or an integer (not a bool) in (lo, hi] with every option of `needs` (name, value) switched on"""
    if rows is None:
        return
    for need, on in needs:
        if not on:
            raise _lib.AntqError("%s: %s needs %s=True" % (who, name, need))
    if not (isinstance(rows, int) and not isinstance(rows, bool) and lo < rows <= hi):
        raise _lib.AntqError("%s: %s must be an integer in (%d, %d] (got %r)" % (who, name, lo, hi, rows))


def _check_fused_rows(who, fused_linear, fused_rows):
    _check_rows_option(who, "fused_rows", fused_rows, (("fused_linear", fused_linear),), _lib.LINEAR4_MAX_M, _lib.LINEAR4_MM_MAX_M)


def _check_fused_byte_rows(who, fused_linear, fused_bytes, fused_byte_rows):
    _check_rows_option(who, "fused_byte_rows", fused_byte_rows, (("fused_linear", fused_linear), ("fused_bytes", fused_bytes)),
                       _lib.LINEAR8_MAX_M, _lib.LINEAR8_MM_MAX_M)


def _check_fused_gemm_rows(who, fused_linear, fused_gemm_rows):
    _check_rows_option(who, "fused_gemm_rows", fused_gemm_rows, (("fused_linear", fused_linear),), _lib.LINEAR4_MM_MAX_M,
                       _lib.LINEAR4_GEMM_MAX_M)


def _check_fused_byte_gemm_rows(who, fused_linear, fused_bytes, fused_byte_gemm_rows):
    _check_rows_option(who, "fused_byte_gemm_rows", fused_byte_gemm_rows, (("fused_linear", fused_linear), ("fused_bytes", fused_bytes)),
                       _lib.LINEAR8_MM_MAX_M, _lib.LINEAR8_GEMM_MAX_M)


def _is_conv1d(mod):
    """Whether `mod` is OliVe's Conv1dQuantizer (GPT-2's Conv1D: weight [in, out], y = x @ W + b)."""
    from .olive.quant_modules import Conv1dQuantizer       # (here: that module is loaded by whoever built such a layer)
    return isinstance(mod, Conv1dQuantizer)


def _no_auto_bank(model):
    """The automatic weight bank steps aside (as for set_weights_at_rest(resident=False)), and the choice stays with the
    module: a deep copy carries the mark, so its forward hook does not arm a fresh AutoBank for it."""
    ab = getattr(model, "_antq_auto_bank", None)
    if ab is not None:
        ab.disable()
    object.__setattr__(model, "_antq_no_auto_bank", True)


def _bank_of(model):
    for _, _, q, _ in _weight_layers(model):
        if isinstance(q._bank, PackedBank):
            return q._bank
    return None


def pack_model(model, release_weights=False, fused_linear=False, keep_images=True, fused_rows=None, byte_codes=False,
               fused_bytes=False, fused_byte_rows=None, fused_gemm_rows=None, fused_byte_gemm_rows=None, fused_conv1d=False):
    """Encode every suitable calibrated weight of `model` as 4-bit codes and serve the layers from one batched decode
    (PackedBank).  Returns the bank; `.skipped` lists the layers that stay float, with reasons.
    byte_codes: layers the 4-bit codec refuses for their codebook (5- to 8-bit layers, OliVe's unsigned 16 + 15) or their row
    length (4 mod 8) are packed one code per byte (entries of width 8, one more decode launch per group); they always keep
    their decoded image and run F.linear on it unless fused_bytes is given.
    fused_bytes (with fused_linear): byte-coded Linear layers of K % 8 == 0 compute calls of at most _lib.LINEAR8_MAX_M rows from
    their byte codes (antq_linear8, .fused_byte_calls) and, with keep_images=False, keep no image -- see the module docstring.
    fused_byte_rows=R (with fused_linear and fused_bytes, 8 < R <= 64): their bf16 / f16 calls of 9 .. R rows compute from the byte
    codes on the matrix cores (antq_linear8_mm, .fused_byte_mm_calls) and, with keep_images=False, leave the scratch alone.
    Measured (profiles/packed_linear8_mm.md, one MI355X, one run; A = F.linear on the image, C = antq_decode8 into scratch +
    F.linear, B = antq_linear8_mm): M at which B beats A / beats C in all four runs (bf16, f16, ANT and OliVe int-8), per
    layer [N, K]: [4096, 4096] A 16, C 8 ... 64; [16384, 4096] A 16, 32, C 8 ... 64; [4096, 16384] A 16, C 8 ... 64; [3072, 768] A
    8 ... 64, C 8 ... 64; [768, 3072] A none, C 8 ... 32.  Worth turning on with keep_images=False (R = 64; 32 for layers like
    [768, 3072]); with kept images only around M = 16 and for [3072, 768]-like layers.  Not measured: other M, per-tensor
    scales, a whole model's forward time, more than one run.
    fused_linear: Linear layers called with at most _lib.LINEAR4_MAX_M input rows compute from the codes (antq_linear4);
    keep_images=False (with fused_linear): those layers keep no decoded image -- see the module docstring.
    fused_rows=R (with fused_linear, 8 < R <= 64): bf16 / f16 calls of 9 .. R rows compute from the codes on the matrix cores
    (antq_linear4_mm); a row's low bits differ between the two kernels.
    Measured (profiles/packed_linear_mm.md): one MI355X, one run, M = 8 / 16 / 32 / 64, bf16 and f16, ANT flint-4 and
    OliVe; A = F.linear on the image, C = antq_decode4 into scratch + F.linear, B = antq_linear4_mm.  Largest M up to
    which B beats A / beats C in all four runs, per layer [N, K]: [4096, 4096] A 32, C 64; [16384, 4096] A 64, C 64;
    [4096, 16384] A 16, C 64; [3072, 768] A 64, C 64; [768, 3072] A 16, C 32.  At M = 8 B is faster than antq_linear4 in
    20 of 20 rows (1.27-1.82x), so M = 5 ... 8 would be better served by it (only M = 8 was timed; the routing keeps
    antq_linear4 up to 8 rows).  B never streams the codes at more than 21 % of 8 TB/s; its time grows with M (x is
    re-read from L2 by every workgroup) and with fewer, larger workgroups, and did not change with a deeper load ring: it
    appears bound by the x stream from L2 at M >= 32 and by parallelism and the table look-ups below -- inferred from the
    scaling, no hardware counters were collected.  Not measured: other M, the 4-byte code path, per-tensor scales, a whole
    model, more than one run per point.  The 16-bit MFMA keeps subnormal operands (measured): W is the image there too.
    fused_gemm_rows=R (with fused_linear, 64 < R <= 4096): bf16 / f16 calls of the 4-bit layers with more rows than the other
    kernels take (more than 8, or more than fused_rows) and at most R rows compute from the codes as a tiled matrix-core product
    (antq_linear4_gemm, .fused_gemm_calls) and, with keep_images=False, decode nothing and leave the scratch alone.
    Measured (profiles/packed_linear4_gemm.md, one MI355X, one run; A = F.linear on the image, C = antq_decode4 into
    scratch + F.linear, B = antq_linear4_gemm; M = 64 ... 4096, five layer shapes, bf16 / f16, ANT and OliVe): B loses to
    C and to A at all 120 points (C / B 0.20 ... 0.92, best on [16384, 4096] at M = 128 / 256), so no R is worth choosing
    for speed; the option buys the memory and the free scratch.  Give fused_rows=64 beside it (at M = 64 B takes 2.9 ...
    4.7 times antq_linear4_mm's time).  Not measured: other M, the 4-byte code path, per-tensor scales, a whole model.
    fused_byte_gemm_rows=R (with fused_linear and fused_bytes, 64 < R <= 4096): the same for the byte-coded layers -- their bf16 /
    f16 calls with more rows than the other byte kernels take (more than 8, or more than fused_byte_rows) and at most R rows
    compute from the byte codes as a tiled matrix-core product (antq_linear8_gemm, .fused_byte_gemm_calls) and, with
    keep_images=False, decode nothing and leave the scratch alone.  Measured (profiles/packed_linear8_gemm.md, one MI355X, one
    run; A / C / B as above with antq_decode8 and antq_linear8_gemm; M = 64 ... 4096, five layer shapes, bf16 / f16, ANT and
    OliVe int-8): B loses to C and to A at all 120 points (C / B 0.17 ... 0.78, best on [16384, 4096] at M = 64 ... 256; A / B
    0.09 ... 0.46), so no R is worth choosing for speed; the option buys the memory and a model without scratch decodes.  Give
    fused_byte_rows=64 beside it (at M = 64 B takes 2.8 ... 6.1 times antq_linear8_mm's time).  Not measured: other M, the 8-byte
    code path, per-tensor scales, a whole model.
    fused_conv1d (with fused_linear, else AntqError): the 4-bit Conv1dQuantizer layers of a GPT-2 (weight [K, N] with N = nf and
    K % 8 == 0) compute calls of at most _lib.LINEAR4_T_MAX_M rows from their codes (antq_linear4_t, .fused_t_calls) and, with
    keep_images=False, keep no image; calls of more rows run the layer's addmm on the image or on the scratch decode.
    fused_rows / fused_gemm_rows do not apply to them.  Measurements: see the module docstring (profiles/packed_linear_t.md)."""
    return PackedBank(model, release_weights=release_weights, fused_linear=fused_linear, keep_images=keep_images, fused_rows=fused_rows,
                      byte_codes=byte_codes, fused_bytes=fused_bytes, fused_byte_rows=fused_byte_rows, fused_gemm_rows=fused_gemm_rows,
                      fused_byte_gemm_rows=fused_byte_gemm_rows, fused_conv1d=fused_conv1d)


def packed_state_dict(model):
    """The checkpoint of a packed model: state_dict() without the packed layers' `.weight`, plus their codes."""
    bank = _bank_of(model)
    if bank is None:
        raise _lib.AntqError("packed_state_dict: the model is not packed (pack_model first)")
    return _packed_keys(model.state_dict(), {e["name"]: e["codes"] for e in bank.entries.values()})


def _packed_keys(sd, codes):
    """state_dict `sd` -> packed layout: `<layer>.weight` of every layer in `codes` leaves, `<layer>.quant_weight.codes` comes."""
    sd = type(sd)(sd)
    for name, c in codes.items():
        prefix = name + "." if name else ""
        sd.pop(prefix + "weight", None)
        sd[prefix + CODES_KEY] = c
    return sd


def load_packed_state_dict(model, sd, release_weights=True, fused_linear=False, keep_images=True, fused_rows=None,
                           fused_bytes=False, fused_byte_rows=None, fused_gemm_rows=None, fused_byte_gemm_rows=None, fused_conv1d=False):
    """Load a packed checkpoint into a freshly wrapped, uncalibrated model living on the GPU: the quantiser state is
    installed the way load_ant_state_dict + load_state_dict do (scales keep the dtype they were stored with), a PackedBank is attached from the stored codes without
    re-encoding (a layer's code width is the one its stored size says: numel / 2 bytes are 4-bit codes, numel bytes byte codes;
    any other size raises AntqError naming the layer), and the weights are materialised by the batched decode
    (release_weights=False: copied into the layers' own float weights instead of replacing them).  fused_linear / keep_images / fused_rows / fused_bytes / fused_byte_rows / fused_gemm_rows / fused_byte_gemm_rows / fused_conv1d: as in pack_model (the code width still comes from the stored size).  Returns the bank."""
    if not keep_images and not fused_linear:
        raise _lib.AntqError("load_packed_state_dict: keep_images=False needs fused_linear=True")
    _check_fused_rows("load_packed_state_dict", fused_linear, fused_rows)
    if fused_bytes and not fused_linear:
        raise _lib.AntqError("load_packed_state_dict: fused_bytes needs fused_linear=True")
    _check_fused_byte_rows("load_packed_state_dict", fused_linear, fused_bytes, fused_byte_rows)
    _check_fused_gemm_rows("load_packed_state_dict", fused_linear, fused_gemm_rows)
    _check_fused_byte_gemm_rows("load_packed_state_dict", fused_linear, fused_bytes, fused_byte_gemm_rows)
    if fused_conv1d and not fused_linear:
        raise _lib.AntqError("load_packed_state_dict: fused_conv1d needs fused_linear=True")
    suffix = "." + CODES_KEY
    codes = {k[:-len(suffix)]: v for k, v in sd.items() if k.endswith(suffix)}
    rest = {k: v for k, v in sd.items() if not k.endswith(suffix)}
    load_ant_state_dict(model, rest)
    missing, unexpected = model.load_state_dict(rest, strict=False)
    want_missing = {(n + "." if n else "") + "weight" for n in codes}
    if unexpected or set(missing) != want_missing:
        raise _lib.AntqError("load_packed_state_dict: checkpoint and model disagree (missing %s, unexpected %s)"
                             % (sorted(set(missing) ^ want_missing), sorted(unexpected)))
    # load_state_dict copies INTO the Parameters, so a bf16 / f16 model would round the checkpoint's float32 scales to its own
    # dtype (calibration leaves float32 alphas in such a model): install them as stored, the codes were made with those
    for name, module in model.named_modules():
        a = rest.get(name + ".alpha")
        if a is not None and hasattr(module, "quant_grid") and module.alpha.dtype != a.dtype:
            module.alpha.data = a.detach().clone().to(module.alpha.device)
    for _, _, q, _ in _weight_layers(model):
        _settle(q)
    bank = PackedBank(model, release_weights=release_weights, codes=codes, fused_linear=fused_linear, keep_images=keep_images,
                      fused_rows=fused_rows, fused_bytes=fused_bytes, fused_byte_rows=fused_byte_rows, fused_gemm_rows=fused_gemm_rows,
                      fused_byte_gemm_rows=fused_byte_gemm_rows, fused_conv1d=fused_conv1d)
    if not release_weights:
        with torch.no_grad():
            for e in bank.entries.values():
                e["mod"].weight.data.copy_(e["out"] if e["out"] is not None else bank._image(e))
    return bank
