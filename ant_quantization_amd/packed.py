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
`<layer>.quant_weight.codes` (uint8, numel / 2 bytes for 4-bit codes, numel bytes for byte codes) for packed layers and
`<layer>.weight` only for skipped ones; `load_packed_state_dict(model, sd)` loads it into a freshly wrapped, uncalibrated
model without re-encoding and takes each layer's code width from the stored size (anything else raises AntqError naming the
layer).

The options.  All are off by default, and without one everything said before it is unchanged.  `_OPTIONS` below holds what each
needs switched on and its range (else AntqError naming the missing option); `_ROUTES` holds which kernel serves which call.
Measurements, and the reasons behind each verdict, are in the profile and the DESIGN.md section named, not here.

A call "qualifies" when it runs without gradients and its quantised input is a contiguous, 16-byte-aligned GPU tensor [..., K] of
the layer's dtype on its device (the bias alike).  A qualifying call of a fusable layer runs the first kernel of the layer's
route list whose row limit covers its rows and, for the matrix-core kernels, whose dtype is bfloat16 / float16.  Every other call
runs the layer's own product -- F.linear, a Conv1D's `addmm` -- on the decoded image, with today's bits.  Every kernel
computes y = x . W^T + bias with W bit for bit the image the decoder writes, products and sum in fp32 in the kernel's own fixed
order: the result is that of F.linear on the image up to the rounding of an fp32 sum, not its bits, and the same row of x has
different low bits from two kernels (each independent of the other rows).  Each kernel has its counter (`.fused_*_calls`).

`fused_linear=True`: 4-bit Linear layers (2-D weight, in_features = K, K % 8 == 0) are fusable; calls of at most
`_lib.LINEAR4_MAX_M` rows run `antq_linear4` (`.fused_calls`).  Wins against F.linear on the image at every shape up to 4 rows and
loses on wide layers at 5 ... 8 (profiles/packed_linear.md).

`keep_images=False` (needs fused_linear): fusable layers keep no decoded image.  A call no kernel serves decodes that one layer
into ONE scratch buffer owned by the bank -- sized to the largest such layer of either width per (device, dtype) -- and runs the
layer's own product on it.  The scratch is valid only until the next such layer's call on the same stream: nothing may keep a
reference to it (a captured graph is fine, a side stream or autograd through the input is not).  A call a kernel serves decodes
nothing and leaves the scratch alone.  With `release_weights=True` such a layer's `weight.data` becomes an empty tensor (the bank
remembers the shape): a deep copy of such a model has no weights to fall back on, and a forward with the layer's quantiser
disabled or re-calibrating raises AntqError ("its float weight is gone").  Layers that are not fusable behave as without the option.

`fused_rows=R` (needs fused_linear): bf16 / f16 calls of 9 .. R rows of the 4-bit layers run `antq_linear4_mm`, the product on the
matrix cores (`.fused_mm_calls`).  Beats the scratch decode up to 64 rows on every layer measured but one and the kept image up
to 16 ... 64 rows depending on the layer (profiles/packed_linear_mm.md).

`fused_gemm_rows=R` (needs fused_linear): bf16 / f16 calls of the 4-bit layers with more rows than the kernels above take -- more
than 8, or more than `fused_rows` when that is given -- and at most R rows run `antq_linear4_gemm`, a tiled matrix-core product
(`.fused_gemm_calls`).  Loses to F.linear on the image and to the scratch decode at every point measured; it buys the memory and
the free scratch buffer, and wants fused_rows=64 beside it (profiles/packed_linear4_gemm.md).

`byte_codes=True`: a layer the 4-bit codec refuses for its codebook (the 5- to 8-bit layers of `set_8_bit_layer_n/_l`, OliVe's
unsigned 16 + 15 values) or for its row length (4 mod 8, such as 20) and that the byte codec accepts -- at most 256 values, with
OliVe at most 255 normal and 255 outlier values, rows of a multiple of 4 elements -- is encoded with `antq_encode8`, one code per
byte, 255 the pair identifier: an entry with `width == 8`.  Layers the 4-bit codec accepts keep 4-bit codes.  What stays in
`.skipped`: rows that are no multiple of 4 (conv1: K = 147), `base` / `outlier` modes, float64, quantisers that are disabled or
not calibrated.  Byte-coded layers are decoded by `antq_decode8_batch`, one more launch per (device, dtype, pair rule) group
(`.launches` counts it).  Without `fused_bytes` such a layer is never fusable and always keeps its decoded image (also under
`keep_images=False`); `release_weights`, `nbytes()` and the gradient error work on it as on any image-keeping layer.  Removes
the per-forward weight launches of a mixed-precision model and shrinks its checkpoint (profiles/packed_bytes.md).

`fused_bytes=True` (needs fused_linear): byte-coded Linear layers (2-D weight, in_features = K, K % 8 == 0) are fusable; calls of
at most `_lib.LINEAR8_MAX_M` rows run `antq_linear8` (`.fused_byte_calls`).  A byte-coded layer's call qualifies only while its
codes are 8-byte aligned.  Other byte-coded layers (K = 20, conv layers) keep their image.  Beats the scratch decode everywhere, the kept image everywhere up to 2 rows, and loses
to it on most 16-bit shapes at 8 (profiles/packed_linear8.md).

`fused_byte_rows=R` (needs fused_linear and fused_bytes): bf16 / f16 calls of 9 .. R rows of the fusable byte-coded layers run
`antq_linear8_mm` (`.fused_byte_mm_calls`).  `fused_rows` means 4-bit entries only, because the break-even differs.  Worth
turning on against the scratch decode (R = 64; 32 for layers like [768, 3072]); against kept images only around 16 rows
(profiles/packed_linear8_mm.md).

`fused_byte_gemm_rows=R` (needs fused_linear and fused_bytes): `fused_gemm_rows` for the fusable byte-coded layers, which run
`antq_linear8_gemm` (`.fused_byte_gemm_calls`); `fused_gemm_rows` means 4-bit entries only.  A mixed-precision model packed
with both, `keep_images=False` and R at least its largest call needs no scratch decode at all.  Loses to both alternatives at
every point measured; it buys the memory, and wants fused_byte_rows=64 beside it (profiles/packed_linear8_gemm.md).

`fused_conv1d=True` (needs fused_linear) is for GPT-2, whose projections are HF `Conv1D` layers behind OliVe's `Conv1dQuantizer`:
weight [in, out] = [K, N], y = x @ W + b, one scale per INPUT feature k.  Such a layer is packed with or without the option, but
without it always keeps its image.  With it a 4-bit entry whose module is a Conv1dQuantizer with a 2-D weight, `w.shape[1] ==
nf` and `w.shape[0] % 8 == 0` is fusable with kind `conv1d`: calls of at most `_lib.LINEAR4_T_MAX_M` rows run `antq_linear4_t`
(`.fused_t_calls`), its sum order a function of K alone.  `fused_rows` and `fused_gemm_rows` mean Linear entries only and do not
apply (the matrix-core form of this layout is `fused_conv1d_mm`, below); byte-coded Conv1D entries keep their image.  Buys a GPT-2
the memory and, at one row, roughly the speed of the image; with kept images not worth turning on beyond one row
(profiles/packed_linear_t.md).

`fused_conv1d_mm=True` (needs fused_linear and fused_conv1d): bf16 / f16 calls of 9 .. `_lib.LINEAR4_T_MM_MAX_M` = 64 rows of
the fusable Conv1D entries run `antq_linear4_t_mm`, the same product on the matrix cores (`.fused_t_mm_calls`): batched decode,
speculative or chunked decode and short prompts then decode nothing into the scratch buffer.  Calls of at most 8 rows keep
`antq_linear4_t`, float32 calls and calls of more than 64 rows the layer's `addmm`.  A flag, not a rows option: the set of
rows options is pinned (tests/test_packed_routing_host.py).  Faster than the scratch decode + `addmm` at 98 of 128 points of 9 ... 64 rows (0.69 ... 1.84x) and than `addmm` on a kept image at
19 of 128 (0.45 ... 1.09x): turn it on with `keep_images=False`; with kept images it is not worth turning on (profiles/packed_linear_t_mm.md).

`fused_conv1d_gemm=True` (needs fused_linear and fused_conv1d): bf16 / f16 calls of the fusable Conv1D entries with more rows than
the kernels above take -- more than 8, or more than 64 when `fused_conv1d_mm` is on as well -- and at most
`_lib.LINEAR4_T_GEMM_MAX_M` = 4096 rows run `antq_linear4_t_gemm`, a tiled matrix-core product whose workgroups decode each
weight once into LDS for 128 or 256 rows of x (`.fused_t_gemm_calls`).  A GPT-2 packed with it and `keep_images=False` computes
its 1024-token forwards without a scratch decode.  A flag like `fused_conv1d_mm`, for the same reason.  What it costs against
the scratch decode + `addmm` and against a kept image is in profiles/packed_linear_t_gemm.md and DESIGN.md 5p.

`integer_linear=True` (needs fused_linear) is a DIFFERENT contract, not one more kernel for the image product.  Every 4-bit ANT /
OliVe codebook but two (OliVe flint4 with its outlier list, ANT's unsigned pot4) is a set of small integers times one scale
(`grids.integer_image`), so a layer's product is an exact int32 sum times `alpha_x / I_x * alpha_w[n] / I_w`.  A 4-bit Linear entry
whose weight book has such an image and whose K is a multiple of 32 is integer-fusable (others: `.integer_skipped`, with the
reason).  Its forward, float32 / bfloat16 / float16 alike and for any number of rows, hands the RAW input to
`bank.integer_linear_call` before `quant_input` runs: `antq_quant_i8` writes the input's int8 image -- the activation quantiser's
decisions exactly as today -- and `antq_linear4_i8` multiplies it with the codes on the int8 matrix cores and scales each output
once (`.int_linear_calls`; include/antq.h has the formula).  The result does not depend on tile shape, sum order, M, N or the run.
It is NOT the bits of the image product: in float32 the two agree to fp32 rounding; in bfloat16 / float16 the integer path does
not carry the image's rounding of every factor to 8 / 11 bits (2^-9 / 2^-12), so it is the more exact of the two and differs
from today's output by that much.  The call is served only when lookup() served the weight, the input quantiser is steady,
enabled, per tensor, in neither `base` nor `outlier` mode, its book has an integer image, `I_x * I_w * K < 2^31` and the call
qualifies; in every other case the forward proceeds exactly as without the option, same launches, same bits.  Conv1D entries,
byte codes and ViT's attention wrapper are out of scope.  Measurements and verdict: profiles/int_linear4.md, DESIGN.md 5q.

`integer_split_k=True` (needs fused_linear and integer_linear) sends the integer calls of at most `_lib.LINEAR4_I8_SK_MAX_M` = 64
rows -- token generation, batched and speculative decode -- to `antq_linear4_i8_sk`, which cuts K across workgroups
(`.int_linear_sk_calls`; they still count in `.int_linear_calls`).  The sum is an exact integer, so the bits are those of
`antq_linear4_i8`: the flag changes launches and time, never a result.  The partial sums go through ONE workspace per device
owned by the bank, grown on demand and, like the decode scratch, valid only until the next such call on the same stream.  A flag,
not a rows option, for the reason `fused_conv1d_mm` is one.  Calls of more rows run `antq_linear4_i8` as before.  Measurements:
profiles/int_linear4_sk.md, DESIGN.md 5r.

`integer_bytes=True` (needs fused_linear, fused_bytes and integer_linear) extends the integer contract to the byte-coded Linear
entries -- the 8-bit layers of ANT's mixed-precision recipe (`set_8_bit_layer_n` / `_l`): W8A8 on the int8 matrix cores.  Such an
entry is integer-fusable when it is fusable, K is a multiple of 32, its book is plain and has an int8 image with I up to 128
(`Plan.integer_image8`: ANT int 5 to 8 bit signed, 5 to 7 bit unsigned, signed flint5; not unsigned int8, whose 255 levels need
a row-sum correction, nor flint6 and wider, pot / float books of 5 bits or more, or OliVe's byte books); every other byte-coded
entry is listed in `.integer_skipped` with its reason, and so is one whose calibrated input quantiser has no such image.  Its
forward quantises the raw input with the input book's 128-limit image (an 8-bit signed `int` activation quantiser qualifies:
xq may hold -128) and runs `antq_linear8_i8` -- for ANT's signed int8 book the code is the weight plus 128, one XOR per four
weights in front of the MFMA; other books go through an LDS table -- or, with `integer_split_k` and at most 64 rows,
`antq_linear8_i8_sk` on the bank's workspace (`.int_linear_byte_calls`, `.int_linear_byte_sk_calls`; both also count in
`.int_linear_calls` / `.int_linear_sk_calls`).  With the option off every path takes today's launches and gives today's bits.
Measurements and verdict: profiles/int_linear8.md, DESIGN.md 5s.

`integer_conv=True` (needs fused_linear and integer_linear) carries the integer contract over to convolutions: conv2d as an implicit
GEMM from the 4-bit codes on the int8 matrix cores (`antq_conv2d4_i8`; include/antq.h has the formula -- int_linear4's with the sum
over the receptive field; zero padding is exact because the image of 0 is 0).  A 4-bit `Conv2dQuantizer` entry of the ant tree is
integer-conv-fusable when groups == 1, C = in_channels is a multiple of 32, its padding is a tuple of integers with
`padding_mode == "zeros"`, and its weight book is plain and has an integer image; every other conv entry is listed in
`.integer_skipped` with its reason (conv1 with C = 3, for one).  A fusable entry gets `conv_codes`: its codes re-ordered nibble-wise
from (c, r, s) to (r, s, c) per output channel, built with torch ops at pack time from fresh or loaded codes alike and not written
to checkpoints -- N K / 2 extra bytes per served layer; the decoded image stays, because every call that is not served needs it.
`Conv2dQuantizer.forward` hands the RAW input to `bank.integer_conv_call` before `quant_input` runs; the call is served under
integer_linear_call's conditions on the weight and the input quantiser, for a 4-D input, when `I_x * I_w * C R S < 2^31`
(`.int_conv_calls`).  The kernel reads NHWC: a channels-last-contiguous input is used as it is, any other is copied once with
`contiguous(memory_format=torch.channels_last)` (`.int_conv_relayouts`); the output has the logical shape [B, N, Ho, Wo] in
channels-last memory, so a chain of served layers pays no relayout after the first.  OliVe's wrapper, byte-coded conv layers and
groups are out of scope.  With the option off every launch and every bit is today's.  Measurements and verdict:
profiles/int_conv4.md, DESIGN.md 5t.

`integer_conv_split_k=True` (needs fused_linear, integer_linear and integer_conv) sends the served conv calls whose output has at
most `_lib.CONV2D4_I8_SK_MAX_M` = 1024 positions B Ho Wo -- single-image and small-batch inference, the 7 x 7 and 14 x 14 stages
-- to `antq_conv2d4_i8_sk`, which cuts K = R S C across workgroups as `antq_linear4_i8_sk` does (`.int_conv_sk_calls`; they still
count in `.int_conv_calls`).  The sum is an exact integer, so the bits are those of `antq_conv2d4_i8`: the flag changes launches
and time, never a result.  The partial sums go through the bank's one workspace per device, the one `integer_split_k` uses.  A
flag, not a rows option.  Larger outputs run `antq_conv2d4_i8` as before; with the flag off every launch and every bit is
today's, in banks that set `integer_split_k` too.  Measurements: profiles/int_conv4_sk.md, DESIGN.md 5u.

`integer_conv_nchw=True` (needs fused_linear, integer_linear and integer_conv) quantises a served conv call's input that is
`is_contiguous()` but not channels-last -- plain NCHW memory, element alignment suffices -- with `antq_quant_i8_nhwc`, which reads
along H W and writes the int8 NHWC image in one launch (`.int_conv_nchw_calls`; no `.int_conv_relayouts`).  The bytes are those of
the copy + `antq_quant_i8`, so nothing downstream changes, the split-K routing included.  Any other stride pattern keeps the copy,
and so does the one class the copy measured as fast or faster for: bfloat16 / float16 inputs of fewer than 2^16 elements with
H W % 8 != 0;
channels-last inputs keep `antq_quant_i8`; with the flag off every launch and every bit is today's.  DESIGN.md 5v.

`integer_conv_bytes=True` (needs fused_linear, fused_bytes, integer_linear, integer_bytes and integer_conv) serves the BYTE-coded
conv entries -- the conv layers ANT's mixed-precision recipe promotes to 8 bit -- with `antq_conv2d8_i8`: W8A8 on the int8 matrix
cores.  A byte-coded `Conv2dQuantizer` entry of the ant tree is integer-conv-fusable under integer_conv's conditions (groups,
C % 32, zero padding by integers, a plain book) when its book has `integer_image8()`; it gets `conv_codes` (the code bytes
permuted to [N, R, S, C]), `wsum` (int32 [N], the sums of `image[conv_codes]` per output channel, formed in int64 at pack time)
and `integer` = I_w; neither `conv_codes` nor `wsum` goes into checkpoints, and every other byte-coded conv entry is listed in
`.integer_skipped` with its reason.  The offset is chosen per call from the input book: `integer_image8()` gives x_offset = 0;
otherwise `Plan.offset_image()` -- an unsigned book with the integers 0 .. I, I <= 255, which is what a `Conv2dQuantizer`'s
8-bit input quantiser has -- gives x_offset = 128: the input is quantised to value - 128, the kernel pads with the byte 0x80 and
adds 128 wsum[n]; `256 * I_w * C R S < 2^31` must hold.  An input book with neither is not served.  The input layout is
integer_conv's; the routing is the measured one: a call with at most 1024 output rows takes `antq_conv2d8_i8_sk` on the bank's
workspace with or without `integer_conv_split_k` (it beat the tiled entry at every such point), larger ones `antq_conv2d8_i8`
(`.int_conv_byte_calls`, `.int_conv_byte_sk_calls`,
`.int_conv_offset_calls` for the calls that took x_offset = 128; all of them also count in `.int_conv_calls` /
`.int_conv_sk_calls`).  With the flag off every launch, every bit and every `.integer_skipped` text is today's.
Measurements and verdict: profiles/int_conv8.md, DESIGN.md 5w.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._model import load_ant_state_dict
from .weight_bank import _weight_layers

__all__ = ["PackedBank", "pack_model", "packed_state_dict", "load_packed_state_dict"]

CODES_KEY = "quant_weight.codes"

# Every option that depends on another, once, in the order they are checked.  default: also what "not given" means (a rows
# option: None).  needs: the options that have to be on.  limits: rows lie in (lo, hi], constants of _lib; None for a flag.
_Option = namedtuple("_Option", "name default needs limits")
_OPTIONS = (
    _Option("fused_conv1d", False, ("fused_linear",), None),
    _Option("fused_conv1d_mm", False, ("fused_linear", "fused_conv1d"), None),
    _Option("fused_conv1d_gemm", False, ("fused_linear", "fused_conv1d"), None),
    _Option("fused_bytes", False, ("fused_linear",), None),
    _Option("fused_byte_rows", None, ("fused_linear", "fused_bytes"), ("LINEAR8_MAX_M", "LINEAR8_MM_MAX_M")),
    _Option("fused_byte_gemm_rows", None, ("fused_linear", "fused_bytes"), ("LINEAR8_MM_MAX_M", "LINEAR8_GEMM_MAX_M")),
    _Option("keep_images", True, ("fused_linear",), None),
    _Option("fused_rows", None, ("fused_linear",), ("LINEAR4_MAX_M", "LINEAR4_MM_MAX_M")),
    _Option("fused_gemm_rows", None, ("fused_linear",), ("LINEAR4_MM_MAX_M", "LINEAR4_GEMM_MAX_M")),
    _Option("integer_linear", False, ("fused_linear",), None),
    _Option("integer_split_k", False, ("fused_linear", "integer_linear"), None),
    _Option("integer_bytes", False, ("fused_linear", "fused_bytes", "integer_linear"), None),
    _Option("integer_conv", False, ("fused_linear", "integer_linear"), None),
    _Option("integer_conv_split_k", False, ("fused_linear", "integer_linear", "integer_conv"), None),
    _Option("integer_conv_nchw", False, ("fused_linear", "integer_linear", "integer_conv"), None),
    _Option("integer_conv_bytes", False, ("fused_linear", "fused_bytes", "integer_linear", "integer_bytes", "integer_conv"), None),
)
_NOTES = {("PackedBank", "keep_images"): " (nothing else computes from the codes)"}

# The routing rule: a fusable entry's call of M rows runs the FIRST route of its (kind, code width) whose row limit is at least
# M and, if half_only, whose dtype is bfloat16 / float16 -- else the layer's own product on the image.  fn: the function of _lib;
# counter: the bank's attribute that counts its calls; limit: a constant of _lib, or an option of the bank (None: no such route);
# when: the flag of the bank that has to be on for the route to exist (None: always).
# The last key is no kind of entry: ("conv1d", "tiled") holds the routes a ("conv1d", 4) entry tries AFTER its own list while the
# bank's flag `fused_conv1d_gemm` is on (_TAILS: key -> (flag, key of the routes appended)).  Without the flag -- off, or absent
# from a bank built before it existed -- the list of ("conv1d", 4) is all there is, as before.
_Route = namedtuple("_Route", "fn counter limit half_only when", defaults=(None,))
_ROUTES = {
    ("linear", 4): (_Route("linear4", "fused_calls", "LINEAR4_MAX_M", False),
                    _Route("linear4_mm", "fused_mm_calls", "fused_rows", True),
                    _Route("linear4_gemm", "fused_gemm_calls", "fused_gemm_rows", True)),
    ("linear", 8): (_Route("linear8", "fused_byte_calls", "LINEAR8_MAX_M", False),
                    _Route("linear8_mm", "fused_byte_mm_calls", "fused_byte_rows", True),
                    _Route("linear8_gemm", "fused_byte_gemm_calls", "fused_byte_gemm_rows", True)),
    ("conv1d", 4): (_Route("linear4_t", "fused_t_calls", "LINEAR4_T_MAX_M", False),
                    _Route("linear4_t_mm", "fused_t_mm_calls", "LINEAR4_T_MM_MAX_M", True, "fused_conv1d_mm")),
    ("conv1d", "tiled"): (_Route("linear4_t_gemm", "fused_t_gemm_calls", "LINEAR4_T_GEMM_MAX_M", True),),
}
_TAILS = {("conv1d", 4): ("fused_conv1d_gemm", ("conv1d", "tiled"))}
_HALF = (torch.bfloat16, torch.float16)


def _check_options(who, **options):
    """Every given option of _OPTIONS has what it needs switched on and lies in its range, else AntqError; a keyword that is
    neither one of them nor fused_linear is a TypeError."""
    for name in options:
        if name != "fused_linear" and all(name != o.name for o in _OPTIONS):
            raise TypeError("%s() got an unexpected keyword argument %r" % (who, name))
    for o in _OPTIONS:
        v = options.get(o.name, o.default)
        if (v is None) if o.limits else (bool(v) == o.default):
            continue                       # not given
        for need in o.needs:
            if not options.get(need, False):
                raise _lib.AntqError("%s: %s needs %s=True" % (who, o.name + ("=False" if o.default else ""), need)
                                     + _NOTES.get((who, o.name), ""))
        if o.limits:
            lo, hi = (getattr(_lib, c) for c in o.limits)
            if not (isinstance(v, int) and not isinstance(v, bool) and lo < v <= hi):
                raise _lib.AntqError("%s: %s must be an integer in (%d, %d] (got %r)" % (who, o.name, lo, hi, v))


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
                 fused_conv1d=False, fused_conv1d_mm=False, fused_conv1d_gemm=False, integer_linear=False,
                 integer_split_k=False, integer_bytes=False, integer_conv=False, integer_conv_split_k=False,
                 integer_conv_nchw=False, integer_conv_bytes=False):
        """codes: {layer name: uint8 tensor} -- stored codes to attach instead of encoding the weights (load_packed_state_dict);
        a layer's code width is then the one its stored size says (numel / 2 bytes: 4-bit, numel bytes: byte codes).
        Every other parameter: see the module docstring."""
        given = dict(locals())     # (the options by name, for the table)
        _check_options("PackedBank", fused_linear=fused_linear, **{o.name: given[o.name] for o in _OPTIONS})
        for o in _OPTIONS:         # a flag as a bool, a rows option as None or an int
            v = given[o.name]
            setattr(self, o.name, (None if v is None else int(v)) if o.limits else bool(v))
        for routes in _ROUTES.values():
            for r in routes:
                setattr(self, r.counter, 0)      # forwards that route's kernel served
        self.model = model
        self.release_weights = bool(release_weights)
        self.byte_codes = bool(byte_codes)
        self.fused_linear = bool(fused_linear)
        self._scratch = {}         # (device, dtype) -> the one decode buffer of the layers without an image
        self.entries = {}          # id(quantiser) -> dict
        self.skipped = []          # (layer name, reason): layers that keep their float weight and per-layer launch
        self.integer_skipped = []  # (layer name, reason): 4-bit Linear entries integer_linear does not serve (integer_bytes: and byte-coded entries; integer_conv: and conv entries)
        self.int_linear_calls = 0  # forwards antq_quant_i8 + antq_linear4_i8 (or _sk) served
        self.int_linear_sk_calls = 0  # ... of them through antq_linear4_i8_sk (integer_split_k)
        self.int_linear_byte_calls = 0  # ... of int_linear_calls, those from byte codes: antq_linear8_i8 (or _sk) (integer_bytes)
        self.int_linear_byte_sk_calls = 0  # ... of them through antq_linear8_i8_sk
        self.int_conv_calls = 0    # forwards antq_quant_i8 + antq_conv2d4_i8 served (integer_conv)
        self.int_conv_sk_calls = 0  # ... of them through antq_conv2d4_i8_sk (integer_conv_split_k)
        self.int_conv_relayouts = 0  # ... of them whose input was copied to channels-last memory first
        self.int_conv_nchw_calls = 0  # ... of them whose contiguous NCHW input antq_quant_i8_nhwc quantised (integer_conv_nchw)
        self.int_conv_byte_calls = 0  # ... of int_conv_calls, those from byte codes: antq_conv2d8_i8 (or _sk) (integer_conv_bytes)
        self.int_conv_byte_sk_calls = 0  # ... of them through antq_conv2d8_i8_sk
        self.int_conv_offset_calls = 0  # ... of int_conv_byte_calls, those with an unsigned input image: x_offset = 128
        self._sk_workspace = {}    # device -> the one workspace of antq_linear4_i8_sk / antq_linear8_i8_sk / antq_conv2d4_i8_sk, grown on demand
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
                    if self.integer_conv and w.dim() == 4:       # (a conv layer that is not even packed: conv1, C = 3, K = 27)
                        self.integer_skipped.append((name, "C = %d is not a multiple of 32" % w.shape[1] if w.shape[1] % 32
                                                     else "not packed: %s" % reason))
                    continue
                per_row = bool(q.is_perchannel)
                rows, row_len = (w.shape[0], w.numel() // w.shape[0]) if per_row else (1, w.numel())
                plan, gmax, n_normal, ovp = _codebook(q)
                if codes is not None:
                    c = codes[name].to(w.device).contiguous()
                else:
                    with torch.no_grad():
                        alpha = q.alpha.detach().reshape(-1).to(torch.float32).contiguous()
                        enc = getattr(_lib, "encode%d" % width)
                        c = enc(w.detach(), alpha, plan, gmax, rows, row_len, per_row, n_normal=n_normal, ovp=ovp)
                # (byte codes: only with fused_bytes -- without it a byte-coded layer always keeps its image)
                fusable = ((width == 4 or self.fused_bytes) and self.fused_linear and w.dim() == 2
                           and getattr(mod, "in_features", None) == w.shape[1] and w.shape[1] % 8 == 0)
                kind = "linear"
                if (self.fused_conv1d and width == 4 and _is_conv1d(mod) and w.dim() == 2 and getattr(mod, "nf", None) == w.shape[1]
                        and w.shape[0] % 8 == 0):
                    fusable, kind = True, "conv1d"     # weight [K, N]: the codes' rows are k (antq_linear4_t)
                image = self.keep_images or not fusable
                integer = None             # (integer_linear) the weight book's I, when the entry is integer-fusable
                if self.integer_linear and width == 4 and kind == "linear" and fusable:
                    why = ("the weight's codebook has no integer image" if plan.integer_image() is None
                           else "K = %d is not a multiple of 32" % w.shape[1] if w.shape[1] % 32 else None)
                    if why is None:
                        integer = plan.integer_image()[0]
                    else:
                        self.integer_skipped.append((name, why))
                conv_codes = wsum = None   # (integer_conv) the codes in tap-major order, when the entry is integer-conv-fusable
                if self.integer_conv_bytes and width == 8 and w.dim() == 4:
                    # (integer_conv_bytes) a byte-coded conv entry: the bytes tap-major, and the sums of its image per channel
                    why = ("not a Conv2dQuantizer of the ant tree" if not _is_ant_conv2d(mod)
                           else self._conv_integer_refusal(mod, tuple(w.shape), plan, ovp, width, bytes_too=True))
                    if why is None:
                        integer = plan.integer_image8()[0]
                        conv_codes = _tap_major_bytes(c, tuple(w.shape))
                        wsum = _image_sums(conv_codes, plan.integer_image8()[1], w.shape[0])
                    else:
                        self.integer_skipped.append((name, why))
                elif self.integer_linear and self.integer_bytes and width == 8:
                    why = self._byte_integer_refusal(mod, w, plan, ovp, kind == "linear" and fusable)
                    if why is None:
                        integer = plan.integer_image8()[0]
                    else:
                        self.integer_skipped.append((name, why))
                if self.integer_conv and w.dim() == 4 and not (self.integer_bytes and width == 8):      # (those are listed above)
                    why = ("not a Conv2dQuantizer of the ant tree" if not _is_ant_conv2d(mod)
                           else self._conv_integer_refusal(mod, tuple(w.shape), plan, ovp, width))
                    if why is None:
                        integer, conv_codes = plan.integer_image()[0], _tap_major(c, tuple(w.shape))
                    else:
                        self.integer_skipped.append((name, why))
                self.entries[id(q)] = dict(name=name, q=q, mod=mod, rows=rows, row_len=row_len, per_row=per_row, codes=c, width=width, conv_codes=conv_codes, wsum=wsum,
                                           fusable=fusable, kind=kind, shape=tuple(w.shape), dtype=w.dtype, device=w.device, integer=integer,
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
    def _byte_integer_refusal(mod, w, plan, ovp, fusable):
        """(integer_bytes) Why a byte-coded entry is not integer-fusable (None: it is).  The input quantiser is looked at as
        well when it is calibrated already -- integer_linear_call asks again at every call."""
        if not fusable:
            return "not a fusable Linear layer"
        if w.shape[1] % 32:
            return "K = %d is not a multiple of 32" % w.shape[1]
        if ovp:
            return "a pair-rule byte book has no integer image"
        if plan.integer_image8() is None:
            return "the weight's codebook has no integer image"
        qi = getattr(mod, "quant_input", None)
        if qi is not None and getattr(qi, "_steady", False) and qi.mode not in ("base", "outlier"):
            plan_x, _, _, ovp_x = _codebook(qi)
            if ovp_x or plan_x.integer_image8() is None:
                return "the input's codebook has no integer image"
        return None

    @staticmethod
    def _conv_integer_refusal(mod, shape, plan, ovp, width, bytes_too=False):
        """(integer_conv) Why the entry of an ANT Conv2dQuantizer `mod` with weight [N, C, R, S] is not integer-conv-fusable
        (None: it is).  bytes_too (integer_conv_bytes): byte codes are allowed, and then the book needs integer_image8()."""
        if width != 4 and not (bytes_too and width == 8):
            return "byte codes"
        if mod.groups != 1:
            return "groups = %d" % mod.groups
        if shape[1] % 32:
            return "C = %d is not a multiple of 32" % shape[1]
        pad = mod.padding
        if (isinstance(pad, str) or getattr(mod, "padding_mode", "zeros") != "zeros"
                or not all(isinstance(p, int) and p >= 0 for p in (pad if isinstance(pad, (tuple, list)) else (pad,)))):
            return "padding %r (%s) is not zero padding by integers" % (pad, getattr(mod, "padding_mode", "zeros"))
        if ovp:
            return "a pair-rule book does not survive the tap-major order"
        if (plan.integer_image8() if width == 8 else plan.integer_image()) is None:
            return "the weight's codebook has no integer image"
        return None

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
        return (sum(e["codes"].numel() + (0 if e.get("conv_codes") is None else e["conv_codes"].numel()) for e in self.entries.values()),
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
                if e.get("conv_codes") is not None:
                    e["conv_codes"] = e["conv_codes"].to(w.device)
                e["dtype"], e["device"] = w.dtype, w.device
            plan, gmax, n_normal, ovp = _codebook(q)
            alpha = q.alpha.detach().reshape(-1)
            e["alpha32"] = None
            if alpha.dtype != torch.float32 or not alpha.is_contiguous() or alpha.device != w.device:
                # (a 16-bit model's alpha: the kernel reads a float32 copy, brought up to date in place at every refresh)
                alpha = e["alpha32"] = alpha.to(device=w.device, dtype=torch.float32).contiguous()
            e["alpha"] = alpha
            e["unit_stamp"] = None         # (integer_linear: the scales as antq_linear4_i8 takes them, formed at the first call)
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
        dec = getattr(_lib, "decode%d" % e["width"])
        dec(e["codes"], e["alpha"], plan, gmax, e["rows"], e["row_len"], e["per_row"], e["dtype"], n_normal=n_normal, ovp=ovp, out=buf)
        return buf.view(e["shape"])

    def _route(self, e, M):
        """The route (of _ROUTES) that serves a call of M rows of entry `e`, or None: the rule stated at the table.  Looks at
        the entry's kind, width and dtype and at the bank's options; touches no tensor."""
        key = (e["kind"], e["width"])
        routes = _ROUTES.get(key, ())
        flag, tail = _TAILS.get(key, (None, None))
        if flag is not None and getattr(self, flag, False):
            routes = routes + _ROUTES[tail]
        for r in routes:
            if r.when is not None and not getattr(self, r.when, False):      # (a route whose flag is off or absent does not exist)
                continue
            limit = getattr(_lib, r.limit) if r.limit.isupper() else getattr(self, r.limit)
            if limit is not None and M <= limit and (e["dtype"] in _HALF or not r.half_only):
                return r
        return None

    def _fits(self, e, input, bias, K):
        """Whether a call may run from the codes: a contiguous, 16-byte-aligned no-grad input [..., K], not empty, in the
        layer's dtype on its device, the bias (if any) alike.  (How many rows: the route's business.)"""
        return (input.is_cuda and input.dtype == e["dtype"] and input.device == e["device"] and input.dim() >= 1 and input.shape[-1] == K
                and input.numel() > 0 and input.is_contiguous() and input.data_ptr() % 16 == 0
                and not (torch.is_grad_enabled() and (input.requires_grad or (bias is not None and bias.requires_grad)))
                and (bias is None or (bias.dtype == input.dtype and bias.is_contiguous() and bias.device == input.device)))

    def integer_linear_call(self, mod, input, weight):
        """(integer_linear) The output of a LinearQuantizer from its RAW input and what quant_weight returned, in the integer
        domain: antq_quant_i8 of the input, then antq_linear4_i8 from the codes.  None -- and nothing touched, so that the
        forward goes on exactly as without the option -- unless lookup() served the weight (linear()'s own test; the mark is
        popped only when the call is served here), the entry is integer-fusable, the input quantiser is steady, enabled, per
        tensor with one alpha, in neither `base` nor `outlier` mode and its book has an integer image, I_x I_w K < 2^31 and
        the call qualifies (_fits; no gradient wanted through the input quantiser's alpha either)."""
        q, qi = mod.quant_weight, mod.quant_input
        e = self.entries.get(id(q))
        if e is None or e["integer"] is None:
            return None
        if e["out"] is None:
            served = e.get("served", False) and weight is mod.weight and q._steady and q.is_enable and q.is_enable_weight
        else:
            served = weight is e["out"]
        N, K = e["shape"]
        if not (served and self._input_serves(qi) and self._fits(e, input, mod.bias, K) and input.numel() // K <= _lib.LINEAR4_I8_MAX_M):
            return None
        plan_x, gmax_x, nn_x, ovp_x = _codebook(qi)
        wide = e["width"] == 8             # (integer_bytes) byte codes: images with I up to 128, plain books on both sides
        image_x = plan_x.integer_image8() if wide else plan_x.integer_image()
        if image_x is None or image_x[0] * e["integer"] * K >= 2 ** 31 or (wide and ovp_x):
            return None
        e.pop("served", None)
        plan_w, gmax_w, nn_w, ovp_w = _codebook(q)
        dev = e["device"]
        self._integer_units(e, qi, plan_w, gmax_w, plan_x, gmax_x)
        xq = _lib.quant_i8(input, e["alpha_x"], plan_x, gmax_x, 1, input.numel(), False, plan_x.image_dev(dev, 128 if wide else 127),
                           n_normal=nn_x, ovp=ovp_x)
        self.int_linear_calls += 1
        if wide:
            return self._integer_byte_call(e, mod, xq, plan_w, image_x[0], input.numel() // K)
        args = (e["codes"], xq, e["unit_w"], plan_w.image_dev(dev), e["integer"], e["unit_x"], image_x[0], N, K, e["per_row"], e["dtype"])
        kw = dict(bias=None if mod.bias is None else mod.bias.detach(), n_normal=nn_w, ovp=ovp_w)
        M = input.numel() // K
        if getattr(self, "integer_split_k", False) and M <= _lib.LINEAR4_I8_SK_MAX_M:
            # K split across workgroups: the same bits.  The bank's one workspace per device, like the decode scratch valid
            # until the next such call on the same stream
            need = _lib.int_linear4_sk_workspace_bytes(M, N, K, dev)
            ws = self._sk_workspace.get(dev)
            if ws is None or ws.numel() < need:
                ws = self._sk_workspace[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self.int_linear_sk_calls += 1
            return _lib.int_linear4_sk(*args, workspace=ws, **kw)
        return _lib.int_linear4(*args, **kw)

    @staticmethod
    def _input_serves(qi):
        """Whether an input quantiser is one the integer calls take: steady, enabled, per tensor with one alpha, in neither
        `base` nor `outlier` mode, nothing pending, no gradient wanted through its alpha."""
        if qi._steady and not qi._hm_fresh():
            # (buffers rebound since -- a deep copy, .to(): what the quantiser's own forward would re-read, _init_quant_para)
            qi._hm_get('bit')
            if qi._hm_get('has_inited_quant_para') == 0:
                return False
        return (qi._steady and qi._hm_fresh() and getattr(qi, "_pending", None) is None and qi.is_enable
                and qi.is_enable_activation and not qi.is_perchannel and qi.mode not in ("base", "outlier") and qi.alpha.numel() == 1
                and not (torch.is_grad_enabled() and qi.alpha.requires_grad))

    @staticmethod
    def _integer_units(e, qi, plan_w, gmax_w, plan_x, gmax_x):
        """The scales as the integer entries take them (e["unit_w"], e["unit_x"], e["alpha_x"]), formed again only when an alpha
        or the input's book changed."""
        dev = e["device"]
        stamp = (qi.alpha.data_ptr(), qi.alpha._version, qi.alpha.dtype, id(plan_x), gmax_x, e["alpha"].data_ptr(), e["alpha"]._version)
        if e["unit_stamp"] != stamp:
            with torch.no_grad():
                e["unit_w"] = _unit_alpha(e["alpha"], plan_w, gmax_w)
                e["unit_x"] = _unit_alpha(qi.alpha.to(dev), plan_x, gmax_x)
                e["alpha_x"] = qi.alpha.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
            e["unit_stamp"] = stamp

    def integer_conv_call(self, mod, input, weight):
        """(integer_conv) The output of a Conv2dQuantizer from its RAW input and what quant_weight returned, in the integer
        domain: antq_quant_i8 of the input in channels-last memory, then antq_conv2d4_i8 from the tap-major codes.  None -- and
        nothing touched -- unless lookup() served the weight, the entry is integer-conv-fusable, the input quantiser is one
        integer_linear_call takes and its book is plain with an integer image, I_x I_w C R S < 2^31, and the input is a 4-D
        no-grad GPU tensor [B, C, H, W] of the layer's dtype on its device whose sizes the library takes.  An input that is not
        channels-last contiguous is copied once (`.int_conv_relayouts`) -- or, with integer_conv_nchw and plain contiguous NCHW
        memory, quantised by antq_quant_i8_nhwc without a copy (`.int_conv_nchw_calls`).  Returns [B, N, Ho, Wo] in channels-last
        memory."""
        q, qi = mod.quant_weight, mod.quant_input
        e = self.entries.get(id(q))
        if e is None or e.get("conv_codes") is None or weight is not e["out"]:
            return None
        N, C, R, S = e["shape"]
        bias = mod.bias
        if not (self._input_serves(qi) and input.dim() == 4 and input.is_cuda and input.dtype == e["dtype"] and input.device == e["device"]
                and input.shape[1] == C and input.numel() > 0
                and not (torch.is_grad_enabled() and (input.requires_grad or (bias is not None and bias.requires_grad)))
                and (bias is None or (bias.dtype == input.dtype and bias.is_contiguous() and bias.device == input.device))):
            return None
        plan_x, gmax_x, nn_x, ovp_x = _codebook(qi)
        wide = e["width"] == 8             # (integer_conv_bytes) byte codes: images with I up to 128, or the input's offset image
        image_x, x_offset = (plan_x.integer_image8() if wide else plan_x.integer_image()), 0
        if wide and image_x is None:
            image_x, x_offset = plan_x.offset_image(), 128     # (an unsigned book 0 .. I, I <= 255: value - 128, 128 wsum added)
        if image_x is None or ovp_x or (256 if x_offset else image_x[0]) * e["integer"] * C * R * S >= 2 ** 31:
            return None
        image_key = "offset" if x_offset else 128 if wide else 127
        B, _, H, W = input.shape
        (sh, sw), (ph, pw), (dh, dw) = _lib._pair(mod.stride), _lib._pair(mod.padding), _lib._pair(mod.dilation)
        Ho, Wo = (H + 2 * ph - dh * (R - 1) - 1) // sh + 1, (W + 2 * pw - dw * (S - 1) - 1) // sw + 1
        if (Ho < 1 or Wo < 1 or max(H, W, R, S, sh, sw, ph, pw, dh, dw) > _lib.CONV2D4_I8_MAX_DIM or B * Ho * Wo > _lib.CONV2D4_I8_MAX_M
                or input.numel() > _lib.CONV2D4_I8_MAX_XQ_BYTES):
            return None
        last = input.is_contiguous(memory_format=torch.channels_last)
        if last and input.data_ptr() % 16:
            return None
        # (integer_conv_nchw) a contiguous NCHW input goes to the transposing quantiser: no copy, element alignment suffices
        # (measured, DESIGN 5v: 16-bit rows that are no whole 16-byte vectors take element loads, and below 2^16 elements the
        # copy is then as fast or 6 % faster: those keep it)
        nchw = (not last and getattr(self, "integer_conv_nchw", False) and input.is_contiguous() and C % 16 == 0
                and not (input.element_size() == 2 and (H * W) % 8 and input.numel() < 1 << 16))
        if not last and not nchw:
            input = input.contiguous(memory_format=torch.channels_last)
            self.int_conv_relayouts += 1
        plan_w, gmax_w, _, _ = _codebook(q)
        dev = e["device"]
        self._integer_units(e, qi, plan_w, gmax_w, plan_x, gmax_x)
        if nchw:
            xq = _lib.quant_i8_nhwc(input, e["alpha_x"], plan_x, gmax_x, plan_x.image_dev(dev, image_key))
            self.int_conv_nchw_calls += 1
        else:
            xq = _lib.quant_i8(input.permute(0, 2, 3, 1), e["alpha_x"], plan_x, gmax_x, 1, input.numel(), False,
                               plan_x.image_dev(dev, image_key))
        self.int_conv_calls += 1
        if wide:
            return self._integer_conv_byte_call(e, mod, xq, plan_w, image_x[0], x_offset, B * Ho * Wo)
        args = (e["conv_codes"], xq, e["unit_w"], plan_w.image_dev(dev), e["integer"], e["unit_x"], image_x[0], N, (R, S), (sh, sw), (ph, pw),
                (dh, dw), e["per_row"], e["dtype"])
        bias = None if bias is None else bias.detach()
        M = B * Ho * Wo
        if getattr(self, "integer_conv_split_k", False) and M <= _lib.CONV2D4_I8_SK_MAX_M:
            # K = R S C split across workgroups: the same bits, on the bank's one workspace per device (integer_linear_call)
            need = _lib.int_conv2d4_sk_workspace_bytes(M, N, C * R * S, dev)
            ws = self._sk_workspace.get(dev)
            if ws is None or ws.numel() < need:
                ws = self._sk_workspace[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self.int_conv_sk_calls += 1
            return _lib.int_conv2d4_sk(*args, bias=bias, workspace=ws)
        return _lib.int_conv2d4(*args, bias=bias)

    def _integer_conv_byte_call(self, e, mod, xq, plan_w, I_x, x_offset, M):
        """(integer_conv_bytes) integer_conv_call's product for a byte-coded entry: antq_conv2d8_i8, or its split-K form."""
        N, C, R, S = e["shape"]
        dev = e["device"]
        args = (e["conv_codes"], xq, e["unit_w"], plan_w.image_dev(dev, 128), plan_w.integer_image8()[1], e["integer"], e["unit_x"], I_x,
                N, (R, S), _lib._pair(mod.stride), _lib._pair(mod.padding), _lib._pair(mod.dilation), e["per_row"], e["dtype"])
        kw = dict(bias=None if mod.bias is None else mod.bias.detach(), x_offset=x_offset, wsum=e["wsum"] if x_offset else None)
        self.int_conv_byte_calls += 1
        self.int_conv_offset_calls += 1 if x_offset else 0
        # the measured rule (profiles/int_conv8.md): up to 1024 rows the split-K entry beat the tiled one at all 44 points, the
        # one-slice ones included, so byte-coded calls take it with or without integer_conv_split_k
        if M <= _lib.CONV2D8_I8_SK_MAX_M:
            need = _lib.int_conv2d8_sk_workspace_bytes(M, N, C * R * S, dev)
            ws = self._sk_workspace.get(dev)
            if ws is None or ws.numel() < need:
                ws = self._sk_workspace[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self.int_conv_sk_calls += 1
            self.int_conv_byte_sk_calls += 1
            return _lib.int_conv2d8_sk(*args, workspace=ws, **kw)
        return _lib.int_conv2d8(*args, **kw)

    def _integer_byte_call(self, e, mod, xq, plan_w, I_x, M):
        """(integer_bytes) integer_linear_call's product for a byte-coded entry: antq_linear8_i8, or its split-K form."""
        N, K = e["shape"]
        dev = e["device"]
        args = (e["codes"], xq, e["unit_w"], plan_w.image_dev(dev, 128), plan_w.integer_image8()[1], e["integer"], e["unit_x"], I_x,
                N, K, e["per_row"], e["dtype"])
        bias = None if mod.bias is None else mod.bias.detach()
        self.int_linear_byte_calls += 1
        if getattr(self, "integer_split_k", False) and M <= _lib.LINEAR8_I8_SK_MAX_M:
            need = _lib.int_linear8_sk_workspace_bytes(M, N, K, dev)
            ws = self._sk_workspace.get(dev)
            if ws is None or ws.numel() < need:
                ws = self._sk_workspace[dev] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self.int_linear_sk_calls += 1
            self.int_linear_byte_sk_calls += 1
            return _lib.int_linear8_sk(*args, bias=bias, workspace=ws)
        return _lib.int_linear8(*args, bias=bias)

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
        N, K = e["shape"] if e["kind"] == "linear" else e["shape"][::-1]      # (conv1d: weight [K, N])
        route = self._route(e, input.numel() // K)
        if (route is not None and self._fits(e, input, bias, K)
                and not (e["width"] == 8 and e["codes"].data_ptr() % 8)):      # (byte codes are read 8 bytes at a time)
            plan, gmax, n_normal, ovp = _codebook(e["q"])
            setattr(self, route.counter, getattr(self, route.counter) + 1)
            return getattr(_lib, route.fn)(e["codes"], input, e["alpha"], plan.grid_dev(e["device"]), gmax, N, K, e["per_row"],
                                           bias=None if bias is None else bias.detach(), n_normal=n_normal, ovp=ovp)
        if e["out"] is None:
            weight = self._image(e)
        return mod._conv_forward(input, weight) if conv else F.linear(input, weight, bias)


def _unit_alpha(alpha, plan, gmax):
    """alpha * max|grid| / gmax as float32, formed in float64 (one rounding): the alpha whose quotient by the book's I is the
    unit of the fake-quantised image, value = integer * alpha' / I.  gmax is max(grid) -- of the normal values for OliVe --
    and differs from max|grid| for ANT's signed int (-8 .. 7) and for every book with an outlier list."""
    r = float(np.max(np.abs(plan.grid.astype(np.float64)))) / float(gmax)
    a = alpha.detach().reshape(-1)
    return a.to(torch.float32).contiguous() if r == 1.0 else (a.to(torch.float64) * r).to(torch.float32).contiguous()


def _tap_major(codes, shape):
    """The 4-bit codes of a conv weight [N, C, R, S] (encode4's layout: element 2 i in the low nibble of byte i) re-ordered
    nibble-wise to [N, R, S, C], as antq_conv2d4_i8 reads them."""
    N, C, R, S = shape
    c = codes.reshape(-1)
    nib = torch.stack((c & 15, c >> 4), dim=1).reshape(N, C, R, S).permute(0, 2, 3, 1).reshape(-1, 2)
    return (nib[:, 0] | (nib[:, 1] << 4)).contiguous()


def _tap_major_bytes(codes, shape):
    """The byte codes of a conv weight [N, C, R, S] (encode8's layout: one byte per element) re-ordered to [N, R, S, C], as
    antq_conv2d8_i8 reads them."""
    N, C, R, S = shape
    return codes.reshape(N, C, R, S).permute(0, 2, 3, 1).contiguous().reshape(-1)


def _image_sums(conv_codes, image, N):
    """wsum of antq_conv2d8_i8: int32 [N], the sum of image[code] over each output channel's codes (a code past the image
    counts 0), formed in int64 on the codes' device."""
    table = torch.zeros(256, dtype=torch.int64)
    table[:len(image)] = torch.from_numpy(np.asarray(image, dtype=np.int64))
    return table.to(conv_codes.device)[conv_codes.reshape(N, -1).long()].sum(dim=1).to(torch.int32).contiguous()


def _is_ant_conv2d(mod):
    """Whether `mod` is the ant tree's Conv2dQuantizer (OliVe's wrapper is out of integer_conv's scope)."""
    from .ant.quant_modules import Conv2dQuantizer
    return isinstance(mod, Conv2dQuantizer)


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


def pack_model(model, release_weights=False, **options):
    """Encode every suitable calibrated weight of `model` as 4-bit codes and serve the layers from one batched decode
    (PackedBank).  Returns the bank; `.skipped` lists the layers that stay float, with reasons.
    options: fused_linear, keep_images, fused_rows, byte_codes, fused_bytes, fused_byte_rows, fused_gemm_rows,
    fused_byte_gemm_rows, fused_conv1d, fused_conv1d_mm, fused_conv1d_gemm, integer_linear, integer_split_k, integer_bytes, integer_conv, integer_conv_split_k, integer_conv_nchw, integer_conv_bytes -- PackedBank's keywords with its defaults; see the module docstring."""
    return PackedBank(model, release_weights, None, **options)     # (codes: not an option here -- given, it is a TypeError)


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


def load_packed_state_dict(model, sd, release_weights=True, **options):
    """Load a packed checkpoint into a freshly wrapped, uncalibrated model living on the GPU: the quantiser state is
    installed the way load_ant_state_dict + load_state_dict do (scales keep the dtype they were stored with), a PackedBank is attached from the stored codes without
    re-encoding (a layer's code width is the one its stored size says: numel / 2 bytes are 4-bit codes, numel bytes byte codes;
    any other size raises AntqError naming the layer), and the weights are materialised by the batched decode
    (release_weights=False: copied into the layers' own float weights instead of replacing them).
    options: fused_linear, keep_images, fused_rows, fused_bytes, fused_byte_rows, fused_gemm_rows, fused_byte_gemm_rows,
    fused_conv1d, fused_conv1d_mm, fused_conv1d_gemm, integer_linear, integer_split_k, integer_bytes, integer_conv, integer_conv_split_k, integer_conv_nchw, integer_conv_bytes, as in pack_model (no byte_codes: the code width comes from the stored size).  Returns the bank."""
    _check_options("load_packed_state_dict", **options)        # (before the model is touched)
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
    bank = PackedBank(model, release_weights=release_weights, codes=codes, **options)
    if not release_weights:
        with torch.no_grad():
            for e in bank.entries.values():
                e["mod"].weight.data.copy_(e["out"] if e["out"] is not None else bank._image(e))
    return bank
