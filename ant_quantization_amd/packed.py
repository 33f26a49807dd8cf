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
"""
from collections import namedtuple

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
    _Option("fused_bytes", False, ("fused_linear",), None),
    _Option("fused_byte_rows", None, ("fused_linear", "fused_bytes"), ("LINEAR8_MAX_M", "LINEAR8_MM_MAX_M")),
    _Option("fused_byte_gemm_rows", None, ("fused_linear", "fused_bytes"), ("LINEAR8_MM_MAX_M", "LINEAR8_GEMM_MAX_M")),
    _Option("keep_images", True, ("fused_linear",), None),
    _Option("fused_rows", None, ("fused_linear",), ("LINEAR4_MAX_M", "LINEAR4_MM_MAX_M")),
    _Option("fused_gemm_rows", None, ("fused_linear",), ("LINEAR4_MM_MAX_M", "LINEAR4_GEMM_MAX_M")),
)
_NOTES = {("PackedBank", "keep_images"): " (nothing else computes from the codes)"}

# The routing rule: a fusable entry's call of M rows runs the FIRST route of its (kind, code width) whose row limit is at least
# M and, if half_only, whose dtype is bfloat16 / float16 -- else the layer's own product on the image.  fn: the function of _lib;
# counter: the bank's attribute that counts its calls; limit: a constant of _lib, or an option of the bank (None: no such route);
# when: the flag of the bank that has to be on for the route to exist (None: always).
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
}
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
                 fused_conv1d=False, fused_conv1d_mm=False):
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
        dec = getattr(_lib, "decode%d" % e["width"])
        dec(e["codes"], e["alpha"], plan, gmax, e["rows"], e["row_len"], e["per_row"], e["dtype"], n_normal=n_normal, ovp=ovp, out=buf)
        return buf.view(e["shape"])

    def _route(self, e, M):
        """The route (of _ROUTES) that serves a call of M rows of entry `e`, or None: the rule stated at the table.  Looks at
        the entry's kind, width and dtype and at the bank's options; touches no tensor."""
        for r in _ROUTES.get((e["kind"], e["width"]), ()):
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
    fused_byte_gemm_rows, fused_conv1d, fused_conv1d_mm -- PackedBank's keywords with its defaults; see the module docstring."""
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
    fused_conv1d, fused_conv1d_mm, as in pack_model (no byte_codes: the code width comes from the stored size).  Returns the bank."""
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
