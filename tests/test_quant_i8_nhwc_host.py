"""antq_quant_i8_nhwc without a GPU: its refusals in the order include/antq.h states (every one precedes the first HIP call and
the first read of the plan, so made-up pointers do), the option's row, the binding."""
import pytest

OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -5
X, Q, ALPHA, PLAN_HOST, PLAN_DEV, IMAGE = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def _call(antq_lib, x=X, q=Q, alpha=ALPHA, plan_host=PLAN_HOST, plan_dev=PLAN_DEV, image=IMAGE, shape=(2, 32, 49), flags=0, dtype=None):
    B, C, P = shape
    return antq_lib.lib().antq_quant_i8_nhwc(x, q, B, C, P, alpha, 1.0, plan_host, plan_dev, image, flags,
                                             antq_lib.F32 if dtype is None else dtype, None)


@pytest.mark.parametrize("kw, code", [
    (dict(x=None), ARG), (dict(q=None), ARG), (dict(alpha=None), ARG), (dict(plan_host=None), ARG), (dict(plan_dev=None), ARG),
    (dict(image=None), ARG), (dict(flags=2), ARG), (dict(dtype=77), ARG),
    (dict(flags=2, shape=(0, 32, 49)), ARG),                               # a bad flag comes before the empty call
    (dict(shape=(0, 24, 49), q=Q + 1), OK), (dict(shape=(2, 0, 49)), OK), (dict(shape=(2, 24, 0), flags=1), OK),   # empty: before any shape check
    (dict(flags=1), UNSUPPORTED), (dict(shape=(2, 24, 49)), UNSUPPORTED), (dict(shape=(2, 24, 49), q=Q + 1), UNSUPPORTED),
    (dict(shape=(1 << 11, 1 << 10, 1 << 10)), UNSUPPORTED), (dict(shape=(1 << 40, 1 << 40, 1 << 40)), UNSUPPORTED),
    (dict(q=Q + 8), ALIGN), (dict(x=X + 2), ALIGN), (dict(x=X + 1, dtype="bf16"), ALIGN), (dict(alpha=ALPHA + 2), ALIGN)])
def test_refusals_in_the_headers_order(antq_lib, kw, code):
    if kw.get("dtype") == "bf16":
        kw = dict(kw, dtype=antq_lib.BF16)
    assert _call(antq_lib, **kw) == code


def test_the_option_the_binding_and_the_abi(antq_lib):
    from ant_quantization_amd import packed
    with pytest.raises(antq_lib.AntqError, match="integer_conv_nchw needs integer_conv=True"):
        packed._check_options("pack_model", integer_conv_nchw=True, fused_linear=True, integer_linear=True)
    packed._check_options("pack_model", integer_conv_nchw=True, fused_linear=True, integer_linear=True, integer_conv=True)
    row = [o for o in packed._OPTIONS if o.name == "integer_conv_nchw"]
    assert len(row) == 1 and row[0].default is False and row[0].limits is None and "integer_conv" in row[0].needs
    assert callable(antq_lib.quant_i8_nhwc) and len(antq_lib.lib().antq_quant_i8_nhwc.argtypes) == 13
    assert antq_lib.ABI_VERSION == 7 and antq_lib.lib().antq_abi_version() == 7
    assert antq_lib.QUANT_I8_NHWC_MAX_BYTES == antq_lib.CONV2D4_I8_MAX_XQ_BYTES == 2 ** 31 - 1
