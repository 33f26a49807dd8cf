"""The integer-domain conv2d on the host: the integer_conv option's place in the option table, the tap-major re-ordering of the
codes and the eligibility reasons.  The launches: tests/test_gpu_int_conv4.py."""
import types

import numpy as np
import pytest


def test_integer_conv_needs_its_prerequisites(antq_lib):
    from ant_quantization_amd import packed
    on = dict(fused_linear=True, integer_linear=True)
    with pytest.raises(antq_lib.AntqError, match="integer_conv needs integer_linear=True"):
        packed._check_options("pack_model", integer_conv=True, fused_linear=True)
    with pytest.raises(antq_lib.AntqError, match="needs fused_linear=True"):
        packed._check_options("pack_model", integer_conv=True, integer_linear=True)
    packed._check_options("pack_model", integer_conv=True, **on)
    assert callable(antq_lib.int_conv2d4) and len(antq_lib.lib().antq_conv2d4_i8.argtypes) == 27


def test_tap_major_codes_match_an_independent_restatement():
    import torch
    from ant_quantization_amd import packed
    N, C, R, S = 5, 32, 3, 2
    codes = np.random.default_rng(0).integers(0, 256, N * C * R * S // 2, dtype=np.uint8)
    nibble = lambda buf, e: (buf[e >> 1] >> (4 * (e & 1))) & 15           # element e of encode4's layout
    n, r, s, c = np.indices((N, R, S, C)).reshape(4, -1)
    moved = nibble(codes, ((n * C + c) * R + r) * S + s)                  # element (n, r, s, c), in that order, from [N, C, R, S]
    want = (moved[0::2] | (moved[1::2] << 4)).astype(np.uint8)
    got = packed._tap_major(torch.from_numpy(codes), (N, C, R, S))
    assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("what, reason", [("groups", "groups = 2"), ("c_48", "C = 48 is not a multiple of 32"), ("same", "padding 'same'"),
                                          ("olive", "pair-rule"), ("fine", None)])
def test_conv_eligibility_reasons(antq_lib, what, reason):
    from ant_quantization_amd import grids, packed
    mod = types.SimpleNamespace(groups=2 if what == "groups" else 1, padding="same" if what == "same" else (1, 1))
    olive = what == "olive"
    grid = np.concatenate([grids.olive_grid("int", 4, True), grids.olive_outliers(4, True)]) if olive else grids.ant_grid("flint", 4, True)
    why = packed.PackedBank._conv_integer_refusal(mod, (64, 48 if what == "c_48" else 64, 3, 3), antq_lib.plan_for(grid), olive, 4)
    assert (why is None) if reason is None else (reason in why)
