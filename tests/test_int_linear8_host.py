"""The byte-code integer linear on the host: grids.integer_image's limit keyword (I = 128 for ANT's signed int8 book, today's
answers under the default), Plan.integer_image8, and the integer_bytes option's place in the option table.  The launches:
tests/test_gpu_int_linear8.py."""
import numpy as np
import pytest


def test_the_int8_book_has_an_image_under_limit_128_only():
    from ant_quantization_amd import grids
    book = grids.ant_grid("int", 8, True)
    assert grids.integer_image(book) is None and grids.integer_image(book, limit=127) is None
    I, image = grids.integer_image(book, limit=128)
    assert I == 128 and image.dtype == np.int8 and np.array_equal(image, np.arange(-128, 128))
    assert grids.integer_image(grids.ant_grid("int", 8, False), limit=128) is None         # 255 levels
    assert grids.integer_image(np.array([-1.0, 0.0, 1.0]) * 3.0, limit=128)[0] == 1         # +128 never enters an image
    assert grids.integer_image(np.arange(-127, 129) / 128.0, limit=128) is None


@pytest.mark.parametrize("kind, bit, signed, want", [("int", 4, True, 8), ("int", 4, False, 15), ("flint", 4, True, None), ("pot", 4, True, None),
                                                     ("int", 6, True, 32), ("int", 7, False, 127), ("flint", 5, True, 64),
                                                     ("flint", 6, True, 0), ("pot", 5, True, 0)])
def test_books_with_an_image_keep_it_under_both_limits(antq_lib, kind, bit, signed, want):
    """want: the I (None: whatever it is; 0: no image under either limit)"""
    from ant_quantization_amd import grids
    book = grids.ant_grid(kind, bit, signed)
    a, b = grids.integer_image(book), grids.integer_image(book, limit=128)
    assert (a is None) == (b is None) == (want == 0)
    if a is not None:
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and (want is None or a[0] == want)
        plan = antq_lib.plan_for(book)
        assert plan.integer_image8()[0] == plan.integer_image()[0] and plan.integer_image8() is plan.integer_image8()


def test_integer_bytes_needs_its_prerequisites(antq_lib):
    from ant_quantization_amd import packed
    on = dict(fused_linear=True, fused_bytes=True, integer_linear=True)
    for missing in on:
        with pytest.raises(antq_lib.AntqError, match="%s needs %s=True" % ("fused_bytes" if missing == "fused_linear" else "integer_bytes", missing)):
            packed._check_options("pack_model", integer_bytes=True, **{k: v for k, v in on.items() if k != missing})
    packed._check_options("pack_model", integer_bytes=True, **on)
    assert callable(antq_lib.int_linear8) and callable(antq_lib.int_linear8_sk) and antq_lib.LINEAR8_I8_SK_MAX_M == 64
    assert len(antq_lib.lib().antq_linear8_i8.argtypes) == 18 and len(antq_lib.lib().antq_linear8_i8_sk.argtypes) == 20
