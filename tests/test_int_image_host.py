"""The integer image of a codebook (grids.integer_image) and the integer_linear option's place in the option table."""
import numpy as np
import pytest

from ant_quantization_amd import _lib, grids, packed


def _olive(mode):
    return np.concatenate([grids.olive_grid(mode, 4, True), grids.olive_outliers(4, True)])


_POT = [1, 2, 4, 8, 16, 32, 64]
_FLINT = [1, 2, 3, 4, 6, 8, 16]
_OUTL = [12, 16, 24, 32, 48, 64, 96]
BOOKS = {        # name: (grid, I, integers in the grid's own order)
    "ant_int4_s": (grids.ant_grid("int", 4, True), 8, list(range(-8, 8))),
    "ant_flint4_s": (grids.ant_grid("flint", 4, True), 16, [-v for v in _FLINT[::-1]] + [0, 0] + _FLINT),
    "ant_pot4_s": (grids.ant_grid("pot", 4, True), 64, [-v for v in _POT[::-1]] + [0, 0] + _POT),
    "ant_float4_s": (grids.ant_grid("float", 4, True), 64, [-v for v in _POT[::-1]] + [0, 0] + _POT),
    "ant_int4_u": (grids.ant_grid("int", 4, False), 15, list(range(16))),
    "ant_flint4_u": (grids.ant_grid("flint", 4, False), 64, list(range(9)) + [10, 12, 14, 16, 24, 32, 64]),
    "olive_int4_s": (_olive("int"), 96, list(range(-7, 8)) + [-v for v in _OUTL[::-1]] + _OUTL),
}


@pytest.mark.parametrize("name", sorted(BOOKS))
def test_integer_image(name):
    grid, I, ints = BOOKS[name]
    got = grids.integer_image(grid)
    assert got is not None and got[0] == I and got[1].dtype == np.int8 and got[1].tolist() == ints
    g = grid.astype(np.float64)
    assert np.max(np.abs(g / np.max(np.abs(g)) - got[1].astype(np.float64) / I)) <= 4 * 2.0 ** -24


def test_no_integer_image():
    assert grids.integer_image(_olive("flint")) is None                 # needs 192
    assert grids.integer_image(grids.ant_grid("pot", 4, False)) is None   # needs 2^14
    assert grids.integer_image(np.array([0.0, np.inf], dtype=np.float32)) is None
    assert grids.integer_image(np.array([0.0, np.nan], dtype=np.float32)) is None


def test_option_needs_fused_linear():
    with pytest.raises(_lib.AntqError, match="integer_linear needs fused_linear=True"):
        packed._check_options("pack_model", integer_linear=True)
    packed._check_options("pack_model", fused_linear=True, integer_linear=True)
