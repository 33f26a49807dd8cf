"""The special-value cases of antq_linear8_gemm (tests/linear8_gemm_special_cases.py) held to what
test_linear_special_cases_host.py holds the other entry points' cases to, by that module's own checks: the finite parts exact
in any order, every class of result where it has meaning, every promised position planted in the load unit that padded lanes
repeat, and each restated mistake -- a tail that is not zeroed among them, (a), at every K with a tail on both code paths --
changing at least one compared element."""
import pytest

import linear8_gemm_special_cases as gsc
import linear_special_cases as sc
import test_linear_special_cases_host as host

SETS = pytest.mark.parametrize("entry,dtype_name", gsc.SETS)


def test_the_entry_is_registered_beside_the_others():
    e = sc.ENTRIES[gsc.ENTRY]
    assert gsc.ENTRY not in {s[0] for s in sc.SETS} and len(sc.SETS) == 12          # the existing parametrisation is as it was
    assert e["NK"] == sc.ENTRIES["linear4_gemm"]["NK"] and e["Ms"] == sc.ENTRIES["linear4_gemm"]["Ms"] and e["knob"] == 23
    paths = sc.paths(gsc.ENTRY)
    assert (144, True) in paths and (272, True) in paths and (136, False) in paths and (256, True) in paths and (256, False) in paths
    assert sc.has_tail(gsc.ENTRY, 144, True) and not sc.has_tail(gsc.ENTRY, 256, True) and sc.has_tail(gsc.ENTRY, 16, True)
    # the unit a padded lane repeats: 16 elements on the 16-byte path, 8 on the narrow one
    assert sc.last_unit(gsc.ENTRY, 144, True) == slice(128, 144) and sc.last_unit(gsc.ENTRY, 136, False) == slice(128, 136)


@SETS
def test_cases_are_exact_and_cover_what_they_claim(entry, dtype_name):
    host.test_cases_are_exact_and_cover_what_they_claim(entry, dtype_name)


@SETS
def test_every_class_of_result_occurs(entry, dtype_name):
    host.test_every_class_of_result_occurs(entry, dtype_name)


@SETS
def test_non_finite_rows_hold_their_plants(entry, dtype_name):
    host.test_non_finite_rows_hold_their_plants(entry, dtype_name)


@SETS
def test_restated_mistakes_show(entry, dtype_name):
    host.test_restated_mistakes_show(entry, dtype_name)
