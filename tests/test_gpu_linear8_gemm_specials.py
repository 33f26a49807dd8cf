"""Non-finite weights, inputs and biases, the padded tail of K and the edges of the one rounding through antq_linear8_gemm on the
GPU: the loop of test_gpu_linear_specials.py over the cases linear8_gemm_special_cases.py registers for the new entry point
(which test_linear8_gemm_specials_host.py holds to their premises).  NaN is compared by class, everything else by bits, y sits
between guard words, and for the weight cases antq_decode8's own image is held to the numpy rule first."""
import pytest

import linear8_gemm_special_cases as gsc
import test_gpu_linear_specials as specials

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def knobs(antq_lib):
    """set(key, value): force a tile shape for the calling thread's later launches; the rule is restored afterwards"""
    knob = antq_lib.lib().antq_debug_set
    yield knob
    knob(23, 0)


@pytest.mark.parametrize("entry,dtype_name", gsc.SETS)
def test_special_values(antq_lib, dev, knobs, entry, dtype_name):
    specials.test_special_values(antq_lib, dev, knobs, entry, dtype_name)
