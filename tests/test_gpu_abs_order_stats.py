"""antq_abs_order_stats: the k-th and (k + 1)-th smallest |x|, the maximum and the NaN count, exactly as a sort gives them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A = 0x3F9AB155                                   # 1.2085..., every digit of its pattern non-zero


def _data(kind, n, k):
    """uint32 patterns of the n values.  straddleD: ranks 0..k hold A, the others the value one step of digit D above
    it (D = 0: they differ in the top 11 bits only, D = 2: in the lowest bit), so ranks k and k + 1 sit in two bins."""
    rng = np.random.default_rng(n + k)
    if kind == "equal":
        u = np.full(n, A, np.uint32)
    elif kind.startswith("straddle"):
        u = np.where(np.arange(n) <= k, A, A + (1 << (20, 10, 0)[int(kind[-1])])).astype(np.uint32)
    else:                                        # mixed: a normal sample with NaNs, Inf, zeros and denormals planted
        x = rng.standard_normal(n).astype(np.float32)
        sp = np.array([np.nan, 0.0, -0.0, 1e-40, -1e-42, np.inf, np.nan, -np.inf], np.float32)
        at = rng.permutation(n)[:sp.size]
        x[at] = sp[:at.size]
        return x.view(np.uint32)
    return rng.permutation(u | (rng.integers(0, 2, n, dtype=np.uint32) << 31))      # (random signs)


@pytest.mark.parametrize("n", [1, 2, 3, 2047, 2048, 2049, 100003])
@pytest.mark.parametrize("kind", ["equal", "straddle0", "straddle1", "straddle2", "mixed"])
def test_order_stats_exact(antq_lib, kind, n):
    """Compared as bit patterns; the maximum is the sort's last entry that is not a NaN (the NaN count reports those)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for k in sorted({0, n // 2, max(n - 2, 0), n - 1}):
        u = _data(kind, n, k)
        srt = np.sort(np.abs(u.view(np.float32))).view(np.uint32)
        nans = int(np.isnan(u.view(np.float32)).sum())
        want = [srt[k], srt[min(k + 1, n - 1)], srt[n - 1 - nans] if nans < n else 0, np.float32(nans).view(np.uint32)]
        for off in (0, 1):                                                       # 16-byte aligned, base + 4 bytes
            xt = torch.zeros(n + 1, device="cuda:0")[off:off + n].copy_(torch.from_numpy(u.view(np.float32)))
            got = antq_lib.abs_order_stats(xt, k).cpu().numpy().view(np.uint32)
            again = antq_lib.abs_order_stats(xt, k).cpu().numpy().view(np.uint32)
            assert list(got) == [int(w) for w in want], (k, off)
            assert np.array_equal(got, again)

