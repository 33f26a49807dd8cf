"""ANT `outlier` mode: the forward of AQ:438-465 restated in numpy float32 (one rounding per operation) and its inputs."""
import numpy as np

F = np.float32
STEP = F(2.0 ** -10)        # p16 = p4 + level * STEP: the int16 step is exactly STEP, so rint's ties can be planted exactly


def reference(x, p4, p16, grid, level, tail):
    p4, p16, grid = F(p4), F(p16), np.asarray(grid, F)
    with np.errstate(all="ignore"):
        a, body = np.abs(x), x.copy()
        if p4 > 0:
            s = p4 / grid.max()
            dist = np.abs((x / s)[:, None] - grid[None, :])
            dist[np.isnan(dist)] = np.inf
            j = grid.size - 1 - np.argmin(dist[:, ::-1], axis=1)          # antq_nearest: the LAST entry at the least distance,
            body = np.where(dist.min(axis=1) <= F(102400), grid[j], F(0)) * s     # 0 when none lies within 102400
        if not tail:
            return body
        step = (p16 - p4) / F(level)
        fine = (np.rint((a - p4) / step) * step + p4) * np.sign(x)
        return np.where(a > p4, (fine - body) + body, body)


def inputs(n, p4, s):
    """n values around p4 with the edge values planted across the first vector, a task boundary and the tail."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 1.2).astype(F)
    ties = [p4 + (F(k) + F(0.5)) * STEP for k in (0, 1, 2, 7, 40)]       # (a - p4) / STEP = k + 0.5, k even and odd
    sp = np.array([p4, -p4, np.nextafter(p4, F(np.inf)), 0.0, -0.0, np.nan, np.inf, -np.inf, 204800 * s, -204800 * s,
                   1e-40, -1e-42] + ties + [-t for t in ties[:2]], F)
    sp = np.roll(sp, n)
    for at in (0, 1017, n - sp.size):
        if 0 <= at < n:
            x[at:at + sp.size] = sp[:n - at]
    return x
