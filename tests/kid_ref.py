"""The restatement of `cleanfid.fid.kernel_distance` the KID tests compare against: numpy fp64, the subsets as explicit index lists, every
sum through `math.fsum` -- so an expectation carries only the round-off of the products and of the cube, not that of a summation order.

Tolerance (derived, and valid for ANY summation order of the code under test).  With u = 2^-53, a dot product of d non-negative terms is
within d u (relative) of the exact value; `/ d + 1` and the cube bring that to 3 (d + 3) u; a sum of m^2 positive terms in any order adds
m^2 u; the last fold over S subsets adds S u.  So each side is within gamma scale of the exact value, gamma = (3 (d + 3) + m^2 + S) u,
and two sides differ by at most 2 gamma scale, where scale_s = |A_s| / (m - 1) + 2 |B_s| / m is what the sums of subset s add up to."""
import functools
import math

import numpy as np

U = 2.0 ** -53
# (n1, n2, d, max_subset_size, num_subsets): one partial tile; exactly one tile with a true gather; full K with two ragged tiles and
# m = n2; three tiles (six tile pairs) at a width that is no power of two
CASES = [(5, 7, 64, 1000, 3), (130, 97, 128, 64, 4), (130, 97, 2048, 1000, 2), (200, 333, 192, 150, 5)]


def gamma(d: int, m: int, num_subsets: int) -> float:
    return (3 * (d + 3) + m * m + num_subsets) * U


def make_features(n1: int, n2: int, d: int, seed: int = 0):
    """non-negative, as the real ones are (means of a post-ReLU map): rows of seeded uniform [0, 1) times linspace(0.2, 2.0, d); the second
    set shifted by 0.05"""
    rng = np.random.RandomState(1000 + seed)
    w = np.linspace(0.2, 2.0, d)
    f1 = rng.random_sample((n1, d)) * w
    f2 = rng.random_sample((n2, d)) * w + 0.05
    return f1, f2


def make_subsets(n1: int, n2: int, m: int, num_subsets: int, seed: int = 0):
    """int32 (idx1 [S, m], idx2 [S, m]) from a private stream (the draw order is tested on its own)"""
    rng = np.random.RandomState(2000 + seed)
    idx2 = np.stack([rng.choice(n2, m, replace=False) for _ in range(num_subsets)]).astype(np.int32)
    idx1 = np.stack([rng.choice(n1, m, replace=False) for _ in range(num_subsets)]).astype(np.int32)
    return idx1, idx2


def kernel_distance(f1, f2, idx1, idx2):
    """(kid, per_subset [S], scale [S]): x = f2[idx2[s]] (the side the package draws first), y = f1[idx1[s]]"""
    f1, f2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    d = f1.shape[1]
    num_subsets, m = idx1.shape
    per, scale = [], []
    for s in range(num_subsets):
        x, y = f2[idx2[s]], f1[idx1[s]]
        xx, yy, xy = (x @ x.T / d + 1) ** 3, (y @ y.T / d + 1) ** 3, (x @ y.T / d + 1) ** 3
        off = ~np.eye(m, dtype=bool)
        a = math.fsum(xx[off].tolist() + yy[off].tolist())
        b = math.fsum(xy.ravel().tolist())
        per.append(math.fsum([a / (m - 1), -b * 2 / m]))
        scale.append(abs(a) / (m - 1) + 2 * abs(b) / m)
    return math.fsum(per) / num_subsets / m, np.array(per), np.array(scale)


@functools.lru_cache(maxsize=None)
def case(n1, n2, d, cap, num_subsets):
    """{f1, f2, idx1, idx2, m, kid, per, scale, gamma} of one of CASES, computed once and shared (treat as read-only)"""
    m = min(n1, n2, cap)
    f1, f2 = make_features(n1, n2, d, seed=d + n1)
    idx1, idx2 = make_subsets(n1, n2, m, num_subsets, seed=d + n2)
    kid, per, scale = kernel_distance(f1, f2, idx1, idx2)
    out = dict(f1=f1, f2=f2, idx1=idx1, idx2=idx2, m=m, kid=kid, per=per, scale=scale, gamma=gamma(d, m, num_subsets))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
