"""8-bit descriptors (include/lf_mkd.h, "8-bit descriptors"): the numpy restatements of the quantiser and of the exact int8
matcher, and the inputs the CPU and GPU tests share."""
import numpy as np

import match_pairs_cases as pcases

INT32_MIN = np.int32(-2 ** 31)
SCALE = np.float32(256.0)
RATIO = np.float32(0.8)

# (na, nb) of the matcher cases, seed 3000 + position: one row, below / at / above a 32-row tile on either side, several
# tiles and LDS stages, more than one a block's worth of waves, nb beyond anything the f32 one-launch form takes
SHAPES = [(1, 2), (31, 33), (32, 32), (33, 65), (513, 1025), (2000, 2000), (300, 6000)]


def quantize(x, scale=SCALE):
    """byte = clamp(rint(x * scale), -127, 127) + 128: one f32 product, ties to even, NaN -> 0, +-inf saturate"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.asarray(x, np.float32) * np.float32(scale)
    assert p.dtype == np.float32
    q = np.where(np.isnan(p), np.float32(0), np.clip(np.rint(p), -127, 127))
    return (q.astype(np.int32) + 128).astype(np.uint8)


def saturated(x, scale=SCALE):
    """rows with an element the quantiser clamps (or a NaN): the error bound does not cover them"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.rint(np.asarray(x, np.float32) * np.float32(scale))
    return ~(np.abs(p) <= 127).all(axis=1)


def similarities(qa, qb):
    """s[i, j] = sum_k (a[i][k] - 128) (b[j][k] - 128) as int32.  (The product is formed in float64, where every partial sum
    -- an integer below 2^21 in magnitude -- is exact whatever the order: the BLAS path instead of numpy's integer loops.)"""
    s = (qa.astype(np.float64) - 128.0) @ (qb.astype(np.float64) - 128.0).T
    out = s.astype(np.int32)
    assert np.array_equal(out, s)
    return out


def match_q8(qa, qb, ratio=RATIO, lo=None, hi=None):
    """(match, best, second), all int32: lf_mkd_match_q8_device restated.  A stable ascending sort leaves the highest index
    last among equals; excluded rows are INT32_MIN, below every sum; the acceptance is one f32 multiplication."""
    s = similarities(qa, qb)
    if lo is not None:
        j = np.arange(s.shape[1], dtype=np.int64)[None, :]
        s = np.where((j >= np.asarray(lo, np.int64)[:, None]) & (j < np.asarray(hi, np.int64)[:, None]), INT32_MIN, s)
    order = np.argsort(s, axis=1, kind="stable")
    rows = np.arange(len(s))
    idx = order[:, -1]
    best, second = s[rows, idx], s[rows, order[:, -2]]
    idx = np.where(best == INT32_MIN, -1, idx)
    ok = (idx >= 0) & ((np.float32(ratio) <= 0) | (best.astype(np.float32) * np.float32(ratio) > second.astype(np.float32)))
    return np.where(ok, idx, -1).astype(np.int32), best.astype(np.int32), second.astype(np.int32)


def match_loops(qa, qb, ratio, lo=None, hi=None):
    """the same from the header's sentences, one pair at a time (tiny inputs only)"""
    out = []
    for i in range(len(qa)):
        best = second = int(INT32_MIN)
        idx = -1
        for j in range(len(qb)):
            if lo is not None and lo[i] <= j < hi[i]:
                continue
            s = sum((int(x) - 128) * (int(y) - 128) for x, y in zip(qa[i], qb[j]))
            if s >= best:
                best, second, idx = s, best, j
            elif s > second:
                second = s
        ok = idx >= 0 and (ratio <= 0 or np.float32(best) * np.float32(ratio) > np.float32(second))
        out.append((idx if ok else -1, best, second))
    return tuple(np.array(c, np.int32) for c in zip(*out))


def error_bound(l1_a, l1_b, scale=SCALE):
    """|s / scale^2 - <a, b>| <= (|a|_1 + |b|_1) / (2 scale) + 128 / (4 scale^2) for rows without a saturated element: with
    q = x scale + e, |e| <= 1/2,  q_a q_b / scale^2 - a b = (a e_b + b e_a) / scale + e_a e_b / scale^2 per element."""
    scale = float(scale)
    return (np.asarray(l1_a, np.float64) + np.asarray(l1_b, np.float64)) / (2 * scale) + 128 / (4 * scale * scale)


def quantized_sets(na, nb, seed, scale=SCALE):
    a, b = pcases.descriptor_sets(na, nb, seed)
    return quantize(a, scale), quantize(b, scale)


def shape_cases():
    return [(na, nb, 3000 + k) for k, (na, nb) in enumerate(SHAPES)]


def random_ranges(na, nb, seed):
    """exclusion ranges that start and end mid-tile; every eighth row excludes nothing (lo == hi)"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, nb, na)
    hi = np.minimum(lo + rng.integers(1, 100, na), nb)
    hi[::8] = lo[::8]
    return lo.astype(np.uint32), hi.astype(np.uint32)


def edge_values(scale=SCALE):
    """the quantiser's edges as one padded block of rows: ties (to even), the clamp, the largest golden magnitude's
    neighbourhood, +-1, +-inf, NaN, -0.0, a subnormal"""
    s = np.float32(scale)
    v = []
    for m in (0.5, 1.5, 2.5, 126.5, 127.5, 127.0, 127.49, 128.0):
        v += [np.float32(m) / s, -np.float32(m) / s]
    v += [0.496, -0.496, 0.476, -0.476, 1.0, -1.0, np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1e-40, 3e38, -3e38]
    x = np.zeros((2, 128), np.float32)
    x.reshape(-1)[:len(v)] = np.array(v, np.float32)
    x[1] = np.roll(x[0], 37)
    return x
