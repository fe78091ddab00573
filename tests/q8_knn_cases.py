"""k-nearest-neighbour search over 8-bit descriptors (include/lf_mkd.h, lf_mkd_knn_q8_device): the numpy restatement the CPU
and GPU tests compare against, built on q8_cases."""
import numpy as np

import q8_cases as cases

INT32_MIN = cases.INT32_MIN
KS = (1, 2, 3, 4, 5, 8, 16)
# the matcher's shapes plus one candidate, fewer candidates than any k > 3, and a k between nb / 2 and nb
EXTRA_SHAPES = [(1, 1), (5, 3), (40, 17)]


def knn_q8(qa, qb, k, lo=None, hi=None):
    """(index, score) [na, k] int32: lf_mkd_knn_q8_device restated.  A stable ascending sort, reversed, is "score descending,
    index descending"; excluded rows are INT32_MIN, below every sum, and give index -1; nb < k is padded with -1 / INT32_MIN."""
    s = cases.similarities(qa, qb)
    if lo is not None:
        j = np.arange(s.shape[1], dtype=np.int64)[None, :]
        s = np.where((j >= np.asarray(lo, np.int64)[:, None]) & (j < np.asarray(hi, np.int64)[:, None]), INT32_MIN, s)
    order = np.argsort(s, axis=1, kind="stable")[:, ::-1][:, :k]
    score = np.take_along_axis(s, order, axis=1)
    index = np.where(score == INT32_MIN, -1, order)
    pad = k - index.shape[1]
    if pad > 0:
        index = np.concatenate([index, np.full((len(s), pad), -1)], axis=1)
        score = np.concatenate([score, np.full((len(s), pad), INT32_MIN)], axis=1)
    return np.ascontiguousarray(index, np.int32), np.ascontiguousarray(score, np.int32)


def knn_loops(qa, qb, k, lo=None, hi=None):
    """the same from the header's sentences, one pair at a time (tiny inputs only): the candidates of a row, ordered by larger
    s first and among equal s the higher index first; the first k of them; -1 / INT32_MIN beyond their number"""
    index, score = [], []
    for i in range(len(qa)):
        cand = []
        for j in range(len(qb)):
            if lo is not None and lo[i] <= j < hi[i]:
                continue
            cand.append((sum((int(x) - 128) * (int(y) - 128) for x, y in zip(qa[i], qb[j])), j))
        cand.sort(key=lambda c: (-c[0], -c[1]))
        cand = cand[:k] + [(int(INT32_MIN), -1)] * (k - min(k, len(cand)))
        index.append([c[1] for c in cand])
        score.append([c[0] for c in cand])
    return np.array(index, np.int32).reshape(len(qa), k), np.array(score, np.int32).reshape(len(qa), k)


def shape_cases():
    """q8_cases.shape_cases() and the extra shapes (seeds 3050 + position)"""
    return cases.shape_cases() + [(na, nb, 3050 + p) for p, (na, nb) in enumerate(EXTRA_SHAPES)]


def strictly_ordered(index, score):
    """every row descends strictly in (score, index) over its candidates, and the padding follows them"""
    key = score.astype(np.int64) * (1 << 32) + index.astype(np.int64)
    real = index >= 0
    ok = (key[:, :-1] > key[:, 1:]) | ~real[:, 1:]
    return bool(ok.all() and (real[:, :-1] | ~real[:, 1:]).all() and (score[~real] == INT32_MIN).all())
