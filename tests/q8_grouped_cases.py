"""Grouped matching over 8-bit descriptors (include/lf_mkd.h, lf_mkd_match_q8_grouped_device, lf_mkd_vote_groups_device): the
numpy restatements the CPU and GPU tests compare against, built on q8_cases."""
import numpy as np

import q8_cases as cases

INT32_MIN = cases.INT32_MIN
RATIO = cases.RATIO
# the matcher's shapes plus one candidate, a handful, and a pool below one tile
EXTRA_SHAPES = [(1, 1), (5, 3), (40, 17)]
# sorted runs whose borders fall inside a lane's run of 4 rows, between the two lane halves, on a tile border and on the
# 128-row stage border
RUN_LENGTHS = (1, 3, 4, 5, 31, 32, 33, 95, 96)


def match_q8_grouped(qa, qb, groups, ratio=RATIO, lo=None, hi=None):
    """(match, best, rival), all int32: lf_mkd_match_q8_grouped_device restated.  A stable ascending sort, reversed, is
    "score descending, index descending"; excluded rows are INT32_MIN, below every sum; best is the first column, rival the
    score of the first column whose group differs from the first's (INT32_MIN: none); the acceptance is one f32
    multiplication."""
    return from_similarities(cases.similarities(qa, qb), groups, ratio, lo, hi)


def from_similarities(s, groups, ratio=RATIO, lo=None, hi=None):
    """match_q8_grouped on the int32 similarities [na, nb] themselves"""
    groups = np.asarray(groups, np.uint32)
    assert groups.shape == (s.shape[1],)
    if lo is not None:
        j = np.arange(s.shape[1], dtype=np.int64)[None, :]
        s = np.where((j >= np.asarray(lo, np.int64)[:, None]) & (j < np.asarray(hi, np.int64)[:, None]), INT32_MIN, s)
    order = np.argsort(s, axis=1, kind="stable")[:, ::-1]
    score = np.take_along_axis(s, order, axis=1)
    group = groups[order]
    rows = np.arange(len(s))
    best = score[:, 0]
    idx = np.where(best == INT32_MIN, -1, order[:, 0])
    other = (group != group[:, :1]) & (score != INT32_MIN)
    rival = np.where(other.any(axis=1), score[rows, np.argmax(other, axis=1)], INT32_MIN)
    ok = (idx >= 0) & ((np.float32(ratio) <= 0) | (best.astype(np.float32) * np.float32(ratio) > rival.astype(np.float32)))
    return np.where(ok, idx, -1).astype(np.int32), best.astype(np.int32), rival.astype(np.int32)


def grouped_loops(qa, qb, groups, ratio, lo=None, hi=None):
    """the same from the header's sentences, one pair at a time (tiny inputs only): the candidates of a row in the order
    "larger s first, among equal s the higher index first"; best is the first; rival the first of another group than its"""
    out = []
    for i in range(len(qa)):
        cand = []
        for j in range(len(qb)):
            if lo is not None and lo[i] <= j < hi[i]:
                continue
            cand.append((sum((int(x) - 128) * (int(y) - 128) for x, y in zip(qa[i], qb[j])), j))
        cand.sort(key=lambda c: (-c[0], -c[1]))
        if not cand:
            out.append((-1, int(INT32_MIN), int(INT32_MIN)))
            continue
        best, idx = cand[0]
        rival = next((s for s, j in cand if int(groups[j]) != int(groups[idx])), int(INT32_MIN))
        ok = ratio <= 0 or np.float32(best) * np.float32(ratio) > np.float32(rival)
        out.append((idx if ok else -1, best, rival))
    return tuple(np.array(c, np.int32) for c in zip(*out))


def from_knn(index, score, groups):
    """(best index, best, rival or None-mask) from a top-k table: rival is the score of the first column whose row has another
    group than column 0's; `known` says where such a column exists among the k"""
    groups = np.asarray(groups, np.uint32)
    g = np.where(index >= 0, groups[np.maximum(index, 0)].astype(np.int64), -1)
    other = (g != g[:, :1]) & (index >= 0)
    known = other.any(axis=1)
    rival = score[np.arange(len(index)), np.argmax(other, axis=1)]
    return index[:, 0], score[:, 0], rival, known


def vote_groups(match, groups_a, n_groups_a, groups_b, n_groups_b):
    """lf_mkd_vote_groups_device restated with np.add.at: votes [n_groups_a, n_groups_b] uint32"""
    match = np.asarray(match, np.int64)
    gb_all = np.asarray(groups_b, np.uint32).astype(np.int64)
    ga_all = np.zeros(len(match), np.int64) if groups_a is None else np.asarray(groups_a, np.uint32).astype(np.int64)
    votes = np.zeros((n_groups_a, n_groups_b), np.uint32)
    ok = (match >= 0) & (match < len(gb_all))
    ga, gb = ga_all[ok], gb_all[match[ok]]
    keep = (ga < n_groups_a) & (gb < n_groups_b)
    np.add.at(votes, (ga[keep], gb[keep]), 1)
    return votes


def shape_cases():
    """q8_cases.shape_cases() and the extra shapes (seeds 3050 + position, as q8_knn_cases)"""
    return cases.shape_cases() + [(na, nb, 3050 + p) for p, (na, nb) in enumerate(EXTRA_SHAPES)]


def runs(nb, length):
    """sorted runs of `length` rows"""
    return (np.arange(nb) // length).astype(np.uint32)


def group_layouts(nb, seed=0):
    """{name: groups [nb] uint32}: the layouts the GPU tests run"""
    rng = np.random.default_rng(4100 + seed)
    out = {f"runs of {n}": runs(nb, n) for n in RUN_LENGTHS}
    out["j % 3"] = (np.arange(nb) % 3).astype(np.uint32)
    out["permuted labels"] = rng.permutation(nb).astype(np.uint32)
    out["0 and 0xFFFFFFFF"] = np.where(rng.integers(0, 2, nb) == 1, 0xFFFFFFFF, 0).astype(np.uint32)
    out["random runs"] = np.cumsum(rng.integers(0, 2, nb)).astype(np.uint32) * np.uint32(2654435761)
    return out


def groups_for(nb, seed):
    """the groups of a shape case: random run lengths of 1 .. 9 rows, labels scattered over the uint32 range"""
    rng = np.random.default_rng(4000 + seed)
    labels = rng.permutation(nb + 1).astype(np.uint32) * np.uint32(2654435761)
    starts = np.zeros(nb, np.int64)
    pos = 0
    g = 0
    while pos < nb:
        n = int(rng.integers(1, 10))
        starts[pos:pos + n] = g
        pos += n
        g += 1
    return labels[starts]
