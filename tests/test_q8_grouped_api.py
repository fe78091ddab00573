"""CPU tests of grouped matching over 8-bit descriptors (include/lf_mkd.h, lf_mkd_match_q8_grouped_device,
lf_mkd_vote_groups_device): the four symbols exist and refuse bad arguments without a device, the launch plan keeps its
invariants, the numpy restatement the GPU tests compare against (tests/q8_grouped_cases.py) is right about itself and agrees
with the matcher's and the top-k search's, and the example's exact vote relates to its k = 8 rule as it says."""
import ctypes
import os
import sys

import numpy as np
import pytest

import q8_cases as cases
import q8_grouped_cases as gcases
import q8_knn_cases as kcases
from conftest import ROOT

import local_features_python as lfp

NAMES = ("lf_mkd_match_q8_grouped_device", "lf_mkd_match_q8_grouped", "lf_mkd_match_q8_grouped_plan", "lf_mkd_vote_groups_device")
M = int(cases.INT32_MIN)


def test_the_symbols_are_exported():
    L = lfp.load_library()
    for name in NAMES:
        assert name in lfp.SYMBOLS and hasattr(L, name), name
    for method in ("match_q8_grouped", "vote_groups"):
        assert hasattr(lfp.LocalFeatures, method), method
    for method in ("match_q8_grouped", "match_q8_grouped_device", "vote_groups_device"):
        assert hasattr(lfp.MkdHandle, method), method
    assert callable(lfp.match_q8_grouped_plan) and "match_q8_grouped_plan" in lfp.__all__


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)   # never dereferenced: the arguments are refused first
    big = (1 << 31) - 1

    def refused(rc, who, what, kw):
        assert rc == -1, (who, kw)
        msg = L.lf_mkd_last_error(None)
        assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)

    def device_call(a=p, na=64, b=p, nb=64, group=p, lo=None, hi=None, ratio=0.8, match=p, best=p, rival=p):
        return L.lf_mkd_match_q8_grouped_device(None, a, na, b, nb, group, lo, hi, ratio, match, best, rival, None)

    odd = ctypes.c_void_p(66)
    for kw, what in [({}, b"null handle"), ({"na": 0}, b"null handle"), ({"lo": p, "hi": p}, b"null handle"),
                     ({"best": None, "rival": None}, b"null handle"),          # d_best and d_rival may be NULL
                     ({"nb": 1}, b"null handle"),                              # one candidate is a question here
                     ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"), ({"group": None}, b"null pointer"),
                     ({"match": None}, b"null pointer"),
                     ({"lo": p}, b"go together"), ({"hi": p}, b"go together"),
                     ({"a": ctypes.c_void_p(72)}, b"16-byte aligned"), ({"b": ctypes.c_void_p(68)}, b"16-byte aligned"),
                     ({"group": odd}, b"4-byte aligned"), ({"match": odd}, b"4-byte aligned"), ({"best": odd}, b"4-byte aligned"),
                     ({"rival": odd}, b"4-byte aligned"), ({"lo": odd, "hi": p}, b"4-byte aligned"),
                     ({"lo": p, "hi": odd}, b"4-byte aligned"),
                     ({"nb": 0}, b"one candidate"), ({"na": big + 1}, b"2^31"), ({"nb": 1 << 40}, b"2^31"),
                     ({"na": big, "nb": big}, b"null handle")]:
        refused(device_call(**kw), b"match_q8_grouped_device", what, kw)

    def host_call(a=p, na=64, b=p, nb=64, group=p, ratio=0.8, match=p, best=p, rival=p):
        return L.lf_mkd_match_q8_grouped(None, a, na, b, nb, group, ratio, match, best, rival)

    for kw, what in [({}, b"null handle"), ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"),
                     ({"group": None}, b"null pointer"), ({"match": None}, b"null pointer"),
                     ({"best": None, "rival": None}, b"null handle"),
                     ({"a": ctypes.c_void_p(65), "group": odd}, b"null handle"),   # host arrays need no alignment
                     ({"nb": 0}, b"one candidate"), ({"nb": 1}, b"null handle"),
                     ({"na": big + 1}, b"2^31"), ({"nb": big + 1}, b"2^31")]:
        refused(host_call(**kw), b"match_q8_grouped", what, kw)

    # the plan
    for na, nb, what in ((5, 0, b"one candidate"), (big + 1, 5, b"2^31"), (5, big + 1, b"2^31")):
        refused(L.lf_mkd_match_q8_grouped_plan(na, nb, 0, None, None, None), b"match_q8_grouped_plan", what, (na, nb))
    assert L.lf_mkd_match_q8_grouped_plan(big, big, 0, None, None, None) == 0         # the largest problem, no output wanted
    assert L.lf_mkd_match_q8_grouped_plan(5, 1, 0, None, None, None) == 0             # one candidate is a question here

    def vote_call(match=p, na=64, ga=p, n_ga=3, gb=p, nb=64, n_gb=5, votes=p):
        return L.lf_mkd_vote_groups_device(None, match, na, ga, n_ga, gb, nb, n_gb, votes, None)

    for kw, what in [({}, b"null handle"), ({"ga": None}, b"null handle"), ({"na": 0, "match": None, "gb": None}, b"null handle"),
                     ({"n_ga": 1, "n_gb": 1}, b"null handle"), ({"n_ga": 1, "n_gb": big}, b"null handle"),
                     ({"match": None}, b"null pointer"), ({"gb": None}, b"null pointer"),
                     ({"votes": None}, b"null d_votes"), ({"votes": None, "na": 0}, b"null d_votes"),
                     ({"n_ga": 0}, b"group count"), ({"n_gb": 0}, b"group count"),
                     ({"n_ga": 1 << 16, "n_gb": 1 << 15}, b"2^31"), ({"n_ga": 0xFFFFFFFF, "n_gb": 0xFFFFFFFF}, b"2^31"),
                     ({"na": big + 1}, b"2^31"), ({"nb": big + 1}, b"2^31"),
                     ({"match": odd}, b"4-byte aligned"), ({"votes": odd}, b"4-byte aligned")]:
        refused(vote_call(**kw), b"vote_groups_device", what, kw)


SIZES = [(1, 1), (1, 2), (1, 128), (1, 129), (31, 33), (32, 32), (513, 1025), (1024, 2000), (1025, 129), (2000, 2000),
         (300, 6000), (2000, 200000), (10000, 10000), (65536, 65536), (1 << 20, 1 << 20), (1, 1 << 20), (1 << 20, 2),
         ((1 << 31) - 1, (1 << 31) - 1)]


@pytest.mark.parametrize("num_cus", [0, 256, 1, 304])
def test_plan_invariants(num_cus):
    # rows per a block, from the plan itself: the largest na that is still one block
    rows = next(n for n in range(1, 1 << 16) if lfp.match_q8_grouped_plan(n + 1, 2, num_cus)[0] >= 2)
    for na, nb in SIZES:
        a_blocks, splits, scratch = lfp.match_q8_grouped_plan(na, nb, num_cus)
        b_tiles = (nb + 31) // 32
        assert a_blocks * rows >= na > (a_blocks - 1) * rows, (na, nb)
        assert 1 <= splits <= b_tiles, (na, nb, splits)
        per = -(-b_tiles // splits)
        assert (splits - 1) * per < b_tiles, (na, nb, splits)                  # no empty split
        assert a_blocks < (1 << 31) and splits < (1 << 16), (na, nb)          # a launchable grid
        assert (scratch == 0) == (splits == 1), (na, nb, splits, scratch)
        assert scratch == 0 or scratch >= splits * na * 16, (na, nb, splits, scratch)   # one 16-byte state per (split, a row)
        assert (splits == 1) == (nb <= 128), (na, nb, splits)                 # a condition on nb alone
    assert lfp.match_q8_grouped_plan(0, 5, num_cus) == (0, 1, 0)
    if num_cus == 0:
        assert [lfp.match_q8_grouped_plan(na, nb, 0) for na, nb in SIZES] == [lfp.match_q8_grouped_plan(na, nb, 256) for na, nb in SIZES]
    # the scratch is monotone in na: a handle warmed up on the largest a never allocates for a smaller one
    for nb in (1, 128, 129, 2000, 65536, 1 << 20):
        nas = sorted(set([1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5000, 65536, 1 << 18,
                          (1 << 18) + 1, 1 << 19, (1 << 19) + 1, 1 << 20, (1 << 21) + 5, (1 << 31) - 1]
                         + list(range(1, 1 << 20, 37 * 1024 + 1))))
        scratch = [lfp.match_q8_grouped_plan(na, nb, num_cus)[2] for na in nas]
        assert all(x <= y for x, y in zip(scratch, scratch[1:])), (nb, num_cus)


def _tiny():
    rng = np.random.default_rng(11)
    qa = rng.integers(1, 256, (7, 128)).astype(np.uint8)
    qb = rng.integers(1, 256, (9, 128)).astype(np.uint8)
    qb[6] = qb[2]                      # a duplicated b row ...
    qa[3] = qb[2]                      # ... that is row 3's best: equal scores, the higher index first
    qa[4] = 255                        # the extreme sums, both signs
    qb[0], qb[8] = 255, 1
    lo = np.array([0, 0, 3, 0, 1, 0, 4], np.uint32)
    hi = np.array([0, 8, 5, 0, 9, 9, 4], np.uint32)   # row 1: one candidate left (b row 8); row 4: one (row 0); row 5: none
    return qa, qb, lo, hi


TINY_GROUPS = {"two copies in one group": [0, 0, 7, 1, 1, 2, 7, 2, 0xFFFFFFFF],
               "two copies in two groups": [0, 0, 7, 1, 1, 2, 8, 2, 0xFFFFFFFF],
               "one group": [5] * 9, "index": list(range(9)), "j % 3": [j % 3 for j in range(9)]}


def test_the_restatement_against_loops():
    qa, qb, lo, hi = _tiny()
    for name, groups in TINY_GROUPS.items():
        groups = np.array(groups, np.uint32)
        for ratio in (0.0, 0.8, 1.0):
            for ranges in ((None, None), (lo, hi)):
                got = gcases.match_q8_grouped(qa, qb, groups, ratio, *ranges)
                want = gcases.grouped_loops(qa, qb, groups, ratio, *ranges)
                for g, w in zip(got, want):
                    assert g.dtype == np.int32 and g.shape == (7,) and np.array_equal(g, w), (name, ratio, ranges[0] is None)
    # it is a stable argsort of the product, then the first column of another group
    m, best, rival = gcases.match_q8_grouped(qa, qb, TINY_GROUPS["two copies in one group"], 0.8)
    assert best[3] == cases.similarities(qa[3:4], qb[6:7])[0, 0] and rival[3] < best[3]
    assert gcases.match_q8_grouped(qa, qb, TINY_GROUPS["two copies in one group"], 0.0)[0][3] == 6
    m, best, rival = gcases.match_q8_grouped(qa, qb, TINY_GROUPS["two copies in two groups"], 0.8)
    assert rival[3] == best[3] and m[3] == -1                               # the copy in another group IS the rival: rejected
    assert best[4] == 2064512 and gcases.match_q8_grouped(qa, qb, TINY_GROUPS["index"], 0.0)[0][4] == 0
    m, best, rival = gcases.match_q8_grouped(qa, qb, TINY_GROUPS["index"], 0.8, lo, hi)
    assert m[1] == 8 and rival[1] == M and best[1] > M                      # one candidate: accepted, no rival
    assert m[4] == 0 and rival[4] == M
    assert m[5] == -1 and best[5] == M and rival[5] == M                    # none
    m, best, rival = gcases.match_q8_grouped(qa, qb[:1], [3], 0.8)          # one candidate in all
    assert m.tolist() == [0] * 7 and (rival == M).all()


def test_consequence_a_group_is_index():
    """with group = index every output equals the matcher's, rival == second"""
    qa, qb, lo, hi = _tiny()
    for ratio in (0.0, 0.8):
        for ranges in ((None, None), (lo, hi)):
            assert all(np.array_equal(g, w) for g, w in zip(gcases.match_q8_grouped(qa, qb, np.arange(9), ratio, *ranges),
                                                           cases.match_q8(qa, qb, ratio, *ranges)))
    for na, nb, seed in cases.shape_cases():
        qa, qb = cases.quantized_sets(na, nb, seed)
        got, want = gcases.match_q8_grouped(qa, qb, np.arange(nb), cases.RATIO), cases.match_q8(qa, qb, cases.RATIO)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (na, nb)
        # (b) one group: no rival, every row accepted at any ratio
        m, best, rival = gcases.match_q8_grouped(qa, qb, np.full(nb, 9), 1.0)
        assert (rival == M).all() and np.array_equal(m, cases.match_q8(qa, qb, 0.0)[0]) and (m >= 0).all()


def test_consequence_c_the_top_k_table():
    """best / match at ratio 0 are column 0; rival is the first column of another group wherever one is among the k"""
    some_unknown = 0
    for na, nb, seed in gcases.shape_cases():
        qa, qb = cases.quantized_sets(na, nb, seed)
        index, score = kcases.knn_q8(qa, qb, 16)
        for groups in (gcases.groups_for(nb, seed), gcases.runs(nb, 40)):
            m, best, rival = gcases.match_q8_grouped(qa, qb, groups, 0.0)
            i0, b0, r, known = gcases.from_knn(index, score, groups)
            assert np.array_equal(m, i0) and np.array_equal(best, b0), (na, nb)
            assert np.array_equal(rival[known], r[known]), (na, nb)
            assert (rival[~known] <= score[~known, -1]).all()               # otherwise it lies behind the k-th neighbour
            some_unknown += int((~known).sum())
    assert some_unknown > 0                                                  # (runs of 40 hide some rivals from k = 16)


def _example():
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import find_image
    return find_image


def test_rank_images_exact_against_the_k8_rule():
    """the exact vote of every image is at most the k = 8 rule's, and the two agree on the rows whose rival lies within
    their 8 neighbours"""
    ex = _example()
    assert ex.rank_images_exact([3, -1, 12, 25, 30, 7], np.repeat([0, 1, 2], 10), 3).tolist() == [2, 1, 1]   # 30: out of range
    assert ex.rank_images_exact([3, 12, 25], np.repeat([0, 1, 2], 10), 2).tolist() == [1, 1]                 # image 2: not counted
    assert ex.rank_images_exact(np.zeros(0, np.int32), np.repeat([0, 1], 5), 2).tolist() == [0, 0]
    for na, nb, seed, run in ((513, 1025, 3004, 5), (300, 6000, 3006, 40), (2000, 2000, 3005, 400)):
        qa, qb = cases.quantized_sets(na, nb, seed)
        groups = gcases.runs(nb, run)                                        # a pool sorted by image
        n_images = int(groups[-1]) + 1
        offsets = np.minimum(np.arange(n_images + 1) * run, nb)
        index, score = kcases.knn_q8(qa, qb, ex.K)
        # (a laxer ratio than the example's: on random rows 0.8 accepts next to nothing)
        for ratio in (ex.RATIO, 0.97, 1.0):
            match, _, _ = gcases.match_q8_grouped(qa, qb, groups, ratio)
            exact = ex.rank_images_exact(match, groups, n_images)
            approx = ex.rank_images(index, score, offsets, ratio)
            assert exact.shape == approx.shape and (exact <= approx).all(), (na, nb, ratio)
            known = gcases.from_knn(index, score, groups)[3]
            assert np.array_equal(ex.rank_images_exact(match[known], groups, n_images),
                                  ex.rank_images(index[known], score[known], offsets, ratio)), (na, nb, ratio)
    # more than k near-duplicates of the match in one image: image 1 holds every row nine times, image 0 once, so the 8
    # neighbours all lie in image 1, the k = 8 rule sees no rival and counts every vote; the exact rule meets rival == best
    qa, b0 = cases.quantized_sets(100, 50, 3007)
    qb, groups = np.concatenate([b0] * 10), np.repeat([0, 1], [50, 450]).astype(np.uint32)
    index, score = kcases.knn_q8(qa, qb, ex.K)
    match, best, rival = gcases.match_q8_grouped(qa, qb, groups, ex.RATIO)
    assert not gcases.from_knn(index, score, groups)[3].any() and (rival == best).all() and (best > 0).all()
    assert ex.rank_images(index, score, [0, 50, 500], ex.RATIO).tolist() == [0, 100]
    assert ex.rank_images_exact(match, groups, 2).tolist() == [0, 0]
