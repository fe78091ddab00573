"""CPU tests of the k-nearest-neighbour search over 8-bit descriptors (include/lf_mkd.h, lf_mkd_knn_q8_device): the three
symbols exist and refuse bad arguments without a device, the launch plan keeps its invariants, the numpy restatement the GPU
tests compare against (tests/q8_knn_cases.py) is right about itself and agrees with the matcher's, and the example's decision
rule does what it says."""
import ctypes
import os
import sys

import numpy as np
import pytest

import q8_cases as cases
import q8_knn_cases as kcases
from conftest import ROOT

import local_features_python as lfp

NAMES = ("lf_mkd_knn_q8_device", "lf_mkd_knn_q8", "lf_mkd_knn_q8_plan")


def test_the_symbols_are_exported():
    L = lfp.load_library()
    for name in NAMES:
        assert name in lfp.SYMBOLS and hasattr(L, name), name
    assert hasattr(lfp.LocalFeatures, "knn_q8")
    for method in ("knn_q8", "knn_q8_device"):
        assert hasattr(lfp.MkdHandle, method), method
    assert lfp.KNN_MAX == 16 and callable(lfp.knn_q8_plan)
    assert "KNN_MAX" in lfp.__all__ and "knn_q8_plan" in lfp.__all__


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)   # never dereferenced: the arguments are refused first
    big = (1 << 31) - 1

    def refused(rc, who, what, kw):
        assert rc == -1, (who, kw)
        msg = L.lf_mkd_last_error(None)
        assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)

    def device_call(a=p, na=64, b=p, nb=64, lo=None, hi=None, k=4, index=p, score=p):
        return L.lf_mkd_knn_q8_device(None, a, na, b, nb, lo, hi, k, index, score, None)

    for kw, what in [({}, b"null handle"), ({"na": 0}, b"null handle"), ({"lo": p, "hi": p}, b"null handle"),
                     ({"score": None}, b"null handle"),                        # d_score may be NULL
                     ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"), ({"index": None}, b"null pointer"),
                     ({"lo": p}, b"go together"), ({"hi": p}, b"go together"),
                     ({"a": ctypes.c_void_p(72)}, b"aligned"), ({"b": ctypes.c_void_p(68)}, b"aligned"),
                     ({"k": 0}, b"k must be"), ({"k": lfp.KNN_MAX + 1}, b"k must be"), ({"k": 1 << 31}, b"k must be"),
                     ({"nb": 0}, b"one candidate"), ({"na": big + 1}, b"2^31"), ({"nb": 1 << 40}, b"2^31"),
                     ({"na": big, "nb": big}, b"null handle"),
                     ({"k": lfp.KNN_MAX, "nb": 1}, b"null handle"), ({"k": 1, "nb": 1}, b"null handle")]:
        refused(device_call(**kw), b"knn_q8_device", what, kw)

    def host_call(a=p, na=64, b=p, nb=64, k=4, index=p, score=p):
        return L.lf_mkd_knn_q8(None, a, na, b, nb, k, index, score)

    for kw, what in [({}, b"null handle"), ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"),
                     ({"index": None}, b"null pointer"), ({"score": None}, b"null handle"),
                     ({"a": ctypes.c_void_p(65)}, b"null handle"),             # host rows need no alignment
                     ({"k": 0}, b"k must be"), ({"k": 17}, b"k must be"), ({"nb": 0}, b"one candidate"),
                     ({"na": big + 1}, b"2^31"), ({"nb": big + 1}, b"2^31"), ({"k": lfp.KNN_MAX, "nb": 1}, b"null handle")]:
        refused(host_call(**kw), b"knn_q8", what, kw)

    # the plan
    for na, nb, k, what in ((5, 0, 4, b"one candidate"), (5, 5, 0, b"k must be"), (5, 5, 17, b"k must be"), (big + 1, 5, 4, b"2^31"),
                            (5, big + 1, 4, b"2^31")):
        refused(L.lf_mkd_knn_q8_plan(na, nb, k, 0, None, None, None), b"knn_q8_plan", what, (na, nb, k))
    assert L.lf_mkd_knn_q8_plan(big, big, lfp.KNN_MAX, 0, None, None, None) == 0      # the largest problem, no output wanted
    assert L.lf_mkd_knn_q8_plan(5, 1, lfp.KNN_MAX, 0, None, None, None) == 0          # one candidate is an answer here


SIZES = [(1, 1), (1, 2), (1, 128), (1, 129), (31, 33), (32, 32), (513, 1025), (1024, 2000), (1025, 129), (2000, 2000),
         (300, 6000), (10000, 10000), (65536, 65536), (1 << 20, 1 << 20), (1, 1 << 20), (1 << 20, 2), ((1 << 31) - 1, (1 << 31) - 1)]


@pytest.mark.parametrize("num_cus", [0, 256, 1, 304])
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_plan_invariants(k, num_cus):
    # rows per a block, from the plan itself: the largest na that is still one block
    rows = next(n for n in range(1, 1 << 16) if lfp.knn_q8_plan(n + 1, 2, k, num_cus)[0] >= 2)
    for na, nb in SIZES:
        a_blocks, splits, scratch = lfp.knn_q8_plan(na, nb, k, num_cus)
        b_tiles = (nb + 31) // 32
        assert a_blocks * rows >= na > (a_blocks - 1) * rows, (na, nb)
        assert 1 <= splits <= b_tiles, (na, nb, splits)
        assert a_blocks < (1 << 31) and splits < (1 << 16), (na, nb)          # a launchable grid
        assert (scratch == 0) == (splits == 1), (na, nb, splits, scratch)
        assert scratch == 0 or scratch >= splits * na * k * 8, (na, nb, splits, scratch)   # k 64-bit keys per (split, a row)
        assert (splits == 1) == (nb <= 128), (na, nb, splits)                 # a condition on nb alone
    assert lfp.knn_q8_plan(0, 5, k, num_cus) == (0, 1, 0)
    if num_cus == 0:
        assert [lfp.knn_q8_plan(na, nb, k, 0) for na, nb in SIZES] == [lfp.knn_q8_plan(na, nb, k, 256) for na, nb in SIZES]
    # the scratch is monotone in na: a handle warmed up on the largest a never allocates for a smaller one
    for nb in (1, 128, 129, 2000, 65536, 1 << 20):
        nas = sorted(set([1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5000, 65536, 1 << 18,
                          (1 << 18) + 1, 1 << 19, (1 << 19) + 1, 1 << 20, (1 << 21) + 5, (1 << 31) - 1]
                         + list(range(1, 1 << 20, 37 * 1024 + 1))))
        scratch = [lfp.knn_q8_plan(na, nb, k, num_cus)[2] for na in nas]
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


def test_the_restatement_against_loops():
    qa, qb, lo, hi = _tiny()
    for k in (1, 2, 3, 9, 16):                         # 16 > nb = 9: padded
        for ranges in ((None, None), (lo, hi)):
            got, want = kcases.knn_q8(qa, qb, k, *ranges), kcases.knn_loops(qa, qb, k, *ranges)
            for g, w in zip(got, want):
                assert g.dtype == np.int32 and g.shape == (7, k) and np.array_equal(g, w), (k, ranges[0] is None)
            assert kcases.strictly_ordered(*got)
    index, score = kcases.knn_q8(qa, qb, 3)
    assert index[3, 0] == 6 and index[3, 1] == 2 and score[3, 0] == score[3, 1]
    assert score[4, 0] == 128 * 127 * 127 == 2064512 and index[4, 0] == 0
    assert kcases.knn_q8(qa, qb, 9)[1][4, 8] == -2064512 and kcases.knn_q8(qa, qb, 9)[0][4, 8] == 8
    index, score = kcases.knn_q8(qa, qb, 3, lo, hi)
    assert index[1].tolist() == [8, -1, -1] and score[1, 0] > cases.INT32_MIN and (score[1, 1:] == cases.INT32_MIN).all()
    assert index[4].tolist() == [0, -1, -1]
    assert index[5].tolist() == [-1, -1, -1] and (score[5] == cases.INT32_MIN).all()         # none
    index, score = kcases.knn_q8(qa, qb, 16)
    assert (index[:, 9:] == -1).all() and (score[:, 9:] == cases.INT32_MIN).all() and (index[:, :9] >= 0).all()
    # one candidate in all
    index, score = kcases.knn_q8(qa, qb[:1], 2)
    assert index.tolist() == [[0, -1]] * 7 and (score[:, 1] == cases.INT32_MIN).all()


def test_the_restatement_against_the_matcher():
    """column 0 is the matcher's index and best at ratio 0, column 1's score its second; every row strictly ordered"""
    qa, qb, lo, hi = _tiny()
    for ranges in ((None, None), (lo, hi)):
        m, best, second = cases.match_q8(qa, qb, 0.0, *ranges)
        index, score = kcases.knn_q8(qa, qb, 2, *ranges)
        assert np.array_equal(index[:, 0], m) and np.array_equal(score[:, 0], best) and np.array_equal(score[:, 1], second)
    tied_rows = {}
    for na, nb, seed in cases.shape_cases():
        qa, qb = cases.quantized_sets(na, nb, seed)
        m, best, second = cases.match_q8(qa, qb, 0.0)
        index, score = kcases.knn_q8(qa, qb, 16)
        assert np.array_equal(index[:, 0], m) and np.array_equal(score[:, 0], best), (na, nb)
        assert np.array_equal(score[:, 1], second), (na, nb)
        assert kcases.strictly_ordered(index, score), (na, nb)
        assert ((index >= 0).sum(1) == min(nb, 16)).all()
        tied_rows[(na, nb)] = int(((score[:, :-1] == score[:, 1:]) & (index[:, 1:] >= 0)).any(1).sum())
    # the random sets hold naturally tied neighbouring scores among the 16 best
    print(f"[q8 knn] rows with tied neighbouring scores among the 16 best: {tied_rows}")
    assert tied_rows[(513, 1025)] > 0 and tied_rows[(2000, 2000)] > 0 and tied_rows[(300, 6000)] > 0, tied_rows


def _example():
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import find_image
    return find_image


def test_rank_images_on_a_hand_built_table():
    ex = _example()
    M = int(cases.INT32_MIN)
    offsets = [0, 10, 20, 30]                           # three images of ten rows
    index = np.array([[3, 5, 12, 25],                   # best in image 0, rival (image 1) at column 2: 1000 * 0.8 > 700, counts
                      [13, 14, 3, 4],                   # best in image 1, rival (image 0) at column 2: 1000 * 0.8 > 900 fails
                      [21, 29, 20, 22],                 # every neighbour in image 2: counts
                      [7, -1, -1, -1],                  # one candidate: counts
                      [15, 2, 16, 17],                  # rival at column 1, exactly at the threshold: 1000 * 0.8 > 800 fails
                      [-1, -1, -1, -1]], np.int32)      # no candidate: no vote
    score = np.array([[1000, 990, 700, 650],
                      [1000, 950, 900, 100],
                      [500, 499, 498, 497],
                      [-300, M, M, M],
                      [1000, 800, 700, 600],
                      [M, M, M, M]], np.int32)
    assert ex.rank_images(index, score, offsets, 0.8).tolist() == [2, 0, 1]
    assert ex.rank_images(index, score, offsets, 0.95).tolist() == [2, 2, 1]        # a laxer test lets rows 1 and 4 through
    assert ex.rank_images(index[:, :1], score[:, :1], offsets, 0.8).tolist() == [2, 2, 1]   # k = 1: no rival in sight
    # a negative best against a rival: -300 * 0.8 = -240 > -250 counts, > -200 does not
    assert ex.rank_images(np.array([[7, 12]]), np.array([[-300, -250]], np.int32), offsets, 0.8).tolist() == [1, 0, 0]
    assert ex.rank_images(np.array([[7, 12]]), np.array([[-300, -200]], np.int32), offsets, 0.8).tolist() == [0, 0, 0]
    assert ex.rank_images(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), offsets).tolist() == [0, 0, 0]
