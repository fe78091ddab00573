"""CPU tests of feature tracks (include/lf_mkd.h, lf_mkd_build_tracks_device): the symbol exists and refuses bad arguments
without a device; the numpy restatement the GPU tests compare against (tests/tracks_cases.py) equals a brute-force transitive
closure, accumulates, and finds conflicting and long tracks on the edge matcher's decoy pool."""
import ctypes
import os
import re

import numpy as np

import match_pairs_cases as pcases
import q8_edges_cases as ecases
import tracks_cases as cases
from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
TILE = lfp.TRACKS_DUP_TILE


def test_the_symbol_is_exported():
    L = lfp.load_library()
    assert "lf_mkd_build_tracks_device" in lfp.SYMBOLS and hasattr(L, "lf_mkd_build_tracks_device")
    assert len(L.lf_mkd_build_tracks_device.argtypes) == 15                   # the header's arity
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    proto = re.search(r"int lf_mkd_build_tracks_device\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == 15
    assert hasattr(lfp.LocalFeatures, "build_tracks") and hasattr(lfp.MkdHandle, "build_tracks_device")
    # the constants are the header's
    assert int(re.search(r"#define LF_MKD_TRACKS_ACCUMULATE (\d+)u", header).group(1)) == lfp.TRACKS_ACCUMULATE == 1
    assert int(re.search(r"#define LF_MKD_TRACKS_DUP_TILE \((\d+)\)", header).group(1)) == lfp.TRACKS_DUP_TILE


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(io=p, n_images=3, total=64, ea=p, eb=p, la=p, cap=64, n_edges=5, match=p, flags=0, track=p, length=p, dup=p):
        return L.lf_mkd_build_tracks_device(None, io, n_images, total, ea, eb, la, cap, n_edges, match, flags, track, length, dup, None)

    for kw, what in [({}, b"null handle"), ({"flags": lfp.TRACKS_ACCUMULATE}, b"null handle"),
                     ({"length": None, "dup": None}, b"null handle"), ({"length": None}, b"null handle"), ({"dup": None}, b"null handle"),
                     ({"n_edges": 0, "ea": None, "eb": None, "la": None, "match": None}, b"null handle"),   # no edges: no edge arrays
                     ({"total": 0}, b"null handle"), ({"n_images": 0}, b"null handle"), ({"n_images": 0xFFFFFFFF, "dup": None}, b"null handle"),
                     ({"total": BIG, "cap": BIG, "n_edges": 1}, b"null handle"),
                     ({"io": None}, b"null pointer"), ({"track": None}, b"null pointer"), ({"io": None, "n_edges": 0}, b"null pointer"),
                     ({"ea": None}, b"null edge array"), ({"eb": None}, b"null edge array"), ({"la": None}, b"null layout array"),
                     ({"match": None}, b"null match array"),
                     ({"io": odd8}, b"8-byte aligned"), ({"la": odd8}, b"8-byte aligned"),
                     ({"ea": odd4}, b"4-byte aligned"), ({"eb": odd4}, b"4-byte aligned"), ({"match": odd4}, b"4-byte aligned"),
                     ({"track": odd4}, b"4-byte aligned"), ({"length": odd4}, b"4-byte aligned"), ({"dup": odd4}, b"4-byte aligned"),
                     ({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
                     ({"total": BIG + 1}, b"2^31 - 1"), ({"cap": BIG + 1}, b"2^31 - 1"), ({"total": 1 << 40}, b"2^31 - 1"),
                     # the link grid: floor(cap / 256) + n_edges; d_track_dup's: floor(total / tile) + n_images, only when it is given
                     ({"cap": BIG, "n_edges": 0xFFFFFFFF}, b"workgroups"),
                     ({"cap": BIG, "n_edges": BIG - BIG // 256}, b"null handle"),
                     ({"cap": BIG, "n_edges": BIG - BIG // 256 + 1}, b"workgroups"),
                     ({"total": BIG, "n_images": BIG - BIG // TILE}, b"null handle"),
                     ({"total": BIG, "n_images": BIG - BIG // TILE + 1}, b"workgroups"),
                     ({"total": BIG, "n_images": BIG - BIG // TILE + 1, "dup": None}, b"null handle")]:
        _refused(L, call(**kw), b"build_tracks_device", what, kw)


def test_the_restatement_equals_the_transitive_closure():
    """pools of up to 60 rows: labels against boolean matrix powers, len and dup against their definitions row by row"""
    merged = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        sizes = rng.integers(0, 9, rng.integers(2, 9))
        io = 3 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total = int(io[-1]) + int(rng.integers(-2, 3))                       # the total may cut the last image
        if seed % 5 == 4 and len(io) > 3:
            io[1] = io[2] + 1                                                # an inverted range
        assert total <= 60
        c = cases.random_case((io, total), int(rng.integers(5, 12)), seed, share=float(rng.choice([0.15, 0.5])),
                              layout_from_b=seed % 7 == 3)
        if seed % 3 == 2:
            c.cap = max(c.size - int(rng.integers(0, 6)), 0)                 # a capacity cut short
        track, length, dup = c.reference()
        u, v = c.links()
        assert np.array_equal(track, cases.closure(total, u, v)), seed
        assert (track <= np.arange(total)).all() and (track[track] == track).all()
        for t in range(total):
            rows = np.flatnonzero(track == t)
            assert length[t] == len(rows), (seed, t)
            want = 0
            for m in range(len(io) - 1):
                first, n = ecases.image_bounds(io, total, m)
                want += max(int(((rows >= first) & (rows < first + n)).sum()) - 1, 0)
            assert dup[t] == want, (seed, t)
        merged += int((length > 1).sum())
    assert merged > 50                                                       # tracks of more than one row, over all seeds


def test_links_are_read_as_the_header_says():
    io = np.array([2, 5, 5, 9], np.int64)                                    # images of 3, 0 and 4 rows behind 2 rows of no image
    c = cases.Case((io, 10), [(0, 2), (2, 0), (1, 2), (3, 0), (0, cases.NO_IMAGE)], [])
    assert c.la.tolist() == [0, 3, 7, 7, 7, 10]
    c.match[:] = [3, 4, -7, 0, cases.INT32_MAX, 3, 2, 1, 0, 2]                # edge 0: 3, (4 = nB), -7; edge 1: 0, MAX, (3 = nB), 2
    u, v = c.links()                                                         # edges 3 and 4 have an empty image: no link
    assert sorted(zip(u.tolist(), v.tolist())) == [(2, 8), (5, 2), (8, 4)]
    track, length, dup = c.reference()
    assert track.tolist() == [0, 1, 2, 3, 2, 2, 6, 7, 2, 9] and length[2] == 4 and dup[2] == 2 and dup.sum() == 2
    c.cap = 6                                                                # cut inside edge 1: its rows 3 .. 5 only
    assert sorted(zip(*[x.tolist() for x in c.links()])) == [(2, 8), (5, 2)]


def test_two_calls_equal_one():
    """the links split between two calls, the second accumulating onto the first's labels; and onto an array of anything"""
    T = TILE
    p = cases.pool(T)
    c = cases.random_case(p[:2], 60, 11)
    want = c.reference()
    rng = np.random.default_rng(3)
    part = rng.integers(0, 2, c.size)
    first = c.reference(match=np.where(part == 0, c.match, -1).astype(np.int32))
    both = c.reference(into=first[0], match=np.where(part == 1, c.match, -1).astype(np.int32))
    assert all(np.array_equal(x, y) for x, y in zip(both, want))
    assert not np.array_equal(first[0], want[0]) and want[1].max() >= 3
    # anything: the clamp makes it a forest, and the labels are the minima of the merged trees
    junk = rng.integers(-2 ** 31, 2 ** 31, c.total).astype(np.int32)
    junk[::3] = rng.integers(0, c.total, len(junk[::3]))                       # (some entries in range, above and below their index)
    got = c.reference(into=junk)
    assert (got[0] <= want[0]).all() and (got[0][got[0]] == got[0]).all() and not np.array_equal(got[0], want[0])
    io = np.array([1, 9, 20, 20, 41, 55], np.int64)
    small = cases.random_case((io, 58), 9, 5, share=0.6)
    junk = rng.integers(-70, 70, 58).astype(np.int32)
    r = np.arange(58)
    parent = np.where((junk < 0) | (junk > r), r, junk)
    u, v = small.links()
    assert np.array_equal(small.reference(into=junk)[0], cases.closure(58, np.concatenate([u, r]), np.concatenate([v, parent])))
    assert (parent != r).sum() > 5 and len(u) > 5


def test_the_decoy_pool_has_conflicting_and_long_tracks():
    """the numpy matcher's own mutual matches on q8_edges_cases' shared pool: the GPU tests on matched data bite"""
    R = lfp.match_q8_pairs_plan(0, 0, 0)[0]
    q, io, _, _, ea, eb = ecases.shared_pool(R)
    la, lb, (ab, ba, _, _) = ecases.shared_reference(R)
    m_ab, _ = pcases.mutual(ab, ba, la.astype(np.int64), lb.astype(np.int64))
    track, length, dup = cases.build_tracks(io, len(q), ea, eb, la, int(la[-1]), m_ab)
    assert (dup > 0).any() and (length >= 3).any() and (length[dup == 0] >= 3).any()
    assert length.sum() == len(q) and (length[track] >= 1).all()


def test_the_shared_cases():
    """what the GPU tests rely on: the chains are one track, the stars contend on one root, the cycles conflict where planted"""
    T = TILE
    io, total, names = cases.pool(T)
    assert total <= 40000 and sorted(set(np.diff(io).tolist())) == sorted({0, 1, 2, 3, 11, 40, 63, 64, 65, 255, 256, 257, 290, 300, 305, 310, 2 * T + 1})
    for descending in (False, True):
        track, length, dup = cases.chain(T, descending).reference()
        first = int(io[names["small"]])
        assert length[first] == cases.SMALL and dup.sum() == 0 and (length > 0).sum() == total - cases.SMALL + 1
    one, two = cases.stars(T, False), cases.stars(T, True)
    hub = int(io[names["X"]]) + 5
    t1, l1, d1 = one.reference()
    assert l1.max() == l1[t1[hub]] >= 2000 and (l1 > 1).sum() == 1
    t2, l2, d2 = two.reference()
    assert (l2 > 1).sum() == 1 and l2.max() == l1.max() + 1         # one track again, through the single joining link
    two.match[-1] = -1
    assert (two.reference()[1] > 1).sum() == 2
    track, length, dup = cases.cycles(T).reference()
    X, L = int(io[names["X"]]), int(io[names["L"]])
    assert all(length[X + k] == 3 and dup[X + k] == 0 for k in range(100))
    assert all(length[X + k] == 4 and dup[X + k] == 1 for k in range(100, 150))
    assert length[X + 270] == 2 and dup[X + 270] == 1
    assert length[L + 3] == 4 and dup[L + 3] == 2 and dup.sum() == 50 + 1 + 2
