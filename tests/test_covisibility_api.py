"""CPU tests of covisibility tables (include/lf_mkd.h: lf_mkd_covisibility_plan, lf_mkd_covisibility_device): the symbols exist
with the header's arities and constants, every refusal is made with its message without a device, the plan reports what the
header says and grows with its arguments, and the two formulations of the numpy restatement the GPU tests compare against
(tests/covisibility_cases.py) agree on every case of the generator."""
import ctypes
import os
import re

import numpy as np

import covisibility_cases as cases
from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_covisibility_plan", 9), ("lf_mkd_covisibility_device", 13)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "covisibility") and hasattr(lfp.MkdHandle, "covisibility_device")
    assert int(re.search(r"#define LF_MKD_COVIS_ACCUMULATE \((\d+)u\)", header).group(1)) == lfp.COVIS_ACCUMULATE == cases.ACCUMULATE == 1
    assert int(re.search(r"#define LF_MKD_COVIS_FORM_LDS \((\d+)u\)", header).group(1)) == lfp.COVIS_FORM_LDS == 256


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def call(off=p, t_cap=10, img=p, o_cap=30, counts=p, n=5, ea=None, eb=None, n_edges=0, flags=0, covis=p):
        return L.lf_mkd_covisibility_device(None, off, t_cap, img, o_cap, counts, n, ea, eb, n_edges, flags, covis, None)

    for kw, what in [({}, b"null handle"), ({"flags": 1}, b"null handle"), ({"ea": p, "eb": p, "n_edges": 7}, b"null handle"),
                     ({"ea": p, "eb": p}, b"null handle"),                       # both given, n_edges == 0: nothing to mask
                     ({"n": 0, "covis": None}, b"null handle"), ({"o_cap": 0, "img": None}, b"null handle"),
                     ({"t_cap": 0}, b"null handle"), ({"n": 46340, "t_cap": BIG, "o_cap": BIG}, b"null handle"),
                     ({"covis": None}, b"null d_covis"), ({"counts": None}, b"null d_table_counts"),
                     ({"off": None}, b"null d_track_offsets"), ({"img": None}, b"null d_obs_image"),
                     ({"ea": p}, b"only one of"), ({"eb": p, "n_edges": 3}, b"only one of"),
                     ({"n_edges": 3}, b"n_edges > 0 without"),
                     ({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
                     ({"off": odd8}, b"8-byte aligned"), ({"off": odd4}, b"8-byte aligned"),
                     ({"img": odd4}, b"4-byte aligned"), ({"counts": odd4}, b"4-byte aligned"), ({"covis": odd4}, b"4-byte aligned"),
                     ({"ea": odd4, "eb": p, "n_edges": 1}, b"4-byte aligned"), ({"ea": p, "eb": odd4, "n_edges": 1}, b"4-byte aligned"),
                     ({"n": 46341}, b"n_images^2"), ({"n": 2 ** 32 - 1}, b"n_images^2"),
                     ({"t_cap": BIG + 1}, b"2^31 - 1"), ({"o_cap": BIG + 1}, b"2^31 - 1"), ({"o_cap": 1 << 40}, b"2^31 - 1")]:
        if what == b"null handle":
            assert call(**kw) == -1 and L.lf_mkd_last_error(None) == b"covisibility_device: null handle", kw
        else:
            _refused(L, call(**kw), b"covisibility_device", what, kw)


def test_the_plan():
    L = lfp.load_library()
    none = (None,) * 4
    for args, what in (((5, 10, 30, 0, 2), b"unknown flag bits"), ((46341, 10, 30, 0, 0), b"n_images^2"),
                       ((5, BIG + 1, 30, 0, 0), b"2^31 - 1"), ((5, 10, BIG + 1, 0, 1), b"2^31 - 1")):
        _refused(L, L.lf_mkd_covisibility_plan(*args, *none), b"covisibility_plan", what, args)
    assert L.lf_mkd_covisibility_plan(46340, BIG, BIG, 1 << 40, 1, *none) == 0  # every output is optional
    for t_cap, o_cap, n_edges in ((0, 0, 0), (10, 30, 0), (BIG, BIG, 5)):
        assert lfp.covisibility_plan(0, t_cap, o_cap, n_edges)[1:] == (0, 0, 0)  # no image: nothing is launched or kept
    # launches: the zeroing, the two counting launches unless a capacity is 0, the mask iff there are edges
    assert lfp.covisibility_plan(5, 10, 30)[2] == lfp.covisibility_plan(5, 10, 30, flags=1)[2] == 3
    assert lfp.covisibility_plan(5, 10, 30, 9)[2] == 4
    assert lfp.covisibility_plan(5, 0, 30)[1:] == (0, 1, 0) and lfp.covisibility_plan(5, 10, 0, 2)[1:] == (0, 2, 0)
    # the scratch: one bit per 64 observations, in words
    for o_cap in (1, 2047, 2048, 2049, 1 << 20, BIG):
        assert lfp.covisibility_plan(5, 10, o_cap)[3] == 4 * -(-o_cap // 2048)
    # form: the lanes that share a track hold twice the mean length the capacities allow, never more than the images
    for n, t_cap, o_cap, lanes in ((1, 10, 1000, 4), (4, 10, 1000, 4), (5, 10, 1000, 8), (8, 10, 1000, 8), (9, 10, 1000, 16),
                                   (33, 10, 1000, 64), (1000, 1000, 1000, 4), (1000, 1000, 2000, 4), (1000, 1000, 2001, 8),
                                   (1000, 1000, 4000, 8), (1000, 1000, 4001, 16), (1000, 1000, 16001, 64), (1000, 1, BIG, 64)):
        form = lfp.covisibility_plan(n, t_cap, o_cap)[0]
        assert form & 255 == lanes and form & ~(255 | lfp.COVIS_FORM_LDS) == 0, (n, t_cap, o_cap, form)
    lds = [n for n in range(1, 200) if lfp.covisibility_plan(n, 100, 1000)[0] & lfp.COVIS_FORM_LDS]
    assert lds == list(range(1, len(lds) + 1)) and len(lds) in (0, 64)          # one threshold, below it the private table
    # monotone: in n_images, in obs_capacity, in n_edges, and in track_capacity along a fixed mean length.  The grid grows with
    # n_images in the direct form; with the private table every workgroup adds n_images^2 words at its end, so there the grid
    # is held to 2^22 words in all (never below 256 workgroups) and may shrink as n_images grows
    grow = [1, 2, 3, 4, 5, 63, 64, 65, 1000, 46340]
    for t_cap in (1, 100, 10 ** 6):
        for o_cap in (1, 1000, 10 ** 7):
            rows = [lfp.covisibility_plan(n, t_cap, o_cap) for n in grow]
            assert all(a[0] & 255 <= b[0] & 255 and a[2:] == b[2:] for a, b in zip(rows, rows[1:]))
            assert all(a[1] <= b[1] for a, b in zip(rows, rows[1:]) if not (a[0] | b[0]) & lfp.COVIS_FORM_LDS)
            assert all(r[1] <= max(256, (1 << 22) // (n * n)) for n, r in zip(grow, rows) if r[0] & lfp.COVIS_FORM_LDS)
    for n in (3, 64, 1000):
        for t_cap in (1, 100, 10 ** 6):
            rows = [lfp.covisibility_plan(n, t_cap, o) for o in (1, 10, 100, 10 ** 4, 10 ** 6, 10 ** 8, BIG)]
            assert all(a[0] <= b[0] and a[1] <= b[1] and a[2] == b[2] and a[3] <= b[3] for a, b in zip(rows, rows[1:]))
        for mean in (1, 3, 50):
            rows = [lfp.covisibility_plan(n, t, t * mean) for t in (1, 7, 64, 1000, 10 ** 5, 10 ** 7)]
            assert all(a[0] == b[0] and a[1] <= b[1] and a[3] <= b[3] for a, b in zip(rows, rows[1:]))
        rows = [lfp.covisibility_plan(n, 100, 1000, e) for e in (0, 1, 1000, BIG)]
        assert [r[2] for r in rows] == [3, 4, 4, 4] and len({(r[0], r[1], r[3]) for r in rows}) == 1


def test_the_two_formulations_agree_on_every_case():
    all_cases = cases.cases() + cases.capacity_cases()
    assert len(all_cases) > 50
    total = 0
    for name, tab, n in all_cases:
        a = cases.covisibility(tab, n)
        b = cases.covisibility(tab, n, matrix=True)
        assert a.dtype == b.dtype == np.uint32 and a.shape == (n, n) and (a == b).all(), name
        sparse = cases.pairs(tab, n, matrix=True)
        assert sparse == cases.pairs(tab, n) and all(a[i, j] == v for (i, j), v in sparse.items()), name
        assert np.count_nonzero(a) == len(sparse), name
        if name.split("-")[0] in ("consistent", "duplicated"):
            assert (a == a.T).all(), name                                        # images that do not decrease: symmetric,
            lists = cases.counted_lists(tab, n)                                  # one count per distinct image of a track
            assert all(len(set(D)) == len(D) for D in lists), name
            assert a.trace() == sum(len(D) for D in lists)
        total += int(a.sum())
    assert total > 10 ** 5


def test_the_restatement_by_hand():
    tab = cases.from_tracks([[0, 0, 1, 1, 1, 2], [2], [], [1, 2]])
    for matrix in (False, True):
        assert cases.covisibility(tab, 3, matrix=matrix).tolist() == [[1, 1, 1], [1, 2, 2], [1, 2, 3]]
        # ids at or beyond n_images are never counted, but break a run of equal raw neighbours
        assert cases.covisibility(tab, 2, matrix=matrix).tolist() == [[1, 1], [1, 2]]
        out = cases.from_tracks([[1, 7, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0]])
        assert cases.covisibility(out, 2, matrix=matrix).tolist() == [[1, 2], [2, 2]]
        # unsorted images: ordered pairs of distinct positions with different images, the diagonal counts positions
        assert cases.covisibility(cases.from_tracks([[0, 1, 0]]), 2, matrix=matrix).tolist() == [[2, 2], [2, 1]]
        # the mask, ACCUMULATE and the reduction mod 2^32
        into = np.array([[0xFFFFFFFF, 5, 0], [0, 0, 0], [9, 0, 7]], np.uint32)
        got = cases.covisibility(tab, 3, edges=([0, 2, 5, 1], [1, 2, 0, 0xFFFFFFFF]), into=into, matrix=matrix)
        assert got.tolist() == [[0, 0, 1], [0, 2, 2], [10, 2, 0]]
    parts = cases.split(tab, 3)
    acc = None
    for part in parts:
        acc = cases.covisibility(part, 3, into=acc)
    assert (acc == cases.covisibility(tab, 3)).all()
