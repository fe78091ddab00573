"""CPU tests of candidate edges (include/lf_mkd.h: lf_mkd_select_edges_plan, lf_mkd_select_edges_device): the symbols exist with
the header's arities and constants, every refusal is made with its message without a device, the plan reports what the header
says and grows with the shape, and the two formulations of the numpy restatement the GPU tests compare against
(tests/select_edges_cases.py) agree on every case of the generator."""
import ctypes
import os
import re

import numpy as np

import select_edges_cases as cases
from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_select_edges_plan", 10), ("lf_mkd_select_edges_device", 15)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "select_edges") and hasattr(lfp.MkdHandle, "select_edges_device")
    assert int(re.search(r"#define LF_MKD_SELECT_SKIP_SELF \((\d+)u\)", header).group(1)) == lfp.SELECT_SKIP_SELF == cases.SKIP_SELF == 1
    assert int(re.search(r"#define LF_MKD_SELECT_UNIQUE \((\d+)u\)", header).group(1)) == lfp.SELECT_UNIQUE == cases.UNIQUE == 2
    assert int(re.search(r"#define LF_MKD_SELECT_MAX_K \((\d+)\)", header).group(1)) == lfp.SELECT_MAX_K == 32


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)

    def call(votes=p, n_a=5, n_b=5, k=3, min_votes=1, flags=0, cap=15, rank=p, rank_votes=p, ea=p, eb=p, ev=p, counts=p):
        return L.lf_mkd_select_edges_device(None, votes, n_a, n_b, k, min_votes, flags, cap, rank, rank_votes, ea, eb, ev, counts, None)

    for kw, what in [({}, b"null handle"), ({"flags": 3}, b"null handle"), ({"k": 32, "min_votes": 2 ** 32 - 1}, b"null handle"),
                     ({"rank": None, "rank_votes": None, "ev": None}, b"null handle"),
                     ({"cap": 0, "ea": None, "eb": None}, b"null handle"),
                     ({"n_a": 0, "votes": None, "n_b": 0}, b"null handle"), ({"n_a": 0, "flags": 1}, b"null handle"),
                     ({"n_a": 1, "n_b": BIG, "cap": BIG}, b"null handle"), ({"n_a": BIG // 32, "n_b": 32, "k": 32}, b"null handle"),
                     ({"votes": None}, b"null d_votes"), ({"counts": None}, b"null d_counts"),
                     ({"ea": None}, b"null d_edge_a or d_edge_b"), ({"eb": None}, b"null d_edge_a or d_edge_b"),
                     ({"n_b": 0}, b"n_b == 0"), ({"k": 0}, b"k must be in [1, 32]"), ({"k": 33}, b"k must be in [1, 32]"),
                     ({"k": 2 ** 32 - 1}, b"k must be in [1, 32]"),
                     ({"flags": 4}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
                     ({"flags": 2, "n_b": 6}, b"n_a == n_b"), ({"flags": 3, "n_a": 4}, b"n_a == n_b"),
                     ({"votes": odd}, b"4-byte aligned"), ({"rank": odd}, b"4-byte aligned"), ({"rank_votes": odd}, b"4-byte aligned"),
                     ({"ea": odd}, b"4-byte aligned"), ({"eb": odd}, b"4-byte aligned"), ({"ev": odd}, b"4-byte aligned"),
                     ({"counts": odd}, b"4-byte aligned"),
                     ({"n_a": 1 << 16, "n_b": 1 << 15}, b"n_a * n_b"), ({"n_a": 2, "n_b": 1 << 30}, b"n_a * n_b"),
                     ({"n_a": BIG // 32 + 1, "n_b": 1, "k": 32}, b"2^31 - 1"), ({"cap": BIG + 1}, b"2^31 - 1"),
                     ({"cap": 1 << 40}, b"2^31 - 1")]:
        if what == b"null handle":
            assert call(**kw) == -1 and L.lf_mkd_last_error(None) == b"select_edges_device: null handle", kw
        else:
            _refused(L, call(**kw), b"select_edges_device", what, kw)


def test_the_plan():
    L = lfp.load_library()
    none = (None,) * 5
    for args, what in (((5, 5, 0, 5, 0), b"k must be"), ((5, 5, 33, 5, 0), b"k must be"), ((5, 5, 3, 5, 4), b"unknown flag bits"),
                       ((5, 6, 3, 5, 2), b"n_a == n_b"), ((5, 0, 3, 5, 0), b"n_b == 0"), ((1 << 16, 1 << 15, 3, 5, 0), b"n_a * n_b"),
                       ((5, 5, 3, BIG + 1, 0), b"2^31 - 1")):
        _refused(L, L.lf_mkd_select_edges_plan(*args, *none), b"select_edges_plan", what, args)
    assert L.lf_mkd_select_edges_plan(1, BIG, 32, BIG, 1, *none) == 0          # every output is optional
    assert lfp.select_edges_plan(0, 0, 3) == (4, 4, 0, 1, 0)                   # no row: one launch, no scratch
    assert lfp.select_edges_plan(0, 9, 3, 100)[2:] == (0, 1, 0)
    # compiled_k: the smallest instantiation at or above k
    forms = sorted({lfp.select_edges_plan(7, 7, k)[0] for k in range(1, 33)})
    assert forms[-1] == 32 and 2 <= len(forms) <= 6
    for k in range(1, 33):
        assert lfp.select_edges_plan(7, 7, k)[0] == min(f for f in forms if f >= k)
    # the forms along n_b: short rows share a workgroup, long ones own one, and few long rows are cut into segments
    for n_a in (1, 3, 7, 64, 1024, 16384):
        last_groups = last_scratch = 0
        seen = []
        for n_b in (1, 2, 63, 64, 65, 255, 1023, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 65536, BIG // n_a):
            ck, rows, groups, launches, scratch = lfp.select_edges_plan(n_a, n_b, 4)
            assert ck == 4 and rows in (1, 4) and launches in (4, 5)
            if rows == 4:
                assert groups == -(-n_a // 4) and launches == 4
            else:
                assert groups % n_a == 0 and (launches == 5) == (groups > n_a)
            segments = groups // n_a if rows == 1 else 1
            assert scratch == 12 * n_a * 4 + 16 * -(-n_a * 4 // 256) + (8 * n_a * segments * 4 if segments > 1 else 0)
            assert groups >= last_groups and scratch >= last_scratch            # monotone in n_b
            last_groups, last_scratch = groups, scratch
            seen.append((rows, launches))
        assert seen[0] == (4, 4) and seen[-1][0] == 1
        assert (seen[-1][1] == 5) == (n_a < 1024)                              # a device's worth of rows is not cut
    assert lfp.select_edges_plan(16384, 16384, 32)[1:4] == (1, 16384, 4)
    assert lfp.select_edges_plan(1, 1024, 4)[1:4] == (4, 1, 4)
    assert lfp.select_edges_plan(1, 65536, 4)[1] == 1 and lfp.select_edges_plan(1, 65536, 4)[3] == 5
    # scratch grows with k and n_a
    assert lfp.select_edges_plan(100, 100, 8)[4] > lfp.select_edges_plan(100, 100, 4)[4] > lfp.select_edges_plan(50, 100, 4)[4]


def test_the_two_formulations_agree_on_every_case():
    all_cases = cases.cases()
    assert len(all_cases) > 500
    edges = 0
    for name, v, k, m, skip_self, unique in all_cases:
        a = cases.select_edges(v, k, m, skip_self, unique)
        b = cases.select_edges(v, k, m, skip_self, unique, loops=True)
        assert a.same(b), name
        n_a = v.shape[0]
        assert a.rank.shape == (n_a, k) and len(a.edge_a) == n_a * k and a.counts[0] == a.counts[1] <= a.counts[2] <= n_a * k
        kept = a.counts[0]
        assert (a.edge_a[kept:] == cases.PAD).all() and (a.edge_b[kept:] == cases.PAD).all() and (a.edge_votes[kept:] == 0).all()
        if unique:
            pairs = list(zip(a.edge_a[:kept].tolist(), a.edge_b[:kept].tolist()))
            assert len(set(pairs)) == len(pairs) and all(x < y for x, y in pairs), name
            # every pair either image picked is there
            want = {(min(i, int(j)), max(i, int(j))) for i in range(n_a) for j in a.rank[i] if j >= 0 and j != i}
            assert set(pairs) == want, name
        else:
            assert a.counts[1] == a.counts[2]
        edges += kept
    assert edges > 5000


def test_the_restatement_by_hand():
    v = cases.unique_table()
    r = cases.select_edges(v, 2, 1, unique=True)
    assert r.rank.tolist() == [[1, -1], [0, 3], [0, -1], [4, -1], [4, 3]]
    assert r.rank_votes.tolist() == [[9, 0], [8, 5], [7, 0], [6, 0], [10, 2]]
    assert list(zip(r.edge_a[:4].tolist(), r.edge_b[:4].tolist(), r.edge_votes[:4].tolist())) == [(0, 1, 9), (1, 3, 5), (0, 2, 7), (3, 4, 6)]
    assert r.counts == [4, 4, 7, 5] and (r.edge_a[4:] == cases.PAD).all() and len(r.edge_a) == 10
    r = cases.select_edges(v, 2, 1)
    assert r.counts == [7, 7, 7, 5] and (4, 4) in zip(r.edge_a.tolist(), r.edge_b.tolist())
    # ties go to the LOWER column, larger votes first, and unsigned: 2^32 - 1 beats 2^31
    t = np.array([[5, 9, 5, 9, 0, 2 ** 31, 2 ** 32 - 1, 5]], np.uint32)
    for loops in (False, True):
        r = cases.select_edges(t, 6, 1, loops=loops)
        assert r.rank.tolist() == [[6, 5, 1, 3, 0, 2]]
        assert cases.select_edges(t, 32, 0, loops=loops).rank[0, :8].tolist() == [6, 5, 1, 3, 0, 2, 7, 4]
        for cap in range(0, 9):
            c = cases.select_edges(t, 6, 1, capacity=cap, loops=loops)
            assert c.counts == [min(cap, 6), 6, 6, 1] and len(c.edge_a) == cap and c.edge_b[:min(cap, 6)].tolist() == [6, 5, 1, 3, 0, 2][:cap]
