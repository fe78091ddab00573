"""CPU tests of link tables (include/lf_mkd.h: lf_mkd_link_table_plan, lf_mkd_link_table_device): the symbols exist and refuse
bad arguments without a device, the plan reports what the header says, and the two formulations of the numpy restatement the GPU
tests compare against (tests/link_table_cases.py) agree -- on the shared track cases, on every min_links around an edge's count,
on every link capacity of a small case, and with tracks_cases.build_tracks on the pruned match array."""
import ctypes
import os
import re

import numpy as np

import link_table_cases as cases
import tracks_cases as tcases
from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
TILE = lfp.TRACKS_DUP_TILE


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_link_table_plan", 7), ("lf_mkd_link_table_device", 21)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "link_table") and hasattr(lfp.MkdHandle, "link_table_device")
    assert int(re.search(r"#define LF_MKD_LINK_TABLE_LOCAL \((\d+)u\)", header).group(1)) == lfp.LINK_TABLE_LOCAL == 1


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)
    slot = lfp.link_table_plan(0, 0)[0]

    def call(io=p, n_images=3, total=64, ea=p, eb=p, la=p, cap=64, n_edges=5, match=p, min_links=0, flags=0, l_cap=64, offsets=p,
             link_a=p, link_b=p, link_edge=p, edge_links=p, kept=p, counts=p):
        return L.lf_mkd_link_table_device(None, io, n_images, total, ea, eb, la, cap, n_edges, match, min_links, flags, l_cap,
                                          offsets, link_a, link_b, link_edge, edge_links, kept, counts, None)

    for kw, what in [({}, b"null handle"), ({"flags": lfp.LINK_TABLE_LOCAL}, b"null handle"),
                     ({"link_edge": None, "edge_links": None, "kept": None}, b"null handle"),
                     ({"l_cap": 0, "link_a": None, "link_b": None}, b"null handle"), ({"min_links": 2 ** 32 - 1}, b"null handle"),
                     ({"n_edges": 0, "ea": None, "eb": None, "la": None, "match": None}, b"null handle"),
                     ({"total": BIG, "cap": BIG, "l_cap": BIG}, b"null handle"),
                     ({"cap": BIG, "n_edges": BIG - BIG // slot}, b"null handle"),
                     ({"io": None}, b"null pointer"), ({"offsets": None}, b"null pointer"), ({"counts": None}, b"null pointer"),
                     ({"ea": None}, b"null edge array"), ({"eb": None}, b"null edge array"), ({"la": None}, b"null layout array"),
                     ({"match": None}, b"null match array"), ({"link_a": None}, b"null d_link_a or d_link_b"),
                     ({"link_b": None}, b"null d_link_a or d_link_b"),
                     ({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
                     ({"io": odd8}, b"8-byte aligned"), ({"la": odd8}, b"8-byte aligned"), ({"offsets": odd8}, b"8-byte aligned"),
                     ({"ea": odd4}, b"4-byte aligned"), ({"eb": odd4}, b"4-byte aligned"), ({"match": odd4}, b"4-byte aligned"),
                     ({"link_a": odd4}, b"4-byte aligned"), ({"link_b": odd4}, b"4-byte aligned"),
                     ({"link_edge": odd4}, b"4-byte aligned"), ({"edge_links": odd4}, b"4-byte aligned"),
                     ({"kept": odd4}, b"4-byte aligned"), ({"counts": odd4}, b"4-byte aligned"),
                     ({"total": BIG + 1}, b"2^31 - 1"), ({"cap": BIG + 1}, b"2^31 - 1"), ({"l_cap": BIG + 1}, b"2^31 - 1"),
                     ({"total": 1 << 40}, b"2^31 - 1"),
                     ({"cap": BIG, "n_edges": BIG - BIG // slot + 1}, b"workgroups"), ({"n_edges": BIG + 1}, b"workgroups")]:
        _refused(L, call(**kw), b"link_table_device", what, kw)


def test_the_plan():
    L = lfp.load_library()
    none = (None,) * 5
    assert L.lf_mkd_link_table_plan(BIG + 1, 1, *none) == -1
    assert L.lf_mkd_last_error(None).startswith(b"link_table_plan: ") and b"2^31 - 1" in L.lf_mkd_last_error(None)
    assert L.lf_mkd_link_table_plan(0, BIG + 1, *none) == -1
    assert L.lf_mkd_last_error(None).startswith(b"link_table_plan: ") and b"workgroups" in L.lf_mkd_last_error(None)
    assert L.lf_mkd_link_table_plan(BIG, 5, *none) == 0                        # every output is optional
    S, slots, F, levels, scratch = lfp.link_table_plan(0, 0)
    assert (slots, levels, scratch) == (0, 0, 0)
    assert 64 <= S <= 1024 and S % 64 == 0 and 2 <= F <= 4096
    assert lfp.link_table_plan(10 * S + 3, 0) == (S, 10, F, 0, 0)              # no edge: no scan, no scratch
    last = 0
    for cap in [0, 1, S - 1, S, S + 1, F * S - 1, F * S, F * S + 1, 4032000, F * F * S, 2 ** 30 + 7, BIG]:
        for n_edges in (1, 2, F - 1, F, F + 1, F + 3, F * F, F * F + 3, 2 ** 22 + 1):
            s, slots, f, levels, scratch = lfp.link_table_plan(cap, n_edges)
            assert (s, f) == (S, F) and slots == cap // S + n_edges
            assert levels >= 1 and F ** levels >= slots and (levels == 1 or F ** (levels - 1) < slots), (cap, n_edges)
            values, n = 0, slots
            for k in range(1, levels):
                n = -(-n // F)
                values += n
            assert scratch == 20 * slots + 12 * values + 4 * n_edges + 16, (cap, n_edges)
        scratch = lfp.link_table_plan(cap, 7)[4]
        assert scratch >= last                                                  # monotone in the capacity
        last = scratch
    assert lfp.link_table_plan(0, F)[3] == 1 and lfp.link_table_plan(0, F + 3)[3] == 2     # what the GPU tests' edge counts are for
    assert lfp.link_table_plan(0, F * F)[3] == 2 and lfp.link_table_plan(0, F * F + 3)[3] == 3


def test_the_two_formulations_agree_on_the_shared_cases():
    figures = {}
    for name, case in cases.shared_cases(TILE):
        u, v = case.links()
        for local in (False, True):
            a = cases.of_case(case, local=local, into=case.match)
            b = cases.of_case(case, True, local=local, into=case.match)
            assert a.same(b), (name, local)
            assert a.counts == [len(case.ea), len(u), len(case.ea), len(u)] and int(a.offsets[-1]) == len(u)
        # the table without the flag is tracks_cases.links' list, edge after edge
        a = cases.of_case(case)
        assert np.array_equal(a.link_a, u) and np.array_equal(a.link_b, v), name
        assert np.array_equal(np.diff(a.offsets.astype(np.int64)), a.edge_links) and (np.diff(a.link_edge.astype(np.int64)) >= 0).all()
        figures[name] = (len(case.ea), len(u))
        # a sentinel-filled output keeps its sentinels at the entries of no edge
        out = cases.of_case(case, into=np.full(case.size, tcases.SENTINEL, np.int32)).match_kept
        assert ((out == tcases.SENTINEL) | (out == -1) | (out == case.match)).all()
    assert figures["chain"] == (299, 299) and figures["cycles"] == (5, 454) and figures["star"] == (10, 2378)
    below = dict(cases.shared_cases(TILE))["capacity below"]
    assert below.cap < int(below.la[-1])                                       # the capacity cuts the last edges' ranges


def test_min_links_around_every_count():
    for name, case in cases.shared_cases(TILE)[4:]:
        L = cases.of_case(case).edge_links
        for e in sorted({0, len(L) // 2, len(L) - 1, int(np.argmax(L))}):
            for m in (0, 1, int(L[e]), int(L[e]) + 1, 2 ** 32 - 1):
                a = cases.of_case(case, min_links=m, into=case.match)
                assert a.same(cases.of_case(case, True, min_links=m, into=case.match)), (name, e, m)
                sel = L >= m
                assert a.counts == [int(sel.sum()), int(L[sel].sum())] * 2 and np.array_equal(a.edge_links, L)
                assert np.array_equal(np.diff(a.offsets.astype(np.int64)), np.where(sel, L, 0))
                assert len(a.edge(e)[0]) == (int(L[e]) if m <= int(L[e]) else 0)
        assert cases.of_case(case, min_links=2 ** 32 - 1).counts == [0, 0, 0, 0]


def test_every_link_capacity():
    case = tcases.random_case(tcases.odd_pool(), 30, 3)
    full = cases.of_case(case, min_links=2, into=case.match)
    wanted = full.counts[3]
    assert full.counts[0] == full.counts[2] >= 6 and 20 < wanted < 400
    W = full.offsets.astype(np.int64)
    cut_inside = 0
    for l_cap in range(0, wanted + 2):
        a = cases.of_case(case, min_links=2, link_capacity=l_cap, into=case.match)
        assert a.same(cases.of_case(case, True, min_links=2, link_capacity=l_cap, into=case.match)), l_cap
        o = a.counts[1]
        assert o <= l_cap and a.counts[2:] == full.counts[2:] and o in W
        assert o == wanted or min(w for w in W if w > o) > l_cap               # the next edge did not fit: never cut in the middle
        assert np.array_equal(a.link_a, full.link_a[:o]) and np.array_equal(a.link_b, full.link_b[:o])
        assert np.array_equal(a.offsets.astype(np.int64), np.minimum(W, o))
        assert (a.match_kept >= 0).sum() == o
        cut_inside += o < l_cap and o < wanted
    assert cut_inside > 50


def test_the_pruned_match_array_gives_the_tracks_of_the_kept_edges():
    for name, case in cases.shared_cases(TILE)[4:]:
        L = cases.of_case(case).edge_links
        m = int(np.sort(L)[-3])                                                # three edges or a few more are selected,
        l_cap = int(L[L >= m].sum()) - 1                                       # and the last of them does not fit
        assert m >= 1
        a = cases.of_case(case, min_links=m, link_capacity=l_cap, into=case.match)
        kept = np.diff(a.offsets.astype(np.int64)) > 0
        assert 0 < a.counts[0] < a.counts[2] < len(L), name
        got = case.reference(match=a.match_kept)
        # the links of the kept edges alone, built from a case that holds nothing else
        only = case.match.copy()
        for e in np.flatnonzero(~kept):
            lo, hi = int(min(case.la[e], case.cap)), int(min(case.la[e + 1], case.cap))
            only[lo:hi] = -1
        want = case.reference(match=only)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        track = tcases.components(tcases.forest(case.total), a.link_a.astype(np.int64), a.link_b.astype(np.int64))
        assert np.array_equal(track.astype(np.int32), got[0]), name            # and of the table's own rows
