"""CPU tests of edge-list matching over 8-bit descriptors (include/lf_mkd.h, "edge lists"): the three symbols exist and refuse
bad arguments without a device; the numpy restatements the GPU tests compare against (tests/q8_edges_cases.py) agree with the
pair layout's on chain edges, with cumsum and fancy indexing; and the shared pool's decoys bite."""
import ctypes

import numpy as np

import q8_cases as qcases
import q8_edges_cases as cases
import q8_pairs_cases as pq

import local_features_python as lfp

NAMES = ("lf_mkd_edge_layout_device", "lf_mkd_gather_edge_rows_device", "lf_mkd_match_q8_edges_device")
BIG = (1 << 31) - 1


def test_the_symbols_are_exported():
    L = lfp.load_library()
    for name in NAMES:
        assert name in lfp.SYMBOLS and hasattr(L, name), name
    for method in ("edge_layout", "gather_edge_rows", "match_q8_edges"):
        assert hasattr(lfp.LocalFeatures, method), method
    for method in ("edge_layout_device", "gather_edge_rows_device", "match_q8_edges_device"):
        assert hasattr(lfp.MkdHandle, method), method


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_matcher_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)   # never dereferenced: the arguments are refused first

    def call(a=p, ioa=p, n_a=3, na=64, b=p, iob=p, n_b=3, nb=64, ea=p, eb=p, la=p, cap_a=64, lb=p, cap_b=64, n_edges=5,
             ratio=0.8, flags=0, ab=p, ba=p, best=p, second=p):
        return L.lf_mkd_match_q8_edges_device(None, a, ioa, n_a, na, b, iob, n_b, nb, ea, eb, la, cap_a, lb, cap_b, n_edges, ratio,
                                              flags, ab, ba, best, second, None)

    R = lfp.match_q8_pairs_plan(0, 0, 0)[0]
    for kw, what in [({}, b"null handle"), ({"n_edges": 0}, b"null handle"),
                     ({"best": None, "second": None}, b"null handle"),               # d_best and d_second may be NULL
                     ({"lb": None, "cap_b": 0, "ba": None}, b"null handle"),          # one direction: NULL / 0 together
                     ({"flags": lfp.MATCH_MUTUAL}, b"null handle"),
                     ({"n_a": 0, "n_b": 0xFFFFFFFF}, b"null handle"),                 # any image counts
                     ({"na": BIG, "nb": BIG, "cap_a": BIG, "cap_b": 0, "n_edges": 1}, b"null handle"),
                     ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"), ({"ioa": None}, b"null pointer"),
                     ({"iob": None}, b"null pointer"), ({"ab": None}, b"null pointer"),
                     ({"ea": None}, b"null edge array"), ({"eb": None}, b"null edge array"),
                     ({"la": None}, b"null layout array"), ({"lb": None}, b"null layout array"),
                     ({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
                     ({"flags": lfp.MATCH_MUTUAL, "ba": None}, b"LF_MKD_MATCH_MUTUAL needs d_match_ba"),
                     ({"flags": lfp.MATCH_MUTUAL, "ba": None, "lb": None, "cap_b": 0}, b"LF_MKD_MATCH_MUTUAL needs d_match_ba"),
                     ({"a": ctypes.c_void_p(72)}, b"16-byte aligned"), ({"b": ctypes.c_void_p(68)}, b"16-byte aligned"),
                     ({"na": BIG + 1}, b"2^31 - 1"), ({"nb": 1 << 40}, b"2^31 - 1"), ({"cap_a": BIG + 1}, b"2^31 - 1"),
                     ({"cap_b": BIG + 1}, b"2^31 - 1"),
                     # the grid is the pairs plan's over the capacities: floor(cap / R) + n_edges per direction
                     ({"cap_a": BIG, "cap_b": BIG, "n_edges": 0xFFFFFFFF}, b"workgroups"),
                     ({"cap_a": 0, "cap_b": 0, "n_edges": 1 << 30}, b"workgroups"),
                     ({"cap_a": 0, "cap_b": 0, "n_edges": 1 << 30, "ba": None, "lb": None}, b"null handle"),
                     ({"cap_a": BIG, "cap_b": 0, "n_edges": BIG - BIG // R, "ba": None, "lb": None}, b"null handle"),
                     ({"cap_a": BIG, "cap_b": 0, "n_edges": BIG - BIG // R + 1, "ba": None, "lb": None}, b"workgroups")]:
        _refused(L, call(**kw), b"match_q8_edges_device", what, kw)
    # that grid is what the plan function reports (and refuses) for the same numbers
    assert lfp.match_q8_pairs_plan(BIG, 0, BIG - BIG // R, False)[1] == BIG
    assert L.lf_mkd_match_q8_pairs_plan(BIG, 0, BIG - BIG // R + 1, 0, None, None) == -1


def test_layout_and_gather_refuse_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)

    def layout(io=p, n_images=3, total=64, edge=p, n_edges=5, out=p):
        return L.lf_mkd_edge_layout_device(None, io, n_images, total, edge, n_edges, out, None)

    for kw, what in [({}, b"null handle"), ({"n_edges": 0}, b"null handle"),
                     ({"n_edges": 0, "io": None, "edge": None, "out": None}, b"null handle"),
                     ({"n_images": 0}, b"null handle"), ({"total": BIG, "n_edges": 0xFFFFFFFF}, b"null handle"),
                     ({"io": None}, b"null pointer"), ({"edge": None}, b"null pointer"), ({"out": None}, b"null pointer"),
                     ({"io": odd8}, b"8-byte aligned"), ({"out": odd8}, b"8-byte aligned"), ({"edge": odd4}, b"4-byte aligned"),
                     ({"total": BIG + 1}, b"2^31 - 1")]:
        _refused(L, layout(**kw), b"edge_layout_device", what, kw)

    def gather(src=p, row_bytes=20, io=p, n_images=3, total=64, edge=p, eo=p, cap=64, n_edges=5, dst=p):
        return L.lf_mkd_gather_edge_rows_device(None, src, row_bytes, io, n_images, total, edge, eo, cap, n_edges, dst, None)

    for kw, what in [({}, b"null handle"), ({"n_edges": 0}, b"null handle"), ({"row_bytes": 4}, b"null handle"),
                     ({"row_bytes": 128}, b"null handle"), ({"row_bytes": 512}, b"null handle"),
                     ({"total": BIG, "cap": BIG}, b"null handle"),
                     ({"src": None}, b"null pointer"), ({"io": None}, b"null pointer"), ({"edge": None}, b"null pointer"),
                     ({"eo": None}, b"null pointer"), ({"dst": None}, b"null pointer"),
                     ({"row_bytes": 0}, b"row_bytes"), ({"row_bytes": 2}, b"row_bytes"), ({"row_bytes": 22}, b"row_bytes"),
                     ({"row_bytes": 516}, b"row_bytes"), ({"row_bytes": 1 << 31}, b"row_bytes"),
                     ({"src": odd4}, b"4-byte aligned"), ({"dst": odd4}, b"4-byte aligned"),
                     ({"total": BIG + 1}, b"2^31 - 1"), ({"cap": BIG + 1}, b"2^31 - 1"),
                     ({"cap": BIG, "n_edges": 0xFFFFFFFF}, b"workgroups")]:
        _refused(L, gather(**kw), b"gather_edge_rows_device", what, kw)


def test_chain_edges_equal_the_sequence_layout():
    """frame t against frame t + 1 of one array: the edge reference on edges (t, t + 1) is q8_pairs_cases.match_pairs on the
    array passed twice with shifted offsets, entry for entry once each side's layout is laid beside the array"""
    sizes = [300, 17, 0, 450, 1, 233, 64, 129]
    q, io, _, _ = cases.make_pool(sizes, 31)
    F, n = len(sizes), len(q)
    ea, eb = cases.chain_edges(F)
    la, lb = cases.edge_layout(io, n, ea), cases.edge_layout(io, n, eb)
    # the a side's layout is the frames 0 .. F - 2 back to back: the pool's own offsets, shifted by the lead rows
    assert np.array_equal(la.astype(np.int64), io[:F] - io[0]) and np.array_equal(lb.astype(np.int64), io[1:] - io[1])
    ab, ba, best, second = cases.match_edges(q, io, q, io, ea, eb, la, int(la[-1]), lb, int(lb[-1]))
    want = pq.match_pairs(q, io[:F], q, io[1:])
    assert np.array_equal(ab, want[0][io[0]:io[F - 1]]) and np.array_equal(best, want[2][io[0]:io[F - 1]])
    assert np.array_equal(second, want[3][io[0]:io[F - 1]]) and np.array_equal(ba, want[1][io[1]:io[F]])
    assert (ab >= 0).any() and (ba >= 0).any() and (ab == -1).any()            # accepted and rejected rows both occur
    # nothing of the rows of no image took part: the rows in front of and behind the images changed, the result did not
    q2 = q.copy()
    q2[:io[0]], q2[io[-1]:] = q[io[0] + 20:io[0] + 20 + cases.LEAD], q[io[0] + 40:io[0] + 40 + cases.TRAIL]
    again = cases.match_edges(q2, io, q2, io, ea, eb, la, int(la[-1]), lb, int(lb[-1]))
    assert all(np.array_equal(x, y) for x, y in zip(again, (ab, ba, best, second)))


def test_layout_and_gather_restatements():
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 40, 23)
    io = 9 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(io[-1]) + 4
    edge = rng.integers(0, 23, 500).astype(np.uint32)
    lay = cases.edge_layout(io, total, edge)
    assert lay.dtype == np.uint64 and np.array_equal(lay, np.concatenate([[0], np.cumsum(sizes[edge])]))
    # ids out of range are empty images; a total inside the pool cuts the images behind it; an inverted range is empty
    edge2 = np.concatenate([edge, [23, 24, cases.NO_IMAGE, 5]]).astype(np.uint32)
    assert np.array_equal(cases.edge_layout(io, total, edge2), np.concatenate([lay, lay[-1:], lay[-1:], lay[-1:], lay[-1:] + sizes[5]]))
    cut = int(io[11]) + 3
    rows_cut = np.clip(np.minimum(io[1:], cut) - np.minimum(io[:-1], cut), 0, None)
    assert np.array_equal(cases.edge_layout(io, cut, edge), np.concatenate([[0], np.cumsum(rows_cut[edge])]))
    inv = io.copy()
    inv[7] = inv[8] + 5                                       # image 7 inverted (empty), image 6 longer
    rows_inv = np.clip(inv[1:] - inv[:-1], 0, None)
    assert rows_inv[7] == 0 and np.array_equal(cases.edge_layout(inv, total, edge), np.concatenate([[0], np.cumsum(rows_inv[edge])]))
    assert np.array_equal(cases.edge_layout(io, total, []), [0])
    # the gather is fancy indexing: row lo + r of the layout is row first + r of the pool
    src = rng.integers(0, 1 << 30, (total, 5)).astype(np.int32)
    cap = int(lay[-1])
    index = np.concatenate([np.arange(io[m], io[m + 1]) for m in edge]).astype(np.int64)
    got = cases.gather_edge_rows(src, io, total, edge, lay, cap, np.full((cap + 6, 5), -7, np.int32))
    assert np.array_equal(got[:cap], src[index]) and (got[cap:] == -7).all()
    short = cap - int(sizes[edge[-1]]) - 2                     # cut inside the last but one edge (or at its end)
    got = cases.gather_edge_rows(src, io, total, edge, lay, short, np.full((cap + 6, 5), -7, np.int32))
    assert np.array_equal(got[:short], src[index[:short]]) and (got[short:] == -7).all()


def test_the_shared_pool_and_its_decoys():
    R = lfp.match_q8_pairs_plan(0, 0, 0)[0]
    q, io, ids, decoys, ea, eb = cases.shared_pool(R)
    n_images = len(io) - 1
    sizes = np.diff(io)
    assert [int(sizes[i]) for i in ids] == cases.image_sizes(R) and io[0] == cases.LEAD and len(q) - io[-1] == cases.TRAIL
    assert len(decoys) == len(cases.DESIGNATED) and n_images == len(ids) + 2 * len(decoys)
    assert len(ea) == n_images * n_images + 3 and (ea[:n_images * n_images] * n_images + eb[:n_images * n_images]
                                                    == np.arange(n_images * n_images)).all()
    assert (ea[-3], eb[-3]) == (ea[n_images + 2], eb[n_images + 2]) and ea[-2] == n_images and eb[-1] == cases.NO_IMAGE
    assert (q != 0).all()                                      # every row is a quantiser's output
    # the decoy check bites on at least one edge per designated image, the partner's among them
    hits = cases.decoys_bite(R)
    assert sorted(hits) == [b for _, b, _ in decoys]
    for b, edges in hits.items():
        assert ids[cases.PARTNER] in edges, (b, edges)
    # the planted ties are there: second == best for some row of an edge whose b image holds a duplicated row
    la, lb, (ab, ba, best, second) = cases.shared_reference(R)
    e = ids[cases.PARTNER] * n_images + ids[cases.PARTNER]      # the partner against itself: rows 10 and 250 are the same row
    lo = int(la[e])
    assert best[lo + 10] == second[lo + 10] == best[lo + 250] and ab[lo + 10] == -1
    assert qcases.match_q8(q[io[ids[10]]:io[ids[10] + 1]], q[io[ids[10]]:io[ids[10] + 1]], 0.0)[0][10] == 250   # the highest index
    # too few candidates: every edge onto the 0-row and the 1-row image is refused, whatever the ratio
    for tiny in (ids[0], ids[1]):
        for a in (ids[9], ids[1]):
            s = slice(int(la[a * n_images + tiny]), int(la[a * n_images + tiny + 1]))
            assert (ab[s] == -1).all() and (best[s] == cases.INT32_MIN).all() and s.stop - s.start == sizes[a]
    assert (ab >= 0).sum() > 1000 and len(ab) == la[-1] and len(ba) == lb[-1]
