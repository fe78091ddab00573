"""tests/big_pool_cases.py without a GPU: at the small mark (B = 2^16) every pool is materialised on the host and goes through
the suite's FULL restatement; the sparse expectation -- planted rows only, indices mapped back, sentinels everywhere else --
must equal it.  Every background condition is asserted by the builders at the seeds and at every mark the GPU tests use.  And
the expectations have teeth: a pool read through a wrapped address (row r mod B / R) gives another result for every family."""
from types import SimpleNamespace

import numpy as np
import pytest

import big_pool_cases as big
import match_guided_cases as mgcases
import match_pairs_cases as pcases
import q8_cases as qcases
import q8_edges_cases as ecases
import q8_grouped_cases as gcases
import q8_guided_cases as q8g
import q8_knn_cases as kcases
import q8_pairs_cases as pq
import tracks_cases as tcases

B = big.SMALL
SEED = 7100


def same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5])


def differ(got, want):
    return any(not np.array_equal(g, w) for g, w in zip(got, want))


def test_critical_rows():
    for mark in big.MARKS:
        for R in (128, 512, 20):
            total = big.total_rows(mark, R)
            crit = big.critical_rows(mark, R, total, SEED)
            assert crit[0] == 0 and crit[-1] == total - 1 and (np.diff(crit) > 0).all()
            for m in big.marks(mark):
                assert {m // R - 1, m // R, m // R + 1, -(-m // R), -(-m // R) + 1} <= set(crit.tolist())
                assert 20 <= ((crit >= m // R - 40) & (crit <= m // R + 41)).sum()
            assert total * R > mark and total % 32 != 0 and total % 64 != 0
    assert big.total_rows(1 << 32, 128) == 33558565 and big.total_rows(1 << 32, 512) == 8392741


@pytest.fixture(scope="module")
def single():
    return big.SingleQ8(B, SEED)


@pytest.fixture(scope="module")
def single_full(single):
    full = single.pool.to_numpy()
    assert len(full) == single.total and (full[single.crit] == single.planted).all()
    return full


def test_background_conditions_hold_at_every_mark():
    """the builders assert them; this runs every expectation the GPU tests ask for"""
    for mark in big.MARKS:
        s = big.SingleQ8(mark, SEED)
        s.expect_match_big_b()
        s.expect_match_big_b(ranges=True)
        s.expect_knn_big_b(1)
        s.expect_knn_big_b(5)
        s.expect_grouped_big_b()
        lo, hi, x, y = s.ranges()
        assert set(lo.tolist()) <= set(s.crit.tolist()) and set(hi.tolist()) <= set(s.crit.tolist())
        assert (lo >= mark // 128).any() and (hi > mark // 128).any() and (lo < mark // 256).any()


def test_single_pair_big_b(single, single_full):
    a = single.small[:big.NA_BIG_B]
    same(single.expect_match_big_b(), qcases.match_q8(a, single_full), "match")
    lo, hi, _, _ = single.ranges()
    want = qcases.match_q8(a, single_full, big.RATIO, lo, hi)
    same(single.expect_match_big_b(ranges=True), want, "match, ranges")
    assert differ(want, qcases.match_q8(a, single_full)), "the ranges change nothing"
    for k in (1, 5):
        same(single.expect_knn_big_b(k), kcases.knn_q8(a, single_full, k), ("knn", k))
    same(single.expect_grouped_big_b(), gcases.match_q8_grouped(a, single_full, single.groups_full()), "grouped")
    assert differ(single.expect_grouped_big_b()[1:], single.expect_match_big_b()[1:]), "the groups change nothing"
    # the ties across the marks are there
    m, best, second = single.expect_match_big_b(ratio=0.0)
    tie = np.flatnonzero(best == second)
    assert len(tie) >= 4 and {B // 256, B // 128} <= set(m[tie].tolist())
    # teeth: the pool read through wrapped addresses
    w = big.wrapped(single_full, B, 128)
    assert differ(qcases.match_q8(a, w), single.expect_match_big_b())
    assert differ(qcases.match_q8(a, w, big.RATIO, lo, hi), single.expect_match_big_b(ranges=True))
    assert differ(kcases.knn_q8(a, w, 1), single.expect_knn_big_b(1)) and differ(kcases.knn_q8(a, w, 5), single.expect_knn_big_b(5))
    assert differ(gcases.match_q8_grouped(a, w, single.groups_full()), single.expect_grouped_big_b())


def test_single_pair_big_a(single, single_full):
    b = single.small[:big.NB_BIG_A]
    w = big.wrapped(single_full, B, 128)
    for form, k, full in (("match", None, lambda a: qcases.match_q8(a, b)), ("knn", 1, lambda a: kcases.knn_q8(a, b, 1)),
                          ("knn", 5, lambda a: kcases.knn_q8(a, b, 5)),
                          ("grouped", None, lambda a: gcases.match_q8_grouped(a, b, single.groups_small()))):
        want = full(single_full)
        same(big.expand_big_a(single, *single.expect_big_a(form, k)), want, (form, k))
        assert differ(full(w), want), (form, k, "a wrapped pool gives the same result")


@pytest.mark.parametrize("far", ["a", "b", "both"])
@pytest.mark.parametrize("mutual", [False, True])
def test_pairs(far, mutual):
    P = big.Pooled(B, far, SEED + 1)
    qa, qb = P.pools["a"].to_numpy(), P.pools["b"].to_numpy()
    assert len(P.calls) == 6 and sum(len(oa) - 1 for oa, _ in P.calls) == 8

    def full(qa, qb):
        out = []
        for oa, ob in P.calls:
            oa, ob = oa.astype(np.int64), ob.astype(np.int64)
            got = list(pq.match_pairs(qa, oa, qb, ob, big.RATIO, fill=big.SENTINEL))
            if mutual:
                got[0], got[1] = pcases.mutual(got[0], got[1], oa, ob)
            out += got
        return out

    want = full(qa, qb)
    got = []
    for e in P.expect(mutual=mutual):
        got += [big.expand(e[k], n) for k, n in (("ab", len(qa)), ("ba", len(qb)), ("best", len(qa)), ("second", len(qa)))]
    same(got, want, (far, mutual))
    assert sum((w >= 0).sum() for w in want[0::4]) > 100 and sum((w >= 0).sum() for w in want[1::4]) > 100
    wa = big.wrapped(qa, B, 128) if far in ("a", "both") else qa
    wb = big.wrapped(qb, B, 128) if far in ("b", "both") else qb
    assert differ(full(wa, wb), want), "a wrapped pool gives the same result"


@pytest.mark.parametrize("long_range", [False, True])
@pytest.mark.parametrize("mutual", [False, True])
def test_edges(long_range, mutual):
    E = big.EdgesQ8(B, SEED + 2, long_range)
    q = E.pool.to_numpy()
    if long_range:
        assert E.la[1] == B // 4 + 5 and E.la[0] == 0
    else:
        assert np.array_equal(E.la, ecases.edge_layout(E.io_a, E.total, E.ea))

    def full(q):
        got = list(ecases.match_edges(q, E.io_a, q, E.io_b, E.ea, E.eb, E.la, E.cap_a, E.lb, E.cap_b, big.RATIO, big.SENTINEL))
        if mutual:
            # the device's filter leaves negative entries alone, so the sentinels of the long range stay
            ab, ba = pcases.mutual(got[0], got[1], E.la.astype(np.int64), E.lb.astype(np.int64))
            got[0], got[1] = np.where(got[0] < 0, got[0], ab), np.where(got[1] < 0, got[1], ba)
        return got

    want = full(q)
    e = E.expect(mutual=mutual)
    got = [big.expand(e[k], n) for k, n in (("ab", E.cap_a), ("ba", E.cap_b), ("best", E.cap_a), ("second", E.cap_a))]
    same(got, want, (long_range, mutual))
    assert (want[0] >= 0).sum() > 100
    if long_range:
        assert (want[0][E.control:B // 4 + 5] == big.SENTINEL).all()
    assert differ(full(big.wrapped(q, B, 128)), want), "a wrapped pool gives the same result"


@pytest.mark.parametrize("row_bytes", [512, 128])
def test_gather(row_bytes):
    G = big.Gather(B, row_bytes, SEED + 3)
    src = G.pool.to_numpy()
    c = B // row_bytes
    for k, (io, edge) in enumerate(G.lists):
        lay = G.layout(k)
        cap = int(lay[-1])
        want = ecases.gather_edge_rows(src, io, G.total, edge, lay, cap, np.zeros((cap + 8, row_bytes), np.uint8))
        (s0, d0, n), segs = G.expect(k)
        got = np.zeros_like(want)
        got[d0:d0 + n] = src[s0:s0 + n]
        for first, rows in segs:
            got[first:first + len(rows)] = rows
        assert np.array_equal(got, want), (row_bytes, k)
        # the far images' destination rows lie around and beyond the mark, as their source rows do
        assert any(first < c < first + len(rows) for first, rows in segs) and (k == 1 or any(first > c for first, _ in segs))
        wrapped = ecases.gather_edge_rows(big.wrapped(src, B, row_bytes), io, G.total, edge, lay, cap, np.zeros_like(want))
        assert not np.array_equal(wrapped, want)


def test_quantize():
    Q = big.Quantize(B, SEED + 4)
    full = Q.pool.to_numpy()
    want = qcases.quantize(full)
    rows, bg = Q.expect()
    got = np.tile(bg, (Q.total, 1))
    got[Q.crit] = rows
    assert np.array_equal(got, want)
    assert qcases.saturated(Q.rows).sum() > 10 and not qcases.saturated(Q.background[None]).any()
    assert not np.array_equal(qcases.quantize(big.wrapped(full, B, 512)), want)


@pytest.fixture(scope="module")
def tracks():
    return big.Tracks(B, SEED + 5)


def _tracks_full(T, edges=slice(None), into=None):
    """the full restatement: every image, the long layout, the match array entry by entry"""
    match = np.full(T.cap, -1, np.int32)
    for e, seg in enumerate(T.segments):
        match[int(T.la[e]):int(T.la[e]) + len(seg)] = seg
    sel = np.arange(len(T.ea))[edges]
    lay = T.la[sel[0]:sel[-1] + 2]
    return tcases.build_tracks(T.image_offsets(), T.total, T.ea[sel], T.eb[sel], lay, T.cap, match, into)


def _tracks_expanded(T, track, length, dup):
    rows = T.to_pool_rows(np.arange(len(track)))
    full = [np.arange(T.total, dtype=np.int32), np.ones(T.total, np.uint32), np.zeros(T.total, np.uint32)]
    full[0][rows] = T.to_pool_rows(track)
    full[1][rows], full[2][rows] = length, dup
    # a statistic lives at its label: the rows of a touched image that are not labels hold 0
    return full


def test_tracks(tracks):
    T = tracks
    assert len(T.ea) == 40 and T.la[1] == B // 4 + 5 and T.total == B // 4 + 3 * T.rows + 37
    want = _tracks_full(T)
    got = _tracks_expanded(T, *T.expect())
    same(got, want, "tracks")
    # the chain joins the first image to the last, and some track conflicts
    assert want[0][T.total - 37 - T.rows + len(T.touched) - 1] == 0 and want[1][0] >= len(T.touched) and (want[2] > 0).any()
    # accumulated in two calls: the same labels
    half = len(T.ea) // 2
    first = T.expect(slice(0, half))
    second = T.expect(slice(half, None), into=first[0])
    same(second, T.expect(), "accumulated")
    full_first = _tracks_full(T, slice(0, half))
    same(_tracks_expanded(T, *first), full_first, "first half")
    same(_tracks_full(T, slice(half, None), into=full_first[0]), want, "second half onto the first")
    # teeth: labels and links stored through an offset wrapped at B bytes of the int32 arrays land elsewhere
    wrapped_match = np.full(T.cap, -1, np.int32)
    for e, seg in enumerate(T.segments):
        lo = int(T.la[e]) % (B // 4)
        wrapped_match[lo:lo + len(seg)] = seg
    assert differ(tcases.build_tracks(T.image_offsets(), T.total, T.ea, T.eb, T.la, T.cap, wrapped_match), want)


# --- guided pairs over 8-bit rows ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guided_twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("guided_twin")
    return mgcases.build(d), d


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("far", ["a", "b", "both"])
def test_guided_pairs(guided_twin, far, kind):
    P = big.Pooled(B, far, SEED + 6, guide=kind)
    thr = mgcases.THRESHOLDS[kind][1]
    masks = mgcases.twin_masks(*guided_twin, P.problems(thr))
    qa, qb = P.pools["a"].to_numpy(), P.pools["b"].to_numpy()
    pairs = list(P.pairs())

    def full(qa, qb, mutual):
        """q8_guided_cases.reference over the materialised pools, call by call"""
        out = []
        for c, (oa, ob) in enumerate(P.calls):
            oa, ob = oa.astype(np.int64), ob.astype(np.int64)
            shim = SimpleNamespace(qa=qa, qb=qb, n_pairs=len(oa) - 1,
                                   pair=lambda p, oa=oa, ob=ob: (slice(oa[p], oa[p + 1]), slice(ob[p], ob[p + 1])))
            got = list(q8g.reference(shim, [m for m, q in zip(masks, pairs) if q[0] == c], big.RATIO, fill=big.SENTINEL))
            if mutual:
                got[0], got[1] = pcases.mutual(got[0], got[1], oa, ob)
            out += got
        return out

    for mutual in (False, True):
        want = full(qa, qb, mutual)
        got = []
        for e in P.expect_guided(masks, mutual=mutual):
            got += [big.expand(e[k], n) for k, n in (("ab", len(qa)), ("ba", len(qb)), ("best", len(qa)), ("second", len(qa)))]
        same(got, want, (far, kind, mutual))
        wa = big.wrapped(qa, B, 128) if far in ("a", "both") else qa
        wb = big.wrapped(qb, B, 128) if far in ("b", "both") else qb
        assert differ(full(wa, wb, mutual), want), "a wrapped pool gives the same result"
    ab = np.concatenate([v for e in P.expect_guided(masks) for _, v in e["ab"]])
    assert (ab >= 0).sum() > 15 and (ab < 0).sum() > 15
    # the keypoints of a call lie where its rows lie, and the masks admit some pairs and refuse most
    for c, (oa, ob) in enumerate(P.calls):
        assert P.kps[c]["a"][0] == oa[0] and len(P.kps[c]["a"][1]) == oa[-1] - oa[0] and len(P.kps[c]["b"][1]) == ob[-1] - ob[0]
    assert all(0 < m[0].mean() < 0.5 for m in masks)


# --- the f32 families: the expected values are oracle.match's, the builders supply rows and conditions -------------------------
def test_f32_single_pair(oracle):
    for mark in big.MARKS:                                   # the background condition, with its gap, at every mark
        S = big.SingleF32(mark, SEED + 7)
        for screen in (False, True):
            a = S.a_rows(screen)
            want, s1, s2 = oracle.match(a, S.compressed())
            S.background_below(a, s2)
            assert (S.to_rows(want) >= mark // 512).any() and (want >= 0).mean() > 0.5
        assert len(S.a_rows(True)) == big.SCREEN_ROWS and len(np.unique(S.a_rows(True), axis=0)) == big.NA_BIG_B
    S = big.SingleF32(B, SEED + 7)
    full, a = S.pool.to_numpy(), S.a_rows(False)
    want = oracle.match(a, full)
    got = oracle.match(a, S.compressed())
    assert np.array_equal(S.to_rows(got[0]), want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    tie = np.flatnonzero(want[1] == want[2])
    assert len(tie) >= 4
    assert differ(oracle.match(a, big.wrapped(full, B, 512)), want)
    # big a: the planted rows and ONE background row stand for the pool
    got = oracle.match(S.big_a_rows(), S.small_b)
    want = oracle.match(full, S.small_b)
    for g, w in zip(got, want):
        x = np.empty(S.total, g.dtype)
        x[:] = g[-1]
        x[S.crit] = g[:-1]
        assert np.array_equal(x, w)
    assert differ(oracle.match(big.wrapped(full, B, 512), S.small_b), want)


@pytest.mark.parametrize("far", ["a", "b", "both"])
def test_f32_pairs(oracle, far):
    P = big.Pooled(B, far, SEED + 8, f32=True)
    fa, fb = P.pools["a"].to_numpy(), P.pools["b"].to_numpy()
    wa = big.wrapped(fa, B, 512) if far in ("a", "both") else fa
    wb = big.wrapped(fb, B, 512) if far in ("b", "both") else fb
    accepted, changed = 0, False
    for c, p, a0, x, b0, y in P.pairs():
        assert np.array_equal(fa[a0:a0 + len(x)], x) and np.array_equal(fb[b0:b0 + len(y)], y)
        want = oracle.match(x, y)
        accepted += int((want[0] >= 0).sum())
        changed |= differ(oracle.match(wa[a0:a0 + len(x)], wb[b0:b0 + len(y)]), want)
    assert accepted > 20 and changed
    assert max(int(oa[-1]) * 512 for oa, _ in P.calls) > B or far == "b"


@pytest.mark.parametrize("kind", [0, 1])
def test_verifier_pool(kind):
    V = big.Verify(B, kind, SEED + 9)
    assert V.total * 20 > B and len(V.calls) == 6
    starts = [int(c["oa"][k]) for c in V.calls for k in range(len(c["oa"]) - 1)]
    for m in big.marks(B):
        assert m // 20 in starts and any(int(c["oa"][-1]) == m // 20 + big.SIZES["a"][1] for c in V.calls)
        assert any(c["oa"][0] < m // 20 < c["oa"][-1] and len(c["oa"]) == 2 for c in V.calls)
    for c in V.calls:
        oa, ob = c["oa"], c["ob"]
        assert np.array_equal(np.diff(oa), np.diff(ob)) and (ob[-1] <= oa[0] or oa[-1] <= ob[0]) and 0 <= ob[0] and ob[-1] <= V.total
        pool = np.full((V.total, 5), np.nan, np.float32)
        pool[oa[0]:oa[-1]], pool[ob[0]:ob[-1]] = c["ka"], c["kb"]
        for p, (ka, kb, match) in enumerate(c["pairs"]):
            assert np.array_equal(pool[oa[p]:oa[p + 1]], ka) and np.array_equal(pool[ob[p]:ob[p + 1]], kb)
            assert np.array_equal(c["match"][oa[p] - oa[0]:oa[p + 1] - oa[0]], match)
            assert (match >= 0).sum() == len(match) - 3 and np.array_equal(np.sort(match[match >= 0]), np.setdiff1d(np.arange(len(kb)), np.setdiff1d(np.arange(len(kb)), match)))
        if oa[-1] * 20 > B:                                     # a wrapped address reads other rows: NaN here
            w = big.wrapped(pool, B, 20)
            assert not np.array_equal(w[oa[0]:oa[-1]], pool[oa[0]:oa[-1]], equal_nan=True)
