"""Grouped matching over 8-bit descriptors on the GPU (include/lf_mkd.h, lf_mkd_match_q8_grouped_device,
lf_mkd_vote_groups_device) against its numpy restatement (tests/q8_grouped_cases.py): every comparison is ==, there are no
tolerances.  Then the Python faces and, end to end on photographs, the retrieval example's --exact mode."""
import os
import sys

import numpy as np
import pytest

import q8_cases as cases
import q8_grouped_cases as gcases
import q8_knn_cases as kcases
from conftest import GOLDEN, ROOT, _report

import local_features_python as lfp

pytestmark = pytest.mark.gpu

GUARD = 8              # sentinel words in front of and behind every output
SENTINEL = 0x7F0F0F0F  # above every sum (|s| <= 2 064 512), every index and every count of these tests
M = int(cases.INT32_MIN)
NAMES = ("match", "best", "rival")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def references():
    """{(na, nb, seed): (qa, qb, groups, (match, best, rival) at RATIO)}: computed once, never changed"""
    out = {}
    for na, nb, seed in gcases.shape_cases():
        qa, qb = cases.quantized_sets(na, nb, seed)
        groups = gcases.groups_for(nb, seed)
        out[(na, nb, seed)] = (qa, qb, groups, gcases.match_q8_grouped(qa, qb, groups, cases.RATIO))
    return out


class Out:
    """match / best / rival [na] on the device, each between GUARD sentinel words"""

    def __init__(self, torch, na, scores=True):
        self.n = na
        self.bufs = [torch.full((na + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3 if scores else 1)]

    def ptr(self, j):
        return self.bufs[j].data_ptr() + 4 * GUARD if j < len(self.bufs) else None

    def result(self):
        """the outputs as numpy arrays, after checking that the guard words are untouched and every entry was written"""
        got = []
        for b in self.bufs:
            h = b.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.n:] == SENTINEL).all()
            got.append(h[GUARD:GUARD + self.n].copy())
            assert (got[-1] != SENTINEL).all()       # exactly na entries: none was left out
        return got


def words(torch, x):
    """uint32 values on the device (as their int32 bit patterns)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint32)).view(np.int32)).cuda()


def run(handle, torch, qa, qb, groups, ratio=float(cases.RATIO), lo=None, hi=None, scores=True, stream=None, out=None, dev=None):
    """lf_mkd_match_q8_grouped_device on numpy rows -> [match, best, rival] (or [match])"""
    d_a, d_b, d_g = dev if dev is not None else (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), words(torch, groups))
    d_lo = words(torch, lo) if lo is not None else None
    d_hi = words(torch, hi) if hi is not None else None
    out = out or Out(torch, len(qa), scores)
    torch.cuda.synchronize()
    handle.match_q8_grouped_device(d_a.data_ptr(), len(qa), d_b.data_ptr(), len(qb), d_g.data_ptr(), out.ptr(0), ratio,
                                   d_lo.data_ptr() if lo is not None else None, d_hi.data_ptr() if hi is not None else None,
                                   out.ptr(1), out.ptr(2), stream)
    torch.cuda.synchronize()
    return out.result()


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert (w != SENTINEL).all(), (what, name, "the sentinel occurs in the expected output")
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[g != w][:5], w[g != w][:5])


@pytest.mark.parametrize("case", gcases.shape_cases(), ids=lambda c: f"{c[0]}x{c[1]}")
def test_grouped_equals_the_restatement(handle, torch, references, case):
    qa, qb, groups, want = references[case]
    same(run(handle, torch, qa, qb, groups), want, case)
    assert np.array_equal(run(handle, torch, qa, qb, groups, scores=False)[0], want[0])          # d_best = d_rival = NULL
    # a ratio at which the planted matches of these sets divide into accepted and rejected, and ratio 0
    for ratio in (0.27, 0.0):
        w = gcases.match_q8_grouped(qa, qb, groups, ratio)
        if case[:2] == (2000, 2000) and ratio:
            assert 0 < (w[0] >= 0).sum() < len(qa)
        same(run(handle, torch, qa, qb, groups, ratio), w, (case, ratio))


def _smallest_split_shape():
    """block_rows + 1 rows of a (two a blocks) against the smallest b with two splits"""
    na = next(n for n in range(1, 1 << 16) if lfp.match_q8_grouped_plan(n, 1)[0] >= 2)
    nb = next(n for n in range(1, 1 << 16) if lfp.match_q8_grouped_plan(na, n)[1] >= 2)
    return na, nb


def test_two_blocks_and_two_splits(handle, torch):
    na, nb = _smallest_split_shape()
    a_blocks, splits, scratch = lfp.match_q8_grouped_plan(na, nb)
    assert nb == 129 and a_blocks >= 2 and splits >= 2 and scratch > 0
    assert lfp.match_q8_grouped_plan(na - 1, nb)[0] < 2 and lfp.match_q8_grouped_plan(na, nb - 1)[1] < 2
    qa, qb = cases.quantized_sets(na, nb, 4200)
    groups = gcases.runs(nb, 5)
    lo, hi = cases.random_ranges(na, nb, 4201)
    for ratio in (float(cases.RATIO), 0.27):
        same(run(handle, torch, qa, qb, groups, ratio), gcases.match_q8_grouped(qa, qb, groups, ratio), (na, nb, ratio))
        same(run(handle, torch, qa, qb, groups, ratio, lo, hi), gcases.match_q8_grouped(qa, qb, groups, ratio, lo, hi),
             (na, nb, ratio, "ranges"))


def test_group_layouts(handle, torch):
    na, nb = 70, 300
    qa, qb = cases.quantized_sets(na, nb, 4300)
    s = cases.similarities(qa, qb)
    dev_rows = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda())
    layouts = gcases.group_layouts(nb)
    assert {f"runs of {n}" for n in gcases.RUN_LENGTHS} <= set(layouts) and {"j % 3", "permuted labels", "0 and 0xFFFFFFFF"} <= set(layouts)
    rivals = {}
    for name, groups in layouts.items():
        for ratio in (float(cases.RATIO), 0.27):
            want = gcases.match_q8_grouped(qa, qb, groups, ratio)
            same(run(handle, torch, qa, qb, groups, ratio, dev=dev_rows + (words(torch, groups),)), want, (name, ratio))
        rivals[name] = want[2]
        assert (want[2] <= np.sort(s, axis=1)[:, -2]).all()                    # never above the second best of all rows
    # the layouts ask different questions: longer runs push the rival further down
    assert (rivals["runs of 96"] <= rivals["runs of 1"]).all() and (rivals["runs of 96"] < rivals["runs of 1"]).any()


_FILLER = {}


def _filler(nb):
    """4 random query rows, nb random rows and their similarities: made once per size"""
    if nb not in _FILLER:
        rng = np.random.default_rng(4400 + nb)
        qa, qb = rng.integers(1, 256, (4, 128)).astype(np.uint8), rng.integers(1, 256, (nb, 128)).astype(np.uint8)
        _FILLER[nb] = (qa, qb, cases.similarities(qa, qb))
    return _FILLER[nb]


def _planted(nb, base, copies, rival_at, other=None, ratio=cases.RATIO):
    """3 random rows and one planted query row (the last) against nb random rows, among which the query's exact copies lie at
    base + copies (group G) and a row of lower, known similarity -- the query with its first 48 dimensions zeroed -- at
    base + rival_at, in the filler's group of that position.  other = (offset, group): one more exact copy.  Returns the
    inputs, the restatement's answer (the filler's similarities with the planted columns recomputed) and the two planted
    similarities."""
    qa, qb, s = _filler(nb)
    qb, s = qb.copy(), s.copy()
    groups = gcases.runs(nb, 7) + np.uint32(1000)
    x = qa[3]
    near = x.copy()
    near[:48] = 128
    rows = {base + c: (x, np.uint32(0xFFFFFFFE)) for c in copies}
    rows[base + rival_at] = (near, groups[base + rival_at])
    if other is not None:
        rows[base + other[0]] = (x, np.uint32(other[1]))
    for j, (row, g) in rows.items():
        qb[j], groups[j] = row, g
    at = sorted(rows)
    s[:, at] = cases.similarities(qa, qb[at])
    want = gcases.from_similarities(s, groups, ratio)
    return qa, qb, groups, want, int(cases.similarities(x[None], x[None])[0, 0]), int(cases.similarities(x[None], near[None])[0, 0])


# distance between the rival and G's copies: the same 4-row run of a lane, the other lane half, another tile, another LDS
# stage, another split
DISTANCES = {"same run": 0, "other lane half": 4, "another tile": 32, "another stage": 128, "another split": 160}


@pytest.mark.parametrize("nb", [128, None], ids=["one split", "splits of two stages"])
def test_planted_rows(handle, torch, nb):
    if nb == 128:
        base, dist = 32, {k: v for k, v in DISTANCES.items() if v <= 32}
        assert lfp.match_q8_grouped_plan(4, nb)[1] == 1
    else:
        # The plan the handle itself uses, from THIS device's CU count.  With one a block it wants W = 2 * CUs splits (at most
        # 1024), so 4 W + 15 tiles of b make a split of 5 tiles: the scan of one split walks two LDS stages (4 + 1 tiles).
        # The planted rows start on a split's first row.  (256 CUs: nb = 66 000.)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        nb = 32 * (4 * min(2 * cus, 1024) + 15) - 16
        splits = lfp.match_q8_grouped_plan(4, nb, cus)[1]
        per = -(-((nb + 31) // 32) // splits)
        assert per == 5 and DISTANCES["another stage"] < per * 32 == DISTANCES["another split"], (cus, nb, splits, per)
        base, dist = 100 * per * 32, DISTANCES
    checked = 0
    for name, d in dist.items():
        for order in ("rival after", "rival before"):
            # G's three copies in one 4-row run, the rival d rows behind its start or in front of it
            if order == "rival after":
                copies, rival_at = (0, 1, 2), d + 3
            else:
                copies, rival_at = ((1, 2, 3), 0) if d == 0 else ((d, d + 1, d + 2), 0)
            qa, qb, groups, want, s_copy, s_near = _planted(nb, base, copies, rival_at)
            assert want[0][3] == base + copies[-1] and want[1][3] == s_copy and want[2][3] == s_near < s_copy, (name, order)
            same(run(handle, torch, qa, qb, groups), want, (name, order))
            # a copy in a DIFFERENT group at a lower index: rival == best, rejected at 0.8, accepted at ratio 0
            low = min(copies + (rival_at,)) - 1
            qa, qb, groups, want, s_copy, _ = _planted(nb, base, copies, rival_at, other=(low, 7))
            assert want[0][3] == -1 and want[1][3] == want[2][3] == s_copy, (name, order)
            same(run(handle, torch, qa, qb, groups), want, (name, order, "copy below"))
            # ... at a higher index: it becomes the best, and the old best becomes the rival
            high = max(copies + (rival_at,)) + 1 + d
            qa, qb, groups, want, s_copy, _ = _planted(nb, base, copies, rival_at, other=(high, 7), ratio=0.0)
            assert want[0][3] == base + high and want[1][3] == want[2][3] == s_copy, (name, order)
            same(run(handle, torch, qa, qb, groups, 0.0), want, (name, order, "copy above"))
            checked += 1
    assert checked == 2 * len(dist)


def test_extreme_sums(handle, torch):
    # all-255 rows against all-255 and all-1 rows are +-128 * 127^2
    qa = np.full((33, 128), 255, np.uint8)
    qa[1::2] = 1
    qb = np.full((70, 128), 1, np.uint8)
    qb[[3, 40, 69]] = 255
    groups = np.zeros(70, np.uint32)
    groups[[3, 40, 69]] = 5                                                   # the three maxima of row 0 in one group
    want = gcases.match_q8_grouped(qa, qb, groups, cases.RATIO)
    assert (want[0][0], want[1][0], want[2][0]) == (69, 2064512, -2064512)
    assert (want[0][1], want[1][1], want[2][1]) == (68, 2064512, -2064512)     # the all-1 query: the other sign
    same(run(handle, torch, qa, qb, groups), want, "extremes")
    groups[40] = 6
    want = gcases.match_q8_grouped(qa, qb, groups, cases.RATIO)
    assert (want[0][0], want[1][0], want[2][0]) == (-1, 2064512, 2064512)
    same(run(handle, torch, qa, qb, groups), want, "extremes, the maximum in two groups")
    # a negative best against a lower rival: -2064512 * 0.8 > -2064512 holds, so a row whose every sum is the minimum is
    # accepted against an equal rival
    qb[:] = 1
    want = gcases.match_q8_grouped(qa[:1], qb, gcases.runs(70, 35), cases.RATIO)
    assert (want[0][0], want[1][0], want[2][0]) == (69, -2064512, -2064512)
    same(run(handle, torch, qa[:1], qb, gcases.runs(70, 35)), want, "extremes, all negative")


def test_exclusion_ranges(handle, torch):
    na, nb, seed = 513, 1025, 4500
    qa, qb = cases.quantized_sets(na, nb, seed)
    groups = gcases.runs(nb, 41)                                               # 25 groups, sorted
    lo, hi = cases.random_ranges(na, nb, seed + 1)
    lo[4], hi[4] = 41, nb             # only group 0 is left: no rival
    lo[5], hi[5] = 1, nb              # exactly one candidate left: the first row ...
    lo[6], hi[6] = 0, nb - 1          # ... the last row
    lo[7], hi[7] = 0, nb              # none
    lo[8], hi[8] = 0, 0xFFFFFFFF      # none, a bound beyond nb
    lo[9], hi[9] = 40, 30             # an inverted range excludes nothing
    lo[10], hi[10] = 0, nb - 40       # only the last group (rows 984 ..) is left
    want = gcases.match_q8_grouped(qa, qb, groups, cases.RATIO, lo, hi)
    match, best, rival = want
    assert 0 <= match[4] < 41 and rival[4] == M and best[4] > M
    assert (match[5], rival[5]) == (0, M) and (match[6], rival[6]) == (nb - 1, M)
    assert (match[7], best[7], rival[7]) == (-1, M, M) and (match[8], best[8], rival[8]) == (-1, M, M)
    assert [w[9] for w in want] == [w[0] for w in gcases.match_q8_grouped(qa[9:10], qb, groups, cases.RATIO)]
    assert match[10] >= nb - 40 and rival[10] == M
    same(run(handle, torch, qa, qb, groups, lo=lo, hi=hi), want, "ranges")
    # own-group exclusion on a pool sorted by group: the best's whole group removed, the old rival leads
    base = gcases.match_q8_grouped(qa, qb, groups, 0.0)
    g = groups[base[0]].astype(np.int64)
    lo2, hi2 = (g * 41).astype(np.uint32), np.minimum((g + 1) * 41, nb).astype(np.uint32)
    want = gcases.match_q8_grouped(qa, qb, groups, 0.0, lo2, hi2)
    assert np.array_equal(want[1], base[2])
    same(run(handle, torch, qa, qb, groups, 0.0, lo2, hi2), want, "the best's group removed")


class MatchOut:
    def __init__(self, torch, n):
        self.bufs = [torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]


@pytest.mark.parametrize("case", [(513, 1025, 3004), (2000, 2000, 3005)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_consequences_on_the_device(handle, torch, references, case):
    qa, qb, groups, _ = references[case]
    na, nb = len(qa), len(qb)
    d_a, d_b = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
    lo, hi = cases.random_ranges(na, nb, 4600)
    for ratio in (float(cases.RATIO), 0.27):
        for ranges in ((None, None), (lo, hi)):
            # (a) group = index: every output is lf_mkd_match_q8_device's, rival == second
            m = MatchOut(torch, na)
            d_lo, d_hi = (words(torch, r) if r is not None else None for r in ranges)
            torch.cuda.synchronize()
            handle.match_q8_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, m.bufs[0].data_ptr(), ratio,
                                   d_lo.data_ptr() if d_lo is not None else None, d_hi.data_ptr() if d_hi is not None else None,
                                   m.bufs[1].data_ptr(), m.bufs[2].data_ptr())
            want = [b.cpu().numpy() for b in m.bufs]
            same(run(handle, torch, qa, qb, np.arange(nb), ratio, *ranges, dev=(d_a, d_b, words(torch, np.arange(nb)))), want,
                 (case, ratio, "group = index"))
            # (b) one group: no rival, every row with a candidate accepted at any ratio
            match, best, rival = run(handle, torch, qa, qb, np.full(nb, 77), ratio, *ranges)
            assert (rival == M).all() and np.array_equal(best, want[1]) and (match >= 0).all()
            assert np.array_equal(match, cases.match_q8(qa, qb, 0.0, *ranges)[0])
    # (c) against lf_mkd_knn_q8_device at k = 16
    k = 16
    index = torch.full((na, k), SENTINEL, dtype=torch.int32, device="cuda")
    score = torch.full((na, k), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    handle.knn_q8_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, k, index.data_ptr(), score.data_ptr())
    index, score = index.cpu().numpy(), score.cpu().numpy()
    for g in (groups, gcases.runs(nb, 400)):
        match, best, rival = run(handle, torch, qa, qb, g, 0.0)
        i0, b0, r, known = gcases.from_knn(index, score, g)
        assert np.array_equal(match, i0) and np.array_equal(best, b0) and np.array_equal(rival[known], r[known])
        assert known.any() and (rival[~known] <= score[~known, -1]).all()


def test_repeatability_stream_and_capture(handle, torch, references):
    for case in ((513, 1025, 3004), (32, 32, 3002)):                         # a merged plan and a one-split plan
        qa, qb, groups, want = references[case]
        assert (lfp.match_q8_grouped_plan(case[0], case[1])[1] == 1) == (case[0] == 32)
        # the caller's stream; two runs of one call give the same bits
        dev = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), words(torch, groups))
        s = torch.cuda.Stream()
        got = run(handle, torch, qa, qb, groups, stream=s.cuda_stream, dev=dev)
        same(got, want, (case, "stream"))
        same(run(handle, torch, qa, qb, groups, stream=s.cuda_stream, dev=dev), got, (case, "again"))
        # a warmed-up call captured in a graph (a linear chain) replays to the same bits
        out = Out(torch, len(qa))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            handle.match_q8_grouped_device(dev[0].data_ptr(), len(qa), dev[1].data_ptr(), len(qb), dev[2].data_ptr(), out.ptr(0),
                                           float(cases.RATIO), None, None, out.ptr(1), out.ptr(2),
                                           torch.cuda.current_stream().cuda_stream)
        for b in out.bufs:
            b.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(out.result(), want, (case, "replay"))
        # the host form, with and without the scores
        same(handle.match_q8_grouped(qa, qb, groups, float(cases.RATIO)), want, (case, "host form"))
    # na == 0 writes nothing
    out = Out(torch, 4)
    handle.match_q8_grouped_device(None, 0, None, 5, None, out.ptr(0), 0.8, None, None, out.ptr(1), out.ptr(2))
    assert all((b == SENTINEL).all() for b in out.bufs)


def test_the_shared_scratch_is_stream_ordered(handle, torch, references):
    """a match_q8_device call of another size between two grouped calls, same handle and stream: neither result changes"""
    qa, qb, groups, want = references[(513, 1025, 3004)]
    qa2, qb2, _, _ = references[(300, 6000, 3006)]
    want2 = cases.match_q8(qa2, qb2)
    assert lfp.match_q8_grouped_plan(513, 1025)[2] > 0 and lfp.match_q8_plan(300, 6000)[2] > 0
    dev = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), words(torch, groups))
    dev2 = (torch.from_numpy(qa2).cuda(), torch.from_numpy(qb2).cuda())
    first_out, second_out = Out(torch, len(qa)), Out(torch, len(qa))
    m = MatchOut(torch, len(qa2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for o in (first_out, None, second_out):
        if o is None:
            handle.match_q8_device(dev2[0].data_ptr(), len(qa2), dev2[1].data_ptr(), len(qb2), m.bufs[0].data_ptr(),
                                   float(cases.RATIO), None, None, m.bufs[1].data_ptr(), m.bufs[2].data_ptr(), s.cuda_stream)
        else:
            handle.match_q8_grouped_device(dev[0].data_ptr(), len(qa), dev[1].data_ptr(), len(qb), dev[2].data_ptr(), o.ptr(0),
                                           float(cases.RATIO), None, None, o.ptr(1), o.ptr(2), s.cuda_stream)
    torch.cuda.synchronize()
    same(first_out.result(), want, "before the matcher's call")
    same(second_out.result(), want, "after the matcher's call")
    for g, w in zip((b.cpu().numpy() for b in m.bufs), want2):
        assert np.array_equal(g, w)


class Votes:
    """the vote table [n_a][n_b] on the device between GUARD sentinel words"""

    def __init__(self, torch, n_a, n_b):
        self.shape = (n_a, n_b)
        self.buf = torch.full((n_a * n_b + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")

    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def result(self):
        h = self.buf.cpu().numpy()
        n = self.shape[0] * self.shape[1]
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + n:] == SENTINEL).all()
        return h[GUARD:GUARD + n].reshape(self.shape).view(np.uint32).copy()


def test_vote_groups(handle, torch):
    rng = np.random.default_rng(4700)
    na, nb, n_a, n_b = 5000, 700, 3, 11
    match = rng.integers(0, nb, na).astype(np.int32)
    match[::7] = -1                                                           # no match
    match[3::50] = nb                                                         # out of range, just
    match[5::50] = 0x7FFFFFF0                                                 # ... by far
    match[9::50] = -2 ** 31
    ga = rng.integers(0, n_a, na).astype(np.uint32)
    ga[11::40] = n_a                                                          # a group id at the count
    ga[13::40] = 0xFFFFFFFF                                                   # ... beyond it
    gb = rng.integers(0, n_b, nb).astype(np.uint32)
    gb[::9] = n_b
    gb[4::9] = 0x80000000
    d_m, d_ga, d_gb = torch.from_numpy(match).cuda(), words(torch, ga), words(torch, gb)

    def call(n_a, n_b, d_ga, na=na, stream=None):
        v = Votes(torch, n_a, n_b)
        torch.cuda.synchronize()
        handle.vote_groups_device(d_m.data_ptr(), na, d_gb.data_ptr(), nb, n_b, v.ptr(), d_ga.data_ptr() if d_ga is not None else None,
                                  n_a, stream)
        torch.cuda.synchronize()
        return v.result()

    want = gcases.vote_groups(match, ga, n_a, gb, n_b)
    assert 0 < want.sum() < na and want.min() > 0
    assert np.array_equal(call(n_a, n_b, d_ga), want)
    want = gcases.vote_groups(match, None, 1, gb, n_b)                         # d_group_of_a = NULL: one row of the table
    assert want.shape == (1, n_b) and np.array_equal(call(1, n_b, None), want)
    assert np.array_equal(call(1, 1, d_ga), gcases.vote_groups(match, ga, 1, gb, 1))   # a 1 x 1 table
    assert np.array_equal(call(5, 20, d_ga), gcases.vote_groups(match, ga, 5, gb, 20))  # more groups than occur: zero rows
    assert np.array_equal(call(2, 3, None, na=0), np.zeros((2, 3), np.uint32))         # na == 0: the table is zeroed
    s = torch.cuda.Stream()
    assert np.array_equal(call(n_a, n_b, d_ga, stream=s.cuda_stream), gcases.vote_groups(match, ga, n_a, gb, n_b))
    # a captured replay zeroes and counts again
    v = Votes(torch, n_a, n_b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        handle.vote_groups_device(d_m.data_ptr(), na, d_gb.data_ptr(), nb, n_b, v.ptr(), d_ga.data_ptr(), n_a,
                                  torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        v.buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(v.result(), gcases.vote_groups(match, ga, n_a, gb, n_b))


def test_faces(torch, references):
    feats = lfp.LocalFeatures(64, 64, 16)
    qa, qb, groups, want = references[(33, 65, 3003)]
    m = feats.match_q8_grouped(qa, qb, groups)                                # numpy in, numpy out: the host form
    assert isinstance(m, np.ndarray) and m.dtype == np.int32 and np.array_equal(m, want[0])
    got = feats.match_q8_grouped(qa, qb, groups, scores=True)
    assert all(isinstance(g, np.ndarray) and g.dtype == np.int32 for g in got)
    same(got, want, "numpy")
    d = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), words(torch, groups))
    t = feats.match_q8_grouped(*d, scores=True)                               # device in, device out
    assert all(x.is_cuda and x.dtype == torch.int32 and x.shape == (33,) for x in t)
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in t], want, "device")
    s = torch.cuda.Stream()
    t_m = feats.match_q8_grouped(*d, ratio=0.27, stream=s)
    s.synchronize()
    assert np.array_equal(t_m.cpu().numpy(), gcases.match_q8_grouped(qa, qb, groups, 0.27)[0])
    lo, hi = np.zeros(33, np.uint32), np.full(33, 5, np.uint32)
    same(feats.match_q8_grouped(qa, qb, groups, exclude=(lo, hi), scores=True),
         gcases.match_q8_grouped(qa, qb, groups, cases.RATIO, lo, hi), "exclude")
    m = feats.match_q8_grouped(qa[:0], qb, groups)                            # empty qa
    assert m.shape == (0,) and m.dtype == np.int32
    with pytest.raises(RuntimeError, match="one id per row"):
        feats.match_q8_grouped(qa, qb, groups[:-1])
    # vote_groups: numpy in, numpy out; device in, device out
    ga = (np.arange(33) % 2).astype(np.uint32)
    n_b = 4
    gb = (groups % np.uint32(5)).astype(np.uint32)                           # ids 0 .. 4: 4 is beyond the count
    wv = gcases.vote_groups(want[0], ga, 2, gb, n_b)
    v = feats.vote_groups(want[0], gb, n_b, ga, 2)
    assert isinstance(v, np.ndarray) and v.dtype == np.uint32 and np.array_equal(v, wv)
    assert np.array_equal(feats.vote_groups(want[0], gb, n_b), gcases.vote_groups(want[0], None, 1, gb, n_b))
    tv = feats.vote_groups(t[0], words(torch, gb), n_b, words(torch, ga), 2)
    assert tv.is_cuda and tv.dtype == torch.int32 and tv.shape == (2, n_b)
    torch.cuda.synchronize()
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), wv)


# --- end to end -------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_q8.py


def _frames():
    """the 1024 x 768 centre crop of houses.jpg and its perspective warp, as test_gpu_q8_knn.py builds them"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    hi = np.linalg.inv(H_TRUE)
    hi /= hi[2, 2]
    return [crop, crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC)]


def _main_lines(ex, capsys, argv_tail):
    capsys.readouterr()
    argv = sys.argv
    try:
        sys.argv = ["find_image.py"] + argv_tail
        assert ex.main() == 0
    finally:
        sys.argv = argv
    return capsys.readouterr().out.splitlines()


def test_find_image_exact(torch, tmp_path, capsys):
    """examples/find_image.py --exact: the crop as query against its warp and bird.jpg.  The votes are rank_images_exact
    applied to the restatement of the same quantised rows, the warp ranks first, the printed lines are checked, and the
    default mode prints what it printed before."""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import find_image as ex
    crop, warp = _frames()
    paths = [str(tmp_path / "query.png"), str(tmp_path / "warp.png"), os.path.join(GOLDEN, "bird.jpg")]
    crop.save(paths[0])
    warp.save(paths[1])
    images = [ex.load_gray(p) for p in paths]
    votes, offsets, q, pool, groups, match = ex.find_image_exact(images[0], images[1:])
    assert len(q) > 1000 and offsets[1] > 1000 and offsets[2] > offsets[1] and len(pool) == offsets[2] == len(groups)
    assert np.array_equal(groups, np.repeat([0, 1], np.diff(offsets)))
    want = gcases.match_q8_grouped(q, pool, groups, ex.RATIO)
    assert np.array_equal(match, want[0])
    assert np.array_equal(votes, ex.rank_images_exact(want[0], groups, 2))
    assert votes[0] > votes[1]                                               # the warp ranks first
    # the k = 8 rule on the same rows never counts fewer
    index, score = kcases.knn_q8(q, pool, ex.K)
    approx = ex.rank_images(index, score, offsets, ex.RATIO)
    assert (votes <= approx).all()
    _report(f"[q8 grouped] find_image --exact: the crop of houses.jpg ({len(q)} keypoints) against its warp ({int(offsets[1])}) "
            f"and bird.jpg ({int(offsets[2] - offsets[1])}): votes {votes.tolist()}; the k = 8 rule's {approx.tolist()}")
    lines = _main_lines(ex, capsys, ["--exact"] + paths)
    assert lines == [f"Query: {len(q)} keypoints against {int(offsets[2])} in 2 images",
                     f"1. {paths[1]}: {int(votes[0])} votes ({int(offsets[1])} keypoints)",
                     f"2. {paths[2]}: {int(votes[1])} votes ({int(offsets[2] - offsets[1])} keypoints)"], lines
    # the default mode is the k = 8 rule, as before
    lines = _main_lines(ex, capsys, paths)
    assert lines == [f"Query: {len(q)} keypoints against {int(offsets[2])} in 2 images",
                     f"1. {paths[1]}: {int(approx[0])} votes ({int(offsets[1])} keypoints)",
                     f"2. {paths[2]}: {int(approx[1])} votes ({int(offsets[2] - offsets[1])} keypoints)"], lines
