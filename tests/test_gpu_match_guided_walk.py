"""Guided matching on the GPU where match_small_guided_pairs' own control flow does all it can do (the walk batch of
tests/match_guided_cases.py): waves that walk three to sixteen tiles with any run of them skipped, the prefetch of the next
used tile, and y sides of more than one 4096-row keypoint chunk in either direction.  Every row is held bit for bit to the
existing matcher over its admissible rows alone, and independently to float64; the rows planted at the seam are asserted by
name; a pair alone, a second run and a captured run give the batch's bits; the mutual filter is the filter."""
import os

import numpy as np
import pytest

import match_guided_cases as cases
import match_pairs_cases as pcases
from test_gpu_match_guided import KINDS, NEG_INF, Dev, bits, direct, expected

import local_features_python as lfp

pytestmark = pytest.mark.gpu

RATIOS = (0.8, 0.0)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def masks(tmp_path_factory):
    """{(kind, thr): [(fwd [na, nb], rev [nb, na], ref)] per pair run at thr} from the host twin: computed once, never changed"""
    d = tmp_path_factory.mktemp("guided_twin_walk")
    exe = cases.build(d)
    return {(kind, thr): cases.walk_masks(exe, d, kind, thr) for kind in KINDS for thr in cases.THRESHOLDS[kind]}


@pytest.fixture(scope="module")
def dev(torch):
    return {kind: Dev(torch, kind, cases.walk_batch(kind)) for kind in KINDS}


@pytest.fixture(scope="module")
def outputs(dev, handle):
    """(kind, thr, ratio) -> (match_ab, match_ba, best, second) of the batch's pairs that are run at thr: one call each, kept"""
    kept = {}

    def get(kind, thr, ratio):
        if (kind, thr, ratio) not in kept:
            kept[(kind, thr, ratio)] = dev[kind].call(handle, thr, ratio=ratio, n_pairs=dev[kind].B.run_pairs(thr))
        return kept[(kind, thr, ratio)]
    return get


def directions(B, p, per_pair, out):
    """[(name, x, y, mask, match of the x rows, best or None, second or None)] of pair p: a -> b, then b -> a"""
    sa, sb = B.pair(p)
    fwd, rev, _ = per_pair[p]
    ab, ba, s1, s2 = out
    return [("ab", B.a[sa], B.b[sb], fwd, ab[sa], s1[sa], s2[sa]), ("ba", B.b[sb], B.a[sa], rev, ba[sb], None, None)]


def untouched(B, n, out):
    """the rows in front of the first pair and behind the last pair run (n pairs) keep their sentinels"""
    ab, ba, s1, s2 = out
    a0, a1, b0, b1 = int(B.oa[0]), int(B.oa[n]), int(B.ob[0]), int(B.ob[n])
    assert a1 < len(ab) and b1 < len(ba) and a0 > 0 and b0 > 0
    return (ab[:a0] == -7).all() and (ab[a1:] == -7).all() and (ba[:b0] == -7).all() and (ba[b1:] == -7).all() \
        and np.isnan(s1[:a0]).all() and np.isnan(s1[a1:]).all() and np.isnan(s2[:a0]).all() and np.isnan(s2[a1:]).all() \
        and (ab[a0:a1] != -7).all() and (ba[b0:b1] != -7).all() and not np.isnan(s1[a0:a1]).any() and not np.isnan(s2[a0:a1]).any()


def test_every_row_against_the_existing_matcher_bit_for_bit(dev, masks, outputs, handle, torch):
    """Both kinds, the thresholds each pair is run at, ratio 0.8 and 0, every row of every pair in both directions: match (and, a
    -> b, best and second) equal lf_mkd_match_pairs_device's over the row's admissible rows alone; about 150 rows per (kind,
    threshold) are held to lf_mkd_match_device itself.  Rows of no pair, and of the pairs a call leaves out, keep their
    sentinels."""
    assert "LF_MKD_MATCH" not in os.environ
    for kind in KINDS:
        B = dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            n = B.run_pairs(thr)
            calls = 0
            for ratio in RATIOS:
                out = outputs(kind, thr, ratio)
                assert untouched(B, n, out), (kind, thr, ratio)
                tally = {"none": 0, "one": 0, "many": 0, "accepted": 0}
                todo = []
                for p in range(n):
                    for name, x, y, mask, got, g1, g2 in directions(B, p, masks[(kind, thr)], out):
                        want, w1, w2, cand = expected(handle, torch, x, y, mask, ratio)
                        assert np.array_equal(got, want), (kind, thr, ratio, p, name, np.flatnonzero(got != want)[:8])
                        if g1 is not None:
                            assert np.array_equal(bits(g1), bits(w1)) and np.array_equal(bits(g2), bits(w2)), \
                                (kind, thr, ratio, p, np.flatnonzero(bits(g1) != bits(w1))[:8], np.flatnonzero(bits(g2) != bits(w2))[:8])
                        n_c = np.array([len(c) for c in cand], np.int64)
                        tally["none"] += int((n_c == 0).sum())
                        tally["one"] += int((n_c == 1).sum())
                        tally["many"] += int((n_c >= 2).sum())
                        tally["accepted"] += int((got >= 0).sum())
                        todo += [(name, x[i], y[cand[i]], cand[i], int(got[i]), None if g1 is None else g1[i], None if g1 is None else g2[i])
                                 for i in np.flatnonzero(n_c >= 2)[::7]]
                for name, row, rows, cand, got, g1, g2 in todo[::max(1, len(todo) // 75)][:75]:
                    m, w1, w2 = direct(handle, torch, row, rows, ratio)
                    calls += 1
                    assert got == (cand[m] if m >= 0 else -1), (kind, thr, ratio, name)
                    if g1 is not None:
                        assert bits(g1) == bits(np.float32(w1)) and bits(g2) == bits(np.float32(w2)), (kind, thr, ratio)
                print(f"[match_guided_walk] kind {kind} thr {thr} ratio {ratio}: {n} pairs, rows with no / one / several candidates "
                      f"{tally['none']} / {tally['one']} / {tally['many']}, accepted {tally['accepted']}")
                assert tally["none"] and tally["one"] and tally["many"] and tally["accepted"]
            assert 100 <= calls <= 150, calls


@pytest.fixture(scope="module")
def top2_f64(dev, masks):
    """(kind, thr) -> per pair run, per direction: (candidates per row, best index, best, second) from float64 dot products over
    the twin's admissible rows, the later index first among equals; -1 / -inf where there is no such row"""
    kept = {}

    def get(kind, thr):
        if (kind, thr) in kept:
            return kept[(kind, thr)]
        B, res = dev[kind].B, []
        for p in range(B.run_pairs(thr)):
            per_dir = []
            for rev in (False, True):
                x, y = (v.astype(np.float64) for v in B.sides(p, rev))
                mask = masks[(kind, thr)][p][1 if rev else 0]
                n_c, idx = mask.sum(axis=1), np.full(len(x), -1, np.int64)
                best, second = np.full(len(x), -np.inf), np.full(len(x), -np.inf)
                for i in np.flatnonzero(n_c):
                    cand = np.flatnonzero(mask[i])
                    s = (y[cand] * x[i]).sum(axis=1)          # (row by row: equal rows of y give equal sums, which BLAS does not promise)
                    order = np.lexsort((-cand, -s))
                    idx[i], best[i] = cand[order[0]], s[order[0]]
                    if len(cand) > 1:
                        second[i] = s[order[1]]
                per_dir.append((n_c, idx, best, second))
            res.append(per_dir)
        kept[(kind, thr)] = res
        return res
    return get


def test_every_row_against_float64(dev, outputs, top2_f64):
    """The same calls against best and second from float64 dot products over the twin's admissible rows, under the rule of
    tests/test_gpu_match.py for the three-term forms on unit rows (match_pairs_cases.compare): scores within 2e-6, a differing
    decision only at a near-tie of that size.  A row with one candidate: that candidate, its score within 2e-6, second -inf."""
    differing = rows = 0
    for kind in KINDS:
        B = dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            ref = top2_f64(kind, thr)
            for ratio in RATIOS:
                ab, ba, s1, s2 = outputs(kind, thr, ratio)
                for p in range(B.run_pairs(thr)):
                    sa, sb = B.pair(p)
                    for rev, got, g1, g2 in ((False, ab[sa], s1[sa], s2[sa]), (True, ba[sb], None, None)):
                        n_c, idx, best, second = ref[p][rev]
                        what = (kind, thr, ratio, p, rev)
                        none, one, many = n_c == 0, n_c == 1, n_c >= 2
                        assert (got[none] == -1).all() and np.array_equal(got[one], idx[one]), what
                        want = (idx if ratio <= 0 else np.where(best * ratio > second, idx, -1)).astype(np.int32)
                        if g1 is not None:
                            assert (g1[none] == NEG_INF).all() and (g2[none] == NEG_INF).all() and (g2[one] == NEG_INF).all(), what
                            assert np.abs(g1[one] - best[one]).max(initial=0.0) < 2e-6, what
                            differing += pcases.compare(got[many], g1[many], g2[many], want[many], best[many], second[many], ratio, what)
                        else:
                            differing += pcases.compare(got[many], None, None, want[many], best[many], second[many], ratio, what)
                        rows += len(got)
    print(f"[match_guided_walk] float64: {rows} rows, {differing} decisions differ at a near-tie")


def test_the_rows_planted_at_the_seam(dev, outputs, handle, torch):
    """Pairs 3 (x = a) and 5 (x = b), both kinds and thresholds: the duplicates -- one descriptor and keypoint below row 4096 and
    one above -- give the higher index with best == second in bits (ratio 0) and are therefore refused at ratio 0.8; a row
    whose only admissible rows lie in the second chunk is matched to its planted row; a row whose best and second lie on
    different sides of the seam reports the best's index, and the scores of exactly those two rows."""
    checked = 0
    for kind in KINDS:
        B = dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            for p, S in cases.SEAMS.items():
                plants, rev = S["plants"], S["rev"]
                if not plants:
                    continue
                x, y = B.sides(p, rev)
                sa, sb = B.pair(p)
                out = {r: outputs(kind, thr, r) for r in RATIOS}
                got = {r: (out[r][1][sb] if rev else out[r][0][sa]) for r in RATIOS}
                s1, s2 = (None, None) if rev else (out[0.0][2][sa], out[0.0][3][sa])
                what = (kind, thr, p)
                if "dup" in plants:
                    rows, j0, j1 = plants["dup"]
                    for i in rows:
                        assert got[0.0][i] == j1 > j0 and got[0.8][i] == -1, what + (i, got[0.0][i], got[0.8][i])
                        if s1 is not None:
                            assert bits(s1[i]) == bits(s2[i]) and s1[i] > 0.9, what + (i, s1[i], s2[i])
                        checked += 1
                for name in ("b0s1", "b1s0"):
                    for i, jb, js in plants.get(name, []):
                        assert got[0.0][i] == jb and got[0.8][i] == jb and (jb < cases.CHUNK) == (name == "b0s1") \
                            and (js < cases.CHUNK) != (jb < cases.CHUNK), what + (name, i, got[0.0][i])
                        if s1 is not None:                                  # best and second are those of the two planted rows
                            m, w1, w2 = direct(handle, torch, x[i], y[[jb, js]], 0.0)
                            assert m == 0 and bits(s1[i]) == bits(np.float32(w1)) and bits(s2[i]) == bits(np.float32(w2)), what + (name, i)
                        checked += 1
                for i, j in plants.get("only1", []):
                    assert got[0.0][i] == j >= cases.CHUNK and got[0.8][i] == j, what + (i, got[0.0][i], got[0.8][i])
                    checked += 1
    assert checked == 4 * (2 * 12 + 1), checked


def same(x, y):
    return all(np.array_equal(bits(u) if u.dtype == np.float32 else u, bits(v) if v.dtype == np.float32 else v) for u, v in zip(x, y))


def test_a_pair_alone_a_second_run_and_a_captured_run_give_the_same_bits(dev, outputs, handle, torch):
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][0 if kind == cases.FUNDAMENTAL else 1]     # a threshold every pair is run at
        assert B.run_pairs(thr) == B.n_pairs
        ab, ba, s1, s2 = whole = outputs(kind, thr, 0.8)
        for p in range(B.n_pairs):                                          # n_pairs = 1, the pair's two offsets, its model
            off = (D.oa[p:p + 2].clone(), D.ob[p:p + 2].clone())
            out = D.call(handle, thr, offsets=off, n_pairs=1, model=D.model[p:p + 1].clone())
            sa, sb = B.pair(p)
            assert np.array_equal(out[0][sa], ab[sa]) and np.array_equal(out[1][sb], ba[sb]), (kind, p)
            assert np.array_equal(bits(out[2][sa]), bits(s1[sa])) and np.array_equal(bits(out[3][sa]), bits(s2[sa])), (kind, p)
            assert (out[0][:sa.start] == -7).all() and (out[0][sa.stop:] == -7).all() and (out[1][:sb.start] == -7).all() \
                and (out[1][sb.stop:] == -7).all() and np.isnan(out[2][:sa.start]).all() and np.isnan(out[2][sa.stop:]).all(), (kind, p)
        assert same(whole, D.call(handle, thr))                             # two runs agree
        out = D.outputs()                                                   # a captured call replays to the same bits
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            D.run(handle, out, thr, stream=torch.cuda.current_stream().cuda_stream)
        for v, fill in zip(out, (-7, -7, np.nan, np.nan)):
            v.fill_(fill)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(whole, [v.cpu().numpy() for v in out])


def test_mutual_is_the_filter_of_the_unfiltered_outputs(dev, outputs, handle):
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            n = B.run_pairs(thr)
            ab0, ba0, s1_0, s2_0 = outputs(kind, thr, 0.8)
            ab, ba, s1, s2 = D.call(handle, thr, flags=lfp.MATCH_MUTUAL, n_pairs=n)
            want_ab, want_ba = pcases.mutual(ab0, ba0, B.oa[:n + 1], B.ob[:n + 1])
            assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba), (kind, thr)
            assert np.array_equal(bits(s1), bits(s1_0)) and np.array_equal(bits(s2), bits(s2_0))     # best / second are not filtered
            kept, fwd = int((ab[B.oa[0]:B.oa[n]] >= 0).sum()), int((ab0[B.oa[0]:B.oa[n]] >= 0).sum())
            print(f"[match_guided_walk] kind {kind} thr {thr}: {fwd} forward matches, {kept} mutual")
            assert 0 < kept <= fwd
