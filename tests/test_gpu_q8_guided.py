"""Guided matching over 8-bit rows on the GPU (lf_mkd_match_q8_guided_pairs_device, LocalFeatures.match_q8_guided_batch): every
row of a ragged batch equal to the integer reference over the host twin's masks (tests/q8_guided_cases.py); everything
admissible equals the unguided q8 call; nothing admissible; the mutual filter; one admissibility relation with the f32 guided
call; shape independence and capture; offsets beyond the totals; the superset property; the Python faces; the example.  Every
comparison is ==: integer sums, ties by index."""
import os
import sys

import numpy as np
import pytest

import match_guided_cases as gcases
import match_pairs_cases as pcases
import q8_cases as qcases
import q8_guided_cases as cases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

KINDS = cases.KINDS
INT32_MIN = cases.INT32_MIN
FILL = cases.SENTINEL


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
    """{(kind, thr): [(fwd [na, nb], rev [nb, na], ref)] per pair} from the host twin: computed once, never changed"""
    d = tmp_path_factory.mktemp("q8_guided_twin")
    return cases.all_masks(gcases.build(d), d)


@pytest.fixture(scope="module")
def refs(masks):
    """{(kind, thr, ratio): (match_ab, match_ba, best, second)} without the mutual filter: computed once, read-only"""
    out = {}
    for (kind, thr), m in masks.items():
        for ratio in (0.8, 0.0):
            out[(kind, thr, ratio)] = cases.reference(cases.batch(kind), m, np.float32(ratio))
            for arr in out[(kind, thr, ratio)]:
                arr.setflags(write=False)
    return out


class Dev:
    """cases.batch(kind) on the device, and outputs pre-filled with the sentinel."""

    def __init__(self, torch, kind):
        self.B = B = cases.batch(kind)
        self.kind, self.torch = kind, torch
        up = lambda x: torch.from_numpy(np.array(x)).cuda()                  # (a copy: the batch's arrays are read-only)
        self.qa, self.qb, self.ka, self.kb = up(B.qa), up(B.qb), up(B.ka), up(B.kb)
        self.a, self.b = up(B.a), up(B.b)                                   # the f32 rows the bytes were quantised from
        self.oa, self.ob, self.model = up(B.oa), up(B.ob), up(B.model)

    def outputs(self):
        t, B = self.torch, self.B
        new = lambda n: t.full((n,), FILL, dtype=t.int32, device="cuda")
        return new(len(B.qa)), new(len(B.qb)), new(len(B.qa)), new(len(B.qa))

    def run(self, handle, out, thr, ratio=0.8, flags=0, stream=None, offsets=None, n_pairs=None, model=None, totals=None,
            both=True, scores=True, kind=None, ka=None):
        ab, ba, s1, s2 = out
        oa, ob = offsets if offsets is not None else (self.oa, self.ob)
        na, nb = totals if totals is not None else (len(self.B.qa), len(self.B.qb))
        handle.match_q8_guided_pairs_device(self.qa.data_ptr(), (self.ka if ka is None else ka).data_ptr(), oa.data_ptr(), na,
                                            self.qb.data_ptr(), self.kb.data_ptr(), ob.data_ptr(), nb,
                                            (self.model if model is None else model).data_ptr(),
                                            self.B.n_pairs if n_pairs is None else n_pairs, ab.data_ptr(),
                                            ba.data_ptr() if both else None, self.kind if kind is None else kind, thr, ratio, flags,
                                            s1.data_ptr() if scores else None, s2.data_ptr() if scores else None, stream)

    def call(self, handle, thr, **kw):
        out = self.outputs()
        self.run(handle, out, thr, stream=self.torch.cuda.current_stream().cuda_stream, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]


@pytest.fixture(scope="module")
def dev(torch):
    return {kind: Dev(torch, kind) for kind in KINDS}


def same(x, y):
    return all(np.array_equal(u, v) for u, v in zip(x, y))


# --- 1 ------------------------------------------------------------------------------------------------------------------
def test_every_row_equals_the_masked_integer_reference(dev, refs, handle):
    """Both kinds, both thresholds, ratio 0.8 and 0, with and without LF_MKD_MATCH_MUTUAL, both directions and one: match, best
    and second of every row of every pair; rows outside the pairs keep the sentinel."""
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            for ratio in (0.8, 0.0):
                want = refs[(kind, thr, ratio)]
                got = D.call(handle, thr, ratio=ratio)
                for name, g, w in zip(("match_ab", "match_ba", "best", "second"), got, want):
                    bad = np.flatnonzero(g != w)
                    assert len(bad) == 0, (kind, thr, ratio, name, bad[:8], g[bad[:8]], w[bad[:8]])
                ia = slice(int(B.oa[0]), int(B.oa[-1]))
                n_none, n_one = int((got[2][ia] == INT32_MIN).sum()), int(((got[3][ia] == INT32_MIN) & (got[2][ia] != INT32_MIN)).sum())
                print(f"[q8_guided] kind {kind} thr {thr} ratio {ratio}: {int((got[0][ia] >= 0).sum())} of {ia.stop - ia.start} a rows "
                      f"accepted, {n_none} without a candidate, {n_one} with one")
                assert n_none and n_one and (got[0][ia] >= 0).any() and (got[0][ia] == -1).any()
                m_ab, m_ba = pcases.mutual(want[0], want[1], B.oa, B.ob)
                got = D.call(handle, thr, ratio=ratio, flags=lfp.MATCH_MUTUAL)
                assert same(got, (m_ab, m_ba, want[2], want[3])), (kind, thr, ratio, "mutual")
                one_way = D.call(handle, thr, ratio=ratio, both=False, scores=False)     # what is not asked for is not written
                assert np.array_equal(one_way[0], want[0]) and all((x == FILL).all() for x in one_way[1:]), (kind, thr, ratio)


# --- 2 ------------------------------------------------------------------------------------------------------------------
def test_everything_admissible_equals_the_unguided_call(dev, handle, torch):
    """H = identity at 1e4 px: every pair of points is admissible, and every pair with ny >= 2 gives exactly
    lf_mkd_match_q8_pairs_device's outputs, with and without the mutual filter; a direction with ny == 1, which that call
    refuses, accepts its one candidate with second == INT32_MIN."""
    for kind in KINDS:                                                       # (the two batches' rows; the call's kind is H)
        D, B = dev[kind], dev[kind].B
        model = torch.from_numpy(np.ascontiguousarray(np.tile(np.eye(3, dtype=np.float32).reshape(9), (B.n_pairs, 1)))).cuda()
        for p in range(B.n_pairs):                                           # the premise, in float64
            sa, sb = B.pair(p)
            assert gcases.f64_residual(cases.HOMOGRAPHY, np.eye(3).reshape(9), B.ka[sa, :2], B.kb[sb, :2], 1e4)[0].all()
        ref = D.outputs()
        handle.match_q8_pairs_device(D.qa.data_ptr(), D.oa.data_ptr(), len(B.qa), D.qb.data_ptr(), D.ob.data_ptr(), len(B.qb),
                                     B.n_pairs, ref[0].data_ptr(), ref[1].data_ptr(), 0.8, 0, ref[2].data_ptr(), ref[3].data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = [x.cpu().numpy() for x in ref]
        ones = 0
        for p, (na, nb) in enumerate(cases.SIZES):
            sa, sb = B.pair(p)
            if nb == 1:
                want[0][sa], want[3][sa] = 0, INT32_MIN
                want[2][sa] = qcases.similarities(B.qa[sa], B.qb[sb])[:, 0]
                ones += 1
            if na == 1:
                want[1][sb] = 0
                ones += 1
        assert ones == 4                                                     # (1, 1) both ways, (2, 1) forward, (1, 2) back
        got = D.call(handle, 1e4, model=model, kind=cases.HOMOGRAPHY)
        assert same(got, want), kind
        m_ab, m_ba = pcases.mutual(want[0], want[1], B.oa, B.ob)
        got = D.call(handle, 1e4, model=model, kind=cases.HOMOGRAPHY, flags=lfp.MATCH_MUTUAL)
        assert same(got, (m_ab, m_ba, want[2], want[3])), kind
        mref = D.outputs()
        handle.match_q8_pairs_device(D.qa.data_ptr(), D.oa.data_ptr(), len(B.qa), D.qb.data_ptr(), D.ob.data_ptr(), len(B.qb),
                                     B.n_pairs, mref[0].data_ptr(), mref[1].data_ptr(), 0.8, lfp.MATCH_MUTUAL, None, None,
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for p, (na, nb) in enumerate(cases.SIZES):                            # where the unguided call refuses nothing: its own filter
            if na >= 2 and nb >= 2:
                sa, sb = B.pair(p)
                assert np.array_equal(got[0][sa], mref[0].cpu().numpy()[sa]) and np.array_equal(got[1][sb], mref[1].cpu().numpy()[sb]), p


# --- 3 ------------------------------------------------------------------------------------------------------------------
def test_nothing_admissible(dev, refs, handle, torch):
    """All-zero models, NaN models and a NaN coordinate: -1 and INT32_MIN twice, under either kind."""
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][1]
        ia, ib = slice(int(B.oa[0]), int(B.oa[-1])), slice(int(B.ob[0]), int(B.ob[-1]))
        nan_model = B.model.copy()
        nan_model[:, kind + 3] = np.nan
        for model in (np.zeros_like(B.model), nan_model):
            for flags in (0, lfp.MATCH_MUTUAL):
                got = D.call(handle, thr, ratio=0.0, flags=flags, model=torch.from_numpy(model).cuda())
                assert (got[0][ia] == -1).all() and (got[1][ib] == -1).all()
                assert (got[2][ia] == INT32_MIN).all() and (got[3][ia] == INT32_MIN).all()
                assert (got[0][:ia.start] == FILL).all() and (got[1][ib.stop:] == FILL).all()
        # the batch's own two pairs, among sound ones
        got = D.call(handle, thr)
        for p in (cases.ZERO_MODEL, cases.NAN_MODEL):
            sa, sb = B.pair(p)
            assert (got[0][sa] == -1).all() and (got[1][sb] == -1).all() and (got[2][sa] == INT32_MIN).all() and len(got[0][sa])
        # a NaN coordinate: that row has no candidate and is nobody's candidate; every other row of the a side is as it was
        ka = B.ka.copy()
        row = int(B.oa[0]) + 2
        ka[row, 0] = np.nan
        got = D.call(handle, thr, ratio=0.0, ka=torch.from_numpy(ka).cuda())
        want = refs[(kind, thr, 0.0)]
        assert got[0][row] == -1 and got[2][row] == INT32_MIN and got[3][row] == INT32_MIN
        assert not (got[1][B.pair(0)[1]] == 2).any() and (want[1][B.pair(0)[1]] == 2).any()
        keep = np.arange(len(got[0])) != row
        assert np.array_equal(got[0][keep], want[0][keep]) and np.array_equal(got[2][keep], want[2][keep])


# --- 4 ------------------------------------------------------------------------------------------------------------------
def test_mutual_is_the_filter_of_the_unfiltered_outputs(dev, handle):
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            ab0, ba0, s1_0, s2_0 = D.call(handle, thr)
            ab, ba, s1, s2 = D.call(handle, thr, flags=lfp.MATCH_MUTUAL)
            want_ab, want_ba = pcases.mutual(ab0, ba0, B.oa, B.ob)
            assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba), (kind, thr)
            assert np.array_equal(s1, s1_0) and np.array_equal(s2, s2_0)     # best / second are not filtered
            kept, fwd = int((ab[B.oa[0]:B.oa[-1]] >= 0).sum()), int((ab0[B.oa[0]:B.oa[-1]] >= 0).sum())
            print(f"[q8_guided] kind {kind} thr {thr}: {fwd} forward matches, {kept} mutual")
            assert 0 < kept < fwd
    with pytest.raises(RuntimeError, match="match_q8_guided_pairs_device: LF_MKD_MATCH_MUTUAL needs d_match_ba"):
        D.run(handle, D.outputs(), 3.0, flags=lfp.MATCH_MUTUAL, both=False)


# --- 5 ------------------------------------------------------------------------------------------------------------------
def test_one_admissibility_relation_with_the_f32_guided_call(dev, handle, torch):
    """The same keypoints, model and threshold through lf_mkd_match_guided_pairs_device on the f32 rows: a row has no candidate
    here (best == INT32_MIN; at ratio 0, match == -1) exactly where it has none there (best == -inf; match == -1)."""
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            got = D.call(handle, thr, ratio=0.0)
            ab = torch.full((len(B.a),), FILL, dtype=torch.int32, device="cuda")
            ba = torch.full((len(B.b),), FILL, dtype=torch.int32, device="cuda")
            s1 = torch.full((len(B.a),), np.nan, device="cuda")
            handle.match_guided_pairs_device(D.a.data_ptr(), D.ka.data_ptr(), D.oa.data_ptr(), len(B.a), D.b.data_ptr(),
                                             D.kb.data_ptr(), D.ob.data_ptr(), len(B.b), D.model.data_ptr(), B.n_pairs, ab.data_ptr(),
                                             ba.data_ptr(), kind, thr, 0.0, 0, s1.data_ptr(), None,
                                             torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ab, ba, s1 = ab.cpu().numpy(), ba.cpu().numpy(), s1.cpu().numpy()
            ia, ib = slice(int(B.oa[0]), int(B.oa[-1])), slice(int(B.ob[0]), int(B.ob[-1]))
            assert np.array_equal(got[2][ia] == INT32_MIN, s1[ia] == -np.inf), (kind, thr)
            assert np.array_equal(got[0][ia] == -1, ab[ia] == -1) and np.array_equal(got[1][ib] == -1, ba[ib] == -1), (kind, thr)
            assert (got[0][ia] == -1).any() and (got[1][ib] == -1).any() and (got[0][ia] >= 0).any()


# --- 6 ------------------------------------------------------------------------------------------------------------------
def test_shape_independent_repeatable_and_capturable(dev, handle, torch):
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][0]
        whole = D.call(handle, thr)
        ab, ba, s1, s2 = whole
        assert (ab[:B.oa[0]] == FILL).all() and (ab[B.oa[-1]:] == FILL).all() and (ba[:B.ob[0]] == FILL).all() and (ba[B.ob[-1]:] == FILL).all()
        assert (ab[B.oa[0]:B.oa[-1]] != FILL).all() and (ba[B.ob[0]:B.ob[-1]] != FILL).all()
        assert (s1[:B.oa[0]] == FILL).all() and (s2[B.oa[-1]:] == FILL).all() and (s1[B.oa[0]:B.oa[-1]] != FILL).all()
        # pair p alone (n_pairs = 1, its two offsets, its model) equals pair p of the batch
        for p in range(B.n_pairs):
            off = (D.oa[p:p + 2].clone(), D.ob[p:p + 2].clone())
            out = D.call(handle, thr, offsets=off, n_pairs=1, model=D.model[p:p + 1].clone())
            sa, sb = B.pair(p)
            assert np.array_equal(out[0][sa], ab[sa]) and np.array_equal(out[1][sb], ba[sb]), (kind, p)
            assert np.array_equal(out[2][sa], s1[sa]) and np.array_equal(out[3][sa], s2[sa]), (kind, p)
            assert (out[0][:sa.start] == FILL).all() and (out[0][sa.stop:] == FILL).all() and (out[1][:sb.start] == FILL).all() \
                and (out[1][sb.stop:] == FILL).all(), (kind, p)
        # the first five pairs: the others' presence changes nothing
        head = D.call(handle, thr, n_pairs=5)
        ea, eb = int(B.oa[5]), int(B.ob[5])
        assert np.array_equal(head[0][:ea], ab[:ea]) and np.array_equal(head[1][:eb], ba[:eb]) and np.array_equal(head[2][:ea], s1[:ea])
        assert (head[0][ea:] == FILL).all() and (head[1][eb:] == FILL).all()
        none = D.call(handle, thr, n_pairs=0)                                         # n_pairs == 0 writes nothing
        assert all((x == FILL).all() for x in none)
        for flags in (0, lfp.MATCH_MUTUAL):
            first = D.call(handle, thr, flags=flags)
            assert same(first, D.call(handle, thr, flags=flags))                      # two runs agree
            s = torch.cuda.Stream()                                                   # a stream of the caller's
            out = D.outputs()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                D.run(handle, out, thr, flags=flags, stream=s.cuda_stream)
            s.synchronize()
            assert same(first, [x.cpu().numpy() for x in out])
            out = D.outputs()                                                         # the handle's own stream
            D.run(handle, out, thr, flags=flags, stream=None)
            assert same(first, [x.cpu().numpy() for x in out])
            out = D.outputs()                                                         # a captured call replays to the same values
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                D.run(handle, out, thr, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
            for x in out:
                x.fill_(FILL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same(first, [x.cpu().numpy() for x in out])


# --- 7 ------------------------------------------------------------------------------------------------------------------
def test_offsets_beyond_the_totals_touch_nothing(dev, handle, torch):
    """Whatever the offsets hold, no row at or beyond a total is read or written: an offset beyond the total counts as the
    total, an inverted pair as an empty one.  (The totals the call is told end inside the arrays, whose tails must keep their
    sentinels.)"""
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][1]
        na, nb = int(B.oa[2]), int(B.ob[2])                                 # pairs 0 and 1 and nothing behind them
        o = lambda v: torch.tensor(v, dtype=torch.int64).cuda()
        a0, a1, b0, b1 = int(B.oa[0]), int(B.oa[1]), int(B.ob[0]), int(B.ob[1])
        alone = D.call(handle, thr, offsets=(o([a0, a1]), o([b0, b1])), n_pairs=1, flags=lfp.MATCH_MUTUAL)
        for oa, ob in (([a0, a1, 5000], [b0, b1, nb]), ([a0, a1, na], [b0, b1, 1 << 40]), ([a0, a1, a0 + 5], [b0, b1, nb]),
                       ([1 << 33, 1 << 34, 1 << 35], [b0, b1, nb])):
            out = D.call(handle, thr, offsets=(o(oa), o(ob)), n_pairs=2, totals=(na, nb), flags=lfp.MATCH_MUTUAL)
            assert (out[0][na:] == FILL).all() and (out[1][nb:] == FILL).all() and (out[2][na:] == FILL).all() \
                and (out[3][na:] == FILL).all(), (kind, oa, ob)
            if oa[0] == a0:                                                  # pair 0 is intact: decided as alone
                assert np.array_equal(out[0][a0:a1], alone[0][a0:a1]) and np.array_equal(out[1][b0:b1], alone[1][b0:b1]), (oa, ob)
                assert np.array_equal(out[2][a0:a1], alone[2][a0:a1]) and np.array_equal(out[3][a0:a1], alone[3][a0:a1])
            else:                                                            # no a row is in range: b's rows find no candidates
                assert (out[0] == FILL).all() and (out[1][b0:nb] == -1).all() and (out[1][:b0] == FILL).all()


# --- 8 ------------------------------------------------------------------------------------------------------------------
def _scene(kind, seed, n=900, n_decoys=300, n_stray=150):
    """Two synthetic frames under one true model: n points seen in both (b = the true image of a + 0.3 px), each with a pair
    of descriptors the ratio test accepts; n_decoys further b rows that copy a b descriptor closely but lie elsewhere -- the
    unguided ratio test rejects the rows they shadow, the guided one does not see them --; n_stray unrelated rows on either
    side.  b is shuffled.  -> (a desc, a kps, b desc, b kps)"""
    rng = np.random.default_rng(seed)
    if kind == cases.HOMOGRAPHY:
        h = np.array([[0.97, 0.04, 14.0], [-0.03, 1.02, -9.0], [3e-5, -2e-5, 1.0]])
        xa = gcases._uniform(rng, n)
        xb = gcases.map_points(h, xa)
    else:
        K = np.array([[520.0, 0, gcases.W / 2], [0, 520.0, gcases.H / 2], [0, 0, 1]])
        X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2.2, 2.2, n), rng.uniform(5, 12, n)], axis=1)
        ry = 0.08
        Rm = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
        proj = lambda P: (P @ K.T)[:, :2] / (P @ K.T)[:, 2:3]
        xa, xb = proj(X), proj(X @ Rm.T + np.array([0.8, 0.1, -0.1]))
    xb = xb + rng.normal(0, 0.3, xb.shape)
    db = pcases.unit(rng.normal(size=(n, 128)))
    da = pcases.unit(db + 0.3 * pcases.unit(rng.normal(size=(n, 128))))
    shadowed = rng.permutation(n)[:n_decoys]
    d_decoy = pcases.unit(db[shadowed] + 0.15 * pcases.unit(rng.normal(size=(n_decoys, 128))))
    x_decoy = xb[shadowed] + rng.choice([-1.0, 1.0], (n_decoys, 2)) * rng.uniform(60, 200, (n_decoys, 2))
    stray = lambda: (pcases.unit(rng.normal(size=(n_stray, 128))), gcases._uniform(rng, n_stray))
    sa, sb = stray(), stray()
    da, xa = np.concatenate([da, sa[0]]), np.concatenate([xa, sa[1]])
    db, xb = np.concatenate([db, d_decoy, sb[0]]), np.concatenate([xb, x_decoy, sb[1]])
    order = rng.permutation(len(db))
    return da, gcases._keypoints(xa), db[order], gcases._keypoints(xb[order])


def test_guided_matching_never_loses_a_verified_match(torch):
    """The superset property (include/lf_mkd.h) on the device, two pairs a call: match_q8_batch(mutual), the batched verifier,
    match_q8_guided_batch with its model at its threshold and ratio -- every verified match is found again in both directions,
    and the guided pass finds more than verification kept.  Once under H, once under F."""
    feats = lfp.LocalFeatures(64, 64, 64)
    for kind, name, verify in ((cases.HOMOGRAPHY, "homography", feats.verify_homography_batch),
                               (cases.FUNDAMENTAL, "fundamental", feats.verify_fundamental_batch)):
        scenes = [_scene(kind, 900 + 10 * kind + k, n=900 - 250 * k) for k in range(2)]
        da, ka = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
        db, kb = np.concatenate([s[2] for s in scenes]), np.concatenate([s[3] for s in scenes])
        oa = torch.tensor(np.cumsum([0] + [len(s[0]) for s in scenes]))
        ob = torch.tensor(np.cumsum([0] + [len(s[2]) for s in scenes]))
        qa, qb = feats.quantize(torch.from_numpy(da)), feats.quantize(torch.from_numpy(db))
        ka, kb = torch.from_numpy(ka).cuda(), torch.from_numpy(kb).cuda()
        ab, ba, _, _ = feats.match_q8_batch(qa, oa, qb, ob, mutual=True)
        model, ver, st = verify(ka, oa, kb, ob, ab, seed=21)
        g_ab, g_ba, _, _ = feats.match_q8_guided_batch(qa, ka, oa, qb, kb, ob, model, kind=name)
        torch.cuda.synchronize()
        v, g, gb = ver.cpu().numpy(), g_ab.cpu().numpy(), g_ba.cpu().numpy()
        for p in range(2):
            sa, sb = slice(int(oa[p]), int(oa[p + 1])), slice(int(ob[p]), int(ob[p + 1]))
            i = np.flatnonzero(v[sa] >= 0)
            n_mutual, n_ver, n_guided = int((ab[sa] >= 0).sum()), len(i), int((g[sa] >= 0).sum())
            print(f"[q8_guided] synthetic pair {p} under one {name}: {n_mutual} mutual, {n_ver} verified, {n_guided} guided")
            assert n_ver >= 100
            assert np.array_equal(g[sa][i], v[sa][i]), (name, p)                  # guided_ab[i] == verified[i]
            assert np.array_equal(gb[sb][v[sa][i]], i), (name, p)                 # ... and match_ba[j] == i
            assert n_guided > n_ver, (name, p, n_guided, n_ver)


# --- 9 ------------------------------------------------------------------------------------------------------------------
def test_match_q8_guided_batch_and_match_q8_guided_faces(dev, handle, torch):
    """LocalFeatures.match_q8_guided_batch / match_q8_guided return what the C call wrote: keypoints, offsets and model of
    other dtypes and on the host are accepted, the outputs have the stated shapes and dtypes, rows outside every pair read
    -1 / INT32_MIN, and the single-pair form equals pair 0 of the batch."""
    feats = lfp.LocalFeatures(64, 64, 64)
    host = lambda x: torch.from_numpy(np.array(x))                            # (a copy: the batch's arrays are read-only)
    for kind, name in zip(KINDS, ("homography", "fundamental")):
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][0]                                       # the verifiers' own: the default
        want = D.call(handle, thr, flags=lfp.MATCH_MUTUAL)
        ab, ba, s1, s2 = feats.match_q8_guided_batch(host(B.qa), host(B.ka), host(B.oa).to(torch.int32),
                                                     D.qb, D.kb.double(), D.ob, host(B.model).reshape(-1, 3, 3), kind=name)
        torch.cuda.synchronize()
        assert ab.shape == (len(B.qa),) and ba.shape == (len(B.qb),) and s1.shape == s2.shape == (len(B.qa),)
        assert ab.dtype == ba.dtype == s1.dtype == s2.dtype == torch.int32 and ab.is_cuda and ba.is_cuda and s1.is_cuda
        ia, ib = slice(B.oa[0], B.oa[-1]), slice(B.ob[0], B.ob[-1])
        assert np.array_equal(ab.cpu().numpy()[ia], want[0][ia]) and np.array_equal(ba.cpu().numpy()[ib], want[1][ib])
        assert np.array_equal(s1.cpu().numpy()[ia], want[2][ia]) and np.array_equal(s2.cpu().numpy()[ia], want[3][ia])
        assert (ab[:B.oa[0]] == -1).all() and (ba[B.ob[-1]:] == -1).all() and (s1[:B.oa[0]] == -2 ** 31).all()
        # GUIDE_* constants, an explicit threshold, no mutual filter, a stream of the caller's; one direction gives no match_ba
        s = torch.cuda.Stream()
        thr2 = cases.THRESHOLDS[kind][1]
        plain = D.call(handle, thr2, ratio=0.0)
        ab2, ba2, _, _ = feats.match_q8_guided_batch(D.qa, D.ka, D.oa, D.qb, D.kb, D.ob, D.model, kind=kind, threshold=thr2, ratio=0.0,
                                                     mutual=False, both=True, stream=s)
        ab3, none, _, _ = feats.match_q8_guided_batch(D.qa, D.ka, D.oa, D.qb, D.kb, D.ob, D.model, kind=kind, threshold=thr2, ratio=0.0,
                                                      mutual=False, stream=s)
        s.synchronize()
        assert np.array_equal(ab2.cpu().numpy()[ia], plain[0][ia]) and np.array_equal(ba2.cpu().numpy()[ib], plain[1][ib])
        assert none is None and torch.equal(ab3, ab2)
        # one pair: all of a against all of b, equal to pair 0 of the batch
        sa, sb = B.pair(0)
        one = feats.match_q8_guided(host(B.qa[sa]), host(B.ka[sa]), D.qb[sb], D.kb[sb],
                                    host(B.model[0]).reshape(3, 3), kind=name)
        torch.cuda.synchronize()
        assert one[0].shape == (sa.stop - sa.start,) and one[1].shape == (sb.stop - sb.start,)
        assert np.array_equal(one[0].cpu().numpy(), want[0][sa]) and np.array_equal(one[1].cpu().numpy(), want[1][sb])
        assert np.array_equal(one[2].cpu().numpy(), want[2][sa]) and np.array_equal(one[3].cpu().numpy(), want[3][sa])
        # an empty side, no pairs
        e, z = torch.zeros((0, 128), dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
        ab, ba, s1, _ = feats.match_q8_guided_batch(e, torch.zeros((0, 5)), z, D.qb[:10], D.kb[:10], torch.tensor([0, 10]), D.model[:1], kind=name)
        assert ab.shape == (0,) and ba.shape == (10,) and (ba == -1).all() and s1.shape == (0,)
        with pytest.raises(RuntimeError, match="n_pairs"):
            feats.match_q8_guided_batch(D.qa, D.ka, D.oa, D.qb, D.kb, D.ob[:-1], D.model, kind=name)
        with pytest.raises(RuntimeError, match="kind"):
            feats.match_q8_guided_batch(D.qa, D.ka, D.oa, D.qb, D.kb, D.ob, D.model, kind="affine")
        with pytest.raises(RuntimeError, match="uint8"):
            feats.match_q8_guided_batch(D.a, D.ka, D.oa, D.qb, D.kb, D.ob, D.model, kind=name)


# --- 10 -----------------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_match_pairs.py::_frames, warp 0


def test_match_sequence_guided_q8_on_the_houses_crop_and_its_warp(torch):
    """examples/match_sequence.py's guided_q8 on the 1024 x 768 centre crop of houses.jpg against its warp: it runs, its
    columns are those of `guided`, guided >= verified; and q8 with guided still runs its second pass on the f32 rows -- what it
    returns is what the same public calls give when made by hand."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_sequence as ex
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    hi = np.linalg.inv(H_TRUE)
    warp = crop.transform((1024, 768), Image.PERSPECTIVE, tuple((hi / hi[2, 2]).reshape(-1)[:8]), resample=Image.BICUBIC)
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in (crop, warp)])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=2)
    seed = 21
    kps, desc, o, m_ab, ver, model, per_pair = ex.match_sequence(frames, seed=seed, feats=feats, guided_q8=True)
    torch.cuda.synchronize()
    raw, mutual, inl, guided, again = per_pair.cpu().numpy()[0]
    print(f"[q8_guided] crop -> warp, both passes on 8-bit rows: {raw} matches, {mutual} mutual, {inl} verified, {guided} guided, "
          f"{again} verified again")
    assert per_pair.shape == (1, 5) and raw >= mutual >= inl >= 8 and guided >= inl and guided >= again >= inl
    n0 = int(o[1])
    assert int((m_ab[:n0] >= 0).sum()) == guided and int((ver[:n0] >= 0).sum()) == again and (m_ab[n0:] == -1).all()
    # (the verifiers write the pairs' a rows only: the last frame's rows of `ver` are not compared)
    # by hand: quantise once, match_q8_batch, verify, match_q8_guided_batch, verify with the same seed
    oa, ob = o[:2], o[1:]
    q = feats.quantize(desc)
    ab1, _, _, _ = feats.match_q8_batch(q, oa, q, ob, mutual=True)
    model1, ver1, _ = feats.verify_homography_batch(kps, oa, kps, ob, ab1, seed=seed)
    ab2, _, _, _ = feats.match_q8_guided_batch(q, kps, oa, q, kps, ob, model1)
    model2, ver2, _ = feats.verify_homography_batch(kps, oa, kps, ob, ab2, seed=seed)
    assert torch.equal(ab2, m_ab) and torch.equal(ver2[:n0], ver[:n0]) and torch.equal(model2.view(torch.int32), model.view(torch.int32))
    v1 = ver1.cpu().numpy()[:n0]
    i = np.flatnonzero(v1 >= 0)
    assert np.array_equal(ab2.cpu().numpy()[:n0][i], v1[i])                        # no verified match is lost
    # q8 with guided: the second pass on f32, as before
    _, _, o_b, m_b, ver_b, model_b, per_b = ex.match_sequence(frames, seed=seed, feats=feats, q8=True, guided=True)
    ab3, _, _, _ = feats.match_guided_batch(desc, kps, oa, desc, kps, ob, model1)
    model3, ver3, _ = feats.verify_homography_batch(kps, oa, kps, ob, ab3, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(o_b, o) and torch.equal(m_b, ab3) and torch.equal(ver_b[:n0], ver3[:n0])
    assert torch.equal(model_b.view(torch.int32), model3.view(torch.int32))
    assert per_b.cpu().numpy()[0].tolist() == [raw, mutual, inl, int((ab3[:n0] >= 0).sum()), int((ver3[:n0] >= 0).sum())]
