"""Guided matching on the GPU (lf_mkd_match_guided_pairs_device, LocalFeatures.match_guided_batch): every row of a ragged
batch decided bit for bit as the existing matcher decides it over the row's admissible candidates alone (the host twin's
masks, tests/match_guided_cases.py); everything admissible equals the unguided call; nothing admissible; the mutual filter;
shape independence and capture; the superset property from frames to re-matched pairs; the Python faces; the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_guided_cases as cases
import match_pairs_cases as pcases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

KINDS = (cases.HOMOGRAPHY, cases.FUNDAMENTAL)
NEG_INF = np.float32(-np.inf)


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
    d = tmp_path_factory.mktemp("guided_twin")
    exe = cases.build(d)
    return {(kind, thr): cases.batch_masks(exe, d, kind, thr) for kind in KINDS for thr in cases.THRESHOLDS[kind]}


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class Dev:
    """cases.batch(kind), or another batch of its layout, on the device, and outputs pre-filled with sentinels (-7 / NaN)."""

    def __init__(self, torch, kind, B=None):
        self.B = B = cases.batch(kind) if B is None else B
        self.kind, self.torch = kind, torch
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.a, self.b, self.ka, self.kb = up(B.a), up(B.b), up(B.ka), up(B.kb)
        self.oa, self.ob, self.model = up(B.oa), up(B.ob), up(B.model)

    def outputs(self):
        t, B = self.torch, self.B
        return (t.full((len(B.a),), -7, dtype=t.int32, device="cuda"), t.full((len(B.b),), -7, dtype=t.int32, device="cuda"),
                t.full((len(B.a),), np.nan, device="cuda"), t.full((len(B.a),), np.nan, device="cuda"))

    def run(self, handle, out, thr, ratio=0.8, flags=0, stream=None, offsets=None, n_pairs=None, model=None, totals=None,
            both=True, scores=True):
        ab, ba, s1, s2 = out
        oa, ob = offsets if offsets is not None else (self.oa, self.ob)
        na, nb = totals if totals is not None else (len(self.B.a), len(self.B.b))
        handle.match_guided_pairs_device(self.a.data_ptr(), self.ka.data_ptr(), oa.data_ptr(), na, self.b.data_ptr(),
                                         self.kb.data_ptr(), ob.data_ptr(), nb, (self.model if model is None else model).data_ptr(),
                                         self.B.n_pairs if n_pairs is None else n_pairs, ab.data_ptr(),
                                         ba.data_ptr() if both else None, self.kind, thr, ratio, flags,
                                         s1.data_ptr() if scores else None, s2.data_ptr() if scores else None, stream)

    def call(self, handle, thr, **kw):
        out = self.outputs()
        self.run(handle, out, thr, stream=self.torch.cuda.current_stream().cuda_stream, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]


@pytest.fixture(scope="module")
def dev(torch):
    return {kind: Dev(torch, kind) for kind in KINDS}


# --- the existing matcher over a row's admissible candidates ------------------------------------------------------------
def one_row_pairs(handle, torch, rows, cands, ratio):
    """rows [n, 128], cands: list of [k_i, 128] (k_i >= 2): lf_mkd_match_pairs_device over n pairs of (one row, its
    candidates) -- which is lf_mkd_match_device on each pair, bit for bit (tests/test_gpu_match_pairs.py holds it to that).
    -> (match [n] local to the candidates, best [n], second [n])"""
    n = len(rows)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)
    d_a = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(np.concatenate(cands))).cuda()
    oa = torch.arange(n + 1, dtype=torch.int64).cuda()
    ob = torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)).cuda()
    m = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s1, s2 = torch.full((n,), np.nan, device="cuda"), torch.full((n,), np.nan, device="cuda")
    handle.match_pairs_device(d_a.data_ptr(), oa.data_ptr(), n, d_b.data_ptr(), ob.data_ptr(), d_b.shape[0], n, m.data_ptr(), None,
                              ratio, 0, s1.data_ptr(), s2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return m.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy()


def direct(handle, torch, row, cands, ratio):
    """lf_mkd_match_device on (one row, its candidates): (match, best, second)"""
    d_x, d_y = torch.from_numpy(np.ascontiguousarray(row[None])).cuda(), torch.from_numpy(np.ascontiguousarray(cands)).cuda()
    m = torch.empty(1, dtype=torch.int32, device="cuda")
    s1, s2 = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    handle.match_device(d_x.data_ptr(), 1, d_y.data_ptr(), len(cands), m.data_ptr(), ratio, None, None, s1.data_ptr(), s2.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(m[0]), float(s1[0]), float(s2[0])


def expected(handle, torch, x, y, mask, ratio):
    """What guided matching owes rows x against candidates y under mask [nx, ny]: (match [nx], best, second, the rows'
    candidate lists).  >= 2 candidates: the existing matcher on (the row, the gathered rows), mapped back through the gather;
    1 candidate: accepted, second = -inf, best = the similarity the existing matcher reports for the row against that
    candidate presented twice (ratio 0); none: -1 / -inf / -inf."""
    nx = len(x)
    match, best, second = np.full(nx, -1, np.int32), np.full(nx, NEG_INF), np.full(nx, NEG_INF)
    cand = [np.flatnonzero(mask[i]) for i in range(nx)]
    many = [i for i in range(nx) if len(cand[i]) >= 2]
    m, s1, s2 = one_row_pairs(handle, torch, x[many], [y[cand[i]] for i in many], ratio)
    for k, i in enumerate(many):
        match[i] = cand[i][m[k]] if m[k] >= 0 else -1
        best[i], second[i] = s1[k], s2[k]
    one = [i for i in range(nx) if len(cand[i]) == 1]
    m, s1, s2 = one_row_pairs(handle, torch, x[one], [y[np.repeat(cand[i], 2)] for i in one], 0.0)
    for k, i in enumerate(one):
        assert m[k] == 1 and bits(s1[k]) == bits(s2[k])          # the two copies tie: the higher index, equal scores
        match[i], best[i] = cand[i][0], s1[k]
    return match, best, second, cand


def test_every_row_against_the_existing_matcher_bit_for_bit(dev, masks, handle, torch):
    """Both kinds, both thresholds, ratio 0.8 and 0, every row of every pair in both directions: match (and, in the a -> b
    direction, which alone reports them, best and second) equal the existing matcher's over the admissible rows alone.  Every
    row is held to lf_mkd_match_pairs_device over one-row pairs (one call per case); a spread of about 1200 rows in all is
    held to lf_mkd_match_device itself, one call per row."""
    assert "LF_MKD_MATCH" not in os.environ
    calls = 0
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            for ratio in (0.8, 0.0):
                ab, ba, s1, s2 = D.call(handle, thr, ratio=ratio)
                tally = {"none": 0, "one": 0, "many": 0, "accepted": 0}
                todo = []
                for p in range(B.n_pairs):
                    sa, sb = B.pair(p)
                    fwd, rev, _ = masks[(kind, thr)][p]
                    for name, x, y, mask, got in (("ab", B.a[sa], B.b[sb], fwd, ab[sa]), ("ba", B.b[sb], B.a[sa], rev, ba[sb])):
                        want, w1, w2, cand = expected(handle, torch, x, y, mask, ratio)
                        assert np.array_equal(got, want), (kind, thr, ratio, p, name, np.flatnonzero(got != want)[:8])
                        if name == "ab":
                            assert np.array_equal(bits(s1[sa]), bits(w1)) and np.array_equal(bits(s2[sa]), bits(w2)), (kind, thr, ratio, p)
                        n_c = np.array([len(c) for c in cand], np.int64)
                        tally["none"] += int((n_c == 0).sum())
                        tally["one"] += int((n_c == 1).sum())
                        tally["many"] += int((n_c >= 2).sum())
                        tally["accepted"] += int((got >= 0).sum())
                        assert (got[n_c == 0] == -1).all() and np.array_equal(got[n_c == 1], np.array([c[0] for c in cand if len(c) == 1], np.int32))
                        todo += [(name, x[i], y[cand[i]], cand[i], int(got[i]), s1[sa][i] if name == "ab" else None,
                                  s2[sa][i] if name == "ab" else None) for i in np.flatnonzero(n_c >= 2)]
                for name, row, rows, cand, got, g1, g2 in todo[::max(1, len(todo) // 150)][:150]:
                    m, w1, w2 = direct(handle, torch, row, rows, ratio)
                    calls += 1
                    assert got == (cand[m] if m >= 0 else -1), (kind, thr, ratio, name)
                    if g1 is not None:
                        assert bits(g1) == bits(np.float32(w1)) and bits(g2) == bits(np.float32(w2)), (kind, thr, ratio)
                print(f"[match_guided] kind {kind} thr {thr} ratio {ratio}: rows with no / one / several candidates "
                      f"{tally['none']} / {tally['one']} / {tally['many']}, accepted {tally['accepted']}")
                assert tally["none"] and tally["one"] and tally["many"] and tally["accepted"]
    assert 400 < calls <= 1500, calls


def _unguided(D, handle, torch, ratio, flags):
    B = D.B
    ab, ba, s1, s2 = D.outputs()
    handle.match_pairs_device(D.a.data_ptr(), D.oa.data_ptr(), len(B.a), D.b.data_ptr(), D.ob.data_ptr(), len(B.b), B.n_pairs,
                              ab.data_ptr(), ba.data_ptr(), ratio, flags, s1.data_ptr(), s2.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (ab, ba, s1, s2)]


def test_everything_admissible_equals_the_unguided_call(dev, handle, torch):
    """H = I and any F whose Sampson denominator is positive, at a threshold of 1e9 px: every pair of points is admissible, and
    every output of every pair with at least two candidates per row equals lf_mkd_match_pairs_device's, bit for bit, with and
    without the mutual filter.  A direction the unguided call refuses (one candidate: pair 4's b -> a) follows the
    one-candidate rule instead."""
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        one = np.eye(3, dtype=np.float32).reshape(9) if kind == cases.HOMOGRAPHY else B.model[0]
        model = torch.from_numpy(np.ascontiguousarray(np.tile(one, (B.n_pairs, 1)))).cuda()
        for p in range(B.n_pairs):                                        # the premise, in float64
            sa, sb = B.pair(p)
            ok, _ = cases.f64_residual(kind, one, B.ka[sa, :2], B.kb[sb, :2], 1e9)
            assert ok.all()
        for flags in (0, lfp.MATCH_MUTUAL):
            got = D.call(handle, 1e9, model=model, flags=flags)
            plain = D.call(handle, 1e9, model=model)
            ref = _unguided(D, handle, torch, 0.8, 0)
            want_ab, want_ba = ref[0].copy(), ref[1].copy()
            refused = 0
            for p, (na, nb) in enumerate(cases.SIZES):
                sa, sb = B.pair(p)
                if nb == 1:
                    want_ab[sa] = 0
                    refused += 1
                if na == 1:
                    want_ba[sb] = 0
                    refused += 1
            assert refused == 1 and cases.SIZES[4] == (1, 2)
            assert np.array_equal(plain[0], want_ab) and np.array_equal(plain[1], want_ba), kind
            assert np.array_equal(bits(plain[2]), bits(ref[2])) and np.array_equal(bits(plain[3]), bits(ref[3])), kind
            if flags:
                want_ab, want_ba = pcases.mutual(want_ab, want_ba, B.oa, B.ob)
                mref = _unguided(D, handle, torch, 0.8, flags)
                for p, (na, nb) in enumerate(cases.SIZES):                # where the unguided call refuses nothing: its own filter
                    if na >= 2 and nb >= 2:
                        sa, sb = B.pair(p)
                        assert np.array_equal(got[0][sa], mref[0][sa]) and np.array_equal(got[1][sb], mref[1][sb]), (kind, p)
            assert np.array_equal(got[0], want_ab) and np.array_equal(got[1], want_ba), (kind, flags)
            assert np.array_equal(bits(got[2]), bits(ref[2])) and np.array_equal(bits(got[3]), bits(ref[3])), (kind, flags)


def test_nothing_admissible(dev, handle, torch):
    """The all-zero model and the model with a NaN: -1 / -inf for every row of those pairs; and the other pairs' outputs do
    not depend on their presence (the same batch with a sound model in their place)."""
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][1]
        sound = B.model.copy()
        sound[cases.ZERO_MODEL], sound[cases.NAN_MODEL] = B.model[5], B.model[5]
        for flags in (0, lfp.MATCH_MUTUAL):
            got = D.call(handle, thr, flags=flags)
            other = D.call(handle, thr, flags=flags, model=torch.from_numpy(sound).cuda())
            for p in range(B.n_pairs):
                sa, sb = B.pair(p)
                if p in (cases.ZERO_MODEL, cases.NAN_MODEL):
                    assert (got[0][sa] == -1).all() and (got[1][sb] == -1).all() and len(got[0][sa]) and len(got[1][sb])
                    assert (got[2][sa] == NEG_INF).all() and (got[3][sa] == NEG_INF).all()
                else:
                    assert np.array_equal(got[0][sa], other[0][sa]) and np.array_equal(got[1][sb], other[1][sb]), (kind, p)
                    assert np.array_equal(bits(got[2][sa]), bits(other[2][sa])) and np.array_equal(bits(got[3][sa]), bits(other[3][sa]))
        # a NaN coordinate: that row has no candidate and is nobody's candidate
        ka = B.ka.copy()
        row = int(B.oa[0]) + 2
        ka[row, 0] = np.nan
        keep = D.ka
        D.ka = torch.from_numpy(ka).cuda()
        try:
            nan_row = D.call(handle, thr, ratio=0.0)
        finally:
            D.ka = keep
        assert nan_row[0][row] == -1 and nan_row[2][row] == NEG_INF and not (nan_row[1][B.pair(0)[1]] == 2).any()


def test_mutual_is_the_filter_of_the_unfiltered_outputs(dev, handle):
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        for thr in cases.THRESHOLDS[kind]:
            ab0, ba0, s1_0, s2_0 = D.call(handle, thr)
            ab, ba, s1, s2 = D.call(handle, thr, flags=lfp.MATCH_MUTUAL)
            want_ab, want_ba = pcases.mutual(ab0, ba0, B.oa, B.ob)
            assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba), (kind, thr)
            assert np.array_equal(bits(s1), bits(s1_0)) and np.array_equal(bits(s2), bits(s2_0))     # best / second are not filtered
            kept, fwd = int((ab[B.oa[0]:B.oa[-1]] >= 0).sum()), int((ab0[B.oa[0]:B.oa[-1]] >= 0).sum())
            print(f"[match_guided] kind {kind} thr {thr}: {fwd} forward matches, {kept} mutual")
            assert 0 < kept <= fwd
    with pytest.raises(RuntimeError, match="match_guided_pairs_device: LF_MKD_MATCH_MUTUAL needs d_match_ba"):
        D.run(handle, D.outputs(), 3.0, flags=lfp.MATCH_MUTUAL, both=False)


def test_shape_independent_repeatable_and_capturable(dev, handle, torch):
    same = lambda x, y: all(np.array_equal(bits(u) if u.dtype == np.float32 else u, bits(v) if v.dtype == np.float32 else v)
                            for u, v in zip(x, y))
    for kind in KINDS:
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][1]
        whole = D.call(handle, thr)
        # rows outside the offsets keep their sentinels; every row inside is written
        ab, ba, s1, s2 = whole
        assert (ab[:B.oa[0]] == -7).all() and (ab[B.oa[-1]:] == -7).all() and (ba[:B.ob[0]] == -7).all() and (ba[B.ob[-1]:] == -7).all()
        assert (ab[B.oa[0]:B.oa[-1]] != -7).all() and (ba[B.ob[0]:B.ob[-1]] != -7).all()
        assert np.isnan(s1[:B.oa[0]]).all() and np.isnan(s2[B.oa[-1]:]).all() and not np.isnan(s1[B.oa[0]:B.oa[-1]]).any()
        # one direction, no scores: what is not asked for is not written
        one_way = D.call(handle, thr, both=False, scores=False)
        assert np.array_equal(one_way[0], ab) and (one_way[1] == -7).all() and np.isnan(one_way[2]).all() and np.isnan(one_way[3]).all()
        # pair p alone (n_pairs = 1, its two offsets, its model) equals pair p of the batch
        for p in range(B.n_pairs):
            off = (D.oa[p:p + 2].clone(), D.ob[p:p + 2].clone())
            out = D.call(handle, thr, offsets=off, n_pairs=1, model=D.model[p:p + 1].clone())
            sa, sb = B.pair(p)
            assert np.array_equal(out[0][sa], ab[sa]) and np.array_equal(out[1][sb], ba[sb]), (kind, p)
            assert np.array_equal(bits(out[2][sa]), bits(s1[sa])) and np.array_equal(bits(out[3][sa]), bits(s2[sa])), (kind, p)
            assert (out[0][:sa.start] == -7).all() and (out[0][sa.stop:] == -7).all() and (out[1][:sb.start] == -7).all() \
                and (out[1][sb.stop:] == -7).all(), (kind, p)
        none = D.call(handle, thr, n_pairs=0)                                         # n_pairs == 0 writes nothing
        assert (none[0] == -7).all() and (none[1] == -7).all() and np.isnan(none[2]).all()
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
            out = D.outputs()                                                         # a captured call replays to the same bits
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                D.run(handle, out, thr, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
            for x, fill in zip(out, (-7, -7, np.nan, np.nan)):
                x.fill_(fill)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same(first, [x.cpu().numpy() for x in out])


def test_offsets_beyond_the_totals_touch_nothing(dev, handle, torch):
    """Whatever the offsets hold, no row at or beyond a total is read or written: an offset beyond the total counts as the
    total, an inverted pair as an empty one.  (The totals the call is told end inside the arrays, whose tails -- the rows
    behind the last pair -- must keep their sentinels.)"""
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
            assert (out[0][na:] == -7).all() and (out[1][nb:] == -7).all() and np.isnan(out[2][na:]).all() \
                and np.isnan(out[3][na:]).all(), (kind, oa, ob)
            if oa[0] == a0:                                                  # pair 0 is intact: decided as alone
                assert np.array_equal(out[0][a0:a1], alone[0][a0:a1]) and np.array_equal(out[1][b0:b1], alone[1][b0:b1]), (oa, ob)
                assert np.array_equal(bits(out[2][a0:a1]), bits(alone[2][a0:a1]))
            else:                                                            # no a row is in range: b's rows find no candidates
                assert (out[0] == -7).all() and (out[1][b0:nb] == -1).all() and (out[1][:b0] == -7).all()


# --- frames to re-matched pairs -----------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_match_pairs.py::_frames, warp 0


def _frames(n_warps=1):
    """the 1024 x 768 centre crop of houses.jpg and its first perspective warp(s) (PIL images)"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    out = [crop]
    for k in range(n_warps):
        h = H_TRUE.copy()
        h[:2, 2] += 7.0 * k                                                  # (further frames for the example: shifted copies)
        hi = np.linalg.inv(h)
        hi = hi / hi[2, 2]
        out.append(crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC))
    return out


def test_guided_matching_never_loses_a_verified_match(torch):
    """The superset property (include/lf_mkd.h), end to end on the device: detect, match (mutual), verify (H and F), then the
    guided call with each model at the verifier's threshold and ratio -- every verified match is found again, in both
    directions."""
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, n_scales=5, max_frames=2)
    cap = 6000
    d_img = torch.from_numpy(frames).cuda()
    kps = torch.empty((cap, 5), device="cuda")
    fid = torch.empty((cap,), dtype=torch.int32, device="cuda")
    desc = torch.empty((cap, 128), device="cuda")
    m, _, dropped = feats._inner.detect_frames_device(d_img.data_ptr(), 2, 1024, 768, 2000, 0.0, kps.data_ptr(), fid.data_ptr(),
                                                     desc.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    assert dropped == 0
    kps, fid, desc = kps[:m], fid[:m].long(), desc[:m]
    o = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.bincount(fid, minlength=2), 0)])
    oa, ob = o[:2], o[1:]                                                    # frame 0 against frame 1, no row copied
    n0 = int(o[1])
    assert n0 > 1000
    ab, ba, _, _ = feats.match_batch(desc, oa, desc, ob, mutual=True)
    for kind, verify in (("homography", feats.verify_homography_batch), ("fundamental", feats.verify_fundamental_batch)):
        model, ver, st = verify(kps, oa, kps, ob, ab, seed=21)
        g_ab, g_ba, _, _ = feats.match_guided_batch(desc, kps, oa, desc, kps, ob, model, kind=kind)
        torch.cuda.synchronize()
        v, g, gb = ver.cpu().numpy()[:n0], g_ab.cpu().numpy()[:n0], g_ba.cpu().numpy()[n0:]
        i = np.flatnonzero(v >= 0)
        n_mutual, n_ver, n_guided = int((ab[:n0] >= 0).sum()), len(i), int((g >= 0).sum())
        print(f"[match_guided] crop -> warp under one {kind}: {n_mutual} mutual, {n_ver} verified, {n_guided} guided")
        assert n_ver >= 8
        assert np.array_equal(g[i], v[i]), kind                               # guided_ab[i] == verified[i]
        assert np.array_equal(gb[v[i]], i), kind                              # ... and match_ba[j] == i
        assert n_guided >= n_ver, (kind, n_guided, n_ver)
        assert (g_ab[n0:] == -1).all() and (g_ba[:n0] == -1).all()            # rows outside the pair


def test_match_guided_batch_and_match_guided_faces(dev, handle, torch):
    """LocalFeatures.match_guided_batch / match_guided: tensors of other dtypes and on the host are accepted, the outputs have
    the stated shapes, rows outside every pair read -1 / -inf, and the single-pair form equals pair 0 of the batch."""
    feats = lfp.LocalFeatures(64, 64, 64)
    for kind, name in zip(KINDS, ("homography", "fundamental")):
        D, B = dev[kind], dev[kind].B
        thr = cases.THRESHOLDS[kind][0]
        want = D.call(handle, thr, flags=lfp.MATCH_MUTUAL)
        ab, ba, s1, s2 = feats.match_guided_batch(torch.from_numpy(B.a).double(), torch.from_numpy(B.ka), torch.from_numpy(B.oa).to(torch.int32),
                                                  D.b, D.kb.double(), D.ob, torch.from_numpy(B.model).reshape(-1, 3, 3), kind=name)
        torch.cuda.synchronize()
        assert ab.shape == (len(B.a),) and ba.shape == (len(B.b),) and s1.shape == s2.shape == (len(B.a),)
        assert ab.dtype == ba.dtype == torch.int32 and s1.dtype == torch.float32 and ab.is_cuda and ba.is_cuda and s1.is_cuda
        ia, ib = slice(B.oa[0], B.oa[-1]), slice(B.ob[0], B.ob[-1])
        assert np.array_equal(ab.cpu().numpy()[ia], want[0][ia]) and np.array_equal(ba.cpu().numpy()[ib], want[1][ib])     # the default threshold
        assert np.array_equal(bits(s1.cpu().numpy()[ia]), bits(want[2][ia])) and np.array_equal(bits(s2.cpu().numpy()[ia]), bits(want[3][ia]))
        assert (ab[:B.oa[0]] == -1).all() and (ba[B.ob[-1]:] == -1).all() and bool(torch.isinf(s1[:B.oa[0]]).all())
        # GUIDE_* constants, an explicit threshold, no mutual filter, a stream of the caller's
        s = torch.cuda.Stream()
        thr2 = cases.THRESHOLDS[kind][1]
        plain = D.call(handle, thr2, ratio=0.0)
        ab2, ba2, _, _ = feats.match_guided_batch(D.a, D.ka, D.oa, D.b, D.kb, D.ob, D.model, kind=kind, threshold=thr2, ratio=0.0,
                                                  mutual=False, stream=s)
        s.synchronize()
        assert np.array_equal(ab2.cpu().numpy()[ia], plain[0][ia]) and np.array_equal(ba2.cpu().numpy()[ib], plain[1][ib])
        # one pair: all of a against all of b, equal to pair 0 of the batch
        sa, sb = B.pair(0)
        one = feats.match_guided(torch.from_numpy(B.a[sa]), torch.from_numpy(B.ka[sa]), D.b[sb], D.kb[sb], torch.from_numpy(B.model[0]).reshape(3, 3),
                                 kind=name)
        torch.cuda.synchronize()
        assert one[0].shape == (sa.stop - sa.start,) and one[1].shape == (sb.stop - sb.start,)
        assert np.array_equal(one[0].cpu().numpy(), want[0][sa]) and np.array_equal(one[1].cpu().numpy(), want[1][sb])
        assert np.array_equal(bits(one[2].cpu().numpy()), bits(want[2][sa]))
        # an empty side, no pairs
        e, z = torch.zeros((0, 128)), torch.zeros(2, dtype=torch.int64)
        ab, ba, s1, _ = feats.match_guided_batch(e, torch.zeros((0, 5)), z, D.b[:10], D.kb[:10], torch.tensor([0, 10]), D.model[:1], kind=name)
        assert ab.shape == (0,) and ba.shape == (10,) and (ba == -1).all() and s1.shape == (0,)
        with pytest.raises(RuntimeError, match="n_pairs"):
            feats.match_guided_batch(D.a, D.ka, D.oa, D.b, D.kb, D.ob[:-1], D.model, kind=name)
        with pytest.raises(RuntimeError, match="kind"):
            feats.match_guided_batch(D.a, D.ka, D.oa, D.b, D.kb, D.ob, D.model, kind="affine")


def test_match_sequence_example_guided(tmp_path):
    """examples/match_sequence.py --guided on three generated frames: two more figures per line, guided >= verified."""
    paths = []
    for t, f in enumerate(_frames(2)):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_sequence.py")
    for extra in (["--guided"], ["--fundamental", "--guided"]):
        out = subprocess.run([sys.executable, exe] + extra + paths, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        print("\n".join(lines))
        assert lines[0].startswith("Extracted ") and len(lines) == 3
        for t, line in enumerate(lines[1:]):
            w = line.replace(",", "").split()
            assert line.startswith(f"Pair {t + 1} -> {t + 2}: ") and w[5] == "matches" and w[7] == "mutual"
            assert w[-5] == "guided" and w[-3:] == ["agree", "after", "re-verification"], line
            raw, mutual, inl, guided, again = int(w[4]), int(w[6]), int(w[8]), int(w[-6]), int(w[-4])
            assert raw >= mutual >= inl >= 8 and guided >= inl and guided >= again >= 8, line
