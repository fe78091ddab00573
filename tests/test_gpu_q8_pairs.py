"""The batched int8 matcher on the GPU (lf_mkd_match_q8_pairs_device, LocalFeatures.match_q8_batch): every pair of a ragged
batch of quantised rows decided exactly as the single-pair call (lf_mkd_match_q8_device) decides it, and as the numpy integer
product does -- every comparison is ==, integer sums have no tolerance; ties, the mutual filter, the copy-free sequence
layout, independence of the batch, graph capture, offsets beyond the totals, and frames to verified matches in 8 bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import homography_ref as href
import match_pairs_cases as pcases
import q8_cases as qcases
import q8_pairs_cases as cases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

GUARD = 8                        # sentinel words in front of and behind every output
SENTINEL = cases.SENTINEL
RATIO = float(cases.RATIO)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def R():
    return lfp.match_q8_pairs_plan(0, 0, 0)[0]            # only the plan function knows the block size


class Batch:
    """Quantised rows and offsets on the device in the verifiers' layout; outputs between GUARD sentinel words."""

    def __init__(self, torch, qa, oa, qb, ob, na_total=None, nb_total=None):
        self.torch = torch
        self.qa, self.qb = np.array(qa, np.uint8, order="C"), np.array(qb, np.uint8, order="C")   # copies: the shared batch is read-only
        self.oa, self.ob = np.array(oa, np.int64), np.array(ob, np.int64)
        self.na = len(qa) if na_total is None else na_total           # the totals the call is told
        self.nb = len(qb) if nb_total is None else nb_total
        self.n_pairs = len(self.oa) - 1
        self.d_a, self.d_b = torch.from_numpy(self.qa).cuda(), torch.from_numpy(self.qb).cuda()
        self.d_oa, self.d_ob = torch.from_numpy(self.oa).cuda(), torch.from_numpy(self.ob).cuda()

    def outputs(self):
        """match_ab, match_ba, best, second: as long as the ALLOCATED rows (which may exceed the totals), plus the guards"""
        t = self.torch
        return [t.full((n + 2 * GUARD,), SENTINEL, dtype=t.int32, device="cuda") for n in (len(self.qa), len(self.qb), len(self.qa), len(self.qa))]

    def run(self, handle, out, ratio=RATIO, flags=0, both=True, scores=True, stream=None, offsets=None, n_pairs=None):
        ptr = lambda k: out[k].data_ptr() + 4 * GUARD
        d_oa, d_ob = offsets if offsets is not None else (self.d_oa, self.d_ob)
        handle.match_q8_pairs_device(self.d_a.data_ptr(), d_oa.data_ptr(), self.na, self.d_b.data_ptr(), d_ob.data_ptr(), self.nb,
                                     self.n_pairs if n_pairs is None else n_pairs, ptr(0), ptr(1) if both else None, ratio, flags,
                                     ptr(2) if scores else None, ptr(3) if scores else None, stream)

    @staticmethod
    def result(out):
        """the outputs as numpy arrays without their guards, after checking that the guard words are untouched"""
        got = []
        for b in out:
            h = b.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "a guard word was written"
            got.append(h[GUARD:-GUARD].copy())
        return got

    def call(self, handle, **kw):
        out = self.outputs()
        self.torch.cuda.synchronize()
        self.run(handle, out, stream=self.torch.cuda.current_stream().cuda_stream, **kw)
        self.torch.cuda.synchronize()
        return self.result(out)


def single(handle, torch, d_x, d_y, ratio=RATIO):
    """lf_mkd_match_q8_device on one pair's device rows (views, nothing copied): (match, best, second) as numpy, or the
    too-few rule where the call refuses the pair"""
    nx, ny = d_x.shape[0], d_y.shape[0]
    if nx == 0 or ny < 2:
        return np.full(nx, -1, np.int32), np.full(nx, cases.INT32_MIN, np.int32), np.full(nx, cases.INT32_MIN, np.int32)
    out = [torch.full((nx + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    handle.match_q8_device(d_x.data_ptr(), nx, d_y.data_ptr(), ny, out[0].data_ptr() + 4 * GUARD, float(ratio), None, None,
                           out[1].data_ptr() + 4 * GUARD, out[2].data_ptr() + 4 * GUARD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return Batch.result(out)


def same(got, want, what):
    for name, g, w in zip(("match_ab", "match_ba", "best", "second"), got, want):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.fixture(scope="module")
def ragged(torch, R):
    qa, oa, qb, ob, _ = cases.ragged_q8_batch(R)
    return Batch(torch, qa, oa, qb, ob)


@pytest.fixture(scope="module")
def ragged_out(ragged, handle):
    """the unfiltered result of the ragged batch, both directions with best / second"""
    return ragged.call(handle)


# --- 1 ----------------------------------------------------------------------------------------------------------------
def test_batched_equals_single_and_the_integer_product(ragged, ragged_out, handle, torch, R):
    B = ragged
    sizes = cases.ragged_q8_batch(R)[4]
    want = cases.ragged_reference(R)
    # the numpy restatement, rows outside the pairs included: they keep their sentinel
    same(ragged_out, want, "ragged batch")
    ab, ba, best, second = ragged_out
    assert (ab[:B.oa[0]] == SENTINEL).all() and (ab[B.oa[-1]:] == SENTINEL).all() and B.oa[0] == 5 and len(ab) - B.oa[-1] == 7
    assert (ba[:B.ob[0]] == SENTINEL).all() and (ba[B.ob[-1]:] == SENTINEL).all() and (best[:B.oa[0]] == SENTINEL).all()
    for p, (na, nb) in enumerate(sizes):
        sa, sb = slice(B.oa[p], B.oa[p + 1]), slice(B.ob[p], B.ob[p + 1])
        m, s1, s2 = single(handle, torch, B.d_a[sa], B.d_b[sb])
        assert np.array_equal(ab[sa], m) and np.array_equal(best[sa], s1) and np.array_equal(second[sa], s2), (p, na, nb, "a -> b")
        m, _, _ = single(handle, torch, B.d_b[sb], B.d_a[sa])
        assert np.array_equal(ba[sb], m), (p, na, nb, "b -> a")
        if nb < 2:            # too few candidates: -1 / INT32_MIN whatever the ratio
            assert (ab[sa] == -1).all() and (best[sa] == cases.INT32_MIN).all() and (second[sa] == cases.INT32_MIN).all(), p
        if na < 2:
            assert (ba[sb] == -1).all(), p
    # one direction only, and without the scores: the same values, and what was not asked for is not written
    one_way, no_scores = B.call(handle, both=False), B.call(handle, scores=False)
    assert np.array_equal(one_way[0], ab) and (one_way[1] == SENTINEL).all() and np.array_equal(one_way[2], best)
    assert np.array_equal(no_scores[0], ab) and np.array_equal(no_scores[1], ba) and (no_scores[2] == SENTINEL).all() \
        and (no_scores[3] == SENTINEL).all()
    # ratio <= 0: the best index as is
    same(B.call(handle, ratio=0.0), cases.match_pairs(B.qa, B.oa, B.qb, B.ob, np.float32(0.0)), "ratio 0")


# --- 2 ----------------------------------------------------------------------------------------------------------------
def test_planted_ties_inside_later_pairs(handle, torch):
    """Every b row of pairs 1 and 2 occurs twice, n rows apart: n = 48 puts a row and its copy on either side of a 32-row tile
    border, n = 100 on either side of the 128-row LDS stage border for rows 28 .. 99.  The HIGHEST index wins and
    second == best, local to the pair; with the ratio test on, a duplicated best is rejected."""
    pairs = [qcases.quantized_sets(40, 50, 5101)]
    for n, na in ((48, 70), (100, 60)):
        qa, b0 = qcases.quantized_sets(na, n, 5100 + n)
        pairs.append((qa, np.concatenate([b0, b0])))
    pairs.append(qcases.quantized_sets(64, 64, 5102))
    qa, qb = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    oa = np.cumsum([0] + [len(p[0]) for p in pairs])
    ob = np.cumsum([0] + [len(p[1]) for p in pairs])
    B = Batch(torch, qa, oa, qb, ob)
    for ratio in (0.0, RATIO):
        want = cases.match_pairs(qa, oa, qb, ob, np.float32(ratio))
        same(B.call(handle, ratio=ratio), want, ("ties", ratio))
        for p, n in ((1, 48), (2, 100)):
            sa = slice(oa[p], oa[p + 1])
            assert (want[2][sa] == want[3][sa]).all()
            assert (want[0][sa] >= n).all() if ratio == 0.0 else (want[0][sa] == -1).all()
    # some a row's best is a b row whose copy lies behind the stage border (rows 28 .. 99 of pair 2 and their copies)
    w0 = cases.match_pairs(qa, oa, qb, ob, np.float32(0.0))[0][oa[2]:oa[3]]
    assert ((w0 - 100 >= 28) & (w0 - 100 < 100)).any()


# --- 3 ----------------------------------------------------------------------------------------------------------------
def test_mutual_filter(ragged, ragged_out, handle, R):
    ab0, ba0, s1_0, s2_0 = ragged_out
    B = ragged
    ab, ba, s1, s2 = B.call(handle, flags=lfp.MATCH_MUTUAL)
    want_ab, want_ba = pcases.mutual(ab0, ba0, B.oa, B.ob)
    assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba)
    assert np.array_equal(s1, s1_0) and np.array_equal(s2, s2_0)              # best / second are not filtered
    kept, fwd = (ab[B.oa[0]:B.oa[-1]] >= 0).sum(), (ab0[B.oa[0]:B.oa[-1]] >= 0).sum()
    assert 0 < kept < fwd and kept == (ba[B.ob[0]:B.ob[-1]] >= 0).sum()
    with pytest.raises(RuntimeError, match="match_q8_pairs_device: LF_MKD_MATCH_MUTUAL needs d_match_ba"):
        B.run(handle, B.outputs(), flags=lfp.MATCH_MUTUAL, both=False)


# --- 4 ----------------------------------------------------------------------------------------------------------------
def test_sequence_layout_without_a_copied_row(handle, torch):
    """One array of 6 quantised frames: frame t against frame t + 1 (five pairs, both directions) through the shifted view of
    the same array, and through the array itself with the next frames' offsets."""
    sizes = [300, 17, 450, 233, 64, 129]
    rng = np.random.default_rng(31)
    base = pcases.unit(rng.normal(size=(500, 128)))
    frames = [pcases.unit(base[rng.integers(0, 500, n)] + 0.03 * rng.normal(size=(n, 128))) for n in sizes]   # one scene, six views
    q = np.ascontiguousarray(np.concatenate([qcases.quantize(f) for f in frames]))
    o = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    F = len(sizes)
    d = torch.from_numpy(q).cuda()
    results = []
    for view, ob in ((d[o[1]:], o[1:F + 1] - o[1]), (d, o[1:F + 1])):
        oa = o[0:F]
        d_oa, d_ob = torch.from_numpy(np.ascontiguousarray(oa)).cuda(), torch.from_numpy(np.ascontiguousarray(ob)).cuda()
        ab = torch.full((len(q),), SENTINEL, dtype=torch.int32, device="cuda")
        ba = torch.full((view.shape[0],), SENTINEL, dtype=torch.int32, device="cuda")
        handle.match_q8_pairs_device(d.data_ptr(), d_oa.data_ptr(), len(q), view.data_ptr(), d_ob.data_ptr(), view.shape[0], F - 1,
                                     ab.data_ptr(), ba.data_ptr(), RATIO, 0, None, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ab, ba = ab.cpu().numpy(), ba.cpu().numpy()
        for t in range(F - 1):
            x, y = d[o[t]:o[t + 1]], d[o[t + 1]:o[t + 2]]
            assert np.array_equal(ab[o[t]:o[t + 1]], single(handle, torch, x, y)[0]), t
            assert np.array_equal(ba[ob[t]:ob[t + 1]], single(handle, torch, y, x)[0]), t
        assert (ab[o[F - 1]:] == SENTINEL).all() and (ba[:ob[0]] == SENTINEL).all()   # the last frame has no successor, the first no predecessor
        assert (ab >= 0).sum() > 100 and (ba >= 0).sum() > 100
        results.append((ab, ba[ob[0]:]))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


# --- 5 ----------------------------------------------------------------------------------------------------------------
def test_independent_repeatable_and_capturable(ragged, ragged_out, handle, torch, R):
    B = ragged
    n = B.n_pairs
    # the single-pair q8 call on this handle, with a plan that uses the handle's q8 scratch: before ...
    na1, nb1 = 513, 1025
    assert lfp.match_q8_plan(na1, nb1)[2] > 0
    q1a, q1b = qcases.quantized_sets(na1, nb1, 3004)
    d1a, d1b = torch.from_numpy(q1a).cuda(), torch.from_numpy(q1b).cuda()
    want1 = qcases.match_q8(q1a, q1b)
    before = single(handle, torch, d1a, d1b)
    # pair p alone (n_pairs = 1, its two offsets) equals pair p of the batch
    for p in (0, 2, 9, 16, 17, 20, 26, n - 5, n - 2, n - 1):
        off = (B.d_oa[p:p + 2].clone(), B.d_ob[p:p + 2].clone())
        out = B.call(handle, offsets=off, n_pairs=1)
        sa, sb = slice(B.oa[p], B.oa[p + 1]), slice(B.ob[p], B.ob[p + 1])
        for k, s in ((0, sa), (1, sb), (2, sa), (3, sa)):
            assert np.array_equal(out[k][s], ragged_out[k][s]), (p, k)
            assert (out[k][:s.start] == SENTINEL).all() and (out[k][s.stop:] == SENTINEL).all(), (p, k)
    # n_pairs == 0 writes nothing
    assert all((x == SENTINEL).all() for x in B.call(handle, n_pairs=0))
    for flags in (0, lfp.MATCH_MUTUAL):
        first = B.call(handle, flags=flags)
        same(B.call(handle, flags=flags), first, "two runs")
        # a stream of the caller's
        s = torch.cuda.Stream()
        out = B.outputs()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            B.run(handle, out, flags=flags, stream=s.cuda_stream)
        s.synchronize()
        same(B.result(out), first, "caller's stream")
        # the handle's own stream (stream = None: the binding waits before and after)
        out = B.outputs()
        B.run(handle, out, flags=flags, stream=None)
        same(B.result(out), first, "handle's stream")
        # a captured call (one launch, or a chain of three) replays to the same values
        out = B.outputs()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            B.run(handle, out, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
        for x in out:
            x.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(B.result(out), first, "replay")
        if flags == 0:
            same(first, ragged_out, "unfiltered")
    # ... and after: the handle's q8 scratch was not disturbed, and the batched call left no state behind
    after = single(handle, torch, d1a, d1b)
    for g, b, w in zip(after, before, want1):
        assert np.array_equal(g, w) and np.array_equal(b, w)


# --- 6 ----------------------------------------------------------------------------------------------------------------
def test_offsets_beyond_the_totals_touch_nothing(handle, torch):
    """Whatever the offsets hold, no row at or beyond a total is read or written: an offset beyond the total counts as the
    total, an inverted pair as an empty one.  (The arrays end where the totals say, inside a larger allocation whose tail must
    keep its sentinel.)"""
    pa, pb = qcases.quantized_sets(40, 50, 5201), qcases.quantized_sets(30, 20, 5202)
    rng = np.random.default_rng(5203)
    tail = lambda: rng.integers(1, 256, (40, 128)).astype(np.uint8)
    qa, qb = np.concatenate([pa[0], pb[0], tail()]), np.concatenate([pa[1], pb[1], tail()])
    na, nb = 70, 70                                                          # the totals the call is told: the tails lie beyond
    for oa, ob in (([0, 40, 5000], [0, 50, 70]), ([0, 40, 70], [0, 50, 1 << 40]), ([0, 40, 20], [0, 50, 70]),
                   ([1 << 33, 1 << 34, 1 << 35], [0, 50, 70]), ([0, 40, 70], [0, 50, 70])):
        B = Batch(torch, qa, oa, qb, ob, na_total=na, nb_total=nb)
        for flags in (0, lfp.MATCH_MUTUAL):
            ab, ba, s1, s2 = B.call(handle, flags=flags)
            assert (ab[na:] == SENTINEL).all() and (ba[nb:] == SENTINEL).all() and (s1[na:] == SENTINEL).all() \
                and (s2[na:] == SENTINEL).all(), (oa, ob)
            want = cases.match_pairs(qa[:na], oa, qb[:nb], ob)
            w_ab, w_ba = pcases.mutual(want[0], want[1], oa, ob) if flags else (want[0], want[1])
            same([ab[:na], ba[:nb], s1[:na], s2[:na]], [w_ab, w_ba, want[2], want[3]], (oa, ob, flags))
            if oa[0] == 0 and flags == 0:                                    # pair 0 is intact: decided as it is alone
                m, b1, b2 = single(handle, torch, B.d_a[:40], B.d_b[:50])
                assert np.array_equal(ab[:40], m) and np.array_equal(s1[:40], b1) and np.array_equal(s2[:40], b2), (oa, ob)
                assert np.array_equal(ba[:50], single(handle, torch, B.d_b[:50], B.d_a[:40])[0]), (oa, ob)
            if oa[0] != 0:                                                   # no a row is in range: b's rows find no candidates
                assert (ab == SENTINEL).all() and (ba[:nb] == -1).all()


# --- 7 ----------------------------------------------------------------------------------------------------------------
def test_match_q8_batch_face(ragged, ragged_out, torch):
    """LocalFeatures.match_q8_batch: host tensors and other integer dtypes for the offsets are accepted; the outputs have the
    stated shapes and dtypes; rows outside every pair come back as -1 / INT32_MIN."""
    B = ragged
    feats = lfp.LocalFeatures(64, 64, 64)
    int_min = int(cases.INT32_MIN)
    ab, ba, s1, s2 = feats.match_q8_batch(torch.from_numpy(B.qa), torch.from_numpy(B.oa).to(torch.int32), B.d_b,
                                          B.d_ob.to(torch.int32), both=True)    # rows and int32 offsets on the host
    torch.cuda.synchronize()
    assert ab.shape == s1.shape == s2.shape == (len(B.qa),) and ba.shape == (len(B.qb),)
    assert ab.dtype == ba.dtype == s1.dtype == s2.dtype == torch.int32 and ab.is_cuda and ba.is_cuda and s1.is_cuda and s2.is_cuda
    inside_a, inside_b = slice(B.oa[0], B.oa[-1]), slice(B.ob[0], B.ob[-1])
    for got, want, ins in ((ab, ragged_out[0], inside_a), (ba, ragged_out[1], inside_b), (s1, ragged_out[2], inside_a), (s2, ragged_out[3], inside_a)):
        assert np.array_equal(got.cpu().numpy()[ins], want[ins])
    assert (ab[:B.oa[0]] == -1).all() and (ab[B.oa[-1]:] == -1).all() and (ba[:B.ob[0]] == -1).all()
    assert (s1[:B.oa[0]] == int_min).all() and (s2[B.oa[-1]:] == int_min).all()
    one, none, _, _ = feats.match_q8_batch(B.d_a, B.d_oa, B.d_b, B.d_ob)
    assert none is None and torch.equal(one, ab)
    s = torch.cuda.Stream()
    mab, mba, m1, m2 = feats.match_q8_batch(B.d_a, B.d_oa, B.d_b, B.d_ob, mutual=True, stream=s)
    s.synchronize()
    w_ab, w_ba = pcases.mutual(ab.cpu().numpy(), ba.cpu().numpy(), B.oa, B.ob)
    assert np.array_equal(mab.cpu().numpy(), w_ab) and np.array_equal(mba.cpu().numpy(), w_ba) and torch.equal(m1, s1) and torch.equal(m2, s2)
    # an empty side, no pairs
    e = torch.zeros((0, 128), dtype=torch.uint8)
    z = torch.zeros(3, dtype=torch.int64)
    ab, ba, s1, s2 = feats.match_q8_batch(e, z, B.d_b[:10], torch.tensor([0, 4, 10]), both=True)
    assert ab.shape == (0,) and ba.shape == (10,) and (ba == -1).all() and s1.shape == (0,) and s1.dtype == torch.int32
    ab, ba, s1, _ = feats.match_q8_batch(B.d_a[:10], torch.zeros(1, dtype=torch.int64), B.d_b[:10], torch.zeros(1, dtype=torch.int64))
    assert (ab == -1).all() and ba is None and (s1 == int_min).all()
    with pytest.raises(RuntimeError, match="n_pairs"):
        feats.match_q8_batch(B.d_a, B.d_oa, B.d_b, B.d_ob[:-1])
    with pytest.raises(RuntimeError, match="uint8"):
        feats.match_q8_batch(B.d_a.float(), B.d_oa, B.d_b, B.d_ob)
    with pytest.raises(RuntimeError, match="uint8"):
        feats.match_q8_batch(B.d_a.reshape(-1, 64), B.d_oa, B.d_b, B.d_ob)


# --- 8: frames to verified matches in 8 bits --------------------------------------------------------------------------
H_TRUE = [np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]]),      # of test_gpu_match_pairs.py::_frames
          np.array([[1.03, -0.05, -12.0], [0.03, 1.02, 9.0], [-3e-5, 2e-5, 1.0]]),
          np.array([[0.98, 0.02, 31.0], [-0.01, 0.94, -18.0], [2e-5, 5e-5, 1.0]])]


def _frames():
    """the 1024 x 768 centre crop of houses.jpg and three perspective warps of it (PIL images)"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    out = [crop]
    for h_true in H_TRUE:
        hi = np.linalg.inv(h_true)
        hi = hi / hi[2, 2]
        out.append(crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC))
    return out


def test_frames_to_verified_matches_in_8_bits(torch):
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_sequence as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    F, seed = len(frames), 21
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=F)
    h = feats._inner
    kps, desc, o, m_ab, ver, model, per_pair = ex.match_sequence(frames, seed=seed, feats=feats, q8=True)
    _, _, o32, _, _, _, per_pair32 = ex.match_sequence(frames, seed=seed, feats=feats)
    torch.cuda.synchronize()
    assert torch.equal(o, o32)
    q = feats.quantize(desc)
    torch.cuda.synchronize()
    o_h, m_ab, ver, model = o.cpu().numpy(), m_ab.cpu().numpy(), ver.cpu().numpy(), model.cpu().numpy()
    per_pair, per_pair32, k_h = per_pair.cpu().numpy(), per_pair32.cpu().numpy(), kps.cpu().numpy()
    assert m_ab.shape == ver.shape == (int(o_h[-1]),) and (m_ab[o_h[F - 1]:] == -1).all()      # the last frame has no successor
    corners = np.array([[0, 0], [1024, 0], [1024, 768], [0, 768]], np.float64)
    for p in range(F - 1):
        sa, sb = slice(o_h[p], o_h[p + 1]), slice(o_h[p + 1], o_h[p + 2])
        # (a) the same device rows through the single-pair q8 calls: match, the mutual rule, verify with seed + p
        f_ab, s1, s2 = single(h, torch, q[sa], q[sb])
        f_ba, _, _ = single(h, torch, q[sb], q[sa])
        w_ab, _ = pcases.mutual(f_ab, f_ba, [0, len(f_ab)], [0, len(f_ba)])
        assert np.array_equal(m_ab[sa], w_ab), p
        assert per_pair[p][0] == (s1.astype(np.float32) * np.float32(0.8) > s2.astype(np.float32)).sum() == (f_ab >= 0).sum(), p
        assert per_pair[p][1] == (w_ab >= 0).sum(), p
        ka, kb = k_h[sa], k_h[sb]
        h1, v1, st1 = h.verify_homography(ka, kb, w_ab, 2048, 3.0, seed + p, 0)
        assert np.array_equal(model[p].reshape(-1).view(np.uint32), h1.reshape(-1).view(np.uint32)) and np.array_equal(ver[sa], v1), p
        assert per_pair[p][2] == int(st1[0]) == (v1 >= 0).sum() and st1[2] != href.INVALID
        i = np.flatnonzero(v1 >= 0)
        assert len(i) >= 4
        print(f"[q8_pairs] frame {p} -> {p + 1} ({len(ka)} x {len(kb)}): q8 {per_pair[p][0]} ratio-test matches, {per_pair[p][1]} mutual, "
              f"{per_pair[p][2]} verified; f32 {per_pair32[p][0]}, {per_pair32[p][1]}, {per_pair32[p][2]}")
        if p == 0:      # the bars of test_end_to_end_on_a_perspective_warp_of_a_photograph: frame 0 -> frame 1 is its warp
            err = np.linalg.norm(href.map_points(H_TRUE[0], ka[i, :2]) - kb[v1[i], :2], axis=1)
            within = (err < 3.0).mean()
            img_err = np.abs(href.map_points(model[0].astype(np.float64), corners) - href.map_points(H_TRUE[0], corners)).max()
            print(f"[q8_pairs] pair 0: {within:.1%} of the verified matches within 3 px of the true map; H vs the true map at the "
                  f"image corners: {img_err:.2f} px")
            assert within >= 0.98, within
            assert img_err < 1.5, img_err


def test_match_sequence_example_q8(tmp_path):
    """examples/match_sequence.py --q8 and --q8 --guided on four generated frames: one line per pair, exit status 0."""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_sequence.py")
    for extra in (["--q8"], ["--q8", "--guided"]):
        out = subprocess.run([sys.executable, exe] + extra + paths, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        print("\n".join(lines))
        assert lines[0].startswith("Extracted ") and len(lines) == 4
        for t, line in enumerate(lines[1:]):
            w = line.replace(",", "").split()
            assert line.startswith(f"Pair {t + 1} -> {t + 2}: ") and w[5] == "matches" and w[7] == "mutual"
            raw, mutual, inl = int(w[4]), int(w[6]), int(w[8])
            assert raw >= mutual >= inl >= 8, line
            assert ("guided" in line) == ("--guided" in extra), line
