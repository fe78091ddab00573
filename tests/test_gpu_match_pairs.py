"""The batched pair matcher on the GPU (lf_mkd_match_pairs_device, LocalFeatures.match_batch): every pair of a ragged batch
decided bit for bit as the single-pair call decides it, and as the oracle does; ties, the mutual filter, the copy-free
sequence layout, shape independence, graph capture, and the whole device pipeline from frames to verified matches."""
import os
import subprocess
import sys

import numpy as np
import pytest

import homography_ref as href
import match_pairs_cases as cases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


class Batch:
    """The pairs' rows on the device in the verifiers' layout, and outputs pre-filled with sentinels (-7 / NaN)."""

    def __init__(self, torch, pairs, lead=(0, 0), trail=(0, 0)):
        self.pairs = pairs
        self.a, self.oa, self.b, self.ob = cases.concatenate(pairs, lead, trail)
        self.d_a, self.d_b = torch.from_numpy(self.a).cuda(), torch.from_numpy(self.b).cuda()
        self.d_oa, self.d_ob = torch.from_numpy(self.oa).cuda(), torch.from_numpy(self.ob).cuda()
        self.torch = torch

    def outputs(self):
        t = self.torch
        return (t.full((len(self.a),), -7, dtype=t.int32, device="cuda"), t.full((len(self.b),), -7, dtype=t.int32, device="cuda"),
                t.full((len(self.a),), np.nan, device="cuda"), t.full((len(self.a),), np.nan, device="cuda"))

    def run(self, handle, out, ratio=0.8, flags=0, both=True, scores=True, stream=None, offsets=None, n_pairs=None):
        ab, ba, s1, s2 = out
        d_oa, d_ob = offsets if offsets is not None else (self.d_oa, self.d_ob)
        handle.match_pairs_device(self.d_a.data_ptr(), d_oa.data_ptr(), len(self.a), self.d_b.data_ptr(), d_ob.data_ptr(),
                                  len(self.b), len(self.pairs) if n_pairs is None else n_pairs, ab.data_ptr(),
                                  ba.data_ptr() if both else None, ratio, flags, s1.data_ptr() if scores else None,
                                  s2.data_ptr() if scores else None, stream)

    def call(self, handle, **kw):
        out = self.outputs()
        self.run(handle, out, stream=self.torch.cuda.current_stream().cuda_stream, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]


def single(handle, torch, x, y, ratio=0.8):
    """lf_mkd_match_device on one pair's rows: (match, best, second), or -1 / -inf where the call refuses the pair."""
    if len(x) == 0 or len(y) < 2:
        return np.full(len(x), -1, np.int32), np.full(len(x), -np.inf, np.float32), np.full(len(x), -np.inf, np.float32)
    d_x, d_y = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()
    m = torch.empty(len(x), dtype=torch.int32, device="cuda")
    s1, s2 = torch.empty(len(x), device="cuda"), torch.empty(len(x), device="cuda")
    handle.match_device(d_x.data_ptr(), len(x), d_y.data_ptr(), len(y), m.data_ptr(), ratio, None, None, s1.data_ptr(),
                        s2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return m.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def ragged(torch):
    return Batch(torch, cases.ragged_batch(), lead=(5, 19), trail=(7, 3))


@pytest.fixture(scope="module")
def ragged_out(ragged, handle):
    """the unfiltered result of the ragged batch, both directions with best / second"""
    return ragged.call(handle)


def test_batched_equals_single_bit_for_bit(ragged, ragged_out, handle, torch):
    assert "LF_MKD_MATCH" not in os.environ          # the single-pair call picks its form by size: the one-launch form here
    one_way = ragged.call(handle, both=False)
    no_scores = ragged.call(handle, scores=False)
    B = ragged
    for out, both, scores in ((ragged_out, True, True), (one_way, False, True), (no_scores, True, False)):
        ab, ba, s1, s2 = out
        for p, (a, b, kind) in enumerate(B.pairs):
            sa, sb = slice(B.oa[p], B.oa[p + 1]), slice(B.ob[p], B.ob[p + 1])
            if kind == "degenerate":                  # a direction the single-pair call refuses: -1 / -inf, whatever the ratio
                assert len(b) >= 2 or ((ab[sa] == -1).all() and (not scores or ((s1[sa] == -np.inf).all() and (s2[sa] == -np.inf).all()))), p
                assert not both or len(a) >= 2 or (ba[sb] == -1).all(), p
            if kind != "beyond":                      # (the pair beyond the one-launch form is held to the oracle below)
                assert kind == "degenerate" or cases.small_fits(len(a), len(b))
                m, w1, w2 = single(handle, torch, a, b)
                assert np.array_equal(ab[sa], m), (p, "a -> b")
                if scores:
                    assert np.array_equal(bits(s1[sa]), bits(w1)) and np.array_equal(bits(s2[sa]), bits(w2)), (p, "best / second")
            if both:
                assert kind == "degenerate" or len(a) < 2 or cases.small_fits(len(b), len(a))
                m, _, _ = single(handle, torch, b, a)
                assert np.array_equal(ba[sb], m), (p, "b -> a")
        # rows outside the offsets keep their sentinels; a direction that was not asked for is not written
        assert (ab[:B.oa[0]] == -7).all() and (ab[B.oa[-1]:] == -7).all() and B.oa[0] == 5 and len(ab) - B.oa[-1] == 7
        if both:
            assert (ba[:B.ob[0]] == -7).all() and (ba[B.ob[-1]:] == -7).all()
            assert (ba[B.ob[0]:B.ob[-1]] != -7).all() and (ab[B.oa[0]:B.oa[-1]] != -7).all()
        else:
            assert (ba == -7).all()
        if scores:
            assert np.isnan(s1[:B.oa[0]]).all() and np.isnan(s1[B.oa[-1]:]).all() and np.isnan(s2[:B.oa[0]]).all()
            assert not np.isnan(s1[B.oa[0]:B.oa[-1]]).any() and not np.isnan(s2[B.oa[0]:B.oa[-1]]).any()
        else:
            assert np.isnan(s1).all() and np.isnan(s2).all()
    assert np.array_equal(one_way[0], ragged_out[0]) and np.array_equal(no_scores[0], ragged_out[0])
    assert np.array_equal(no_scores[1], ragged_out[1])
    assert handle.match_overflowed(torch.cuda.current_stream().cuda_stream) == 0      # this form redoes nothing


def test_every_pair_against_the_oracle(ragged, ragged_out, oracle):
    ab, ba, s1, s2 = ragged_out
    B = ragged
    checked = 0
    for p, (a, b, kind) in enumerate(B.pairs):
        if kind == "degenerate":
            continue
        sa, sb = slice(B.oa[p], B.oa[p + 1]), slice(B.ob[p], B.ob[p + 1])
        want, w1, w2 = oracle.match(a, b)
        n_ab = cases.compare(ab[sa], s1[sa], s2[sa], want, w1, w2, cases.RATIO, (p, len(a), len(b), "a -> b"))
        n_ba = 0
        if len(a) >= 2:
            want, w1, w2 = oracle.match(b, a)
            n_ba = cases.compare(ba[sb], None, None, want, w1, w2, cases.RATIO, (p, len(a), len(b), "b -> a"))
        else:
            assert (ba[sb] == -1).all()
        acc = (ab[sa] >= 0).mean()
        print(f"[match_pairs] pair {p} ({len(a)} x {len(b)}): accepted {acc:.1%} a -> b, {(ba[sb] >= 0).mean():.1%} b -> a; "
              f"decisions differing from the oracle's: {n_ab}, {n_ba}")
        if len(a) >= 250:
            assert 0.1 < acc <= 1.0
        checked += 1
    assert checked == len(cases.SIZED) + 1


def test_planted_ties_inside_a_later_pair(handle, torch, oracle):
    """Duplicate rows on both sides of pair 1: with the ratio test off the HIGHEST index among equal maxima wins, in both
    directions and local to the pair."""
    pairs = [cases.descriptor_sets(40, 50, 1), cases.descriptor_sets(300, 280, 2), cases.descriptor_sets(64, 64, 3)]
    a, b = pairs[1]
    b[7], b[19] = b[3].copy(), b[3].copy()
    a[11], a[5] = a[2].copy(), a[2].copy()
    B = Batch(torch, [p + ("sized",) for p in pairs])
    ab, ba, _, _ = B.call(handle, ratio=0.0)
    ab, ba = ab[B.oa[1]:B.oa[2]], ba[B.ob[1]:B.ob[2]]
    w_ab, _, _ = oracle.match(a, b, ratio=0.0)
    w_ba, _, _ = oracle.match(b, a, ratio=0.0)
    assert np.array_equal(ab[[2, 5, 11]], w_ab[[2, 5, 11]]) and np.array_equal(ba[[3, 7, 19]], w_ba[[3, 7, 19]])
    assert ba[3] == ba[7] == ba[19] and ab[2] == ab[5] == ab[11]
    # rows of a that found the triplicated b row report its last copy, rows of b that found the triplicated a row likewise
    assert not np.isin(ab, [3, 7]).any() and not np.isin(ba, [2, 5]).any()
    s_ab, s_ba = oracle.match(a, b, ratio=0.0)[1:], oracle.match(b, a, ratio=0.0)[1:]
    cases.compare(ab, None, None, w_ab, s_ab[0], s_ab[1], np.float32(0.0), "ties, a -> b")
    cases.compare(ba, None, None, w_ba, s_ba[0], s_ba[1], np.float32(0.0), "ties, b -> a")
    # with the ratio test on, a duplicated best is rejected (best * 0.8 > second fails on equal values)
    ab8, ba8, _, _ = B.call(handle)
    assert (ab8[B.oa[1]:B.oa[2]][w_ab == 19] == -1).all() and (ba8[B.ob[1]:B.ob[2]][w_ba == 11] == -1).all()


def test_mutual_filter(ragged, ragged_out, handle):
    ab0, ba0, s1_0, s2_0 = ragged_out
    B = ragged
    ab, ba, s1, s2 = B.call(handle, flags=lfp.MATCH_MUTUAL)
    want_ab, want_ba = cases.mutual(ab0, ba0, B.oa, B.ob)
    assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba)
    assert np.array_equal(bits(s1), bits(s1_0)) and np.array_equal(bits(s2), bits(s2_0))     # best / second are not filtered
    for p, (a, b, kind) in enumerate(B.pairs):
        x, y = ab[B.oa[p]:B.oa[p + 1]], ba[B.ob[p]:B.ob[p + 1]]
        i = np.flatnonzero(x >= 0)
        assert (y[x[i]] == i).all() and (x >= 0).sum() == (y >= 0).sum(), p
        fwd = int((ab0[B.oa[p]:B.oa[p + 1]] >= 0).sum())
        print(f"[match_pairs] pair {p} ({len(a)} x {len(b)}, {kind}): {fwd} forward matches, {len(i)} mutual")
        if kind != "degenerate" and len(a) >= 250:
            assert 0 < len(i) < fwd, (p, len(i), fwd)
    with pytest.raises(RuntimeError, match="match_pairs_device: LF_MKD_MATCH_MUTUAL needs d_match_ba"):
        B.run(handle, B.outputs(), flags=lfp.MATCH_MUTUAL, both=False)


def test_sequence_layout_without_a_copied_row(handle, torch):
    """One descriptor array of 6 frames: frame t against frame t + 1 (five pairs, both directions: ten single-pair calls)
    through the shifted view of the same array, and through the array itself with the next frames' offsets."""
    sizes = [300, 17, 450, 233, 64, 129]
    rng = np.random.default_rng(31)
    base = cases.unit(rng.normal(size=(500, 128)))
    frames = [cases.unit(base[rng.integers(0, 500, n)] + 0.03 * rng.normal(size=(n, 128))) for n in sizes]   # one scene, six views
    desc = np.ascontiguousarray(np.concatenate(frames))
    o = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    F = len(sizes)
    d = torch.from_numpy(desc).cuda()
    results = []
    for view, ob in ((d[o[1]:], o[1:F + 1] - o[1]), (d, o[1:F + 1])):
        oa = o[0:F]
        d_oa, d_ob = torch.from_numpy(np.ascontiguousarray(oa)).cuda(), torch.from_numpy(np.ascontiguousarray(ob)).cuda()
        ab = torch.full((len(desc),), -7, dtype=torch.int32, device="cuda")
        ba = torch.full((view.shape[0],), -7, dtype=torch.int32, device="cuda")
        handle.match_pairs_device(d.data_ptr(), d_oa.data_ptr(), len(desc), view.data_ptr(), d_ob.data_ptr(), view.shape[0], F - 1,
                                  ab.data_ptr(), ba.data_ptr(), 0.8, 0, None, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ab, ba = ab.cpu().numpy(), ba.cpu().numpy()
        for t in range(F - 1):
            m, _, _ = single(handle, torch, frames[t], frames[t + 1])
            assert np.array_equal(ab[o[t]:o[t + 1]], m), t
            m, _, _ = single(handle, torch, frames[t + 1], frames[t])
            assert np.array_equal(ba[ob[t]:ob[t + 1]], m), t
        assert (ab[o[F - 1]:] == -7).all() and (ba[:ob[0]] == -7).all()       # the last frame has no successor, the first no predecessor
        assert (ab >= 0).sum() > 100 and (ba >= 0).sum() > 100
        results.append((ab, ba[ob[0]:]))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


def test_shape_independent_repeatable_and_capturable(ragged, ragged_out, handle, torch):
    B = ragged
    # pair p alone (n_pairs = 1, its two offsets) equals pair p of the batch
    for p in (0, 2, 3, 5, 9, 12, 16):
        off = (B.d_oa[p:p + 2].clone(), B.d_ob[p:p + 2].clone())
        out = B.call(handle, offsets=off, n_pairs=1)
        sa, sb = slice(B.oa[p], B.oa[p + 1]), slice(B.ob[p], B.ob[p + 1])
        assert np.array_equal(out[0][sa], ragged_out[0][sa]) and np.array_equal(out[1][sb], ragged_out[1][sb]), p
        assert np.array_equal(bits(out[2][sa]), bits(ragged_out[2][sa])) and np.array_equal(bits(out[3][sa]), bits(ragged_out[3][sa])), p
        assert (out[0][:B.oa[p]] == -7).all() and (out[0][B.oa[p + 1]:] == -7).all() and (out[1][:B.ob[p]] == -7).all() \
            and (out[1][B.ob[p + 1]:] == -7).all(), p
    # n_pairs == 0 writes nothing
    none = B.call(handle, n_pairs=0)
    assert (none[0] == -7).all() and (none[1] == -7).all() and np.isnan(none[2]).all()
    same = lambda x, y: all(np.array_equal(bits(u), bits(v)) for u, v in zip(x, y))
    for flags in (0, lfp.MATCH_MUTUAL):
        first = B.call(handle, flags=flags)
        assert same(first, B.call(handle, flags=flags))                                # two runs agree
        # a stream of the caller's
        s = torch.cuda.Stream()
        out = B.outputs()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            B.run(handle, out, flags=flags, stream=s.cuda_stream)
        s.synchronize()
        assert same(first, [x.cpu().numpy() for x in out])
        # the handle's own stream (stream = None: the binding waits before and after)
        out = B.outputs()
        B.run(handle, out, flags=flags, stream=None)
        assert same(first, [x.cpu().numpy() for x in out])
        # a captured call replays to the same bits
        out = B.outputs()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            B.run(handle, out, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
        for x, fill in zip(out, (-7, -7, np.nan, np.nan)):
            x.fill_(fill)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(first, [x.cpu().numpy() for x in out])
    assert same(first[2:], ragged_out[2:])


def test_offsets_beyond_the_totals_touch_nothing(handle, torch):
    """Whatever the offsets hold, no row at or beyond a total is read or written: an offset beyond the total counts as the
    total, an inverted pair as an empty one.  (The arrays end where the totals say, inside a larger allocation whose tail
    must keep its sentinel.)"""
    pairs = [cases.descriptor_sets(40, 50, 4) + ("sized",), cases.descriptor_sets(30, 20, 5) + ("sized",)]
    B = Batch(torch, pairs, trail=(40, 40))
    na, nb = int(B.oa[-1]), int(B.ob[-1])                                   # the totals the call is told: the tails lie beyond
    ab, ba, s1, s2 = B.outputs()
    for oa, ob in (([0, 40, 5000], [0, 50, 70]), ([0, 40, 70], [0, 50, 1 << 40]), ([0, 40, 20], [0, 50, 70]),
                   ([1 << 33, 1 << 34, 1 << 35], [0, 50, 70])):
        d_oa, d_ob = torch.tensor(oa, dtype=torch.int64).cuda(), torch.tensor(ob, dtype=torch.int64).cuda()
        for t, fill in zip((ab, ba, s1, s2), (-7, -7, np.nan, np.nan)):
            t.fill_(fill)
        handle.match_pairs_device(B.d_a.data_ptr(), d_oa.data_ptr(), na, B.d_b.data_ptr(), d_ob.data_ptr(), nb, 2, ab.data_ptr(),
                                  ba.data_ptr(), 0.8, lfp.MATCH_MUTUAL, s1.data_ptr(), s2.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (ab[na:] == -7).all() and (ba[nb:] == -7).all() and bool(s1[na:].isnan().all()), (oa, ob)
        if oa[0] == 0:                                                       # pair 0 is intact: decided as alone
            m, _, _ = single(handle, torch, pairs[0][0], pairs[0][1])
            mb, _, _ = single(handle, torch, pairs[0][1], pairs[0][0])
            w_ab, w_ba = cases.mutual(m, mb, [0, 40], [0, 50])
            assert np.array_equal(ab[:40].cpu().numpy(), w_ab) and np.array_equal(ba[:50].cpu().numpy(), w_ba), (oa, ob)
        else:                                                                # no a row is in range: b's rows find no candidates
            assert (ab == -7).all() and (ba[:nb] == -1).all()


def test_match_batch_face(ragged, ragged_out, torch):
    """LocalFeatures.match_batch: tensors of other dtypes and on the host are accepted; the outputs have the stated shapes."""
    B = ragged
    feats = lfp.LocalFeatures(64, 64, 64)
    a64 = torch.from_numpy(B.a).double()                                   # float64 on the host
    oa32 = torch.from_numpy(B.oa).to(torch.int32)                          # int32 on the host
    ab, ba, s1, s2 = feats.match_batch(a64, oa32, B.d_b, B.d_ob.to(torch.int32), both=True)
    torch.cuda.synchronize()
    assert ab.shape == (len(B.a),) and ba.shape == (len(B.b),) and s1.shape == s2.shape == (len(B.a),)
    assert ab.dtype == ba.dtype == torch.int32 and s1.dtype == torch.float32 and ab.is_cuda and ba.is_cuda and s1.is_cuda
    inside_a, inside_b = slice(B.oa[0], B.oa[-1]), slice(B.ob[0], B.ob[-1])
    assert np.array_equal(ab.cpu().numpy()[inside_a], ragged_out[0][inside_a])
    assert np.array_equal(ba.cpu().numpy()[inside_b], ragged_out[1][inside_b])
    assert np.array_equal(bits(s1.cpu().numpy()[inside_a]), bits(ragged_out[2][inside_a]))
    assert (ab[:B.oa[0]] == -1).all() and bool(torch.isinf(s1[:B.oa[0]]).all())       # rows outside every pair: -1 / -inf
    one, none, _, _ = feats.match_batch(B.d_a, B.d_oa, B.d_b, B.d_ob)
    assert none is None and torch.equal(one, ab)
    s = torch.cuda.Stream()
    mab, mba, m1, _ = feats.match_batch(B.d_a, B.d_oa, B.d_b, B.d_ob, mutual=True, stream=s)
    s.synchronize()
    w_ab, w_ba = cases.mutual(ab.cpu().numpy(), ba.cpu().numpy(), B.oa, B.ob)
    assert np.array_equal(mab.cpu().numpy(), w_ab) and np.array_equal(mba.cpu().numpy(), w_ba) and torch.equal(m1, s1)
    # an empty side, no pairs
    e = torch.zeros((0, 128))
    z = torch.zeros(3, dtype=torch.int64)
    ab, ba, s1, s2 = feats.match_batch(e, z, B.d_b[:10], torch.tensor([0, 4, 10]), both=True)
    assert ab.shape == (0,) and ba.shape == (10,) and (ba == -1).all() and s1.shape == (0,)
    ab, ba, _, _ = feats.match_batch(B.d_a[:10], torch.zeros(1, dtype=torch.int64), B.d_b[:10], torch.zeros(1, dtype=torch.int64))
    assert (ab == -1).all() and ba is None
    with pytest.raises(RuntimeError, match="n_pairs"):
        feats.match_batch(B.d_a, B.d_oa, B.d_b, B.d_ob[:-1])


# --- frames to verified matches, on the device ------------------------------------------------------------------------
H_TRUE = [np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]]),      # of test_gpu_homography.py's end-to-end test
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


def test_frames_to_verified_matches_on_the_device(torch):
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    F, seed = len(frames), 21
    feats = lfp.LocalFeatures(1024, 768, 3000, n_scales=5, max_frames=F)
    h = feats._inner
    cap = 3000 * F
    d_img = torch.from_numpy(frames).cuda()
    kps = torch.empty((cap, 5), device="cuda")
    fid = torch.empty((cap,), dtype=torch.int32, device="cuda")
    desc = torch.empty((cap, 128), device="cuda")
    m, _, dropped = h.detect_frames_device(d_img.data_ptr(), F, 1024, 768, 2000, 0.0, kps.data_ptr(), fid.data_ptr(), desc.data_ptr(),
                                           cap, torch.cuda.current_stream().cuda_stream)
    assert dropped == 0
    kps, fid, desc = kps[:m], fid[:m].long(), desc[:m]
    o = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.bincount(fid, minlength=F), 0)])
    n0 = int(o[1])
    assert n0 > 1000
    # pair p = the crop against warp p: the crop's rows repeated per pair, the warps' rows as they lie
    n_pairs = F - 1
    d_a, k_a = desc[:n0].repeat(n_pairs, 1), kps[:n0].repeat(n_pairs, 1)
    oa = torch.arange(n_pairs + 1, device="cuda") * n0
    d_b, k_b, ob = desc[n0:], kps[n0:], o[1:] - o[1]
    ab, ba, _, _ = feats.match_batch(d_a, oa, d_b, ob, mutual=True)
    H, ver, st = feats.verify_homography_batch(k_a, oa, k_b, ob, ab, seed=seed)
    fwd, _, _, _ = feats.match_batch(d_a, oa, d_b, ob)
    torch.cuda.synchronize()
    ab, ver, H, st, fwd = ab.cpu().numpy(), ver.cpu().numpy(), H.cpu().numpy(), st.cpu().numpy(), fwd.cpu().numpy()
    ob_h = ob.cpu().numpy()
    ka, kb_all = kps[:n0].cpu().numpy(), kps[n0:].cpu().numpy()
    corners = np.array([[0, 0], [1024, 0], [1024, 768], [0, 768]], np.float64)
    for p in range(n_pairs):
        # (a) the same device rows through the single-pair calls: match, the mutual rule, verify with seed + p
        xa, xb = desc[:n0].cpu().numpy(), desc[n0:][ob_h[p]:ob_h[p + 1]].cpu().numpy()
        m_ab, _, _ = single(h, torch, xa, xb)
        m_ba, _, _ = single(h, torch, xb, xa)
        w_ab, _ = cases.mutual(m_ab, m_ba, [0, len(xa)], [0, len(xb)])
        mine = ab[p * n0:(p + 1) * n0]
        assert np.array_equal(mine, w_ab) and np.array_equal(fwd[p * n0:(p + 1) * n0], m_ab), p
        kb = kb_all[ob_h[p]:ob_h[p + 1]]
        h1, v1, s1 = h.verify_homography(ka, kb, w_ab, 2048, 3.0, seed + p, 0)
        assert np.array_equal(bits(H[p].reshape(-1)), bits(h1.reshape(-1))) and np.array_equal(ver[p * n0:(p + 1) * n0], v1), p
        assert int(st[p][0]) == int(s1[0]) == (v1 >= 0).sum() and s1[2] != href.INVALID
        # (b), (c) the verified matches against the true map
        i = np.flatnonzero(v1 >= 0)
        err = np.linalg.norm(href.map_points(H_TRUE[p], ka[i, :2]) - kb[v1[i], :2], axis=1)
        within = (err < 3.0).mean()
        img_err = np.abs(href.map_points(H[p].astype(np.float64), corners) - href.map_points(H_TRUE[p], corners)).max()
        print(f"[match_pairs] crop -> warp {p}: {(m_ab >= 0).sum()} ratio-test matches, {(w_ab >= 0).sum()} mutual, {len(i)} verified "
              f"({within:.1%} within 3 px of the true map); H vs the true map at the image corners: {img_err:.2f} px")
        assert len(i) >= 4
        if p == 0:      # the bars of test_end_to_end_on_a_perspective_warp_of_a_photograph, on its warp
            assert within >= 0.98, within
            assert img_err < 1.5, img_err


def test_match_sequence_example(tmp_path):
    """examples/match_sequence.py on four generated frames: one line per pair, exit status 0."""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_sequence.py")
    for extra in ([], ["--fundamental"]):
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
    assert subprocess.run([sys.executable, exe, paths[0]], capture_output=True).returncode == 1
