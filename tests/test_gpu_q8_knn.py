"""k-nearest-neighbour search over 8-bit descriptors on the GPU (include/lf_mkd.h, lf_mkd_knn_q8_device) against its numpy
restatement (tests/q8_knn_cases.py): every comparison is ==, there are no tolerances.  Then, end to end on photographs, the
retrieval example built on it."""
import os
import sys

import numpy as np
import pytest

import q8_cases as cases
import q8_knn_cases as kcases
from conftest import GOLDEN, ROOT, _report

import local_features_python as lfp

pytestmark = pytest.mark.gpu

GUARD = 8           # sentinel words in front of and behind every output
SENTINEL = 0x7F0F0F0F  # above every sum (|s| <= 2 064 512) and every index of these tests


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
    """{(na, nb, seed): (qa, qb, (index, score) at k = 16)}: computed once, never changed.  The first k columns of the k = 16
    table ARE the table at k (the order is total)."""
    out = {}
    for na, nb, seed in kcases.shape_cases():
        qa, qb = cases.quantized_sets(na, nb, seed)
        out[(na, nb, seed)] = (qa, qb, kcases.knn_q8(qa, qb, 16))
    return out


class Out:
    """index / score [na][k] on the device, each between GUARD sentinel words"""

    def __init__(self, torch, na, k, scores=True):
        self.n = na * k
        self.shape = (na, k)
        self.bufs = [torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2 if scores else 1)]

    def ptr(self, j):
        return self.bufs[j].data_ptr() + 4 * GUARD if j < len(self.bufs) else None

    def result(self):
        """the outputs as numpy arrays, after checking that the guard words are untouched and every entry was written"""
        got = []
        for b in self.bufs:
            h = b.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.n:] == SENTINEL).all()
            got.append(h[GUARD:GUARD + self.n].reshape(self.shape).copy())
            assert (got[-1] != SENTINEL).all()       # exactly na * k entries: none was left out
        return got


def run(handle, torch, qa, qb, k, lo=None, hi=None, scores=True, stream=None, out=None, dev=None):
    """lf_mkd_knn_q8_device on numpy rows -> [index, score] (or [index])"""
    d_a, d_b = dev if dev is not None else (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda())
    d_lo = torch.from_numpy(np.asarray(lo, np.uint32).view(np.int32)).cuda() if lo is not None else None
    d_hi = torch.from_numpy(np.asarray(hi, np.uint32).view(np.int32)).cuda() if hi is not None else None
    out = out or Out(torch, len(qa), k, scores)
    torch.cuda.synchronize()
    handle.knn_q8_device(d_a.data_ptr(), len(qa), d_b.data_ptr(), len(qb), k, out.ptr(0), out.ptr(1),
                         d_lo.data_ptr() if lo is not None else None, d_hi.data_ptr() if hi is not None else None, stream)
    torch.cuda.synchronize()
    return out.result()


def same(got, want, what):
    for name, g, w in zip(("index", "score"), got, want):
        assert (w != SENTINEL).all(), (what, name, "the sentinel occurs in the expected output")
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[g != w][:5], w[g != w][:5])


def first(want, k):
    """the k = 16 reference cut to k columns"""
    return [np.ascontiguousarray(w[:, :k]) for w in want]


@pytest.mark.parametrize("k", kcases.KS)
@pytest.mark.parametrize("case", kcases.shape_cases(), ids=lambda c: f"{c[0]}x{c[1]}")
def test_knn_equals_the_integer_product(handle, torch, references, case, k):
    qa, qb, want = references[case]
    want = first(want, k)
    assert want[0].shape == (len(qa), k) and ((want[0] >= 0).sum(1) == min(k, len(qb))).all()      # padded when k > nb
    same(run(handle, torch, qa, qb, k), want, (case, k))
    assert np.array_equal(run(handle, torch, qa, qb, k, scores=False)[0], want[0])                 # d_score = NULL


def _smallest_split_shape(k):
    """the smallest (na, nb) for which the plan has at least two a blocks AND at least two b splits"""
    na = next(n for n in range(1, 1 << 16) if lfp.knn_q8_plan(n, 1, k)[0] >= 2)
    nb = next(n for n in range(1, 1 << 16) if lfp.knn_q8_plan(na, n, k)[1] >= 2)
    return na, nb


def test_two_blocks_and_two_splits(handle, torch):
    k = 16
    na, nb = _smallest_split_shape(k)
    a_blocks, splits, scratch = lfp.knn_q8_plan(na, nb, k)
    assert a_blocks >= 2 and splits >= 2 and scratch > 0
    assert lfp.knn_q8_plan(na - 1, nb, k)[0] < 2 and lfp.knn_q8_plan(na, nb - 1, k)[1] < 2
    qa, qb = cases.quantized_sets(na, nb, 3400)
    same(run(handle, torch, qa, qb, k), kcases.knn_q8(qa, qb, k), (na, nb))
    lo, hi = cases.random_ranges(na, nb, 3401)
    same(run(handle, torch, qa, qb, k, lo, hi), kcases.knn_q8(qa, qb, k, lo, hi), (na, nb, "ranges"))


def test_ties_go_to_the_highest_index(handle, torch):
    # every b row three times, n rows apart: within a tile (n = 7), across a tile border (48), across LDS stages and b splits
    k = 5
    for n, na in ((7, 20), (48, 70), (1000, 300)):
        qa, b0 = cases.quantized_sets(na, n, 3500 + n)
        qb = np.concatenate([b0, b0, b0])
        if n == 1000:
            a_blocks, splits, _ = lfp.knn_q8_plan(na, len(qb), k)
            per = -(-((len(qb) + 31) // 32) // splits)
            assert splits >= 3 and per * 32 < n + 1, "a row and its copies must lie in different splits"
        want = kcases.knn_q8(qa, qb, k)
        index, score = want
        assert (score[:, 0] == score[:, 1]).all() and (score[:, 1] == score[:, 2]).all() and (score[:, 3] == score[:, 4]).all()
        assert (index[:, 0] >= 2 * n).all() and (index[:, 1] == index[:, 0] - n).all() and (index[:, 2] == index[:, 0] - 2 * n).all()
        assert (index[:, 3] >= 2 * n).all() and ((index[:, 4] == index[:, 3] - n) | ((index[:, 4] >= 2 * n) & (index[:, 4] < index[:, 3]))).all()   # (or, where two rows of b0 tie naturally, the other row's highest copy)
        same(run(handle, torch, qa, qb, k), want, ("copies", n))
        # with the copies at the highest indices excluded the same rows lead at the middle ones
        lo, hi = np.full(na, 2 * n, np.uint32), np.full(na, 3 * n, np.uint32)
        want = kcases.knn_q8(qa, qb, k, lo, hi)
        assert (want[0][:, 0] == index[:, 1]).all() and (want[0][:, 1] == index[:, 2]).all()
        same(run(handle, torch, qa, qb, k, lo, hi), want, ("lower copies", n))
    # the extreme sums: all-255 rows against all-255 and all-1 rows are +-128 * 127^2 -- sign, order and the key's bias
    qa = np.full((33, 128), 255, np.uint8)
    qa[1::2] = 1
    qb = np.full((70, 128), 1, np.uint8)
    qb[[3, 40, 69]] = 255
    want = kcases.knn_q8(qa, qb, k)
    assert want[0][0].tolist() == [69, 40, 3, 68, 67] and want[1][0].tolist() == [2064512] * 3 + [-2064512] * 2
    assert want[0][1].tolist() == [68, 67, 66, 65, 64] and want[1][1].tolist() == [2064512] * 5
    same(run(handle, torch, qa, qb, k), want, "extremes")
    qb[:] = 1
    qb[5] = 255
    want = kcases.knn_q8(qa, qb, 2)
    assert want[0][0].tolist() == [5, 69] and want[1][0].tolist() == [2064512, -2064512]
    same(run(handle, torch, qa, qb, 2), want, "extremes, one positive")


def test_exclusion_ranges(handle, torch):
    na, nb, seed, k = 513, 1025, 3600, 8
    qa, qb = cases.quantized_sets(na, nb, seed)
    lo, hi = cases.random_ranges(na, nb, seed + 1)
    lo[4], hi[4] = k - 1, nb          # exactly k - 1 candidates left
    lo[5], hi[5] = 1, nb              # exactly one candidate left: the first row ...
    lo[6], hi[6] = 0, nb - 1          # ... the last row
    lo[7], hi[7] = 0, nb              # none
    lo[8], hi[8] = 0, 0xFFFFFFFF      # none, a bound beyond nb
    lo[9], hi[9] = 40, 30             # an inverted range excludes nothing
    want = kcases.knn_q8(qa, qb, k, lo, hi)
    index, score = want
    assert (index[4, :k - 1] >= 0).all() and (index[4, :k - 1] < k - 1).all() and index[4, k - 1] == -1 and score[4, k - 1] == cases.INT32_MIN
    assert index[5].tolist() == [0] + [-1] * (k - 1) and index[6].tolist() == [nb - 1] + [-1] * (k - 1)
    assert (index[7] == -1).all() and (index[8] == -1).all() and (score[7] == cases.INT32_MIN).all()
    assert np.array_equal(index[9], kcases.knn_q8(qa[9:10], qb, k)[0][0])
    same(run(handle, torch, qa, qb, k, lo, hi), want, "ranges")
    # excluding a row's best shifts every column up by one
    base = kcases.knn_q8(qa, qb, k + 1)
    lo2, hi2 = base[0][:, 0].astype(np.uint32), base[0][:, 0].astype(np.uint32) + 1
    want = kcases.knn_q8(qa, qb, k, lo2, hi2)
    assert np.array_equal(want[0], base[0][:, 1:]) and np.array_equal(want[1], base[1][:, 1:])
    same(run(handle, torch, qa, qb, k, lo2, hi2), want, "best removed")


class MatchOut:
    def __init__(self, torch, na):
        self.bufs = [torch.full((na,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]


@pytest.mark.parametrize("case", [(513, 1025, 3004), (2000, 2000, 3005)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_agreement_with_the_matcher_on_the_device(handle, torch, references, case):
    qa, qb, _ = references[case]
    d_a, d_b = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
    m = MatchOut(torch, len(qa))
    torch.cuda.synchronize()
    handle.match_q8_device(d_a.data_ptr(), len(qa), d_b.data_ptr(), len(qb), m.bufs[0].data_ptr(), 0.0, None, None,
                           m.bufs[1].data_ptr(), m.bufs[2].data_ptr())
    match, best, second = (b.cpu().numpy() for b in m.bufs)
    for k in (2, 16):
        index, score = run(handle, torch, qa, qb, k, dev=(d_a, d_b))
        assert np.array_equal(index[:, 0], match) and np.array_equal(score[:, 0], best) and np.array_equal(score[:, 1], second), (case, k)


def test_repeatability_stream_and_capture(handle, torch, references):
    k = 8
    for case in ((513, 1025, 3004), (32, 32, 3002)):                         # a merged plan and a one-split plan
        qa, qb, want = references[case]
        want = first(want, k)
        assert (lfp.knn_q8_plan(case[0], case[1], k)[1] == 1) == (case[0] == 32)
        # the caller's stream; two runs of one call give the same bits
        dev = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda())
        s = torch.cuda.Stream()
        got = run(handle, torch, qa, qb, k, stream=s.cuda_stream, dev=dev)
        same(got, want, (case, "stream"))
        same(run(handle, torch, qa, qb, k, stream=s.cuda_stream, dev=dev), got, (case, "again"))
        # a warmed-up call captured in a graph (a linear chain) replays to the same bits
        out = Out(torch, len(qa), k)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            handle.knn_q8_device(dev[0].data_ptr(), len(qa), dev[1].data_ptr(), len(qb), k, out.ptr(0), out.ptr(1), None, None,
                                 torch.cuda.current_stream().cuda_stream)
        for b in out.bufs:
            b.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(out.result(), want, (case, "replay"))
        # the host form
        same(handle.knn_q8(qa, qb, k), want, (case, "host form"))
    # na == 0 writes nothing
    out = Out(torch, 4, k)
    handle.knn_q8_device(None, 0, None, 5, k, out.ptr(0), out.ptr(1))
    assert all((b == SENTINEL).all() for b in out.bufs)


def test_the_shared_scratch_is_stream_ordered(handle, torch, references):
    """a match_q8_device call of another size between two knn calls, same handle and stream: neither result changes"""
    k = 16
    qa, qb, want = references[(513, 1025, 3004)]
    qa2, qb2, _ = references[(300, 6000, 3006)]
    want2 = cases.match_q8(qa2, qb2)
    assert lfp.knn_q8_plan(513, 1025, k)[2] > 0 and lfp.match_q8_plan(300, 6000)[2] > 0
    dev = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda())
    dev2 = (torch.from_numpy(qa2).cuda(), torch.from_numpy(qb2).cuda())
    first_out, second_out = Out(torch, len(qa), k), Out(torch, len(qa), k)
    m = MatchOut(torch, len(qa2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    handle.knn_q8_device(dev[0].data_ptr(), len(qa), dev[1].data_ptr(), len(qb), k, first_out.ptr(0), first_out.ptr(1), None, None,
                         s.cuda_stream)
    handle.match_q8_device(dev2[0].data_ptr(), len(qa2), dev2[1].data_ptr(), len(qb2), m.bufs[0].data_ptr(), float(cases.RATIO),
                           None, None, m.bufs[1].data_ptr(), m.bufs[2].data_ptr(), s.cuda_stream)
    handle.knn_q8_device(dev[0].data_ptr(), len(qa), dev[1].data_ptr(), len(qb), k, second_out.ptr(0), second_out.ptr(1), None, None,
                         s.cuda_stream)
    torch.cuda.synchronize()
    same(first_out.result(), want, "before the matcher's call")
    same(second_out.result(), want, "after the matcher's call")
    for g, w in zip((b.cpu().numpy() for b in m.bufs), want2):
        assert np.array_equal(g, w)


def test_faces(torch, references):
    feats = lfp.LocalFeatures(64, 64, 16)
    qa, qb, want = references[(33, 65, 3003)]
    index, score = feats.knn_q8(qa, qb, 5)                                   # numpy in, numpy out
    assert isinstance(index, np.ndarray) and isinstance(score, np.ndarray) and index.dtype == score.dtype == np.int32
    same((index, score), first(want, 5), "numpy")
    t_index, t_score = feats.knn_q8(torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), 5)   # device in, device out
    assert t_index.is_cuda and t_score.is_cuda and t_index.dtype == t_score.dtype == torch.int32 and t_index.shape == (33, 5)
    torch.cuda.synchronize()
    same((t_index.cpu().numpy(), t_score.cpu().numpy()), first(want, 5), "device")
    s = torch.cuda.Stream()
    t_index, _ = feats.knn_q8(torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), 16, stream=s)
    s.synchronize()
    assert np.array_equal(t_index.cpu().numpy(), want[0])
    lo, hi = np.zeros(33, np.uint32), np.full(33, 5, np.uint32)
    same(feats.knn_q8(qa, qb, 3, exclude=(lo, hi)), kcases.knn_q8(qa, qb, 3, lo, hi), "exclude")
    index, score = feats.knn_q8(qa[:0], qb, 4)                               # empty qa
    assert index.shape == score.shape == (0, 4) and index.dtype == np.int32
    with pytest.raises(RuntimeError, match="k must be"):
        feats.knn_q8(qa, qb, 17)


# --- end to end -------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_q8.py


def _frames():
    """the 1024 x 768 centre crop of houses.jpg and its perspective warp, as test_gpu_q8.py builds them"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    hi = np.linalg.inv(H_TRUE)
    hi = hi / hi[2, 2]
    return [crop, crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC)]


def test_find_image_example(torch, tmp_path, capsys):
    """examples/find_image.py: the crop as query against its warp and bird.jpg.  The warp ranks first, the votes are
    rank_images applied to the restatement's k = 8 table of the same quantised rows, and the printed lines are checked."""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import find_image as ex
    crop, warp = _frames()
    paths = [str(tmp_path / "query.png"), str(tmp_path / "warp.png"), os.path.join(GOLDEN, "bird.jpg")]
    crop.save(paths[0])
    warp.save(paths[1])
    images = [ex.load_gray(p) for p in paths]
    votes, offsets, q, pool, index, score = ex.find_image(images[0], images[1:])
    assert len(q) > 1000 and offsets[1] > 1000 and offsets[2] > offsets[1] and len(pool) == offsets[2]
    want = kcases.knn_q8(q, pool, ex.K)
    same((index, score), want, "find_image's table")
    assert np.array_equal(votes, ex.rank_images(want[0], want[1], offsets, ex.RATIO))
    assert votes[0] > votes[1]                                               # the warp ranks first
    _report(f"[q8 knn] find_image: the crop of houses.jpg ({len(q)} keypoints) against its warp ({int(offsets[1])}) and bird.jpg "
            f"({int(offsets[2] - offsets[1])}): votes {votes.tolist()}; nearest neighbours per image "
            f"{np.bincount(np.searchsorted(offsets, index[:, 0], side='right') - 1, minlength=2).tolist()}")
    capsys.readouterr()                                                      # (the report's own line)
    argv = sys.argv
    try:
        sys.argv = ["find_image.py"] + paths
        assert ex.main() == 0
    finally:
        sys.argv = argv
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"Query: {len(q)} keypoints against {int(offsets[2])} in 2 images",
                     f"1. {paths[1]}: {int(votes[0])} votes ({int(offsets[1])} keypoints)",
                     f"2. {paths[2]}: {int(votes[1])} votes ({int(offsets[2] - offsets[1])} keypoints)"], lines
