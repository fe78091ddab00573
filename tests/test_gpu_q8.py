"""8-bit descriptors on the GPU (include/lf_mkd.h, "8-bit descriptors"): the device quantiser against its numpy restatement
and the int8 matcher against an integer matrix product (tests/q8_cases.py) -- every comparison is ==, there are no
tolerances -- then, end to end on a photograph, the 8-bit decisions against the f32 matcher's under the derived error bound."""
import glob
import os

import numpy as np
import pytest

import q8_cases as cases
from conftest import GOLDEN, ROOT, _report

import local_features_python as lfp

pytestmark = pytest.mark.gpu

GUARD = 8           # sentinel words in front of and behind every output
SENTINEL = -7


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
    """{(na, nb, seed): (qa, qb, (match, best, second))}: computed once, never changed"""
    out = {}
    for na, nb, seed in cases.shape_cases():
        qa, qb = cases.quantized_sets(na, nb, seed)
        out[(na, nb, seed)] = (qa, qb, cases.match_q8(qa, qb))
    return out


class Out:
    """match / best / second on the device, each between GUARD sentinel words"""

    def __init__(self, torch, na, scores=True):
        self.na = na
        self.bufs = [torch.full((na + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3 if scores else 1)]

    def ptr(self, k):
        return self.bufs[k].data_ptr() + 4 * GUARD if k < len(self.bufs) else None

    def result(self):
        """the outputs as numpy arrays, after checking that the guard words are untouched"""
        got = []
        for b in self.bufs:
            h = b.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.na:] == SENTINEL).all()
            got.append(h[GUARD:GUARD + self.na].copy())
        return got


def run(handle, torch, qa, qb, ratio=cases.RATIO, lo=None, hi=None, scores=True, stream=None, out=None, dev=None):
    """lf_mkd_match_q8_device on numpy rows -> [match, best, second] (or [match])"""
    d_a, d_b = dev if dev is not None else (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda())
    d_lo = torch.from_numpy(np.asarray(lo, np.uint32).view(np.int32)).cuda() if lo is not None else None
    d_hi = torch.from_numpy(np.asarray(hi, np.uint32).view(np.int32)).cuda() if hi is not None else None
    out = out or Out(torch, len(qa), scores)
    torch.cuda.synchronize()
    handle.match_q8_device(d_a.data_ptr(), len(qa), d_b.data_ptr(), len(qb), out.ptr(0), float(ratio),
                           d_lo.data_ptr() if lo is not None else None, d_hi.data_ptr() if hi is not None else None,
                           out.ptr(1), out.ptr(2), stream)
    torch.cuda.synchronize()
    return out.result()


def same(got, want, what):
    for name, g, w in zip(("match", "best", "second"), got, want):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


# --- the quantiser ----------------------------------------------------------------------------------------------------
def _golden_rows():
    return np.concatenate([np.load(f)["desc_shader"] for f in sorted(glob.glob(os.path.join(GOLDEN, "patches_*.npz")))]).astype(np.float32)


def _quantize_device(handle, torch, x, scale):
    n = len(x)
    d_x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    d_q = torch.zeros((n + 1, 128), dtype=torch.uint8, device="cuda")       # (byte 0 never occurs: the guard row stays 0)
    torch.cuda.synchronize()
    handle.quantize_descriptors_device(d_x.data_ptr(), n, d_q.data_ptr(), float(scale))
    q = d_q.cpu().numpy()
    assert (q[n] == 0).all(), "the row behind d_q[n] was written"
    return q[:n]


@pytest.mark.parametrize("scale", [256.0, 100.0])
def test_quantiser_equals_its_restatement(handle, torch, scale):
    rng = np.random.default_rng(5)
    rand = (rng.normal(size=(1000, 128)) * rng.uniform(0.01, 0.3, (1000, 1))).astype(np.float32)
    golden = _golden_rows()
    assert golden.shape == (78, 128)
    for what, x in (("edges", cases.edge_values(scale)), ("golden", golden), ("random", rand), ("n=1", rand[:1]), ("n=63", rand[:63]),
                    ("n=64", rand[:64]), ("n=65", rand[:65])):
        got, want = _quantize_device(handle, torch, x, scale), cases.quantize(x, scale)
        assert np.array_equal(got, want), (what, scale, np.argwhere(got != want)[:5])
        assert np.array_equal(handle.quantize(x, scale), want), (what, scale, "host form")
    assert got.min() >= 1
    # scale 0 is the default, 256
    assert np.array_equal(_quantize_device(handle, torch, golden, 0.0), cases.quantize(golden, 256.0))


def test_quantize_faces(torch):
    feats = lfp.LocalFeatures(64, 64, 16)
    x = _golden_rows()
    want = cases.quantize(x)
    q = feats.quantize(x)
    assert isinstance(q, np.ndarray) and q.dtype == np.uint8 and np.array_equal(q, want)
    t = feats.quantize(torch.from_numpy(x).cuda().double())                  # any float dtype, on the device
    torch.cuda.synchronize()
    assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), want)
    assert feats.quantize(torch.zeros((0, 128))).shape == (0, 128)
    d = feats.dequantize(t)
    assert d.is_cuda and np.array_equal(d.cpu().numpy(), feats.dequantize(want))
    pairs, best, second = feats.match_q8(q[:40], t[40:], scores=True)        # numpy against a device tensor
    m, b, s = cases.match_q8(want[:40], want[40:])
    assert pairs == [(int(i), int(j)) for i, j in enumerate(m) if j >= 0] and np.array_equal(best, b) and np.array_equal(second, s)
    lo, hi = np.zeros(40, np.uint32), np.full(40, 5, np.uint32)
    m, _, _ = cases.match_q8(want[:40], want[40:], 0.0, lo, hi)
    assert feats.match_q8(q[:40], q[40:], ratio=0.0, exclude=(lo, hi)) == [(i, int(j)) for i, j in enumerate(m)]
    assert feats.match_q8(q[:0], q) == []


# --- the matcher ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.shape_cases(), ids=lambda c: f"{c[0]}x{c[1]}")
def test_matcher_equals_the_integer_product(handle, torch, references, case):
    qa, qb, want = references[case]
    same(run(handle, torch, qa, qb), want, case)
    assert (want[0] >= 0).any() or len(qa) < 30


def _smallest_split_shape():
    """the smallest (na, nb) for which the plan has at least two a blocks AND at least two b splits"""
    na = next(n for n in range(1, 1 << 16) if lfp.match_q8_plan(n, 2)[0] >= 2)
    nb = next(n for n in range(2, 1 << 16) if lfp.match_q8_plan(na, n)[1] >= 2)
    return na, nb


def test_two_blocks_and_two_splits(handle, torch):
    na, nb = _smallest_split_shape()
    a_blocks, splits, scratch = lfp.match_q8_plan(na, nb)
    assert a_blocks >= 2 and splits >= 2 and scratch > 0
    assert lfp.match_q8_plan(na - 1, nb)[0] < 2 and lfp.match_q8_plan(na, nb - 1)[1] < 2
    qa, qb = cases.quantized_sets(na, nb, 3100)
    same(run(handle, torch, qa, qb), cases.match_q8(qa, qb), (na, nb))
    lo, hi = cases.random_ranges(na, nb, 3101)
    same(run(handle, torch, qa, qb, lo=lo, hi=hi), cases.match_q8(qa, qb, cases.RATIO, lo, hi), (na, nb, "ranges"))


def test_ties_go_to_the_highest_index(handle, torch):
    # every b row twice, n rows apart: across a tile border (n = 48), within a tile (n = 7), across LDS stages and b splits
    for n, na in ((7, 20), (48, 70), (1000, 300)):
        qa, b0 = cases.quantized_sets(na, n, 3200 + n)
        qb = np.concatenate([b0, b0])
        if n == 1000:
            a_blocks, splits, _ = lfp.match_q8_plan(na, len(qb))
            per = -(-((len(qb) + 31) // 32) // splits)
            assert splits >= 2 and per * 32 < n + 1, "a row and its copy must lie in different splits"
        want = cases.match_q8(qa, qb, 0.0)
        assert (want[1] == want[2]).all() and (want[0] >= n).all()
        same(run(handle, torch, qa, qb, ratio=0.0), want, ("duplicates", n))
        same(run(handle, torch, qa, qb), cases.match_q8(qa, qb), ("duplicates, ratio test", n))
        # with the copies at the higher indices excluded the same rows win at the lower ones
        lo, hi = np.full(na, n, np.uint32), np.full(na, 2 * n, np.uint32)
        same(run(handle, torch, qa, qb, ratio=0.0, lo=lo, hi=hi), cases.match_q8(qa, qb, 0.0, lo, hi), ("lower copy", n))
    # the extreme sums: all-255 rows against all-255 and all-1 rows are +-128 * 127^2 -- sign and overflow
    qa = np.full((33, 128), 255, np.uint8)
    qa[1::2] = 1
    qb = np.full((70, 128), 1, np.uint8)
    qb[[3, 40, 69]] = 255
    want = cases.match_q8(qa, qb, 0.0)
    assert set(want[1].tolist()) == {2064512} and set(want[2].tolist()) == {2064512} and set(want[0].tolist()) == {69, 68}
    same(run(handle, torch, qa, qb, ratio=0.0), want, "extremes")
    qb[:] = 1
    qb[5] = 255
    want = cases.match_q8(qa, qb, 0.9)
    assert set(want[2][::2].tolist()) == {-2064512} and set(want[0][::2].tolist()) == {5}
    same(run(handle, torch, qa, qb, ratio=0.9), want, "extremes, one positive")


def test_exclusion_ranges(handle, torch):
    na, nb, seed = 513, 1025, 3300
    qa, qb = cases.quantized_sets(na, nb, seed)
    lo, hi = cases.random_ranges(na, nb, seed + 1)
    lo[5], hi[5] = 1, nb              # exactly one candidate left: the first row ...
    lo[6], hi[6] = 0, nb - 1          # ... the last row
    lo[7], hi[7] = 0, nb              # none
    lo[8], hi[8] = 0, 0xFFFFFFFF      # none, a bound beyond nb
    lo[9], hi[9] = 40, 30             # an inverted range excludes nothing
    for ratio in (cases.RATIO, 0.0):
        want = cases.match_q8(qa, qb, ratio, lo, hi)
        assert want[0][5] == 0 and want[0][6] == nb - 1 and want[2][5] == want[2][6] == cases.INT32_MIN
        assert want[0][7] == want[0][8] == -1 and want[1][7] == want[2][7] == want[1][8] == cases.INT32_MIN
        same(run(handle, torch, qa, qb, ratio, lo, hi), want, ("ranges", ratio))
    # a range that removes the best candidate changes the answer
    base = cases.match_q8(qa, qb, 0.0)
    lo2, hi2 = base[0].astype(np.uint32), base[0].astype(np.uint32) + 1
    want = cases.match_q8(qa, qb, 0.0, lo2, hi2)
    assert (want[0] != base[0]).all() and np.array_equal(want[1], base[2])
    same(run(handle, torch, qa, qb, 0.0, lo2, hi2), want, "best removed")


def test_optional_outputs_repeatability_and_capture(handle, torch, references):
    for case in ((513, 1025, 3004), (32, 32, 3002)):                         # a merged plan and a one-split plan
        qa, qb, want = references[case]
        assert (lfp.match_q8_plan(case[0], case[1])[1] == 1) == (case[0] == 32)
        # NULL d_best / d_second; ratio = 0: the best index as is
        assert np.array_equal(run(handle, torch, qa, qb, scores=False)[0], want[0])
        got0 = run(handle, torch, qa, qb, ratio=0.0)
        same(got0, cases.match_q8(qa, qb, 0.0), (case, "ratio 0"))
        assert (got0[0] >= 0).all()
        # the caller's stream; two runs of one call give the same bits
        dev = (torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda())
        s = torch.cuda.Stream()
        first = run(handle, torch, qa, qb, stream=s.cuda_stream, dev=dev)
        same(first, want, (case, "stream"))
        same(run(handle, torch, qa, qb, stream=s.cuda_stream, dev=dev), first, (case, "again"))
        # a warmed-up call captured in a graph (a linear chain) replays to the same bits
        out = Out(torch, len(qa))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            handle.match_q8_device(dev[0].data_ptr(), len(qa), dev[1].data_ptr(), len(qb), out.ptr(0), float(cases.RATIO), None, None,
                                   out.ptr(1), out.ptr(2), torch.cuda.current_stream().cuda_stream)
        for b in out.bufs:
            b.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(out.result(), want, (case, "replay"))
        # the host form
        assert np.array_equal(handle.match_q8(qa, qb, float(cases.RATIO)), want[0])
    # na == 0 writes nothing
    out = Out(torch, 4)
    handle.match_q8_device(None, 0, None, 5, out.ptr(0), 0.8, None, None, out.ptr(1), out.ptr(2))
    assert all((b == SENTINEL).all() for b in out.bufs)


# --- end to end -------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_match_guided.py::_frames


def _frames():
    """the 1024 x 768 centre crop of houses.jpg and its perspective warp, as test_gpu_match_guided.py builds them"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    hi = np.linalg.inv(H_TRUE)
    hi = hi / hi[2, 2]
    return [crop, crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC)]


def pair_bound(a, qa, b, qb, scale):
    """E[i, j] >= |s(i, j) / scale^2 - a_i . b_j|, element by element: with q = x scale + e,
    q_a q_b / scale^2 - a b = (a e_b + b e_a) / scale + e_a e_b / scale^2, and |e| <= ebar = 1/2 for an element that does
    not saturate, |q - x scale| (the clamp's error) for one that does.  So
    E[i, j] = sum_k (|a_ik| ebar_bjk + |b_jk| ebar_aik) / scale + sum_k ebar_aik ebar_bjk / scale^2,
    which for two rows without a saturated element IS the header's (|a|_1 + |b|_1) / (2 scale) + 128 / (4 scale^2), and for a
    pair with a saturated element k0 is that plus about |other row's element k0| * (clamp error) / scale.
    Returns (E [na, nb], ebar_a, ebar_b)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ebar_a = np.maximum(0.5, np.abs(qa.astype(np.float64) - 128 - a * scale))
    ebar_b = np.maximum(0.5, np.abs(qb.astype(np.float64) - 128 - b * scale))
    E = (np.abs(a) @ ebar_b.T + ebar_a @ np.abs(b).T) / scale + ebar_a @ ebar_b.T / scale ** 2
    return E, ebar_a, ebar_b


def test_decisions_on_a_photograph_differ_only_within_the_bound(torch):
    """Detect and describe the crop and its warp, match with lf_mkd_match_device, quantise at 256 and match with
    lf_mkd_match_q8_device.  A row whose 8-bit decision differs from the f32 decision must be a near-tie of the f32 scores:
    best - second <= 2 E (another index), or |best * ratio - second| <= (1 + ratio) E (another verdict on the same index),
    E = the row's bound of |s / scale^2 - a.b| against any b row.
    For rows without a saturated element E is the header's (|a|_1 + |b|_1) / (2 scale) + 128 / (4 scale^2) with the largest
    |b|_1; the few pairs with a saturated element get pair_bound's per-element form of the same derivation, and E of a row is
    the maximum over b.  The pairs whose bound is not the header's are counted and must be few (under 1 %), and so must the
    saturated rows.  Every pair's error is also checked against its own bound.
    Derived, not measured: a wrong kernel fails the exact tests above, this one fails only if quantisation is worse than its
    bound.  The share of differing rows, the largest observed error and the range of E are reported, not gated.
    (On the MI355X: 2375 x 2380 rows, 4 decisions differ; the figures are in DESIGN.md 6e.)"""
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, n_scales=5, max_frames=2)
    h = feats._inner
    cap = 6000
    d_img = torch.from_numpy(frames).cuda()
    kps = torch.empty((cap, 5), device="cuda")
    fid = torch.empty((cap,), dtype=torch.int32, device="cuda")
    desc = torch.empty((cap, 128), device="cuda")
    m, _, dropped = h.detect_frames_device(d_img.data_ptr(), 2, 1024, 768, 2000, 0.0, kps.data_ptr(), fid.data_ptr(),
                                           desc.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    assert dropped == 0
    n0 = int((fid[:m] == 0).sum())
    d_a, d_b = desc[:n0].contiguous(), desc[n0:m].contiguous()
    na, nb = n0, m - n0
    assert na > 1000 and nb > 1000
    ratio = float(cases.RATIO)
    f_m = torch.empty((na,), dtype=torch.int32, device="cuda")
    f_1, f_2 = torch.empty((na,), device="cuda"), torch.empty((na,), device="cuda")
    torch.cuda.synchronize()
    h.match_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, f_m.data_ptr(), ratio, None, None, f_1.data_ptr(), f_2.data_ptr())
    q_a, q_b = feats.quantize(d_a), feats.quantize(d_b)
    torch.cuda.synchronize()
    out = Out(torch, na)
    h.match_q8_device(q_a.data_ptr(), na, q_b.data_ptr(), nb, out.ptr(0), ratio, None, None, out.ptr(1), out.ptr(2))
    got = out.result()
    a, b = d_a.cpu().numpy(), d_b.cpu().numpy()
    qa, qb = q_a.cpu().numpy(), q_b.cpu().numpy()
    # the device pipeline is the restatement's, on these rows too
    assert np.array_equal(qa, cases.quantize(a)) and np.array_equal(qb, cases.quantize(b))
    same(got, cases.match_q8(qa, qb, ratio), "photograph")
    f_m, f_1, f_2 = f_m.cpu().numpy(), f_1.cpu().numpy().astype(np.float64), f_2.cpu().numpy().astype(np.float64)
    scale = float(cases.SCALE)
    Eij, ebar_a, ebar_b = pair_bound(a, qa, b, qb, scale)
    sat_a, sat_b = (ebar_a > 0.5).any(1), (ebar_b > 0.5).any(1)
    assert np.array_equal(sat_a, cases.saturated(a)) and np.array_equal(sat_b, cases.saturated(b))
    l1_a, l1_b = np.abs(a.astype(np.float64)).sum(1), np.abs(b.astype(np.float64)).sum(1)
    header = cases.error_bound(l1_a[:, None], l1_b[None, :])
    clean = ~sat_a[:, None] & ~sat_b[None, :]
    # for every pair of unsaturated rows the bound IS the issue's, and saturation only ever widens it
    assert clean.mean() >= 0.99 and np.allclose(Eij[clean], header[clean], rtol=1e-12, atol=0) and (Eij >= header * (1 - 1e-12)).all()
    assert sat_a.mean() <= 0.01 and sat_b.mean() <= 0.01, (int(sat_a.sum()), int(sat_b.sum()))
    # every pair against its own bound
    true = a.astype(np.float64) @ b.astype(np.float64).T
    pair_err = np.abs(cases.similarities(qa, qb) / scale ** 2 - true)
    assert (pair_err <= Eij).all(), float((pair_err - Eij).max())
    E = Eij.max(1)
    plain = cases.error_bound(l1_a, l1_b.max())              # the issue's E: the row's |a|_1 and the largest |b|_1
    widened = E > plain * (1 + 1e-12)
    assert np.allclose(E[~widened], plain[~widened], rtol=1e-12, atol=0)      # every other row: the issue's E itself
    err = max(np.abs(got[1] / scale ** 2 - f_1).max(), np.abs(got[2] / scale ** 2 - f_2).max())
    diff = np.flatnonzero(got[0] != f_m)
    _report(f"[q8] crop -> warp of houses.jpg, {na} x {nb} rows, scale 256: {len(diff)} of {na} decisions differ from the f32 "
            f"matcher's ({len(diff) / na:.2%}; accepted: f32 {(f_m >= 0).sum()}, q8 {(got[0] >= 0).sum()}); largest "
            f"|s / scale^2 - a.b| over all pairs {pair_err.max():.4f}, of best / second against the f32 scores {err:.4f}; "
            f"the issue's E {plain.min():.4f} .. {plain.max():.4f}, E used {E.min():.4f} .. {E.max():.4f}; rows with a "
            f"saturated element: a {int(sat_a.sum())}, b {int(sat_b.sum())}; pairs not under the header's bound "
            f"{(~clean).mean():.3%}; a rows whose E exceeds the issue's {int(widened.sum())} (by at most "
            f"{(E / plain).max():.2f} x, median of those {np.median((E / plain)[widened]) if widened.any() else 1.0:.3f} x); "
            f"E of the differing rows {[round(float(E[i]), 4) for i in diff]} against the issue's "
            f"{[round(float(plain[i]), 4) for i in diff]}")
    for i in diff:
        near_index = f_1[i] - f_2[i] <= 2 * E[i]
        near_accept = abs(f_1[i] * ratio - f_2[i]) <= (1 + ratio) * E[i]
        assert near_index or near_accept, (i, got[0][i], f_m[i], f_1[i], f_2[i], E[i])
    # (1e-6: the f32 matcher's own scores are within ~1e-7 of the dot product, include/lf_mkd.h)
    assert (np.abs(got[1] / scale ** 2 - f_1) <= E + 1e-6).all() and (np.abs(got[2] / scale ** 2 - f_2) <= E + 1e-6).all()


def test_match_images_example_q8(torch, tmp_path, capsys):
    """examples/match_images.py --q8: the flag reaches match_images(q8=True), both directions are lf_mkd_match_q8 on the
    quantised descriptors, and the printed lines are those of the default path."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_images as ex
    paths = []
    for k, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{k}.png"))
        f.save(paths[-1])
    img1, img2 = ex.load_gray(paths[0]), ex.load_gray(paths[1])
    kp1, kp2, d1, d2, m12, m21 = ex.match_images(img1, img2, q8=True)
    assert len(kp1) > 1000 and len(kp2) > 1000
    q1, q2 = cases.quantize(d1), cases.quantize(d2)
    for got, (x, y) in ((m12, (q1, q2)), (m21, (q2, q1))):
        want = cases.match_q8(x, y)[0]
        assert got == [(int(i), int(j)) for i, j in enumerate(want) if j >= 0]
    assert len(m12) > 300
    argv = sys.argv
    try:
        sys.argv = ["match_images.py", "--q8", paths[0], paths[1], str(tmp_path / "out.png")]
        assert ex.main() == 0
    finally:
        sys.argv = argv
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"Extracted {len(kp1)} and {len(kp2)} keypoints", f"Matching 1 -> 2: {len(m12)} matches",
                     f"Matching 2 -> 1: {len(m21)} matches"], lines
    assert os.path.getsize(tmp_path / "out.png") > 0
