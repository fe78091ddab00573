"""Feature tracks on the GPU (lf_mkd_build_tracks_device; LocalFeatures.build_tracks): the label, the length and the
conflicting rows of every track equal the numpy restatement's (tests/tracks_cases.py) -- every comparison is ==.  Shapes of
components that stress the lock-free union (chains, stars on one root, cycles), the input conventions, independence of the
edge order and of the split into accumulating calls, graph capture, matched pictures, and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import q8_edges_cases as ecases
import tracks_cases as cases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # entries every output array is longer than needed
SENTINEL = cases.SENTINEL
TILE = lfp.TRACKS_DUP_TILE       # rows one workgroup of the d_track_dup launch owns (include/lf_mkd.h)
LINK = 256                       # layout entries one workgroup of the link launch owns (include/lf_mkd.h, "Launches")
NAMES = ("track", "len", "dup")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


def words(torch, x):
    """uint32 values as an int32 device tensor of their bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint32)).view(np.int32)).cuda()


class Device:
    """a case's arrays on the device; outputs EXTRA entries longer than the pool and sentinel-filled"""

    def __init__(self, torch, handle, case):
        self.torch, self.handle, self.case = torch, handle, case
        self.d_io = torch.from_numpy(np.array(case.io, np.int64)).cuda()
        self.d_ea, self.d_eb = words(torch, case.ea), words(torch, case.eb)
        self.d_la = torch.from_numpy(case.la.astype(np.int64)).cuda()
        self.d_match = torch.from_numpy(np.concatenate([case.match, np.full(EXTRA, 3, np.int32)])).cuda()   # (3: a link, were it read)

    def outputs(self, into=None):
        t = self.torch
        out = [t.full((self.case.total + EXTRA,), SENTINEL, dtype=t.int32, device="cuda") for _ in range(3)]
        if into is not None:
            out[0][:self.case.total] = t.from_numpy(np.asarray(into, np.int32)).cuda()
        return out

    def run(self, out, flags=0, length=True, dup=True, n_edges=None, cap=None, d_match=None, stream=None):
        c = self.case
        self.handle.build_tracks_device(
            self.d_io.data_ptr(), len(c.io) - 1, c.total, self.d_ea.data_ptr(), self.d_eb.data_ptr(), self.d_la.data_ptr(),
            c.cap if cap is None else cap, len(c.ea) if n_edges is None else n_edges,
            (self.d_match if d_match is None else d_match).data_ptr(), out[0].data_ptr(), out[1].data_ptr() if length else None,
            out[2].data_ptr() if dup else None, flags, self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def call(self, into=None, **kw):
        out = self.outputs(into)
        self.torch.cuda.synchronize()
        self.run(out, flags=lfp.TRACKS_ACCUMULATE if into is not None else 0, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]


def tailed(want):
    """a reference (track, len, dup) as the device arrays hold it: int32 bit patterns, the EXTRA entries behind still sentinels"""
    return [np.concatenate([np.asarray(w).astype(np.int64).astype(np.int32), np.full(EXTRA, SENTINEL, np.int32)]) for w in want]


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def check(torch, handle, case, what):
    got = Device(torch, handle, case).call()
    same(got, tailed(case.reference()), what)
    return got


# --- shapes of components ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_chains(descending, torch, handle):
    """one track through 300 small images, the edges in ascending order and from the far end (deep trees before flattening)"""
    case = cases.chain(TILE, descending)
    track, length, dup = check(torch, handle, case, ("chain", descending))
    first = int(case.io[cases.pool(TILE)[2]["small"]])
    assert length[first] == cases.SMALL and (track[:-EXTRA] == first).sum() == cases.SMALL


def test_stars(torch, handle):
    """about 2400 rows of ten images all matched to one row (every link contends on one root); two such stars joined by a single
    link that lies in the last slot of the link grid"""
    one, two = cases.stars(TILE, False), cases.stars(TILE, True)
    got = check(torch, handle, one, "star")
    assert got[1][:-EXTRA].max() > 2000 and (got[1][:-EXTRA] > 1).sum() == 1
    e = len(two.ea) - 1
    grid = two.cap // LINK + len(two.ea)
    assert int(two.la[e]) // LINK + e == grid - 1 and two.match[-1] == 5       # the joining entry's slot is the grid's last
    got2 = check(torch, handle, two, "two stars")
    assert got2[1][:-EXTRA].max() == got[1][:-EXTRA].max() + 1 and (got2[1][:-EXTRA] > 1).sum() == 1
    two.match[-1] = -1                                                       # without that link: two tracks
    apart = check(torch, handle, two, "two stars apart")
    two.match[-1] = 5
    assert (apart[1][:-EXTRA] > 1).sum() == 2


def test_cycles_and_conflicts(torch, handle):
    """consistent 3-cycles; cycles that come back to another row of their first image (dup == 1 exactly there); a self edge that
    links two rows of one image; duplicates that sit in three different dup tiles of the large image"""
    case = cases.cycles(TILE)
    track, length, dup = check(torch, handle, case, "cycles")
    io, _, names = cases.pool(TILE)
    X, L = int(io[names["X"]]), int(io[names["L"]])
    assert (length[X:X + 100] == 3).all() and (dup[X:X + 100] == 0).all()
    assert (length[X + 100:X + 150] == 4).all() and (dup[X + 100:X + 150] == 1).all()
    assert (length[X + 270], dup[X + 270]) == (2, 1) and (length[L + 3], dup[L + 3]) == (4, 2)
    assert dup[:-EXTRA].sum() == 50 + 1 + 2


# --- input conventions ------------------------------------------------------------------------------------------------
def test_input_conventions(torch, handle):
    """random edges -- ids at and beyond n_images, a self edge, a repeated edge -- with match entries of -1, -7, nB, nB + 3 and
    INT32_MAX among the links; a layout made from other ids; a capacity cut in the middle of an edge; a pool whose last offset
    lies beyond the total and which holds an inverted range"""
    p = cases.pool(TILE)[:2]
    case = cases.random_case(p, 2000, 21, share=0.03)
    got = check(torch, handle, case, "random")
    assert 100 < (got[1][:-EXTRA] > 1).sum() and (got[2][:-EXTRA] > 0).any() and (got[1][:-EXTRA] == 1).any()
    for junk in (-1, -7, cases.INT32_MAX):
        assert (case.match == junk).any()
    check(torch, handle, cases.random_case(p, 2000, 22, share=0.9), "random, dense")
    other = cases.random_case(p, 2000, 23, share=0.05, layout_from_b=True, extra=11)
    assert (np.diff(other.la.astype(np.int64)) != [ecases.image_bounds(p[0], p[1], m)[1] for m in other.ea]).any()
    check(torch, handle, other, "a layout made from other ids")
    # the capacity: in the middle of an edge, at 0, and everything below it as before
    D = Device(torch, handle, case)
    e = int(np.argmax(np.diff(case.la.astype(np.int64)) > 200))
    full = case.cap
    for cap in (int(case.la[e]) + 130, 1, 0):
        case.cap = cap
        try:
            same(D.call(cap=cap), tailed(case.reference()), ("capacity", cap))
        finally:
            case.cap = full
    odd = cases.random_case(cases.odd_pool(), 90, 24, share=0.3)
    assert odd.io[-1] > odd.total and (np.diff(odd.io) < 0).any()
    got = check(torch, handle, odd, "odd pool")
    assert (got[2][:-EXTRA] > 0).any()


def test_no_edges_and_optional_statistics(torch, handle):
    case = cases.random_case(cases.pool(TILE)[:2], 1000, 31, share=0.05)
    D = Device(torch, handle, case)
    want = tailed(case.reference())
    same(D.call(), want, "all three")
    tail = np.full(case.total + EXTRA, SENTINEL, np.int32)
    same(D.call(dup=False), [want[0], want[1], tail], "len alone")
    same(D.call(length=False), [want[0], tail, want[2]], "dup alone")
    same(D.call(length=False, dup=False), [want[0], tail, tail], "labels alone")
    # no edges: every row its own track, the statistics written
    own = [np.arange(case.total), np.ones(case.total, np.uint32), np.zeros(case.total, np.uint32)]
    same(D.call(n_edges=0), tailed(own), "n_edges == 0")
    none = cases.Case((case.io, case.total), [], [])
    assert all(np.array_equal(x, y) for x, y in zip(none.reference(), own))
    # accumulating no edges onto labels leaves them, and writes their statistics
    same(D.call(into=want[0][:-EXTRA], n_edges=0), want, "n_edges == 0, accumulate")
    # a pool of no rows: nothing is written
    out = D.outputs()
    handle.build_tracks_device(D.d_io.data_ptr(), len(case.io) - 1, 0, D.d_ea.data_ptr(), D.d_eb.data_ptr(), D.d_la.data_ptr(), case.cap,
                               len(case.ea), D.d_match.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all((x == SENTINEL).all() for x in out)


# --- order and run ----------------------------------------------------------------------------------------------------
def test_order_run_and_split(torch, handle):
    p = cases.pool(TILE)[:2]
    case = cases.random_case(p, 1500, 41, share=0.04)
    D = Device(torch, handle, case)
    want = tailed(case.reference())
    first = D.call()
    same(first, want, "one call")
    same(D.call(), first, "two runs")
    out = D.outputs()                                                        # the handle's own stream (the binding waits)
    handle.build_tracks_device(D.d_io.data_ptr(), len(case.io) - 1, case.total, D.d_ea.data_ptr(), D.d_eb.data_ptr(), D.d_la.data_ptr(),
                               case.cap, len(case.ea), D.d_match.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0, None)
    same([x.cpu().numpy() for x in out], first, "handle's stream")
    rng = np.random.default_rng(5)
    for order in (np.arange(len(case.ea))[::-1], rng.permutation(len(case.ea))):
        same(Device(torch, handle, case.permuted(order)).call(), first, "permuted")
    # the links split over two and over five calls, all but the first accumulating
    for parts in (2, 5):
        part = rng.integers(0, parts, case.size)
        out = D.outputs()
        for k in range(parts):
            d_m = torch.from_numpy(np.concatenate([np.where(part == k, case.match, -1).astype(np.int32), np.full(EXTRA, 3, np.int32)])).cuda()
            D.run(out, flags=lfp.TRACKS_ACCUMULATE if k else 0, d_match=d_m)
            torch.cuda.synchronize()
            if k == 0:
                assert not np.array_equal(out[0].cpu().numpy(), first[0])
        same([x.cpu().numpy() for x in out], first, ("split", parts))
    # onto an array of anything: the restatement with the clamp
    junk = rng.integers(-2 ** 31, 2 ** 31, case.total).astype(np.int32)
    junk[::3] = rng.integers(0, case.total, len(junk[::3]))
    want_junk = tailed(case.reference(into=junk))
    assert not np.array_equal(want_junk[0], want[0])
    same(D.call(into=junk), want_junk, "onto anything")
    same(D.call(into=junk, n_edges=0), tailed(none_onto(case, junk)), "onto anything, no edges")


def none_onto(case, into):
    return cases.Case((case.io, case.total), [], []).reference(into=into)


# --- graph capture ----------------------------------------------------------------------------------------------------
def test_capturable(torch, handle):
    """one capture, replayed after the match array has been overwritten in place"""
    p = cases.pool(TILE)[:2]
    case, later = cases.random_case(p, 1000, 51, share=0.05), cases.random_case(p, 1000, 51, share=0.6)
    assert np.array_equal(case.la, later.la) and not np.array_equal(case.match, later.match)
    D = Device(torch, handle, case)
    out = D.outputs()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(out, stream=torch.cuda.current_stream().cuda_stream)
    for x in out:
        x.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in out], tailed(case.reference()), "replay")
    D.d_match[:later.size] = torch.from_numpy(later.match).cuda()
    g.replay()
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in out], tailed(later.reference()), "replay on new matches")


# --- matched pictures -------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_q8_edges.py::_frames


def _frames():
    """the 1024 x 768 centre crop of houses.jpg, a perspective warp of it, and bird.jpg brought to that size (PIL images)"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    hi = np.linalg.inv(H_TRUE)
    hi = hi / hi[2, 2]
    warp = crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC)
    bird = Image.open(os.path.join(GOLDEN, "bird.jpg")).convert("L").resize((1024, 768), Image.BICUBIC)
    return [crop, warp, bird]


def test_pictures(torch):
    """houses, its crop-and-warp and bird.jpg, all ordered pairs as edges, the device's own verified matches: the tracks equal the
    restatement on those same arrays read back, through LocalFeatures.build_tracks"""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "all", seed=21, feats=feats)
    kps, q, o = got["keypoints"], got["q8"], got["offsets"]
    m = q.shape[0]
    ea = torch.tensor([0, 0, 1, 1, 2, 2], dtype=torch.int32, device=q.device)
    eb = torch.tensor([1, 2, 0, 2, 0, 1], dtype=torch.int32, device=q.device)
    cap = 2 * m
    m_ab, _, _, _, la, lb = feats.match_q8_edges(q, o, q, o, ea, eb, ratio=0.8, mutual=True, capacity_a=cap, capacity_b=cap)
    ka, kb = feats.gather_edge_rows(kps, o, ea, la, capacity=cap), feats.gather_edge_rows(kps, o, eb, lb, capacity=cap)
    _, ver, _ = feats.verify_homography_batch(ka, la, kb, lb, m_ab, seed=21)
    track, length, dup = feats.build_tracks(o, ea, eb, la, ver, capacity=cap, n_rows=m)
    torch.cuda.synchronize()
    io = o.cpu().numpy()
    want = cases.build_tracks(io, m, ea.cpu().numpy(), eb.cpu().numpy(), la.cpu().numpy().astype(np.uint64), cap, ver.cpu().numpy())
    same([track.cpu().numpy(), length.cpu().numpy(), dup.cpu().numpy()], [np.asarray(w).astype(np.int64).astype(np.int32) for w in want], "pictures")
    length_h, dup_h, track_h = want[1], want[2], want[0]
    print(f"[tracks] {m} keypoints: {(length_h >= 2).sum()} tracks of length >= 2, {(length_h >= 3).sum()} of length >= 3, "
          f"{((length_h >= 2) & (dup_h == 0)).sum()} consistent, longest {length_h.max()}")
    assert (length_h >= 3).any()
    assert (length_h >= 2).sum() >= 8                                        # the crop and its warp share at least a homography's worth
    # the verified matches added to the mutual ones: a second call that accumulates, against the restatement on both arrays
    both, length2, dup2 = feats.build_tracks(o, ea, eb, la, m_ab, capacity=cap, into=track.clone())
    want2 = cases.build_tracks(io, m, ea.cpu().numpy(), eb.cpu().numpy(), la.cpu().numpy().astype(np.uint64), cap, m_ab.cpu().numpy(), into=track_h)
    same([both.cpu().numpy(), length2.cpu().numpy(), dup2.cpu().numpy()], [np.asarray(w).astype(np.int64).astype(np.int32) for w in want2], "pictures, accumulated")
    without = feats.build_tracks(o, ea, eb, la, ver, capacity=cap, n_rows=m, stats=False)
    assert torch.equal(without[0], track) and without[1] is None and without[2] is None


# --- the example ------------------------------------------------------------------------------------------------------
def test_match_collection_example_with_tracks(tmp_path):
    """examples/match_collection.py --all --tracks on three generated frames: the edge lines as before, then the track lines"""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_collection.py")
    out = subprocess.run([sys.executable, exe, "--all", "--tracks"] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    print("\n".join(lines))
    assert lines[0].startswith("Extracted ") and len(lines) == 6 and all(line.startswith("Edge ") for line in lines[1:4])
    m = re.match(r"Tracks: (\d+) of length >= 2 \((\d+) consistent\), (\d+) of length >= 3 \((\d+) consistent\)$", lines[4])
    assert m, lines[4]
    n2, c2, n3, c3 = (int(x) for x in m.groups())
    assert n2 >= n3 >= c3 >= 0 and n2 >= c2 >= c3 and n2 >= 8
    m = re.match(r"Longest track: (\d+) keypoints; ([0-9.]+) % of the keypoints sit in a consistent track of length >= 2$", lines[5])
    assert m and int(m.group(1)) >= 2 and 0.0 < float(m.group(2)) <= 100.0, lines[5]
