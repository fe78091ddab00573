"""Track tables on the GPU (lf_mkd_track_table_device, lf_mkd_gather_track_rows_device; LocalFeatures.track_table /
gather_track_rows): every output equals the numpy restatement's (tests/track_table_cases.py) -- every comparison is ==, the
entries behind every array included.  The shared track cases with lf_mkd_build_tracks_device's own output as the input,
synthetic labels whose tracks lie across every block, the sizes around a workgroup's block, capacity cuts, arrays of anything,
relabelled inputs, graph capture, the gather, matched pictures and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tracks_cases as tcases
import track_table_cases as cases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # entries every output array is longer than needed
SENTINEL = tcases.SENTINEL
TILE = lfp.TRACKS_DUP_TILE
NAMES = ("offsets", "obs_row", "obs_image", "row_track", "counts")
LARGE = 3 * 2 ** 16 + 5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


def bits32(x):
    """uint32 or int32 values as int32 bit patterns"""
    return np.asarray(x).astype(np.int64).astype(np.uint32).view(np.int32)


class Device:
    """(track, length, dup) and the image offsets on the device; outputs EXTRA entries longer than needed, sentinel-filled"""

    def __init__(self, torch, handle, track, length, dup, io=None):
        self.torch, self.handle, self.n = torch, handle, len(track)
        up = lambda x: torch.from_numpy(np.concatenate([bits32(x), np.full(EXTRA, 0, np.int32)])).cuda()   # (0: a root, were it read)
        self.d_track, self.d_len, self.d_dup = up(track), up(length), up(dup)
        self.io = io
        self.d_io = torch.from_numpy(np.array(io, np.int64)).cuda() if io is not None else None

    def outputs(self, t_cap, o_cap):
        t = self.torch
        full = lambda n, dtype: t.full((n + EXTRA,), SENTINEL, dtype=dtype, device="cuda")
        return [full(t_cap + 1, t.int64), full(o_cap, t.int32), full(o_cap, t.int32), full(self.n, t.int32), full(4, t.int32)]

    def run(self, out, min_len, consistent, t_cap, o_cap, images=True, row_track=True, stream=None):
        images = images and self.d_io is not None
        self.handle.track_table_device(
            self.d_io.data_ptr() if self.d_io is not None else None, len(self.io) - 1 if self.io is not None else 0, self.n,
            self.d_track.data_ptr(), self.d_len.data_ptr(), self.d_dup.data_ptr(), min_len,
            lfp.TRACK_TABLE_CONSISTENT if consistent else 0, t_cap, o_cap, out[0].data_ptr(), out[1].data_ptr(),
            out[2].data_ptr() if images else None, out[3].data_ptr() if row_track else None, out[4].data_ptr(),
            self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def call(self, min_len, consistent, t_cap=None, o_cap=None, **kw):
        t_cap = self.n // min_len if t_cap is None else t_cap
        o_cap = self.n if o_cap is None else o_cap
        out = self.outputs(t_cap, o_cap)
        self.torch.cuda.synchronize()
        self.run(out, min_len, consistent, t_cap, o_cap, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]


def tailed(table, o_cap, images=True, row_track=True):
    """a restatement's Table as the device arrays hold it: entries beyond O and the EXTRA entries behind still sentinels"""
    tail = lambda x, n, dtype: np.concatenate([np.asarray(x, dtype), np.full(n + EXTRA - len(x), SENTINEL, dtype)])
    o = table.counts[1]
    assert len(table.obs_row) == o <= o_cap
    return [tail(table.offsets.astype(np.int64), len(table.offsets), np.int64), tail(table.obs_row, o_cap, np.int32),
            tail(bits32(table.obs_image) if images and table.obs_image is not None else [], o_cap, np.int32),
            tail(table.row_track if row_track else [], len(table.row_track), np.int32), tail(bits32(table.counts), 4, np.int32)]


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def check(D, arrays, min_len, consistent, what, t_cap=None, o_cap=None, **kw):
    track, length, dup = arrays
    want = cases.track_table(track, length, dup, min_len, consistent, t_cap, o_cap, image_offsets=D.io)
    got = D.call(min_len, consistent, t_cap, o_cap, **kw)
    same(got, tailed(want, D.n if o_cap is None else o_cap, **kw), what)
    return want


# --- the shared track cases, lf_mkd_build_tracks_device's own output as the input ------------------------------------------
def built(torch, handle, case):
    """the arrays lf_mkd_build_tracks_device leaves for a case of tests/tracks_cases.py (they equal its restatement)"""
    words = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint32)).view(np.int32)).cuda()
    d_io, d_ea, d_eb = torch.from_numpy(np.array(case.io, np.int64)).cuda(), words(case.ea), words(case.eb)
    d_la, d_match = torch.from_numpy(case.la.astype(np.int64)).cuda(), torch.from_numpy(case.match).cuda()
    out = [torch.full((case.total,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    handle.build_tracks_device(d_io.data_ptr(), len(case.io) - 1, case.total, d_ea.data_ptr(), d_eb.data_ptr(), d_la.data_ptr(), case.cap,
                               len(case.ea), d_match.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32), out[2].cpu().numpy().view(np.uint32)]
    assert all(np.array_equal(g, w) for g, w in zip(got, case.reference()))
    return got


SHARED = {"chain": lambda: tcases.chain(TILE, False), "star": lambda: tcases.stars(TILE, False), "two stars": lambda: tcases.stars(TILE, True),
          "cycles": lambda: tcases.cycles(TILE), "random": lambda: tcases.random_case(tcases.pool(TILE)[:2], 40, 5)}


@pytest.mark.parametrize("name", list(SHARED))
def test_shared_track_cases(name, torch, handle):
    """the 3197-row pool at min_len 1, 2, 3 with and without the flag; d_obs_image on a pool whose 5 leading and 7 trailing rows
    belong to no image.  The star without the flag is ONE track of 2379 rows: every key equal."""
    case = SHARED[name]()
    arrays = built(torch, handle, case)
    D = Device(torch, handle, *arrays, io=case.io)
    seen = {}
    for min_len in (1, 2, 3):
        for consistent in (False, True):
            want = check(D, arrays, min_len, consistent, (name, min_len, consistent))
            seen[min_len, consistent] = (want.counts[0], want.counts[1])
    assert case.total == 3197
    if name == "star":
        assert seen[2, False] == (1, 2379) and seen[1, True] == (818, 818)
    if name == "cycles":
        assert seen[2, True] == (100, 300) and seen[2, False] == (152, 506)
    if name == "random":
        assert seen[2, False] == (64, 322)
    if name == "chain":                                                      # without the optional outputs: they stay untouched
        check(D, arrays, 2, True, "no optional outputs", images=False, row_track=False)
        none = Device(torch, handle, *arrays)                                # no image offsets at all
        check(none, arrays, 2, True, "no image offsets")


# --- synthetic labels, no edge list --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    """LARGE rows in LARGE // 3 groups drawn at random: a track's rows lie across the whole pool and across every block"""
    arrays = cases.random_groups(LARGE, LARGE // 3, 4)
    assert (arrays[1] > 0).sum() == 62247 and arrays[1].max() == 12
    return arrays


def test_large_pool_across_every_block(large, torch, handle):
    passes, block = lfp.track_table_plan(LARGE, 1)[1:3]
    assert passes > lfp.track_table_plan(3197, 1)[1]                         # one more radix pass than the shared cases take
    assert LARGE > 8 * block
    D = Device(torch, handle, *large)
    want = check(D, large, 1, False, "large, min_len 1")
    assert want.counts[0] == 62247
    t, offs = want.counts[0], want.offsets.astype(np.int64)
    assert (want.obs_row[offs[1:t + 1] - 1] - want.obs_row[offs[:t]]).max() > LARGE // 2   # tracks whose rows lie blocks apart
    check(D, large, 2, True, "large, min_len 2")
    check(D, large, 5, False, "large, min_len 5")


def test_large_pool_one_track_and_single_rows(torch, handle):
    one = cases.from_groups(np.zeros(LARGE, np.int64))
    D = Device(torch, handle, *one)
    want = check(D, one, 1, False, "one track of all rows")
    assert want.counts[:2] == [1, LARGE] and np.array_equal(want.obs_row, np.arange(LARGE))
    check(D, one, 2, True, "one track of all rows, min_len 2")
    own = cases.from_groups(np.arange(LARGE))
    D = Device(torch, handle, *own)
    want = check(D, own, 1, True, "every row its own track")
    assert want.counts[:2] == [LARGE, LARGE]
    assert check(D, own, 2, True, "every row its own track, min_len 2").counts == [0, 0, 0, 0]


def test_boundary_sizes(torch, handle):
    block = lfp.track_table_plan(1, 1)[2]
    for n in (0, 1, 2, 63, 64, 65, block - 1, block, block + 1, 2 * block + 1):
        arrays = cases.random_groups(n, max(n // 3, 1), n)
        io = np.array([min(1, n), n // 2, n // 2, max(n - 1, 0)], np.int64)
        D = Device(torch, handle, *arrays, io=io)
        for min_len in (1, 2):
            want = check(D, arrays, min_len, True, ("size", n, min_len))
            assert n < 63 or want.counts[0] > 0
        if n == 0:                                                           # the counts 0, every offset 0, whatever the capacity
            want = check(D, arrays, 2, True, "no rows, capacities", t_cap=3, o_cap=5)
            assert want.counts == [0, 0, 0, 0] and want.offsets.tolist() == [0, 0, 0, 0]
        one = cases.from_groups(np.zeros(n, np.int64))
        check(Device(torch, handle, *one), one, 1, False, ("size, one track", n))


# --- capacities ------------------------------------------------------------------------------------------------------------
def test_capacities(large, torch, handle):
    case = SHARED["random"]()
    arrays = case.reference()
    D = Device(torch, handle, *arrays, io=case.io)
    full = cases.track_table(*arrays, 2, False)
    t, o = full.counts[:2]
    assert (t, o) == (64, 322)
    for t_cap in (t + 5, t, t - 1, 1, 0):
        want = check(D, arrays, 2, False, ("track_capacity", t_cap), t_cap=t_cap)
        assert want.counts == [min(t, t_cap), int(full.offsets[min(t, t_cap)]), t, o]
        assert (want.offsets[want.counts[0]:] == want.counts[1]).all() and len(want.offsets) == t_cap + 1
    inside = int(full.offsets[40]) + 1                                       # ends inside track 40: it and all behind it are dropped
    assert int(full.offsets[41]) - int(full.offsets[40]) >= 2
    for o_cap in (o + 9, o, o - 1, inside, int(full.offsets[1]), int(full.offsets[1]) - 1, 1, 0):
        want = check(D, arrays, 2, False, ("obs_capacity", o_cap), o_cap=o_cap)
        assert want.counts[1] <= o_cap and want.counts[2:] == [t, o]
    assert cases.track_table(*arrays, 2, False, None, inside).counts[:2] == [40, inside - 1]
    want = check(D, arrays, 2, False, "both", t_cap=50, o_cap=inside)
    assert want.counts == [40, inside - 1, t, o]
    # the large pool: a cut in a later block
    check(Device(torch, handle, *large), large, 2, True, "large, cut", t_cap=30000, o_cap=100001)


# --- whatever the arrays hold ------------------------------------------------------------------------------------------------
def test_arrays_of_anything(torch, handle):
    """random int32 in all three arrays: the call returns, the counts are the restatement's, nothing behind any array is written"""
    rng = np.random.default_rng(61)
    for n, t_cap, o_cap in ((3197, 3197, 3197), (3197, 100, 5000), (3197, 7, 3197), (LARGE, LARGE // 2, LARGE // 2)):
        track = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
        roots = rng.random(n) < 0.3
        track[roots] = np.flatnonzero(roots)                                  # (else a random array has next to no root)
        inside = ~roots & (rng.random(n) < 0.4)
        track[inside] = rng.integers(0, n, int(inside.sum()))
        length = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32).view(np.uint32).copy()
        small = rng.random(n) < 0.7
        length[small] = rng.integers(0, 9, int(small.sum()))
        dup = np.where(rng.random(n) < 0.5, 0, rng.integers(-2 ** 31, 2 ** 31, n)).astype(np.int32).view(np.uint32)
        io = np.sort(rng.integers(0, n + 50, 9)).astype(np.int64)
        D = Device(torch, handle, track, length, dup, io=io)
        for min_len, consistent in ((1, False), (2, True), (3, False)):
            got = D.call(min_len, consistent, t_cap, o_cap)
            counts = cases.counts_of(track, length, dup, min_len, consistent, t_cap, o_cap)[0]
            assert got[4][:4].view(np.uint32).tolist() == counts and counts[0] <= t_cap and counts[1] <= o_cap, (n, min_len, counts)
            for name, g, used in zip(NAMES, got, (t_cap + 1, o_cap, o_cap, n, 4)):
                assert (g[used:] == SENTINEL).all() and len(g) == used + EXTRA, (name, n, min_len)
            assert (got[1][counts[1]:] == SENTINEL).all() and (got[2][counts[1]:] == SENTINEL).all()   # nothing at or beyond O
            offs = got[0][:t_cap + 1]
            assert (offs[counts[0]:] == counts[1]).all() and (np.diff(offs) >= 0).all()


def test_labels_out_of_range(torch, handle):
    """rows labelled -3 and N + 2 are members of nothing"""
    track, length, dup = (x.copy() for x in cases.random_groups(700, 200, 2))
    n = len(track)
    moved = np.flatnonzero((track != np.arange(n)) & (length[track] >= 3))[:40]
    assert len(moved) == 40
    for k, r in enumerate(moved):
        length[track[r]] -= 1
        track[r] = -3 if k % 2 else n + 2
    D = Device(torch, handle, track, length, dup)
    for min_len in (1, 2):
        want = check(D, (track, length, dup), min_len, True, ("out of range", min_len))
        assert (want.row_track[moved] == -1).all() and not np.isin(moved, want.obs_row).any()


# --- determinism and capture ---------------------------------------------------------------------------------------------
def test_two_runs_and_relabelled_rows(torch, handle):
    arrays = SHARED["cycles"]().reference()
    n = len(arrays[0])
    D = Device(torch, handle, *arrays)
    first = D.call(2, True)
    same(D.call(2, True), first, "two runs")
    want = cases.track_table(*arrays, 2, True)
    same(first, tailed(want, n), "cycles")
    perm = np.random.default_rng(9).permutation(n)
    renamed = cases.relabelled(*arrays, perm)
    got = Device(torch, handle, *renamed).call(2, True)
    same(got, tailed(cases.track_table(*renamed, 2, True), n), "relabelled")
    inv = np.argsort(perm)

    def sets(out, back):
        t = int(out[4][0])
        return sorted(tuple(sorted(back[out[1][int(out[0][i]):int(out[0][i + 1])]].tolist())) for i in range(t))
    assert sets(first, np.arange(n)) == sets(got, inv) and int(first[4][0]) == 100    # undone: the same tracks


def test_capturable(torch, handle):
    """one capture of the warmed-up call, replayed after the inputs have been overwritten in place"""
    first, later = cases.random_groups(5000, 1500, 1), cases.random_groups(5000, 900, 2)
    later[2][later[1] > 6] = 1
    io = np.array([3, 1000, 1000, 2500, 4990], np.int64)
    D = Device(torch, handle, *first, io=io)
    same(D.call(2, True), tailed(cases.track_table(*first, 2, True, image_offsets=io), 5000), "warm-up")
    out = D.outputs(2500, 5000)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(out, 2, True, 2500, 5000, stream=torch.cuda.current_stream().cuda_stream)
    for x in out:
        x.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in out], tailed(cases.track_table(*first, 2, True, image_offsets=io), 5000), "replay")
    for d, x in zip((D.d_track, D.d_len, D.d_dup), later):
        d[:5000] = torch.from_numpy(bits32(x)).cuda()
    for x in out:
        x.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    want = cases.track_table(*later, 2, True, image_offsets=io)
    assert (later[2] > 0).any() and want.counts[0] > 100
    same([x.cpu().numpy() for x in out], tailed(want, 5000), "replay on new inputs")


# --- the gather ------------------------------------------------------------------------------------------------------------
def test_gather(torch, handle):
    arrays = SHARED["random"]().reference()
    n = len(arrays[0])
    D = Device(torch, handle, *arrays)
    out = D.outputs(n // 2, n)
    torch.cuda.synchronize()
    D.run(out, 2, False, n // 2, n)
    torch.cuda.synchronize()
    want = cases.track_table(*arrays, 2, False)
    o = want.counts[1]
    rng = np.random.default_rng(3)
    kps = rng.random((n, 5), dtype=np.float32)
    q8 = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    for src in (kps, q8):
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.from_numpy(np.full((n + EXTRA,) + src.shape[1:], 7, src.dtype)).cuda()
        torch.cuda.synchronize()
        handle.gather_track_rows_device(d_src.data_ptr(), src.shape[1] * src.itemsize, n, out[1].data_ptr(), out[4].data_ptr(), n,
                                        d_dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        assert np.array_equal(got[:o], src[want.obs_row]) and (got[o:] == 7).all()           # rows beyond O are untouched
        # a capacity below the count: only that many rows
        d_dst.fill_(7)
        torch.cuda.synchronize()
        handle.gather_track_rows_device(d_src.data_ptr(), src.shape[1] * src.itemsize, n, out[1].data_ptr(), out[4].data_ptr(), 65,
                                        d_dst.data_ptr(), stream)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        assert np.array_equal(got[:65], src[want.obs_row[:65]]) and (got[65:] == 7).all()
    # indices out of range give zero rows
    rows = out[1].clone()
    bad = [0, 64, 65, o - 1]
    rows[bad] = torch.tensor([-1, n, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device="cuda")
    d_src = torch.from_numpy(kps).cuda()
    d_dst = torch.from_numpy(np.full((n + EXTRA, 5), 7, np.float32)).cuda()
    torch.cuda.synchronize()
    handle.gather_track_rows_device(d_src.data_ptr(), 20, n, rows.data_ptr(), out[4].data_ptr(), n, d_dst.data_ptr(), stream)
    torch.cuda.synchronize()
    expect = np.full((n + EXTRA, 5), 7, np.float32)
    cases.gather_track_rows(kps, rows.cpu().numpy(), o, expect)
    assert (expect[bad] == 0).all() and np.array_equal(d_dst.cpu().numpy(), expect)


# --- matched pictures ------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_tracks.py::_frames


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
    """match_collection(..., table=True) on houses, its crop-and-warp and bird.jpg: the table and the gathered keypoints equal the
    restatement on the track arrays read back"""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "all", seed=21, feats=feats, table=True)
    torch.cuda.synchronize()
    track, length, dup = (got[k].cpu().numpy() for k in ("track", "track_len", "track_dup"))
    io, kps = got["offsets"].cpu().numpy(), got["keypoints"].cpu().numpy()
    n = len(track)
    want = cases.track_table(track, length.view(np.uint32), dup.view(np.uint32), 2, True, image_offsets=io)
    assert want.counts[0] >= 8
    assert got["table_counts"].cpu().numpy().view(np.uint32).tolist() == want.counts
    assert np.array_equal(got["table_offsets"].cpu().numpy(), want.offsets.astype(np.int64)) and len(want.offsets) == n // 2 + 1
    o = want.counts[1]
    assert got["table_rows"].shape[0] == n and np.array_equal(got["table_rows"].cpu().numpy()[:o], want.obs_row)
    assert np.array_equal(got["table_images"].cpu().numpy()[:o].view(np.uint32), want.obs_image)
    assert np.array_equal(got["table_row_track"].cpu().numpy(), want.row_track)
    tk = got["table_keypoints"].cpu().numpy()
    assert tk.shape == (n, 5) and np.array_equal(tk[:o], kps[want.obs_row]) and (tk[o:] == 0).all()
    # a consistent track has one keypoint per image: its images ascend strictly
    for i in range(want.counts[0]):
        assert (np.diff(want.obs_image[int(want.offsets[i]):int(want.offsets[i + 1])].astype(np.int64)) > 0).all()
    # without the table the entries are None and the rest is what it was
    plain = ex.match_collection(frames, "all", seed=21, feats=feats, tracks=True)
    assert plain["table_rows"] is None and plain["table_counts"] is None and torch.equal(plain["track"], got["track"])


# --- the example -----------------------------------------------------------------------------------------------------------
def test_match_collection_example_with_table(tmp_path):
    """examples/match_collection.py --all --table on three generated frames: the six lines of --all --tracks unchanged, then the
    table lines"""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_collection.py")
    old = subprocess.run([sys.executable, exe, "--all", "--tracks"] + paths, capture_output=True, text=True, timeout=600)
    out = subprocess.run([sys.executable, exe, "--all", "--table"] + paths, capture_output=True, text=True, timeout=600)
    assert old.returncode == 0 and out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    print("\n".join(lines))
    assert len(old.stdout.splitlines()) == 6 and lines[:6] == old.stdout.splitlines()
    m = re.match(r"Track table: (\d+) tracks, (\d+) observations \(consistent, length >= 2\)$", lines[6])
    assert m, lines[6]
    n_tracks, n_obs = int(m.group(1)), int(m.group(2))
    c2 = int(re.match(r"Tracks: (\d+) of length >= 2 \((\d+) consistent\)", lines[4]).group(2))
    assert n_tracks == c2 >= 8 and n_obs >= 2 * n_tracks
    assert len(lines) == 7 + min(n_tracks, 3)
    for k, line in enumerate(lines[7:]):
        m = re.match(r"Track %d: ((?:\d+:-?[0-9.]+,-?[0-9.]+ ?)+)$" % (k + 1), line)
        assert m, line
        images = [int(x.split(":")[0]) for x in m.group(1).split()]
        assert len(images) >= 2 and images == sorted(set(images)) and 1 <= images[0] and images[-1] <= 3
