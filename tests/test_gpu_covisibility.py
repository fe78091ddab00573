"""Covisibility tables on the GPU (lf_mkd_covisibility_device; LocalFeatures.covisibility): the table equals the numpy
restatement's (tests/covisibility_cases.py) -- every comparison is ==, and d_covis sits between sentinel entries that must
survive.  Track lengths around the group widths and the chunk of 64, image counts either side of every threshold of the plan,
every form of the plan on one table, images that repeat, do not ascend and lie outside the range, contention, one long track,
capacities and offsets, offsets that decrease, ACCUMULATE, the mask, two runs and graph capture, the chain from random links to
a second round of candidate edges, tables past the 2 GiB and 4 GiB byte marks, matched pictures and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import covisibility_cases as cases
import select_edges_cases as scases
import tracks_cases as tcases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel entries in front of and behind the table
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


def bits32(x):
    return np.asarray(x).astype(np.int64).astype(np.uint32).view(np.int32)


class Device:
    """a track table on the device: the arrays hold exactly what the capacities say, so a read beyond them leaves the
    allocation's used part; d_covis between sentinels"""

    def __init__(self, torch, handle, tab, n_images):
        self.torch, self.handle, self.tab, self.n = torch, handle, tab, n_images
        self.d_off = torch.from_numpy(tab.offsets[:tab.track_capacity + 1].view(np.int64).copy()).cuda()
        self.d_img = torch.from_numpy(bits32(tab.images[:tab.obs_capacity])).cuda()
        self.d_counts = torch.from_numpy(bits32(tab.counts)).cuda()
        self.edges = None

    def mask(self, edge_a, edge_b):
        self.edges = (self.torch.from_numpy(bits32(edge_a)).cuda(), self.torch.from_numpy(bits32(edge_b)).cuda())
        return self

    def buffer(self, fill=None):
        buf = self.torch.full((self.n * self.n + 2 * EXTRA,), SENTINEL, dtype=self.torch.int32, device="cuda")
        if fill is not None:
            buf[EXTRA:EXTRA + self.n * self.n] = self.torch.from_numpy(bits32(fill).reshape(-1)).cuda()
        return buf

    def run(self, buf, flags=0, stream=None):
        ea, eb = self.edges if self.edges is not None else (None, None)
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        self.handle.covisibility_device(self.d_off.data_ptr(), self.tab.track_capacity, ptr(self.d_img), self.tab.obs_capacity,
                                        self.d_counts.data_ptr(), self.n, ptr(ea), ptr(eb), ea.numel() if ea is not None else 0,
                                        flags, buf.data_ptr() + 4 * EXTRA if self.n else None,
                                        self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def call(self, flags=0, fill=None):
        buf = self.buffer(fill)
        self.torch.cuda.synchronize()
        self.run(buf, flags)
        self.torch.cuda.synchronize()
        return body(buf.cpu().numpy(), self.n)


def body(raw, n):
    """the table out of its frame; the sentinels must have survived"""
    assert (raw[:EXTRA] == SENTINEL).all() and (raw[EXTRA + n * n:] == SENTINEL).all(), "a write outside d_covis"
    return raw[EXTRA:EXTRA + n * n].view(np.uint32).reshape(n, n)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(want[tuple(b)]) for b in bad[:5]])


def check(torch, handle, tab, n, what, edges=None, flags=0, fill=None):
    want = cases.covisibility(tab, n, edges=edges, into=fill if flags & cases.ACCUMULATE else None)
    D = Device(torch, handle, tab, n)
    if edges is not None:
        D.mask(*edges)
    got = D.call(flags, fill)
    same(got, want, what)
    return want


# --- lengths, image counts, contents ---------------------------------------------------------------------------------------
SHARED = {name: (tab, n) for name, tab, n in cases.cases()}


@pytest.mark.parametrize("name", list(SHARED))
def test_shared_cases(name, torch, handle):
    """every kind of contents at every n_images: track lengths 0 .. 129, n_images and n_images + 1, and a crowd of short ones"""
    tab, n = SHARED[name]
    lens = set(np.diff(tab.offsets.astype(np.int64)).tolist())
    assert name == "by-hand" or {min(l, n) if name.startswith("consistent") else l for l in cases.LENGTHS + (n,)} <= lens
    want = check(torch, handle, tab, n, name)
    assert want.sum() > 0


def padded(tab, track_capacity):
    """the same table in a longer offsets array: the entries beyond the last track repeat the number of observations"""
    T = tab.track_capacity
    off = np.concatenate([tab.offsets[:T + 1], np.full(track_capacity - T, tab.offsets[T], np.uint64)])
    return cases.Table(off, tab.images, counts=[T, tab.obs_capacity, 0, 0], track_capacity=track_capacity, obs_capacity=tab.obs_capacity)


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_every_form_on_one_table(kind, torch, handle):
    """the plan chooses the lanes per track from the capacities: one table in offsets arrays of growing capacity goes through
    every width, and with it through both counting kernels (a track of more than 16 x the width belongs to the second)"""
    n = 200
    rng = np.random.default_rng(5)
    lens = list(cases.LENGTHS) + [n, 190, 17, 31, 33, 300 if kind != "consistent" else 199] + rng.integers(0, 9, 60).tolist()
    tab = cases.from_tracks(cases.KINDS[kind](rng, n, lens))
    want = cases.covisibility(tab, n)
    O = tab.obs_capacity
    seen = set()
    for lanes in (64, 32, 16, 8, 4):
        t_cap = max(tab.track_capacity, -(-2 * O // lanes))
        form = lfp.covisibility_plan(n, t_cap, O)[0]
        assert form == lanes, (form, lanes)
        seen.add(form)
        same(Device(torch, handle, padded(tab, t_cap), n).call(), want, (kind, lanes))
        # either side of the width's own boundary for the longest track that stays with the first kernel
        edge = cases.from_tracks(cases.KINDS[kind](rng, n, [16 * lanes - 1, 16 * lanes, 16 * lanes + 1, 2, 3]))
        t_cap = -(-2 * edge.obs_capacity // lanes)
        if kind != "consistent":                                                 # (its lengths stop at n_images)
            assert lfp.covisibility_plan(n, t_cap, edge.obs_capacity)[0] == lanes
            same(Device(torch, handle, padded(edge, t_cap), n).call(), cases.covisibility(edge, n, matrix=True), (kind, lanes, "16 x lanes"))
    assert seen == {4, 8, 16, 32, 64}


def test_lds_threshold(torch, handle):
    """n_images either side of the size up to which a workgroup counts into its private table first, many workgroups"""
    lds = [n for n in range(1, 100) if lfp.covisibility_plan(n, 100, 1000)[0] & lfp.COVIS_FORM_LDS]
    rng = np.random.default_rng(11)
    for n in sorted({max(lds + [1]), max(lds + [1]) + 1, 2, 7}):
        tab = cases.from_tracks(cases.duplicated(rng, n, rng.integers(0, 12, 6000).tolist()))
        assert lfp.covisibility_plan(n, tab.track_capacity, tab.obs_capacity)[1] > 8
        check(torch, handle, tab, n, ("lds", n))


def test_contention(torch, handle):
    """20 000 tracks over 2 images: every add lands on four words"""
    T = 20000
    tab = cases.from_tracks([[0, 1]] * T)
    got = Device(torch, handle, tab, 2).call()
    assert got.tolist() == [[T, T], [T, T]]
    same(got, cases.covisibility(tab, 2, matrix=True), "contention")


def test_one_long_track(torch, handle):
    """one track over all of 300 images plus 5000 short ones; then the same long track with every image repeated 40 times
    (12 000 positions, 300 distinct), as a table made without LF_MKD_TRACK_TABLE_CONSISTENT holds it"""
    rng = np.random.default_rng(3)
    short = cases.consistent(rng, 300, rng.integers(2, 6, 5000).tolist())
    tab = cases.from_tracks(short[:2500] + [np.arange(300)] + short[2500:])
    want = check(torch, handle, tab, 300, "long")
    assert want.min() >= 1
    rep = cases.from_tracks(short[:100] + [np.repeat(np.arange(300), 40)] + short[100:200])
    assert lfp.covisibility_plan(300, rep.track_capacity, rep.obs_capacity)[0] == 64
    got = Device(torch, handle, rep, 300).call()
    same(got, cases.covisibility(rep, 300, matrix=True), "long, repeated")


# --- capacities, offsets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in cases.capacity_cases()])
def test_capacities_and_offsets(name, torch, handle):
    tab, n = {c[0]: c[1:] for c in cases.capacity_cases()}[name]
    want = check(torch, handle, tab, n, name)
    whole = cases.capacity_cases()[0][1]
    assert want.sum() > 0 and not np.array_equal(want, cases.covisibility(cases.Table(whole.offsets, whole.images), n))


def test_no_image_no_track_no_observation(torch, handle):
    tab = cases.from_tracks([[0, 1], [1, 2]])
    D = Device(torch, handle, tab, 0)
    buf = D.buffer()
    D.run(buf)                                                                   # n_images == 0: LF_MKD_OK, nothing written
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()
    fill = np.arange(9, dtype=np.uint32).reshape(3, 3) + 5
    for t in (cases.Table(tab.offsets, tab.images, counts=[0, 4, 0, 0]), cases.Table(tab.offsets, tab.images, counts=[2, 0, 0, 0]),
              cases.Table(tab.offsets, tab.images, obs_capacity=0), cases.Table(tab.offsets[:1], tab.images)):
        D = Device(torch, handle, t, 3).mask([0, 2], [1, 2])                     # T == 0 still zeroes and masks
        assert (D.call(fill=fill) == 0).all()
        got = D.call(cases.ACCUMULATE, fill=fill)
        assert got.tolist() == [[5, 0, 7], [0, 9, 10], [11, 12, 0]]


def test_offsets_that_decrease(torch, handle):
    """d_covis is unspecified: the call returns, the sentinels survive, and a good call behind it is exact"""
    rng = np.random.default_rng(13)
    tab = cases.from_tracks(cases.duplicated(rng, 50, [3, 1500, 4, 70, 2000, 5, 9, 0, 2]))
    off = tab.offsets.copy()
    off[[2, 5]] = off[[5, 2]]                                                    # a long range that reaches back, inverted ones
    off[7] = 1
    bad = cases.Table(off, tab.images)
    for t_cap in (bad.track_capacity, 600):
        got = Device(torch, handle, padded(bad, t_cap), 50).call()
        assert got.shape == (50, 50)
    check(torch, handle, tab, 50, "the good call behind")


# --- ACCUMULATE and the mask -----------------------------------------------------------------------------------------------
def test_accumulate(torch, handle):
    rng = np.random.default_rng(17)
    n = 40
    tab = cases.from_tracks(cases.duplicated(rng, n, rng.integers(0, 30, 400).tolist() + [900, 70]))
    want = cases.covisibility(tab, n)
    for parts in (2, 5):
        buf = None
        for i, part in enumerate(cases.split(tab, parts)):
            D = Device(torch, handle, part, n)
            if buf is None:
                buf = D.buffer()
            torch.cuda.synchronize()
            D.run(buf, cases.ACCUMULATE if i else 0)
        torch.cuda.synchronize()
        same(body(buf.cpu().numpy(), n), want, ("split", parts))
    fill = rng.integers(0, 2 ** 32, (n, n), dtype=np.uint64).astype(np.uint32)
    fill[:4] = 0xFFFFFFFF                                                        # wrap-around
    got = check(torch, handle, tab, n, "pre-filled", flags=cases.ACCUMULATE, fill=fill)
    assert (got[:4] == want[:4] - 1).all() and want[:4].min() >= 1
    # without the flag what the table held does not matter
    check(torch, handle, tab, n, "pre-filled, no flag", fill=fill)


def test_mask(torch, handle):
    rng = np.random.default_rng(19)
    n = 30
    tab = cases.from_tracks(cases.consistent(rng, n, rng.integers(2, 12, 500).tolist()))
    full = cases.covisibility(tab, n)
    assert full.min() >= 1
    # self edges, repeats, (j, i) beside (i, j), ids out of range
    ea = np.array([0, 3, 3, 7, 9, n, 0xFFFFFFFF, 5, n - 1, 1 << 31, 12], np.uint32)
    eb = np.array([1, 3, 3, 9, 7, 2, 0xFFFFFFFF, n, n - 1, 4, 0xFFFFFFFF], np.uint32)
    want = check(torch, handle, tab, n, "mask", edges=(ea, eb))
    assert np.count_nonzero(want == 0) == 6 and want[3, 3] == 0 and want[9, 7] == want[7, 9] == 0 and want[5, 2] > 0
    # with ACCUMULATE the mask applies to the sum
    fill = rng.integers(1, 100, (n, n)).astype(np.uint32)
    got = check(torch, handle, tab, n, "mask + accumulate", edges=(ea, eb), flags=cases.ACCUMULATE, fill=fill)
    assert np.count_nonzero(got == 0) == 6 and got[5, 2] == full[5, 2] + fill[5, 2]
    # the padded list of a real select_edges call, passed whole
    k = 3
    out = [torch.full((n * k,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.zeros(4, dtype=torch.int32, device="cuda")]
    d_full = torch.from_numpy(bits32(full)).cuda()
    handle.select_edges_device(d_full.data_ptr(), n, n, k, 1, lfp.SELECT_SKIP_SELF | lfp.SELECT_UNIQUE, n * k, None, None,
                               out[0].data_ptr(), out[1].data_ptr(), None, out[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sel = scases.select_edges(full, k, 1, True, True)
    kept = sel.counts[0]
    assert 0 < kept <= n * k and np.array_equal(out[0].cpu().numpy().view(np.uint32), sel.edge_a) and (sel.edge_a[kept:] == cases.PAD).all()
    D = Device(torch, handle, tab, n)
    D.edges = (out[0], out[1])
    got = D.call()
    same(got, cases.covisibility(tab, n, edges=(sel.edge_a, sel.edge_b)), "select_edges' list")
    assert np.count_nonzero(got == 0) == 2 * kept


# --- repeatability, capture ------------------------------------------------------------------------------------------------
def test_two_runs_and_capture(torch, handle):
    rng = np.random.default_rng(23)
    n = 70
    make = lambda seed: cases.from_tracks(cases.duplicated(np.random.default_rng(seed), n, rng.integers(0, 40, 300).tolist() + [1300]))
    first, later = make(1), make(2)
    later = cases.Table(np.concatenate([later.offsets, np.full(len(first.offsets), later.offsets[-1], np.uint64)])[:len(first.offsets)],
                        np.concatenate([later.images, np.zeros(first.obs_capacity, np.uint32)])[:first.obs_capacity],
                        counts=[min(later.track_capacity, first.track_capacity), min(later.obs_capacity, first.obs_capacity), 0, 0])
    ea, eb = np.array([1, 5, 99], np.uint32), np.array([2, 5, 0], np.uint32)
    D = Device(torch, handle, first, n).mask(ea, eb)
    a, b = D.call(), D.call()
    want = cases.covisibility(first, n, edges=(ea, eb))
    same(a, want, "first run")
    assert a.tobytes() == b.tobytes()
    buf = D.buffer()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(buf, stream=torch.cuda.current_stream().cuda_stream)
    buf.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(body(buf.cpu().numpy(), n), want, "replay")
    D.d_off.copy_(torch.from_numpy(later.offsets.view(np.int64).copy()))
    D.d_img.copy_(torch.from_numpy(bits32(later.images)))
    D.d_counts.copy_(torch.from_numpy(bits32(later.counts)))
    buf.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    same(body(buf.cpu().numpy(), n), cases.covisibility(later, n, edges=(ea, eb)), "replay on new inputs")


# --- the chain: links -> tracks -> table -> covisibility -> candidate edges ------------------------------------------------
@pytest.mark.parametrize("consistent,min_len", [(True, 2), (False, 1), (False, 2), (True, 1)])
def test_chain(consistent, min_len, torch, handle):
    case = tcases.random_case(tcases.pool(lfp.TRACKS_DUP_TILE)[:2], 40, 5)
    io, total = np.array(case.io, np.int64), case.total
    n = len(io) - 1
    assert (np.diff(io) >= 0).all()
    words = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint32)).view(np.int32)).cuda()
    d_io, d_ea, d_eb = torch.from_numpy(io).cuda(), words(case.ea), words(case.eb)
    d_la, d_match = torch.from_numpy(case.la.astype(np.int64)).cuda(), torch.from_numpy(case.match).cuda()
    trk = [torch.empty((total,), dtype=torch.int32, device="cuda") for _ in range(3)]
    s = torch.cuda.current_stream().cuda_stream
    handle.build_tracks_device(d_io.data_ptr(), n, total, d_ea.data_ptr(), d_eb.data_ptr(), d_la.data_ptr(), case.cap, len(case.ea),
                               d_match.data_ptr(), trk[0].data_ptr(), trk[1].data_ptr(), trk[2].data_ptr(), 0, s)
    t_cap, o_cap = total // min_len, total
    off = torch.empty((t_cap + 1,), dtype=torch.int64, device="cuda")
    rows, img = (torch.empty((o_cap,), dtype=torch.int32, device="cuda") for _ in range(2))
    counts = torch.empty((4,), dtype=torch.int32, device="cuda")
    handle.track_table_device(d_io.data_ptr(), n, total, trk[0].data_ptr(), trk[1].data_ptr(), trk[2].data_ptr(), min_len,
                              lfp.TRACK_TABLE_CONSISTENT if consistent else 0, t_cap, o_cap, off.data_ptr(), rows.data_ptr(),
                              img.data_ptr(), None, counts.data_ptr(), s)
    buf = torch.full((n * n + 2 * EXTRA,), SENTINEL, dtype=torch.int32, device="cuda")
    handle.covisibility_device(off.data_ptr(), t_cap, img.data_ptr(), o_cap, counts.data_ptr(), n, d_ea.data_ptr(), d_eb.data_ptr(),
                               len(case.ea), 0, buf.data_ptr() + 4 * EXTRA, s)
    k = 4
    sel = [torch.empty((n * k,), dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.empty(4, dtype=torch.int32, device="cuda")]
    handle.select_edges_device(buf.data_ptr() + 4 * EXTRA, n, n, k, 1, lfp.SELECT_SKIP_SELF | lfp.SELECT_UNIQUE, n * k, None, None,
                               sel[0].data_ptr(), sel[1].data_ptr(), None, sel[2].data_ptr(), s)
    torch.cuda.synchronize()
    # brute force from the label array: the images of every selected label's rows, one count per pair of distinct images
    track, length, dup = trk[0].cpu().numpy(), trk[1].cpu().numpy(), trk[2].cpu().numpy()
    image_of = np.searchsorted(io, np.arange(total), side="right") - 1          # -1 and n: rows of no image
    want = np.zeros((n, n), np.uint32)
    tracks = 0
    for t in np.flatnonzero((length >= min_len) & ((dup == 0) | (not consistent))):
        seen = sorted({int(m) for m in image_of[track == t] if 0 <= m < n})
        tracks += 1
        for i in seen:
            for j in seen:
                want[i, j] += 1
    assert tracks == int(counts.cpu()[0]) > 20 and want.sum() > want.trace() > 0
    for a, b in zip(case.ea.tolist(), case.eb.tolist()):
        if a < n and b < n:
            want[a, b] = want[b, a] = 0
    got = body(buf.cpu().numpy(), n)
    same(got, want, "chain")
    ref = scases.select_edges(want, k, 1, True, True)
    assert np.array_equal(sel[0].cpu().numpy().view(np.uint32), ref.edge_a) and np.array_equal(sel[1].cpu().numpy().view(np.uint32), ref.edge_b)
    assert sel[2].cpu().numpy().view(np.uint32).tolist() == ref.counts
    listed = set(zip(case.ea.tolist(), case.eb.tolist())) | set(zip(case.eb.tolist(), case.ea.tolist()))
    assert not listed & set(zip(ref.edge_a[:ref.counts[0]].tolist(), ref.edge_b[:ref.counts[0]].tolist()))


# --- the byte marks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [23200, 32800])
def test_byte_marks(n, torch, handle):
    """tables past 2 GiB and 4 GiB with a few hundred tracks that touch the last rows; checked on the device, never copied whole"""
    assert 4 * n * n > (2 << 30 if n == 23200 else 4 << 30)
    rng = np.random.default_rng(n)
    tracks = [np.sort(np.concatenate([rng.choice(n - 8, int(rng.integers(0, 6)), replace=False), n - 1 - rng.choice(8, int(rng.integers(1, 4)), replace=False)]))
              for _ in range(300)]
    tab = cases.from_tracks(tracks)
    want = cases.pairs(tab, n)
    D = Device(torch, handle, tab, n).mask([n - 1, 5], [n - 2, n - 1])
    for key in ((n - 1, n - 2), (n - 2, n - 1), (5, n - 1), (n - 1, 5)):
        want.pop(key, None)
    assert want[n - 1, n - 1] > 20 and len(want) > 1000
    buf = D.buffer()
    buf[EXTRA:EXTRA + 1000] = 7                                                  # what it held is zeroed, far end included
    buf[EXTRA + n * n - 1000:EXTRA + n * n] = 7
    torch.cuda.synchronize()
    D.run(buf)
    torch.cuda.synchronize()
    assert (buf[:EXTRA] == SENTINEL).all() and (buf[EXTRA + n * n:] == SENTINEL).all()
    table = buf[EXTRA:EXTRA + n * n]
    assert int(torch.count_nonzero(table)) == len(want)
    assert int(table.sum(dtype=torch.int64)) == sum(want.values())
    keys = np.array(list(want), np.int64)
    flat = torch.from_numpy(keys[:, 0] * n + keys[:, 1]).cuda()
    assert np.array_equal(table[flat].cpu().numpy().astype(np.int64), np.array(list(want.values()), np.int64))
    del buf, table
    torch.cuda.empty_cache()


# --- matched pictures ------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_track_table.py::_frames
H_MILD = np.array([[0.98, -0.03, -12.0], [0.02, 0.99, 9.0], [-2e-5, 3e-5, 1.0]])     # the second, milder warp of the crop


def _frames():
    """the 1024 x 768 centre crop of houses.jpg, two perspective warps of it, and bird.jpg brought to that size (PIL images)"""
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    warps = []
    for h in (H_TRUE, H_MILD):
        hi = np.linalg.inv(h)
        hi = hi / hi[2, 2]
        warps.append(crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC))
    bird = Image.open(os.path.join(GOLDEN, "bird.jpg")).convert("L").resize((1024, 768), Image.BICUBIC)
    return [crop, warps[0], warps[1], bird]


def test_pictures(torch):
    """match_collection(frames, "window", 1, expand=1): crop - warp - second warp - bird.  The crop and the second warp are never
    matched in the first round, and the tracks through the first warp propose them.  Measured: see profiles/covisibility.md"""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=4)
    plain = ex.match_collection(frames, "window", 1, seed=21, feats=feats, table=True)
    got = ex.match_collection(frames, "window", 1, seed=21, feats=feats, expand=1)
    torch.cuda.synchronize()
    first = got["first_round"]
    # the covisibility table == the restatement on the first round's table read back
    tab = cases.Table(first["table_offsets"].cpu().numpy().view(np.uint64), first["table_images"].cpu().numpy().view(np.uint32),
                      counts=first["table_counts"].cpu().numpy().view(np.uint32))
    ea, eb = got["edge_a"].cpu().numpy(), got["edge_b"].cpu().numpy()
    assert list(zip(ea.tolist(), eb.tolist())) == [(0, 1), (1, 2), (2, 3)]
    covis = got["covisibility"].cpu().numpy().view(np.uint32)
    same(covis, cases.covisibility(tab, 4, edges=(ea, eb)), "pictures")
    print("shared tracks, first round's edges zeroed:", covis.tolist())
    # no proposed edge is on the first round's list; (crop, second warp) is proposed with at least 8 shared tracks
    kept = int(got["expand_counts"].cpu()[0])
    proposed = list(zip(got["expand_edge_a"].cpu().tolist()[:kept], got["expand_edge_b"].cpu().tolist()[:kept]))
    assert not set(proposed) & ({(0, 1), (1, 2), (2, 3)} | {(1, 0), (2, 1), (3, 2)})
    assert (0, 2) in proposed and covis[0, 2] == covis[2, 0] >= 8
    assert all(covis[a, b] >= 8 for a, b in proposed)
    assert int(got["expand_per_edge"][proposed.index((0, 2)), 1]) >= 8
    # the expanded forest == one build_tracks call over both rounds' links
    m = got["track"].numel()
    la, xla = got["layout_a"], got["expand_layout_a"]
    used, xused = int(la[-1]), int(xla[-1])
    both = feats.build_tracks(got["offsets"], torch.cat([got["edge_a"], got["expand_edge_a"]]), torch.cat([got["edge_b"], got["expand_edge_b"]]),
                              torch.cat([la, xla[1:] + used]), torch.cat([got["verified"][:used], got["expand_verified"][:xused]]).contiguous(),
                              n_rows=m)
    torch.cuda.synchronize()
    for name, x in zip(("track", "track_len", "track_dup"), both):
        assert torch.equal(x, got[name]), name
    assert int(got["track_counts"][4]) >= int(first["track_counts"][4])
    assert not torch.equal(got["track"], plain["track"])                         # the second round did tie tracks together
    # without expand: the new entries are None, and every old entry is what the first round of the expanded run computed
    for key in ("covisibility", "expand_edge_a", "expand_edge_b", "expand_counts", "first_round"):
        assert plain[key] is None
    for key in ("edge_a", "edge_b", "offsets", "keypoints", "q8", "layout_a", "layout_b", "model", "stats", "per_edge"):
        assert torch.equal(plain[key], got[key]), key
    for key in ("match", "verified"):                                            # (entries behind the layout are left as allocated)
        assert torch.equal(plain[key][:used], got[key][:used]), key
    n_obs = int(first["table_counts"][1])
    for key in first:
        cut = n_obs if key in ("table_rows", "table_images") else None           # (so are the entries behind the observations)
        assert torch.equal(plain[key][:cut], first[key][:cut]), key


# --- the example -----------------------------------------------------------------------------------------------------------
def test_match_collection_example_with_expand(tmp_path):
    """examples/match_collection.py --window 1 --table prints what it printed; --expand 1 prints those lines, then its own"""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_collection.py")
    old = subprocess.run([sys.executable, exe, "--window", "1", "--table"] + paths, capture_output=True, text=True, timeout=600)
    out = subprocess.run([sys.executable, exe, "--window", "1", "--expand", "1"] + paths, capture_output=True, text=True, timeout=600)
    assert old.returncode == 0 and out.returncode == 0, out.stderr
    was, lines = old.stdout.splitlines(), out.stdout.splitlines()
    print("\n".join(lines))
    assert len(was) >= 8 and was[0].startswith("Extracted ") and was[4].startswith("Tracks: ") and was[6].startswith("Track table: ")
    assert lines[:len(was)] == was
    m = re.match(r"Expanded: (\d+) edges proposed from the tracks two unmatched images share \(at least 8\), (\d+) of them with "
                 r"verified matches$", lines[len(was)])
    assert m and 1 <= int(m.group(2)) <= int(m.group(1)) <= 4, lines[len(was)]
    rest = lines[len(was) + 1:]
    assert rest[0].startswith("Tracks: ") and rest[1].startswith("Longest track: ") and rest[2].startswith("Track table: ")
    assert all(line.startswith("Track %d: " % (k + 1)) for k, line in enumerate(rest[3:])) and len(rest) <= 6
    longest = lambda line: int(re.match(r"Longest track: (\d+) keypoints", line).group(1))
    assert longest(rest[1]) >= longest(was[5])
