"""Link tables on the GPU (lf_mkd_link_table_device; LocalFeatures.link_table): every output equals the numpy restatement's
(tests/link_table_cases.py) -- every comparison is ==, the entries behind every array included.  The shared track cases with
and without the flag, the optional outputs and the in-place form, links at the ends of waves and slots, edge counts that cross
every level of the slot scan, selection and capacity cuts, arrays of anything, two runs and permuted edges, the hand-off to
lf_mkd_build_tracks_device, the gather, graph capture, matched pictures and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import link_table_cases as cases
import tracks_cases as tcases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # entries every array is longer than needed
SENTINEL = tcases.SENTINEL
TILE = lfp.TRACKS_DUP_TILE
NAMES = ("offsets", "link_a", "link_b", "link_edge", "edge_links", "match_kept", "counts")
S, _, F, _, _ = lfp.link_table_plan(0, 0)


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
    """a case's arrays on the device -- the match array EXTRA sentinels longer than its size --, and sentinel-filled outputs
    EXTRA entries longer than needed"""

    def __init__(self, torch, handle, case):
        self.torch, self.handle, self.case = torch, handle, case
        self.n_edges = len(case.ea)
        self.d_io = torch.from_numpy(np.array(case.io, np.int64)).cuda()
        self.d_ea, self.d_eb = torch.from_numpy(bits32(case.ea)).cuda(), torch.from_numpy(bits32(case.eb)).cuda()
        self.d_la = torch.from_numpy(np.asarray(case.la).astype(np.int64)).cuda()
        self.padded = np.concatenate([case.match, np.full(EXTRA, SENTINEL, np.int32)])
        self.d_match = torch.from_numpy(self.padded).cuda()

    def outputs(self, l_cap):
        t = self.torch
        full = lambda n, dtype=t.int32: t.full((n + EXTRA,), SENTINEL, dtype=dtype, device="cuda")
        return [full(self.n_edges + 1, t.int64), full(l_cap), full(l_cap), full(l_cap), full(self.n_edges), full(self.case.size), full(4)]

    def run(self, out, min_links=0, local=False, l_cap=None, cap=None, skip=(), in_place=False, stream=None, n_images=None):
        l_cap = self.case.cap if l_cap is None else l_cap
        ptr = lambda k: None if NAMES[k] in skip or (k in (1, 2, 3) and l_cap == 0) else out[k].data_ptr()
        self.handle.link_table_device(
            self.d_io.data_ptr(), len(self.case.io) - 1 if n_images is None else n_images, self.case.total,
            self.d_ea.data_ptr() if self.n_edges else None, self.d_eb.data_ptr() if self.n_edges else None, self.d_la.data_ptr(),
            self.case.cap if cap is None else cap, self.n_edges, self.d_match.data_ptr(), min_links,
            lfp.LINK_TABLE_LOCAL if local else 0, l_cap, out[0].data_ptr(), ptr(1), ptr(2), ptr(3), ptr(4),
            self.d_match.data_ptr() if in_place else ptr(5), out[6].data_ptr(),
            self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def call(self, l_cap=None, **kw):
        l_cap = self.case.cap if l_cap is None else l_cap
        out = self.outputs(l_cap)
        self.torch.cuda.synchronize()
        self.run(out, l_cap=l_cap, **kw)
        self.torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in out]
        if kw.get("in_place"):
            got[5] = self.d_match.cpu().numpy()
            self.d_match.copy_(self.torch.from_numpy(self.padded).cuda())      # as it was, for the next call
        return got


def tailed(table, n_edges, size, l_cap, skip=()):
    """a restatement's Table as the device arrays hold it: entries beyond O and the EXTRA entries behind still sentinels"""
    def tail(x, n, dtype=np.int32):
        return np.concatenate([np.asarray(x, dtype), np.full(n + EXTRA - len(x), SENTINEL, dtype)])
    o = table.counts[1]
    assert len(table.link_a) == len(table.link_b) == len(table.link_edge) == o <= l_cap and len(table.match_kept) == size + EXTRA
    pick = lambda name, x: [] if name in skip else x
    return [tail(table.offsets.astype(np.int64), n_edges + 1, np.int64), tail(pick("link_a", table.link_a), l_cap),
            tail(pick("link_b", table.link_b), l_cap), tail(pick("link_edge", bits32(table.link_edge)), l_cap),
            tail(pick("edge_links", bits32(table.edge_links)), n_edges),
            table.match_kept if "match_kept" not in skip else np.full(size + EXTRA, SENTINEL, np.int32), tail(bits32(table.counts), 4)]


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def check(D, what, vectorised=False, min_links=0, local=False, l_cap=None, skip=(), in_place=False):
    c = D.case
    into = D.padded if in_place else np.full(c.size + EXTRA, SENTINEL, np.int32)
    want = cases.of_case(c, vectorised, min_links=min_links, link_capacity=l_cap, local=local, into=into)
    got = D.call(l_cap, min_links=min_links, local=local, skip=skip, in_place=in_place)
    if l_cap == 0:
        skip = tuple(skip) + ("link_a", "link_b", "link_edge")
    same(got, tailed(want, D.n_edges, c.size, c.cap if l_cap is None else l_cap, skip), what)
    return want


# --- the shared track cases ------------------------------------------------------------------------------------------------
SHARED = dict(cases.shared_cases(TILE))


@pytest.mark.parametrize("name", list(SHARED))
def test_shared_cases(name, torch, handle):
    """the 3197-row pool (images of 0, 1, 63 .. 65, 255 .. 257 and 2 S + 1 rows, S = the slot) and the odd pool, with and
    without the flag, in place and out of place, with every optional output NULL in turn"""
    assert TILE == S                                                          # the dup tile the pool is built around is the slot
    D = Device(torch, handle, SHARED[name])
    want = check(D, (name, "pool rows"))
    u, v = D.case.links()
    assert np.array_equal(want.link_a, u) and np.array_equal(want.link_b, v)
    check(D, (name, "local"), local=True)
    check(D, (name, "in place"), in_place=True)
    check(D, (name, "in place, min_links 2"), in_place=True, min_links=2, local=True)
    for out in ("link_edge", "edge_links", "match_kept"):
        check(D, (name, "without", out), skip=(out,))
    check(D, (name, "without any"), skip=("link_edge", "edge_links", "match_kept"), min_links=1)


# --- where the links sit ---------------------------------------------------------------------------------------------------
def test_link_placement(torch, handle):
    io, total, names = tcases.pool(TILE)
    L, X, W, e1, s63, s256 = (names[k] for k in ("L", "X", "W", "e1", "s63", "s256"))
    n_images = len(io) - 1
    nW, nX = tcases.rows_of((io, total), W), tcases.rows_of((io, total), X)
    edges = [(L, W),                      # 0: its only link in the last lane of the last wave of its last full slot ...
             (L, X),                      # 1: ... and in the one entry of its last slot
             (X, W),                      # 2: every entry a link
             (W, X),                      # 3: none
             (X, X),                      # 4: a self edge
             (X, W),                      # 5: edge 2 once more
             (W, X), (X, W),              # 6, 7: (j, i) beside (i, j)
             (n_images, X), (X, n_images + 7), (tcases.NO_IMAGE, W),   # 8 .. 10: ids at and beyond n_images
             (s63, e1),                   # 11: the values around nB = 1
             (X, W),                      # 12: the values around nB
             (s256, W)]                   # 13: S rows, its only link in the last lane of the last wave of its one slot
    triples = [(0, 2 * S - 1, 4), (1, 2 * S, 9), (13, S - 1, 2)]
    assert tcases.rows_of((io, total), s256) == S == 256
    triples += [(2, r, (7 * r) % nW) for r in range(nX)] + [(5, r, (3 * r + 1) % nW) for r in range(nX)]
    triples += [(4, r, r) for r in range(0, nX, 3)]
    triples += [(6, r, r % nX) for r in range(0, nW, 2)] + [(7, r, r) for r in range(1, nX, 2)]
    triples += [(9, r, 0) for r in range(nX)] + [(11, 0, 0), (11, 1, 1), (11, 2, -1), (11, 3, cases.INT32_MIN), (11, 62, 0)]
    triples += [(12, 0, nW), (12, 1, nW - 1), (12, 2, -1), (12, 3, cases.INT32_MIN), (12, 4, tcases.INT32_MAX), (12, nX - 1, 0)]
    case = tcases.Case((io, total), edges, triples)
    D = Device(torch, handle, case)
    want = check(D, "placement")
    assert want.edge_links.tolist() == [1, 1, nX, 0, len(range(0, nX, 3)), nX, len(range(0, nW, 2)), len(range(1, nX, 2)), 0, 0, 0, 2, 2, 1]
    assert want.edge(0)[0].tolist() == [int(io[L]) + 2 * S - 1] and want.edge(1)[0].tolist() == [int(io[L]) + 2 * S]
    assert want.edge(11)[0].tolist() == [int(io[s63]), int(io[s63]) + 62] and want.edge(12)[1].tolist() == [int(io[W]) + nW - 1, int(io[W])]
    check(D, "placement, local, in place", local=True, in_place=True)
    check(D, "placement, min_links 2", min_links=2)
    check(D, "placement, a capacity", min_links=1, l_cap=int(want.offsets[6]) + 3)


# --- edge counts that cross every level of the scan over the slots -----------------------------------------------------------
@pytest.mark.parametrize("n_edges", [1, F - 1, F, F + 3] + ([F * F, F * F + 3] if F * F + 3 <= 2 ** 21 else []))
def test_scan_boundaries(n_edges, torch, handle):
    """many edges of 0- to 2-row images: the slots are the edges.  The reference is the vectorised formulation."""
    case = cases.tiny_edges(n_edges, n_edges)
    levels = lfp.link_table_plan(case.cap, n_edges)[3]
    assert levels == (1 if case.cap // S + n_edges <= F else 2 if case.cap // S + n_edges <= F * F else 3)
    D = Device(torch, handle, case)
    want = check(D, ("scan", n_edges), vectorised=True)
    assert n_edges < F or (want.counts[1] > n_edges // 8 and (want.edge_links == 2).any() and (want.edge_links == 0).any())
    check(D, ("scan, min_links 2, local", n_edges), vectorised=True, min_links=2, local=True, in_place=True)
    check(D, ("scan, cut", n_edges), vectorised=True, min_links=1, l_cap=want.counts[1] * 3 // 5)


def test_no_edges(torch, handle):
    case = tcases.Case(tcases.pool(TILE)[:2], [], [], extra=5)
    got = Device(torch, handle, case).call(3)
    assert got[0][:1].tolist() == [0] and (got[0][1:] == SENTINEL).all() and got[6][:4].tolist() == [0, 0, 0, 0]
    assert all((g == SENTINEL).all() for g in got[1:6]) and (got[6][4:] == SENTINEL).all()


# --- selection and cut -------------------------------------------------------------------------------------------------------
def test_selection_and_cut(torch, handle):
    case = tcases.random_case(tcases.odd_pool(), 30, 3)
    D = Device(torch, handle, case)
    full = check(D, "all")
    L = full.edge_links
    e = int(np.argsort(L)[len(L) // 2])
    assert L[e] >= 2
    for m in (int(L[e]) - 1, int(L[e]), int(L[e]) + 1, 2 ** 32 - 1):
        want = check(D, ("min_links", m), min_links=m)
        assert want.counts[2] == int((L >= m).sum()) and want.counts[3] == int(L[L >= m].sum()) and want.counts[:2] == want.counts[2:]
        assert (len(want.edge(e)[0]) > 0) == (m <= L[e])
    sel = cases.of_case(case, min_links=2)
    W = sel.offsets.astype(np.int64)
    marks = sorted({int(W[k]) for k in (3, len(W) // 2, len(W) - 1)})
    assert len(marks) == 3 and marks[0] > 0
    for l_cap in [0] + [w + d for w in marks for d in (-1, 0, 1)]:
        want = check(D, ("link_capacity", l_cap), min_links=2, l_cap=l_cap, in_place=l_cap % 2 == 1)
        assert want.counts[1] <= l_cap and want.counts[2:] == sel.counts[2:]   # what was wanted is reported whatever was cut
        assert want.counts[1] == max(w for w in W if w <= l_cap)


# --- whatever the arrays hold ------------------------------------------------------------------------------------------------
def test_arrays_of_anything(torch, handle):
    """arbitrary int32 in the edge ids and the match array, a layout that decreases, offsets beyond the totals: the call
    returns, d_counts[1] <= link_capacity and nothing behind O, n_edges + 1 or ea_capacity is written"""
    rng = np.random.default_rng(71)
    base = tcases.random_case(tcases.pool(TILE)[:2], 60, 13)
    for kind in ("content", "decreasing layout", "offsets beyond"):
        case = tcases.random_case(tcases.pool(TILE)[:2], 60, 13)
        io = np.array(case.io)
        if kind == "content":
            case.ea = rng.integers(0, 2 ** 32, 60).astype(np.uint32)
            case.eb = rng.integers(0, 2 ** 32, 60).astype(np.uint32)
            case.ea[::3], case.eb[::2] = base.ea[::3], base.eb[::2]
            case.match = rng.integers(-2 ** 31, 2 ** 31, case.size).astype(np.int32)
            case.match[::2] = rng.integers(0, 3, len(case.match[::2]))
        elif kind == "decreasing layout":
            la = np.array(case.la)
            la[1:-1] = rng.permutation(la[1:-1])
            la[7], la[20] = 2 ** 40, 2 ** 63 + 5
            case.la = la
        else:
            io[len(io) // 2:] += case.total
            io[5] = 2 ** 62
            case.io = io
            case.la = np.array(case.la) + np.uint64(case.size // 2)
        D = Device(torch, handle, case)
        for min_links, l_cap, cap in ((0, case.size, case.size), (2, 150, case.size - 9), (1, 0, case.size)):
            out = D.outputs(l_cap)
            torch.cuda.synchronize()
            D.run(out, min_links=min_links, l_cap=l_cap, cap=cap)
            torch.cuda.synchronize()
            got = [x.cpu().numpy() for x in out]
            o = int(got[6][1])
            assert 0 <= o <= l_cap and int(got[6][0]) <= 60, (kind, min_links, got[6][:4])
            for name, g, used in zip(NAMES, got, (61, o, o, o, 60, cap, 4)):
                assert (g[used:] == SENTINEL).all(), (kind, name, min_links)
            assert (got[0][:61] <= o).all() and (got[0][:61] >= 0).all()
            if kind == "content":                                              # the layout is in order: the restatement holds
                want = cases.link_table(case.io, case.total, case.ea, case.eb, case.la, cap, case.match, min_links, l_cap,
                                        into=np.full(case.size + EXTRA, SENTINEL, np.int32))
                skip = ("link_a", "link_b", "link_edge") if l_cap == 0 else ()
                same(got, tailed(want, 60, case.size, l_cap, skip), (kind, min_links))


# --- determinism -------------------------------------------------------------------------------------------------------------
def test_two_runs_and_permuted_edges(torch, handle):
    case = SHARED["odd pool"]
    D = Device(torch, handle, case)
    first = D.call(min_links=2)
    same(D.call(min_links=2), first, "two runs")
    want = cases.of_case(case, min_links=2)
    order = np.random.default_rng(5).permutation(len(case.ea))
    moved = case.permuted(order)
    got = check(Device(torch, handle, moved), "permuted", min_links=2)
    assert got.counts == want.counts
    for k, e in enumerate(order):                                              # per edge the same lists
        assert all(np.array_equal(x, y) for x, y in zip(got.edge(k), want.edge(e)))


# --- the hand-off to the tracks and the gather -----------------------------------------------------------------------------
def test_match_kept_builds_the_tracks_of_the_kept_edges(torch, handle):
    case = SHARED["cycles"]
    D = Device(torch, handle, case)
    for min_links, l_cap in ((0, None), (2, None), (100, 310)):
        want = cases.of_case(case, min_links=min_links, link_capacity=l_cap, into=case.match)
        out = D.outputs(case.cap if l_cap is None else l_cap)
        track = [torch.full((case.total,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        D.run(out, min_links=min_links, l_cap=l_cap)
        handle.build_tracks_device(D.d_io.data_ptr(), len(case.io) - 1, case.total, D.d_ea.data_ptr(), D.d_eb.data_ptr(),
                                   D.d_la.data_ptr(), case.cap, D.n_edges, out[5].data_ptr(), track[0].data_ptr(),
                                   track[1].data_ptr(), track[2].data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref = case.reference(match=want.match_kept)
        assert all(np.array_equal(bits32(g.cpu().numpy()), bits32(w)) for g, w in zip(track, ref)), min_links
        only = tcases.components(tcases.forest(case.total), want.link_a.astype(np.int64), want.link_b.astype(np.int64))
        assert np.array_equal(only.astype(np.int32), ref[0])                  # the tracks of the table's links alone
    assert want.counts[:2] == [2, 300] and want.counts[2] == 3                # the third 150-link edge did not fit


def test_gather(torch, handle):
    case = SHARED["odd pool"]
    D = Device(torch, handle, case)
    l_cap = case.cap
    out = D.outputs(l_cap)
    torch.cuda.synchronize()
    D.run(out, min_links=3)
    want = cases.of_case(case, min_links=3)
    o = want.counts[1]
    assert 100 < o < l_cap
    kps = np.random.default_rng(3).random((case.total, 5), dtype=np.float32)
    d_src = torch.from_numpy(kps).cuda()
    for k, rows in ((1, want.link_a), (2, want.link_b)):
        d_dst = torch.from_numpy(np.full((l_cap + EXTRA, 5), 7, np.float32)).cuda()
        handle.gather_track_rows_device(d_src.data_ptr(), 20, case.total, out[k].data_ptr(), out[6].data_ptr(), l_cap, d_dst.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        assert np.array_equal(got[:o], kps[rows]) and (got[o:] == 7).all()


# --- capture ---------------------------------------------------------------------------------------------------------------
def test_capturable(torch, handle):
    """one capture of the warmed-up call, replayed after the match array has been overwritten in place"""
    case = tcases.random_case(tcases.odd_pool(), 30, 3)
    later = tcases.random_case(tcases.odd_pool(), 30, 3, share=0.7)
    assert np.array_equal(case.la, later.la) and not np.array_equal(case.match, later.match)
    D = Device(torch, handle, case)
    check(D, "warm-up", min_links=3)
    out = D.outputs(case.cap)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(out, min_links=3, stream=torch.cuda.current_stream().cuda_stream)
    for first in (True, False):
        for x in out:
            x.fill_(SENTINEL)
        if not first:
            D.d_match[:case.size] = torch.from_numpy(later.match).cuda()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c = case if first else later
        want = cases.of_case(c, min_links=3, into=np.full(c.size + EXTRA, SENTINEL, np.int32))
        same([x.cpu().numpy() for x in out], tailed(want, D.n_edges, c.size, c.cap), ("replay", first))
    g.replay()
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in out], tailed(want, D.n_edges, c.size, c.cap), "replay twice")
    assert want.counts[1] > cases.of_case(case, min_links=3).counts[1]


# --- matched pictures ------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_track_table.py::_frames


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
    """match_collection(..., pairs=True, min_inliers=M) on houses, its crop-and-warp and bird.jpg: the table equals the
    restatement of the returned `verified`, the tracks equal build_tracks of the pruned array"""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    M = 30
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "all", seed=21, feats=feats, pairs=True, min_inliers=M, tracks=True)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in got.items() if v is not None}
    io, kps, ver = host["offsets"], host["keypoints"], host["verified"]
    n, cap = len(kps), len(ver)
    ea, eb, la = host["edge_a"].view(np.uint32), host["edge_b"].view(np.uint32), host["layout_a"]
    want = cases.link_table(io, n, ea, eb, la, cap, ver, min_links=M, into=np.full(cap, -1, np.int32))
    assert np.array_equal(want.edge_links, host["per_edge"][:, 2])            # the ranking line's count
    print("verified per edge:", want.edge_links.tolist(), "counts:", want.counts)
    assert want.edge_links[0] >= M and want.counts[0] == int((want.edge_links >= M).sum())   # houses and its warp are supported
    assert host["link_counts"].view(np.uint32).tolist() == want.counts
    o = want.counts[1]
    assert np.array_equal(host["link_offsets"], want.offsets.astype(np.int64)) and len(host["link_a"]) == cap
    assert np.array_equal(host["link_a"][:o], want.link_a) and np.array_equal(host["link_b"][:o], want.link_b)
    assert np.array_equal(host["link_edge"][:o].view(np.uint32), want.link_edge)
    assert np.array_equal(host["edge_links"].view(np.uint32), want.edge_links)
    assert np.array_equal(host["match_kept"], want.match_kept)
    ka, kb = host["link_keypoints_a"], host["link_keypoints_b"]
    assert np.array_equal(ka[:o], kps[want.link_a]) and np.array_equal(kb[:o], kps[want.link_b]) and (ka[o:] == 0).all()
    ref = tcases.build_tracks(io, n, ea, eb, la, cap, want.match_kept)
    assert all(np.array_equal(bits32(host[k]), bits32(w)) for k, w in zip(("track", "track_len", "track_dup"), ref))
    # without the new arguments the new entries are None and the rest is what it was
    plain = ex.match_collection(frames, "all", seed=21, feats=feats, tracks=True)
    used = int(la[-1])                                                         # (entries behind the last edge are nobody's)
    assert plain["link_a"] is None and plain["match_kept"] is None and torch.equal(plain["verified"][:used], got["verified"][:used])
    if (want.edge_links[1:] > 0).any():                                        # unsupported edges had links: the tracks differ
        assert (plain["track_len"] >= 2).sum() >= (got["track_len"] >= 2).sum()


# --- the example -----------------------------------------------------------------------------------------------------------
def test_match_collection_example_with_pairs(tmp_path):
    """examples/match_collection.py --all --tracks --table on three generated frames prints the lines of today, and with --pairs
    the new ones after them"""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_collection.py")
    old = subprocess.run([sys.executable, exe, "--all", "--tracks", "--table"] + paths, capture_output=True, text=True, timeout=600)
    out = subprocess.run([sys.executable, exe, "--all", "--tracks", "--table", "--pairs"] + paths, capture_output=True, text=True, timeout=600)
    assert old.returncode == 0 and out.returncode == 0, out.stderr
    before, lines = old.stdout.splitlines(), out.stdout.splitlines()
    print("\n".join(lines))
    assert re.match(r"Track table: (\d+) tracks", before[6]) and lines[:len(before)] == before
    new = lines[len(before):]
    m = re.match(r"Link table: (\d+) edges, (\d+) correspondences$", new[0])
    assert m and int(m.group(1)) == 3
    agree = [int(re.match(r"Edge \d+ -> \d+: \d+ matches, \d+ mutual, (\d+) agree", x).group(1)) for x in before[1:4]]
    assert int(m.group(2)) == sum(agree) and agree[0] >= 30
    assert len(new) == 4
    best = re.match(r"Edge (\d+ -> \d+):", before[1]).group(1)
    for line in new[1:]:
        assert re.match(r"Edge %s: -?[0-9.]+,-?[0-9.]+ -> -?[0-9.]+,-?[0-9.]+$" % best, line), line
