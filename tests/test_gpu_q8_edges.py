"""Edge-list matching over 8-bit descriptors on the GPU (lf_mkd_edge_layout_device, lf_mkd_gather_edge_rows_device,
lf_mkd_match_q8_edges_device; LocalFeatures.edge_layout / gather_edge_rows / match_q8_edges): every edge of a pool decided
exactly as the numpy integer product decides its two images and as lf_mkd_match_q8_pairs_device decides the same rows once they
are copied into pair layout -- every comparison is ==.  Two pools, capacities cut short mid-edge, independence of the edge
list, graph capture, the layout and the gather on their own, frames to verified matches, and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_pairs_cases as pcases
import q8_edges_cases as cases
import q8_pairs_cases as pq
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # entries every output array is longer than needed
SENTINEL = cases.SENTINEL
RATIO = float(cases.RATIO)
NAMES = ("match_ab", "match_ba", "best", "second")


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


def words(torch, x):
    """uint32 values as an int32 device tensor of their bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint32)).view(np.int32)).cuda()


class Edges:
    """Two pools and an edge list on the device; layouts made by lf_mkd_edge_layout_device; outputs EXTRA entries longer than
    the capacities and sentinel-filled."""

    def __init__(self, torch, handle, qa, ioa, qb, iob, ea, eb):
        self.torch, self.handle = torch, handle
        self.qa, self.qb = np.array(qa, np.uint8, order="C"), np.array(qb, np.uint8, order="C")
        self.ioa, self.iob = np.array(ioa, np.int64), np.array(iob, np.int64)
        self.ea, self.eb = np.array(ea, np.uint32), np.array(eb, np.uint32)
        self.n_edges = len(self.ea)
        self.d_a, self.d_b = torch.from_numpy(self.qa).cuda(), torch.from_numpy(self.qb).cuda()
        self.d_ioa, self.d_iob = torch.from_numpy(self.ioa).cuda(), torch.from_numpy(self.iob).cuda()
        self.d_ea, self.d_eb = words(torch, self.ea), words(torch, self.eb)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.d_la, self.d_lb = self.layout(self.d_ioa, len(self.qa), self.d_ea), self.layout(self.d_iob, len(self.qb), self.d_eb)
        torch.cuda.synchronize()
        self.la, self.lb = self.d_la.cpu().numpy().astype(np.uint64), self.d_lb.cpu().numpy().astype(np.uint64)
        self.cap_a, self.cap_b = int(self.la[-1]), int(self.lb[-1])

    def layout(self, d_io, total, d_edge):
        out = self.torch.full((d_edge.numel() + 1,), -1, dtype=self.torch.int64, device="cuda")
        self.handle.edge_layout_device(d_io.data_ptr(), d_io.numel() - 1, total, d_edge.data_ptr(), d_edge.numel(), out.data_ptr(),
                                       self.stream)
        return out

    def outputs(self, cap_a=None, cap_b=None):
        t = self.torch
        ca, cb = self.cap_a if cap_a is None else cap_a, self.cap_b if cap_b is None else cap_b
        return [t.full((n + EXTRA,), SENTINEL, dtype=t.int32, device="cuda") for n in (ca, cb, ca, ca)]

    def run(self, out, cap_a=None, cap_b=None, ratio=RATIO, flags=0, both=True, scores=True, edges=None, n_edges=None, stream=None):
        ca, cb = self.cap_a if cap_a is None else cap_a, self.cap_b if cap_b is None else cap_b
        d_ea, d_eb, d_la, d_lb = edges if edges is not None else (self.d_ea, self.d_eb, self.d_la, self.d_lb)
        self.handle.match_q8_edges_device(
            self.d_a.data_ptr(), self.d_ioa.data_ptr(), len(self.ioa) - 1, len(self.qa), self.d_b.data_ptr(), self.d_iob.data_ptr(),
            len(self.iob) - 1, len(self.qb), d_ea.data_ptr(), d_eb.data_ptr(), d_la.data_ptr(), ca, d_ea.numel() if n_edges is None else n_edges, out[0].data_ptr(),
            d_lb.data_ptr() if both else None, cb if both else 0, out[1].data_ptr() if both else None, ratio, flags,
            out[2].data_ptr() if scores else None, out[3].data_ptr() if scores else None, self.stream if stream is None else stream)

    def call(self, cap_a=None, cap_b=None, **kw):
        out = self.outputs(cap_a, cap_b)
        self.torch.cuda.synchronize()
        self.run(out, cap_a, cap_b, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]

    def reference(self, cap_a=None, cap_b=None, ratio=RATIO):
        """the numpy restatement with the same capacities, the EXTRA entries behind them still sentinels"""
        ca, cb = self.cap_a if cap_a is None else cap_a, self.cap_b if cap_b is None else cap_b
        want = cases.match_edges(self.qa, self.ioa, self.qb, self.iob, self.ea, self.eb, self.la, ca, self.lb, cb, np.float32(ratio))
        return [np.concatenate([w, np.full(EXTRA, SENTINEL, np.int32)]) for w in want]


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def filtered(want, la, lb):
    """LF_MKD_MATCH_MUTUAL on a reference [ab, ba, best, second] (with their EXTRA tails): best / second are not filtered"""
    ab, ba = pcases.mutual(want[0][:-EXTRA], want[1][:-EXTRA], la.astype(np.int64), lb.astype(np.int64))
    tail = np.full(EXTRA, SENTINEL, np.int32)
    return [np.concatenate([ab, tail]), np.concatenate([ba, tail]), want[2], want[3]]


@pytest.fixture(scope="module")
def shared(torch, handle, R):
    q, io, _, _, ea, eb = cases.shared_pool(R)
    return Edges(torch, handle, q, io, q, io, ea, eb)


@pytest.fixture(scope="module")
def shared_want(shared, R):
    la, lb, want = cases.shared_reference(R)
    assert np.array_equal(shared.la, la) and np.array_equal(shared.lb, lb)         # the device's layouts are the restatement's
    return [np.concatenate([w, np.full(EXTRA, SENTINEL, np.int32)]) for w in want]


@pytest.fixture(scope="module")
def shared_out(shared):
    return shared.call()


# --- (a) --------------------------------------------------------------------------------------------------------------
def test_every_edge_equals_the_integer_product_and_the_pairs_call(shared, shared_out, shared_want, handle, torch, R):
    E = shared
    same(shared_out, shared_want, "shared pool")
    got_mutual = E.call(flags=lfp.MATCH_MUTUAL)
    same(got_mutual, filtered(shared_want, E.la, E.lb), "shared pool, mutual")
    kept, fwd = (got_mutual[0] >= 0).sum(), (shared_out[0] >= 0).sum()
    assert 0 < kept < fwd and kept == (got_mutual[1] >= 0).sum()
    # the parent's route: the rows copied into pair layout by the gather call, then lf_mkd_match_q8_pairs_device on the layouts
    ga = torch.zeros((E.cap_a, 128), dtype=torch.uint8, device="cuda")
    gb = torch.zeros((E.cap_b, 128), dtype=torch.uint8, device="cuda")
    for src, d_io, d_e, d_l, cap, dst in ((E.d_a, E.d_ioa, E.d_ea, E.d_la, E.cap_a, ga), (E.d_b, E.d_iob, E.d_eb, E.d_lb, E.cap_b, gb)):
        handle.gather_edge_rows_device(src.data_ptr(), 128, d_io.data_ptr(), d_io.numel() - 1, src.shape[0], d_e.data_ptr(),
                                       d_l.data_ptr(), cap, E.n_edges, dst.data_ptr(), E.stream)
    for flags, want in ((0, shared_out), (lfp.MATCH_MUTUAL, got_mutual)):
        out = E.outputs()
        handle.match_q8_pairs_device(ga.data_ptr(), E.d_la.data_ptr(), E.cap_a, gb.data_ptr(), E.d_lb.data_ptr(), E.cap_b, E.n_edges,
                                     out[0].data_ptr(), out[1].data_ptr(), RATIO, flags, out[2].data_ptr(), out[3].data_ptr(), E.stream)
        torch.cuda.synchronize()
        same([x.cpu().numpy() for x in out], want, ("pairs call on gathered rows", flags))
    # one direction only, and without the scores: the same values, and what was not asked for is not written
    one_way, no_scores = E.call(both=False), E.call(scores=False)
    assert np.array_equal(one_way[0], shared_out[0]) and (one_way[1] == SENTINEL).all() and np.array_equal(one_way[2], shared_out[2])
    assert np.array_equal(no_scores[0], shared_out[0]) and np.array_equal(no_scores[1], shared_out[1]) \
        and (no_scores[2] == SENTINEL).all() and (no_scores[3] == SENTINEL).all()
    same(E.call(ratio=0.0), E.reference(ratio=0.0), "ratio 0")
    with pytest.raises(RuntimeError, match="match_q8_edges_device: LF_MKD_MATCH_MUTUAL needs d_match_ba"):
        E.run(E.outputs(), flags=lfp.MATCH_MUTUAL, both=False)


# --- (b) --------------------------------------------------------------------------------------------------------------
def test_two_pools(torch, handle, R):
    """a query pool of 4 images against a database pool of 7: other offsets, other image counts, ids that exist in one pool only"""
    qa, ioa, _, _ = cases.make_pool([40, 200, 0, R + 3], 9201)
    qb, iob, _, _ = cases.make_pool([300, 33, 64, 1, 257, 129, 2], 9202)
    i, j = np.divmod(np.arange(4 * 7), 7)
    ea = np.concatenate([i, [3, 5, 1]]).astype(np.uint32)        # (5, 4): no such query image; (3, 6) twice
    eb = np.concatenate([j, [6, 4, 7]]).astype(np.uint32)        # (1, 7): no such database image
    E = Edges(torch, handle, qa, ioa, qb, iob, ea, eb)
    assert np.array_equal(E.la, cases.edge_layout(ioa, len(qa), ea)) and np.array_equal(E.lb, cases.edge_layout(iob, len(qb), eb))
    want = E.reference()
    same(E.call(), want, "two pools")
    same(E.call(flags=lfp.MATCH_MUTUAL), filtered(want, E.la, E.lb), "two pools, mutual")
    assert (want[0][:-EXTRA] >= 0).any()


# --- (c) --------------------------------------------------------------------------------------------------------------
def test_short_capacities(shared, shared_out, R):
    """capacities that end in the middle of an edge: nothing at or beyond them is written, everything below them is as before"""
    E = shared
    n_images = len(E.ioa) - 1
    big = int(np.argmax(np.diff(E.ioa)))                                          # the image of 2 R + 1 rows
    e = big * n_images + 4
    cuts = [(int(E.la[e]) + R + 9, int(E.lb[e + 40]) + 1), (int(E.la[7]) + 1, E.cap_b), (E.cap_a, int(E.lb[e])), (0, 0)]
    assert E.la[e] + R + 9 < E.la[e + 1] and E.lb[e + 40] + 1 < E.lb[e + 41]       # both really are mid-edge
    for cap_a, cap_b in cuts:
        for flags in (0, lfp.MATCH_MUTUAL):
            got = E.call(cap_a, cap_b, flags=flags)
            want = E.reference(cap_a, cap_b)
            if flags:
                want = filtered(want, E.la, E.lb)
            same(got, want, ("short", cap_a, cap_b, flags))
            if flags == 0:
                for k, cap in ((0, cap_a), (1, cap_b), (2, cap_a), (3, cap_a)):
                    assert np.array_equal(got[k][:cap], shared_out[k][:cap]) and (got[k][cap:] == SENTINEL).all(), (k, cap_a, cap_b)


# --- (d) --------------------------------------------------------------------------------------------------------------
def test_independent_and_capturable(shared, shared_out, torch):
    E = shared
    # a subset of the edges, in another order: every edge's entries are what they were in the full list
    pick = np.concatenate([np.arange(E.n_edges - 1, -1, -7), [5, 5]])
    S = Edges(torch, E.handle, E.qa, E.ioa, E.qb, E.iob, E.ea[pick], E.eb[pick])
    for flags in (0, lfp.MATCH_MUTUAL):
        sub, full = S.call(flags=flags), (shared_out if flags == 0 else E.call(flags=flags))
        for k, (lay_s, lay_f) in enumerate(((S.la, E.la), (S.lb, E.lb), (S.la, E.la), (S.la, E.la))):
            for n, e in enumerate(pick):
                assert np.array_equal(sub[k][int(lay_s[n]):int(lay_s[n + 1])], full[k][int(lay_f[e]):int(lay_f[e + 1])]), (flags, k, e)
    # n_edges == 0 writes nothing
    assert all((x == SENTINEL).all() for x in E.call(n_edges=0))
    for flags in (0, lfp.MATCH_MUTUAL):
        first = E.call(flags=flags)
        same(E.call(flags=flags), first, "two runs")
        out = E.outputs()                                         # the handle's own stream (the binding waits before and after)
        E.handle.match_q8_edges_device(
            E.d_a.data_ptr(), E.d_ioa.data_ptr(), len(E.ioa) - 1, len(E.qa), E.d_b.data_ptr(), E.d_iob.data_ptr(), len(E.iob) - 1,
            len(E.qb), E.d_ea.data_ptr(), E.d_eb.data_ptr(), E.d_la.data_ptr(), E.cap_a, E.n_edges, out[0].data_ptr(), E.d_lb.data_ptr(),
            E.cap_b, out[1].data_ptr(), RATIO, flags, out[2].data_ptr(), out[3].data_ptr(), None)
        same([x.cpu().numpy() for x in out], first, "handle's stream")
        # a captured call -- both layouts, the matcher and the filter -- replays to the same arrays
        out = E.outputs()
        d_la, d_lb = torch.full_like(E.d_la, -1), torch.full_like(E.d_lb, -1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream().cuda_stream
            E.handle.edge_layout_device(E.d_ioa.data_ptr(), len(E.ioa) - 1, len(E.qa), E.d_ea.data_ptr(), E.n_edges, d_la.data_ptr(), s)
            E.handle.edge_layout_device(E.d_iob.data_ptr(), len(E.iob) - 1, len(E.qb), E.d_eb.data_ptr(), E.n_edges, d_lb.data_ptr(), s)
            E.run(out, flags=flags, edges=(E.d_ea, E.d_eb, d_la, d_lb), stream=s)
        for x in out + [d_la, d_lb]:
            x.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same([x.cpu().numpy() for x in out], first, "replay")
        assert torch.equal(d_la, E.d_la) and torch.equal(d_lb, E.d_lb)
        if flags == 0:
            same(first, shared_out, "unfiltered")


# --- (e) --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_pool():
    """image offsets of 40 images with one inverted range, behind 9 rows of no image; the pool is told 6 rows fewer than the
    last offset says"""
    rng = np.random.default_rng(77)
    sizes = rng.integers(0, 50, 40)
    sizes[39] = 20                                             # the image the pool's total cuts
    io = 9 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    io[17] = io[18] + 4                                        # image 17 inverted: empty; image 16 longer
    return io, int(io[-1]) - 6


@pytest.mark.parametrize("n_edges", [1, 2, 1023, 1024, 1025, 70000])
def test_layout(n_edges, odd_pool, handle, torch):
    io, total = odd_pool
    rng = np.random.default_rng(n_edges)
    edge = rng.integers(0, 40, n_edges).astype(np.uint32)
    edge[rng.integers(0, n_edges, max(n_edges // 50, 1))] = rng.choice([40, 41, 1 << 31, cases.NO_IMAGE], max(n_edges // 50, 1))
    edge[-1] = 17 if n_edges == 1 else 39                      # the inverted image alone; the image the total cuts
    rows = np.array([cases.image_bounds(io, total, m)[1] for m in range(40)] + [0], np.int64)
    want = np.concatenate([[0], np.cumsum(rows[np.minimum(edge, 40)])])
    assert rows[17] == 0 and rows[39] == io[40] - io[39] - 6 and (n_edges > 2000 or np.array_equal(want, cases.edge_layout(io, total, edge)))
    d_io, d_e = torch.from_numpy(io).cuda(), words(torch, edge)
    out = torch.full((n_edges + 1 + 2 * EXTRA,), SENTINEL, dtype=torch.int64, device="cuda")
    handle.edge_layout_device(d_io.data_ptr(), 40, total, d_e.data_ptr(), n_edges, out.data_ptr() + 8 * EXTRA,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:EXTRA] == SENTINEL).all() and (got[-EXTRA:] == SENTINEL).all()                # exactly n_edges + 1 entries
    bad = np.flatnonzero(got[EXTRA:-EXTRA] != want)
    assert len(bad) == 0, (n_edges, bad[:5], got[EXTRA:-EXTRA][bad[:5]], want[bad[:5]])
    # n_edges == 0 writes nothing
    out.fill_(SENTINEL)
    handle.edge_layout_device(d_io.data_ptr(), 40, total, d_e.data_ptr(), 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("row_bytes", [4, 20, 128, 512])
def test_gather(row_bytes, odd_pool, handle, torch):
    io, total = odd_pool
    rng = np.random.default_rng(row_bytes)
    edge = np.concatenate([rng.integers(0, 40, 300), [17, 39, 40, cases.NO_IMAGE, 39]]).astype(np.uint32)
    lay = cases.edge_layout(io, total, edge)
    full = int(lay[-1])
    src = rng.integers(0, 256, (int(io[-1]) + 3, row_bytes)).astype(np.uint8)         # rows at and beyond `total` exist but are not read
    d_src, d_io, d_e = torch.from_numpy(src).cuda(), torch.from_numpy(io).cuda(), words(torch, edge)
    d_lay = torch.from_numpy(lay.astype(np.int64)).cuda()
    for cap in (full, full - 7, int(lay[150]) + 3, 0):          # the whole layout; cut inside the last edge; mid-way; nothing
        dst = torch.full((full + EXTRA, row_bytes), 0xA5, dtype=torch.uint8, device="cuda")
        handle.gather_edge_rows_device(d_src.data_ptr(), row_bytes, d_io.data_ptr(), 40, total, d_e.data_ptr(), d_lay.data_ptr(), cap,
                                       len(edge), dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = cases.gather_edge_rows(src, io, total, edge, lay, cap, np.full((full + EXTRA, row_bytes), 0xA5, np.uint8))
        assert np.array_equal(dst.cpu().numpy(), want), (row_bytes, cap)
        assert (want[cap:] == 0xA5).all() and (cap == 0 or (want[:cap] != 0xA5).any())
    # a layout that leaves rows between its edges: they are untouched
    gaps = lay + 2 * np.arange(len(lay), dtype=np.uint64)
    dst = torch.full((int(gaps[-1]) + EXTRA, row_bytes), 0xA5, dtype=torch.uint8, device="cuda")
    handle.gather_edge_rows_device(d_src.data_ptr(), row_bytes, d_io.data_ptr(), 40, total, d_e.data_ptr(),
                                   torch.from_numpy(gaps.astype(np.int64)).cuda().data_ptr(), int(gaps[-1]), len(edge), dst.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = np.full((int(gaps[-1]) + EXTRA, row_bytes), 0xA5, np.uint8)
    for e, m in enumerate(edge):
        first, n = cases.image_bounds(io, total, m)
        want[int(gaps[e]):int(gaps[e]) + n] = src[first:first + n]
    assert np.array_equal(dst.cpu().numpy(), want), row_bytes


def test_local_features_face(shared, shared_out, torch):
    """LocalFeatures.match_q8_edges / edge_layout / gather_edge_rows: host tensors and other integer dtypes for the offsets and
    the ids are accepted; a capacity of None is the layout's last entry; entries of no edge come back as -1 / INT32_MIN"""
    E = shared
    feats = lfp.LocalFeatures(64, 64, 64)
    ids_a, ids_b = torch.from_numpy(E.ea.astype(np.int64)), E.d_eb                 # int64 on the host, int32 bit patterns on the device
    ab, ba, s1, s2, la, lb = feats.match_q8_edges(E.d_a, torch.from_numpy(E.ioa).to(torch.int32), E.d_b, E.d_iob, ids_a, ids_b)
    torch.cuda.synchronize()
    assert torch.equal(la, E.d_la) and torch.equal(lb, E.d_lb) and la.dtype == torch.int64
    assert ab.shape == s1.shape == s2.shape == (E.cap_a,) and ba.shape == (E.cap_b,) and ab.dtype == ba.dtype == s1.dtype == torch.int32
    for got, want in zip((ab, ba, s1, s2), shared_out):
        assert np.array_equal(got.cpu().numpy(), want[:-EXTRA])
    more = feats.match_q8_edges(E.d_a, E.d_ioa, E.d_b, E.d_iob, E.d_ea, E.d_eb, mutual=True, capacity_a=E.cap_a + 50, capacity_b=E.cap_b + 3)
    w_ab, w_ba = pcases.mutual(shared_out[0][:-EXTRA], shared_out[1][:-EXTRA], E.la.astype(np.int64), E.lb.astype(np.int64))
    assert np.array_equal(more[0].cpu().numpy()[:E.cap_a], w_ab) and np.array_equal(more[1].cpu().numpy()[:E.cap_b], w_ba)
    assert (more[0][E.cap_a:] == -1).all() and (more[2][E.cap_a:] == int(cases.INT32_MIN)).all() and more[1].shape == (E.cap_b + 3,)
    kps = torch.arange(len(E.qa) * 5, dtype=torch.float32, device="cuda").reshape(-1, 5)
    got = feats.gather_edge_rows(kps, E.d_ioa, E.d_ea, la)
    want = cases.gather_edge_rows(kps.cpu().numpy(), E.ioa, len(E.qa), E.ea, E.la, E.cap_a, np.zeros((E.cap_a, 5), np.float32))
    assert got.shape == (E.cap_a, 5) and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="one id per edge"):
        feats.match_q8_edges(E.d_a, E.d_ioa, E.d_b, E.d_iob, E.d_ea, E.d_eb[:-1])
    with pytest.raises(RuntimeError, match="uint8"):
        feats.match_q8_edges(E.d_a.float(), E.d_ioa, E.d_b, E.d_iob, E.d_ea, E.d_eb)


# --- (f) --------------------------------------------------------------------------------------------------------------
H_TRUE = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])      # of test_gpu_match_pairs.py::_frames


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


def test_frames_to_verified_matches_over_edges(torch):
    """three images, all three pairs: match_q8_edges, gathered keypoints and verify_homography_batch give the matches, the
    verified matches, H and the stats of the existing route on rows copied into pair layout with torch, same seed"""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    seed = 21
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "all", seed=seed, feats=feats)
    torch.cuda.synchronize()
    ea, eb, o, la, lb = (got[k] for k in ("edge_a", "edge_b", "offsets", "layout_a", "layout_b"))
    assert ea.tolist() == [0, 0, 1] and eb.tolist() == [1, 2, 2]
    # the existing route on the same pool: every edge's rows copied into pair layout with torch, match_q8_batch, verify
    kps, q, dev = got["keypoints"], got["q8"], ea.device
    o_h = o.cpu().tolist()
    assert o_h[-1] == q.shape[0] == kps.shape[0] and min(np.diff(o_h)) >= 2
    rows = lambda side: torch.cat([torch.arange(o_h[i], o_h[i + 1], device=dev) for i in side])
    ia, ib = rows([0, 0, 1]), rows([1, 2, 2])
    oa = torch.tensor(np.concatenate([[0], np.cumsum([o_h[i + 1] - o_h[i] for i in (0, 0, 1)])]))
    ob = torch.tensor(np.concatenate([[0], np.cumsum([o_h[i + 1] - o_h[i] for i in (1, 2, 2)])]))
    assert torch.equal(la.cpu(), oa) and torch.equal(lb.cpu(), ob)
    w_ab, _, w_best, w_second = feats.match_q8_batch(q.index_select(0, ia), oa, q.index_select(0, ib), ob, ratio=0.8, mutual=True)
    w_model, w_ver, w_stats = feats.verify_homography_batch(kps.index_select(0, ia), oa, kps.index_select(0, ib), ob, w_ab, seed=seed)
    torch.cuda.synchronize()
    size = int(oa[-1])
    m_ab, ver = got["match"], got["verified"]
    assert torch.equal(m_ab[:size], w_ab) and torch.equal(ver[:size], w_ver) and (m_ab[size:] == -1).all()
    assert np.array_equal(got["model"].cpu().numpy().view(np.uint32), w_model.cpu().numpy().view(np.uint32))
    assert torch.equal(got["stats"], w_stats)
    per_edge, w_stats = got["per_edge"].cpu().numpy(), w_stats.cpu().numpy()
    w_ab_h, w_ver_h = w_ab.cpu().numpy(), w_ver.cpu().numpy()
    raw = (w_best.cpu().numpy().astype(np.float32) * np.float32(0.8) > w_second.cpu().numpy().astype(np.float32))
    for e in range(3):
        s = slice(int(oa[e]), int(oa[e + 1]))
        assert per_edge[e].tolist() == [raw[s].sum(), (w_ab_h[s] >= 0).sum(), (w_ver_h[s] >= 0).sum()], e
        assert per_edge[e][2] == w_stats[e][0]
        print(f"[q8_edges] edge {ea[e].item()} -> {eb[e].item()}: {per_edge[e][0]} matches, {per_edge[e][1]} mutual, {per_edge[e][2]} verified")


# --- (g) --------------------------------------------------------------------------------------------------------------
def test_match_collection_example(tmp_path):
    """examples/match_collection.py --all on three generated frames: one line per edge, ranked, exit status 0"""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_collection.py")
    out = subprocess.run([sys.executable, exe, "--all"] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    print("\n".join(lines))
    assert lines[0].startswith("Extracted ") and len(lines) == 4
    assert lines[1].startswith("Edge 1 -> 2: ")                 # the crop and its warp rank first
    verified = []
    for line in lines[1:]:
        w = line.replace(",", "").split()
        assert w[0] == "Edge" and w[5] == "matches" and w[7] == "mutual"
        raw, mutual, inl = int(w[4]), int(w[6]), int(w[8])
        assert raw >= mutual >= inl >= 0, line
        verified.append(inl)
    assert verified == sorted(verified, reverse=True) and verified[0] >= 8
