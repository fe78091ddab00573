"""Candidate edges on the GPU (lf_mkd_select_edges_device; LocalFeatures.select_edges): every output equals the numpy
restatement's (tests/select_edges_cases.py) -- every comparison is ==, and every output sits between sentinel entries that must
survive.  The vote table sits between sentinels too, at every 16-byte phase, so a read outside it would change the picks.  Row
lengths around the wave and the load width, every k form and the value above it, tables that tie, ascend, descend and carry the
sign bit, the flags, shapes either side of every threshold of the plan, long and many rows, every capacity, two runs and the
optional outputs, graph capture, the hand-off to the edge-list calls with the padding in place, a table past the 2 GiB and
4 GiB byte marks, matched pictures and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import select_edges_cases as cases
from conftest import GOLDEN, ROOT

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel entries in front of and behind every array
SENTINEL = 0x5A5A5A5A            # as a vote it beats nearly everything: a read outside the table shows
NAMES = ("rank", "rank_votes", "edge_a", "edge_b", "edge_votes", "counts")
OPTIONAL = ("rank", "rank_votes", "edge_votes")
FORMS = sorted({lfp.select_edges_plan(7, 7, k)[0] for k in range(1, 33)})
KS = sorted({1, 2, 3, 32} | set(FORMS) | {f + 1 for f in FORMS if f < 32})


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
    """a vote table on the device between sentinels, `shift` entries off a 16-byte boundary, and sentinel-filled outputs"""

    def __init__(self, torch, handle, votes, shift=0):
        self.torch, self.handle = torch, handle
        self.n_a, self.n_b = votes.shape
        self.front = 4 * EXTRA + shift                                          # (allocations are 256-byte aligned)
        self.d_votes = torch.full((self.front + votes.size + EXTRA,), SENTINEL, dtype=torch.int32, device="cuda")
        self.load(votes)

    def load(self, votes):
        assert votes.shape == (self.n_a, self.n_b)
        self.d_votes[self.front:self.front + votes.size] = self.torch.from_numpy(bits32(votes).reshape(-1)).cuda()

    def sizes(self, k, cap):
        return [self.n_a * k, self.n_a * k, cap, cap, cap, 4]

    def outputs(self, k, cap):
        return [self.torch.full((n + 2 * EXTRA,), SENTINEL, dtype=self.torch.int32, device="cuda") for n in self.sizes(k, cap)]

    def run(self, out, k, min_votes=1, flags=0, cap=None, skip=(), stream=None):
        cap = self.n_a * k if cap is None else cap
        ptr = lambda i: None if NAMES[i] in skip or (i in (2, 3, 4) and cap == 0) else out[i].data_ptr() + 4 * EXTRA
        self.handle.select_edges_device(self.d_votes.data_ptr() + 4 * self.front, self.n_a, self.n_b, k, min_votes, flags, cap,
                                        ptr(0), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5),
                                        self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def call(self, k, cap=None, **kw):
        cap = self.n_a * k if cap is None else cap
        out = self.outputs(k, cap)
        self.torch.cuda.synchronize()
        self.run(out, k, cap=cap, **kw)
        self.torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]


def framed(want, skip=()):
    """a restatement's Result as the device arrays hold it: sentinels in front, behind, and all over an output that was NULL"""
    pad = np.full(EXTRA, SENTINEL, np.int32)
    out = []
    for name, x in zip(NAMES, want.arrays()):
        body = np.full(x.size, SENTINEL, np.int32) if name in skip else bits32(x).reshape(-1)
        out.append(np.concatenate([pad, body, pad]))
    return out


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def check(D, votes, what, k, min_votes=1, flags=0, cap=None, skip=()):
    want = cases.select_edges(votes, k, min_votes, bool(flags & cases.SKIP_SELF), bool(flags & cases.UNIQUE), cap)
    got = D.call(k, cap=cap, min_votes=min_votes, flags=flags, skip=skip)
    if cap == 0:
        skip = tuple(skip) + ("edge_a", "edge_b", "edge_votes")
    same(got, framed(want, skip), what)
    return want


# --- row lengths, k and tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_b", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099])
def test_shapes(n_b, torch, handle):
    """n_a in {1, 3, 7}: every k form, the value above it, k above n_b and above the candidates, on every kind of table; every
    min_votes of a kind at k = 3; SKIP_SELF on the table whose maximum is the diagonal; the table at every 16-byte phase"""
    assert KS[:3] == [1, 2, 3] and KS[-1] == 32 and len(KS) >= 8
    for n_a in (1, 3, 7):
        D = {shift: Device(torch, handle, np.zeros((n_a, n_b), np.uint32), shift) for shift in range(4)}
        for kind in cases.KINDS:
            votes, mins = cases.table(kind, n_a, n_b)
            for d in D.values():
                d.load(votes)
            for k in KS:
                check(D[(k + n_a) % 4], votes, (kind, n_a, n_b, k), k, mins[0])
            for m in mins[1:] + (0,):
                check(D[m % 4], votes, (kind, n_a, n_b, "min", m), 3, m)
            if kind == "diagonal":
                for k in (1, 2, 32):
                    plain = check(D[1], votes, (kind, n_a, n_b, k), k)
                    skipped = check(D[2], votes, (kind, n_a, n_b, k, "skip self"), k, flags=cases.SKIP_SELF)
                    for i in range(min(n_a, n_b)):
                        assert plain.rank[i, 0] == i and i not in skipped.rank[i]


@pytest.mark.parametrize("n", [1, 2, 3, 65, 257])
def test_flags_on_square_tables(n, torch, handle):
    """one pool: no flag, SKIP_SELF, UNIQUE and both; under UNIQUE every pair at most once with a < b, and the edges with
    d_rank NULL (the rank table then lives in the handle's scratch) equal those with it given"""
    D = Device(torch, handle, np.zeros((n, n), np.uint32), shift=n % 4)
    for kind in cases.KINDS:
        votes, mins = cases.table(kind, n, n, seed=2)
        D.load(votes)
        for k in (1, 2, 4, 32):
            for flags in (0, cases.SKIP_SELF, cases.UNIQUE, cases.SKIP_SELF | cases.UNIQUE):
                want = check(D, votes, (kind, n, k, flags), k, mins[0], flags)
                if flags & cases.UNIQUE:
                    kept = want.counts[0]
                    pairs = list(zip(want.edge_a[:kept].tolist(), want.edge_b[:kept].tolist()))
                    assert len(set(pairs)) == len(pairs) and all(a < b for a, b in pairs)
                    check(D, votes, (kind, n, k, flags, "rank NULL"), k, mins[0], flags, skip=("rank",))
                    check(D, votes, (kind, n, k, flags, "ranks NULL"), k, mins[0], flags, skip=("rank", "rank_votes"))


def test_unique_by_hand(torch, handle):
    """mutual picks, one-sided picks in both orientations and a self pick without SKIP_SELF (select_edges_cases.unique_table)"""
    votes = cases.unique_table()
    D = Device(torch, handle, votes, shift=3)
    want = check(D, votes, "by hand", 2, 1, cases.UNIQUE)
    assert list(zip(want.edge_a[:4].tolist(), want.edge_b[:4].tolist())) == [(0, 1), (1, 3), (0, 2), (3, 4)] and want.counts == [4, 4, 7, 5]
    assert want.rank[4].tolist() == [4, 3]                                     # the self pick is a pick, and no edge
    got = D.call(2, flags=cases.UNIQUE, skip=("rank",))
    assert got[2][EXTRA:EXTRA + 10].tolist() == [0, 1, 0, 3] + [-1] * 6 and got[3][EXTRA:EXTRA + 10].tolist() == [1, 3, 2, 4] + [-1] * 6
    want = check(D, votes, "by hand, skip self", 2, 1, cases.UNIQUE | cases.SKIP_SELF)
    assert want.rank[4].tolist() == [3, -1] and want.counts == [4, 4, 6, 5]
    plain = check(D, votes, "by hand, every pick", 2, 1)
    assert plain.counts == [7, 7, 7, 5]


# --- the plan's forms ------------------------------------------------------------------------------------------------------
def _thresholds(n_a, k, upto):
    """the n_b at which the plan of (n_a, n_b, k) differs from that of n_b - 1 in its form: rows per workgroup, launches or grid"""
    out, last = [], lfp.select_edges_plan(n_a, 1, k)[1:4]
    for n_b in range(2, upto):
        now = lfp.select_edges_plan(n_a, n_b, k)[1:4]
        if now != last:
            out.append((n_b, last, now))
        last = now
    return out


@pytest.mark.parametrize("n_a", [1, 3, 7])
def test_either_side_of_every_threshold_of_the_plan(n_a, torch, handle):
    """the shapes at which rows stop sharing a workgroup, at which a row is first cut into segments, and at which it gets one
    more segment: n_b - 1 and n_b, read from the plan"""
    found = _thresholds(n_a, 4, 13000)
    assert any(a[0] != b[0] for _, a, b in found) and any(a[2] != b[2] for _, a, b in found) and 3 <= len(found) <= 8
    for n_b, _, _ in found:
        for width in (n_b - 1, n_b):
            D = Device(torch, handle, np.zeros((n_a, width), np.uint32), shift=width % 4)
            for kind in ("ties", "ascending", "descending", "huge"):
                votes, mins = cases.table(kind, n_a, width)
                D.load(votes)
                for k in (3, 32):
                    check(D, votes, (kind, n_a, width, k), k, mins[0])


@pytest.mark.parametrize("n_a, n_b, k", [(1, 300001, 32), (2, 70003, 4), (1500, 2500, 8), (1031, 70, 3), (9000, 40, 32)])
def test_long_rows_and_many_rows(n_a, n_b, k, torch, handle):
    """a row of many segments; rows beyond what is cut (a workgroup each); many short rows (more than one workgroup of waves);
    pick slots beyond one pass of the scan over the workgroups' counts"""
    groups, launches = lfp.select_edges_plan(n_a, n_b, k)[2:4]
    assert (launches == 5 and groups > 10 * n_a) if n_a < 3 else (launches == 4 and groups >= n_a // 4)
    assert n_a != 9000 or n_a * k > 256 * 1024                                 # (the scan takes 1024 counts of 256 slots a pass)
    D = Device(torch, handle, np.zeros((n_a, n_b), np.uint32), shift=1)
    for kind, m in (("ties", 3), ("ascending", 1), ("huge", 0xFFFFFFFF)):
        if kind == "ascending" and n_a > 2:
            continue
        votes, _ = cases.table(kind, n_a, n_b)
        D.load(votes)
        want = check(D, votes, (kind, n_a, n_b, k), k, m)
        assert 0 < want.counts[2] <= n_a * k and (n_a != 9000 or kind != "ties" or want.counts[2] < n_a * k // 2)   # rows run out of candidates


def test_many_rows_of_one_pool(torch, handle):
    """UNIQUE over several workgroups of pick slots: positions come from the scan, not from the slot"""
    n, k = 700, 32
    votes, _ = cases.table("ties", n, n, seed=5)
    D = Device(torch, handle, votes, shift=2)
    want = check(D, votes, "unique 700", k, 3, cases.UNIQUE | cases.SKIP_SELF)
    assert n * k // 3 < want.counts[1] < want.counts[2] <= n * k
    check(D, votes, "unique 700, rank NULL, capacity below", k, 3, cases.UNIQUE | cases.SKIP_SELF, cap=want.counts[1] - 5, skip=("rank",))


# --- capacity, runs, optional outputs --------------------------------------------------------------------------------------
def test_every_capacity(torch, handle):
    """every capacity from 0 to n_a k + 2: the first min(S, capacity) edges, the padding, and counts[1] says what was wanted"""
    votes, _ = cases.table("ties", 5, 5, seed=3)
    D = Device(torch, handle, votes)
    for flags in (0, cases.UNIQUE | cases.SKIP_SELF):
        full = check(D, votes, "full", 3, 1, flags)
        wanted = full.counts[1]
        assert 5 <= wanted <= 15
        for cap in range(0, 5 * 3 + 3):
            want = check(D, votes, ("capacity", cap), 3, 1, flags, cap=cap)
            assert want.counts == [min(cap, wanted), wanted] + full.counts[2:]
            assert np.array_equal(want.edge_a[:min(cap, wanted)], full.edge_a[:min(cap, wanted)])


def test_two_runs_and_optional_outputs(torch, handle):
    """two runs agree; each optional output NULL in turn, and all of them, changes nothing else; n_a == 0 writes the padding"""
    votes, _ = cases.table("ties", 7, 300, seed=4)
    D = Device(torch, handle, votes, shift=3)
    first = D.call(5, min_votes=2)
    same(D.call(5, min_votes=2), first, "second run")
    want = check(D, votes, "all outputs", 5, 2)
    same(first, framed(want), "first run")
    for out in OPTIONAL:
        check(D, votes, ("without", out), 5, 2, skip=(out,))
    check(D, votes, "without any", 5, 2, skip=OPTIONAL)
    E = Device(torch, handle, np.zeros((0, 9), np.uint32))
    got = E.call(3, cap=11)
    pad = np.full(EXTRA, SENTINEL, np.int32)
    for i, fill in ((2, -1), (3, -1), (4, 0)):
        assert np.array_equal(got[i], np.concatenate([pad, np.full(11, fill, np.int32), pad]))
    assert np.array_equal(got[5], np.concatenate([pad, np.zeros(4, np.int32), pad])) and (got[0] == SENTINEL).all()


# --- capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a, n_b", [(40, 40), (2, 9001)])
def test_capturable(n_a, n_b, torch, handle):
    """one capture of the warmed-up call (a single chain of launches), replayed after the table has been overwritten"""
    flags = cases.UNIQUE if n_a == n_b else 0
    votes, _ = cases.table("ties", n_a, n_b, seed=6)
    later, _ = cases.table("huge", n_a, n_b, seed=7)
    D = Device(torch, handle, votes, shift=1)
    check(D, votes, "warm-up", 4, 2, flags)
    out = D.outputs(4, n_a * 4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(out, 4, min_votes=2, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    for table in (votes, later, votes):
        for x in out:
            x.fill_(SENTINEL)
        D.load(table)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same([x.cpu().numpy() for x in out], framed(cases.select_edges(table, 4, 2, unique=bool(flags))), "replay")


# --- the hand-off to the edge-list calls -----------------------------------------------------------------------------------
def test_hand_off_with_the_padding(torch):
    """edge_layout / match_q8_edges / build_tracks on a small synthetic pool with n_edges = edge_capacity, padding included:
    the layouts' leading entries, the matches and the labels of the same calls on the kept edges trimmed on the host, and an
    empty range for every padded edge"""
    rng = np.random.default_rng(11)
    rows = [5, 0, 17, 64, 3, 33, 20]
    n, total = len(rows), sum(rows)
    io = torch.from_numpy(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)).cuda()
    base = rng.integers(0, 256, (64, 128))
    q = np.concatenate([np.clip(base[rng.permutation(64)[:r]] + rng.integers(-2, 3, (r, 128)), 0, 255) for r in rows]).astype(np.uint8)
    d_q = torch.from_numpy(q).cuda()
    votes, _ = cases.table("ties", n, n, seed=8)
    feats = lfp.LocalFeatures(64, 64, 64)
    k, cap = 2, n * 2
    ea, eb, ev, rank, rank_votes, counts = feats.select_edges(torch.from_numpy(bits32(votes)).cuda(), k, min_votes=2, skip_self=True,
                                                              unique=True)
    torch.cuda.synchronize()
    want = cases.select_edges(votes, k, 2, True, True)
    for g, w in zip((rank, rank_votes, ea, eb, ev, counts), want.arrays()):
        assert np.array_equal(g.cpu().numpy().reshape(-1), bits32(w).reshape(-1))
    kept = want.counts[0]
    assert 3 <= kept < cap and ea.numel() == cap and (ea[kept:] == -1).all() and (eb[kept:] == -1).all()
    bound = cap * max(rows)
    full = feats.match_q8_edges(d_q, io, d_q, io, ea, eb, ratio=0.8, mutual=True, capacity_a=bound, capacity_b=bound)
    trim = feats.match_q8_edges(d_q, io, d_q, io, ea[:kept].clone(), eb[:kept].clone(), ratio=0.8, mutual=True, capacity_a=bound,
                                capacity_b=bound)
    torch.cuda.synchronize()
    for side in (4, 5):                                                        # the two layouts
        lf, lt = full[side].cpu().numpy(), trim[side].cpu().numpy()
        assert np.array_equal(lf[:kept + 1], lt) and (lf[kept:] == lt[kept]).all() and len(lf) == cap + 1
    for i in range(4):                                                         # match_ab, match_ba, best, second
        assert torch.equal(full[i], trim[i]), i
    assert int((full[0] >= 0).sum()) > 20                                      # the pool's images do share rows
    tf = feats.build_tracks(io, ea, eb, full[4], full[0], capacity=bound, n_rows=total)
    tt = feats.build_tracks(io, ea[:kept].clone(), eb[:kept].clone(), trim[4], trim[0], capacity=bound, n_rows=total)
    torch.cuda.synchronize()
    for a, b in zip(tf, tt):
        assert torch.equal(a, b)
    assert int((tf[1] >= 2).sum()) > 5


# --- past the byte marks ---------------------------------------------------------------------------------------------------
def test_a_table_past_2_and_4_gib(torch, handle):
    """n_a = 3, n_b = 2^29 + 5: rows 1 and 2 begin past 2 GiB and 4 GiB.  All zeros but a handful of plants per row, the last
    column included; k = 4, min_votes = 1; the expectation is computed from the plants"""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 2 ** 30:
        pytest.skip("less than 8 GiB of device memory free")
    n_a, n_b, k = 3, 2 ** 29 + 5, 4
    assert n_b * 4 > 2 ** 31 and 2 * n_b * 4 > 2 ** 32 and lfp.select_edges_plan(n_a, n_b, k)[3] == 5
    plants = [{0: 7, 12345: 9, 2 ** 28 + 3: 9, n_b - 1: 8, n_b - 2: 1, 77: 8},                # ties: 12345 before 2^28 + 3, 77 before n_b - 1
              {n_b - 1: 0xFFFFFFFF, 1: 2 ** 31, 2 ** 29: 5},                                  # fewer plants than k
              {2: 3, n_b - 1: 3, 2 ** 29 + 1: 3, 5: 3, 2 ** 27: 3, 2 ** 29 - 1: 4}]           # the lowest columns of one tie
    d_votes = torch.zeros((n_a * n_b,), dtype=torch.int32, device="cuda")
    for i, row in enumerate(plants):
        cols = torch.tensor([i * n_b + c for c in row], dtype=torch.int64, device="cuda")
        d_votes[cols] = torch.from_numpy(bits32(list(row.values()))).cuda()
    rank = np.full((n_a, k), -1, np.int32)
    rank_votes = np.zeros((n_a, k), np.uint32)
    edges = []
    for i, row in enumerate(plants):
        for c, (v, j) in enumerate(sorted((-v, j) for j, v in row.items())[:k]):
            rank[i, c], rank_votes[i, c] = j, -v
            edges.append((i, j, -v))
    assert rank[0].tolist() == [12345, 2 ** 28 + 3, 77, n_b - 1] and rank[1].tolist() == [n_b - 1, 1, 2 ** 29, -1]
    assert rank[2].tolist() == [2 ** 29 - 1, 2, 5, 2 ** 27]
    want = cases.finish(n_a, k, rank, rank_votes, edges, None)
    assert want.counts == [11, 11, 11, 3]
    out = [torch.full((s + 2 * EXTRA,), SENTINEL, dtype=torch.int32, device="cuda") for s in (n_a * k,) * 5 + (4,)]
    ptr = lambda i: out[i].data_ptr() + 4 * EXTRA
    torch.cuda.synchronize()
    handle.select_edges_device(d_votes.data_ptr(), n_a, n_b, k, 1, 0, n_a * k, ptr(0), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in out], framed(want), "past the byte marks")


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


@pytest.mark.parametrize("k", [1, 2])
def test_pictures(k, torch):
    """match_collection(..., "select", K) on houses, its crop-and-warp and bird.jpg: the edge list equals the restatement
    applied to the vote table read back, no pair appears twice, and the calls behind it see the padding as empty edges"""
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "select", k, seed=21, feats=feats, tracks=True)
    torch.cuda.synchronize()
    host = {key: v.cpu().numpy() for key, v in got.items() if v is not None}
    votes = host["votes"].view(np.uint32)
    print("votes:", votes.tolist())
    assert votes.shape == (3, 3) and (np.diag(votes) == 0).all() and votes[0, 1] > 100 and votes[1, 0] > 100
    want = cases.select_edges(votes, k, 1, True, True)
    for name, w in zip(("rank", "rank_votes", "edge_a", "edge_b", "edge_votes", "select_counts"), want.arrays()):
        assert np.array_equal(bits32(host[name]).reshape(-1), bits32(w).reshape(-1)), name
    kept = want.counts[0]
    pairs = list(zip(want.edge_a[:kept].tolist(), want.edge_b[:kept].tolist()))
    assert pairs[0] == (0, 1) and len(set(pairs)) == len(pairs) == kept < 3 * k and all(a < b for a, b in pairs)
    la, per_edge = host["layout_a"], host["per_edge"]
    assert len(la) == 3 * k + 1 and (la[kept:] == la[kept]).all() and (per_edge[kept:] == 0).all() and per_edge[0, 2] > 100


def test_match_collection_example_with_select(tmp_path):
    """examples/match_collection.py --select 1 on three generated frames: houses and its warp pick each other, which is ONE
    edge, and no line is printed for the padding"""
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    exe = os.path.join(ROOT, "local-features_amd", "examples", "match_collection.py")
    out = subprocess.run([sys.executable, exe, "--select", "1"] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    print("\n".join(lines))
    assert lines[0].startswith("Extracted ") and 2 <= len(lines) <= 3
    edges = [re.match(r"Edge (\d+) -> (\d+): \d+ matches, \d+ mutual, (\d+) agree", x) for x in lines[1:]]
    assert all(edges) and (edges[0].group(1), edges[0].group(2)) == ("1", "2") and int(edges[0].group(3)) > 100
    assert all(int(m.group(1)) < int(m.group(2)) for m in edges) and len({m.group(1, 2) for m in edges}) == len(edges)
