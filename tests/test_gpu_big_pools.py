"""Every pooled entry point past the 2 GiB and 4 GiB byte marks (tests/big_pool_cases.py): pools of 4.3 GB made on the device,
a few hundred planted rows copied in from the host, and the suite's numpy restatements on the planted rows as the expected
values.  Every comparison is ==, except where lf_mkd_match_device and lf_mkd_match_pairs_device are held to the oracle's f32
matcher under the suite's existing compare (its tolerances, its near-tie rule).  Each check also runs at B = 2^16, where tests/test_big_pool_cases.py has proved the
sparse expectation equal to the full restatement: a failure at a real mark beside a pass at the small one is an addressing
fault of the kernel, the launcher or the binding, not of this harness.

Only planted rows and the entries the expectations name cross to the host; everything else -- background rows, sentinels,
untouched labels -- is checked on the device.  A test frees its tensors, closes its handle and empties the cache."""
import time

import numpy as np
import pytest

import big_pool_cases as big
import fundamental_cases as fcases
import fundamental_twin as ft
import homography_cases as hcases
import homography_f32 as h32
import match_guided_cases as mgcases
import match_pairs_cases as pcases
import match_twin as mt
import q8_edges_cases as ecases
from conftest import _report
from test_gpu_match import compare
from test_gpu_match_guided import expected as guided_expected

import local_features_python as lfp

pytestmark = pytest.mark.gpu

SEED = 7100                     # tests/test_big_pool_cases.py asserts the background conditions at these seeds
SENTINEL = big.SENTINEL
CHUNK = 1 << 21                 # rows (or 64 entries each) of one device-side step


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture
def handle(torch, request):
    """a handle of the test's own, closed behind it (the scratch goes with it); reports the test's wall time and peak memory"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    h = lfp.MkdHandle(max_features=64)
    yield h
    torch.cuda.synchronize()
    h.close()
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    _report(f"[big pools] {request.node.name}: {time.perf_counter() - t0:.2f} s, peak {peak / 2 ** 30:.2f} GiB of tensors")


def need(torch, gib):
    free = torch.cuda.mem_get_info()[0]
    if free < gib * 2 ** 30:
        pytest.skip(f"needs {gib} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")


def words(torch, x):
    """uint32 values as an int32 device tensor of their bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint32)).view(np.int32)).cuda()


def u64(torch, x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.uint64)).view(np.int64)).cuda()


def to_device(torch, pool, seed=1):
    """a SparsePool on the device: the background row or seeded noise made there, the planted blocks copied in through slices
    (a slice is a 64-bit pointer offset: no index arithmetic of the framework's stands between the host rows and their place)"""
    t = torch.empty((pool.total, pool.width), dtype=getattr(torch, pool.dtype.name), device="cuda")
    if pool.fill_row is not None:
        t[:] = torch.from_numpy(pool.fill_row).cuda()
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        for r in range(0, pool.total, CHUNK):
            n = min(CHUNK, pool.total - r)
            if pool.dtype == np.uint8:
                t[r:r + n] = torch.randint(1, 256, (n, pool.width), dtype=torch.uint8, device="cuda", generator=g)
            else:
                t[r:r + n] = 0.09 * torch.randn((n, pool.width), device="cuda", generator=g)
    for first, rows in pool.blocks:
        t[first:first + len(rows)].copy_(torch.from_numpy(rows))
    return t


def rows_of(t, index):
    """single rows of a device tensor on the host, each read through a slice"""
    return np.stack([t[int(i)].cpu().numpy() for i in index])


def filled(torch, n, value=SENTINEL, dtype=None):
    return torch.full((n,), value, dtype=dtype or torch.int32, device="cuda")


def holds(torch, t, value, ranges):
    """every entry of the 1-d device tensor t outside the sorted, disjoint `ranges` [(first, n)] equals `value`"""
    pos = 0
    for first, n in list(ranges) + [(t.numel(), 0)]:
        assert first >= pos, "ranges overlap"
        for lo in range(pos, first, CHUNK * 64):
            hi = min(lo + CHUNK * 64, first)
            if not bool((t[lo:hi] == value).all()):
                bad = lo + int(torch.nonzero(t[lo:hi] != value)[0])
                return bad
        pos = first + n
    return None


def check_segments(torch, t, segments, what, fill=SENTINEL):
    """the entries [(first, values)] of the device tensor equal their expected values, every other entry holds `fill`"""
    segments = sorted(segments, key=lambda s: s[0])
    for first, want in segments:
        got = t[first:first + len(want)].cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (what, "entries from", first, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    bad = holds(torch, t, fill, [(first, len(v)) for first, v in segments])
    assert bad is None, (what, "an entry outside every pair was written", bad, int(t[bad]))


# --- 1 and 2: the single-pair calls, every b row a candidate ------------------------------------------------------------
def _call(handle, torch, form, d_a, na, d_b, nb, out, k=None, d_groups=None, lo=None, hi=None):
    p = [o.data_ptr() for o in out]
    x = (lo.data_ptr(), hi.data_ptr()) if lo is not None else (None, None)
    if form == "match":
        handle.match_q8_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, p[0], float(big.RATIO), x[0], x[1], p[1], p[2])
    elif form == "knn":
        handle.knn_q8_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, k, p[0], p[1], x[0], x[1])
    else:
        handle.match_q8_grouped_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, d_groups.data_ptr(), p[0], float(big.RATIO), x[0], x[1],
                                       p[1], p[2])
    torch.cuda.synchronize()


FORMS = [("match", None), ("knn", 1), ("knn", 5), ("grouped", None)]
FORM_IDS = ["match", "knn1", "knn5", "grouped"]


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("form,k", FORMS + [("ranges", None)], ids=FORM_IDS + ["match-ranges"])
def test_single_pair_big_b(torch, handle, B, form, k):
    """96 queries against a pool of 33 558 565 rows (at B = 2^32): the matcher, the matcher with exclusion ranges that start
    and end at critical rows, top-1, top-5 and the grouped form whose ids change at critical rows"""
    need(torch, 6)
    S = big.SingleQ8(B, SEED)
    na, nb, width = big.NA_BIG_B, S.total, k or 1
    d_b, d_a = to_device(torch, S.pool), torch.from_numpy(S.small[:na]).cuda()
    lo = hi = d_groups = None
    if form == "ranges":
        form, (rlo, rhi, _, _) = "match", S.ranges()
        lo, hi, want = words(torch, rlo), words(torch, rhi), S.expect_match_big_b(ranges=True)
    elif form == "match":
        want = S.expect_match_big_b()
    elif form == "knn":
        want = S.expect_knn_big_b(k)
    else:
        want = S.expect_grouped_big_b()
        at = torch.zeros(nb, dtype=torch.int32, device="cuda")
        at[torch.from_numpy(S.crit).cuda()] = 1
        d_groups = torch.div(torch.cumsum(at, 0, dtype=torch.int32), big.GROUP_RUN, rounding_mode="floor").to(torch.int32)
        at = None
        got = rows_of(d_groups, S.crit)
        assert np.array_equal(got.astype(np.uint32), S.groups_of_planted())
    guard = 8
    out = [filled(torch, na * width + 2 * guard) for _ in want]
    _call(handle, torch, form, d_a, na, d_b, nb, [o[guard:] for o in out], k, d_groups, lo, hi)
    for name, o, w in zip(("match / index", "best / score", "second / rival"), out, want):
        g = o.cpu().numpy()
        assert (g[:guard] == SENTINEL).all() and (g[guard + na * width:] == SENTINEL).all(), (form, name, "guard words")
        g = g[guard:guard + na * width].reshape(w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (form, k, B, name, len(bad), bad[:5].tolist(), g[g != w][:5], w[g != w][:5])
    assert (want[0] >= B // 128).any() and ((want[0] >= 0) & (want[0] < B // 256)).any()


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("form,k", FORMS, ids=FORM_IDS)
def test_single_pair_big_a(torch, handle, B, form, k):
    """a pool of 33 558 565 query rows against 64 candidates: every background row's outputs equal one scalar tuple (checked
    on the device), the planted rows' are read back"""
    need(torch, 8)
    S = big.SingleQ8(B, SEED)
    na, nb, width = S.total, big.NB_BIG_A, k or 1
    d_a, d_b = to_device(torch, S.pool), torch.from_numpy(S.small[:nb]).cuda()
    d_groups = words(torch, S.groups_small()) if form == "grouped" else None
    planted, background = S.expect_big_a(form, k)
    guard = 8
    out = [filled(torch, na * width + 2 * guard) for _ in planted]
    _call(handle, torch, form, d_a, na, d_b, nb, [o[guard:] for o in out], k, d_groups)
    crit = torch.from_numpy(S.crit).cuda()
    for name, o, w, bg in zip(("match / index", "best / score", "second / rival"), out, planted, background):
        assert bool((o[:guard] == SENTINEL).all()) and bool((o[guard + na * width:] == SENTINEL).all()), (form, name, "guard words")
        body = o[guard:guard + na * width].view(na, width)
        got = rows_of(body, S.crit).reshape(w.shape)
        bad = np.argwhere(got != w)
        assert len(bad) == 0, (form, k, B, name, len(bad), S.crit[bad[:5, 0]], got[got != w][:5], w[got != w][:5])
        ok = (body == torch.from_numpy(np.atleast_1d(bg)).cuda()).all(dim=1)
        ok[crit] = True
        assert bool(ok.all()), (form, k, B, name, "a background row differs", int(torch.nonzero(~ok)[0]))
        body = ok = None


# --- 3: pairs and edges ---------------------------------------------------------------------------------------------------
NAMES = ("ab", "ba", "best", "second")


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("far", ["a", "b", "both"])
def test_q8_pairs(torch, handle, B, far):
    """lf_mkd_match_q8_pairs_device with and without LF_MKD_MATCH_MUTUAL: per mark a pair ending exactly at it, one starting
    exactly at it and one straddling it, one ending at the total and a control near row 0; the far images in pool a, pool b
    or both.  One call per group of adjacent pairs (offsets[0] far from 0), so every entry outside them holds its sentinel."""
    need(torch, 11)
    P = big.Pooled(B, far, SEED + 1)
    d_a, d_b = to_device(torch, P.pools["a"], 1), to_device(torch, P.pools["b"], 2)
    na, nb = P.pools["a"].total, P.pools["b"].total
    out = dict(zip(NAMES, (filled(torch, na), filled(torch, nb), filled(torch, na), filled(torch, na))))
    matched = 0
    for mutual in (False, True):
        for (oa, ob), want in zip(P.calls, P.expect(mutual=mutual)):
            d_oa, d_ob = u64(torch, oa), u64(torch, ob)
            handle.match_q8_pairs_device(d_a.data_ptr(), d_oa.data_ptr(), na, d_b.data_ptr(), d_ob.data_ptr(), nb, len(oa) - 1,
                                         out["ab"].data_ptr(), out["ba"].data_ptr(), float(big.RATIO), lfp.MATCH_MUTUAL if mutual else 0,
                                         out["best"].data_ptr(), out["second"].data_ptr())
            torch.cuda.synchronize()
            for name in NAMES:
                check_segments(torch, out[name], want[name], (far, B, mutual, name, oa.tolist()))
                for first, v in want[name]:
                    out[name][first:first + len(v)] = SENTINEL
            matched += sum(int((v >= 0).sum()) for _, v in want["ab"])
    assert matched > 100


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("long_range", [False, True], ids=["layout", "long-range"])
def test_q8_edges(torch, handle, B, long_range):
    """lf_mkd_match_q8_edges_device over one shared pool, with and without LF_MKD_MATCH_MUTUAL.  long-range: a layout not made
    from the ids whose first range is [0, B / 4 + 5) over a 500-row image -- the later edges' match + lo and best + lo lie
    beyond byte B of the outputs, and the entries of the long range beyond the image keep their sentinel."""
    need(torch, 14)
    E = big.EdgesQ8(B, SEED + 2, long_range)
    d_q = to_device(torch, E.pool)
    d_ioa, d_iob = torch.from_numpy(E.io_a).cuda(), torch.from_numpy(E.io_b).cuda()
    d_ea, d_eb, d_la, d_lb = words(torch, E.ea), words(torch, E.eb), u64(torch, E.la), u64(torch, E.lb)
    if not long_range:                                   # the device's layout is the restatement's
        d_lay = torch.full((len(E.ea) + 1,), -1, dtype=torch.int64, device="cuda")
        handle.edge_layout_device(d_ioa.data_ptr(), len(E.io_a) - 1, E.total, d_ea.data_ptr(), len(E.ea), d_lay.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_lay.cpu().numpy().astype(np.uint64), E.la)
    extra = 8
    # (the long range's outputs are 4.3 GB each: match_ab and best only, second stays NULL)
    names = ("ab", "ba", "best") if long_range else NAMES
    out = {n: filled(torch, (E.cap_b if n == "ba" else E.cap_a) + extra) for n in names}
    for mutual in (False, True):
        want = E.expect(mutual=mutual)
        handle.match_q8_edges_device(d_q.data_ptr(), d_ioa.data_ptr(), len(E.io_a) - 1, E.total, d_q.data_ptr(), d_iob.data_ptr(),
                                     len(E.io_b) - 1, E.total, d_ea.data_ptr(), d_eb.data_ptr(), d_la.data_ptr(), E.cap_a, len(E.ea),
                                     out["ab"].data_ptr(), d_lb.data_ptr(), E.cap_b, out["ba"].data_ptr(), float(big.RATIO),
                                     lfp.MATCH_MUTUAL if mutual else 0, out["best"].data_ptr(),
                                     out["second"].data_ptr() if "second" in out else None)
        torch.cuda.synchronize()
        for name in names:
            check_segments(torch, out[name], want[name], (long_range, B, mutual, name))
            for first, v in want[name]:
                out[name][first:first + len(v)] = SENTINEL
        assert sum(int((v >= 0).sum()) for _, v in want["ab"]) > 50
    if long_range:
        assert int(E.la[1]) * 4 > B and E.la[1] - E.la[0] > E.control


# --- 4: the gather and the layout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("row_bytes", [512, 128])
def test_gather_and_layout(torch, handle, B, row_bytes):
    """lf_mkd_edge_layout_device against the numpy cumulative sum and lf_mkd_gather_edge_rows_device from a far pool: the first
    edge names a ballast image of about B / row_bytes rows (compared on the device), so the far images' destination rows lie
    around and beyond byte B of dst as their source rows do of src"""
    need(torch, 10)
    G = big.Gather(B, row_bytes, SEED + 3)
    d_src = to_device(torch, G.pool)
    extra = 8
    cap = max(int(G.layout(k)[-1]) for k in range(len(G.lists)))
    d_dst = torch.zeros((cap + extra, row_bytes), dtype=torch.uint8, device="cuda")      # (byte 0 occurs nowhere in the pool)
    for k, (io, edge) in enumerate(G.lists):
        lay = G.layout(k)
        d_io, d_edge = torch.from_numpy(io).cuda(), words(torch, edge)
        d_lay = torch.full((len(edge) + 1,), -1, dtype=torch.int64, device="cuda")
        handle.edge_layout_device(d_io.data_ptr(), len(io) - 1, G.total, d_edge.data_ptr(), len(edge), d_lay.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_lay.cpu().numpy().astype(np.uint64), lay), (row_bytes, B, k)
        assert np.array_equal(lay, np.concatenate([[0], np.cumsum([ecases.image_bounds(io, G.total, m)[1] for m in edge])]).astype(np.uint64))
        d_dst.zero_()
        handle.gather_edge_rows_device(d_src.data_ptr(), row_bytes, d_io.data_ptr(), len(io) - 1, G.total, d_edge.data_ptr(),
                                       d_lay.data_ptr(), int(lay[-1]), len(edge), d_dst.data_ptr())
        torch.cuda.synchronize()
        (s0, d0, n), segs = G.expect(k)
        for first, rows in segs:
            got = d_dst[first:first + len(rows)].cpu().numpy()
            assert np.array_equal(got, rows), (row_bytes, B, k, first, np.argwhere(got != rows)[:5])
        for r in range(0, n, CHUNK):
            m = min(CHUNK, n - r)
            assert torch.equal(d_dst[d0 + r:d0 + r + m], d_src[s0 + r:s0 + r + m]), (row_bytes, B, k, "ballast rows from", r)
        assert bool((d_dst[int(lay[-1]):] == 0).all()), (row_bytes, B, k, "a row behind the layout was written")


# --- 7: the quantiser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
def test_quantize(torch, handle, B):
    """lf_mkd_quantize_descriptors_device over 8 392 741 f32 rows (at B = 2^32): the critical rows == q8_cases.quantize, every
    background row's 128 bytes == the background row's"""
    need(torch, 7)
    Q = big.Quantize(B, SEED + 4)
    d_x = to_device(torch, Q.pool)
    d_q = torch.zeros((Q.total + 1, 128), dtype=torch.uint8, device="cuda")
    handle.quantize_descriptors_device(d_x.data_ptr(), Q.total, d_q.data_ptr())
    torch.cuda.synchronize()
    rows, bg = Q.expect()
    got = rows_of(d_q, Q.crit)
    assert np.array_equal(got, rows), (B, Q.crit[np.argwhere(got != rows)[:5, 0]])
    ok = (d_q[:Q.total] == torch.from_numpy(bg).cuda()).all(dim=1)
    ok[torch.from_numpy(Q.crit).cuda()] = True
    assert bool(ok.all()), (B, "a background row differs", int(torch.nonzero(~ok)[0]))
    assert bool((d_q[Q.total] == 0).all()), "the row behind d_q[n] was written"


# --- 9: tracks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("accumulate", [False, True], ids=["one-call", "accumulated"])
def test_tracks(torch, handle, B, accumulate):
    """lf_mkd_build_tracks_device on a pool of B / 4 + 3 images + 37 rows: int32 labels and statistics of 4.3 GB each (at
    B = 2^32), the match array addressed through a layout whose entries pass byte B as well.  The touched images' labels,
    lengths and conflicts == tracks_cases.build_tracks on the compressed pool; every other row is its own track of length 1."""
    need(torch, 18)
    T = big.Tracks(B, SEED + 5)
    N = T.total
    d_io = torch.from_numpy(T.image_offsets()).cuda()
    d_ea, d_eb, d_la = words(torch, T.ea), words(torch, T.eb), u64(torch, T.la)
    d_match = filled(torch, T.cap, -1)
    for e, seg in enumerate(T.segments):
        d_match[int(T.la[e]):int(T.la[e]) + len(seg)].copy_(torch.from_numpy(seg))
    d_track, d_len, d_dup = filled(torch, N), filled(torch, N), filled(torch, N)
    n_edges = len(T.ea)

    def build(first, n, flags):
        handle.build_tracks_device(d_io.data_ptr(), T.n_images, N, d_ea.data_ptr() + 4 * first, d_eb.data_ptr() + 4 * first,
                                   d_la.data_ptr() + 8 * first, T.cap, n, d_match.data_ptr(), d_track.data_ptr(), d_len.data_ptr(),
                                   d_dup.data_ptr(), flags)
        torch.cuda.synchronize()

    if accumulate:
        half = n_edges // 2
        build(0, half, 0)
        build(half, n_edges - half, lfp.TRACKS_ACCUMULATE)
    else:
        build(0, n_edges, 0)
    track, length, dup = T.expect()
    track = T.to_pool_rows(track).astype(np.int32)
    for k, (first, n) in enumerate(T.touched_ranges()):
        c = slice(k * T.rows, (k + 1) * T.rows)
        for name, d, w in (("track", d_track, track[c]), ("len", d_len, length[c].view(np.int32)), ("dup", d_dup, dup[c].view(np.int32))):
            got = d[first:first + n].cpu().numpy()
            bad = np.flatnonzero(got != w)
            assert len(bad) == 0, (B, accumulate, name, "image", int(T.touched[k]), len(bad), bad[:5], got[bad[:5]], w[bad[:5]])
    # every untouched row: track == r, len == 1, dup == 0
    pos = 0
    for first, n in T.touched_ranges() + [(N, 0)]:
        for lo in range(pos, first, CHUNK * 16):
            hi = min(lo + CHUNK * 16, first)
            r = torch.arange(lo, hi, dtype=torch.int32, device="cuda")
            assert torch.equal(d_track[lo:hi], r), (B, accumulate, "an untouched row's label, rows from", lo)
            assert bool((d_len[lo:hi] == 1).all()) and bool((d_dup[lo:hi] == 0).all()), (B, accumulate, "statistics, rows from", lo)
        pos = first + n
    assert track[T.rows * (len(T.touched) - 1) + len(T.touched) - 1] == 0 and (dup > 0).any()


# --- 3, guided: lf_mkd_match_q8_guided_pairs_device ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guided_twin(tmp_path_factory):
    """(program, scratch directory) of the guided matchers' host twin: one g++ build for the module"""
    d = tmp_path_factory.mktemp("guided_twin")
    return mgcases.build(d), d


def _plant_keypoints(torch, P, c, d_ka, d_kb, value=None):
    """the keypoints of call c into the NaN pools (value None), or NaN back over them"""
    for side, d in (("a", d_ka), ("b", d_kb)):
        first, rows = P.kps[c][side]
        d[first:first + len(rows)] = torch.from_numpy(rows).cuda() if value is None else value


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("kind", [0, 1], ids=["H", "F"])
@pytest.mark.parametrize("far", ["a", "b", "both"])
def test_q8_guided_pairs(torch, handle, guided_twin, B, far, kind):
    """lf_mkd_match_q8_guided_pairs_device under homographies and fundamental matrices, with and without LF_MKD_MATCH_MUTUAL,
    over test_q8_pairs' layout; keypoint pools of the descriptor pools' length.  == q8_guided_cases.decide under the host
    twin's masks."""
    need(torch, 12)
    P = big.Pooled(B, far, SEED + 6, guide=kind)
    thr = mgcases.THRESHOLDS[kind][1]
    masks = mgcases.twin_masks(*guided_twin, P.problems(thr))
    d_a, d_b = to_device(torch, P.pools["a"], 1), to_device(torch, P.pools["b"], 2)
    na, nb = P.pools["a"].total, P.pools["b"].total
    d_ka, d_kb = (torch.full((n, 5), float("nan"), device="cuda") for n in (na, nb))
    out = dict(zip(NAMES, (filled(torch, na), filled(torch, nb), filled(torch, na), filled(torch, na))))
    tally = [0, 0]
    for mutual in (False, True):
        for c, ((oa, ob), want) in enumerate(zip(P.calls, P.expect_guided(masks, mutual=mutual))):
            _plant_keypoints(torch, P, c, d_ka, d_kb)
            d_oa, d_ob, d_model = u64(torch, oa), u64(torch, ob), torch.from_numpy(P.models[c]).cuda()
            handle.match_q8_guided_pairs_device(d_a.data_ptr(), d_ka.data_ptr(), d_oa.data_ptr(), na, d_b.data_ptr(), d_kb.data_ptr(),
                                                d_ob.data_ptr(), nb, d_model.data_ptr(), len(oa) - 1, out["ab"].data_ptr(),
                                                out["ba"].data_ptr(), kind, thr, float(big.RATIO), lfp.MATCH_MUTUAL if mutual else 0,
                                                out["best"].data_ptr(), out["second"].data_ptr())
            torch.cuda.synchronize()
            for name in NAMES:
                check_segments(torch, out[name], want[name], (far, B, kind, mutual, name, oa.tolist()))
                for first, v in want[name]:
                    out[name][first:first + len(v)] = SENTINEL
            _plant_keypoints(torch, P, c, d_ka, d_kb, float("nan"))
            tally[0] += sum(int((v >= 0).sum()) for _, v in want["ab"])
            tally[1] += sum(int((v < 0).sum()) for _, v in want["ab"])
    assert tally[0] > 30 and tally[1] > 30, tally


# --- 5: lf_mkd_match_device, its scan and its screen form -----------------------------------------------------------------------
@pytest.fixture(params=["scan", "screen"])
def f32_form(request, monkeypatch):
    monkeypatch.setenv("LF_MKD_MATCH", request.param)
    monkeypatch.delenv("LF_MKD_MATCH_SPLITS", raising=False)
    monkeypatch.delenv("LF_MKD_MATCH_SHARE", raising=False)
    return request.param


@pytest.fixture(scope="module")
def match_twin(tmp_path_factory):
    """scan(a, b, ratio): the screen form's host twin, an exhaustive scan with match_verify's own f32 dot product"""
    tmp = tmp_path_factory.mktemp("match_twin")
    exe = mt.build(tmp)
    return lambda a, b, ratio: mt.scan(exe, tmp, a, b, ratio)


def _f32_outputs(torch, n):
    return filled(torch, n), torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
def test_f32_match_big_b(torch, oracle, match_twin, f32_form, handle, B):
    """96 queries (the screen form: 16384 rows that repeat them) against a pool of 8 392 741 f32 rows (at B = 2^32): held to
    oracle.match on the planted rows plus one background row under test_gpu_match.py's compare, its tolerances and its near-tie
    rule; the screen form also to its twin, bit for bit.  Nothing may be redone.

    (With a pool of ONE repeated background row that last demand needs care: big_pool_cases.SingleF32 plants every critical
    row's neighbour as well, and says why.  Without the neighbours 1195 of the 16384 rows were redone at B = 2^31 on the
    MI355X -- correctly, by the fallback scan, which is exactly what this test must not let stand in for the screen form.)"""
    need(torch, 6)
    S = big.SingleF32(B, SEED + 7)
    a, bc = S.a_rows(f32_form == "screen"), S.compressed()
    want, s1, s2 = oracle.match(a, bc)
    S.background_below(a, s2)
    want = S.to_rows(want)
    d_b, d_a = to_device(torch, S.pool), torch.from_numpy(a).cuda()
    m, g1, g2 = _f32_outputs(torch, len(a))
    stream = torch.cuda.current_stream().cuda_stream
    handle.match_device(d_a.data_ptr(), len(a), d_b.data_ptr(), S.total, m.data_ptr(), 0.8, None, None, g1.data_ptr(), g2.data_ptr(), stream)
    torch.cuda.synchronize()
    m, g1, g2 = m.cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy()
    redone = handle.match_overflowed(stream)
    d_a = d_b = None                                         # (a failing assertion keeps this frame: the pool must not stay with it)
    compare(m, g1, g2, want, s1, s2, np.float32(0.8), (f32_form, B))
    assert (want >= B // 512).any() and ((want >= 0) & (want < B // 1024)).any()
    if f32_form == "screen":                                 # bit for bit on every row the fallback scan did not redo
        tw = match_twin(a, bc, 0.8)
        diff = np.flatnonzero((m != S.to_rows(tw.match)) | (_bits(g1) != _bits(tw.best)) | (_bits(g2) != _bits(tw.second)))
        assert len(diff) <= redone, (B, "rows that differ from the twin", len(diff), diff[:5], "rows redone", redone)
    assert redone == 0, (f32_form, B, "rows redone by the fallback scan", redone)


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
def test_f32_match_big_a(torch, oracle, match_twin, f32_form, handle, B):
    """a pool of 8 392 741 f32 query rows against 384 candidates: the planted rows and one background row are held to
    oracle.match (and the screen form's to its twin); every other background row's three outputs have the bits of that one's"""
    need(torch, 6)
    S = big.SingleF32(B, SEED + 7)
    rows, b = S.big_a_rows(), S.small_b
    want, s1, s2 = oracle.match(rows, b)
    d_a, d_b = to_device(torch, S.pool), torch.from_numpy(b).cuda()
    m, g1, g2 = _f32_outputs(torch, S.total)
    stream = torch.cuda.current_stream().cuda_stream
    handle.match_device(d_a.data_ptr(), S.total, d_b.data_ptr(), len(b), m.data_ptr(), 0.8, None, None, g1.data_ptr(), g2.data_ptr(), stream)
    torch.cuda.synchronize()
    bg = next(r for r in range(S.total) if r not in set(S.crit.tolist()))
    at = np.append(S.crit, bg)
    got = [rows_of(x, at) for x in (m, g1, g2)]
    compare(got[0], got[1], got[2], want, s1, s2, np.float32(0.8), (f32_form, B))
    assert handle.match_overflowed(stream) == 0
    if f32_form == "screen":
        tw = match_twin(rows, b, 0.8)
        assert np.array_equal(got[0], tw.match) and np.array_equal(_bits(got[1]), _bits(tw.best)) \
            and np.array_equal(_bits(got[2]), _bits(tw.second)), B
    crit = torch.from_numpy(S.crit).cuda()
    for name, x in (("match", m), ("best", g1), ("second", g2)):
        ok = x.view(torch.int32) == x.view(torch.int32)[bg]
        ok[crit] = True
        assert bool(ok.all()), (f32_form, B, name, "a background row differs", int(torch.nonzero(~ok)[0]))


# --- 6: lf_mkd_match_pairs_device and lf_mkd_match_guided_pairs_device over f32 pools -----------------------------------------
def _read(t, first, n):
    return t[first:first + n].cpu().numpy()


def _nan_outside(torch, t, ranges, what):
    """every entry of the f32 tensor outside the sorted ranges is still the NaN it was filled with"""
    pos = 0
    for first, n in sorted(ranges) + [(t.numel(), 0)]:
        assert bool(torch.isnan(t[pos:first]).all()), (what, "a score outside every pair was written")
        pos = first + n


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("guide", [None, 0, 1], ids=["unguided", "H", "F"])
@pytest.mark.parametrize("far", ["a", "b", "both"])
def test_f32_pairs(torch, oracle, handle, guided_twin, B, far, guide):
    """lf_mkd_match_pairs_device against oracle.match under match_pairs_cases.compare, and lf_mkd_match_guided_pairs_device (H
    and F) against test_gpu_match_guided.py's expected() -- the existing matcher over each row's admissible candidates -- bit
    for bit; far pairs in f32 pools of 8 392 741 rows.  LF_MKD_MATCH_MUTUAL: == the filter of the call's own unfiltered
    outputs."""
    need(torch, 11)
    P = big.Pooled(B, far, SEED + 8, f32=True, guide=guide)
    d_a, d_b = to_device(torch, P.pools["a"], 1), to_device(torch, P.pools["b"], 2)
    na, nb = P.pools["a"].total, P.pools["b"].total
    ab, ba = filled(torch, na), filled(torch, nb)
    best, second = (torch.full((na,), float("nan"), device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    if guide is not None:
        thr = mgcases.THRESHOLDS[guide][1]
        masks = mgcases.twin_masks(*guided_twin, P.problems(thr))
        d_ka, d_kb = (torch.full((n, 5), float("nan"), device="cuda") for n in (na, nb))
    pairs = list(P.pairs())
    accepted = 0
    for c, (oa, ob) in enumerate(P.calls):
        d_oa, d_ob = u64(torch, oa), u64(torch, ob)
        mine = [(k, q) for k, q in enumerate(pairs) if q[0] == c]
        ra, rb = [(q[2], len(q[3])) for _, q in mine], [(q[4], len(q[5])) for _, q in mine]
        if guide is not None:
            _plant_keypoints(torch, P, c, d_ka, d_kb)
            d_model = torch.from_numpy(P.models[c]).cuda()
        unfiltered = {}
        for mutual in (False, True):
            flags = lfp.MATCH_MUTUAL if mutual else 0
            if guide is None:
                handle.match_pairs_device(d_a.data_ptr(), d_oa.data_ptr(), na, d_b.data_ptr(), d_ob.data_ptr(), nb, len(oa) - 1,
                                          ab.data_ptr(), ba.data_ptr(), 0.8, flags, best.data_ptr(), second.data_ptr(), stream)
            else:
                handle.match_guided_pairs_device(d_a.data_ptr(), d_ka.data_ptr(), d_oa.data_ptr(), na, d_b.data_ptr(), d_kb.data_ptr(),
                                                 d_ob.data_ptr(), nb, d_model.data_ptr(), len(oa) - 1, ab.data_ptr(), ba.data_ptr(), guide,
                                                 thr, 0.8, flags, best.data_ptr(), second.data_ptr(), stream)
            torch.cuda.synchronize()
            for k, (_, p, a0, x, b0, y) in mine:
                what = (far, B, guide, mutual, c, p)
                g_ab, g_ba, g1, g2 = _read(ab, a0, len(x)), _read(ba, b0, len(y)), _read(best, a0, len(x)), _read(second, a0, len(x))
                if mutual:
                    u = unfiltered[k]
                    w_ab, w_ba = pcases.mutual(u[0], u[1], [0, len(x)], [0, len(y)])
                    assert np.array_equal(g_ab, w_ab) and np.array_equal(g_ba, w_ba), what
                    assert np.array_equal(_bits(g1), _bits(u[2])) and np.array_equal(_bits(g2), _bits(u[3])), what
                    continue
                unfiltered[k] = (g_ab, g_ba, g1, g2)
                accepted += int((g_ab >= 0).sum())
                if guide is None:
                    want, w1, w2 = oracle.match(x, y)
                    pcases.compare(g_ab, g1, g2, want, w1, w2, pcases.RATIO, what + ("a -> b",))
                    want, w1, w2 = oracle.match(y, x)
                    pcases.compare(g_ba, None, None, want, w1, w2, pcases.RATIO, what + ("b -> a",))
                else:
                    fwd, rev, _ = masks[k]
                    want, w1, w2, _ = guided_expected(handle, torch, x, y, fwd, 0.8)
                    assert np.array_equal(g_ab, want) and np.array_equal(_bits(g1), _bits(w1)) and np.array_equal(_bits(g2), _bits(w2)), what
                    assert np.array_equal(g_ba, guided_expected(handle, torch, y, x, rev, 0.8)[0]), what
            bad = holds(torch, ab, SENTINEL, ra), holds(torch, ba, SENTINEL, rb)
            assert bad == (None, None), ((far, B, guide, mutual, c), "an entry outside every pair was written", bad)
            _nan_outside(torch, best, ra, (far, B, guide, mutual, c))
            _nan_outside(torch, second, ra, (far, B, guide, mutual, c))
        for first, n in ra:
            ab[first:first + n] = SENTINEL
            best[first:first + n] = float("nan")
            second[first:first + n] = float("nan")
        for first, n in rb:
            ba[first:first + n] = SENTINEL
        if guide is not None:
            _plant_keypoints(torch, P, c, d_ka, d_kb, float("nan"))
    assert accepted > (20 if guide is None else 5), accepted


# --- 8: the verifiers over one pool of 20-byte keypoint rows ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def fundamental_twin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fundamental_twin")
    return ft.build(tmp), tmp


@pytest.mark.parametrize("B", big.MARKS, ids=lambda b: f"B{b.bit_length() - 1}")
@pytest.mark.parametrize("kind", [0, 1], ids=["homography", "fundamental"])
def test_verifiers(torch, handle, fundamental_twin, B, kind):
    """lf_mkd_verify_homography_device and lf_mkd_verify_fundamental_device on one pool of 214 752 498 keypoint rows (at
    B = 2^32; a mark falls inside a 20-byte row) that is both d_kps_a and d_kps_b, a match array and a `verified` array of
    that length: the model, the statistics and `verified` of every pair equal the suite's twin word for word, as
    test_gpu_homography_exact.py and test_gpu_fundamental_exact.py compare them"""
    need(torch, 8)
    V = big.Verify(B, kind, SEED + 9)
    d_k = torch.full((V.total, 5), float("nan"), device="cuda")
    d_match, d_ver = filled(torch, V.total, -1), filled(torch, V.total)
    thr, seed, n_hyp = (hcases.THR, 21, big.VERIFY_HYPOTHESES) if kind == 0 else (fcases.THR, 29, big.VERIFY_HYPOTHESES)
    call = handle.verify_homography_device if kind == 0 else handle.verify_fundamental_device
    inliers = 0
    for c in V.calls:
        oa, ob, n = c["oa"], c["ob"], len(c["oa"]) - 1
        d_k[int(oa[0]):int(oa[-1])] = torch.from_numpy(c["ka"]).cuda()
        d_k[int(ob[0]):int(ob[-1])] = torch.from_numpy(c["kb"]).cuda()
        d_match[int(oa[0]):int(oa[-1])] = torch.from_numpy(c["match"]).cuda()
        d_oa, d_ob = torch.from_numpy(oa).cuda(), torch.from_numpy(ob).cuda()
        d_model = torch.full((n, 9), float("nan"), device="cuda")
        d_st = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        call(d_k.data_ptr(), d_oa.data_ptr(), d_k.data_ptr(), d_ob.data_ptr(), d_match.data_ptr(), n, d_model.data_ptr(),
             d_ver.data_ptr(), d_st.data_ptr(), n_hyp, thr, seed, 0)
        torch.cuda.synchronize()
        model, st = d_model.cpu().numpy(), d_st.cpu().numpy().view(np.uint32)
        for p, (ka, kb, match) in enumerate(c["pairs"]):
            if kind == 0:
                want = h32.verify(ka, kb, match, n_hyp=n_hyp, thr=thr, seed=seed + p)
                want_model = want["H"]
            else:
                want = ft.verify(*fundamental_twin, ka, kb, match, n_hyp, thr, seed + p)
                want_model = want["F"]
            what = (B, kind, oa.tolist(), p)
            assert np.array_equal(_bits(model[p]), _bits(want_model.reshape(-1))), (what, model[p], want_model.reshape(-1))
            assert np.array_equal(st[p], want["stats"]), (what, st[p], want["stats"])
            ver = _read(d_ver, int(oa[p]), len(match))
            assert np.array_equal(ver, want["verified"]), (what, int((ver != want["verified"]).sum()))
            inliers += int((ver >= 0).sum())
        bad = holds(torch, d_ver, SENTINEL, [(int(oa[0]), int(oa[-1] - oa[0]))])
        assert bad is None, ((B, kind, oa.tolist()), "an entry of `verified` outside every pair was written", bad)
        d_ver[int(oa[0]):int(oa[-1])] = SENTINEL
        d_match[int(oa[0]):int(oa[-1])] = -1
        d_k[int(oa[0]):int(oa[-1])] = float("nan")
        d_k[int(ob[0]):int(ob[-1])] = float("nan")
    assert inliers > 50, inliers
