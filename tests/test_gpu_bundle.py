"""lf_mkd_bundle_adjust_device on the GPU, every output compared as words against the host twin (tests/cpp/bundle_twin.cpp: the
kernels' own csrc/mkd_bundle_math.h compiled by g++; tests/test_bundle_twin.py ties the twin to the algorithm of
include/lf_mkd.h): the smallest shapes at every seam of the two canonical sums and of the global sums, outputs in place and
apart, capacities above the counts and counts above the capacities, mixed cameras and null optional arrays, held items and the
stops of CG, garbage inputs between guard words, graph capture, the host form, and the example."""
import numpy as np
import pytest

import bundle_cases as cases
import bundle_twin as bt

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
OUTPUTS = ("poses", "points", "obs_state", "trace", "counts")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bundle_twin")
    exe = bt.build(tmp)
    return lambda scene, **kw: bt.run(exe, tmp, scene, **kw)


class Device:
    """a scene on the device: the arrays hold exactly what their lengths say; every output between sentinels (the trace, f64,
    as pairs of words behind an even number of sentinels, so that it stays 8-byte aligned)"""

    def __init__(self, torch, handle, s):
        self.torch, self.handle = torch, handle
        a = bt.arrays(s)
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()
        self.kps, self.ioff, self.toff = up(a["kps"]), up(a["image_offsets"].view(np.int64)), up(a["track_offsets"].view(np.int64))
        self.row, self.img, self.tc = up(a["obs_row"]), up(a["obs_image"].view(np.int32)), up(a["counts"].view(np.int32))
        self.pts, self.K, self.poses = up(a["points"]), up(a["intrinsics"]), up(a["poses"])
        self.state = up(None if a["obs_state"] is None else a["obs_state"].view(np.int32))
        self.fixed = up(None if a["camera_fixed"] is None else a["camera_fixed"].view(np.int32))
        self.n_rows, self.n_images, self.tcap, self.ocap = len(a["kps"]), len(a["intrinsics"]), len(a["points"]), len(a["obs_row"])

    def words(self, iterations):
        return {"poses": 12 * self.n_images, "points": 4 * self.tcap, "obs_state": self.ocap, "trace": 16 * iterations, "counts": 4}

    def buffers(self, iterations):
        return {k: self.torch.full((n + 2 * EXTRA + 2,), bt.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.words(iterations).items()}

    @staticmethod
    def front(k):
        return EXTRA + 1 if k == "trace" else EXTRA     # (torch's allocations are 256-byte aligned: 38 words in is 8-byte aligned)

    def run(self, bufs, stream=None, state_out=True, in_place=False, use_state=True, use_fixed=True, **kw):
        p = {**bt.DEFAULTS, **kw}
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * self.front(k)
        self.handle.bundle_adjust_device(
            ptr(self.kps), self.ioff.data_ptr(), self.n_images, self.n_rows, self.toff.data_ptr(), self.tcap, ptr(self.row),
            ptr(self.img), self.ocap, self.tc.data_ptr(), ptr(self.pts), ptr(self.K), ptr(self.poses),
            ptr(self.poses) if in_place else out("poses"), ptr(self.pts) if in_place else out("points"), out("trace"), out("counts"),
            d_obs_state=ptr(self.state) if use_state else None, d_camera_fixed=ptr(self.fixed) if use_fixed else None,
            d_obs_state_out=out("obs_state") if state_out else None, max_reproj_px=p["px"], lambda0=p["lambda0"],
            iterations=p["iterations"], cg_iterations=p["cg_iterations"], cg_tol=p["cg_tol"],
            stream=self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs, iterations):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.words(iterations).items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            f = self.front(k)
            assert (raw[:f] == bt.FILL).all() and (raw[f + n:] == bt.FILL).all(), "a write outside d_" + k
            res[k] = raw[f:f + n]
        res["poses"], res["points"] = res["poses"].reshape(-1, 12), res["points"].reshape(-1, 4)
        res["trace"] = np.ascontiguousarray(res["trace"]).view(np.uint64).reshape(-1, 8)
        return res

    def call(self, **kw):
        iterations = {**bt.DEFAULTS, **kw}["iterations"]
        bufs = self.buffers(iterations)
        self.torch.cuda.synchronize()
        self.run(bufs, **kw)
        self.torch.cuda.synchronize()
        return self.read(bufs, iterations)


def want_of(tw):
    return {"poses": tw["poses"], "points": tw["points"], "obs_state": tw["obs_state"], "trace": tw["trace_words"], "counts": tw["counts"]}


def same(got, want, what, keys=OUTPUTS):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), [hex(got[k][tuple(b)]) for b in bad[:5]],
                               [hex(want[k][tuple(b)]) for b in bad[:5]])


def check(torch, handle, twin, scene, what, **kw):
    want = want_of(twin(scene, **kw))
    got = Device(torch, handle, scene).call(**kw)
    same(got, want, what)
    return got


def trace_of(got):
    return got["trace"].view(np.float64)


def test_tracks_of_every_length_around_the_four_slots(torch, handle, twin):
    s = cases.track_lengths()
    lengths = np.diff(s["track_offsets"][:61].astype(np.int64))
    assert sorted(set(lengths.tolist())) == [2, 3, 4, 5, 8, 9]
    got = check(torch, handle, twin, s, "track lengths")
    tr = trace_of(got)
    assert tr[:, 3].sum() >= 3 and tr[-1, 1] < 0.5 * tr[0, 0] and got["counts"].tolist()[:3] == [7, 60, int(lengths.sum())]


def test_images_of_255_256_257_and_513_active_rows(torch, handle, twin):
    s = cases.image_rows()
    got = check(torch, handle, twin, s, "image rows")
    act, _, _, _ = cases.active_set(s)
    assert np.bincount(act[:, 2], minlength=6)[2:].tolist() == [255, 256, 257, 513] and got["counts"][2] == len(act)
    assert trace_of(got)[:, 3].sum() >= 3


@pytest.mark.parametrize("n", (1, 2, 256, 257))
def test_the_global_sum_over_the_image_ids(torch, handle, twin, n):
    got = check(torch, handle, twin, cases.many_images(n), "%d images" % n)
    assert got["counts"][0] == max(n - 2, 1)


@pytest.mark.parametrize("T", (255, 256, 257))
def test_the_cost_sum_over_the_track_indices(torch, handle, twin, T):
    got = check(torch, handle, twin, cases.many_tracks(T), "%d tracks" % T)
    assert got["counts"][1] == T and (np.diff(trace_of(got)[:, 0]) <= 0).all()


def test_in_place_equals_apart(torch, handle, twin):
    s = cases.mixed()
    want = check(torch, handle, twin, s, "apart")
    D = Device(torch, handle, s)
    bufs = D.buffers(4)
    D.run(bufs, in_place=True)
    torch.cuda.synchronize()
    res = D.read(bufs, 4)
    assert (res["poses"] == bt.FILL).all() and (res["points"] == bt.FILL).all()
    res["poses"], res["points"] = D.poses.cpu().numpy().view(np.uint32), D.pts.cpu().numpy().view(np.uint32)
    same(res, want, "in place")


def test_capacities_above_the_counts_and_counts_above_the_capacities(torch, handle, twin):
    base = cases.build(21, cases.random_views(21, 70, 6, 2, 5), outliers=0.03)
    roomy = cases.build(21, cases.random_views(21, 70, 6, 2, 5), outliers=0.03, capacity=(300, 1111))
    a, b = check(torch, handle, twin, base, "tight"), check(torch, handle, twin, roomy, "roomy")
    T, O = int(base["counts"][0]), int(base["counts"][1])
    for k in ("poses", "trace", "counts"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["points"], b["points"][:T]) and (b["points"][T:] == bt.FILL).all()
    assert np.array_equal(a["obs_state"], b["obs_state"][:O]) and (b["obs_state"][O:] == bt.FILL).all()
    over = dict(base, counts=np.array([T + 1000, 0xFFFFFFFF], np.uint32))
    c = check(torch, handle, twin, over, "counts above the capacities")
    for k in OUTPUTS:
        assert np.array_equal(a[k], c[k]), k


def test_mixed_cameras_a_null_mask_and_a_null_state(torch, handle, twin):
    s = cases.mixed()
    got = check(torch, handle, twin, s, "mixed")
    P = np.asarray(s["poses"], np.float32).view(np.uint32)
    assert got["counts"][0] == 4 and np.array_equal(got["poses"][[0, 1, 2, 5]], P[[0, 1, 2, 5]]) and (got["poses"][[3, 4, 6, 7]] != P[[3, 4, 6, 7]]).any()
    free = dict(s, camera_fixed=None)
    got2 = check(torch, handle, twin, free, "a null mask")
    assert got2["counts"][0] == 6
    same(Device(torch, handle, s).call(use_fixed=False), got2, "the mask left out of the call")
    # the triangulation call's states: only its inliers are active
    state = np.full(len(s["obs_row"]), 2, np.uint32)
    state[::5], state[1::7] = 1, 0
    got3 = check(torch, handle, twin, dict(s, obs_state=state), "with d_obs_state")
    assert got3["counts"][2] < got["counts"][2] and (got3["obs_state"][::5] == 0).all()
    same(Device(torch, handle, dict(s, obs_state=state)).call(use_state=False), got, "the states left out of the call")
    none = Device(torch, handle, s).call(state_out=False)
    assert (none["obs_state"] == bt.FILL).all()
    same(none, got, "without d_obs_state_out", keys=("poses", "points", "trace", "counts"))


def quiet(seed, views, **kw):
    """a scene near its optimum: every observation an inlier from the first iteration on"""
    return cases.build(seed, views, noise=0.3, perturb=(0.0005, 0.002, 0.002), **kw)


def test_a_point_held_with_one_inlier_and_the_stops_of_cg(torch, handle, twin):
    v = cases.random_views(23, 80, 6, 3, 5)
    v[10] = False
    v[10, [0, 2]] = True                                                     # a track of two views, one of them 30 px off
    s = quiet(23, v)
    s["kps"][s["obs_row"][int(s["track_offsets"][10]) + 1], 0] += 30.0
    got = check(torch, handle, twin, s, "a held point")
    tr = trace_of(got)
    assert tr[:, 7].tolist() == [1, 1, 1, 1] and tr[0, 5] == got["counts"][2] - 1, tr
    assert got["obs_state"][int(s["track_offsets"][10]):int(s["track_offsets"][11])].tolist() == [2, 1]
    stops = trace_of(check(torch, handle, twin, s, "cg stops at step 1", cg_tol=0.999))
    assert (stops[:, 4] == 1).all(), stops
    runs = trace_of(check(torch, handle, twin, s, "cg runs out", cg_tol=0.0, cg_iterations=3))
    assert (runs[:, 4] == 3).all(), runs


def test_a_camera_held_by_a_failed_pivot(torch, handle, twin):
    """camera 4 sees ONE point: its U has rank 2, and under a lambda far below an ulp of its diagonal a pivot of the Cholesky
    factorisation is not positive -- the camera is HELD in the first iteration, and moves in the second (lambda = 2^-40)"""
    v = cases.random_views(25, 50, 5, 3, 4)
    v[:, 4] = False
    v[0, 4] = True
    s = quiet(25, v)
    got = check(torch, handle, twin, s, "failed pivot", lambda0=1.2e-38, iterations=2)
    assert trace_of(got)[:, 6].tolist() == [1, 0] and got["counts"][0] == 3


def test_garbage_inputs_end_equal_the_twin_and_stay_inside(torch, handle, twin):
    s = cases.garbage()
    got = check(torch, handle, twin, s, "garbage")
    assert got["counts"][2] < s["counts"][1] and trace_of(got)[:, 3].sum() >= 1
    bad = dict(s, poses=s["poses"].copy(), points=s["points"].copy())
    bad["poses"][2, 4], bad["points"][9, 1] = np.nan, -np.inf
    check(torch, handle, twin, bad, "garbage with a NaN pose and an infinite point")


def test_nothing_free_copies_through(torch, handle, twin):
    s = cases.mixed()
    s["camera_fixed"][:] = 1
    s["obs_state"] = np.zeros(len(s["obs_row"]), np.uint32)
    got = check(torch, handle, twin, s, "nothing free")
    assert got["counts"].tolist() == [0, 0, 0, 4]
    assert np.array_equal(got["poses"], s["poses"].view(np.uint32)) and np.array_equal(got["points"], s["points"].view(np.uint32))
    empty = dict(s, counts=np.array([0, 0], np.uint32), obs_state=None)
    got = check(torch, handle, twin, empty, "T == 0")
    assert np.array_equal(got["poses"], s["poses"].view(np.uint32)) and (got["points"] == bt.FILL).all()


def test_a_captured_call_replays_to_the_same_words_twice(torch, handle, twin):
    s = cases.track_lengths()
    D = Device(torch, handle, s)
    a = D.call()                                                             # warmed up: the scratch has its size
    same(a, want_of(twin(s)), "first run")
    bufs = D.buffers(4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        for v in bufs.values():
            v.fill_(bt.FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(D.read(bufs, 4), a, "replay")


def test_the_host_form_and_the_wrapper_equal_the_device_form(torch, handle, twin):
    s = cases.track_lengths()
    a = bt.arrays(s)
    want = Device(torch, handle, s).call()
    poses, points, state, trace, counts = handle.bundle_adjust(
        a["kps"], a["image_offsets"], a["track_offsets"], a["obs_row"], a["obs_image"], a["points"], a["intrinsics"], a["poses"],
        camera_fixed=a["camera_fixed"], iterations=4, cg_iterations=8)
    assert np.array_equal(poses.view(np.uint32), want["poses"]) and np.array_equal(points.view(np.uint32), want["points"])
    assert np.array_equal(state, want["obs_state"]) and np.array_equal(trace.view(np.uint64), want["trace"])
    assert np.array_equal(counts, want["counts"])
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    table = (up(a["track_offsets"].view(np.int64)), up(a["obs_row"]), up(a["obs_image"].view(np.int32)), None, up(a["counts"].view(np.int32)))
    out = lf.bundle_adjust(up(a["kps"]), up(a["image_offsets"].view(np.int64)), table, up(a["points"]), up(a["intrinsics"]),
                           up(a["poses"]), camera_fixed=up(a["camera_fixed"].view(np.int32)), iterations=4, cg_iterations=8)
    torch.cuda.synchronize()
    for got, name in zip(out, OUTPUTS):
        words = got.cpu().numpy().view(np.uint64 if name == "trace" else np.uint32)
        assert np.array_equal(words.reshape(want[name].shape), want[name]), name
    # n_images == 0: LF_MKD_OK, nothing written (null pointers everywhere)
    handle.bundle_adjust_device(None, None, 0, 0, None, 0, None, None, 0, None, None, None, None, None, None, None, None)


def test_match_collection_with_bundle(torch):
    """match_collection(..., pose=.., register=1, bundle=3) on the example's frames runs in place and reports its trace (the
    frames are warps of one picture, so the geometry means little; this is about the plumbing)"""
    import os
    import sys
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()[:3]])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), register=1, bundle=3)
    torch.cuda.synchronize()
    tr, counts = got["bundle_trace"].cpu().numpy(), got["bundle_counts"].cpu().numpy()
    assert tr.shape == (3, 8) and (np.diff(tr[:, 0]) <= 0).all() and counts[3] == tr[:, 3].sum()
    state = got["bundle_obs_state"].cpu().numpy()
    assert set(state.tolist()) <= {-1, 0, 1, 2} and (state >= 1).sum() == counts[2]
    lines = ex.bundle_lines(got)
    assert len(lines) == 5 and lines[1].startswith("iteration 1: cost ") and lines[-1].startswith("rms reprojection error ")
