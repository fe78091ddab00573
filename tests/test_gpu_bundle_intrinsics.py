"""lf_mkd_bundle_adjust_intrinsics_device on the GPU, every output compared as words against the host twin
(tests/cpp/bundle_intr_twin.cpp: the kernels' own csrc/mkd_bundle_math.h compiled by g++; tests/test_bundle_intr_twin.py ties
the twin to the algorithm of include/lf_mkd.h): the smallest shapes at every seam of the two canonical sums, of the group sum
over the image ids and of the global sums, every refine mask, the group map's cases, held groups and a rejected focal scale,
nothing refined against lf_mkd_bundle_adjust_device itself, outputs in place and apart, capacities and garbage between guard
words, graph capture, the host form, both wrappers, and the example."""
import numpy as np
import pytest

import bundle_cases as cases
import bundle_intr_cases as ic
import bundle_intr_twin as bit

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
OUTPUTS = bit.OUTPUTS


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
    tmp = tmp_path_factory.mktemp("bundle_intr_twin")
    exe = bit.build(tmp)
    return lambda scene, **kw: bit.run(exe, tmp, scene, **kw)


class Device:
    """a scene on the device: the arrays hold exactly what their lengths say; every output between sentinels (the trace, f64,
    as pairs of words behind an even number of sentinels, so that it stays 8-byte aligned)"""

    def __init__(self, torch, handle, s):
        self.torch, self.handle = torch, handle
        a = bit.arrays(s)
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()
        self.kps, self.ioff, self.toff = up(a["kps"]), up(a["image_offsets"].view(np.int64)), up(a["track_offsets"].view(np.int64))
        self.row, self.img, self.tc = up(a["obs_row"]), up(a["obs_image"].view(np.int32)), up(a["counts"].view(np.int32))
        self.pts, self.K, self.poses = up(a["points"]), up(a["intrinsics"]), up(a["poses"])
        self.state = up(None if a["obs_state"] is None else a["obs_state"].view(np.int32))
        self.fixed = up(None if a["camera_fixed"] is None else a["camera_fixed"].view(np.int32))
        self.group = up(None if a["camera_group"] is None else a["camera_group"].view(np.int32))
        self.n_groups = a["n_groups"]
        self.n_rows, self.n_images, self.tcap, self.ocap = len(a["kps"]), len(a["intrinsics"]), len(a["points"]), len(a["obs_row"])

    def words(self, iterations):
        return {"poses": 12 * self.n_images, "points": 4 * self.tcap, "intrinsics": 4 * self.n_images, "groups": 3 * self.n_groups,
                "obs_state": self.ocap, "trace": 18 * iterations, "counts": 5}

    def buffers(self, iterations):
        return {k: self.torch.full((n + 2 * EXTRA + 2,), bit.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.words(iterations).items()}

    @staticmethod
    def front(k):
        return EXTRA + 1 if k == "trace" else EXTRA     # (torch's allocations are 256-byte aligned: 38 words in is 8-byte aligned)

    def run(self, bufs, stream=None, state_out=True, group_out=True, in_place=False, **kw):
        p = {**bit.DEFAULTS, **kw}
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * self.front(k)
        self.handle.bundle_adjust_intrinsics_device(
            ptr(self.kps), self.ioff.data_ptr(), self.n_images, self.n_rows, self.toff.data_ptr(), self.tcap, ptr(self.row),
            ptr(self.img), self.ocap, self.tc.data_ptr(), ptr(self.pts), ptr(self.K), ptr(self.poses),
            ptr(self.poses) if in_place else out("poses"), ptr(self.pts) if in_place else out("points"),
            ptr(self.K) if in_place else out("intrinsics"), out("trace"), out("counts"), d_obs_state=ptr(self.state),
            d_camera_fixed=ptr(self.fixed), d_camera_group=ptr(self.group), n_groups=self.n_groups, refine=p["refine"],
            d_group_out=out("groups") if group_out else None, d_obs_state_out=out("obs_state") if state_out else None,
            max_reproj_px=p["px"], lambda0=p["lambda0"], iterations=p["iterations"], cg_iterations=p["cg_iterations"],
            cg_tol=p["cg_tol"], stream=self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs, iterations):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.words(iterations).items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            f = self.front(k)
            assert (raw[:f] == bit.FILL).all() and (raw[f + n:] == bit.FILL).all(), "a write outside d_" + k
            res[k] = raw[f:f + n]
        res["poses"], res["points"] = res["poses"].reshape(-1, 12), res["points"].reshape(-1, 4)
        res["intrinsics"], res["groups"] = res["intrinsics"].reshape(-1, 4), res["groups"].reshape(-1, 3)
        res["trace"] = np.ascontiguousarray(res["trace"]).view(np.uint64).reshape(-1, 9)
        return res

    def call(self, **kw):
        iterations = {**bit.DEFAULTS, **kw}["iterations"]
        bufs = self.buffers(iterations)
        self.torch.cuda.synchronize()
        self.run(bufs, **kw)
        self.torch.cuda.synchronize()
        return self.read(bufs, iterations)


def want_of(tw):
    return {k: tw["trace_words"] if k == "trace" else tw[k] for k in OUTPUTS}


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


def groups_of(got):
    return got["groups"].view(np.float32)


@pytest.mark.parametrize("refine", (1, 2, 3))
def test_tracks_of_every_length_around_the_four_slots(torch, handle, twin, refine):
    s = ic.with_groups(cases.track_lengths(), np.arange(9) % 2, 2, scale=1.02, shift=(3, -2))
    got = check(torch, handle, twin, s, "track lengths, refine %d" % refine, refine=refine, px=6.0)
    g = groups_of(got)
    assert got["counts"][4] == 2 and trace_of(got)[:, 3].sum() >= 3
    assert ((g[:, 0] != 1.0) == bool(refine & 1)).all() and ((g[:, 1:] != 0.0) == bool(refine & 2)).all()


def test_images_of_255_256_257_and_513_active_rows_in_two_groups(torch, handle, twin):
    s = ic.with_groups(cases.image_rows(), np.arange(6) % 2, 2, scale=0.98)
    got = check(torch, handle, twin, s, "image rows", refine=3, px=6.0)
    act, _, _, _ = cases.active_set(s)
    assert np.bincount(act[:, 2], minlength=6)[2:].tolist() == [255, 256, 257, 513] and got["counts"][4] == 2
    assert trace_of(got)[:, 3].sum() >= 3 and not trace_of(got)[:, 8].any()


@pytest.mark.parametrize("n", (2, 256, 257))
def test_the_group_sum_over_the_image_ids_one_group(torch, handle, twin, n):
    got = check(torch, handle, twin, ic.with_groups(cases.many_images(n), None, 1, scale=1.01), "%d images, one group" % n, refine=1)
    assert got["counts"][4] == 1 and groups_of(got)[0, 0] != 1.0


@pytest.mark.parametrize("n", (2, 256, 257))
def test_the_group_sum_over_the_image_ids_a_group_per_image(torch, handle, twin, n):
    s = ic.with_groups(cases.many_images(n), np.arange(n), n, scale=1.01)
    got = check(torch, handle, twin, s, "%d images, %d groups" % (n, n), refine=3)
    assert got["counts"][4] == n


@pytest.mark.parametrize("T", (255, 257))
def test_the_cost_sum_over_the_track_indices(torch, handle, twin, T):
    got = check(torch, handle, twin, ic.with_groups(cases.many_tracks(T), None, 1, scale=0.98), "%d tracks" % T, refine=1)
    assert got["counts"][1] == T and (np.diff(trace_of(got)[:, 0]) <= 0).all()


@pytest.mark.parametrize("make", (cases.track_lengths, cases.mixed), ids=("track_lengths", "mixed"))
def test_nothing_refined_equals_the_fixed_intrinsics_call_on_the_device(torch, handle, twin, make):
    s = make()
    n = len(s["intrinsics"])
    got = check(torch, handle, twin, dict(s, camera_group=np.arange(n, dtype=np.uint32) % 2, n_groups=2), "nothing refined", refine=0)
    D = Device(torch, handle, s)
    poses, points, state = torch.empty_like(D.poses), torch.empty_like(D.pts), torch.full((D.ocap,), -1, dtype=torch.int32, device="cuda")
    trace, counts = torch.zeros((4, 8), dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    handle.bundle_adjust_device(D.kps.data_ptr(), D.ioff.data_ptr(), D.n_images, D.n_rows, D.toff.data_ptr(), D.tcap, D.row.data_ptr(),
                                D.img.data_ptr(), D.ocap, D.tc.data_ptr(), D.pts.data_ptr(), D.K.data_ptr(), D.poses.data_ptr(),
                                poses.data_ptr(), points.data_ptr(), trace.data_ptr(), counts.data_ptr(),
                                d_camera_fixed=D.fixed.data_ptr(), d_obs_state_out=state.data_ptr(), iterations=4, cg_iterations=8,
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    words = lambda x, t=np.uint32: x.cpu().numpy().view(t)
    assert np.array_equal(got["poses"], words(poses)) and np.array_equal(got["points"], words(points))
    O = int(s["counts"][1])
    assert np.array_equal(got["obs_state"][:O], words(state)[:O])
    assert np.array_equal(got["trace"][:, :8], words(trace, np.uint64)) and not got["trace"][:, 8].any()
    assert np.array_equal(got["counts"][:4], words(counts)) and got["counts"][4] == 0
    assert np.array_equal(got["intrinsics"], np.asarray(s["intrinsics"], np.float32).view(np.uint32))
    assert (groups_of(got) == [1.0, 0.0, 0.0]).all()


def test_the_group_map(torch, handle, twin):
    r = cases.realistic()
    N = 12
    a = check(torch, handle, twin, ic.with_groups(r, None, 1, scale=0.97), "a null map", refine=1)
    b = check(torch, handle, twin, ic.with_groups(r, np.zeros(N), 1, scale=0.97), "a map of zeros", refine=1)
    same(a, b, "a null map is a map of zeros")
    out = np.arange(N) % 3 == 0
    s = ic.with_groups(r, np.where(out, 7, 0), 1, scale=0.98)
    got = check(torch, handle, twin, s, "an id out of range", refine=1)
    assert np.array_equal(got["intrinsics"][out], s["intrinsics"].view(np.uint32)[out])
    assert (got["intrinsics"][~out, 0] != s["intrinsics"].view(np.uint32)[~out, 0]).all()
    g = np.zeros(N, np.uint32)
    g[:2] = 1                                                                # cameras 0 and 1 are the fixed ones
    got = check(torch, handle, twin, ic.with_groups(r, g, 2, scale=0.98), "a fixed-only group", refine=1)
    assert got["counts"][4] == 2 and groups_of(got)[1, 0] != 1.0
    s = ic.with_groups(dict(r, poses=r["poses"].copy()), np.where(np.arange(N) == 2, 1, 0), 2, scale=1.02)
    s["poses"][2] = 0
    got = check(torch, handle, twin, s, "an unregistered-only group", refine=3, px=6.0)
    assert got["counts"][4] == 1 and groups_of(got)[1].tolist() == [1.0, 0.0, 0.0]
    assert np.array_equal(got["intrinsics"][2], s["intrinsics"].view(np.uint32)[2])
    s = ic.with_groups(dict(r, camera_fixed=np.ones(N, np.uint32)), None, 1, scale=1.04)
    got = check(torch, handle, twin, s, "every camera fixed", refine=1)
    assert got["counts"][0] == 0 and got["counts"][4] == 1 and np.array_equal(got["poses"], s["poses"].view(np.uint32))


def test_a_held_group(torch, handle, twin):
    """the focal 15 % off under a 4 px threshold: one of the two groups starts without a single inlier and is held"""
    s = cases.build(30, cases.random_views(30, 100, 6, 2, 5), outliers=0.1, perturb=(0.02, 0.1, 0.1))
    got = check(torch, handle, twin, ic.with_groups(s, np.arange(6) % 2, 2, scale=1.15), "a held group", refine=3, lambda0=1e-6, iterations=3)
    tr = trace_of(got)
    assert tr[0, 8] >= 1 and got["counts"][4] == 2, tr[:, 8]


def test_a_rejected_focal_scale(torch, handle, twin):
    from test_bundle_intr_twin import mirrored
    s = mirrored()
    got = check(torch, handle, twin, s, "a rejected s", refine=1, px=3000.0, lambda0=1e-9, iterations=3, cg_iterations=64, cg_tol=1e-6)
    tr = trace_of(got)
    assert tr[0, 1] < tr[0, 0] and tr[0, 3] == 0
    K = got["intrinsics"].view(np.float32)
    assert np.isfinite(K).all() and (K[:, :2] > 0).all() and groups_of(got)[0, 0] > 0


def test_in_place_equals_apart(torch, handle, twin):
    s = ic.with_groups(cases.mixed(), np.arange(8) % 3, 3, scale=0.99)
    kw = dict(refine=3, px=6.0)
    want = check(torch, handle, twin, s, "apart", **kw)
    D = Device(torch, handle, s)
    bufs = D.buffers(4)
    D.run(bufs, in_place=True, **kw)
    torch.cuda.synchronize()
    res = D.read(bufs, 4)
    assert (res["poses"] == bit.FILL).all() and (res["points"] == bit.FILL).all() and (res["intrinsics"] == bit.FILL).all()
    res["poses"], res["points"] = D.poses.cpu().numpy().view(np.uint32), D.pts.cpu().numpy().view(np.uint32)
    res["intrinsics"] = D.K.cpu().numpy().view(np.uint32)
    same(res, want, "in place")
    none = Device(torch, handle, s).call(state_out=False, group_out=False, **kw)
    assert (none["obs_state"] == bit.FILL).all() and (none["groups"] == bit.FILL).all()
    same(none, want, "without the optional outputs", keys=("poses", "points", "intrinsics", "trace", "counts"))


def test_capacities_above_the_counts_and_counts_above_the_capacities(torch, handle, twin):
    g = dict(camera_group=np.arange(6, dtype=np.uint32) % 2, n_groups=2)
    base = ic.with_groups(cases.build(21, cases.random_views(21, 70, 6, 2, 5), outliers=0.03), scale=1.02, **g)
    roomy = ic.with_groups(cases.build(21, cases.random_views(21, 70, 6, 2, 5), outliers=0.03, capacity=(300, 1111)), scale=1.02, **g)
    a, b = check(torch, handle, twin, base, "tight", refine=1), check(torch, handle, twin, roomy, "roomy", refine=1)
    T, O = int(base["counts"][0]), int(base["counts"][1])
    for k in ("poses", "intrinsics", "groups", "trace", "counts"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["points"], b["points"][:T]) and (b["points"][T:] == bit.FILL).all()
    assert np.array_equal(a["obs_state"], b["obs_state"][:O]) and (b["obs_state"][O:] == bit.FILL).all()
    over = dict(base, counts=np.array([T + 1000, 0xFFFFFFFF], np.uint32))
    c = check(torch, handle, twin, over, "counts above the capacities", refine=1)
    for k in OUTPUTS:
        assert np.array_equal(a[k], c[k]), k


def test_garbage_inputs_end_equal_the_twin_and_stay_inside(torch, handle, twin):
    s = ic.with_groups(cases.garbage(), np.array([0, 1, 0, 9, 1, 0, 1]), 2, scale=1.01)
    got = check(torch, handle, twin, s, "garbage", refine=3, px=6.0)
    assert got["counts"][2] < s["counts"][1] and trace_of(got)[:, 3].sum() >= 1
    bad = dict(s, poses=s["poses"].copy(), points=s["points"].copy(), intrinsics=s["intrinsics"].copy())
    bad["poses"][2, 4], bad["points"][9, 1], bad["intrinsics"][4, 2] = np.nan, -np.inf, np.inf
    check(torch, handle, twin, bad, "garbage with a NaN pose, an infinite point and an infinite principal point", refine=3, px=6.0)


def test_nothing_free_copies_through(torch, handle, twin):
    s = ic.with_groups(cases.mixed(), np.arange(8) % 2, 2, scale=0.99)
    s["camera_fixed"][:] = 1
    s["obs_state"] = np.zeros(len(s["obs_row"]), np.uint32)
    got = check(torch, handle, twin, s, "nothing free", refine=3)
    assert got["counts"].tolist() == [0, 0, 0, 4, 0]
    assert np.array_equal(got["poses"], s["poses"].view(np.uint32)) and np.array_equal(got["points"], s["points"].view(np.uint32))
    assert np.array_equal(got["intrinsics"], s["intrinsics"].view(np.uint32)) and (groups_of(got) == [1.0, 0.0, 0.0]).all()
    empty = dict(s, counts=np.array([0, 0], np.uint32), obs_state=None)
    got = check(torch, handle, twin, empty, "T == 0", refine=3)
    assert np.array_equal(got["intrinsics"], s["intrinsics"].view(np.uint32)) and (got["points"] == bit.FILL).all()


def test_a_captured_call_replays_to_the_same_words_twice(torch, handle, twin):
    s = ic.with_groups(cases.track_lengths(), np.arange(9) % 2, 2, scale=1.02)
    kw = dict(refine=3, px=6.0)
    D = Device(torch, handle, s)
    a = D.call(**kw)                                                         # warmed up: the scratch has its size
    same(a, want_of(twin(s, **kw)), "first run")
    bufs = D.buffers(4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream, **kw)
    for _ in range(2):
        for v in bufs.values():
            v.fill_(bit.FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(D.read(bufs, 4), a, "replay")


def test_the_host_form_and_the_wrappers_equal_the_device_form(torch, handle, twin):
    s = ic.with_groups(cases.track_lengths(), np.arange(9) % 2, 2, scale=1.02)
    a = bit.arrays(s)
    want = Device(torch, handle, s).call(refine=3, px=6.0)
    host = handle.bundle_adjust_intrinsics(
        a["kps"], a["image_offsets"], a["track_offsets"], a["obs_row"], a["obs_image"], a["points"], a["intrinsics"], a["poses"],
        camera_fixed=a["camera_fixed"], camera_group=a["camera_group"], n_groups=2, refine=3, max_reproj_px=6.0, iterations=4,
        cg_iterations=8)
    for got, name in zip(host, OUTPUTS):
        assert np.array_equal(got.view(np.uint64 if name == "trace" else np.uint32).reshape(want[name].shape), want[name]), name
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    table = (up(a["track_offsets"].view(np.int64)), up(a["obs_row"]), up(a["obs_image"].view(np.int32)), None, up(a["counts"].view(np.int32)))
    out = lf.bundle_adjust_intrinsics(up(a["kps"]), up(a["image_offsets"].view(np.int64)), table, up(a["points"]), up(a["intrinsics"]),
                                      up(a["poses"]), camera_fixed=up(a["camera_fixed"].view(np.int32)),
                                      camera_group=up(a["camera_group"].view(np.int32)), n_groups=2, refine_focal=True,
                                      refine_principal=True, max_reproj_px=6.0, iterations=4, cg_iterations=8)
    torch.cuda.synchronize()
    for got, name in zip(out, OUTPUTS):
        words = got.cpu().numpy().view(np.uint64 if name == "trace" else np.uint32)
        assert np.array_equal(words.reshape(want[name].shape), want[name]), name
    # n_images == 0: LF_MKD_OK, nothing written (null pointers everywhere)
    handle.bundle_adjust_intrinsics_device(None, None, 0, 0, None, 0, None, None, 0, None, None, None, None, None, None, None, None,
                                           None, n_groups=0)


def test_match_collection_with_a_refined_focal(torch):
    """match_collection(..., bundle=4, refine_focal=True) on the example's frames runs, its cost does not rise and the focal
    comes back finite and positive (the frames are warps of one picture: the focal is not observable there, so no value is
    asserted; this is about the plumbing)"""
    import os
    import sys
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()[:3]])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), register=1, bundle=4,
                              refine_focal=True)
    torch.cuda.synchronize()
    tr, counts = got["bundle_trace"].cpu().numpy(), got["bundle_counts"].cpu().numpy()
    assert tr.shape == (4, 9) and (np.diff(tr[:, 0]) <= 0).all() and counts[3] == tr[:, 3].sum()
    g, K = got["bundle_groups"].cpu().numpy(), got["intrinsics"].cpu().numpy()
    assert g.shape == (1, 3) and np.isfinite(g).all() and g[0, 0] > 0 and g[0, 1:].tolist() == [0.0, 0.0]
    assert np.isfinite(K).all() and (K[:, :2] > 0).all()
    lines = ex.bundle_lines(got)
    assert any(line.startswith("refined focal ") for line in lines)
