"""lf_mkd_resect_cameras_device on the GPU, every output compared as uint32 words against the host twin
(tests/cpp/resect_twin.cpp: the kernels' own csrc/mkd_resect_math.h compiled by g++; tests/test_resect_twin.py ties the twin to
the algorithm of include/lf_mkd.h): the families batch, every seam of M and of n_samples, the slice boundary, the reading
rules, candidacy and the in-place call, every reason, min_inliers on both sides of the count, other parameters, an image's
place in a batch, graph capture, the host form, the chain from links to five registered cameras, and the example."""
import numpy as np
import pytest

import resect_cases as cases
import resect_twin as rt

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
WIDTH = dict(rt.OUTPUTS)
# the chain's poses against the truth: the CPU recovery bounds of tests/test_resect_twin.py (numpy's own errors, times 2)
ROT_BOUND, T_BOUND = 2 * 8.72e-4, 2 * 6.82e-3


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
    tmp = tmp_path_factory.mktemp("resect_twin")
    exe = rt.build(tmp)
    return lambda scene, **kw: rt.run(exe, tmp, scene, **kw)


class Device:
    """a scene on the device: the arrays hold exactly what their lengths say, so a read beyond them leaves the allocation's
    used part; every output between sentinels"""

    def __init__(self, torch, handle, s):
        self.torch, self.handle = torch, handle
        kps, off, rtk, pts, counts, intr, poses = rt.arrays(s)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.kps, self.off, self.rtk, self.pts = up(kps), up(off.view(np.int64)), up(rtk), up(pts)
        self.counts, self.intr, self.poses = up(counts.view(np.int32)), up(intr), up(poses)
        self.n_rows, self.tcap, self.n_images = len(kps), len(pts), len(intr)
        self.rows = {"poses": self.n_images, "stats": self.n_images, "err": self.n_images, "row_state": self.n_rows}

    def buffers(self):
        return {k: self.torch.full((WIDTH[k] * n + 2 * EXTRA,), rt.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.rows.items()}

    def run(self, bufs, stream=None, err=True, state=True, in_place=False, **kw):
        p = {**rt.DEFAULTS, **kw}
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * EXTRA
        self.handle.resect_cameras_device(ptr(self.kps), self.off.data_ptr(), self.n_images, self.n_rows, ptr(self.rtk), ptr(self.pts),
                                          self.tcap, self.counts.data_ptr(), ptr(self.intr), ptr(self.poses),
                                          ptr(self.poses) if in_place else out("poses"), out("stats"), out("err") if err else None,
                                          out("row_state") if state else None, p["px"], p["deg"], p["n_samples"], p["min_inliers"],
                                          p["rounds"], p["seed"], p["flags"],
                                          self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.rows.items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA] == rt.FILL).all() and (raw[EXTRA + WIDTH[k] * n:] == rt.FILL).all(), "a write outside d_" + k
            res[k] = raw[EXTRA:EXTRA + WIDTH[k] * n].reshape((n, WIDTH[k]) if WIDTH[k] > 1 else (n,))
        return res

    def call(self, **kw):
        bufs = self.buffers()
        self.torch.cuda.synchronize()
        self.run(bufs, **kw)
        self.torch.cuda.synchronize()
        return self.read(bufs)


def same(got, want, what, keys=("poses", "stats", "err", "row_state")):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), [hex(got[k][tuple(b)]) for b in bad[:5]],
                               [hex(want[k][tuple(b)]) for b in bad[:5]])


def check(torch, handle, twin, scene, what, **kw):
    want = twin(scene, **kw)
    got = Device(torch, handle, scene).call(**kw)
    same(got, want, what)
    return got


def test_the_families_batch(torch, handle, twin):
    s = cases.families()
    got = check(torch, handle, twin, s, "families")
    assert got["stats"][:, 0].tolist() == [3, 7, 12, 40, 65, 100, 256, 257, 300, 420, 513, 600]
    assert (got["stats"][3:, 2] == 0).all() and (got["row_state"] == 2).sum() > 1500 and (got["row_state"] == 1).sum() > 500
    for i in range(3, 12):
        r, t = cases.pose_error(rt.f32(got["poses"][i]), s["truth"][i])
        assert r < 0.01 and t < 0.05, (i, r, t)


@pytest.mark.parametrize("n_samples", (1, 63, 64, 65, 256, 257))
def test_every_seam_of_m_and_of_the_candidate_block(torch, handle, twin, n_samples):
    """M around the chunk of the compaction and of the 256-slot sum, and 1025, the smallest M of two slices of rs_score; a
    candidate block is 256 candidates = 64 samples"""
    s = cases.seams()
    got = check(torch, handle, twin, s, "seams x %d" % n_samples, n_samples=n_samples, min_inliers=3)
    assert got["stats"][:, 0].tolist() == list(cases.SEAM_M)
    assert (got["stats"][:3, 2] == 2).all() and (n_samples < 64 or (got["stats"][4:, 2] == 0).all())


@pytest.mark.parametrize("delta", (0, -30, 1000))
def test_the_reading_rules(torch, handle, twin, delta):
    s = cases.reading_rules(counts_delta=delta)
    got = check(torch, handle, twin, s, "reading rules %d" % delta, deg=5.0)
    st = got["stats"].astype(np.int64)
    assert st[0, 0] == 80 - 12 and st[[2, 3, 4, 5], 2].tolist() == [1, 1, 1, 1] and st[[8, 9, 11], 0].tolist() == [0, 0, 0]
    assert st[10, 0] == st[7, 0] == (80 if delta >= 0 else 60)                # the range beyond the pool is clamped to it
    off = s["image_offsets"].astype(np.int64)
    for i in (2, 3, 4, 5):                                                    # no candidate: its rows keep the fill pattern
        assert (got["row_state"][off[i]:off[i + 1]] == rt.FILL).all()
    assert (got["poses"][4] == s["poses"][4].view(np.uint32)).all() and (got["poses"][5] == s["poses"][5].view(np.uint32)).all()


def test_candidacy_and_the_in_place_call(torch, handle, twin):
    s = cases.families()
    s["poses"][[4, 7]] = s["truth"][[5, 8]]                                   # registered, with poses that are not theirs
    got = check(torch, handle, twin, s, "registered")
    assert got["stats"][[4, 7], 2].tolist() == [1, 1] and (got["poses"][[4, 7]] == s["poses"][[4, 7]].view(np.uint32)).all()
    every = check(torch, handle, twin, s, "resect all", flags=lfp.RESECT_ALL)
    assert (every["stats"][3:, 2] == 0).all() and (every["poses"][4] != got["poses"][4]).any()
    for flags, want in ((0, got), (lfp.RESECT_ALL, every)):
        D = Device(torch, handle, s)
        bufs = D.buffers()
        D.run(bufs, in_place=True, flags=flags)
        torch.cuda.synchronize()
        res = D.read(bufs)
        assert (res["poses"] == rt.FILL).all()
        res["poses"] = D.poses.cpu().numpy().view(np.uint32)
        same(res, want, "in place, flags %d" % flags)


def test_every_reason(torch, handle, twin):
    got = check(torch, handle, twin, cases.reasons(), "reasons")
    assert got["stats"][:, 2].tolist() == [0, 1, 2, 2, 3] and got["stats"][:, 0].tolist() == [120, 0, 2, 60, 60]
    assert not got["poses"][[2, 3, 4]].any() and not got["err"][1:].any() and (got["row_state"] <= 2).sum() > 0
    off = cases.reasons()["image_offsets"].astype(np.int64)
    assert (got["row_state"][off[2]:] != 2).all()                             # a no-pose image has 0 and 1 only


def test_min_inliers_on_both_sides_of_the_count(torch, handle, twin):
    s = cases.sub_scene(cases.families(), [5])
    n = int(twin(s)["stats"][0, 1])
    assert n > 12
    at, above = check(torch, handle, twin, s, "at the count", min_inliers=n), check(torch, handle, twin, s, "above", min_inliers=n + 1)
    assert at["stats"][0, 1:3].tolist() == [n, 0] and above["stats"][0, 1:3].tolist() == [0, 3] and not above["poses"].any()
    assert at["stats"][0, 3] == above["stats"][0, 3] and (above["row_state"] != 2).all()


def test_collinear_triples_only(torch, handle, twin):
    got = check(torch, handle, twin, cases.sub_scene(cases.reasons(), [3]), "collinear", seed=3, n_samples=256)
    assert got["stats"][0].tolist() == [60, 0, 2, rt.NONE]


@pytest.mark.parametrize("kw", (dict(rounds=0), dict(rounds=4), dict(px=1e-4), dict(px=1e6), dict(deg=5.0), dict(seed=0xFFFFFFFF)))
def test_other_parameters(torch, handle, twin, kw):
    got = check(torch, handle, twin, cases.families(), str(kw), **kw)
    if kw.get("px") == 1e6:
        assert (got["stats"][2:, 1] == got["stats"][2:, 0]).all()
    if kw.get("px") == 1e-4:
        assert (got["stats"][3:, 2] == 3).all()


def test_null_err_and_row_state(torch, handle, twin):
    s = cases.families()
    got = Device(torch, handle, s).call(err=False, state=False)
    assert (got["err"] == rt.FILL).all() and (got["row_state"] == rt.FILL).all()
    same(got, twin(s), "without the optional outputs", keys=("poses", "stats"))


def test_an_image_alone_equals_the_image_in_any_batch(torch, handle, twin):
    """the sampler is keyed on seed + image id: image i alone under seed + i, or at position i - 3 of a batch under seed + 3"""
    s = cases.families()
    whole = check(torch, handle, twin, s, "whole", seed=11)
    off = s["image_offsets"].astype(np.int64)
    for i in (3, 6, 11):
        alone = Device(torch, handle, cases.sub_scene(s, [i])).call(seed=11 + i)
        for k in ("poses", "stats", "err"):
            assert (alone[k][0] == whole[k][i]).all(), (i, k)
        assert (alone["row_state"] == whole["row_state"][off[i]:off[i + 1]]).all()
    part = Device(torch, handle, cases.sub_scene(s, [3, 4, 5, 6, 7])).call(seed=14)
    for k in ("poses", "stats", "err"):
        assert (part[k] == whole[k][3:8]).all(), k


def test_two_runs_and_capture(torch, handle, twin):
    s = cases.families()
    D = Device(torch, handle, s)
    a, b = D.call(), D.call()
    same(a, twin(s), "first run")
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    bufs = D.buffers()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for v in bufs.values():
        v.fill_(rt.FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), a, "replay")
    # new keypoints in the same arrays: the replay reads them
    later = dict(s, kps=np.asarray(s["kps"]) + np.float32(0.25))
    D.kps.copy_(torch.from_numpy(np.ascontiguousarray(later["kps"], np.float32)))
    for v in bufs.values():
        v.fill_(rt.FILL)
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), twin(later), "replay on new inputs")


def test_the_host_form_equals_the_device_form_and_no_images_is_ok(torch, handle, twin):
    s = cases.sub_scene(cases.families(), [8])
    kps, off, rtk, pts, counts, intr, poses = rt.arrays(s)
    want = Device(torch, handle, s).call(seed=5)
    pose, st, err, state = handle.resect_camera(kps, rtk, pts, intr[0], n_samples=64, seed=5)
    assert np.array_equal(pose.view(np.uint32), want["poses"][0]) and np.array_equal(st, want["stats"][0])
    assert np.array_equal(err.view(np.uint32), want["err"][0]) and np.array_equal(state, want["row_state"])
    pose2, st2, none, none2 = handle.resect_camera(kps, rtk, pts, intr[0], n_samples=64, seed=5, err=False, row_state=False)
    assert none is None and none2 is None and np.array_equal(pose2, pose) and np.array_equal(st2, st)
    # the wrapper, on tensors
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = lf.resect_cameras(up(kps), up(off.view(np.int64)), up(rtk), up(pts), up(counts.view(np.int32)), up(intr), up(poses),
                            n_samples=64, seed=5)
    torch.cuda.synchronize()
    for got, name in zip(out, ("poses", "stats", "err", "row_state")):
        assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(want[name].shape), want[name]), name
    # n_images == 0: LF_MKD_OK, nothing written (null pointers everywhere)
    handle.resect_cameras_device(None, None, 0, 0, None, None, 0, None, None, None, None, None)


def test_chain_from_links_to_five_registered_cameras(torch, twin):
    """synthetic keypoints of 5 cameras, no images: link_table -> two_view_pose on the initial pair -> build_tracks / track_table
    -> triangulate_tracks -> (resect_cameras in place -> triangulate_tracks) x 2, nothing read back in between"""
    kps, off, (ea, eb), matches, K, truth, F = cases.chain()
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = len(kps)
    pool, img_off, dea, deb = up(kps), up(off), up(ea), up(eb)
    layout = lf.edge_layout(img_off, dea, n)
    match = up(np.concatenate(matches))
    l_off, la, lb = lf.link_table(img_off, dea, deb, layout, match, n_rows=n)[:3]
    Ks = up(np.tile(K, (5, 1)))
    R, t, pst, _, _ = lf.two_view_pose(up(F), Ks, pool, (dea, deb), (l_off, la, lb), 2.0)
    poses = torch.zeros((5, 12), dtype=torch.float32, device="cuda")
    poses[0] = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float32)
    poses[1] = torch.cat([R[0].reshape(9), t[0].reshape(3)])                  # edge 0 is (0, 1)
    track, length, dup = lf.build_tracks(img_off, dea, deb, layout, match, n_rows=n)
    table = lf.track_table(track, length, dup, img_off)
    row_track, counts = table[3], table[4]
    pts0, st0, _, _ = lf.triangulate_tracks(pool, table, Ks, poses, 4.0, 2)
    pts, registered, with_point = pts0, [], [st0]
    for _ in range(2):
        _, rst, _, _ = lf.resect_cameras(pool, img_off, row_track, pts, counts, Ks, poses, n_samples=256, out=poses)
        pts, st, _, _ = lf.triangulate_tracks(pool, table, Ks, poses, 4.0, 2)
        registered.append(rst), with_point.append(st)
    torch.cuda.synchronize()
    T = int(counts.cpu()[0])
    n_pts = [int((s.cpu().numpy()[:T, 2] == 0).sum()) for s in with_point]
    P = poses.cpu().numpy()
    errs = [cases.pose_error(P[i], truth[i]) for i in range(5)]
    print("points per round", n_pts, "of", T, "tracks; pose errors", errs)
    assert P[:, :9].any(1).all()                                              # all five registered
    assert registered[0].cpu().numpy()[:2, 2].tolist() == [1, 1] and (registered[0].cpu().numpy()[2:, 2] == 0).all()
    assert (registered[1].cpu().numpy()[:, 2] == 1).all()                     # the second round finds nothing left to do
    assert n_pts[1] > n_pts[0] and n_pts[2] >= n_pts[1] and n_pts[2] > 0.95 * T
    assert max(e[0] for e in errs) <= ROT_BOUND and max(e[1] for e in errs) <= T_BOUND, errs
    # the last resection is the twin's on what the device held
    host = dict(kps=kps, image_offsets=off.astype(np.uint64), row_track=row_track.cpu().numpy(), points=pts0.cpu().numpy(),
                counts=counts.cpu().numpy().view(np.uint32), intrinsics=np.tile(K, (5, 1)), poses=np.zeros((5, 12), np.float32))
    host["poses"][:2] = P[:2]
    want = twin(host, n_samples=256)
    assert np.array_equal(P.view(np.uint32), want["poses"]) and np.array_equal(registered[0].cpu().numpy().view(np.uint32), want["stats"])


def test_match_collection_with_register(torch):
    """match_collection(..., pose=.., register=2) on the example's frames runs and reports its rounds (the frames are warps of
    one picture, so the geometry means little; this is about the plumbing)"""
    import os
    import sys
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()[:3]])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), register=2)
    torch.cuda.synchronize()
    rounds = got["register_rounds"]
    assert len(rounds) == 2 and got["tri_poses"] is not None
    for stats, tri in rounds:
        st = stats.cpu().numpy()
        assert st.shape == (3, 4) and set(st[:, 2].tolist()) <= {0, 1, 2, 3}
    assert (rounds[0][0].cpu().numpy()[:, 2] == 1).sum() == 2                 # the initial pair is registered already
    lines = ex.register_lines(got)
    assert len(lines) == 2 and all(line.startswith("round ") for line in lines)
