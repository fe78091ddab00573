"""lf_mkd_triangulate_tracks_device on the GPU, every output compared as uint32 words against the host twin
(tests/cpp/triangulate_twin.cpp: the kernel's own csrc/mkd_triangulate_math.h compiled by g++; tests/test_triangulate_twin.py
ties the twin to the algorithm of include/lf_mkd.h): the families batch, every seam length up to one track of 5000 positions,
candidates that share a slot, every no-point reason and every cause of an unusable position, the reading rules, NULL d_err /
d_obs_state, rounds 0 and 4, thresholds that keep nothing and everything, a track's place in a batch, graph capture, the host
form, and the chain from verified matches through the pose call to triangulated tracks."""
import numpy as np
import pytest

import triangulate_cases as cases
import triangulate_twin as tt

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
WIDTH = dict(tt.OUTPUTS)
# The chain test's gate on |X_track - X_link|_inf / max(1, |X|_inf) for links of at least 2 degrees of parallax: 4 x the
# largest value measured on the CPU between pose_twin (R and t in f64) and triangulate_twin (their f32 stores) on
# pose_cases.problem(600, 0.3, seed, family) under the true F over the families general, sideways and forward and the seeds 9,
# 10 and 11: 2.5e-7, at depths up to 14 baselines (profiles/triangulate.md).
CHAIN_TOL = 4 * 2.5e-7


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
    tmp = tmp_path_factory.mktemp("triangulate_twin")
    exe = tt.build(tmp)
    return lambda table, px=4.0, rounds=2: tt.run(exe, tmp, table, px, rounds)


class Device:
    """a table on the device: the arrays hold exactly what their lengths say, so a read beyond them leaves the allocation's
    used part; every output between sentinels"""

    def __init__(self, torch, handle, t):
        self.torch, self.handle = torch, handle
        kps, off, row, img, counts, intr, poses = tt.arrays(t)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.kps, self.off, self.row, self.img = up(kps), up(off.view(np.int64)), up(row), up(img.view(np.int32))
        self.counts, self.intr, self.poses = up(counts.view(np.int32)), up(intr), up(poses)
        self.n_rows, self.tcap, self.ocap, self.n_images = len(kps), len(off) - 1, len(row), len(intr)
        self.rows = {"points": self.tcap, "stats": self.tcap, "err": self.tcap, "obs_state": self.ocap}

    def buffers(self):
        return {k: self.torch.full((WIDTH[k] * n + 2 * EXTRA,), tt.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.rows.items()}

    def run(self, bufs, px=4.0, rounds=2, err=True, state=True, stream=None):
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * EXTRA
        self.handle.triangulate_tracks_device(ptr(self.kps), self.n_rows, self.off.data_ptr(), self.tcap, ptr(self.row),
                                              ptr(self.img), self.ocap, self.counts.data_ptr(), ptr(self.intr), ptr(self.poses),
                                              self.n_images, out("points"), out("stats"), out("err") if err else None,
                                              out("obs_state") if state else None, px, rounds, 0,
                                              self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.rows.items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA] == tt.FILL).all() and (raw[EXTRA + WIDTH[k] * n:] == tt.FILL).all(), "a write outside d_" + k
            res[k] = raw[EXTRA:EXTRA + WIDTH[k] * n].reshape((n, WIDTH[k]) if WIDTH[k] > 1 else (n,))
        return res

    def call(self, px=4.0, rounds=2, err=True, state=True):
        bufs = self.buffers()
        self.torch.cuda.synchronize()
        self.run(bufs, px, rounds, err, state)
        self.torch.cuda.synchronize()
        return self.read(bufs)


def same(got, want, what, keys=("points", "stats", "err", "obs_state")):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), [hex(got[k][tuple(b)]) for b in bad[:5]],
                               [hex(want[k][tuple(b)]) for b in bad[:5]])


def check(torch, handle, twin, table, what, px=4.0, rounds=2):
    want = twin(table, px, rounds)
    got = Device(torch, handle, table).call(px, rounds)
    same(got, want, what)
    return got


def test_the_families_batch(torch, handle, twin):
    t, ref = cases.families()
    got = check(torch, handle, twin, t, "families")
    assert (got["stats"].astype(np.int64) == ref["stats"]).all()
    assert (got["stats"][:, 2] == 0).sum() >= 60 and (got["obs_state"] == 1).sum() >= 20     # points, and outliers left out


def test_every_seam_length(torch, handle, twin):
    t, ref = cases.seams()
    got = check(torch, handle, twin, t, "seams")
    assert np.diff(t["track_offsets"].astype(np.int64)).tolist() == list(cases.SEAM_LENGTHS)
    assert got["stats"][:2, 2].tolist() == [1, 1] and (got["stats"][2:, 2] == 0).all() and got["stats"][-1, 1] > 4000


def test_candidates_that_share_a_slot(torch, handle, twin):
    got = check(torch, handle, twin, cases.shared_slots(), "shared slots")
    assert got["stats"][0].tolist() == [7, 7, 0, 1]


def test_every_no_point_reason(torch, handle, twin):
    t, reasons = cases.no_point_reasons()
    got = check(torch, handle, twin, t, "reasons")
    assert got["stats"][:, 2].tolist() == reasons
    none = got["stats"][:, 2] != 0
    assert (got["points"][none] == np.array([0, 0, 0, 0x40000000], np.uint32)).all() and not got["err"][none].any()
    assert not (got["obs_state"][int(t["track_offsets"][1]):] == 2).any()


def test_every_cause_of_an_unusable_position(torch, handle, twin):
    t, bad = cases.unusable_causes()
    got = check(torch, handle, twin, t, "unusable")
    assert np.flatnonzero(got["obs_state"] == 0).tolist() == bad and (got["stats"][:, 2] == 0).all()


def test_the_reading_rules(torch, handle, twin):
    by = {}
    for name, t in cases.reading_rules():
        by[name] = check(torch, handle, twin, t, name)
    assert (by["fewer tracks than the capacity"]["stats"][4:] == tt.FILL).all()                 # tail rows untouched
    assert (by["fewer tracks than the capacity"]["points"][4:] == tt.FILL).all()
    assert all((by["no tracks"][k] == tt.FILL).all() for k in by["no tracks"])
    assert (by["no observations"]["stats"][:, 2] == 1).all() and (by["no observations"]["obs_state"] == tt.FILL).all()
    assert by["an inverted range"]["stats"][5].tolist() == [0, 0, 1, tt.NONE]
    assert (by["fewer observations: offsets beyond O"]["obs_state"][12:] == tt.FILL).all()        # entries of no track untouched
    same(by["more tracks than the capacity"], by["as made"], "counts[0] above the capacity")
    same(by["more observations than the capacity"], by["as made"], "counts[1] above the capacity")


def test_null_err_and_obs_state(torch, handle, twin):
    t, _ = cases.families()
    want = twin(t)
    D = Device(torch, handle, t)
    for err, state in ((False, True), (True, False), (False, False)):
        got = D.call(4.0, 2, err, state)
        same(got, want, (err, state), ("points", "stats") + (("err",) if err else ()) + (("obs_state",) if state else ()))
        assert err or (got["err"] == tt.FILL).all()
        assert state or (got["obs_state"] == tt.FILL).all()


@pytest.mark.parametrize("px,rounds", [(4.0, 0), (4.0, 4), (1e-4, 2), (1e6, 2), (1.0, 1)])
def test_other_rounds_and_thresholds(torch, handle, twin, px, rounds):
    t, ref = cases.decided_scene(31, np.random.default_rng(31).integers(2, 13, 24), 6, px=px, rounds=rounds, noise=0.5, outliers=0.15)
    got = check(torch, handle, twin, t, (px, rounds), px, rounds)
    if px == 1e-4:
        assert (got["stats"][:, 2] == 3).all() and not (got["obs_state"] == 2).any()     # nothing is an inlier
    if px == 1e6:
        assert (got["stats"][:, 1] == got["stats"][:, 0]).all() and (got["obs_state"] == 2).all()   # everything in front is


def test_a_track_alone_equals_the_track_in_any_batch(torch, handle, twin):
    t, _ = cases.seams()
    whole = Device(torch, handle, t).call()
    n = len(cases.SEAM_LENGTHS)
    order = np.random.default_rng(5).permutation(n)
    mixed = Device(torch, handle, cases.subset(t, order)).call()
    for name in ("points", "stats", "err"):
        assert np.array_equal(mixed[name], whole[name][order]), name
    off = t["track_offsets"].astype(np.int64)
    for i in (3, 9, n - 1):
        one = Device(torch, handle, cases.subset(t, [i])).call()
        for name in ("points", "stats", "err"):
            assert np.array_equal(one[name][0], whole[name][i]), (i, name)
        assert np.array_equal(one["obs_state"], whole["obs_state"][off[i]:off[i + 1]]), i


def test_two_runs_and_capture(torch, handle, twin):
    t, _ = cases.families()
    D = Device(torch, handle, t)
    a, b = D.call(), D.call()
    same(a, twin(t), "first run")
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    bufs = D.buffers()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for v in bufs.values():
        v.fill_(tt.FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), a, "replay")
    # new poses and keypoints in the same arrays: the replay reads them
    later = dict(t, kps=np.asarray(t["kps"]) + np.float32(0.25), poses=np.asarray(t["poses"])[::-1].copy())
    D.kps.copy_(torch.from_numpy(np.ascontiguousarray(later["kps"], np.float32)))
    D.poses.copy_(torch.from_numpy(np.ascontiguousarray(later["poses"], np.float32)))
    for v in bufs.values():
        v.fill_(tt.FILL)
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), twin(later), "replay on new inputs")


def test_the_host_form_equals_the_device_form(torch, handle, twin):
    t, _ = cases.unusable_causes()
    kps, off, row, img, counts, intr, poses = tt.arrays(t)
    want = Device(torch, handle, t).call()
    pts, st, err, state = handle.triangulate_tracks(kps, off, row, img, intr, poses)
    assert np.array_equal(pts.view(np.uint32), want["points"]) and np.array_equal(st, want["stats"])
    assert np.array_equal(err.view(np.uint32), want["err"]) and np.array_equal(state, want["obs_state"])
    pts2, st2, none, none2 = handle.triangulate_tracks(kps, off, row, img, intr, poses, err=False, obs_state=False)
    assert none is None and none2 is None and np.array_equal(pts2, pts) and np.array_equal(st2, st)
    # the wrapper, on tensors
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = lf.triangulate_tracks(up(kps), (up(off.view(np.int64)), up(row), up(img.view(np.int32)), up(np.concatenate([counts, counts]).view(np.int32))),
                                up(intr), up(poses))
    torch.cuda.synchronize()
    for got, name in zip(out, ("points", "stats", "err", "obs_state")):
        assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(want[name].shape), want[name]), name


@pytest.mark.parametrize("family", ("general", "sideways", "forward"))
def test_chain_from_matches_to_points(family, torch, handle, twin):
    """two_view keypoints -> verify_fundamental -> link_table -> two_view_pose -> poses {[I | 0], [R | t]} -> build_tracks and
    track_table over that edge -> triangulate_tracks: the result is the twin's on the same device-produced table and poses,
    and a track that is one link gets the pose call's point for that link, within CHAIN_TOL."""
    import pose_cases as pc
    ka, kb, mt = pc.problem(600, 0.3, 9, family)
    na, nb = len(ka), len(kb)
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pool = up(np.concatenate([ka, kb]).astype(np.float32))
    img_off, off_a, off_b = up(np.array([0, na, na + nb], np.int64)), up(np.array([0, na], np.int64)), up(np.array([0, nb], np.int64))
    F, ver, _ = lf.verify_fundamental_batch(pool[:na], off_a, pool[na:], off_b, up(mt), 1.5, 512, 17)
    ea, eb = up(np.array([0], np.int32)), up(np.array([1], np.int32))
    ver = ver.contiguous()
    l_off, la, lb = lf.link_table(img_off, ea, eb, off_a, ver, n_rows=na + nb)[:3]
    K = up(np.tile(pc.K4, (2, 1)).astype(np.float32))
    R, t, pst, _, link_pts = lf.two_view_pose(F.contiguous(), K, pool, (ea, eb), (l_off, la, lb), 2.0)
    poses = torch.cat([torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32, device="cuda"),
                       torch.cat([R.reshape(1, 9), t.reshape(1, 3)], 1)]).contiguous()
    track, length, dup = lf.build_tracks(img_off, ea, eb, off_a, ver, n_rows=na + nb)
    table = lf.track_table(track, length, dup, img_off)
    pts, st, err, state = lf.triangulate_tracks(pool, table, K, poses, 4.0, 2)
    torch.cuda.synchronize()
    offsets, rows, images, _, counts = (x.cpu().numpy() for x in table)
    host = {"kps": pool.cpu().numpy(), "track_offsets": offsets.view(np.uint64), "obs_row": rows, "obs_image": images.view(np.uint32),
            "counts": counts.view(np.uint32), "intrinsics": K.cpu().numpy(), "poses": poses.cpu().numpy()}
    want = twin(host)
    T, O = int(counts[0]), int(counts[1])
    n_links = int(l_off.cpu()[1])
    assert int(pst.cpu()[0, 2]) >= 0 and n_links > 300 and T > 0.9 * n_links
    assert np.array_equal(pts.cpu().numpy().view(np.uint32)[:T], want["points"][:T])
    assert np.array_equal(st.cpu().numpy().view(np.uint32)[:T], want["stats"][:T])
    assert np.array_equal(err.cpu().numpy().view(np.uint32)[:T], want["err"][:T])
    assert np.array_equal(state.cpu().numpy().view(np.uint32)[:O], want["obs_state"][:O])
    # a track of two rows (a, b) is the link a -> b: find it
    link_of = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(la.cpu().numpy()[:n_links], lb.cpu().numpy()[:n_links]))}
    pairs = [(i, link_of.get((int(rows[offsets[i]]), int(rows[offsets[i] + 1])), -1)) for i in range(T) if offsets[i + 1] - offsets[i] == 2]
    ti, ki = np.array([p for p in pairs if p[1] >= 0]).T
    assert len(ti) > 0.9 * n_links
    X, Xl = pts.cpu().numpy()[ti].astype(np.float64), link_pts.cpu().numpy()[ki].astype(np.float64)
    both = (st.cpu().numpy()[ti, 2] == 0) & (Xl[:, 3] <= np.cos(np.radians(2.0)))
    assert both.sum() > 0.5 * n_links                                 # (forward motion: little parallax near the epipole)
    dev = np.abs(X[both, :3] - Xl[both, :3]).max(1) / np.maximum(1.0, np.abs(Xl[both, :3]).max(1))
    print(f"{family}: {T} tracks, {int(both.sum())} compared, largest deviation {dev.max():.3g} (gate {CHAIN_TOL:.3g}), "
          f"cosine deviation {np.abs(X[both, 3] - Xl[both, 3]).max():.3g}")
    assert dev.max() <= CHAIN_TOL


def test_match_collection_with_triangulate(torch, twin):
    """match_collection(frames, "window", 1, fundamental=True, pose=..., triangulate=True): the points are the twin's on the
    track table, the keypoints and the poses the same run left on the device, and the initial pair is the edge with the most
    links with parallax.  (The frames are warps of one picture -- one plane -- so the geometry means little; this is about
    the plumbing.)"""
    import os
    import sys
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()[:3]])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), triangulate=True)
    torch.cuda.synchronize()
    poses, pst = got["tri_poses"].cpu().numpy(), got["pose_stats"].cpu().numpy()
    e = int(np.argmax(np.where(pst[:, 2] >= 0, pst[:, 3], -1)))
    a, b = int(got["edge_a"][e]), int(got["edge_b"][e])
    assert poses[a].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and not poses[3 - a - b].any()
    assert np.array_equal(poses[b], np.concatenate([got["pose_R"][e].cpu().numpy().reshape(9), got["pose_t"][e].cpu().numpy()]))
    table = {"kps": got["keypoints"].cpu().numpy(), "track_offsets": got["table_offsets"].cpu().numpy().view(np.uint64),
             "obs_row": got["table_rows"].cpu().numpy(), "obs_image": got["table_images"].cpu().numpy().view(np.uint32),
             "counts": got["table_counts"].cpu().numpy().view(np.uint32), "intrinsics": np.tile(np.array([800, 800, 512, 384], np.float32), (3, 1)),
             "poses": poses}
    want = twin(table)
    T, O = (int(v) for v in table["counts"][:2])
    assert T > 100
    for key, name in (("points", "tri_points"), ("stats", "tri_stats"), ("err", "tri_err")):
        assert np.array_equal(got[name].cpu().numpy().view(np.uint32)[:T], want[key][:T]), name
    assert np.array_equal(got["tri_obs_state"].cpu().numpy().view(np.uint32)[:O], want["obs_state"][:O])
    assert (want["stats"][:T, 0] <= 2).all()                           # two registered images: at most two usable observations
    plain = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0))
    assert all(plain[k] is None for k in ("tri_poses", "tri_points", "tri_stats", "tri_err", "tri_obs_state"))
