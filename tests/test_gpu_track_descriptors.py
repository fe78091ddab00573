"""lf_mkd_track_descriptors_device on the GPU: every output byte and word == the numpy restatement of the contract
(tests/track_desc_cases.py; tests/test_track_desc_twin.py ties the host twin, the kernel's own header under g++, to the same
restatement), each output between sentinels; then the route it exists for: a model from four cameras, the fifth localised
by one match and one resection."""
import os

import numpy as np
import pytest

import q8_cases
import resect_cases
import track_desc_cases as cases

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 36                       # sentinel words in front of and behind every output (a multiple of 4: d_desc is 16-byte aligned)
FILL = 0x5AA55AA5
CASES = dict(cases.cpu_cases())
_WANT = {}


def want(name):
    """the restatement of a case, computed once"""
    if name not in _WANT:
        _WANT[name] = cases.restate(CASES[name])
    return _WANT[name]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


class Device:
    """a call on the device: the arrays hold exactly what their lengths say, so a read beyond them leaves the allocation's
    used part; both outputs between sentinels"""

    def __init__(self, torch, handle, c):
        self.torch, self.handle, self.c = torch, handle, c
        q, off, row, counts, st, pts = cases.arrays(c)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.q, self.off, self.row, self.counts = up(q), up(off.view(np.int64)), up(row), up(counts.view(np.int32))
        self.st, self.pts = up(None if st is None else st.view(np.int32)), up(pts)
        self.n_rows, self.tcap, self.ocap = len(q), len(off) - 1, len(row)
        self.words = {"desc": 32 * self.tcap, "stats": 2 * self.tcap}

    def buffers(self):
        return {k: self.torch.full((n + 2 * EXTRA,), FILL, dtype=self.torch.int32, device="cuda") for k, n in self.words.items()}

    def run(self, bufs, stream=None):
        c = self.c
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * EXTRA
        self.handle.track_descriptors_device(ptr(self.q), self.n_rows, self.off.data_ptr(), self.tcap, ptr(self.row), self.ocap,
                                             self.counts.data_ptr(), out("desc"), out("stats") if c["stats"] else None,
                                             None if self.st is None else self.st.data_ptr(), c["min_state"],
                                             None if self.pts is None else self.pts.data_ptr(), c["deg"], c["scale"],
                                             self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs):
        """(desc uint8 [track_capacity, 128], stats int32 [track_capacity, 2]) out of their frames; the sentinels must have
        survived"""
        res = []
        for k, n in self.words.items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA] == FILL).all() and (raw[EXTRA + n:] == FILL).all(), "a write outside d_" + k
            res.append(raw[EXTRA:EXTRA + n])
        return res[0].view(np.uint8).reshape(self.tcap, 128), res[1].view(np.int32).reshape(self.tcap, 2)

    def call(self):
        bufs = self.buffers()
        self.torch.cuda.synchronize()
        self.run(bufs)
        self.torch.cuda.synchronize()
        return self.read(bufs)


def same(got, wanted, what, stats=True):
    bad = np.argwhere(got[0] != wanted[0])
    assert len(bad) == 0, (what, "desc", len(bad), bad[:5].tolist())
    if stats:
        bad = np.argwhere(got[1] != wanted[1])
        assert len(bad) == 0, (what, "stats", len(bad), bad[:5].tolist(), got[1][bad[:5, 0]].tolist(), wanted[1][bad[:5, 0]].tolist())
    else:
        assert (got[1].view(np.uint32) == FILL).all(), (what, "d_desc_stats is NULL and was written")


@pytest.mark.parametrize("name", list(CASES))
def test_every_byte_and_word_is_the_restatements(torch, handle, name):
    c = CASES[name]
    got = Device(torch, handle, c).call()
    same(got, want(name), name, stats=c["stats"])
    if name == "lengths":
        long = int(np.argmax(np.diff(c["track_offsets"].astype(np.int64))[:int(c["counts"][0])]))
        assert got[1][long, 0] == cases.MAX_OBS                               # the cap: 65 536 of 70 000


@pytest.mark.parametrize("lanes", ("4", "16"))
def test_the_other_group_widths_give_the_same_bytes(torch, handle, lanes):
    old = os.environ.get("LF_MKD_TRACK_DESC_LANES")
    os.environ["LF_MKD_TRACK_DESC_LANES"] = lanes
    try:
        for name in ("lengths", "many"):
            same(Device(torch, handle, CASES[name]).call(), want(name), "%s at %s lanes" % (name, lanes))
    finally:
        if old is None:
            os.environ.pop("LF_MKD_TRACK_DESC_LANES")
        else:
            os.environ["LF_MKD_TRACK_DESC_LANES"] = old


def test_two_runs_and_capture(torch, handle):
    D = Device(torch, handle, CASES["many"])
    a, b = D.call(), D.call()
    same(a, want("many"), "first run")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    bufs = D.buffers()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for v in bufs.values():
        v.fill_(FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), a, "replay")
    # other rows in the same array: the replay reads them
    later = dict(CASES["many"], q=np.roll(np.asarray(CASES["many"]["q"]), 3, axis=0))
    D.q.copy_(torch.from_numpy(np.ascontiguousarray(later["q"])))
    for v in bufs.values():
        v.fill_(FILL)
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), cases.restate(later), "replay on new inputs")


def test_a_permutation_of_the_tracks_permutes_the_rows(torch, handle):
    q, tracks = cases.length_tracks(long=0)
    order = np.random.default_rng(9).permutation(len(tracks))
    a = Device(torch, handle, cases.call(q, tracks)).call()
    b = Device(torch, handle, cases.permuted(tracks, q, order)).call()
    assert np.array_equal(a[0][order], b[0]) and np.array_equal(a[1][order], b[1])


def test_the_host_form_the_wrapper_and_the_empty_call(torch, handle):
    c = CASES["states and points"]
    q, off, row, counts, st, pts = cases.arrays(c)
    T, O = int(counts[0]), int(counts[1])
    wanted = want("states and points")
    desc, ds = handle.track_descriptors(q, off[:T + 1], row[:O], st[:O], c["min_state"], pts[:T], c["deg"], c["scale"])
    assert np.array_equal(desc, wanted[0][:T]) and np.array_equal(ds, wanted[1][:T])
    desc2, none = handle.track_descriptors(q, off[:T + 1], row[:O], st[:O], c["min_state"], pts[:T], c["deg"], c["scale"], stats=False)
    assert none is None and np.array_equal(desc2, desc)
    # the wrapper, on tensors
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table = (up(off.view(np.int64)), up(row), None, up(np.concatenate([counts, [0, 0]]).astype(np.uint32).view(np.int32)))
    got = lf.track_descriptors(up(q), table, up(st.view(np.int32)), c["min_state"], up(pts), c["deg"], c["scale"], stats=True)
    only = lf.track_descriptors(up(q), table, up(st.view(np.int32)), c["min_state"], up(pts), c["deg"], c["scale"])
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), wanted[0]) and np.array_equal(got[1].cpu().numpy(), wanted[1])
    assert np.array_equal(only.cpu().numpy(), wanted[0])
    # track_capacity == 0: LF_MKD_OK, nothing written (null pointers everywhere)
    handle.track_descriptors_device(None, 0, None, 0, None, 0, None, None)


def rotation_error(P, Q):
    """the angle between two rotations from the Frobenius norm of their difference (well conditioned near zero, where the
    arccos of a trace is not)"""
    d = np.linalg.norm(np.asarray(P, np.float64)[:9] - np.asarray(Q, np.float64)[:9])
    return float(2 * np.arcsin(min(1.0, d / (2 * np.sqrt(2)))))


def test_a_held_out_image_is_localised_by_one_match_and_one_resection(torch):
    """resect_cases.chain()'s scene with descriptors (tests/track_desc_cases.py, route_scene): triangulate four cameras' tracks
    at their true poses, describe the tracks that got a point from their inlier observations, localise the fifth camera's
    image -- its rows among clutter -- and a second image of clutter alone."""
    s = cases.route_scene(sigma=0.1)
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    toff, obs_row, obs_image, counts = s["table"]
    counts4 = np.concatenate([counts, [0, 0]]).astype(np.uint32).view(np.int32)
    table = (up(toff.view(np.int64)), up(obs_row), up(obs_image.view(np.int32)), up(counts4))
    Ks = up(np.tile(s["K"], (4, 1)))
    pts, st, _, obs_state = lf.triangulate_tracks(up(s["pool_kps"]), table, Ks, up(s["truth"][:4].astype(np.float32)), 4.0, 2)
    model = lf.track_descriptors(up(s["pool_q"]), table, obs_state, 2, pts, 0.0)
    Kq = up(np.tile(s["K"], (2, 1)))
    q_kps, q_q, q_off = up(s["query_kps"]), up(s["query_q"]), up(s["query_offsets"])
    poses, stats, err, row_state, row_track = lf.localize(q_q, q_kps, q_off, model, pts, table[3], Kq, ratio=0.8, n_samples=256)
    # the EXISTING resection call on the same images, handed the true row_track
    ref_poses, ref_stats, _, _ = lf.resect_cameras(q_kps, q_off, up(s["true_row_track"]), pts, table[3], Kq,
                                                   torch.zeros((2, 12), dtype=torch.float32, device="cuda"), n_samples=256)
    torch.cuda.synchronize()

    # numpy's model rows from what the device triangulated, and numpy's matcher over them
    points, state = pts.cpu().numpy(), obs_state.cpu().numpy().view(np.uint32)
    model_np, _ = cases.restate(dict(q=s["pool_q"], track_offsets=toff, obs_row=obs_row, counts=counts, obs_state=state,
                                     min_state=2, points=points, deg=0.0, scale=256.0, stats=True))
    assert np.array_equal(model.cpu().numpy(), model_np)
    match_np, _, _ = q8_cases.match_q8(s["query_q"], model_np, 0.8)
    # the input conditions, on the numpy side: the held-out image's true correspondences are the rows whose own track has a
    # point; numpy alone recovers at least 70 % of them, and at most 30 % of what it accepts in that image is wrong
    true, n_held, n0 = s["true_row_track"], s["n_held"], int(s["query_offsets"][1])
    has = (true[:n_held] >= 0) & (points[np.maximum(true[:n_held], 0), 3] < 1.5)
    recovered = float((match_np[:n_held][has] == true[:n_held][has]).mean())
    accepted = match_np[:n0] >= 0
    wrong = float((match_np[:n0][accepted] != true[:n0][accepted]).mean())
    print("true correspondences %d, numpy recovers %.3f; accepted %d, wrong %.3f" % (has.sum(), recovered, accepted.sum(), wrong))
    assert has.sum() > 300 and recovered >= 0.7 and wrong <= 0.3

    assert np.array_equal(row_track.cpu().numpy(), match_np)
    P, ref, truth = poses.cpu().numpy(), ref_poses.cpu().numpy(), s["truth"][4]
    st_q, st_ref = stats.cpu().numpy(), ref_stats.cpu().numpy()
    assert st_q[0, 2] == 0 and st_ref[0, 2] == 0, (st_q, st_ref)
    e_rot, e_t = rotation_error(P[0], truth), resect_cases.pose_error(P[0], truth)[1]
    r_rot, r_t = rotation_error(ref[0], truth), resect_cases.pose_error(ref[0], truth)[1]
    print("localize: rotation %.3e rad, translation %.3e, %d inliers; resection on the true row_track: %.3e, %.3e, %d inliers"
          % (e_rot, e_t, st_q[0, 1], r_rot, r_t, st_ref[0, 1]))
    assert e_rot <= 2 * r_rot and e_t <= 2 * r_t
    # the image of clutter alone: no pose, for want of candidates or of inliers
    assert st_q[1, 2] in (2, 3) and not P[1].any()
    assert (row_state.cpu().numpy()[n0:] != 2).all()
