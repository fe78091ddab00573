"""lf_mkd_tree_poses_device and lf_mkd_global_positions_device on the GPU, every output compared as words against the host
twin (tests/cpp/positions_twin.cpp: the kernels' own csrc/mkd_positions_math.h compiled by g++; tests/test_positions_twin.py
ties the twin to the definitions of include/lf_mkd.h and to the truth): the four scenes with no tolerance and with sentinels
around every output, in place, the host form, the tensor wrappers, a captured graph replayed twice, one handle over calls of
different sizes, and the plan."""
import numpy as np
import pytest

import fundamental_twin
import positions_cases as cases
import positions_twin as pt

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
KEYS = ("poses", "points", "obs_state", "image_stats", "trace", "counts")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("positions_twin")
    return tmp, pt.build(tmp), fundamental_twin.build(tmp)


@pytest.fixture(scope="module")
def twin(programs):
    tmp, exe, _ = programs
    return lambda scene, **kw: pt.run(exe, tmp, scene, **kw)


@pytest.fixture(scope="module")
def scenes(programs):
    tmp, _, f_exe = programs

    def verify(e, ka, kb, match, n_hyp, thr, seed):
        r = fundamental_twin.verify(f_exe, tmp, ka, kb, match, n_hyp, thr, seed)
        return r["F"].reshape(9), r["verified"], r["stats"]
    return dict(A=cases.scene_a(), B=cases.scene_b(), C=cases.scene_c(), D=cases.scene_d(verify))


@pytest.fixture(scope="module")
def want(scenes, twin):
    """the twin on every scene under the default parameters: computed once, not changed"""
    return {k: twin(s) for k, s in scenes.items()}


class Device:
    """a scene on the device: the arrays hold exactly what their lengths say; every output between sentinels"""

    def __init__(self, torch, handle, s):
        self.torch, self.handle = torch, handle
        kps, ioff, toff, row, img, tc, rt, K, P = pt.arrays(s)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.kps, self.ioff, self.toff = up(kps), up(ioff.view(np.int64)), up(toff.view(np.int64))
        self.row, self.img, self.tc, self.rt = up(row), up(img.view(np.int32)), up(tc.view(np.int32)), up(rt)
        self.K, self.P = up(K), up(P)
        self.n, self.n_rows, self.tcap, self.ocap = len(K), len(kps), len(toff) - 1, len(row)

    def words(self, sweeps):
        return dict(poses=12 * self.n, points=4 * self.tcap, obs_state=self.ocap, image_stats=4 * self.n, trace=8 * sweeps, counts=8)

    def buffers(self, sweeps):
        # (an even number of sentinel words in front keeps the trace 8-byte aligned)
        return {k: self.torch.full((n + 2 * EXTRA + 2,), pt.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.words(sweeps).items()}

    def run(self, bufs, stream=None, points=True, state=True, trace=True, in_place=False, **kw):
        p = {**pt.DEFAULTS, **kw}
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * (EXTRA + 1)
        if in_place:
            bufs["poses"][EXTRA + 1:EXTRA + 1 + 12 * self.n] = self.P.reshape(-1).view(self.torch.int32)
        self.handle.global_positions_device(
            ptr(self.kps), self.ioff.data_ptr(), self.n, self.n_rows, self.toff.data_ptr(), self.tcap, ptr(self.row), ptr(self.img),
            self.ocap, self.tc.data_ptr(), ptr(self.rt), ptr(self.K), out("poses") if in_place else ptr(self.P), out("poses"),
            out("image_stats"), out("counts"), out("points") if points else None, out("obs_state") if state else None,
            out("trace") if trace else None, p["sweeps"], p["warm"], p["robust_deg"], p["min_obs"], 0,
            self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs, sweeps):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.words(sweeps).items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA + 1] == pt.FILL).all() and (raw[EXTRA + 1 + n:] == pt.FILL).all(), "a write outside d_" + k
            res[k] = raw[EXTRA + 1:EXTRA + 1 + n]
        return res

    def call(self, **kw):
        sweeps = kw.get("sweeps", pt.DEFAULTS["sweeps"])
        bufs = self.buffers(sweeps)
        self.torch.cuda.synchronize()
        self.run(bufs, **kw)
        self.torch.cuda.synchronize()
        return self.read(bufs, sweeps)


def flat(w):
    """the twin's outputs as the device's frames hold them: uint32 words"""
    return {k: np.ascontiguousarray(w[k]).reshape(-1).view(np.uint32) for k in KEYS}


def same(got, want, what, keys=KEYS):
    want = flat(want)
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), [hex(got[k][b]) for b in bad[:5]], [hex(want[k][b]) for b in bad[:5]])


@pytest.mark.parametrize("which", "ABCD")
def test_the_device_equals_the_twin_in_every_word(torch, handle, scenes, want, which):
    """no tolerance; the sentinels around every output survive (Device.read), and what the call does not define -- the points
    behind T and the states outside every track -- keeps the fill pattern, as in the twin"""
    s = scenes[which]
    got = Device(torch, handle, s).call()
    same(got, want[which], which)
    T, O = int(s["counts"][0]), int(s["counts"][1])
    assert (got["points"][4 * T:] == pt.FILL).all() and (got["obs_state"][O:] == pt.FILL).all()
    assert got["counts"][1] > 0.9 * T and got["counts"][0] == len(s["intrinsics"])


@pytest.mark.parametrize("kw", (dict(sweeps=0), dict(sweeps=1, warm=0), dict(sweeps=7, warm=50), dict(sweeps=12, min_obs=4, robust_deg=1.0)))
def test_other_parameters_and_the_optional_outputs(torch, handle, scenes, twin, kw):
    s = scenes["B"]
    same(Device(torch, handle, s).call(**kw), twin(s, **kw), str(kw))
    got = Device(torch, handle, s).call(points=False, state=False, trace=False, **kw)
    assert all((got[k] == pt.FILL).all() for k in ("points", "obs_state", "trace"))
    same(got, twin(s, **kw), "without the optional outputs", keys=("poses", "image_stats", "counts"))


def test_unregistered_and_broken_inputs(torch, handle, scenes, twin):
    """an all-zero pose, NaN intrinsics, NaN keypoints, rows and images out of range: whatever is broken takes no part"""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scenes["A"].items()}
    s["poses"][2] = 0
    s["intrinsics"][4, 1] = np.nan
    O = int(s["counts"][1])
    s["kps"][s["obs_row"][5], 0] = np.nan
    s["obs_row"][9], s["obs_row"][10], s["obs_image"][11] = -3, len(s["kps"]) + 2, 77
    s["row_track"][s["obs_row"][20]] = int(s["counts"][0]) + 9
    got = Device(torch, handle, s).call()
    same(got, twin(s), "broken")
    assert got["counts"][0] == 4 and (got["poses"].reshape(-1, 12)[[2, 4]] == 0).all() and O > 20


def test_in_place_equals_out_of_place(torch, handle, scenes, want):
    same(Device(torch, handle, scenes["C"]).call(in_place=True), want["C"], "in place")


def test_the_host_form_and_the_wrappers_equal_the_device_form(torch, handle, scenes, want):
    s, w = scenes["D"], flat(want["D"])
    kps, ioff, toff, row, img, tc, rt, K, P = pt.arrays(s)
    T, O = int(tc[0]), int(tc[1])
    poses, points, state, ims, trace, counts = handle.global_positions(kps, ioff, toff[:T + 1], row[:O], img[:O], rt, K, P, **pt.DEFAULTS)
    assert np.array_equal(poses.view(np.uint32).reshape(-1), w["poses"]) and np.array_equal(ims.reshape(-1), w["image_stats"])
    assert np.array_equal(points.view(np.uint32).reshape(-1), w["points"][:4 * T]) and np.array_equal(counts, w["counts"])
    assert np.array_equal(trace.view(np.uint32).reshape(-1), w["trace"])
    expect = np.where(w["obs_state"][:O] == pt.FILL, 0, w["obs_state"][:O])         # the host form returns 0 outside every track
    assert np.array_equal(state, expect)
    # the wrapper, on tensors
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table = (up(toff.view(np.int64)), up(row), up(img.view(np.int32)), up(rt), up(tc.view(np.int32)))
    got = lf.global_positions(up(kps), up(ioff.view(np.int64)), table, up(K), up(P), trace=True, **pt.DEFAULTS)
    torch.cuda.synchronize()
    for t, name in zip(got, KEYS):
        a = t.cpu().numpy().reshape(-1).view(np.uint32)
        if name == "obs_state":
            a, ref = a[:O], np.where(w[name][:O] == pt.FILL, 0xFFFFFFFF, w[name][:O])
        elif name == "points":
            a, ref = a[:4 * T], w[name][:4 * T]
        else:
            ref = w[name]
        assert np.array_equal(a, ref), name


def test_a_captured_graph_replayed_twice(torch, handle, scenes, want):
    s = scenes["A"]
    D = Device(torch, handle, s)
    same(D.call(), want["A"], "warm-up")
    sweeps = pt.DEFAULTS["sweeps"]
    bufs = D.buffers(sweeps)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for k in range(2):
        for v in bufs.values():
            v.fill_(pt.FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(D.read(bufs, sweeps), want["A"], "replay %d" % k)


def test_one_handle_over_c_a_c(torch, scenes, want):
    """the scratch grows for C and is reused, larger than needed, by A: the third run is the first"""
    h = lfp.MkdHandle(max_features=64)
    first = None
    for which in "CAC":
        got = Device(torch, h, scenes[which]).call()
        same(got, want[which], which)
        if which == "C":
            first = first or got
            assert all(got[k].tobytes() == first[k].tobytes() for k in got)
    h.close()


def test_the_plan_is_what_the_call_does(scenes):
    """the launches by the header's rule (the entry point counts its launches and fails a call that issues another number: every
    call above passed that check), and the scratch"""
    s = scenes["C"]
    n, tcap = len(s["intrinsics"]), len(s["track_offsets"]) - 1
    for sweeps in (0, 1, 50):
        launches, scratch = lfp.global_positions_plan(n, tcap, sweeps)
        assert launches == 4 + 3 * sweeps
        assert 24 * n + 24 * tcap + 36 * n + 12 * n + 4 * tcap + 16 <= scratch <= 24 * n + 24 * tcap + 36 * n + 12 * n + 4 * tcap + 16 + 8 * 16
    assert lfp.global_positions_plan(0, 100, 5) == (0, 0)


# ---- tree poses ---------------------------------------------------------------------------------------------------------------
def test_tree_poses_equal_the_twin_in_every_word(torch, handle, programs):
    tmp, exe, _ = programs
    scenes = [cases.tree_scene(), cases.tree_scene(seed=9, n=300, flip=tuple(range(2, 300, 3)))]
    broken = cases.tree_scene(seed=10)
    broken["image_stats"][3, 1] = pt.NONE                                   # images 3 .. 6 lose their chain
    broken["t"][0, 1] = np.nan                                              # and images 1, 2 their first edge
    scenes.append(broken)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    for k, s in enumerate(scenes):
        for depth in (64, 2) if k == 0 else (512,):
            ea, eb, t, rot, st = pt.tree_arrays(s)
            n = len(rot)
            buf = torch.full((12 * n + 2 * EXTRA,), pt.FILL, dtype=torch.int32, device="cuda")
            d = [up(ea.view(np.int32)), up(eb.view(np.int32)), up(t), up(rot), up(st.view(np.int32))]
            handle.tree_poses_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(ea), d[3].data_ptr(), d[4].data_ptr(), n,
                                     buf.data_ptr() + 4 * EXTRA, depth, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            raw = buf.cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA] == pt.FILL).all() and (raw[EXTRA + 12 * n:] == pt.FILL).all()
            expect = pt.run_tree(exe, tmp, s, depth)
            assert np.array_equal(raw[EXTRA:EXTRA + 12 * n].reshape(n, 12), expect), (k, depth)
            assert np.array_equal(handle.tree_poses(ea, eb, t, rot, st, depth).view(np.uint32), expect), "the host form"
            lf = lfp.LocalFeatures(64, 64, 16)
            got = lf.tree_poses((d[0], d[1]), d[2], d[3], d[4], max_depth=depth)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint32), expect), "the wrapper"
    assert (expect[3:7] == 0).all() and (expect[1:3] == 0).all() and expect[0].any()


def test_match_collection_with_the_global_route(torch):
    """match_collection(..., pose=.., view_graph=3.0, global_sweeps=50, bundle=4) on the example's frames (the houses crop, its
    warp, a second warp and the bird), all pairs: the three related images come out with finite poses (the frames are warps
    of one picture, so the geometry means little; this is about the plumbing)"""
    import os
    import sys
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    n = len(frames)
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=n)
    got = ex.match_collection(frames, "all", seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), tracks=True, view_graph=3.0,
                              global_sweeps=50, bundle=4)
    torch.cuda.synchronize()
    poses, counts, ims = got["tri_poses"].cpu().numpy(), got["gp_counts"].cpu().numpy(), got["gp_image_stats"].cpu().numpy()
    labelled = got["vg_image_stats"].cpu().numpy()[:, 1] != -1
    assert poses.shape == (n, 12) and np.isfinite(poses).all() and counts[7] == 50
    assert ((poses[:, :9] != 0).any(1) == labelled).all() and counts[0] == labelled.sum()      # a pose for every labelled image
    assert (ims[labelled, 3] != 1).all() and (ims[~labelled] == [0, 0, 0, 1]).all() and (poses[~labelled] == 0).all()
    assert got["bundle_trace"].shape == (4, 8) and np.isfinite(got["bundle_rms"].cpu().numpy()).all()
    lines = ex.global_lines(got)
    assert len(lines) == 1 and lines[0].startswith("global positions, 50 sweeps: %d images" % counts[0])
    plain = ex.match_collection(frames[:3], "all", seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), tracks=True)
    assert plain["gp_counts"] is None and ex.global_lines(plain) == []
    with pytest.raises(RuntimeError, match="needs view_graph"):
        ex.match_collection(frames[:3], "all", seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), global_sweeps=5)
