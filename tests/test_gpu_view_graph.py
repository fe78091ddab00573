"""lf_mkd_view_graph_device on the GPU, every output compared as uint32 words against the host twin
(tests/cpp/view_graph_twin.cpp: the kernels' own csrc/mkd_view_graph_math.h compiled by g++; tests/test_view_graph_twin.py ties
the twin to the definitions of include/lf_mkd.h and to the truth): the four scenes with no tolerance and with sentinels around
every output, the flag and other parameters, a captured graph replayed three times, one handle over scenes of different sizes,
the match filter in place into build_tracks, the host form, the tensor wrapper and the plan."""
import numpy as np
import pytest

import tracks_cases
import view_graph_cases as cases
import view_graph_twin as vt

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
WIDTH = dict(vt.OUTPUTS)
SCENES = dict(A=cases.scene_a, B=cases.scene_b, C=cases.scene_c, D=cases.scene_d)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def scenes():
    return {k: make() for k, make in SCENES.items()}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("view_graph_twin")
    exe = vt.build(tmp)
    return lambda scene, **kw: vt.run(exe, tmp, scene, **kw)


@pytest.fixture(scope="module")
def want(scenes, twin):
    """the twin on every scene under its own parameters: computed once, not changed"""
    return {k: twin(s, **s["params"]) for k, s in scenes.items()}


class Device:
    """a scene on the device: the arrays hold exactly what their lengths say; every output between sentinels"""

    def __init__(self, torch, handle, s):
        self.torch, self.handle = torch, handle
        ea, eb, R, ps, off, m = vt.arrays(s)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.ea, self.eb, self.R, self.ps = up(ea.view(np.int32)), up(eb.view(np.int32)), up(R), up(ps.view(np.int32))
        self.off, self.match = (up(off.view(np.int64)), up(m)) if m is not None else (None, None)
        self.n_images, self.n_edges = int(s["n_images"]), len(ea)
        self.rows = vt.rows(s)

    def buffers(self):
        return {k: self.torch.full((WIDTH[k] * n + 2 * EXTRA,), vt.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.rows.items()}

    def run(self, bufs, stream=None, match=True, residual=True, **kw):
        p = {**vt.DEFAULTS, **kw}
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * EXTRA
        filt = match and self.match is not None
        self.handle.view_graph_device(
            ptr(self.ea), ptr(self.eb), self.n_edges, ptr(self.R), ptr(self.ps), self.n_images, out("rotations"), out("edge_stats"),
            out("image_stats"), out("counts"), out("residual") if residual else None, self.off.data_ptr() if filt else None,
            self.match.numel() if filt else 0, self.match.data_ptr() if filt else None,
            (self.match.data_ptr() if match == "in place" else out("match_out")) if filt else None, p["deg"], p["min_front"], p["root"],
            p["tree_rounds"], p["iterations"], p["flags"], self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.rows.items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA] == vt.FILL).all() and (raw[EXTRA + WIDTH[k] * n:] == vt.FILL).all(), "a write outside d_" + k
            res[k] = raw[EXTRA:EXTRA + WIDTH[k] * n].reshape((n, WIDTH[k]) if WIDTH[k] > 1 and k != "counts" else (WIDTH[k] * n,))
        return res

    def call(self, **kw):
        bufs = self.buffers()
        self.torch.cuda.synchronize()
        self.run(bufs, **kw)
        self.torch.cuda.synchronize()
        return self.read(bufs)


def same(got, want, what, keys=tuple(k for k, _ in vt.OUTPUTS)):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), [hex(got[k][tuple(b)]) for b in bad[:5]],
                               [hex(want[k][tuple(b)]) for b in bad[:5]])


@pytest.mark.parametrize("which", sorted(SCENES))
def test_the_device_equals_the_twin_in_every_word(torch, handle, scenes, want, which):
    """no tolerance; the sentinels around every output survive (Device.read), and what the call does not define -- the match
    entries of no edge -- keeps the fill pattern, as in the twin"""
    s = scenes[which]
    got = Device(torch, handle, s).call(**s["params"])
    same(got, want[which], which)
    off = s["edge_offsets"].astype(np.int64)
    assert (got["match_out"][:off[0]] == vt.FILL).all() and (got["match_out"][off[-1]:] == vt.FILL).all()
    assert got["counts"][0] > 0 and (got["image_stats"][:, 1] != vt.NONE).sum() == got["counts"][5]


@pytest.mark.parametrize("kw", (dict(flags=cases.USE_UNCHECKED), dict(tree_rounds=0), dict(iterations=0), dict(iterations=1, root=3),
                                dict(deg=0.0), dict(min_front=150, tree_rounds=3)))
def test_other_parameters_and_the_optional_outputs(torch, handle, scenes, twin, kw):
    s = scenes["D"] if "flags" in kw else scenes["A"]
    kw = {**s["params"], **kw}
    same(Device(torch, handle, s).call(**kw), twin(s, **kw), str(kw))
    got = Device(torch, handle, s).call(match=False, residual=False, **kw)
    assert (got["residual"] == vt.FILL).all() and (got["match_out"] == vt.FILL).all()
    same(got, twin(s, **kw), "without the optional outputs", keys=("rotations", "edge_stats", "image_stats", "counts"))


def test_degenerate_shapes(torch, handle, scenes, twin):
    s = scenes["A"]
    empty = dict(s, edge_a=s["edge_a"][:0], edge_b=s["edge_b"][:0], R=s["R"][:0], pose_stats=s["pose_stats"][:0],
                 edge_offsets=s["edge_offsets"][:1])
    for scene, kw in ((empty, {}), (empty, dict(root=7)), (dict(empty, n_images=1), {}), (dict(s, n_images=1), {})):
        same(Device(torch, handle, scene).call(**kw), twin(scene, **kw), "%d images, %d edges, %s" % (scene["n_images"], len(scene["edge_a"]), kw))
    # n_images == 0: LF_MKD_OK, nothing written (null pointers everywhere)
    handle.view_graph_device(None, None, 0, None, None, 0, None, None, None, None)
    got = Device(torch, handle, dict(empty, n_images=0)).call()
    assert all((v == vt.FILL).all() for v in got.values())


def test_a_captured_graph_replayed_three_times(torch, handle, scenes, want):
    s = scenes["B"]
    D = Device(torch, handle, s)
    same(D.call(), want["B"], "warm-up")
    bufs = D.buffers()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for k in range(3):
        for v in bufs.values():
            v.fill_(vt.FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(D.read(bufs), want["B"], "replay %d" % k)


def test_one_handle_over_c_a_d_a(torch, scenes, want):
    """the scratch grows for C and is reused, larger than needed, by A, D and A again: the last run is the first"""
    h = lfp.MkdHandle(max_features=64)
    first = None
    for which in "AC" "ADA":
        s = scenes[which]
        got = Device(torch, h, s).call(**s["params"])
        same(got, want[which], which)
        if which == "A":
            first = first or got
            assert all(got[k].tobytes() == first[k].tobytes() for k in got)
    h.close()


def test_the_filter_in_place_then_build_tracks(torch, handle, scenes, want):
    """the filtered match array is lf_mkd_build_tracks_device's input: a pool of 40 rows per image, the scene's layout and
    matches (an entry is a link iff 0 <= j < 40), against the host composition"""
    s = scenes["B"]
    n_images, rows = s["n_images"], 40
    img_off = np.arange(n_images + 1, dtype=np.int64) * rows
    D = Device(torch, handle, s)
    bufs = D.buffers()
    D.run(bufs, match="in place")
    torch.cuda.synchronize()
    got = D.read(bufs)
    assert (got["match_out"] == vt.FILL).all()
    kept = D.match.cpu().numpy()
    off = s["edge_offsets"].astype(np.int64)
    expect = s["match"].copy()
    expect[off[0]:off[-1]] = want["B"]["match_out"][off[0]:off[-1]].view(np.int32)
    assert np.array_equal(kept, expect)
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    track, length, dup = lf.build_tracks(up(img_off), up(s["edge_a"].view(np.int32)), up(s["edge_b"].view(np.int32)), D.off, D.match,
                                         n_rows=n_images * rows)
    torch.cuda.synchronize()
    t, l, d = tracks_cases.build_tracks(img_off, n_images * rows, s["edge_a"], s["edge_b"], off, len(expect), expect)
    assert np.array_equal(track.cpu().numpy(), t) and np.array_equal(length.cpu().numpy().view(np.uint32), l)
    assert np.array_equal(dup.cpu().numpy().view(np.uint32), d) and (l > 1).sum() > 50


def test_the_host_form_and_the_wrapper_equal_the_device_form(torch, handle, scenes, want):
    s = scenes["D"]
    ea, eb, R, ps, off, m = vt.arrays(s)
    w = want["D"]
    rot, es, res, ims, counts, out = handle.view_graph(ea, eb, R, ps, s["n_images"], edge_offsets_a=off, match=m, **{
        "max_loop_deg": 3.0, "min_front": cases.D_MIN_FRONT})
    expect = np.where(w["match_out"] == vt.FILL, m.view(np.uint32), w["match_out"])      # the host form returns match elsewhere
    for got, name in ((rot, "rotations"), (es, "edge_stats"), (res, "residual"), (ims, "image_stats"), (counts, "counts")):
        assert np.array_equal(got.view(np.uint32).reshape(w[name].shape), w[name]), name
    assert np.array_equal(out.view(np.uint32), expect)
    rot2, es2, none, ims2, counts2, none2 = handle.view_graph(ea, eb, R, ps, s["n_images"], min_front=cases.D_MIN_FRONT, residual=False)
    assert none is None and none2 is None and np.array_equal(rot2, rot) and np.array_equal(es2, es) and np.array_equal(counts2, counts)
    # the wrapper, on tensors
    lf = lfp.LocalFeatures(64, 64, 16)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = lf.view_graph((up(ea.view(np.int32)), up(eb.view(np.int32))), up(R), up(ps.view(np.int32)), s["n_images"],
                        min_front=cases.D_MIN_FRONT, layout=up(off.view(np.int64)), match=up(m))
    torch.cuda.synchronize()
    for t, name in zip(got[:5], ("rotations", "edge_stats", "residual", "image_stats", "counts")):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(w[name].shape), w[name]), name
    assert np.array_equal(got[5].cpu().numpy().view(np.uint32), expect)


def test_match_collection_with_view_graph(torch):
    """match_collection(..., pose=.., view_graph=3.0) on the example's frames, all pairs: it runs, reports its counts, filters
    the matches the tracks are built from and chooses no unsupported initial pair (the frames are warps of one picture, so the
    geometry means little; this is about the plumbing)"""
    import os
    import sys
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()[:3]])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "all", seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), tracks=True, view_graph=3.0)
    torch.cuda.synchronize()
    counts, es = got["vg_counts"].cpu().numpy(), got["vg_edge_stats"].cpu().numpy()
    posed = got["pose_stats"].cpu().numpy()[:, 2] >= 0
    assert es.shape == (3, 4) and counts[0] == posed.sum() and counts[1] + counts[2] + counts[3] == counts[0]
    assert (es[~posed, 2] == 0).all() and (es[posed, 0] == (1 if posed.all() else 0)).all()
    assert got["vg_rotations"].shape == (3, 3, 3) and got["vg_image_stats"].shape == (3, 4) and got["vg_residual"].shape == (3,)
    la, ver, kept = got["layout_a"].cpu().numpy(), got["verified"].cpu().numpy(), got["vg_match"].cpu().numpy()
    for e in range(3):
        want = ver[la[e]:la[e + 1]] if es[e, 2] == 3 else np.full(la[e + 1] - la[e], -1, np.int32)
        assert np.array_equal(kept[la[e]:la[e + 1]], want), e
    assert np.array_equal(kept[la[3]:], ver[la[3]:])
    lines = ex.view_graph_lines(got)
    assert len(lines) == 1 and lines[0].startswith("%d usable edges" % counts[0])
    plain = ex.match_collection(frames, "all", seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0), tracks=True)
    assert plain["vg_counts"] is None and plain["vg_match"] is None and ex.view_graph_lines(plain) == []
    if counts[4] == counts[0] == 3:                                           # every edge kept: the tracks are the plain run's
        assert torch.equal(plain["track"], got["track"])


def test_the_plan_is_what_the_call_does(scenes):
    """the launches by the header's rule for the shapes the tests above run, as the siblings' plans are checked (a call whose
    launches read a layout another count would have made does not survive the word-for-word comparisons), and the scratch"""
    for which, filt in (("C", True), ("A", False)):
        s = scenes[which]
        n, E = s["n_images"], len(s["edge_a"])
        T, I = s["params"].get("tree_rounds", vt.DEFAULTS["tree_rounds"]), vt.DEFAULTS["iterations"]
        launches, scratch, form = lfp.view_graph_plan(n, E, T, I, with_match=filt)
        assert launches == 1 + 2 + 1 + T + I + 1 + filt and form == 0
        assert scratch == 32 * E + 2 * 32 * n + 4 * n * n
