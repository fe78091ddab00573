"""lf_mkd_two_view_pose_device on the GPU, every output compared as uint32 words against the host twin
(tests/cpp/pose_twin.cpp: the kernel's own csrc/mkd_pose_math.h compiled by g++; tests/test_pose_twin.py ties the twin to the
algorithm of include/lf_mkd.h): the five families in one call of 48 edges, edges of 0 .. 1500 links, every no-pose cause,
rows outside the pool, a NaN keypoint, offsets beyond link_capacity and an inverted range, NULL d_sigma / d_points, an edge's
position in a batch, graph capture, the chain verify_fundamental -> link_table -> pose, and the host form."""
import numpy as np
import pytest

import pose_cases as pc
import pose_twin as pt

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind every output
DEG = 2.0
WIDTH = {"R": 9, "t": 3, "stats": 4, "sigma": 3, "points": 4}


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
    tmp = tmp_path_factory.mktemp("pose_twin")
    exe = pt.build(tmp)
    return lambda table, deg=DEG: pt.run(exe, tmp, table, deg)


def bits32(x):
    return np.ascontiguousarray(x).view(np.int32) if np.asarray(x).dtype.itemsize == 4 else np.asarray(x).astype(np.int32)


class Device:
    """a table on the device: the arrays hold exactly what the counts say, so a read beyond them leaves the allocation's used
    part; every output between sentinels"""

    def __init__(self, torch, handle, t):
        self.torch, self.handle = torch, handle
        self.cap = int(t.get("link_capacity", len(t["link_a"])))
        self.n_edges, self.n_images, self.n_rows = len(t["edge_a"]), len(t["intrinsics"]), len(t["kps"])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        self.kps = up(t["kps"].astype(np.float32).reshape(-1, 5))
        self.ea, self.eb = up(bits32(t["edge_a"])), up(bits32(t["edge_b"]))
        self.intr, self.F = up(t["intrinsics"].astype(np.float32)), up(t["F"].astype(np.float32))
        self.off = up(t["link_offsets"].astype(np.uint64).view(np.int64))
        self.la, self.lb = up(t["link_a"][:self.cap].astype(np.int32)), up(t["link_b"][:self.cap].astype(np.int32))
        self.rows = {"R": self.n_edges, "t": self.n_edges, "stats": self.n_edges, "sigma": self.n_edges, "points": self.cap}

    def buffers(self):
        return {k: self.torch.full((WIDTH[k] * n + 2 * EXTRA,), pt.FILL, dtype=self.torch.int32, device="cuda")
                for k, n in self.rows.items()}

    def run(self, bufs, deg=DEG, sigma=True, points=True, stream=None):
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        out = lambda k: bufs[k].data_ptr() + 4 * EXTRA
        self.handle.two_view_pose_device(ptr(self.kps), self.n_rows, ptr(self.ea), ptr(self.eb), self.n_edges, ptr(self.intr),
                                         self.n_images, ptr(self.F), self.off.data_ptr(), ptr(self.la), ptr(self.lb), self.cap,
                                         out("R"), out("t"), out("stats"), out("sigma") if sigma else None,
                                         out("points") if points else None, deg, 0,
                                         self.torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def read(self, bufs):
        """the outputs out of their frames; the sentinels must have survived"""
        res = {}
        for k, n in self.rows.items():
            raw = bufs[k].cpu().numpy().view(np.uint32)
            assert (raw[:EXTRA] == pt.FILL).all() and (raw[EXTRA + WIDTH[k] * n:] == pt.FILL).all(), "a write outside d_" + k
            res[k] = raw[EXTRA:EXTRA + WIDTH[k] * n].reshape(n, WIDTH[k])
        return res

    def call(self, deg=DEG, sigma=True, points=True):
        bufs = self.buffers()
        self.torch.cuda.synchronize()
        self.run(bufs, deg, sigma, points)
        self.torch.cuda.synchronize()
        return self.read(bufs)


def same(got, want, what, keys=("R", "t", "stats", "sigma", "points")):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), [hex(got[k][tuple(b)]) for b in bad[:5]],
                               [hex(want[k][tuple(b)]) for b in bad[:5]])


def check(torch, handle, twin, table, what, deg=DEG):
    want = twin(table, deg)
    got = Device(torch, handle, table).call(deg)
    same(got, want, what)
    return got


def test_the_five_families_in_one_call(torch, handle, twin):
    t = pc.family_batch(48)
    got = check(torch, handle, twin, t, "families")
    st = got["stats"]
    assert (st[:, 2] < 4).all() and (st[:, 0] > st[:, 1]).all() and (st[:, 3] <= st[:, 0]).all()
    assert len({int(c) for c in st[:, 2]}) > 1                      # the Jacobi's signs differ from edge to edge
    links = np.diff(t["link_offsets"].astype(np.int64))
    assert (st[:, 0] > 0.45 * links).all()                           # up to half the matches are planted outliers
    sigma = pt.f32(got["sigma"])
    assert np.abs(sigma[:, 1] - 1).max() < 1e-5 and sigma[:, 2].max() < 1e-5   # the true F under the true intrinsics
    for e in range(48):                                              # the chosen rotation is the true one, t points the true way
        r, tr = pc.MOTIONS[pc.FAMILIES[e % 5]]
        assert pc.rotation_angle_deg(pt.f32(got["R"][e]).reshape(3, 3), r) < 1e-3
        assert float(pt.f32(got["t"][e]) @ tr) > 0
    other = check(torch, handle, twin, t, "another threshold", 0.25)  # only the parallax count depends on the threshold
    assert (other["stats"][:, 3] >= st[:, 3]).all() and (other["stats"][:, 3] > st[:, 3]).any()
    same(other, got, "another threshold", ("R", "t", "sigma", "points"))
    for deg, col in ((0.0, 0), (180.0, None)):                       # the ends of the range: every in-front link, none
        ends = check(torch, handle, twin, t, f"threshold {deg}", deg)
        assert (ends["stats"][:, 3] == (ends["stats"][:, col] if col is not None else 0)).all()


def test_edge_lengths(torch, handle, twin):
    t = pc.length_batch()
    got = check(torch, handle, twin, t, "lengths")
    assert np.diff(t["link_offsets"].astype(np.int64)).tolist() == list(pc.LENGTHS)
    assert got["stats"][0].tolist() == [0, 0, pt.NONE, 0] and not got["R"][0].any()      # no link: the best count is 0
    assert (got["stats"][1:, 2] < 4).all() and got["stats"][-1][0] > 1000


def test_every_no_pose_cause(torch, handle, twin):
    t, names = pc.no_pose_batch()
    got = check(torch, handle, twin, t, "no pose")
    off = t["link_offsets"].astype(np.int64)
    for e, name in enumerate(names):
        rows = pt.f32(got["points"][off[e]:off[e + 1]])
        if name == "ok":
            assert got["stats"][e][2] < 4 and got["stats"][e][0] > 200
        else:
            assert got["stats"][e].tolist() == [0, 0, pt.NONE, 0] and np.array_equal(rows, np.tile(pc.NONE_ROW, (len(rows), 1))), name
            assert not got["R"][e].any() and not got["t"][e].any() and not got["sigma"][e].any(), name


def test_rows_outside_the_pool_and_a_nan_keypoint(torch, handle, twin):
    t = pc.bad_rows_table()
    got = check(torch, handle, twin, t, "bad rows")
    pts = pt.f32(got["points"])
    for k in (3, 40, 7, 41, 100, 20, 21):
        assert np.array_equal(pts[k], pc.NONE_ROW), k
    assert got["stats"][0][0] == (pts[:int(t["link_offsets"][1]), 3] != 2.0).sum()


def test_offsets_beyond_the_capacity_and_an_inverted_range(torch, handle, twin):
    t = pc.odd_offsets_table()
    got = check(torch, handle, twin, t, "odd offsets")
    assert got["stats"][2].tolist() == [0, 0, pt.NONE, 0] and not (got["points"] == pt.FILL).any()
    empty = dict(t, link_offsets=np.array([7, 7, 7, 3], np.uint64))
    got = check(torch, handle, twin, empty, "no range at all")
    assert (got["points"] == pt.FILL).all()                          # entries outside every range are untouched


def test_null_sigma_and_points(torch, handle, twin):
    t = pc.family_batch(12, seed=3)
    want = twin(t)
    D = Device(torch, handle, t)
    for sigma, points in ((False, True), (True, False), (False, False)):
        got = D.call(DEG, sigma, points)
        same(got, want, (sigma, points), ("R", "t", "stats") + (("sigma",) if sigma else ()) + (("points",) if points else ()))
        assert sigma or (got["sigma"] == pt.FILL).all()
        assert points or (got["points"] == pt.FILL).all()


def test_an_edge_alone_equals_the_edge_in_a_batch(torch, handle, twin):
    t = pc.family_batch(48)
    whole = Device(torch, handle, t).call()
    off = t["link_offsets"].astype(np.int64)
    for e in (0, 7, 23, 47):
        one = Device(torch, handle, pc.edge_table(t, e)).call()
        for k in ("R", "t", "stats", "sigma"):
            assert np.array_equal(one[k][0], whole[k][e]), (e, k)
        assert np.array_equal(one["points"][off[e]:off[e + 1]], whole["points"][off[e]:off[e + 1]]), e
        rest = np.delete(one["points"], np.s_[off[e]:off[e + 1]], axis=0)
        assert (rest == pt.FILL).all(), e


def test_two_runs_and_capture(torch, handle, twin):
    first, later = pc.family_batch(16, seed=5), pc.family_batch(16, seed=6)
    D = Device(torch, handle, first)
    a, b = D.call(), D.call()
    same(a, twin(first), "first run")
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    bufs = D.buffers()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.run(bufs, stream=torch.cuda.current_stream().cuda_stream)
    for v in bufs.values():
        v.fill_(pt.FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(D.read(bufs), a, "replay")
    # new inputs in the same arrays (the later table is cut or padded to the first one's sizes)
    L = Device(torch, handle, later)
    n = min(D.cap, L.cap)
    off = np.minimum(later["link_offsets"].astype(np.int64), n)
    cut = dict(later, link_offsets=off.astype(np.uint64), link_a=later["link_a"][:n], link_b=later["link_b"][:n],
               kps=later["kps"][:D.n_rows] if len(later["kps"]) >= D.n_rows else
               np.concatenate([later["kps"], np.zeros((D.n_rows - len(later["kps"]), 5), np.float32)]))
    cut["link_capacity"] = n
    D.off.copy_(torch.from_numpy(off))
    D.la[:n].copy_(L.la[:n])
    D.lb[:n].copy_(L.lb[:n])
    D.kps.copy_(torch.from_numpy(cut["kps"]).cuda())
    D.F.copy_(L.F)
    D.intr.copy_(L.intr)
    for v in bufs.values():
        v.fill_(pt.FILL)
    g.replay()
    torch.cuda.synchronize()
    got, want = D.read(bufs), twin(cut)
    same(got, want, "replay on new inputs", ("R", "t", "stats", "sigma"))
    assert np.array_equal(got["points"][:n], want["points"])


@pytest.mark.parametrize("family", ("general", "sideways", "forward"))   # (a near-planar scene leaves F underdetermined)
def test_chain_from_matches_to_a_pose(family, torch, handle, twin):
    """two_view keypoints -> verify_fundamental_device -> link_table_device -> the pose, on one pool of two images; the result
    is the twin's on the same device-produced F and links, and the rotation is the nearer of the twisted pair to the truth."""
    ka, kb, mt = pc.problem(600, 0.3, 9, family)
    na, nb = len(ka), len(kb)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pool = up(np.concatenate([ka, kb]))
    img_off, off_a, off_b = up(np.array([0, na, na + nb], np.int64)), up(np.array([0, na], np.int64)), up(np.array([0, nb], np.int64))
    match = up(mt)
    F = torch.empty(9, dtype=torch.float32, device="cuda")
    ver = torch.empty(na, dtype=torch.int32, device="cuda")
    vst = torch.empty(4, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    handle.verify_fundamental_device(pool.data_ptr(), off_a.data_ptr(), pool.data_ptr() + 20 * na, off_b.data_ptr(), match.data_ptr(),
                                     1, F.data_ptr(), ver.data_ptr(), vst.data_ptr(), 512, 1.5, 17, 0, s)
    ea, eb = up(np.array([0], np.int32)), up(np.array([1], np.int32))
    l_off = torch.empty(2, dtype=torch.int64, device="cuda")
    la, lb = torch.full((na,), -1, dtype=torch.int32, device="cuda"), torch.full((na,), -1, dtype=torch.int32, device="cuda")
    counts = torch.empty(4, dtype=torch.int32, device="cuda")
    handle.link_table_device(img_off.data_ptr(), 2, na + nb, ea.data_ptr(), eb.data_ptr(), off_a.data_ptr(), na, 1, ver.data_ptr(), 0,
                             0, na, l_off.data_ptr(), la.data_ptr(), lb.data_ptr(), None, None, None, counts.data_ptr(), s)
    torch.cuda.synchronize()
    table = {"kps": pool.cpu().numpy(), "edge_a": np.array([0], np.uint32), "edge_b": np.array([1], np.uint32),
             "intrinsics": np.tile(pc.K4, (2, 1)), "F": F.cpu().numpy().reshape(1, 9),
             "link_offsets": l_off.cpu().numpy().view(np.uint64), "link_a": la.cpu().numpy(), "link_b": lb.cpu().numpy()}
    n_links = int(table["link_offsets"][1])
    assert n_links == int(vst.cpu()[0]) and n_links > 300
    got = check(torch, handle, twin, table, "chain")
    R, t = pt.f32(got["R"][0]).reshape(3, 3).astype(np.float64), pt.f32(got["t"][0]).astype(np.float64)
    r_true, t_true = pc.MOTIONS[family]
    other = (2 * np.outer(t, t) - np.eye(3)) @ R                     # the other twisted rotation: half a turn about t more
    assert got["stats"][0][2] < 4 and got["stats"][0][0] > 0.9 * n_links
    assert pc.rotation_angle_deg(R, r_true) < pc.rotation_angle_deg(other, r_true)
    assert float(t @ t_true) > 0
    print(f"{family}: {n_links} links, front {got['stats'][0][0]}, parallax {got['stats'][0][3]}, rotation error "
          f"{pc.rotation_angle_deg(R, r_true):.3f} deg, sigma {pt.f32(got['sigma'][0])}")


def test_the_host_form_equals_the_device_form(torch, handle, twin):
    ka, kb, mt = pc.problem(500, 0.2, 13, "general")
    mt = mt.copy()
    mt[::7], mt[5] = -1, len(kb) + 2
    t = pc.make_table([(ka, kb, mt)], [pc.f_true(*pc.MOTIONS["general"])])
    want = Device(torch, handle, t).call()
    R, tt, st, sg, pts = handle.two_view_pose(t["F"][0], pc.K4, pc.K4, ka, kb, mt, DEG)
    assert np.array_equal(R.reshape(-1).view(np.uint32), want["R"][0]) and np.array_equal(tt.view(np.uint32), want["t"][0])
    assert np.array_equal(st, want["stats"][0]) and np.array_equal(sg.view(np.uint32), want["sigma"][0])
    rows = np.flatnonzero((mt >= 0) & (mt < len(kb)))
    full = np.tile(pc.NONE_ROW, (len(ka), 1))
    full[rows] = pt.f32(want["points"])
    assert pts.shape == (len(ka), 4) and np.array_equal(pts.view(np.uint32), full.view(np.uint32))
    assert st[2] < 4 and st[0] > 300
    R2, t2, st2, sg2, none = handle.two_view_pose(t["F"][0], pc.K4, pc.K4, ka, kb, mt, DEG, points=False)
    assert none is None and np.array_equal(R2, R) and np.array_equal(st2, st)
    # the wrapper: one pair as host arrays, and the same edge as tensors
    lf = lfp.LocalFeatures(64, 64, 16)
    R3, t3, st3, sg3, p3 = lf.two_view_pose(t["F"][0].reshape(3, 3), (pc.K4, pc.K4), (ka[:, :4], kb[:, :4]),
                                            links=[(int(i), int(mt[i])) for i in rows], min_parallax_deg=DEG)
    assert np.array_equal(R3, R) and np.array_equal(t3, tt) and st3.tolist() == st.astype(np.int64).tolist()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = lf.two_view_pose(up(t["F"]), up(t["intrinsics"]), up(t["kps"]), (up(bits32(t["edge_a"])), up(bits32(t["edge_b"]))),
                           (up(t["link_offsets"].view(np.int64)), up(t["link_a"]), up(t["link_b"])), DEG)
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().reshape(-1).view(np.uint32), want["R"][0])
    assert np.array_equal(out[2].cpu().numpy().view(np.uint32), want["stats"])
    assert np.array_equal(out[4].cpu().numpy().view(np.uint32), want["points"])


# --- the examples ----------------------------------------------------------------------------------------------------------
def _frames():
    """the 1024 x 768 centre crop of houses.jpg and two perspective warps of it (PIL images)"""
    from test_gpu_covisibility import _frames as four
    return four()[:3]


def test_match_collection_with_pose(torch, twin):
    """match_collection(frames, "window", 1, fundamental=True, pose=...): the pose outputs are the twin's on the F, the link
    table and the keypoints the same run left on the device.  (The frames are warps of one picture -- one plane -- so F and the
    pose carry no geometry; this is about the plumbing.)"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import match_collection as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    got = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pose=(800.0, 512.0, 384.0))
    plain = ex.match_collection(frames, "window", 1, seed=21, feats=feats, fundamental=True, pairs=True)
    torch.cuda.synchronize()
    table = {"kps": got["keypoints"].cpu().numpy(), "edge_a": got["edge_a"].cpu().numpy().view(np.uint32),
             "edge_b": got["edge_b"].cpu().numpy().view(np.uint32), "intrinsics": np.tile(np.array([800, 800, 512, 384], np.float32), (3, 1)),
             "F": got["model"].cpu().numpy().reshape(-1, 9), "link_offsets": got["link_offsets"].cpu().numpy().view(np.uint64),
             "link_a": got["link_a"].cpu().numpy(), "link_b": got["link_b"].cpu().numpy()}
    want = twin(table, 1.0)
    n_links = int(table["link_offsets"][-1])
    assert len(table["edge_a"]) == 2 and n_links > 200
    for key, name in (("R", "pose_R"), ("t", "pose_t"), ("stats", "pose_stats"), ("sigma", "pose_sigma")):
        assert np.array_equal(got[name].cpu().numpy().reshape(len(want[key]), -1).view(np.uint32), want[key]), name
    assert np.array_equal(got["pose_points"].cpu().numpy().view(np.uint32)[:n_links], want["points"][:n_links])
    for key in ("pose_R", "pose_t", "pose_stats", "pose_sigma", "pose_points"):
        assert plain[key] is None
    for key in ("model", "link_offsets", "edge_links"):
        assert torch.equal(plain[key], got[key]), key


def test_the_examples_print_the_poses(tmp_path):
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    paths = []
    for t, f in enumerate(_frames()):
        paths.append(str(tmp_path / f"frame{t}.png"))
        f.save(paths[-1])
    ex = os.path.join(ROOT, "local-features_amd", "examples")
    out = subprocess.run([sys.executable, os.path.join(ex, "match_collection.py"), "--window", "1", "--pose", "800"] + paths,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    poses = [line for line in out.stdout.splitlines() if line.startswith("Pose ")]
    assert len(poses) == 2 and all(re.match(r"Pose \d -> \d: (none$|rotation [\d.]+ deg, t [+-][\d.]+ [+-][\d.]+ [+-][\d.]+, \d+ / \d+ "
                                            r"links in front, \d+ with parallax, s2/s1 [\d.]+$)", line) for line in poses), poses
    one = subprocess.run([sys.executable, os.path.join(ex, "match_images.py"), "--fundamental", "--pose", "800", paths[0], paths[1],
                          str(tmp_path / "out.png")], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr
    print(one.stdout)
    assert sum(line.startswith("Pose 1 -> 2: ") for line in one.stdout.splitlines()) == 1
    bad = subprocess.run([sys.executable, os.path.join(ex, "match_images.py"), "--homography", "--pose", "800", paths[0], paths[1],
                          str(tmp_path / "out.png")], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "Required arguments" in bad.stderr
