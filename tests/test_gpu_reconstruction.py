"""The whole reconstruction chain on the GPU, stage after stage on what the stage before left on the device, against the host
chain (tests/reconstruction_twin.py: the C++ twins composed in the same order on the same synthetic collection,
tests/reconstruction_cases.py) word for word: edge_layout -> gather_edge_rows -> verify_fundamental_batch -> link_table ->
two_view_pose -> the initial pair chosen on the device -> build_tracks -> track_table -> triangulate_tracks -> (resect_cameras
in place -> triangulate_tracks) x 3 -> bundle_adjust in place (the second scene: bundle_adjust_intrinsics in place), through
the LocalFeatures wrappers as examples/match_collection.py calls them, nothing read back before the end.

There is no tolerance here but the truth bounds of tests/test_reconstruction_twin.py.  Entries behind a count are compared
only where include/lf_mkd.h defines them, as each stage's own GPU test does."""
import types

import numpy as np
import pytest

import reconstruction_cases as cases
import reconstruction_twin as rtwin
from test_reconstruction_twin import BOUNDS, FOCAL_BOUND, chain_errors, inside

import local_features_python as lfp

pytestmark = pytest.mark.gpu

EXTRA = 37                       # sentinel words in front of and behind the arrays the bundle step writes in place
FILL = rtwin.FILL
OTHER = dict(seed=cases.SEED + 1, extra=45)      # a collection of other sizes, for the run between the two runs of the first one


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


class Framed:
    """a float32 [rows, width] device tensor between EXTRA sentinel words on either side"""

    def __init__(self, torch, rows, width):
        self.n = rows * width
        self.raw = torch.full((self.n + 2 * EXTRA,), FILL, dtype=torch.int32, device="cuda")
        self.view = self.raw[EXTRA:EXTRA + self.n].view(torch.float32).view(rows, width)

    def intact(self):
        raw = self.raw.cpu().numpy().view(np.uint32)
        return bool((raw[:EXTRA] == FILL).all() and (raw[EXTRA + self.n:] == FILL).all())


def device_chain(torch, lf, s, K, focal, params=cases.PARAMS):
    """the chain on the device; returns the device tensors of every stage (nothing is read back here)"""
    p = params
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, n_images = len(s["kps"]), len(s["offsets"]) - 1
    _, _, cap_a, cap_b, match = cases.layouts(s)               # the capacities: sums of image sizes the host knows
    pool, off, ea, eb, m_ab = up(s["kps"]), up(s["offsets"]), up(s["edge_a"]), up(s["edge_b"]), up(match)
    intr = Framed(torch, n_images, 4)
    intr.view.copy_(up(K))
    la, lb = lf.edge_layout(off, ea, n), lf.edge_layout(off, eb, n)
    ka = lf.gather_edge_rows(pool, off, ea, la, capacity=cap_a)
    kb = lf.gather_edge_rows(pool, off, eb, lb, capacity=cap_b)
    model, ver, vstats = lf.verify_fundamental_batch(ka, la, kb, lb, m_ab, threshold=p["f_thr"], n_hypotheses=p["n_hyp"], seed=p["seed"])
    links = lf.link_table(off, ea, eb, la, ver, min_links=p["min_links"], capacity=cap_a, n_rows=n, kept_match=True)
    l_off, l_a, l_b, _, _, l_kept, _ = links
    pose = lf.two_view_pose(model.contiguous(), intr.view, pool, (ea, eb), (l_off, l_a, l_b), p["pose_deg"])
    p_R, p_t, p_stats, _, _ = pose
    # the initial pair, chosen on the device: the edge with the most links with parallax among those that have a pose
    with_pose = torch.where(p_stats[:, 2] >= 0, p_stats[:, 3], torch.full_like(p_stats[:, 3], -1))
    e = torch.argmax(with_pose).reshape(1)
    poses = Framed(torch, n_images, 12)
    poses.view.zero_()
    poses.view.index_copy_(0, ea[e].long(), torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32, device="cuda"))
    poses.view.index_copy_(0, eb[e].long(), torch.cat([p_R[e].reshape(1, 9), p_t[e].reshape(1, 3)], 1))
    poses0 = poses.view.clone()
    tracks = lf.build_tracks(off, ea, eb, la, l_kept, capacity=cap_a, n_rows=n)
    table = lf.track_table(*tracks, image_offsets=off, min_len=2, consistent=True)
    t_off, t_rows, t_img, t_row_track, t_counts = table
    tri = [lf.triangulate_tracks(pool, (t_off, t_rows, t_img, t_counts), intr.view, poses.view, p["px"], p["tri_rounds"])]
    held = (poses.view[:, :9] != 0).any(1).to(torch.int32)
    resect = []
    for _ in range(p["register"]):
        _, r_stats, r_err, r_state = lf.resect_cameras(pool, off, t_row_track, tri[-1][0], t_counts, intr.view, poses.view,
                                                       max_reproj_px=p["px"], min_parallax_deg=0.0, n_samples=p["n_samples"],
                                                       min_inliers=p["min_inliers"], rounds=p["resect_rounds"], seed=p["seed"], out=poses.view)
        resect.append((poses.view.clone(), r_stats, r_err, r_state))
        tri.append(lf.triangulate_tracks(pool, (t_off, t_rows, t_img, t_counts), intr.view, poses.view, p["px"], p["tri_rounds"]))
    points = Framed(torch, tri[-1][0].shape[0], 4)
    points.view.copy_(tri[-1][0])
    kw = dict(obs_state=tri[-1][3], camera_fixed=held, max_reproj_px=p["px"], lambda0=p["lambda0"], iterations=p["iterations"],
              cg_iterations=p["cg_iterations"], cg_tol=p["cg_tol"], out_poses=poses.view, out_points=points.view)
    args = (pool, off, (t_off, t_rows, t_img, t_counts), points.view, intr.view, poses.view)
    if focal:
        b_poses, b_points, b_intr, groups, b_state, trace, counts = lf.bundle_adjust_intrinsics(
            *args, refine_focal=True, refine_principal=False, n_groups=1, out_intrinsics=intr.view, **kw)
        assert b_intr.data_ptr() == intr.view.data_ptr()
    else:
        b_poses, b_points, b_state, trace, counts = lf.bundle_adjust(*args, **kw)
        groups = None
    assert b_poses.data_ptr() == poses.view.data_ptr() and b_points.data_ptr() == points.view.data_ptr()
    return dict(verify=(model, ver, vstats), links=links, pose=pose, edge=e, poses0=poses0, tracks=tracks, table=table, tri=tri,
                resect=resect, bundle=(b_state, trace, counts, groups), frames=dict(poses=poses, points=points, intrinsics=intr),
                focal=focal, keep=(pool, off, ea, eb, m_ab, la, lb, ka, kb, held))


def words(x):
    """a device tensor's words on the host: uint32 (uint64 for 8-byte types)"""
    a = x.detach().cpu().contiguous().numpy()
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def read(d):
    """every stage's words, in the order of the chain, cut to what the header defines: [(stage, array, words)]; and whether the
    sentinels around the arrays the bundle step wrote in place survived"""
    out = []
    add = lambda stage, name, a: out.append((stage, name, np.ascontiguousarray(a)))
    model, ver, vstats = d["verify"]
    add("verify", "F", words(model).reshape(-1, 9)), add("verify", "verified", words(ver))
    add("verify", "stats", (words(vstats) & 0xFFFFFFFF).astype(np.uint32))
    l_off, l_a, l_b, l_edge, l_links, l_kept, l_counts = d["links"]
    n_links = int(words(l_counts)[1])
    add("link_table", "counts", words(l_counts)), add("link_table", "offsets", words(l_off)), add("link_table", "edge_links", words(l_links))
    for name, x in (("link_a", l_a), ("link_b", l_b), ("link_edge", l_edge)):
        add("link_table", name, words(x)[:n_links])
    add("link_table", "match_kept", words(l_kept))
    for name, x in zip(("R", "t", "stats", "sigma"), d["pose"]):
        add("two_view_pose", name, words(x).reshape(len(words(l_links)), -1))
    add("two_view_pose", "points", words(d["pose"][4])[:n_links])
    add("initial pair", "edge", words(d["edge"]).astype(np.uint32)), add("initial pair", "poses", words(d["poses0"]))
    for name, x in zip(("track", "length", "dup"), d["tracks"]):
        add("build_tracks", name, words(x))
    t_off, t_rows, t_img, t_row_track, t_counts = d["table"]
    T, O = (int(v) for v in words(t_counts)[:2])
    add("track_table", "counts", words(t_counts)), add("track_table", "offsets", words(t_off))
    add("track_table", "rows", words(t_rows)[:O]), add("track_table", "images", words(t_img)[:O]), add("track_table", "row_track", words(t_row_track))

    def add_tri(stage, t):
        for name, x in zip(("points", "stats", "err"), t):
            add(stage, name, words(x)[:T])
        add(stage, "obs_state", words(t[3])[:O])

    add_tri("triangulate_tracks 0", d["tri"][0])
    off = d["keep"][1].cpu().numpy()
    for k, (r_poses, r_stats, r_err, r_state) in enumerate(d["resect"]):
        stage = "resect_cameras %d" % (k + 1)
        st = words(r_stats)
        add(stage, "poses", words(r_poses)), add(stage, "stats", st), add(stage, "err", words(r_err))
        resected = np.concatenate([np.arange(off[i], off[i + 1]) for i in range(len(st)) if st[i, 2] != 1] + [np.zeros(0, np.int64)])
        add(stage, "row_state", words(r_state)[resected.astype(np.int64)])       # (defined in the resected images' ranges)
        add_tri("triangulate_tracks %d" % (k + 1), d["tri"][k + 1])
    b_state, trace, counts, groups = d["bundle"]
    stage = "bundle_adjust_intrinsics" if d["focal"] else "bundle_adjust"
    add(stage, "poses", words(d["frames"]["poses"].view)), add(stage, "points", words(d["frames"]["points"].view)[:T])
    add(stage, "obs_state", words(b_state)[:O]), add(stage, "trace", words(trace)), add(stage, "counts", words(counts))
    if d["focal"]:
        add(stage, "intrinsics_out", words(d["frames"]["intrinsics"].view)), add(stage, "group_out", words(groups))
    return out, {k: f.intact() for k, f in d["frames"].items()}


def host_list(s, ch, focal):
    """the host chain's words in read()'s order and cut"""
    out = []
    add = lambda stage, name, a: out.append((stage, name, np.ascontiguousarray(a)))
    u = cases.u32
    v = ch["verify"]
    add("verify", "F", v["F"]), add("verify", "verified", u(v["verified"])), add("verify", "stats", v["stats"])
    L = ch["links"]
    n_links = L.counts[1]
    add("link_table", "counts", np.array(L.counts, np.uint32)), add("link_table", "offsets", L.offsets.astype(np.uint64))
    add("link_table", "edge_links", u(L.edge_links))
    add("link_table", "link_a", u(L.link_a)[:n_links]), add("link_table", "link_b", u(L.link_b)[:n_links])
    add("link_table", "link_edge", u(L.link_edge)[:n_links]), add("link_table", "match_kept", u(L.match_kept))
    for name in ("R", "t", "stats", "sigma"):
        add("two_view_pose", name, ch["pose"][name])
    add("two_view_pose", "points", ch["pose"]["points"][:n_links])
    add("initial pair", "edge", np.array([ch["edge"]], np.uint32)), add("initial pair", "poses", ch["poses0"])
    for name in ("track", "length", "dup"):
        add("build_tracks", name, u(ch["tracks"][name]))
    tt = ch["table"]
    T, O = tt.counts[:2]
    add("track_table", "counts", np.array(tt.counts, np.uint32)), add("track_table", "offsets", tt.offsets.astype(np.uint64))
    add("track_table", "rows", u(tt.obs_row)[:O]), add("track_table", "images", u(tt.obs_image)[:O]), add("track_table", "row_track", u(tt.row_track))

    def add_tri(stage, t):
        for name in ("points", "stats", "err"):
            add(stage, name, t[name][:T])
        add(stage, "obs_state", t["obs_state"][:O])

    add_tri("triangulate_tracks 0", ch["tri"][0])
    off = s["offsets"]
    for k, r in enumerate(ch["resect"]):
        stage = "resect_cameras %d" % (k + 1)
        st = r["stats"]
        add(stage, "poses", r["poses"]), add(stage, "stats", st), add(stage, "err", r["err"])
        resected = np.concatenate([np.arange(off[i], off[i + 1]) for i in range(len(st)) if st[i, 2] != 1] + [np.zeros(0, np.int64)])
        add(stage, "row_state", r["row_state"][resected.astype(np.int64)])
        add_tri("triangulate_tracks %d" % (k + 1), ch["tri"][k + 1])
    b = ch["bundle"]
    stage = "bundle_adjust_intrinsics" if focal else "bundle_adjust"
    add(stage, "poses", b["poses"]), add(stage, "points", b["points"][:T]), add(stage, "obs_state", b["obs_state"][:O])
    add(stage, "trace", b["trace_words"]), add(stage, "counts", b["counts"])
    if focal:
        add(stage, "intrinsics_out", b["intrinsics"]), add(stage, "group_out", b["groups"])
    return out


def first_difference(got, want):
    """None, or a description of the first stage and array in which two word lists differ, with the first few words"""
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    for (stage, name, g), (_, _, w) in zip(got, want):
        if g.shape != w.shape and g.size == w.size:
            g = g.reshape(w.shape)
        if g.shape != w.shape:
            return "%s: %s has shape %s, not %s" % (stage, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        if len(bad):
            some = [(tuple(int(i) for i in b), hex(int(g[tuple(b)])), hex(int(w[tuple(b)]))) for b in bad[:5]]
            return "%s: %s differs in %d of %d words; (index, got, want) of the first: %s" % (stage, name, len(bad), g.size, some)
    return None


def refill(torch, d):
    """every output tensor of a run filled with the twins' FILL pattern, so that a later run that lands in the same memory
    and leaves a word unwritten shows it"""
    seen = []

    def walk(x):
        if isinstance(x, (tuple, list)):
            for y in x:
                walk(y)
        elif isinstance(x, Framed):
            seen.append(x.raw)
        elif x is not None and hasattr(x, "is_cuda"):
            seen.append(x)

    for key in ("verify", "links", "pose", "poses0", "tracks", "table", "tri", "resect", "bundle"):
        walk(d[key])
    walk(list(d["frames"].values()))
    for x in seen:
        if x.is_contiguous():
            x.view(torch.int32).fill_(FILL)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def runs(torch, tmp_path_factory):
    """ONE handle; on it the first scene, the second scene (the same collection, the focal length 3 % too long, the last stage
    bundle_adjust_intrinsics), a collection of other sizes with that last stage, and the first scene once more.  Each run is
    read back after one synchronise at its end; between runs every output buffer is refilled with FILL.  Returns per run the
    device's word list, the sentinels' state and the host chain's word list."""
    lf = lfp.LocalFeatures(64, 64, 16)
    twins = rtwin.Twins(tmp_path_factory.mktemp("reconstruction_twin"))
    s, other = cases.scene(), cases.scene(**OTHER)
    assert len(other["kps"]) > len(s["kps"])
    plan = (("plain", s, 1.0, False), ("focal", s, cases.FOCAL_SCALE, True), ("other sizes", other, cases.FOCAL_SCALE, True),
            ("plain again", s, 1.0, False))
    out = {}
    for name, sc, scale, focal in plan:
        K = cases.intrinsics(sc, scale)
        d = device_chain(torch, lf, sc, K, focal)
        torch.cuda.synchronize()
        got, intact = read(d)
        refill(torch, d)
        del d
        chain = out["plain"]["chain"] if name == "plain again" else rtwin.run(twins, sc, K, focal=focal)
        out[name] = dict(got=got, intact=intact, chain=chain, want=host_list(sc, chain, focal), scene=sc)
    return out


@pytest.mark.parametrize("which", ["plain", "focal", "other sizes"])
def test_every_stage_equals_the_host_chain(runs, which):
    r = runs[which]
    n_words = sum(a.size for _, _, a in r["got"])
    print(which, ": %d arrays, %d words compared" % (len(r["got"]), n_words))
    assert first_difference(r["got"], r["want"]) is None, first_difference(r["got"], r["want"])


def test_the_device_chain_recovers_the_truth(runs):
    """the readable statement of what the chain is for: the device's poses and points against the truth, inside the bounds the
    reference chain's own errors set"""
    for which in ("plain", "focal"):
        r = runs[which]
        by = {(stage, name): a for stage, name, a in r["got"]}
        last = "bundle_adjust_intrinsics" if which == "focal" else "bundle_adjust"
        T = int(by[("track_table", "counts")][0])
        e = int(by[("initial pair", "edge")][0])
        s = r["scene"]
        table = types.SimpleNamespace(counts=[int(x) for x in by[("track_table", "counts")]], offsets=by[("track_table", "offsets")],
                                      obs_row=by[("track_table", "rows")].view(np.int32))
        ch = dict(pair=(int(s["edge_a"][e]), int(s["edge_b"][e])), table=table, poses=by[("resect_cameras 3", "poses")],
                  tri=[dict(points=by[("triangulate_tracks 3", "points")])],
                  bundle=dict(poses=by[(last, "poses")], points=by[(last, "points")]))
        got = chain_errors(s, ch)
        print(which, "device chain, before the bundle (rotation, centre, median point):", ["%.4e" % x for x in got["before"]])
        print(which, "device chain, after the bundle:                                  ", ["%.4e" % x for x in got["after"]])
        assert T > 300 and inside(got["before"], BOUNDS[which]["before"]) and inside(got["after"], BOUNDS[which]["after"]), (which, got)
        if which == "focal":
            err = cases.focal_error(cases.f32(by[(last, "group_out")]))
            print("focal device chain: |s * 1.03 - 1| = %.4e" % err)
            assert err <= FOCAL_BOUND, err


def test_a_run_after_other_stages_and_sizes_equals_the_first(runs):
    """scratch across stages: scene 1, then two runs of other sizes and another last stage on the same handle, then scene 1
    again -- the last run equals the first word for word at every stage"""
    assert first_difference(runs["plain again"]["got"], runs["plain"]["got"]) is None, \
        first_difference(runs["plain again"]["got"], runs["plain"]["got"])
    assert first_difference(runs["plain again"]["got"], runs["plain again"]["want"]) is None


def test_the_bundle_in_place_writes_nothing_outside_its_arrays(runs):
    for which, r in runs.items():
        assert all(r["intact"].values()), (which, "a write outside", [k for k, ok in r["intact"].items() if not ok])
