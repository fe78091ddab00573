"""The host twin of the tree-pose and global-positioning calls (tests/cpp/positions_twin.cpp: csrc/mkd_positions_math.h under
g++ -O2 -ffp-contract=off) against the float64 numpy restatement of include/lf_mkd.h (tests/positions_cases.py), the
restatement against the truth, and the properties the header states, each on a few lines of scene.  No GPU.

The truth bounds are the restatement's own largest centre errors times 2, the chain tests' convention: the
margin absorbs the twin's different summation order and not an algorithmic regression.
    scene A (6 cameras on a ring, 60 points)      1.281e-3  ->  2.562e-3     without robust weights 1.433e-1 (112 x)
    scene B (8 cameras on a line, 112 tracks)     3.948e-3  ->  7.896e-3
in units of the true centres' rms radius, after a similarity fit of the centres.  The twin's f32 words differ from the
restatement's by 0 on the scenes A, B and C (both calls, robust and not); the gate is 2^-23, as the view graph's.  The
trace's cost is a sum of squared residuals |P r|^2, each a difference of values of size 1 that carry the sweeps' rounding
in another summation order (some tens of u = 2^-53; 64 u is allowed for) while the residual itself is no smaller than the
noise, 0.5 px / 800 px = 6e-4 of |r|: 2 * 64 u / 6e-4 = 2.4e-11, so the cost's gate is 2^-35 of its value (the largest
difference seen is printed by the test: 6e-14 on the noise-only scenes, 1e-15 on A, B and C)."""
import numpy as np
import pytest

import positions_cases as cases
import positions_twin as pt

BOUND = dict(A=2 * 1.281e-3, B=2 * 3.948e-3)
GATE = 2.0 ** -23
COST_GATE = 2.0 ** -35
SCENES = dict(A=cases.scene_a, B=cases.scene_b, C=cases.scene_c)


@pytest.fixture(scope="module")
def scenes():
    return {k: make() for k, make in SCENES.items()}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("positions_twin")
    return pt.build(tmp), tmp


@pytest.fixture(scope="module")
def twin(program):
    exe, tmp = program
    return lambda scene, **kw: pt.run(exe, tmp, scene, **kw)


@pytest.fixture(scope="module")
def reference(scenes):
    """the restatement on every scene, robust and not: computed once, not changed"""
    return {(k, robust): cases.reference(s, **{**pt.DEFAULTS, **({} if robust else dict(warm=pt.DEFAULTS["sweeps"]))})
            for k, s in scenes.items() for robust in (True, False)}


def agree(tw, ref, s, what):
    """every integer word equal, every f32 word within GATE, the trace's cost within COST_GATE of its value"""
    T, O = int(s["counts"][0]), int(s["counts"][1])
    state = np.where(tw["obs_state"] == pt.FILL, cases.NONE, tw["obs_state"])
    assert np.array_equal(state, ref["obs_state"]), what
    assert np.array_equal(tw["image_stats"], ref["image_stats"]) and np.array_equal(tw["counts"], ref["counts"]), what
    assert np.array_equal(tw["trace"][:, 1:], ref["trace"][:, 1:]), what
    d_cost = np.abs(tw["trace"][:, 0] - ref["trace"][:, 0]) / np.maximum(np.abs(ref["trace"][:, 0]), 1e-300)
    print("%s: the cost differs by %.3g of its value at most" % (what, d_cost.max() if len(d_cost) else 0.0))
    assert (d_cost <= COST_GATE).all(), what
    d_pose = np.abs(pt.f32(tw["poses"]) - ref["poses"]).max()
    d_pts = np.abs(pt.f32(tw["points"])[:T] - ref["points"]).max() if T else 0.0
    print("%s: f32 words differ by %.3g (poses) and %.3g (points)" % (what, d_pose, d_pts))
    assert d_pose <= GATE and d_pts <= GATE, (what, d_pose, d_pts)
    assert (tw["points"][T:] == pt.FILL).all() and O <= len(state)


@pytest.mark.parametrize("which", "AB")
def test_the_restatement_finds_the_truth(scenes, reference, which):
    s, ref = scenes[which], reference[(which, True)]
    err = cases.similarity_error(ref["centres"], s["truth"]["centres"])
    print("scene %s: the restatement's largest centre error %.4g" % (which, err))
    assert err <= BOUND[which] / 2 * 1.0005                        # the recorded value itself (rounded to four digits)
    assert ref["counts"][0] == len(s["intrinsics"]) and ref["counts"][5] == 0 and ref["trace"][-1, 2] == 0
    # the outliers are what the weights turn down: about the scene's share of wrong rays ends below 1/2
    share = 1.0 - ref["counts"][3] / ref["counts"][2]
    assert 0.04 <= share <= 0.25, share


def test_without_robust_weights_the_wrong_rays_pull_the_centres(scenes, reference):
    s = scenes["A"]
    robust = cases.similarity_error(reference[("A", True)]["centres"], s["truth"]["centres"])
    plain = cases.similarity_error(reference[("A", False)]["centres"], s["truth"]["centres"])
    print("scene A: %.4g with and %.4g without robust weights (%.0f x)" % (robust, plain, plain / robust))
    assert plain >= 4 * robust


@pytest.mark.parametrize("which", "ABC")
@pytest.mark.parametrize("robust", (True, False))
def test_the_twin_agrees_with_the_restatement(scenes, reference, twin, which, robust):
    s = scenes[which]
    tw = twin(s, **({} if robust else dict(warm=pt.DEFAULTS["sweeps"])))
    agree(tw, reference[(which, robust)], s, "%s robust=%s" % (which, robust))
    if which in BOUND and robust:
        err = cases.similarity_error(cases.centres_of(pt.f32(tw["poses"])), s["truth"]["centres"])
        assert err <= BOUND[which], err


def test_the_seams_of_scene_c_are_there(scenes):
    s = scenes["C"]
    rows = np.diff(s["image_offsets"].astype(np.int64))
    T = int(s["counts"][0])
    lengths = np.diff(s["track_offsets"].astype(np.int64))[:T]
    assert {255, 256, 257} <= set(rows.tolist()) and {2, 3, 4, 5, 8, 9} <= set(lengths.tolist())
    assert len(s["track_offsets"]) - 1 > T and len(s["obs_row"]) > int(s["counts"][1]) and (s["row_track"] < 0).any()
    lo, hi = int(s["track_offsets"][260]), int(s["track_offsets"][261])
    assert len(set(s["obs_image"][lo:hi].tolist())) < hi - lo                   # two rows of one image in track 260


# ---- tree poses ---------------------------------------------------------------------------------------------------------------
def test_tree_poses_agree_with_the_restatement_and_the_truth(program):
    exe, tmp = program
    s = cases.tree_scene()
    got, ref = pt.f32(pt.run_tree(exe, tmp, s)), cases.tree_reference(s)
    assert np.abs(got - ref).max() <= GATE
    c, truth = cases.centres_of(got), s["truth"]
    for i in range(1, len(c)):                                     # unit steps along the true directions
        d = truth[i] - truth[i - 1]
        assert np.abs(c[i] - c[i - 1] - d / np.linalg.norm(d)).max() < 1e-6
    assert np.array_equal(got[:, :9], s["rotations"]) and (got[0, 9:] == 0).all()


def test_the_order_of_the_edge_list_does_not_show(program):
    exe, tmp = program
    s = cases.tree_scene()
    order = np.random.default_rng(1).permutation(len(s["edge_a"]))
    where = np.argsort(order)                                      # edge e is entry where[e] of the permuted list
    p = dict(s, edge_a=s["edge_a"][order], edge_b=s["edge_b"][order], t=s["t"][order], image_stats=s["image_stats"].copy())
    p["image_stats"][1:, 2] = where[s["image_stats"][1:, 2]]
    assert np.array_equal(pt.run_tree(exe, tmp, s), pt.run_tree(exe, tmp, p))


def test_either_end_of_a_tree_edge_gets_the_mirrored_step(program):
    exe, tmp = program
    eye = np.eye(3, dtype=np.float32).reshape(9)
    base = dict(edge_a=[0], edge_b=[1], t=np.array([[0.3, -1.1, 2.0]], np.float32), rotations=np.stack([eye, eye]))
    at_b = pt.f32(pt.run_tree(exe, tmp, dict(base, image_stats=np.array([[1, 0, cases.NONE, 0], [1, 1, 0, 0]], np.uint32))))
    at_a = pt.f32(pt.run_tree(exe, tmp, dict(base, image_stats=np.array([[1, 1, 0, 0], [1, 0, cases.NONE, 0]], np.uint32))))
    assert (at_b[0, 9:] == 0).all() and (at_a[1, 9:] == 0).all()
    assert np.array_equal(at_b[1, 9:], -at_a[0, 9:]) and abs(np.linalg.norm(at_b[1, 9:]) - 1) < 1e-6
    # c_b - c_a is parallel to -R_b^T t: with R = I the image at b stands at -t / |t|, so its translation is t / |t|
    assert np.allclose(at_b[1, 9:], base["t"][0] / np.linalg.norm(base["t"][0]), atol=1e-6)


def test_an_unlabelled_image_and_a_cut_chain_give_zero_rows(program):
    exe, tmp = program
    s = cases.tree_scene()
    full = pt.run_tree(exe, tmp, s)
    cut = pt.run_tree(exe, tmp, s, max_depth=3)
    assert np.array_equal(cut[:4], full[:4]) and (cut[4:] == 0).all() and full[4:].any(1).all()
    u = dict(s, image_stats=s["image_stats"].copy(), rotations=s["rotations"].copy())
    u["image_stats"][2, 1] = cases.NONE                             # image 2 unlabelled: 2 and everything below it
    got = pt.run_tree(exe, tmp, u)
    assert np.array_equal(got[:2], full[:2]) and (got[2:] == 0).all()
    u = dict(s, rotations=s["rotations"].copy())
    u["rotations"][5] = 0                                          # an all-zero rotation: the same for 5 and 6
    got = pt.run_tree(exe, tmp, u)
    assert np.array_equal(got[:5], full[:5]) and (got[5:] == 0).all()


# ---- properties of global positions -------------------------------------------------------------------------------------------
def test_no_sweep_returns_the_input_in_the_gauge(twin):
    s = cases.tiny()
    tw = twin(s, sweeps=0)
    c0 = cases.centres_of(s["poses"])
    c0 = c0 - c0.mean(0)
    c0 = c0 / np.sqrt((c0 * c0).sum(1).mean())
    assert np.abs(cases.centres_of(pt.f32(tw["poses"])) - c0).max() < 1e-6
    T = int(s["counts"][0])
    assert np.array_equal(pt.f32(tw["points"])[:T], np.tile(np.float32([0, 0, 0, 2]), (T, 1)))
    assert tw["counts"].tolist() == [4, 0, 0, 0, 0, 0, T, 0] and tw["trace"].shape == (0, 4)
    assert (tw["image_stats"] == 0).all() and set(tw["obs_state"][:int(s["counts"][1])].tolist()) == {1}
    agree(tw, cases.reference(s, sweeps=0), s, "no sweep")


def test_an_unregistered_image_stays_zero_and_its_observations_count_for_nothing(twin):
    s = cases.tiny()
    s["poses"][2] = 0
    gone = dict(s, obs_row=np.where(s["obs_image"] == 2, -1, s["obs_row"]).astype(np.int32))
    a, b = twin(s), twin(gone)
    assert (a["poses"][2] == 0).all() and a["image_stats"][2].tolist() == [0, 0, 0, 1] and a["counts"][0] == 3
    for k in ("poses", "points", "image_stats", "counts", "trace"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["obs_state"][s["obs_image"] == 2] == 0).all() and (a["obs_state"][s["obs_image"] != 2] == 2).all()
    agree(a, cases.reference(s), s, "unregistered")


def test_a_camera_with_too_few_observations_is_held_in_every_sweep(twin):
    g = np.random.default_rng(2)
    ang = np.linspace(0, 2 * np.pi, 4, endpoint=False)
    centres = np.stack([4 * np.cos(ang), np.zeros(4), 4 * np.sin(ang)], 1)
    visible = np.ones((12, 4), bool)
    visible[1:, 3] = False                                         # camera 3 sees one point
    s = cases.build(7, centres, np.zeros((4, 3)), g.standard_normal((12, 3)), visible, outliers=0.0)
    tw, ref = twin(s, sweeps=9), cases.reference(s, sweeps=9)
    agree(tw, ref, s, "held")
    assert tw["image_stats"][3, [0, 2, 3]].tolist() == [1, 9, 2] and (tw["image_stats"][:3, 2:] == 0).all()
    assert (tw["trace"][:, 2] == 1).all() and tw["counts"][4] == 1
    # it keeps its initial centre, re-gauged: the gauges are similarities, so it stays where it was among its own images'
    # initial centres only up to the others' motion; what is checked is that no step moved it -- its centre is the
    # restatement's, which applies nothing but the gauges to it
    assert np.abs(cases.centres_of(pt.f32(tw["poses"]))[3] - ref["centres"][3]).max() < 1e-6


def test_cameras_that_are_all_held_stay_where_the_input_put_them(twin):
    """independent of the restatement: with min_obs above every camera's rows every camera is held in every sweep, so no step
    moves a centre and the sweeps' gauges find centroid 0 and radius 1 already there -- the output is the call without a
    sweep"""
    s = cases.tiny()
    still, none = twin(s, sweeps=9, min_obs=13), twin(s, sweeps=0)
    assert np.abs(cases.centres_of(pt.f32(still["poses"])) - cases.centres_of(pt.f32(none["poses"]))).max() < 1e-6
    assert (still["image_stats"][:, 2:] == [9, 2]).all() and (still["trace"][:, 2] == 4).all() and still["counts"][4] == 4


def test_a_track_of_parallel_rays_is_unsolved(twin):
    g = np.random.default_rng(3)
    ang = np.linspace(0, 2 * np.pi, 4, endpoint=False)
    centres = np.stack([4 * np.cos(ang), np.zeros(4), 4 * np.sin(ang)], 1)
    visible = np.ones((12, 4), bool)
    visible[0] = [False, True, False, False]
    s = cases.build(8, centres, np.zeros((4, 3)), g.standard_normal((12, 3)), visible, outliers=0.0, twice=((0, 1),))
    assert s["track_offsets"][1] == 2 and (s["obs_image"][:2] == 1).all()
    s["kps"][s["obs_row"][1]] = s["kps"][s["obs_row"][0]]          # two rows of image 1 with one keypoint: one ray twice
    tw = twin(s)
    assert pt.f32(tw["points"])[0].tolist() == [0, 0, 0, 2] and tw["obs_state"][:2].tolist() == [1, 1]
    assert tw["counts"][1] == 11 and (tw["trace"][:, 3] == 1).all()
    agree(tw, cases.reference(s), s, "parallel rays")


def test_a_similarity_of_the_input_does_not_show(twin):
    """four cameras (a mean over a power of two is exact) with the identity as rotation and centres on a grid of eighths: a scale
    of 2 and a shift by eighths are exact in every operation up to the first gauge, which removes them, so every output word
    is equal"""
    g = np.random.default_rng(4)
    centres = np.array([[0, 0, 0], [1.5, 0.25, 0], [3.0, -0.25, 0.125], [4.5, 0, -0.125]])
    X = np.stack([g.uniform(-1, 6, 40), g.uniform(-2, 2, 40), g.uniform(5, 9, 40)], 1)
    s = cases.build(9, centres, centres + np.array([0, 0, 6.0]), X, g.random((40, 4)) < 0.8, outliers=0.05)
    assert np.array_equal(s["poses"][:, :9], np.tile(np.eye(3, dtype=np.float32).reshape(9), (4, 1)))
    start = np.round(cases.centres_of(s["poses"]) * 8) / 8
    s["poses"][:, 9:] = -start
    moved = dict(s, poses=s["poses"].copy())
    moved["poses"][:, 9:] = -(2 * start + np.array([3.0, -1.5, 0.25]))
    a, b = twin(s), twin(moved)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["counts"][1] > 30
