"""CPU tests of the whole reconstruction chain on one synthetic collection (tests/reconstruction_cases.py): the float64 numpy
restatements of every stage composed in the order examples/match_collection.py calls them (the reference chain), and the same
composition with the C++ twins in their place (the host chain, tests/reconstruction_twin.py), which
tests/test_gpu_reconstruction.py holds the device chain to word for word.  Here the scene is shown to contain what the seams
between the stages need -- an image that cannot register, one that registers late, an edge between strangers, inconsistent
tracks -- and both chains are held to the truth: the reference's own errors are the measurement, twice that is the bound.

Measured on cases.SEED with cases.PARAMS (DESIGN.md 6v repeats them); printed by every run (pytest -s)."""
import numpy as np
import pytest

import reconstruction_cases as cases
import reconstruction_twin as rtwin

# The reference chain's errors against the truth in the gauge of the initial pair, before and after the bundle step: the
# largest rotation error (rad) and the largest distance of the camera centres over the registered images, and the median point
# error over the tracks with a point (the unit is the initial pair's baseline).  The bounds are these times 2, the convention
# of ROT_BOUND in tests/test_resect_twin.py: room for f32 outputs and a flipped near-tie, far below what a slipped convention
# costs (a transposed R or a pose in the wrong direction is an error of the order of the rotation itself, 0.1 rad and more).
MEASURED = {
    "plain": dict(before=(5.478e-3, 2.503e-2, 1.558e-2), after=(9.470e-4, 4.630e-3, 7.336e-3)),
    # the second scene: the chain is handed focal lengths 3 % too long, its last stage refines them
    "focal": dict(before=(1.781e-2, 7.689e-2, 5.928e-2), after=(3.359e-3, 1.976e-2, 4.954e-2)),
}
FOCAL_MEASURED = 4.959e-3        # |s * 1.03 - 1| of the reference chain's refined focal scale (before the bundle: 0.03)
FACTOR = 2.0
BOUNDS = {k: {w: tuple(FACTOR * x for x in v[w]) for w in ("before", "after")} for k, v in MEASURED.items()}
FOCAL_BOUND = FACTOR * FOCAL_MEASURED
SCENES = ("plain", "focal")


def inside(errors, bound):
    return all(e <= b for e, b in zip(errors, bound))


def chain_errors(s, ch):
    """{before, after}: cases.errors of the chain's poses and points entering and leaving the bundle step"""
    last, b = ch["tri"][-1], ch["bundle"]
    return dict(before=cases.errors(s, ch, cases.f32(ch["poses"]).reshape(-1, 12), cases.f32(last["points"]).reshape(-1, 4)),
                after=cases.errors(s, ch, cases.f32(b["poses"]).reshape(-1, 12), cases.f32(b["points"]).reshape(-1, 4)))


def conditions(s, ch, what):
    """what the scene was built to contain, as a chain shows it (conditions, not measurements)"""
    n, E = cases.N_IMAGES, len(s["edge_a"])
    U, L = cases.UNREGISTERABLE, cases.LATE
    registerable = [i for i in range(n) if i != U]
    st = np.asarray(ch["pose"]["stats"]).astype(np.uint32).view(np.int32).reshape(E, 4)
    false_edge = [e for e in range(E) if (s["edge_a"][e], s["edge_b"][e]) == cases.FALSE_EDGE]
    assert len(false_edge) == 1 and st[false_edge[0], 2] == -1, (what, "the false edge has a pose", st[false_edge[0]])
    assert ch["links"].edge_links[false_edge[0]] > 0 and ch["links"].offsets[false_edge[0]] == ch["links"].offsets[false_edge[0] + 1], what
    assert not set(ch["pair"]) & {U, L} and not (s["seen"][:, L] & (s["seen"][:, ch["pair"][0]] | s["seen"][:, ch["pair"][1]])).any(), what
    stages = [cases.f32(ch["poses0"]).reshape(n, 12)] + [cases.f32(r["poses"]).reshape(n, 12) for r in ch["resect"]]
    stages.append(cases.f32(ch["bundle"]["poses"]).reshape(n, 12))
    for k, P in enumerate(stages):
        assert not P[U].any(), (what, "the unregisterable image has a pose after stage", k)
    assert ch["table"].obs_image.tolist().count(U) > 0, (what, "the unregisterable image is in no track")
    P = stages[-2]
    assert (P[registerable][:, :9] != 0).any(1).all(), (what, "not every registerable image is registered", P[:, :9].any(1))
    first, last = ch["resect"][0]["stats"], ch["resect"][-1]["stats"]
    assert first[L, 2] != 0 and not stages[1][L].any(), (what, "the late image registered in round 1", first[L])
    assert any(r["stats"][L, 2] == 0 for r in ch["resect"][1:]), (what, "the late image never registered")
    assert first[U, 0] < ch["params"]["min_inliers"] and all(r["stats"][U, 2] in (2, 3) for r in ch["resect"]), (what, first[U])
    assert (last[registerable, 2] == 1).all() and np.array_equal(ch["resect"][-1]["poses"], ch["resect"][-2]["poses"]), \
        (what, "the last round changed a pose", last[:, 2])
    tr = ch["tracks"]
    dropped = int(((tr["length"] >= 2) & (tr["dup"] > 0)).sum())
    assert dropped >= 1 and ch["table"].counts[0] == int(((tr["length"] >= 2) & (tr["dup"] == 0)).sum()), (what, dropped)
    T = ch["table"].counts[0]
    with_point = cases.tracks_with_point(ch["tri"][-1], T)
    assert with_point >= 0.9 * T, (what, with_point, T)
    # the bundle step: the unregisterable image's observations are state 0, the held poses keep their words
    b = ch["bundle"]
    O = ch["table"].counts[1]
    state = np.asarray(b["obs_state"])[:O]
    assert (state[ch["table"].obs_image == U] == 0).all() and (state == 2).sum() > 0.8 * O, (what, np.bincount(state.astype(np.int64) & 3))
    held = np.flatnonzero(ch["held"])
    assert sorted(held.tolist()) == sorted(ch["pair"]), what
    assert np.array_equal(np.asarray(b["poses"])[held], ch["poses"].reshape(n, 12)[held]), (what, "a held pose moved")
    assert np.array_equal(np.asarray(b["poses"])[U], ch["poses"].reshape(n, 12)[U]), what
    return dict(dropped=dropped, tracks=T, with_point=with_point)


@pytest.fixture(scope="module")
def scene():
    return cases.scene()


@pytest.fixture(scope="module")
def reference(scene):
    """the reference chain on both scenes: computed once, not changed"""
    be = cases.Reference()
    return {"plain": cases.run_chain(scene, cases.intrinsics(scene), be),
            "focal": cases.run_chain(scene, cases.intrinsics(scene, cases.FOCAL_SCALE), be, focal=True)}


@pytest.fixture(scope="module")
def host(scene, tmp_path_factory):
    """the host chain (the twins) on both scenes: every twin compiled once"""
    twins = rtwin.Twins(tmp_path_factory.mktemp("reconstruction_twin"))
    return {"plain": rtwin.run(twins, scene, cases.intrinsics(scene)),
            "focal": rtwin.run(twins, scene, cases.intrinsics(scene, cases.FOCAL_SCALE), focal=True)}


def test_the_scene_is_what_the_seams_need(scene):
    s = scene
    rows = np.diff(s["offsets"])
    named = [np.zeros(r, bool) for r in rows]
    for e, m in enumerate(s["matches"]):
        a, b = s["edge_a"][e], s["edge_b"][e]
        named[a][m >= 0] = True
        named[b][m[m >= 0]] = True
    print("rows per image", rows.tolist(), "rows no match names", [int((~x).sum()) for x in named])
    assert len(rows) == 8 and 350 <= len(s["truth_points"]) <= 450
    assert all(150 <= r <= 300 for i, r in enumerate(rows) if i not in (cases.UNREGISTERABLE, cases.LATE)), rows
    assert all((~x).sum() >= 15 for x in named)
    assert s["seen"][:, cases.UNREGISTERABLE].sum() < cases.PARAMS["min_inliers"]
    a, b = cases.FALSE_EDGE
    assert not (s["seen"][:, a] & s["seen"][:, b]).any() and (s["matches"][-1] >= 0).sum() > cases.PARAMS["min_links"]
    # about 15 % of the window edges' matches are wrong
    wrong = []
    for e, m in enumerate(s["matches"][:-1]):
        a, b = s["edge_a"][e], s["edge_b"][e]
        at = np.flatnonzero(m >= 0)
        wrong.append(s["row_point"][s["offsets"][a] + at] != s["row_point"][s["offsets"][b] + m[at]])
    assert 0.12 <= np.concatenate(wrong).mean() <= 0.18, np.concatenate(wrong).mean()


@pytest.mark.parametrize("which", SCENES)
def test_the_reference_chain_meets_the_conditions(scene, reference, which):
    print(which, conditions(scene, reference[which], ("reference", which)))


@pytest.mark.parametrize("which", SCENES)
def test_the_host_chain_meets_the_conditions(scene, host, which):
    print(which, conditions(scene, host[which], ("host", which)))


@pytest.mark.parametrize("which", SCENES)
def test_the_reference_reproduces_the_measured_errors(scene, reference, which):
    got = chain_errors(scene, reference[which])
    print(which, "reference chain, before the bundle (rotation, centre, median point):", ["%.4e" % x for x in got["before"]])
    print(which, "reference chain, after the bundle:                                  ", ["%.4e" % x for x in got["after"]])
    for w in ("before", "after"):
        assert np.allclose(got[w], MEASURED[which][w], rtol=0.01, atol=0), (which, w, got[w], MEASURED[which][w])


@pytest.mark.parametrize("which", SCENES)
def test_the_host_chain_is_inside_the_bounds(scene, host, which):
    got = chain_errors(scene, host[which])
    print(which, "host chain, before the bundle (rotation, centre, median point):", ["%.4e" % x for x in got["before"]])
    print(which, "host chain, after the bundle:                                  ", ["%.4e" % x for x in got["after"]])
    for w in ("before", "after"):
        assert inside(got[w], BOUNDS[which][w]), (which, w, got[w], BOUNDS[which][w])


def test_the_bundle_matters(scene, reference):
    """in the reference every error leaving the bundle is below half the error entering it, so a bundle step that did nothing
    is outside the `after` bound (twice the error leaving it)"""
    got = chain_errors(scene, reference["plain"])
    assert all(a < 0.5 * b for a, b in zip(got["after"], got["before"])), got
    tr = reference["plain"]["bundle"]["trace"]
    assert tr[:, 3].sum() >= 3 and tr[-1, 1] < 0.5 * tr[0, 0], tr[:, :4]
    assert not inside(got["before"], BOUNDS["plain"]["after"])


def test_the_focal_scene(scene, reference, host):
    """the wrong focal length shows in the initial edge's singular values before the bundle, and is refined away by it"""
    plain, focal = reference["plain"], reference["focal"]
    assert plain["edge"] == focal["edge"]
    ratio = lambda ch: float(cases.f32(ch["pose"]["sigma"]).reshape(-1, 3)[ch["edge"], 1])
    print("s2 / s1 of the initial edge: %.5f with the true focal length, %.5f with 1.03 times it" % (ratio(plain), ratio(focal)))
    assert abs(ratio(focal) - 1) > abs(ratio(plain) - 1)
    ref_err, host_err = cases.focal_error(cases.f32(focal["bundle"]["groups"])), cases.focal_error(cases.f32(host["focal"]["bundle"]["groups"]))
    print("|s * 1.03 - 1|: reference chain %.4e, host chain %.4e (0.03 before the bundle)" % (ref_err, host_err))
    assert np.isclose(ref_err, FOCAL_MEASURED, rtol=0.01, atol=0), ref_err
    assert host_err <= FOCAL_BOUND, host_err
    for ch in (focal, host["focal"]):
        K = cases.f32(ch["bundle"]["intrinsics"]).reshape(-1, 4)
        s = cases.f32(ch["bundle"]["groups"]).reshape(-1, 3)[0, 0]
        assert np.allclose(K[:, :2], np.float64(s) * ch["K"][:, :2], rtol=2.0 ** -22, atol=0) and np.array_equal(K[:, 2:], ch["K"][:, 2:])
        assert ch["bundle"]["counts"][4] == 1
