"""CPU tests of the track triangulation call's host twin (tests/cpp/triangulate_twin.cpp: the kernel's math header under g++)
against the float64 numpy restatement of the algorithm (tests/triangulate_cases.py), and of the algorithm itself on the
restatement alone.  The twin is what tests/test_gpu_triangulate.py holds the kernel to, word for word; here the twin is held
to the algorithm: counts, reasons, winning pairs and states equal, points within 2^-22 max(1, |X|_inf) per component (the f32
store is 2^-24 relative, the f64 reordering far below that at these parallaxes).  Measured maximum: 5.0e-8 (families), 4.0e-8
(seams); 2^-22 = 2.4e-7."""
import numpy as np
import pytest

import triangulate_cases as cases
import triangulate_twin as twin

TOL = 2.0 ** -22


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return twin.build(tmp_path_factory.mktemp("triangulate_twin"))


def agree(out, ref, table, what=""):
    """the twin's words against the restatement; returns the largest point deviation over max(1, |X|_inf)"""
    T = len(ref["points"])
    counts = np.asarray(table["counts"]).astype(np.int64)
    assert T == min(int(counts[0]), len(out["points"]))
    st = out["stats"][:T].astype(np.int64)
    assert (st == ref["stats"]).all(), (what, np.flatnonzero((st != ref["stats"]).any(1))[:8])
    covered = ref["obs_state"] >= 0
    assert (out["obs_state"].astype(np.int64)[covered] == ref["obs_state"][covered]).all(), what
    # what the call does not write stays as it was
    assert (out["obs_state"][~covered] == twin.FILL).all(), what
    for name in ("points", "stats", "err"):
        assert (out[name][T:] == twin.FILL).all(), (what, name)
    pts, err = twin.f32(out["points"][:T]).astype(np.float64), twin.f32(out["err"][:T]).astype(np.float64)
    none = ref["stats"][:, 2] != 0
    assert (out["points"][:T][none] == np.array([0, 0, 0, 0x40000000], np.uint32)).all(), what
    assert (out["err"][:T][none] == 0).all(), what
    worst = 0.0
    if (~none).any():
        scale = np.maximum(1.0, np.abs(ref["points"][~none, :3]).max(1))[:, None]
        dev = np.abs(pts[~none, :3] - ref["points"][~none, :3]) / scale
        worst = float(dev.max())
        assert worst <= TOL, (what, worst)
        assert np.abs(pts[~none, 3] - ref["points"][~none, 3]).max() <= TOL, what
        # the errors are roots of sums of squares of differences of pixel coordinates (up to 2^10): f32 store, 2^-22 relative
        # plus what cancellation leaves of 2^-53 x 2^10 px
        assert (np.abs(err[~none] - ref["err"][~none]) <= TOL * np.maximum(1.0, ref["err"][~none]) + 1e-9).all(), what
    return worst


def test_the_families_batch_meets_the_issues_conditions_on_the_restatement():
    t, ref = cases.families()
    off = t["track_offsets"].astype(np.int64)
    assert len(off) - 1 == 64 and ((off[1:] - off[:-1]) >= 2).all() and ((off[1:] - off[:-1]) <= 12).all()
    assert len(t["intrinsics"]) == 6
    clean, state = t["clean"], ref["obs_state"]
    tracks = [i for i in range(64) if clean[off[i]:off[i + 1]][:8].sum() >= 2]     # two clean observations among the candidates
    assert len(tracks) >= 48
    with_point = [i for i in tracks if ref["stats"][i, 2] == 0]
    their_clean = np.concatenate([np.flatnonzero(clean[off[i]:off[i + 1]]) + off[i] for i in tracks])
    planted = np.flatnonzero(~clean)
    got, kept, wrong = len(with_point) / len(tracks), (state[their_clean] == 2).mean(), (state[planted] == 2).mean()
    print("families: %d tracks, point %.3f, clean kept %.4f, outliers kept %.4f of %d" % (len(tracks), got, kept, wrong, len(planted)))
    assert len(planted) >= 20
    assert got >= 0.95 and kept >= 0.99 and wrong <= 0.05
    # and the points are where the scene put them: 0.5 px of noise at depth 6 .. 14 with these baselines is centimetres
    err = np.linalg.norm(ref["points"][with_point, :3] - t["X"][with_point], axis=1)
    assert np.median(err) < 0.05, np.median(err)


def test_the_twin_agrees_with_the_restatement_on_the_families_batch(exe, tmp_path):
    t, ref = cases.families()
    worst = agree(twin.run(exe, tmp_path, t), ref, t, "families")
    print("families: largest point deviation %.3g (gate %.3g)" % (worst, TOL))


def test_the_twin_agrees_on_every_seam_length(exe, tmp_path):
    t, ref = cases.seams()
    off = t["track_offsets"].astype(np.int64)
    assert tuple(off[1:] - off[:-1]) == cases.SEAM_LENGTHS
    out = twin.run(exe, tmp_path, t)
    worst = agree(out, ref, t, "seams")
    print("seams: largest point deviation %.3g (gate %.3g)" % (worst, TOL))
    assert (ref["stats"][2:, 2] == 0).all() and tuple(ref["stats"][:2, 2]) == (1, 1)
    assert ref["stats"][-1, 0] == 5000 and ref["stats"][-1, 1] > 4000


@pytest.mark.parametrize("px,rounds", [(4.0, 0), (4.0, 4), (1e-4, 2), (1e6, 2), (1.0, 1)])
def test_the_twin_agrees_under_other_rounds_and_thresholds(exe, tmp_path, px, rounds):
    t, ref = cases.decided_scene(31, np.random.default_rng(31).integers(2, 13, 24), 6, px=px, rounds=rounds, noise=0.5, outliers=0.15)
    agree(twin.run(exe, tmp_path, t, px, rounds), ref, t, (px, rounds))
    if px == 1e-4:
        assert (ref["stats"][:, 2] == 3).all()              # nothing is an inlier
    if px == 1e6:
        assert (ref["stats"][:, 1] == ref["stats"][:, 0]).all() and (ref["stats"][:, 2] == 0).all()   # everything in front is


def test_every_cause_of_an_unusable_position(exe, tmp_path):
    t, bad = cases.unusable_causes()
    ref = cases.reference(t)
    assert cases.decided(ref)
    assert sorted(np.flatnonzero(ref["obs_state"] == 0)) == bad
    assert (ref["stats"][:, 2] == 0).all() and ref["stats"][:, 0].sum() == 48 - len(bad)
    agree(twin.run(exe, tmp_path, t), ref, t, "unusable")


def test_every_no_point_reason(exe, tmp_path):
    t, reasons = cases.no_point_reasons()
    ref = cases.reference(t)
    assert cases.decided(ref)
    assert list(ref["stats"][:, 2]) == reasons
    assert not (ref["obs_state"] == 2)[int(t["track_offsets"][1]):].any()
    agree(twin.run(exe, tmp_path, t), ref, t, "reasons")


def test_candidates_that_share_a_slot(exe, tmp_path):
    t = cases.shared_slots()
    ref = cases.reference(t)
    assert cases.decided(ref)
    assert tuple(ref["stats"][0]) == (7, 7, 0, 0 << 16 | 1) and sorted(np.flatnonzero(ref["obs_state"][:27])) == [0, 3, 8, 11, 16, 24, 26]
    agree(twin.run(exe, tmp_path, t), ref, t, "slots")


def test_the_reading_rules(exe, tmp_path):
    variants = cases.reading_rules()
    outs = twin.run_calls(exe, tmp_path, [(t, 4.0, 2) for _, t in variants])
    for (name, t), out in zip(variants, outs):
        ref = cases.reference(t)
        assert cases.decided(ref), name
        agree(out, ref, t, name)
    by = dict((n, o) for (n, _), o in zip(variants, outs))
    assert (by["fewer tracks than the capacity"]["stats"][4:] == twin.FILL).all()
    assert (by["no tracks"]["stats"] == twin.FILL).all() and (by["no tracks"]["obs_state"] == twin.FILL).all()
    assert (by["no observations"]["stats"][:, 2] == 1).all()
    assert by["an inverted range"]["stats"][5, 0] == 0
    assert (by["more tracks than the capacity"]["stats"] == by["as made"]["stats"]).all()


def test_a_track_alone_equals_the_track_in_any_batch(exe, tmp_path):
    t, _ = cases.families()
    order = np.random.default_rng(5).permutation(64)
    whole, mixed = twin.run_calls(exe, tmp_path, [(t, 4.0, 2), (cases.subset(t, order), 4.0, 2)])
    for name in ("points", "stats", "err"):
        assert (mixed[name] == whole[name][order]).all(), name
    picks = [0, 17, 63]
    alone = twin.run_calls(exe, tmp_path, [(cases.subset(t, [i]), 4.0, 2) for i in picks])
    off = t["track_offsets"].astype(np.int64)
    for i, one in zip(picks, alone):
        for name in ("points", "stats", "err"):
            assert (one[name][0] == whole[name][i]).all(), (i, name)
        assert (one["obs_state"] == whole["obs_state"][off[i]:off[i + 1]]).all(), i
