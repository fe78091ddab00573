"""CPU tests of the camera resection call's host twin (tests/cpp/resect_twin.cpp: the kernels' math header under g++) against
the float64 numpy restatement of the algorithm (tests/resect_cases.py: numpy.roots, plain sums), and of the algorithm's
recovery of known poses.  The twin is what tests/test_gpu_resect.py holds the kernels to, word for word; here the twin is held
to the algorithm.

Gates (DESIGN.md 6s has the measurements): a P3P candidate's R per entry and t / max(1, |t|) per component within SAMPLE_TOL of
numpy's; a whole call's final pose within CALL_TOL; the recovered poses within ROT_BOUND / T_BOUND of the truth."""
import numpy as np
import pytest

import resect_cases as cases
import resect_twin as twin

# Sample by sample, measured on the 4096 samples of cases.realistic() (16 images, M 44 .. 352, 256 samples each): 6.1e-7 per
# entry of R and 2.7e-6 per component of t / max(1, |t|) (u = 0 / 0-like quotients of Grunert's solution amplify the two root
# finders' last bits), none of the samples left out; 4 x 2.7e-6 = 1.1e-5, the next power of two is 2^-16 = 1.5e-5.
SAMPLE_TOL = 2.0 ** -16
# Whole calls (the f32 pose after the refit), measured over families, seams and realistic: 7.5e-9 per value over max(1, |t|)
# (one f32 ulp of a value below 1/8 where the f64 poses round apart); 4 x that is 3.0e-8, the next power of two 2^-24.
CALL_TOL = 2.0 ** -24
# Recovery on cases.realistic() (0.5 px noise, 30 % wrong, 4 px, 256 samples, 3 rounds): the numpy restatement's own largest
# errors against the truth are 8.72e-4 rad and 6.82e-3 (|t - t_true| / max(1, |t_true|)); times 2.
ROT_BOUND, T_BOUND = 2 * 8.72e-4, 2 * 6.82e-3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return twin.build(tmp_path_factory.mktemp("resect_twin"))


@pytest.fixture(scope="module")
def realistic(exe, tmp_path_factory):
    """the realistic scene, the twin's call with its candidates, and the restatement per image: computed once, not changed"""
    s = cases.realistic()
    out = twin.run(exe, tmp_path_factory.mktemp("realistic"), s, dump=True, n_samples=256, rounds=3)
    K = s["intrinsics"][0].astype(np.float64)
    ref = [cases.resect_image(cases.correspondences(s, i)[1], K, i, n_samples=256) for i in range(len(s["poses"]))]
    return s, out, ref


def agree(s, out, kw, what):
    """a twin call against the restatement, image by image; returns (largest pose deviation, images left out, images)"""
    n, worst, left = len(s["poses"]), 0.0, 0
    resect_all = bool(kw.get("flags", 0) & 1)
    for i in range(n):
        K, st = s["intrinsics"][i].astype(np.float64), out["stats"][i].astype(np.int64).tolist()
        off = s["image_offsets"].astype(np.int64)
        lo, hi = min(off[i], len(s["kps"])), min(off[i + 1], len(s["kps"]))
        state = out["row_state"][lo:max(lo, hi)]
        if not cases.candidate_image(K, s["poses"][i], resect_all):
            assert st == [0, 0, 1, cases.NONE] and (out["poses"][i] == s["poses"][i].view(np.uint32)).all(), (what, i)
            assert (out["err"][i] == 0).all(), (what, i)
            continue
        rows, cs = cases.correspondences(s, i, kw.get("deg", 0.0))
        ref = cases.resect_image(cs, K, kw.get("seed", 0) + i, kw.get("px", 4.0), kw.get("n_samples", 64), kw.get("min_inliers", 12),
                                 kw.get("rounds", 3))
        assert st[0] == ref["stats"][0] and ((state != 0) == np.isin(np.arange(lo, max(lo, hi)), rows)).all(), (what, i, "M")
        if st != ref["stats"] or ((out["row_state"][rows] == 2) != ref["inlier"]).any():
            assert ref["tie"], (what, i, st, ref["stats"])        # only a tie of the two best counts excuses an image
            left += 1
            continue
        got = twin.f32(out["poses"][i]).astype(np.float64)
        scale = max(1.0, np.linalg.norm(ref["pose"][9:]))
        dev = max(np.abs(got[:9] - ref["pose"][:9]).max(), np.abs(got[9:] - ref["pose"][9:]).max() / scale)
        worst = max(worst, float(dev))
        err = twin.f32(out["err"][i]).astype(np.float64)
        assert (np.abs(err - ref["err"]) <= 2.0 ** -20 * np.maximum(1.0, ref["err"])).all(), (what, i, err, ref["err"])
    return worst, left, n


def test_the_twin_against_numpy_sample_by_sample(realistic):
    s, out, _ = realistic
    K = s["intrinsics"][0].astype(np.float64)
    total = left = with_pose = 0
    worst_r = worst_t = 0.0
    for i in range(len(s["poses"])):
        cs = cases.correspondences(s, i)[1]
        for k in range(256):
            sm = cases.sample3(i, k, len(cs))
            got = cases.p3p(cs[sm], K) if sm else None
            cand = out["candidates"][i, 4 * k:4 * k + 4]
            total += 1
            if got and cases.unsafe_roots(got[0]):
                left += 1
                continue
            assert {j for j in range(4) if cand[j, 0] == 1} == set(got[1] if got else ()), (i, k)
            for j, (R, t) in (got[1] if got else {}).items():
                with_pose += 1
                worst_r = max(worst_r, float(np.abs(cand[j, 2:11] - R.reshape(-1)).max()))
                worst_t = max(worst_t, float(np.abs(cand[j, 11:] - t).max() / max(1.0, np.linalg.norm(t))))
    print("samples %d, left out %d, poses %d, worst R %.3g, worst t %.3g" % (total, left, with_pose, worst_r, worst_t))
    assert total >= 2000 and left <= 0.01 * total and with_pose >= total
    assert worst_r <= SAMPLE_TOL and worst_t <= SAMPLE_TOL, (worst_r, worst_t)


@pytest.mark.parametrize("name, kw", [("families", {}), ("seams", {}), ("realistic", dict(n_samples=256)),
                                      ("families", dict(rounds=0, seed=7, px=2.0, min_inliers=3))])
def test_whole_calls_against_numpy(exe, tmp_path, realistic, name, kw):
    s = realistic[0] if name == "realistic" else getattr(cases, name)()
    out = realistic[1] if name == "realistic" else twin.run(exe, tmp_path, s, **kw)
    worst, left, n = agree(s, out, kw, name)
    print("%s: worst pose deviation %.3g, left out %d of %d" % (name, worst, left, n))
    assert left < 0.05 * n and worst <= CALL_TOL, (worst, left)


def test_the_true_pose_is_a_candidate_of_every_valid_sample_without_noise(exe, tmp_path):
    # f32 keypoints and points move a projection by 2^-24 x 1280 px = 7.6e-5 px, and a minimal sample amplifies that by its
    # conditioning (the guards only refuse exactly degenerate triangles); the true pose counts as "a candidate" if one candidate
    # has EVERY correspondence within 1 px, a quarter of the default threshold: room for an amplification of 1.3e4
    s = cases.scene(5, (40, 90, 150, 33, 64, 257), noise=0.0, wrong=0.0)
    out = twin.run(exe, tmp_path, s, dump=True, px=1.0, n_samples=64, rounds=0)
    K = s["intrinsics"][0].astype(np.float64)
    valid = 0
    for i in range(len(s["poses"])):
        cs = cases.correspondences(s, i)[1]
        for k in range(64):
            sm = cases.sample3(i, k, len(cs))
            if sm is None or cases.p3p(cs[sm], K) is None:
                continue
            valid += 1
            cand = out["candidates"][i, 4 * k:4 * k + 4]
            assert ((cand[:, 0] == 1) & (cand[:, 1] == len(cs))).any(), (i, k, cand[:, :2])
    assert valid >= 6 * 60
    assert (out["stats"][:, 2] == 0).all() and (out["stats"][:, 1] == out["stats"][:, 0]).all()


def test_recovery_on_the_realistic_case(realistic):
    s, out, ref = realistic
    assert (out["stats"][:, 2] == 0).all()
    te = np.array([cases.pose_error(twin.f32(out["poses"][i]), s["truth"][i]) for i in range(len(ref))])
    ne = np.array([cases.pose_error(ref[i]["pose"], s["truth"][i]) for i in range(len(ref))])
    print("twin: %.3g rad, %.3g; numpy: %.3g rad, %.3g" % (*te.max(0), *ne.max(0)))
    assert (2 * ne.max(0) <= np.array([ROT_BOUND, T_BOUND]) * (1 + 1e-2)).all(), ne.max(0)     # the bounds are numpy's, times 2
    assert te[:, 0].max() <= ROT_BOUND and te[:, 1].max() <= T_BOUND, te.max(0)
    planes = [i for i in range(len(ref)) if i % 3 == 1]
    assert planes and (out["stats"][planes, 2] == 0).all()
    # the inliers are the clean rows, up to the few whose noise reaches 4 px and the wrong ones that land within it
    for i in range(len(ref)):
        rows = cases.correspondences(s, i)[0]
        inl = out["row_state"][rows] == 2
        assert (inl & s["clean"][rows]).sum() >= 0.98 * s["clean"][rows].sum() and (inl & ~s["clean"][rows]).sum() <= 2


def test_fewer_than_three_correspondences_and_the_sampler(exe, tmp_path):
    s = cases.scene(9, (0, 1, 2, 3), wrong=0.0)
    out = twin.run(exe, tmp_path, s, min_inliers=0)
    assert out["stats"][:3, 2].tolist() == [2, 2, 2] and (out["stats"][:3, 3] == cases.NONE).all() and (out["poses"][:3] == 0).all()
    assert out["stats"][3].tolist()[:3] == [3, 3, 0]
    assert cases.sample3(5, 9, 2) is None and sorted(cases.sample3(5, 9, 3)) == [0, 1, 2]
