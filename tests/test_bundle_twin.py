"""The host twin of bundle adjustment (tests/cpp/bundle_twin.cpp: csrc/mkd_bundle_math.h under g++) against the algorithm of
include/lf_mkd.h, restated in plain float64 numpy (tests/bundle_cases.py: restate) -- the same Levenberg-Marquardt loop and
the same preconditioned conjugate gradients, with numpy's own sums, inverses and decompositions.  No GPU.

MEASURED (this file, the scenes below): over all calls of test_the_twin_is_the_restated_algorithm the f32 outputs of the twin
and of the restatement differ in NO word (worst case 0 for the poses per value over max(1, |t|) and for the points over
max(1, |X|)); the f64 states behind them differ by about 1e-13, which the rounding to f32 absorbs.  A measured 0 gives no
bound, so the bound comes from the format: a difference in f64 can move a value across ONE rounding boundary of f32, 2^-23
relative at worst, and times 4 that is TOL = 2^-21.  The restatement flags no near-tie on any of these calls (asserted).
CG against the dense solve, the tiny scene, cg_tol = 0 and 18 steps: the first step's camera update differs from
numpy.linalg.solve by 1.46e-16 at worst (|x| <= 0.0305); times 4 and up to a power of two, DENSE_TOL = 2^-50."""
import numpy as np
import pytest

import bundle_cases as cases
import bundle_twin as bt

TOL = 2.0 ** -21
DENSE_TOL = 2.0 ** -50


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bundle_twin")
    exe = bt.build(tmp)
    return lambda scene, **kw: bt.run(exe, tmp, scene, **kw)


def rejecting():
    """strongly perturbed, a tenth of the observations wrong: under lambda0 = 1e-6 some steps are rejected"""
    return cases.build(30, cases.random_views(30, 100, 6, 2, 5), outliers=0.1, perturb=(0.02, 0.1, 0.1))


CALLS = [("realistic", cases.realistic, dict(iterations=6, cg_iterations=16)),
         ("track lengths", cases.track_lengths, {}), ("image rows", cases.image_rows, {}),
         ("2 images", lambda: cases.many_images(2), {}), ("256 images", lambda: cases.many_images(256), {}),
         ("257 images", lambda: cases.many_images(257), {}),
         ("255 tracks", lambda: cases.many_tracks(255), {}), ("256 tracks", lambda: cases.many_tracks(256), {}),
         ("257 tracks", lambda: cases.many_tracks(257), {}),
         ("mixed", cases.mixed, {}), ("garbage", cases.garbage, {}), ("tiny", cases.tiny, dict(cg_tol=0.0, cg_iterations=18)),
         ("rejecting", rejecting, dict(lambda0=1e-6, iterations=8)),
         ("cg stops at once", cases.track_lengths, dict(cg_tol=0.999)), ("one cg step", cases.mixed, dict(cg_iterations=1))]


@pytest.mark.parametrize("name,make,kw", CALLS, ids=[c[0] for c in CALLS])
def test_the_twin_is_the_restated_algorithm(twin, name, make, kw):
    s = make()
    got, want = twin(s, **kw), cases.restate(s, **{**bt.DEFAULTS, **kw})
    assert not want["near_tie"], "choose another seed: the restatement itself flags a near-tie"
    assert np.array_equal(got["trace"][:, 3:], want["trace"][:, 3:]), (got["trace"][:, 3:], want["trace"][:, 3:])
    assert np.array_equal(got["counts"], want["counts"])
    assert np.allclose(got["trace"][:, :3], want["trace"][:, :3], rtol=1e-9, atol=0)
    T = min(int(s["counts"][0]), len(s["points"]))                            # rows from T on are untouched
    assert (got["points"][T:] == bt.FILL).all()
    P, X = bt.f32(got["poses"]).astype(np.float64), bt.f32(got["points"][:T]).astype(np.float64)
    wp, wx = want["poses"].astype(np.float64), want["points"][:T].astype(np.float64)
    ok_p, ok_x = np.isfinite(wp), np.isfinite(wx)                             # (non-finite inputs are copied: compared as words)
    assert np.array_equal(got["poses"][~ok_p], want["poses"].view(np.uint32)[~ok_p])
    assert np.array_equal(got["points"][:T][~ok_x], want["points"][:T].view(np.uint32)[~ok_x])
    with np.errstate(invalid="ignore"):
        dp = np.abs(P - wp)[ok_p] / np.maximum(1.0, np.abs(wp))[ok_p]
        dx = np.abs(X - wx)[ok_x] / np.maximum(1.0, np.abs(wx))[ok_x]
    print("%s: poses %.3e points %.3e" % (name, dp.max(initial=0.0), dx.max(initial=0.0)))
    assert dp.max(initial=0.0) <= TOL and dx.max(initial=0.0) <= TOL
    state = got["obs_state"].astype(np.int64)
    state[got["obs_state"] == bt.FILL] = -1
    assert np.array_equal(state, want["obs_state"])


def test_cg_against_a_direct_solve(twin):
    s = cases.tiny()
    got = twin(s, dump=True, cg_tol=0.0, cg_iterations=18, iterations=1)
    want = cases.restate(s, cg_tol=0.0, cg_iterations=18, iterations=1, dense_first_step=True)["dense"]
    assert got["counts"][0] == 3 and got["counts"][1] == 12 and got["trace"][0, 4] == 18
    worst = np.abs(got["x"] - want).max()
    print("cg against numpy.linalg.solve: %.3e, largest |x| %.3e" % (worst, np.abs(want).max()))
    assert np.abs(want).max() > 1e-3 and worst <= DENSE_TOL


def test_the_cost_never_rises_and_a_rejected_step_changes_nothing(twin):
    got = twin(rejecting(), lambda0=1e-6, iterations=8)
    tr, words = got["trace"], got["trace_words"]
    assert (np.diff(tr[:, 0]) <= 0).all()
    rejected = np.flatnonzero(tr[:-1, 3] == 0)
    assert len(rejected) >= 2, tr[:, 3]
    for k in rejected:
        assert words[k + 1, 0] == words[k, 0] and tr[k + 1, 2] == min(8 * tr[k, 2], 2.0 ** 40)
    for k in np.flatnonzero(tr[:-1, 3] == 1):
        assert words[k + 1, 0] == words[k, 1] and tr[k + 1, 2] == max(tr[k, 2] / 4, 2.0 ** -40)
    assert got["counts"][3] == tr[:, 3].sum()


def test_recovery_on_the_realistic_scene(twin):
    """the two fixed cameras hold the truth, so the frames are aligned by them; the twin recovers what the restatement does"""
    s = cases.realistic()
    kw = dict(iterations=6, cg_iterations=16)
    got, want = twin(s, **kw), cases.restate(s, **{**bt.DEFAULTS, **kw})
    P, X = bt.f32(got["poses"]), bt.f32(got["points"])
    truth = s["truth"]["poses"]
    mine = np.array([cases.pose_error(P[i], truth[i]) for i in range(12)]).max(0)
    theirs = np.array([cases.pose_error(want["poses"][i], truth[i]) for i in range(12)]).max(0)
    before = np.array([cases.pose_error(s["poses"][i], truth[i]) for i in range(12)]).max(0)
    rms, rms_before = cases.rms_of(s, P, X), cases.rms_of(s, s["poses"], s["points"])
    print("rms %.4f -> %.4f (restatement %.4f); rotation %.2e -> %.2e (%.2e), centre %.2e -> %.2e (%.2e)" %
          (rms_before, rms, want["rms"], before[0], mine[0], theirs[0], before[1], mine[1], theirs[1]))
    assert rms <= 2 * want["rms"] and mine[0] <= 2 * theirs[0] and mine[1] <= 2 * theirs[1]
    assert want["rms"] < 0.5 * rms_before and theirs[0] < 0.5 * before[0] and theirs[1] < 0.5 * before[1]   # and that is a recovery


def test_nothing_free_copies_the_inputs_word_for_word(twin):
    s = cases.mixed()
    s["camera_fixed"][:] = 1
    s["obs_state"] = np.zeros(len(s["obs_row"]), np.uint32)
    s["poses"][4, 3], s["points"][7, 1] = np.nan, np.inf                       # copied as words too
    got = twin(s)
    assert np.array_equal(got["poses"], s["poses"].view(np.uint32)) and np.array_equal(got["points"], s["points"].view(np.uint32))
    assert got["counts"].tolist() == [0, 0, 0, 4] and not got["obs_state"].any() and not got["trace"][:, :2].any()
    none = twin(dict(s, counts=np.zeros(2, np.uint32), obs_state=None, camera_fixed=None))
    assert np.array_equal(none["poses"], s["poses"].view(np.uint32)) and (none["points"] == bt.FILL).all()
    assert none["counts"].tolist() == [5, 0, 0, 4]
