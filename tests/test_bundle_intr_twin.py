"""The host twin of self-calibrating bundle adjustment (tests/cpp/bundle_intr_twin.cpp: csrc/mkd_bundle_math.h under g++)
against the algorithm of include/lf_mkd.h (lf_mkd_bundle_adjust_intrinsics_device), restated in plain float64 numpy
(tests/bundle_intr_cases.py: restate), and against the fixed-intrinsics twin where nothing is refined.  No GPU.

MEASURED (this file): over all calls of test_the_twin_is_the_restated_algorithm the f32 outputs of the twin and of the
restatement (poses, points, intrinsics, the groups' parameters, each value over max(1, |value|)) differ in NO word: the largest
deviation is 0.  Four times 0 names no power of two, so as for the fixed-intrinsics call the gate comes from the format: a
difference in f64 can move a value across ONE rounding boundary of f32, 2^-23 relative at worst, times 4: TOL = 2^-21, the
existing call's gate.  The restatement flags no near-tie on these calls (asserted).
CG against the dense solve, tiny() with two groups, refine 3, cg_tol 0 and 256 steps: the first step differs from
numpy.linalg.solve on the full damped normal equations (cameras, groups, points) by 2.0e-15 at worst in a camera's six
(|x| <= 0.05) and 7.6e-14 in a group's three (|x| <= 2.35: the principal point moves by pixels); 4 x 7.6e-14 = 3.0e-13 and up to
a power of two, DENSE_TOL = 2^-41 (the fixed-intrinsics call: 2^-50 at 1.5e-16, on values 80 times smaller).
RECOVERY, realistic() (400 tracks, 12 cameras, 0.5 px noise, 5 % outliers, cameras 0 and 1 held at the truth), 12 iterations,
cg_iterations 64, cg_tol 1e-3 (CG stops by tolerance in every iteration: at most 30 steps), |s scale - 1| of the twin / of the
restatement with a dense solve in every iteration: focal x 0.95 at 4 px 3.99e-3 / 3.99e-3; x 1.10 at 4 px 4.44e-3 / 4.91e-3;
x 1.05 with the principal point off by (12, -9) at 8 px 2.47e-4 / 2.47e-4 and 1.24 px / 1.24 px.  The bound is 4 x the dense
figure.  The rms with the intrinsics fixed is 1.04, 1.49 and 1.09 px against 0.70, 0.66 and 0.60 px refined."""
import numpy as np
import pytest

import bundle_cases as cases
import bundle_intr_cases as ic
import bundle_intr_twin as bit
import bundle_twin as bt

TOL = 2.0 ** -21
DENSE_TOL = 2.0 ** -41
N = 12                                   # cameras of realistic()


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bundle_intr_twin")
    return tmp, bit.build(tmp), bt.build(tmp)


@pytest.fixture(scope="module")
def twin(programs):
    tmp, exe, _ = programs
    return lambda scene, **kw: bit.run(exe, tmp, scene, **kw)


@pytest.fixture(scope="module")
def fixed_twin(programs):
    tmp, _, exe = programs
    return lambda scene, **kw: bt.run(exe, tmp, scene, **kw)


def fixed_only_group():
    """group 1 is cameras 0 and 1, both held by camera_fixed: it is free all the same and its focal is found"""
    g = np.zeros(N, np.uint32)
    g[:2] = 1
    return ic.with_groups(cases.realistic(), g, 2, scale=0.98)


def unregistered_only_group():
    """group 1 is image 2 alone, whose pose is all zero: the group has no active observation and is not free"""
    s = cases.realistic()
    s["poses"][2] = 0
    g = np.zeros(N, np.uint32)
    g[2] = 1
    return ic.with_groups(s, g, 2, scale=1.02)


def all_fixed():
    """calibration under known poses: every camera held at the truth, only points and the focal move"""
    s = cases.build(3, cases.random_views(3, 400, N), noise=0.5, outliers=0.05, fixed=tuple(range(N)))
    return ic.with_groups(s, None, 1, scale=1.04)


CALLS = [("refine 1", lambda: ic.with_groups(cases.realistic(), scale=0.97), dict(refine=1)),
         ("refine 2", lambda: ic.with_groups(cases.realistic(), shift=(5, -4)), dict(refine=2)),
         ("refine 3", lambda: ic.with_groups(cases.realistic(), scale=1.03, shift=(5, -4)), dict(refine=3, px=8.0)),
         ("one group by a map", lambda: ic.with_groups(cases.realistic(), np.zeros(N), 1, scale=0.97), dict(refine=1)),
         ("two interleaved groups", lambda: ic.with_groups(cases.realistic(), np.arange(N) % 2, 2, scale=0.97), dict(refine=3, px=6.0)),
         ("a group per image", lambda: ic.with_groups(cases.realistic(), np.arange(N), N, scale=1.02), dict(refine=1)),
         ("an id out of range", lambda: ic.with_groups(cases.realistic(), np.where(np.arange(N) % 3 == 0, 7, 0), 1, scale=0.98), dict(refine=1)),
         ("a fixed-only group", fixed_only_group, dict(refine=1)),
         ("an unregistered-only group", unregistered_only_group, dict(refine=3, px=6.0)),
         ("all cameras fixed", all_fixed, dict(refine=1, iterations=6)),
         ("track lengths", lambda: ic.with_groups(cases.track_lengths(), np.arange(9) % 2, 2, scale=1.02), dict(refine=1)),
         ("mixed", lambda: ic.with_groups(cases.mixed(), np.arange(8) % 3, 3, scale=0.99), dict(refine=3, px=6.0)),
         ("garbage", lambda: ic.with_groups(cases.garbage(), np.arange(7) % 2, 2, scale=1.01), dict(refine=1)),
         ("257 images, one group", lambda: ic.with_groups(cases.many_images(257), None, 1, scale=1.01), dict(refine=1)),
         ("nothing refined", lambda: ic.with_groups(cases.realistic(), np.arange(N) % 2, 2), dict(refine=0))]


@pytest.mark.parametrize("name,make,kw", CALLS, ids=[c[0] for c in CALLS])
def test_the_twin_is_the_restated_algorithm(twin, name, make, kw):
    s = make()
    got, want = twin(s, **kw), ic.restate(s, **{**bit.DEFAULTS, **kw})
    assert not want["near_tie"], "choose another seed: the restatement itself flags a near-tie"
    assert np.array_equal(got["trace"][:, 3:], want["trace"][:, 3:]), (got["trace"][:, 3:], want["trace"][:, 3:])
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.allclose(got["trace"][:, :3], want["trace"][:, :3], rtol=1e-9, atol=0)
    T = min(int(s["counts"][0]), len(s["points"]))                            # rows from T on are untouched
    assert (got["points"][T:] == bit.FILL).all()
    worst = 0.0
    for key, rows in (("poses", slice(None)), ("points", slice(0, T)), ("intrinsics", slice(None)), ("groups", slice(None))):
        words, ref = got[key][rows], want[key][rows]
        a, b = bit.f32(words).astype(np.float64), ref.astype(np.float64)
        ok = np.isfinite(b)                                                   # (non-finite inputs are copied: compared as words)
        assert np.array_equal(words[~ok], ref.view(np.uint32)[~ok]), key
        with np.errstate(invalid="ignore"):
            d = (np.abs(a - b)[ok] / np.maximum(1.0, np.abs(b))[ok]).max(initial=0.0)
        worst = max(worst, d)
        assert d <= TOL, (key, d)
    print("%s: largest deviation %.3e, groups %s" % (name, worst, want["groups"][:2].tolist()))
    state = got["obs_state"].astype(np.int64)
    state[got["obs_state"] == bit.FILL] = -1
    assert np.array_equal(state, want["obs_state"])


def test_the_group_rules_of_the_calls_above(twin):
    """what each of the group cases is there to show, on the twin's own outputs"""
    r = twin(fixed_only_group(), refine=1, iterations=8, cg_iterations=32, cg_tol=0.01)
    g = bit.f32(r["groups"])
    assert r["counts"][4] == 2 and abs(g[1, 0] * 0.98 - 1) < 0.5 * 0.02                      # the fixed cameras' lens moved home
    s = unregistered_only_group()
    r = twin(s, refine=3, px=6.0)
    g = bit.f32(r["groups"])
    assert r["counts"][4] == 1 and g[1].tolist() == [1.0, 0.0, 0.0] and np.array_equal(r["intrinsics"][2], s["intrinsics"].view(np.uint32)[2])
    s = ic.with_groups(cases.realistic(), np.where(np.arange(N) % 3 == 0, 7, 0), 1, scale=0.98)
    r = twin(s, refine=1)
    out = np.arange(N) % 3 == 0
    assert np.array_equal(r["intrinsics"][out], s["intrinsics"].view(np.uint32)[out]) and (r["intrinsics"][~out, 0] != s["intrinsics"].view(np.uint32)[~out, 0]).all()
    r = twin(all_fixed(), refine=1, iterations=6)
    assert r["counts"][0] == 0 and r["counts"][4] == 1 and abs(bit.f32(r["groups"])[0, 0] * 1.04 - 1) < 0.5 * 0.04
    # refine 2 keeps s, refine 1 keeps (dx, dy), and the aspect ratio of the input survives
    r = twin(ic.with_groups(cases.realistic(), shift=(5, -4)), refine=2)
    assert bit.f32(r["groups"])[0, 0] == 1.0 and np.array_equal(r["intrinsics"][:, :2], cases.realistic()["intrinsics"].view(np.uint32)[:, :2])
    r = twin(ic.with_groups(cases.realistic(), scale=0.97), refine=1)
    K = bit.f32(r["intrinsics"]).astype(np.float64)
    assert bit.f32(r["groups"])[0, 1:].tolist() == [0.0, 0.0] and np.allclose(K[:, 0] / K[:, 1], 800.0 / 790.0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("make", (cases.realistic, cases.track_lengths, cases.mixed), ids=("realistic", "track_lengths", "mixed"))
def test_nothing_refined_is_the_fixed_intrinsics_twin_word_for_word(twin, fixed_twin, make):
    s = make()
    n = len(s["intrinsics"])
    want = fixed_twin(s)
    for groups in (dict(), dict(camera_group=np.arange(n, dtype=np.uint32) % 2, n_groups=2)):
        got = twin(dict(s, **groups), refine=0)
        for k in ("poses", "points", "obs_state"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["trace_words"][:, :8], want["trace_words"]) and not got["trace"][:, 8].any()
        assert np.array_equal(got["counts"][:4], want["counts"]) and got["counts"][4] == 0
        assert np.array_equal(got["intrinsics"], np.asarray(s["intrinsics"], np.float32).view(np.uint32))
        assert (bit.f32(got["groups"]) == [1.0, 0.0, 0.0]).all()


def test_cg_against_a_direct_solve(twin):
    s = ic.with_groups(cases.tiny(), np.arange(5) % 2, 2, scale=1.01, shift=(2, -1))
    kw = dict(refine=3, iterations=1, cg_iterations=256, cg_tol=0.0)
    got = twin(s, dump=True, **kw)
    dc, dk = ic.restate(s, dense_first_step=True, **{**bit.DEFAULTS, **kw})["dense"]
    assert got["counts"][0] == 3 and got["counts"][1] == 12 and got["counts"][4] == 2
    worst_c, worst_k = np.abs(got["x"] - dc).max(), np.abs(got["xg"] - dk).max()
    print("cg against numpy.linalg.solve: cameras %.3e (largest |x| %.3e), groups %.3e (largest |x| %.3e), %d steps" %
          (worst_c, np.abs(dc).max(), worst_k, np.abs(dk).max(), got["trace"][0, 4]))
    assert np.abs(dc).max() > 1e-3 and np.abs(dk).max() > 1e-3 and max(worst_c, worst_k) <= DENSE_TOL


RECOVERY = dict(iterations=12, cg_iterations=64, cg_tol=1e-3)


def _recover(twin, fixed_twin, scale, shift, refine, px):
    s = ic.with_groups(cases.realistic(), scale=scale, shift=shift)
    kw = dict(RECOVERY, refine=refine, px=px)
    got = twin(s, **kw)
    ref = ic.restate(s, dense=True, **{**bit.DEFAULTS, **kw})
    assert (got["trace"][:, 4] < RECOVERY["cg_iterations"]).all(), "CG must stop by its tolerance"
    g, gr = bit.f32(got["groups"]).astype(np.float64), ref["groups"].astype(np.float64)
    mine, theirs = ic.focal_error(scale, g)[0], ic.focal_error(scale, gr)[0]
    pp_mine, pp_theirs = np.abs(g[0, 1:] + shift).max(), np.abs(gr[0, 1:] + shift).max()
    fx = fixed_twin(s, **{k: v for k, v in kw.items() if k != "refine"})
    rms = cases.rms_of(dict(s, intrinsics=bit.f32(got["intrinsics"])), bit.f32(got["poses"]), bit.f32(got["points"]), px)
    rms_fixed = cases.rms_of(s, bit.f32(fx["poses"]), bit.f32(fx["points"]), px)
    print("focal x%.2f shift %s refine %d: |s scale - 1| twin %.3e dense %.3e; principal point twin %.3f px dense %.3f px; rms %.4f "
          "against %.4f with the intrinsics fixed; CG steps %s" % (scale, shift, refine, mine, theirs, pp_mine, pp_theirs, rms, rms_fixed,
                                                                   got["trace"][:, 4].astype(int).tolist()))
    return mine, theirs, pp_mine, pp_theirs, rms, rms_fixed


@pytest.mark.parametrize("scale", (0.95, 1.10))
def test_the_focal_length_is_recovered(twin, fixed_twin, scale):
    mine, theirs, _, _, rms, rms_fixed = _recover(twin, fixed_twin, scale, (0.0, 0.0), 1, 4.0)
    assert mine <= 4 * theirs
    assert theirs < 0.5 * abs(scale - 1)                                      # and the reference itself is a recovery
    assert rms < rms_fixed


def test_focal_length_and_principal_point_are_recovered(twin, fixed_twin):
    mine, theirs, pp_mine, pp_theirs, rms, rms_fixed = _recover(twin, fixed_twin, 1.05, (12.0, -9.0), 3, 8.0)
    assert mine <= 4 * theirs and pp_mine <= 4 * pp_theirs
    assert theirs < 0.5 * 0.05 and pp_theirs < 0.5 * 9                        # and the reference itself is a recovery
    assert rms < rms_fixed


def rejecting():
    """strongly perturbed, a tenth of the observations wrong, the focal 15 % off: under lambda0 = 1e-6 steps are rejected"""
    s = cases.build(31, cases.random_views(31, 100, 6, 2, 5), outliers=0.1, perturb=(0.02, 0.1, 0.1))
    return ic.with_groups(s, np.arange(6) % 2, 2, scale=1.15)


def test_the_cost_never_rises_and_a_rejected_step_changes_nothing(twin):
    s = rejecting()
    kw = dict(refine=3, px=4.0, lambda0=1e-6, iterations=8)
    got = twin(s, **kw)
    tr, words = got["trace"], got["trace_words"]
    assert (np.diff(tr[:, 0]) <= 0).all()
    rejected = np.flatnonzero(tr[:-1, 3] == 0)
    assert len(rejected) >= 2, tr[:, 3]
    for k in rejected:
        assert words[k + 1, 0] == words[k, 0] and tr[k + 1, 2] == min(8 * tr[k, 2], 2.0 ** 40)
    for k in np.flatnonzero(tr[:-1, 3] == 1):
        assert words[k + 1, 0] == words[k, 1] and tr[k + 1, 2] == max(tr[k, 2] / 4, 2.0 ** -40)
    assert got["counts"][3] == tr[:, 3].sum()
    # a call that ends on rejected steps alone returns the state it had before them
    k = int(np.flatnonzero(tr[:, 3] == 0)[0])
    assert k >= 1 and tr[k:k + 2, 3].tolist() == [0, 0]
    a, b, c = (twin(s, **dict(kw, iterations=n)) for n in (k, k + 1, k + 2))
    for key in ("poses", "points", "intrinsics", "groups", "obs_state"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key


def mirrored():
    """every keypoint reflected through its image's principal point, every camera held, everything an inlier: the best focal
    scale is -1, which one Gauss-Newton step from s = 1 under a tiny lambda all but reaches"""
    s = cases.build(41, cases.random_views(41, 60, 5, 3, 5), noise=0.0, perturb=(0.0, 0.0, 0.0), fixed=tuple(range(5)), extra_rows=0)
    s["kps"][:, 0] = 2 * cases.K0[2] - s["kps"][:, 0]
    s["kps"][:, 1] = 2 * cases.K0[3] - s["kps"][:, 1]
    return ic.with_groups(s, None, 1)


def test_a_step_to_a_focal_scale_that_is_not_positive_is_rejected(twin):
    s = mirrored()
    got = twin(s, dump=True, refine=1, px=3000.0, lambda0=1e-9, iterations=3, cg_iterations=64, cg_tol=1e-6)
    tr = got["trace"]
    assert got["xg"][0, 0] >= 1.0, got["xg"]                                  # the first step would take s to 1 - x <= 0 ...
    assert tr[0, 1] < tr[0, 0] and tr[0, 3] == 0                              # ... to a LOWER cost, and is rejected all the same
    assert tr[1, 2] == 8 * tr[0, 2] and got["trace_words"][1, 0] == got["trace_words"][0, 0]
    K, g = bit.f32(got["intrinsics"]), bit.f32(got["groups"])
    assert np.isfinite(K).all() and (K[:, :2] > 0).all() and np.isfinite(g).all() and g[0, 0] > 0
    assert np.isfinite(bit.f32(got["points"])[:, :3]).all()
    one = twin(s, refine=1, px=3000.0, lambda0=1e-9, iterations=1, cg_iterations=64, cg_tol=1e-6)
    assert np.array_equal(one["intrinsics"], s["intrinsics"].view(np.uint32)) and bit.f32(one["groups"])[0].tolist() == [1.0, 0.0, 0.0]
    assert np.array_equal(one["points"], s["points"].view(np.uint32)[:, :]) or np.array_equal(bit.f32(one["points"])[:, :3], s["points"][:, :3])
