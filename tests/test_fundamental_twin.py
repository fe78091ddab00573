"""The fundamental-matrix verifier's host twin (tests/cpp/fundamental_twin.cpp: the kernel's own math header compiled by g++)
against the float64 restatement (tests/fundamental_ref.py), sample by sample, on the CPU.  The device is held to the twin
bit for bit by tests/test_gpu_fundamental_exact.py; this module is what ties the twin, and so the kernel's arithmetic, to
the algorithm of include/lf_mkd.h.

Decisions f32 and f64 may take differently.  A sample is EXCUSED from the comparison of validity, of the number of
candidates and of the candidates themselves when the restatement itself is near one of its decisions:
  * a pivot within a factor NEAR_PIVOT = 2 of PIVOT_REL times the first pivot (a pivot that small is the difference of
    entries ~1e5 times larger, so f32 knows it to a few per cent only);
  * |c3| / max(|c0|, |c1|, |c2|) at most NEAR_LEAD = 16 times LEAD_REL (c3 is a 3x3 determinant of differences: at 2^-20
    of the other coefficients it is rounding noise in f32);
  * the cubic's value at one of the derivative's roots, relative to the sum of its terms' magnitudes there, at most
    NEAR_END = 2^-16 (a double root: a pair of real roots appears or disappears with the last bits of the coefficients).
The share of excused samples is capped: 2 % per problem (5 of 256 samples), none for M = 7 of the general family.
plane_exact has its own cap, 80 of 256: its matches satisfy one homography exactly, every 7 x 9 system has rank 6 and
the seventh pivot is the rounding noise of the f32 inputs, which scatters around PIVOT_REL; 65 samples fall within the
factor 2 on these seeds and the cap leaves a quarter's room for another platform's libm in the generator.  The samples of
plane_exact that are not excused agree like any other's (nearly all invalid on both sides, 7 candidates valid on both).
Measured shares on these seeds, as excused / 256: 1 for sideways M = 1000, threshold_min and threshold_max; 3 and 2 for
the NaN in a.x and b.x (no candidate either way); 65 for plane_exact; 0 for every other problem.  No sample, excused or
not, disagreed.  (A near tie between two pivots would be a fourth such decision; fundamental_ref reports it as pivot_tie,
no sample here comes within 1e-5 of one, and it is not excused.)

Every candidate both sides hold, in samples that are not excused:
  * count: differs from the restatement's by at most the number of matches the two precisions may decide differently:
    fundamental_cases.undecided = the suite's 5 % Sampson band, or within f32's resolution of the test in pixel
    coordinates (f32_band: 16 roundings of 2^-24 of sum |b_j F_jk a_k|, derived there).  The second adds nothing for
    coordinates in a frame at the origin (measured: 0 matches on the families).  It is what describes the two edge cases
    that the 5 % band cannot: large_offset (coordinates near 1e5 px; F's constant entry is ~1e10 times its leading ones:
    the f32 band holds 95 of 200 matches on average, the counts differ by up to 12) and threshold_min (threshold^2 =
    2^-126: the band is the sample's own 7 matches, whose error is rounding noise in either precision; restatement
    counts 1 .. 4, twin counts 0).  include/lf_mkd.h states both limits;
  * annihilation: max_j |A_j . fn| / (|A_j| |fn|) over the sample's own 7 design rows, fn taken as float64;
  * rank: |det fn| / |fn|^3.
  The last two are bounded at 4x the twin's worst value on these fixed seeds (f32 elimination of a conditioned 7 x 9
  system: no tighter claim is derivable).  Measured worsts over all problems: annihilation twin 1.24e-7 (restatement
  3.9e-16), rank twin 1.37e-6 (restatement 1.5e-15), hence ANNIHILATION = 4.96e-7 and RANK = 5.48e-6.  (Each test prints
  its own worsts.)

Whole calls, every problem: the assertions tests/test_gpu_fundamental.py makes of the device, with `undecided` as the band:
band slack, the near-tie rule, the planted inliers' median epipolar distance to the ground truth below 0.5 px (families,
M >= 50), and 0.05 px between the epipolar lines of the inliers.  That module measures the last as the lines' heights at
x = 0, 512, 1024 and applies it to the general family at M >= 50; it is kept for exactly those here.  Elsewhere that
height is ill conditioned (a steep line under forward motion, a line through one of only 7 or 8 matches: 0.06 to 1.5 px,
1050 px at threshold_max, between F's whose inlier sets, counts and costs are identical), so the other problems take a
weaker form of it: b's distance to its own epipolar line under the two F's agrees within 0.05 px (measured worst
0.0016 px).  That sees a line that shifts at the match, not one that turns about it; what pins the lines' directions
there is the bit-for-bit comparison with the device and the ground-truth distance above."""
import numpy as np
import pytest

import fundamental_cases as fc
import fundamental_ref as ref
import fundamental_twin as ft
from fundamental_cases import FAMILIES, THR, undecided
from test_gpu_fundamental import _line_gap

N_HYP = 256
SEED = 17
NEAR_PIVOT, NEAR_LEAD, NEAR_END = 2.0, 16.0, 2.0 ** -16
ANNIHILATION, RANK = 4.96e-7, 5.48e-6
CAP = 5                      # 2 % of 256 samples
CAP_PLANE_EXACT = 80         # plane_exact's own cap (see above)


TRUTH = {}     # the families' ground truth: noise-free points and the planted inliers


def _problems():
    """{name: (ka, kb, match, threshold)}: every family at M = 7, 8, 50, 1000, the edge cases, the non-finite rows."""
    out = {}
    for fam in FAMILIES:
        for m in (7, 8, 50, 1000):
            ka, kb, mt, info = fc.two_view(m, 0.0 if m <= 8 else 0.4, 500 + m, fam)
            out[f"{fam}-{m}"] = (ka, kb, mt, THR)
            TRUTH[f"{fam}-{m}"] = info
    for name, ka, kb, mt, thr in fc.edge_cases():
        out[name] = (ka, kb, mt, thr)
    for bad, tag in ((np.nan, "nan"), (np.inf, "posinf"), (-np.inf, "neginf")):
        for i, (ka, kb, mt) in enumerate(fc.non_finite(bad)):
            out[f"{tag}_{('ax', 'ay', 'bx', 'by')[i]}"] = (ka, kb, mt, THR)
    return out


PROBLEMS = _problems()
NON_FINITE = tuple(n for n in PROBLEMS if n.split("_")[0] in ("nan", "posinf", "neginf"))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """The twin's results for every problem, from one build and one run of the program: {(name, flags): result}."""
    tmp = tmp_path_factory.mktemp("fundamental_twin")
    exe = ft.build(tmp)
    keys = [(n, fl) for n in PROBLEMS for fl in (ft.NO_REFINE, 0)]
    calls = [ft.Call(*PROBLEMS[n][:3], SEED, N_HYP, PROBLEMS[n][3], fl, records=fl == ft.NO_REFINE) for n, fl in keys]
    res = ft.run_calls(exe, calls, tmp)
    out = {k: r[0] for k, r in zip(keys, res)}
    out["exe"], out["tmp"] = exe, tmp
    return out


_REF = {}


def _restatement(name, flags):
    """ref.verify of a problem, computed once."""
    if (name, flags) not in _REF:
        ka, kb, mt, thr = PROBLEMS[name]
        with np.errstate(all="ignore"):
            _REF[name, flags] = ref.verify(ka, kb, mt, n_hyp=N_HYP, thr=thr, seed=SEED, flags=flags)
    return _REF[name, flags]


def _near(info):
    """The stated margins of a decision the restatement is within in this sample: a set of "pivot", "lead", "end"."""
    ratio = info.get("pivot_ratio", 1.0)
    why = set()
    if ref.PIVOT_REL / NEAR_PIVOT < ratio < ref.PIVOT_REL * NEAR_PIVOT:
        why.add("pivot")
    if info.get("lead", np.inf) <= NEAR_LEAD * ref.LEAD_REL:
        why.add("lead")
    if info.get("end_value", 1.0) <= NEAR_END:
        why.add("end")
    return why


def _annihilation(rows, fn):
    fn = np.asarray(fn, np.float64).reshape(9)
    return float(np.max(np.abs(rows @ fn) / (np.linalg.norm(rows, axis=1) * np.linalg.norm(fn))))


def _rank(fn):
    fn = np.asarray(fn, np.float64).reshape(3, 3)
    return float(abs(np.linalg.det(fn)) / np.linalg.norm(fn) ** 3)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_every_sample_against_the_restatement(twin, name):
    ka, kb, mt, thr = PROBLEMS[name]
    res = twin[name, ft.NO_REFINE]
    recs, pair = res["records"], res["pair"]
    with np.errstate(all="ignore"):
        prob = ref.Problem(ka, kb, mt)
    assert pair.m == prob.m and np.array_equal(pair.rows, prob.rows)
    an = np.stack([pair.xn, pair.yn], axis=1).astype(np.float64)     # the twin's own normalised coordinates
    bn = np.stack([pair.un, pair.vn], axis=1).astype(np.float64)
    excused = compared = 0
    worst = {"annihilation twin": 0.0, "annihilation restatement": 0.0, "rank twin": 0.0, "rank restatement": 0.0}
    for k in range(N_HYP):
        pos = ref.sample(SEED, k, prob.m)
        if pos is None:
            assert recs[k]["valid"] == 0 and (recs[k]["pos"] == ref.INVALID).any(), k
            continue
        assert recs[k]["pos"].tolist() == pos, k
        info = {}
        with np.errstate(all="ignore"):
            cands = prob.candidates(SEED, k, info)
        why = _near(info)
        if why:
            excused += 1
            continue
        want = sum(1 << j for j in range(3) if cands[j] is not None)
        assert int(recs[k]["valid"]) == want, (k, want, int(recs[k]["valid"]), info)
        rows_t, rows_r = ref.design_rows(an[pos], bn[pos]), ref.design_rows(prob.an[pos], prob.bn[pos])
        for j in range(3):
            if cands[j] is None:
                assert recs[k]["count"][j] == ref.INVALID
                continue
            f, fn = cands[j]
            compared += 1
            slack = int(undecided(prob, f, thr).sum())
            assert abs(int(prob.inliers(f, thr).sum()) - int(recs[k]["count"][j])) <= slack, (k, j, slack)
            a_t, r_t = _annihilation(rows_t, recs[k]["fn"][j]), _rank(recs[k]["fn"][j])
            worst["annihilation twin"] = max(worst["annihilation twin"], a_t)
            worst["rank twin"] = max(worst["rank twin"], r_t)
            worst["annihilation restatement"] = max(worst["annihilation restatement"], _annihilation(rows_r, fn))
            worst["rank restatement"] = max(worst["rank restatement"], _rank(fn))
            assert a_t <= ANNIHILATION, (k, j, a_t)
            assert r_t <= RANK, (k, j, r_t)
    print(f"[fundamental twin] {name}: M = {prob.m}, {excused} of {N_HYP} samples excused, "
          f"{compared} candidates compared; worst {worst}")
    assert excused <= (0 if name == "general-7" else CAP_PLANE_EXACT if name == "plane_exact" else CAP), excused
    if name in NON_FINITE or name in ("collinear_a", "identical_rows", "seven_repeated"):
        assert compared == 0 and not recs["valid"].any()       # no valid candidate on either side
    elif name != "plane_exact":
        assert compared > N_HYP // 2


def _root_tolerance(c, r):
    """How far an f32 root finder may be from the exact root r of the cubic c (c0 .. c3): the sign of p is known only
    where |p| exceeds Horner's rounding error, 3 fused steps, each at most 2^-24 of the terms' magnitudes S(r); with the
    coefficients' own rounding to f32 that is 8 * 2^-24 S(r) / |p'(r)|, plus 2 ulp of r for the final rounding."""
    s = sum(abs(c[i]) * abs(r) ** i for i in range(4))
    dp = abs(3 * c[3] * r * r + 2 * c[2] * r + c[1])
    return 8 * 2.0 ** -24 * s / dp + 2 * 2.0 ** -23 * abs(r)


def _cubic(roots, lead=1.0):
    """(c0, c1, c2, c3) as f32 of lead * prod (x - r)"""
    return np.asarray((np.poly(roots) * lead)[::-1], np.float32)


def test_cubic_roots_alone(twin):
    big_root = 4.0e5      # c3 = 1 / big_root against |c0| = 2.1: |c3| / big = 1.2e-6, just above 2^-20 = 9.5e-7
    planted = {
        "three distinct": _cubic([-2.0, 0.5, 1.0]),
        "three distinct, scaled": _cubic([-30.0, 0.125, 7.0], -3.0e-3),
        "one real root": _cubic([1.5, 0.25 + 1.0j, 0.25 - 1.0j]).real,
        "one real root, monotone": np.array([1.0, 3.0, 0.0, 1.0], np.float32),      # x^3 + 3 x + 1: the derivative has no root
        "close pair far below a huge root": _cubic([1.0, 1.05, big_root], 1.0 / big_root),
    }
    names = list(planted)
    n, x = ft.cubic_roots(twin["exe"], twin["tmp"], np.stack([planted[k] for k in names]))
    for i, name in enumerate(names):
        c = planted[name].astype(np.float64)
        exact = np.sort([r.real for r in np.roots(c[::-1]) if abs(r.imag) < 1e-9 * max(1.0, abs(r))])
        assert n[i] == len(exact), (name, n[i], exact)
        assert (np.diff(x[i, :n[i]]) > 0).all() and (x[i, n[i]:] == 0).all(), (name, x[i])
        for got, r in zip(x[i], exact):
            assert abs(float(got) - r) <= _root_tolerance(c, r), (name, float(got), r, _root_tolerance(c, r))
        assert [float(v) for v in x[i, :n[i]]] == pytest.approx(ref.cubic_roots(*c), rel=1e-4, abs=1e-6), name
    # a double root: (x - 1)^2 (x + 2).  The simple root is always found; the double one may show as two roots or none
    n, x = ft.cubic_roots(twin["exe"], twin["tmp"], [_cubic([1.0, 1.0, -2.0])])
    assert n[0] in (1, 3) and abs(float(x[0, 0]) + 2.0) <= 1e-6 and all(abs(float(v) - 1.0) < 2e-3 for v in x[0, 1:n[0]])
    # a root at the bracket's end.  R = 1 + big / |c3| is Cauchy's bound, which no root attains; x^3 - A x^2 comes within one
    # unit of it (roots 0, 0 and A; R = A + 1), and its mirror image does at -R
    big_a = 2.0 ** 19
    n, x = ft.cubic_roots(twin["exe"], twin["tmp"], [[0, 0, -big_a, 1], [0, 0, big_a, 1]])
    assert n[0] >= 1 and float(x[0, n[0] - 1]) == big_a and n[1] >= 1 and float(x[1, 0]) == -big_a, (n, x)
    # the leading coefficient at the threshold: big = 1, |c3| one ulp above and at 2^-20 (the rule is |c3| > 2^-20 big)
    lead = np.float32(2.0 ** -20)
    above = np.nextafter(lead, np.float32(1))
    n, x = ft.cubic_roots(twin["exe"], twin["tmp"], [[-0.5, 1, 0.25, above], [-0.5, 1, 0.25, lead], [-0.5, 1, 0.25, -lead],
                                                     [-0.5, 1, 0.25, -above]])
    assert n[1] == 0 and n[2] == 0 and (x[1:3] == 0).all(), (n, x)
    for i in (0, 3):
        c = np.array([-0.5, 1, 0.25, [above, 0, 0, -above][i]], np.float64)
        exact = np.sort(np.roots(c[::-1]).real)
        assert n[i] == 3, (i, n[i], x[i])
        for got, r in zip(x[i], exact):
            assert abs(float(got) - r) <= _root_tolerance(c, r), (i, float(got), r)
    # a coefficient that is not finite: no root, whichever it is
    bad = [[1.0, -2.0, 0.5, 1.0] for _ in range(8)]
    for i in range(4):
        bad[i][i], bad[4 + i][i] = np.nan, np.inf
    n, x = ft.cubic_roots(twin["exe"], twin["tmp"], bad)
    assert (n == 0).all() and (x == 0).all()


def test_null_space_takes_the_first_pivot_on_a_tie(twin):
    """Row 0 holds the two largest entries, equal, in columns 0 and 1: the rule takes column 0, so that columns 1 and 8 stay
    free (F1 has its 1 in column 1).  Taking the later one would free column 0 instead."""
    a = np.zeros((7, 9))
    a[0, :3] = 4.0, 4.0, 1.0
    for r in range(1, 7):         # rows 1 .. 6 take columns 2 .. 7 and leave columns 0 and 1 alone
        a[r, r + 1] = 2.0 - 0.125 * r
        a[r, 2 + r % 6], a[r, 8] = a[r, 2 + r % 6] + 0.25 * r, 0.5 + 0.0625 * r
    ok, f1, f2 = ft.null_space(twin["exe"], twin["tmp"], [a, -a, a[:, ::-1]])
    want = ref.null_space(a)
    assert ok[0] and f1[0, 1] == 1.0 and f2[0, 1] == 0.0 and f1[0, 8] == 0.0 and f2[0, 8] == 1.0, (f1[0], f2[0])
    assert np.allclose(f1[0], want[0], rtol=1e-5, atol=1e-6) and np.allclose(f2[0], want[1], rtol=1e-5, atol=1e-6)
    assert np.abs(a @ f1[0].astype(np.float64)).max() < 1e-5 and np.abs(a @ f2[0].astype(np.float64)).max() < 1e-5
    assert ok[1] and np.array_equal(f1[1], f1[0]) and np.array_equal(f2[1], f2[0])     # the sign does not matter
    # mirrored columns: the tie is between columns 8 and 7 now and column 7 comes first
    want = ref.null_space(a[:, ::-1])
    assert ok[2] and np.allclose(f1[2], want[0], rtol=1e-5, atol=1e-6) and np.allclose(f2[2], want[1], rtol=1e-5, atol=1e-6)
    assert f1[2, 0] == 1.0 and f2[2, 8] == 1.0 and f1[2, 8] == 0.0, (f1[2], f2[2])
    # a system of rank 6 is refused
    b = a.copy()
    b[6] = b[5]
    assert not ft.null_space(twin["exe"], twin["tmp"], [b])[0][0] and ref.null_space(b) is None


def _invalid(res, m, na):
    return (res["stats"].tolist() == [0, 0, ref.INVALID, m] and (res["F"] == 0).all() and (res["verified"] == -1).all()
            and len(res["verified"]) == na)


WHOLE = list(PROBLEMS)


def _point_gap(prob, f1, f2, mask):
    """Largest difference, over the masked matches, between b's distances to its epipolar line under F1 and under F2."""
    if not mask.any():
        return 0.0
    a = np.concatenate([prob.a[mask], np.ones((int(mask.sum()), 1))], axis=1)
    b = np.concatenate([prob.b[mask], np.ones((int(mask.sum()), 1))], axis=1)
    d = []
    for f in (f1, f2):
        l = a @ np.asarray(f, np.float64).reshape(3, 3).T
        d.append(np.abs((b * l).sum(axis=1)) / np.hypot(l[:, 0], l[:, 1]))
    return float(np.abs(d[0] - d[1]).max())


@pytest.mark.parametrize("name", WHOLE)
def test_whole_call_without_refit(twin, name):
    """What tests/test_gpu_fundamental.py::test_candidates_match_the_restatement asserts of the device, of the twin."""
    ka, kb, mt, thr = PROBLEMS[name]
    res, want = twin[name, ft.NO_REFINE], _restatement(name, ft.NO_REFINE)
    F, ver, st = res["F"], res["verified"], res["stats"].astype(np.int64)
    prob, counts, cands = want["problem"], want["counts"], want["cands"]
    assert st[3] == prob.m
    if name in NON_FINITE:   # include/lf_mkd.h, step 1: the pair is left without a candidate
        assert counts.max() < 0 and prob.m == len(mt)
    if counts.max() < 0:
        assert _invalid(res, prob.m, len(mt)), st
        return
    c = int(st[2])
    assert c < 3 * N_HYP and cands[c] is not None, (c, counts[c] if c < 3 * N_HYP else None)
    f_c = cands[c][0]
    slack_c = int(undecided(prob, f_c, thr).sum())
    assert abs(int(st[1]) - counts[c]) <= slack_c, (st, counts[c], slack_c)
    c_ref = int(np.argmax(counts))
    slack_ref = int(undecided(prob, cands[c_ref][0], thr).sum())
    if c != c_ref:   # only a near tie may choose another candidate
        assert counts[c_ref] - counts[c] <= slack_ref + slack_c, (c, c_ref, counts[c], counts[c_ref])
    assert st[0] == st[1] and (ver >= 0).sum() == st[0]
    assert np.array_equal(ver[ver >= 0], np.asarray(mt)[ver >= 0])
    diff = (ver[prob.rows] >= 0) != prob.inliers(f_c, thr)
    assert not (diff & ~undecided(prob, f_c, thr)).any(), diff.sum()
    assert np.abs(F).max() == 1.0 and (F.reshape(-1) == 1.0).any()


@pytest.mark.parametrize("name", WHOLE)
def test_whole_call_with_refit(twin, name):
    """What tests/test_gpu_fundamental.py::test_refit_matches_the_restatement asserts of the device, of the twin."""
    ka, kb, mt, thr = PROBLEMS[name]
    res, want = twin[name, 0], _restatement(name, 0)
    F, ver, st = res["F"], res["verified"], res["stats"].astype(np.int64)
    prob = want["problem"]
    if want["mask"] is None:
        assert _invalid(res, prob.m, len(mt)), st
        return
    assert st[2] != ref.INVALID and np.isfinite(F).all() and np.abs(F).max() == 1.0 and (ver >= 0).sum() == st[0]
    b = undecided(prob, want["f"], thr) | undecided(prob, F, thr)
    diff = (ver[prob.rows] >= 0) != want["mask"]
    assert not (diff & ~b).any(), diff.sum()
    assert abs(int(st[0]) - int(want["stats"][0])) <= int(b.sum())
    # The inliers' epipolar lines under the two F's, where they are the same solution (the twin took the restatement's
    # candidate; another one is a near tie, which test_whole_call_without_refit bounds) and on the matches both can decide:
    # b's distance to its line agrees within 0.05 px, and across the frame's width (test_gpu_fundamental's measure, the
    # line's height at x = 0, 512, 1024) for the problems that module applies it to
    sure = want["mask"] & ~b
    if int(twin[name, ft.NO_REFINE]["stats"][2]) == want["c"]:
        gap = _point_gap(prob, F, want["F"], sure)
        assert gap < 0.05, gap
        if name in ("general-50", "general-1000"):
            gap = _line_gap(prob, F, want["F"], want["mask"])
            assert gap < 0.05, gap
    # against the ground truth, as that module: the planted inliers' noise-free points lie on the twin's epipolar lines
    if name in TRUTH and prob.m >= 50:
        inl = TRUTH[name]["inlier"]
        d = ref.epipolar_distance(F, TRUTH[name]["a"][inl], TRUTH[name]["b"][inl])
        assert np.median(d) < 0.5, np.median(d)
