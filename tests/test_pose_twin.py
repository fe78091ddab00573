"""The two-view pose call's host twin (tests/cpp/pose_twin.cpp: the kernel's own math header compiled by g++) against the
float64 restatement (tests/pose_cases.py, numpy.linalg.eigh), on the CPU.  The device is held to the twin bit for bit by
tests/test_gpu_two_view_pose.py; this module is what ties the twin, and so the kernel's arithmetic, to the algorithm of
include/lf_mkd.h.

For all five families, noise-free and at sigma 0.5 with 30 % outliers (fundamental_cases.two_view(300, ., 5, family), F the
ground truth rounded to f32):
  * the in-front count, the largest other count, the parallax count and the per-link in-front mask are EQUAL;
  * the chosen R and t agree within GATE = 2^-22 absolute per entry, sigma likewise.  Derivation: both sides read the same
    f32 inputs; they differ by f64 roundings (2^-53) times the conditioning of an eigenvector of E^T E whose two large
    eigenvalues may be close (their gap is what wrong or noisy F leaves: >= 1e-6 here), far below 2^-25; the f32 store then
    adds at most 2^-25 on entries below 1;
  * points agree within GATE relative to |X| (the cosine: absolute), under the same rule; the "none" rows are equal;
  * candidate indices are NOT compared: eigenvector signs are the twin's own.
Before comparing, the restatement alone must leave no link undecided: min(|na|, |nb|) at least MARGIN = 1e-9 of the sum of
the magnitudes of their terms, for every candidate, and the parallax test likewise; f64 rounding moves those by ~1e-15.
The chosen R must be nearer to the true R than the other twisted rotation is, and t . t_true > 0.

Measured here (each test prints its own; profiles/two_view_pose.md has the table): worst |dR| 2.27e-8, |dt| 2.73e-8, |dsigma|
2.93e-8, points 5.37e-8 of their norm, cosine 2.98e-8 -- all of it the f32 store, a tenth of the gate; smallest in-front margin
1.10e-4, smallest parallax margin 7.4e-7; rotation error against MOTIONS below 2.9e-6 degrees (F is the truth rounded to f32,
so the bound asserted is 1e-4 degrees: two orders above what rounding F and R to f32 moves a rotation, 1e-7 rad)."""
import numpy as np
import pytest

import pose_cases as pc
import pose_twin as pt

GATE = 2.0 ** -22
MARGIN = 1e-9
DEG = 2.0
M = 300
CASES = [(fam, noisy) for fam in pc.FAMILIES for noisy in (False, True)]


def _table(fam, noisy):
    prob = pc.problem(M, 0.3 if noisy else 0.0, 5, fam, 0.5 if noisy else 0.0)
    return pc.make_table([prob], [pc.f_true(*pc.MOTIONS[fam])])


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{case: (table, twin's outputs, restatement)} from one build and one run of the program."""
    tmp = tmp_path_factory.mktemp("pose_twin")
    exe = pt.build(tmp)
    tables = [_table(*c) for c in CASES]
    outs = pt.run_calls(exe, tmp, [(t, DEG) for t in tables])
    return {c: (t, o, pc.reference(t, DEG)[0]) for c, t, o in zip(CASES, tables, outs)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{'noisy' if c[1] else 'exact'}")
def test_the_twin_against_the_restatement(results, case):
    fam, noisy = case
    t, got, want = results[case]
    assert want["pose"] and want["margin"] >= MARGIN and want["parallax_margin"] >= MARGIN, (want["margin"], want["parallax_margin"])
    stats = got["stats"][0]
    assert stats[2] in (0, 1, 2, 3)
    assert (int(stats[0]), int(stats[1]), int(stats[3])) == want["stats"]
    if not noisy:
        assert want["stats"][:2] == (M, 0)             # the true candidate sees every link in front, the others none
    R, tt, sigma = pt.f32(got["R"][0]).reshape(3, 3), pt.f32(got["t"][0]), pt.f32(got["sigma"][0])
    d_r, d_t, d_s = np.abs(R - want["R"]).max(), np.abs(tt - want["t"]).max(), np.abs(sigma - want["sigma"]).max()
    pts = pt.f32(got["points"])
    front = pts[:, 3] != 2.0
    assert np.array_equal(front, want["front"])
    assert np.array_equal(pts[~front], np.tile(pc.NONE_ROW, ((~front).sum(), 1)))
    wp = want["points"][front]
    d_x = (np.abs(pts[front, :3] - wp[:, :3]).max(1) / np.linalg.norm(wp[:, :3], axis=1)).max()
    d_c = np.abs(pts[front, 3] - wp[:, 3]).max()
    r_true, t_true = pc.MOTIONS[fam]
    err, err_other = pc.rotation_angle_deg(R, r_true), pc.rotation_angle_deg(want["other_R"], r_true)
    print(f"{fam} noisy={noisy}: |dR| {d_r:.2e} |dt| {d_t:.2e} |dsigma| {d_s:.2e} points {d_x:.2e} cosine {d_c:.2e} "
          f"margin {want['margin']:.2e} parallax margin {want['parallax_margin']:.2e} rotation error {err:.2e} deg "
          f"(other {err_other:.1f}) front {stats[0]} other {stats[1]} parallax {stats[3]} sigma {sigma}")
    assert d_r <= GATE and d_t <= GATE and d_s <= GATE and d_x <= GATE and d_c <= GATE
    assert abs(np.linalg.norm(tt.astype(np.float64)) - 1.0) <= 3 * 2.0 ** -24 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-6
    assert err < err_other and float(tt @ t_true) > 0
    assert err < 1e-4                                   # F is the truth rounded to f32
    # points: in camera a's frame at |t| = 1 the scene's depths are those of the generator over |t_true|
    z = pts[front, 2] * np.linalg.norm(t_true)
    if not noisy:
        assert z.min() > 3.9 and z.max() < 12.5, (z.min(), z.max())


def test_the_twin_on_the_edges_of_the_rule(results, tmp_path):
    """What the header promises of degenerate input, of the twin alone (the device is compared with it on the same tables):
    every no-pose cause gives the all-zero pose and "none" rows, rows outside the pool count nowhere, a NaN keypoint is in
    front of nothing, ranges are read against link_capacity, and entries outside every range are untouched."""
    exe = pt.build(tmp_path)
    nopose, names = pc.no_pose_batch()
    bad, odd = pc.bad_rows_table(), pc.odd_offsets_table()
    r_np, r_bad, r_odd = pt.run_calls(exe, tmp_path, [(nopose, DEG), (bad, DEG), (odd, DEG)])
    off = nopose["link_offsets"].astype(np.int64)
    for e, name in enumerate(names):
        rows = pt.f32(r_np["points"][off[e]:off[e + 1]])
        if name == "ok":
            assert r_np["stats"][e][2] < 4 and r_np["stats"][e][0] > 200 and (rows[:, 3] != 2.0).sum() == r_np["stats"][e][0]
            continue
        assert not r_np["R"][e].any() and not r_np["t"][e].any() and not r_np["sigma"][e].any(), name
        assert r_np["stats"][e].tolist() == [0, 0, pt.NONE, 0], name
        assert len(rows) == 300 and np.array_equal(rows, np.tile(pc.NONE_ROW, (300, 1))), name
    want = pc.reference(nopose, DEG)
    assert [w["pose"] for w in want] == [n == "ok" for n in names]
    # rows outside the pool, a NaN keypoint: "none" rows, and the counts are the restatement's
    want = pc.reference(bad, DEG)[0]
    pts = pt.f32(r_bad["points"])
    for k in (3, 40, 7, 41, 100, 20, 21):
        assert np.array_equal(pts[k], pc.NONE_ROW), k
    assert not want["valid"][[3, 40, 7, 41, 100]].any() and want["valid"][[20, 21]].all()
    assert (int(r_bad["stats"][0][0]), int(r_bad["stats"][0][1]), int(r_bad["stats"][0][3])) == want["stats"]
    assert np.array_equal(pts[:len(want["front"]), 3] != 2.0, want["front"])
    # offsets: edge 1 is cut at link_capacity, edge 2 is empty; nothing else is written
    cap = odd["link_capacity"]
    want = pc.reference(odd, DEG)
    assert [w["range"] for w in want] == [(0, 200), (200, cap), (cap, cap)]
    assert len(r_odd["points"]) == cap and not (r_odd["points"] == pt.FILL).any()
    assert r_odd["stats"][2].tolist() == [0, 0, pt.NONE, 0]
    for e in range(2):
        assert (int(r_odd["stats"][e][0]), int(r_odd["stats"][e][1]), int(r_odd["stats"][e][3])) == want[e]["stats"]
    # an empty table: entries outside every range keep what they held
    empty = dict(odd, link_offsets=np.array([7, 7, 7, 3], np.uint64))
    r = pt.run(exe, tmp_path, empty, DEG)
    assert (r["points"] == pt.FILL).all() and (r["stats"] == np.array([0, 0, pt.NONE, 0], np.uint32)).all()
