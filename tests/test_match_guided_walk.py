"""CPU tests of the walk batch (tests/match_guided_cases.py: walk_batch, walks, walk_coverage), the inputs with which
tests/test_gpu_match_guided_walk.py drives match_small_guided_pairs through long tile walks and across its 4096-row keypoint
chunks: the batch has every walk pattern and seam arrangement the kernel distinguishes, its planted rows are what they claim,
the reference stays affordable, walks() is right on masks written by hand, and the twin's masks agree with float64."""
import numpy as np
import pytest

import match_guided_cases as cases

KINDS = (cases.HOMOGRAPHY, cases.FUNDAMENTAL)


@pytest.fixture(scope="module")
def masks(tmp_path_factory):
    d = tmp_path_factory.mktemp("guided_twin_walk")
    exe = cases.build(d)
    return {(kind, thr): cases.walk_masks(exe, d, kind, thr) for kind in KINDS for thr in cases.THRESHOLDS[kind]}


def test_walks_on_masks_written_by_hand():
    # 20 x 565: two blocks (the second of 4 rows), 36 tiles of which the last has 5 rows; one chunk
    m = np.zeros((20, 565), bool)
    m[0, 0] = m[3, 32 * 16] = True                       # block 0: tiles 0 and 32, wave 0
    m[17, 16 * 16 + 2] = True                            # block 1: tile 16, wave 0
    m[19, 564] = True                                    # block 1: tile 35 (the partial one), wave 3
    w = cases.walks(m, 20, 565)
    assert len(w) == 32 and all(c == 0 for _, _, c in w)
    assert w[(0, 0, 0)] == "USU" and w[(1, 0, 0)] == "SUS" and w[(0, 3, 0)] == "SSS" and w[(1, 3, 0)] == "SSU"
    assert all(w[(b, v, 0)] == ("SSS" if v < 4 else "SS") for b in (0, 1) for v in range(1, 16) if v != 3)
    # 3 x 4113: one block, 258 tiles: a full chunk, then tile 256 and one row of tile 257
    m = np.zeros((3, 4113), bool)
    m[2, 4095] = m[0, 4096] = m[1, 4112] = True
    w = cases.walks(m, 3, 4113)
    assert sorted(w) == sorted([(0, v, 0) for v in range(16)] + [(0, 0, 1), (0, 1, 1)])
    assert w[(0, 15, 0)] == "S" * 15 + "U" and all(w[(0, v, 0)] == "S" * 16 for v in range(15))
    assert w[(0, 0, 1)] == "U" and w[(0, 1, 1)] == "U"
    m[1, 4112] = False
    assert cases.walks(m, 3, 4113)[(0, 1, 1)] == "S"
    assert cases.walks(np.zeros((0, 40), bool), 0, 40) == {} and cases.walks(np.zeros((5, 0), bool), 5, 0) == {}


def test_the_walk_batch_has_the_layout_and_the_sizes():
    assert sorted(cases.WALK_SIZES) == sorted([(1000, 1000), (600, 1003), (2000, 2000), (40, 4096), (40, 4097), (40, 4136),
                                               (16, 8200), (4136, 40)])
    assert cases.CHUNK == 4096 and cases.WAVES == 16
    for kind in KINDS:
        B = cases.walk_batch(kind)
        assert B.n_pairs == len(cases.WALK_SIZES) and [(int(B.oa[p + 1] - B.oa[p]), int(B.ob[p + 1] - B.ob[p]))
                                                       for p in range(B.n_pairs)] == cases.WALK_SIZES
        assert B.oa[0] > 0 and B.ob[0] > 0 and B.oa[-1] < len(B.a) and B.ob[-1] < len(B.b)
        assert np.isnan(B.ka[:, 2:]).all() and np.isnan(B.kb[:, 2:]).all() and np.isfinite(B.ka[:, :2]).all() and np.isfinite(B.kb[:, :2]).all()
        lo, hi = cases.THRESHOLDS[kind]
        assert B.run_pairs(lo) == B.n_pairs and B.run_pairs(hi) == B.n_pairs - (cases.WALK_NARROW_ONLY if kind == cases.FUNDAMENTAL else 0)
        for p, S in cases.SEAMS.items():                                   # the duplicates are one row twice, keypoint included
            if "dup" in S["plants"]:
                _, j0, j1 = S["plants"]["dup"]
                sa, sb = B.pair(p)
                ky = B.ka[sa] if S["rev"] else B.kb[sb]
                assert np.array_equal(ky[j0, :2], ky[j1, :2]) and j0 < 4096 <= j1
    assert cases.SIZES[0] == (37, 300)                                      # the first batch is as it was


def test_the_walk_batch_covers_the_walks_and_the_seam(masks):
    found = cases.walk_coverage(masks)
    print("[match_guided_walk] coverage:", found)
    assert found["longest walk"] == 16 and found["planted rows checked"] == 4 * (2 * 12 + 1)
    for key, per_pair in masks.items():                                     # both directions are one relation here too
        for fwd, rev, ref in per_pair:
            assert np.array_equal(fwd, ref) and np.array_equal(rev, fwd.T), key


def test_sampled_masks_against_float64(masks):
    """Per pair 200 point pairs drawn at random and up to 200 of the admissible ones: the twin's mask equals the float64
    predicate wherever the float64 num / (thr2 den) is not within 1e-4 of 1."""
    rng = np.random.default_rng(11)
    total = aside = hits = 0
    for (kind, thr), per_pair in masks.items():
        B = cases.walk_batch(kind)
        for p, (fwd, _, _) in enumerate(per_pair):
            sa, sb = B.pair(p)
            na, nb = fwd.shape
            i, j = rng.integers(0, na, 200), rng.integers(0, nb, 200)
            ii, jj = np.nonzero(fwd)
            pick = rng.permutation(len(ii))[:200]
            i, j = np.concatenate([i, ii[pick]]), np.concatenate([j, jj[pick]])
            ok, res = cases.f64_residual(kind, B.model[p], B.ka[sa, :2][i], B.kb[sb, :2][j], thr)
            ok, res = np.diagonal(ok), np.diagonal(res)
            near = np.abs(res - 1.0) <= 1e-4
            assert np.array_equal(ok[~near], fwd[i, j][~near]), (kind, thr, p)
            total += len(i)
            aside += int(near.sum())
            hits += int(fwd[i, j].sum())
    print(f"[match_guided_walk] {total} sampled point pairs, {hits} admissible, {aside} within 1e-4 of the threshold in float64")
    assert total > 10000 and hits > 4000 and aside <= 0.01 * total
