"""RANSAC homography verification on the GPU held to its f32 twin (tests/homography_f32.py) bit for bit: every hypothesis of
problem families chosen for where kernels go wrong, ragged hypothesis counts, ties, row slicing, seeds that wrap, non-finite
coordinates and the refit's edges.  The twin's own agreement with the float64 restatement is tests/test_homography_twin.py."""
import numpy as np
import pytest

import homography_cases as cases
import homography_f32 as tw
import homography_ref as ref
from homography_cases import THR, planted

import local_features_python as lfp

pytestmark = pytest.mark.gpu

NO_REFINE = lfp.VERIFY_NO_REFINE


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


def _device_batch(handle, pairs, n_hyp, seed, flags=0, thr=THR):
    """Pairs in one lf_mkd_verify_homography_device call: (H [n, 9] f32, verified [Na] int32, stats [n, 4] uint32, a offsets)."""
    import torch
    oa = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ob = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    ka = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[0] for p in pairs]), np.float32).reshape(-1, 5)).cuda()
    kb = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[1] for p in pairs]), np.float32).reshape(-1, 5)).cuda()
    mt = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[2] for p in pairs]), np.int32)).cuda()
    d_oa, d_ob = torch.from_numpy(oa).cuda(), torch.from_numpy(ob).cuda()
    n = len(pairs)
    H = torch.full((n, 9), np.nan, device="cuda")
    ver = torch.full((max(len(mt), 1),), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    handle.verify_homography_device(ka.data_ptr(), d_oa.data_ptr(), kb.data_ptr(), d_ob.data_ptr(), mt.data_ptr(), n,
                                    H.data_ptr(), ver.data_ptr(), st.data_ptr(), n_hyp, thr, seed, flags,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return H.cpu().numpy(), ver.cpu().numpy()[:len(mt)], st.cpu().numpy().view(np.uint32), oa


def _assert_equal_to_twin(want, H, ver, st, what):
    assert np.array_equal(np.asarray(H, np.float32).reshape(-1).view(np.uint32), want["H"].reshape(-1).view(np.uint32)), \
        (what, np.asarray(H).reshape(-1), want["H"].reshape(-1))
    assert np.array_equal(np.asarray(st).view(np.uint32), want["stats"]), (what, st, want["stats"])
    assert np.array_equal(ver, want["verified"]), (what, int((ver != want["verified"]).sum()))


# ---- every hypothesis, bit for bit ------------------------------------------------------------------------------------
N_COPIES = 4096


def _family(name):
    g = np.random.default_rng(sum(name.encode()))
    if name == "perspective":
        return planted(200, 0.6, 1)
    if name == "large_offset":
        h = cases.random_perspective(g, 4096.0, 3072.0)
        return cases.planted_in(g, 200, 0.6, h, 4096.0, 3072.0, offset=2e4)
    if name == "near_degenerate":
        return cases.near_degenerate(g, 200)
    if name == "vanishing":
        return cases.vanishing(g, 200)
    if name == "duplicates":
        return cases.duplicates(g, 200)
    if name == "exact_integer":
        return cases.exact_integer(g, 200)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["perspective", "large_offset", "near_degenerate", "vanishing", "duplicates",
                                  "exact_integer"])
def test_every_hypothesis_bit_for_bit(handle, name):
    """N copies of one problem, n_hypotheses = 1, no refit: pair p reports hypothesis 0 of seed s + p."""
    ka, kb, mt = _family(name)
    seed = 0x51ED + 977 * len(name)
    H, ver, st, oa = _device_batch(handle, [(ka, kb, mt)] * N_COPIES, 1, seed, NO_REFINE)
    pair = tw.Pair(ka, kb, mt)
    thr2 = tw.thr_square(THR)
    seeds = seed + np.arange(N_COPIES)
    valid, h = pair.hypotheses(seeds, np.zeros(N_COPIES, np.int64))
    inl = np.zeros((N_COPIES, pair.m), bool)
    if valid.any():
        inl[valid] = pair.inliers(h[valid], thr2)[0]
    count = inl.sum(axis=1).astype(np.uint32)
    with np.errstate(all="ignore"):
        want_H = np.where(valid[:, None], h / h[:, 8:9], np.float32(0)).astype(np.float32)
    want_st = np.stack([np.where(valid, count, 0), np.where(valid, count, 0), np.where(valid, 0, ref.INVALID),
                        np.full(N_COPIES, pair.m)], axis=1).astype(np.uint32)
    want_ver = np.full((N_COPIES, len(mt)), -1, np.int32)
    rows = pair.rows
    want_ver[:, rows] = np.where(inl, mt[rows][None, :], -1)
    assert np.array_equal(H.view(np.uint32), want_H.view(np.uint32)), (name, int((H.view(np.uint32) != want_H.view(np.uint32)).any(axis=1).sum()))
    assert np.array_equal(st, want_st), (name, np.flatnonzero((st != want_st).any(axis=1))[:8])
    assert np.array_equal(ver.reshape(N_COPIES, -1), want_ver), name
    # the family does what it is for
    assert 0 < valid.sum(), name
    if name == "near_degenerate":
        assert valid.sum() < N_COPIES
    if name == "vanishing":   # points on both sides of the vanishing line; hypotheses that mix them are invalid
        w = (-1.0 / 600.0) * pair.ax + 1.0
        assert (w <= 0).any() and (w > 0).any() and valid.sum() < N_COPIES


# ---- ragged hypothesis counts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", [1, 3, 255, 257, 1000, 65536])
@pytest.mark.parametrize("flags", [0, NO_REFINE])
def test_ragged_hypothesis_counts(handle, n_hyp, flags):
    m = 40 if n_hyp == 65536 else 300
    ka, kb, mt = planted(m, 0.5, 7 + n_hyp)
    H, ver, st = handle.verify_homography(ka, kb, mt, n_hyp, THR, 21, flags)
    want = tw.verify(ka, kb, mt, n_hyp=n_hyp, thr=THR, seed=21, flags=flags)
    _assert_equal_to_twin(want, H, ver, st, (n_hyp, flags))


# ---- ties go to the smallest k ----------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_k(handle):
    g = np.random.default_rng(5)
    ka, kb, mt = cases.exact_integer(g, 200)
    want = tw.verify(ka, kb, mt, n_hyp=256, thr=THR, seed=3, flags=NO_REFINE)
    assert (want["counts"][want["valid"]] == 200).all() and want["valid"].sum() > 1
    H, ver, st = handle.verify_homography(ka, kb, mt, 256, THR, 3, NO_REFINE)
    assert st[2] == np.flatnonzero(want["valid"])[0]
    _assert_equal_to_twin(want, H, ver, st, "all inliers")
    # two planes of equal size: the best count is reached by hypotheses of both, the first of them wins
    ka, kb, mt = cases.two_planes(g, 200)
    for flags in (NO_REFINE, 0):
        want = tw.verify(ka, kb, mt, n_hyp=512, thr=THR, seed=8, flags=flags)
        top = np.flatnonzero(want["counts"] == want["counts"].max())
        plane = lambda k: set(np.array(ref.sample(8, int(k), 200)) >= 100)
        assert want["counts"].max() == 100 and {frozenset(plane(k)) for k in top} == {frozenset({False}), frozenset({True})}
        H, ver, st = handle.verify_homography(ka, kb, mt, 512, THR, 8, flags)
        assert st[2] == top[0] and st[1] == 100
        _assert_equal_to_twin(want, H, ver, st, ("two planes", flags))


# ---- row slicing ------------------------------------------------------------------------------------------------------
def _slices(n_pairs, n_hyp, cus):
    """verify_slices (mkd_verify.hip), restated"""
    blocks = n_pairs * ((n_hyp + 255) // 256)
    return int(min(16, max(1, (2 * cus + blocks - 1) // blocks)))


def test_row_slicing(handle):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = np.random.default_rng(11)
    probs = []
    for na in (255, 256, 257, 4097):
        ka, kb, mt = planted(na, 0.6, na)
        mt[g.random(na) < 0.3] = -1
        probs.append((ka, kb, mt))
    empty = (np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32))
    n_hyp, seed = 256, 90
    twins = {}
    reached = set()
    for target in (16, 13, 6, 3, 2, 1):
        n_pairs = next(n for n in range(len(probs), 1 << 16) if _slices(n, n_hyp, cus) == target)
        reached.add(_slices(n_pairs, n_hyp, cus))
        batch = probs + [empty] * (n_pairs - len(probs))
        for flags in (0, NO_REFINE):
            H, ver, st, oa = _device_batch(handle, batch, n_hyp, seed, flags)
            for p, (ka, kb, mt) in enumerate(probs):
                if (p, flags) not in twins:
                    twins[p, flags] = tw.verify(ka, kb, mt, n_hyp=n_hyp, thr=THR, seed=seed + p, flags=flags)
                    h1, v1, s1 = handle.verify_homography(ka, kb, mt, n_hyp, THR, seed + p, flags)
                    _assert_equal_to_twin(twins[p, flags], h1, v1, s1, ("single", p, flags))
                _assert_equal_to_twin(twins[p, flags], H[p], ver[oa[p]:oa[p + 1]], st[p], (target, p, flags))
            assert (st[len(probs):, 2] == ref.INVALID).all() and (H[len(probs):] == 0).all()
    assert reached == {16, 13, 6, 3, 2, 1}


# ---- seeds that wrap past 2^32 ----------------------------------------------------------------------------------------
def test_seeds_wrap_inside_a_batch(handle):
    import torch
    pairs = [planted(120, 0.6, 30 + p) for p in range(8)]
    seed = 0xFFFFFFFF - 3
    H, ver, st, oa = _device_batch(handle, pairs, 300, seed)
    feats = lfp.LocalFeatures(64, 64, 64)
    t = lambda i, dt: torch.from_numpy(np.concatenate([p[i] for p in pairs]).astype(dt)).cuda()
    ob = torch.tensor(np.cumsum([0] + [len(p[1]) for p in pairs]))
    Hb, vb, sb = feats.verify_homography_batch(t(0, np.float32), torch.tensor(oa), t(1, np.float32), ob, t(2, np.int32),
                                               seed=seed, n_hypotheses=300)
    torch.cuda.synchronize()
    Hb, vb, sb = Hb.cpu().numpy().reshape(-1, 9), vb.cpu().numpy(), sb.cpu().numpy()
    for p, (ka, kb, mt) in enumerate(pairs):
        sp = (seed + p) & 0xFFFFFFFF
        want = tw.verify(ka, kb, mt, n_hyp=300, thr=THR, seed=sp)
        _assert_equal_to_twin(want, H[p], ver[oa[p]:oa[p + 1]], st[p], ("ctypes", p))
        h1, v1, s1 = handle.verify_homography(ka, kb, mt, 300, THR, sp, 0)
        _assert_equal_to_twin(want, h1, v1, s1, ("single", p))
        assert np.array_equal(Hb[p].view(np.uint32), want["H"].reshape(-1).view(np.uint32)), p
        assert np.array_equal(vb[oa[p]:oa[p + 1]], want["verified"]), p
        assert sb[p].tolist() == [int(want["stats"][0]), int(want["stats"][1]),
                                  -1 if want["stats"][2] == ref.INVALID else int(want["stats"][2]), int(want["stats"][3])]
    assert (seed + 7) >> 32 == 1 and (seed + 3) >> 32 == 0   # the batch did wrap


# ---- non-finite coordinates -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinates(handle, bad):
    ka, kb, mt = planted(300, 0.6, 77)
    mt[[10, 20, 30]] = -1
    clean = tw.verify(ka, kb, mt, n_hyp=256, thr=THR, seed=4)
    assert clean["stats"][2] != ref.INVALID
    # in rows that do not count: nothing changes, bit for bit
    ka2 = ka.copy()
    ka2[10, 0], ka2[20, 1] = bad, bad
    kb2 = np.concatenate([kb, np.full((1, 5), bad, np.float32)])   # an unmatched b row
    mt2 = mt.copy()
    mt2[30] = len(kb2) - 1 + 1000                                     # out of range: does not count either
    H, ver, st = handle.verify_homography(ka2, kb2, mt2, 256, THR, 4, 0)
    _assert_equal_to_twin(clean, H, ver, st, "non-considered")
    # in a considered row (a or b, x or y): no valid hypothesis for that pair, other pairs of the call unaffected
    broken = []
    for which, col in ((0, 0), (0, 1), (1, 0), (1, 1)):
        a, b = ka.copy(), kb.copy()
        (a if which == 0 else b)[5, col] = bad
        broken.append((a, b, mt))
    pairs = [(ka, kb, mt)] + broken + [(ka, kb, mt)]
    H, ver, st, oa = _device_batch(handle, pairs, 256, 4)
    for p in range(len(pairs)):
        if p in (0, len(pairs) - 1):
            want = tw.verify(ka, kb, mt, n_hyp=256, thr=THR, seed=4 + p)
            _assert_equal_to_twin(want, H[p], ver[oa[p]:oa[p + 1]], st[p], ("neighbour", p))
            continue
        want = tw.verify(*pairs[p], n_hyp=256, thr=THR, seed=4 + p)
        assert st[p].tolist() == [0, 0, ref.INVALID, 297] and (H[p] == 0).all() and (ver[oa[p]:oa[p + 1]] == -1).all(), p
        _assert_equal_to_twin(want, H[p], ver[oa[p]:oa[p + 1]], st[p], ("broken", p))


# ---- the refit's edges ------------------------------------------------------------------------------------------------
def test_refit_edges(handle):
    g = np.random.default_rng(13)
    # exactly 4 inliers: four points of a plane among matches that agree with nothing; the refit is an exact solve of
    # 8 equations and stops after one round
    a = g.uniform(0, 1000, (60, 2))
    b = g.uniform(0, 1000, (60, 2))
    b[:4] = ref.map_points(cases.H_TRUE, a[:4])
    ka, kb = cases._rows(a, b)
    mt = np.arange(60, dtype=np.int32)
    want = tw.verify(ka, kb, mt, n_hyp=4096, thr=THR, seed=2)
    assert want["stats"][0] == 4 and want["stats"][1] == 4 and len(want["rounds"]) == 1, (want["stats"], want["rounds"])
    H, ver, st = handle.verify_homography(ka, kb, mt, 4096, THR, 2, 0)
    _assert_equal_to_twin(want, H, ver, st, "4 inliers")
    # exact all-inlier data
    ka, kb, mt = cases.exact_integer(g, 500)
    want = tw.verify(ka, kb, mt, n_hyp=64, thr=THR, seed=6)
    assert want["stats"][0] == 500 and want["rounds"][0] in ("kept", "settled")
    H, ver, st = handle.verify_homography(ka, kb, mt, 64, THR, 6, 0)
    _assert_equal_to_twin(want, H, ver, st, "exact")
    # a refit whose truncated quadratic cost rises: rejected, the 4-point H is kept (found with the twin on the CPU)
    ka, kb, mt = planted(300, 0.5, 144, sigma=1.5)
    want = tw.verify(ka, kb, mt, n_hyp=64, thr=THR, seed=144)
    assert want["rounds"] == ["rejected"] and np.array_equal(want["h"], want["h4"])
    H, ver, st = handle.verify_homography(ka, kb, mt, 64, THR, 144, 0)
    _assert_equal_to_twin(want, H, ver, st, "rejected")


# ---- the scoring grid's limit -----------------------------------------------------------------------------------------
def test_scoring_grid_limit_is_refused_before_launch(handle):
    """65536 pairs x 65536 hypotheses = 2^24 scoring workgroups: LF_MKD_ERR_BAD_ARG, and nothing is written.  Every buffer
    is sized for the call (all pairs empty), so that even a launch would stay in bounds."""
    import torch
    n = 65536
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    kp = torch.zeros((1, 5), device="cuda")
    mt = torch.zeros(1, dtype=torch.int32, device="cuda")
    H = torch.full((n, 9), 7.0, device="cuda")
    ver = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
    L = lfp.load_library()
    rc = L.lf_mkd_verify_homography_device(handle._h, kp.data_ptr(), offs.data_ptr(), kp.data_ptr(), offs.data_ptr(),
                                           mt.data_ptr(), n, 65536, THR, 0, 0, H.data_ptr(), ver.data_ptr(), st.data_ptr(),
                                           None)
    torch.cuda.synchronize()
    assert rc == -1   # LF_MKD_ERR_BAD_ARG
    assert b"scoring grid" in L.lf_mkd_last_error(handle._h)
    assert (H == 7.0).all() and (st == 7).all() and (ver == 7).all()
    # one pair fewer fits (and stays within every buffer)
    assert _slices_ok(n - 1)


def _slices_ok(n_pairs):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return n_pairs * 256 * _slices(n_pairs, 65536, cus) < (1 << 24)
