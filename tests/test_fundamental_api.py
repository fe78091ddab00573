"""CPU tests of RANSAC fundamental-matrix verification: the two entry points exist and refuse bad arguments without a device,
and the numpy restatement the GPU tests compare against (tests/fundamental_ref.py) is right about its own building blocks."""
import ctypes
import math

import numpy as np
import pytest

import fundamental_ref as ref
from fundamental_cases import FAMILIES, THR, two_view
import local_features_python as lfp


def test_both_symbols_are_exported():
    L = lfp.load_library()
    for s in ("lf_mkd_verify_fundamental", "lf_mkd_verify_fundamental_device"):
        assert s in lfp.SYMBOLS and hasattr(L, s)


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    kp = np.zeros((8, 5), np.float32)
    m = np.zeros(8, np.int32)
    F, ver, st = np.zeros(9, np.float32), np.zeros(8, np.int32), np.zeros(4, np.uint32)
    good = dict(kps_a=kp.ctypes.data, na=8, kps_b=kp.ctypes.data, nb=8, match=m.ctypes.data, n_hyp=64, thr=1.5, F=F.ctypes.data,
                ver=ver.ctypes.data, st=st.ctypes.data)

    def host(**kw):
        a = dict(good, **kw)
        return L.lf_mkd_verify_fundamental(None, a["kps_a"], a["na"], a["kps_b"], a["nb"], a["match"], a["n_hyp"], a["thr"], 0, 0,
                                           a["F"], a["ver"], a["st"])

    cases = [({}, b"null handle"), ({"kps_a": None}, b"null pointer"), ({"kps_b": None}, b"null pointer"),
             ({"match": None}, b"null pointer"), ({"F": None}, b"null pointer"), ({"ver": None}, b"null pointer"),
             ({"st": None}, b"null pointer"), ({"n_hyp": 0}, b"n_hypotheses"), ({"n_hyp": 65537}, b"n_hypotheses"),
             ({"thr": 0.0}, b"threshold"), ({"thr": -1.0}, b"threshold"), ({"thr": math.nan}, b"threshold"),
             ({"thr": math.inf}, b"threshold"), ({"thr": 1e-20}, b"threshold"), ({"thr": 1e20}, b"threshold")]
    for kw, what in cases:
        assert host(**kw) == -1, kw
        msg = L.lf_mkd_last_error(None)
        assert what in msg and msg.startswith(b"verify_fundamental"), (kw, msg)
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first

    def dev(**kw):
        a = dict(ka=p, oa=p, kb=p, ob=p, m=p, n=4, n_hyp=64, thr=1.5, F=p, ver=p, st=p)
        a.update(kw)
        return L.lf_mkd_verify_fundamental_device(None, a["ka"], a["oa"], a["kb"], a["ob"], a["m"], a["n"], a["n_hyp"],
                                                  a["thr"], 0, 0, a["F"], a["ver"], a["st"], None)

    for kw, what in [({}, b"null handle"), ({"oa": None}, b"null pointer"), ({"ob": None}, b"null pointer"),
                     ({"F": None}, b"null pointer"), ({"st": None}, b"null pointer"), ({"n_hyp": 0}, b"n_hypotheses"),
                     ({"n_hyp": 1 << 20}, b"n_hypotheses"), ({"thr": 0.0}, b"threshold"), ({"thr": math.nan}, b"threshold")]:
        assert dev(**kw) == -1, kw
        msg = L.lf_mkd_last_error(None)
        assert what in msg and msg.startswith(b"verify_fundamental_device"), (kw, msg)


def test_sampler_draws_seven_distinct_positions_in_range():
    for m in (7, 8, 50, 1000, 20000, 1 << 31):
        for k in range(0, 65536, 811):
            pos = ref.sample(7, k, m)
            assert pos is not None and len(set(pos)) == 7 and all(0 <= q < m for q in pos), (m, k, pos)
    assert ref.sample(3, 0, 6) is None
    # the key: seed + p in the high word, k << 6 and the draw in the low one
    assert ref.sample(1, 0, 1000) != ref.sample(2, 0, 1000) and ref.sample(1, 0, 1000) != ref.sample(1, 1, 1000)
    assert ref.sample(1 << 32, 5, 1000) == ref.sample(0, 5, 1000)   # seed + p wraps at 2^32


@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_recovers_the_true_f(family):
    ka, kb, mt, info = two_view(400, 0.1, 11, family)
    out = ref.verify(ka, kb, mt, n_hyp=128, thr=THR, seed=2)
    assert out["stats"][2] != ref.INVALID
    F = out["F"]
    assert np.abs(F).max() == 1.0 and F.reshape(-1)[np.argmax(np.abs(F))] == 1.0
    inl = info["inlier"]
    d = ref.epipolar_distance(F, info["a"][inl], info["b"][inl])
    print(f"[fundamental] {family}: {out['stats'].tolist()}, noise-free correspondences' symmetric epipolar distance "
          f"median {np.median(d):.3f} px, p95 {np.percentile(d, 95):.3f} px")
    assert np.median(d) < 0.5, np.median(d)
    # the outliers go: at least 90 % of the planted outliers are not kept
    kept = out["verified"] >= 0
    assert (kept & ~inl).sum() <= 0.1 * (~inl).sum() + 2 and (kept & inl).sum() >= 0.9 * inl.sum()


def test_seven_point_candidates_are_rank_two_and_fit_their_sample():
    n_checked = 0
    for family in FAMILIES:
        ka, kb, mt, _ = two_view(200, 0.3, 5, family)
        prob = ref.Problem(ka, kb, mt)
        for k in range(40):
            a = prob.sample_rows(9, k)
            for cand in prob.candidates(9, k):
                if cand is None:
                    continue
                fn = cand[1]
                s = np.linalg.svd(fn.reshape(3, 3), compute_uv=False)
                assert s[2] <= 1e-9 * s[0], s          # det F = 0 to f64 rounding
                assert np.abs(a @ fn.reshape(9)).max() <= 1e-9 * np.abs(a).max()   # the 7 sample constraints
                n_checked += 1
    assert n_checked > 150


def test_cubic_roots_bracketing():
    # (x - 1)(x + 2)(x - 0.5) = x^3 + 0.5 x^2 - 2.5 x + 1: three roots, ascending
    assert np.allclose(ref.cubic_roots(1.0, -2.5, 0.5, 1.0), [-2.0, 0.5, 1.0], atol=1e-12)
    (r,) = ref.cubic_roots(-6.0, 1.0, 0.0, 1.0)                     # x^3 + x - 6: one real root
    assert abs(r ** 3 + r - 6.0) < 1e-12
    assert len(ref.cubic_roots(1.0, 0.0, 0.0, 1.0)) == 1
    assert ref.cubic_roots(1.0, 2.0, 3.0, 0.0) == []                  # vanishing leading coefficient: no candidate
    assert ref.cubic_roots(1.0, 2.0, 3.0, 2.0 ** -22 * 3.0) == []
    assert ref.cubic_roots(math.nan, 2.0, 3.0, 1.0) == []


def test_jacobi_rank_two_step_agrees_with_svd():
    g = np.random.default_rng(4)
    for _ in range(200):
        f = g.normal(size=(3, 3)) * np.exp(g.uniform(-3, 3, (3, 1)))
        d, v = ref.smallest_eigenvector(f.T @ f)
        u, s, vt = np.linalg.svd(f)
        assert abs(abs(v @ vt[2]) - 1.0) < 1e-9 * max(1.0, s[1] ** 2 / max(s[1] ** 2 - s[2] ** 2, 1e-300)), (v, vt[2])
        r2 = ref.rank2(f)
        want = u[:, :2] @ np.diag(s[:2]) @ vt[:2]
        assert np.abs(r2 - want).max() <= 1e-9 * s[0], np.abs(r2 - want).max()


def test_restatement_edge_cases():
    ka, kb, mt, _ = two_view(10, 0.0, 1)
    out = ref.verify(ka, kb, np.array([0, 1, 2, 3, 4, 5, -1, 99, -5, -1]), n_hyp=8)
    assert out["stats"].tolist() == [0, 0, ref.INVALID, 6] and (out["F"] == 0).all() and (out["verified"] == -1).all()
    ka, kb, mt, _ = two_view(7, 0.0, 2)
    out = ref.verify(ka, kb, mt, n_hyp=8, flags=ref.NO_REFINE)   # M = 7: every sample is the whole set
    assert out["stats"][2] != ref.INVALID and out["stats"][0] == 7
    same = np.zeros((20, 5))
    same[:, :2] = 100.0                                            # one point repeated: every pivot vanishes
    out = ref.verify(same, same, np.arange(20), n_hyp=16)
    assert out["stats"][2] == ref.INVALID and out["stats"][3] == 20
