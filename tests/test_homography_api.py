"""CPU tests of RANSAC homography verification: the two entry points exist and refuse bad arguments without a device, and
the numpy restatement the GPU tests compare against (tests/homography_ref.py) is right about its own building blocks."""
import ctypes
import math

import numpy as np

import homography_ref as ref
import local_features_python as lfp


def test_both_symbols_are_exported():
    L = lfp.load_library()
    for s in ("lf_mkd_verify_homography", "lf_mkd_verify_homography_device"):
        assert s in lfp.SYMBOLS and hasattr(L, s)
    assert lfp.VERIFY_NO_REFINE == 1


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    kp = np.zeros((8, 5), np.float32)
    m = np.zeros(8, np.int32)
    H, ver, st = np.zeros(9, np.float32), np.zeros(8, np.int32), np.zeros(4, np.uint32)
    good = dict(kps_a=kp.ctypes.data, na=8, kps_b=kp.ctypes.data, nb=8, match=m.ctypes.data, n_hyp=64, thr=3.0, seed=0,
                flags=0, H=H.ctypes.data, ver=ver.ctypes.data, st=st.ctypes.data)

    def host(**kw):
        a = dict(good, **kw)
        return L.lf_mkd_verify_homography(None, a["kps_a"], a["na"], a["kps_b"], a["nb"], a["match"], a["n_hyp"], a["thr"],
                                          a["seed"], a["flags"], a["H"], a["ver"], a["st"])

    cases = [({}, b"null handle"), ({"kps_a": None}, b"null pointer"), ({"kps_b": None}, b"null pointer"),
             ({"match": None}, b"null pointer"), ({"H": None}, b"null pointer"), ({"ver": None}, b"null pointer"),
             ({"st": None}, b"null pointer"), ({"n_hyp": 0}, b"n_hypotheses"), ({"n_hyp": 65537}, b"n_hypotheses"),
             ({"thr": 0.0}, b"threshold"), ({"thr": -1.0}, b"threshold"), ({"thr": math.nan}, b"threshold"),
             ({"thr": math.inf}, b"threshold")]
    for kw, what in cases:
        assert host(**kw) == -1, kw
        assert what in L.lf_mkd_last_error(None), (kw, L.lf_mkd_last_error(None))
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first

    def dev(**kw):
        a = dict(ka=p, oa=p, kb=p, ob=p, m=p, n=4, n_hyp=64, thr=3.0, H=p, ver=p, st=p)
        a.update(kw)
        return L.lf_mkd_verify_homography_device(None, a["ka"], a["oa"], a["kb"], a["ob"], a["m"], a["n"], a["n_hyp"], a["thr"],
                                                 0, 0, a["H"], a["ver"], a["st"], None)

    for kw, what in [({}, b"null handle"), ({"oa": None}, b"null pointer"), ({"ob": None}, b"null pointer"),
                     ({"st": None}, b"null pointer"), ({"n_hyp": 0}, b"n_hypotheses"), ({"n_hyp": 1 << 20}, b"n_hypotheses"),
                     ({"thr": 0.0}, b"threshold"), ({"thr": math.nan}, b"threshold")]:
        assert dev(**kw) == -1, kw
        assert what in L.lf_mkd_last_error(None), (kw, L.lf_mkd_last_error(None))


def test_splitmix64_is_the_published_one():
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF
    # successive outputs of the generator seeded with 0 (state advances by the pre-increment)
    assert ref.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_sampler_draws_four_distinct_positions_in_range():
    for m in (4, 5, 50, 1000, 20000, 1 << 31):
        for k in range(0, 4096, 97):
            pos = ref.sample(7, k, m)
            assert pos is not None and len(set(pos)) == 4 and all(0 <= q < m for q in pos), (m, k, pos)
    # the key: seed + p in the high word, k << 5 and the draw in the low one -- different seeds or k, different draws
    assert ref.sample(1, 0, 1000) != ref.sample(2, 0, 1000) and ref.sample(1, 0, 1000) != ref.sample(1, 1, 1000)


def _planted(n, seed=0):
    g = np.random.default_rng(seed)
    h = np.array([[0.9, -0.2, 40.0], [0.15, 1.1, -25.0], [1e-4, -2e-4, 1.0]])
    a = g.uniform(0, 1000, (n, 2))
    b = ref.map_points(h, a)
    kps_a, kps_b = np.zeros((n, 5)), np.zeros((n, 5))      # float64: the matches are exact
    kps_a[:, :2], kps_b[:, :2] = a, b
    return h, kps_a, kps_b


def test_restatement_recovers_a_planted_homography():
    h, kps_a, kps_b = _planted(300)
    prob = ref.Problem(kps_a, kps_b, np.arange(300))
    k = next(k for k in range(64) if prob.hypothesis(0, k) is not None)
    got = prob.hypothesis(0, k)
    assert np.abs(got / got[2, 2] - h).max() < 1e-9
    out = ref.verify(kps_a, kps_b, np.arange(300), n_hyp=16)
    assert np.abs(out["H"] - h).max() < 1e-9
    assert out["stats"][0] == 300 and (out["verified"] == np.arange(300)).all()


def test_restatement_edge_cases():
    _, kps_a, kps_b = _planted(10)
    out = ref.verify(kps_a, kps_b, np.array([0, 1, 2, -1, 99, -5, -1, -1, -1, -1]), n_hyp=8)
    assert out["stats"].tolist() == [0, 0, ref.INVALID, 3] and (out["H"] == 0).all() and (out["verified"] == -1).all()
    line = np.zeros((20, 5))
    line[:, 0] = np.arange(20) * 7.0
    line[:, 1] = 3.0 + 2.0 * line[:, 0]
    out = ref.verify(line, line, np.arange(20), n_hyp=64)     # all collinear: every quad is degenerate
    assert out["stats"][2] == ref.INVALID and out["stats"][3] == 20


def test_threshold_square_must_be_a_finite_normal_f32():
    """The kernels compare against thr^2 in f32: below ~1.08e-19 it is subnormal or 0 (an exact match would be no inlier),
    above ~1.84e19 it is inf (every refit would be kept).  Both entry points refuse those thresholds and accept the f32
    values just inside; without a handle, an accepted threshold is then refused for the missing handle."""
    L = lfp.load_library()
    f32 = np.float32
    lo, hi = f32(1.0842022e-19), f32(1.8446743e19)
    assert np.isfinite(lo * lo) and lo * lo >= np.finfo(f32).tiny
    with np.errstate(over="ignore"):
        assert np.isinf(np.nextafter(hi, f32(np.inf)) ** 2) and np.isfinite(hi * hi)
    assert np.nextafter(lo, f32(0)) ** 2 < np.finfo(f32).tiny
    kp = np.zeros((8, 5), np.float32)
    m = np.zeros(8, np.int32)
    H, ver, st = np.zeros(9, np.float32), np.zeros(8, np.int32), np.zeros(4, np.uint32)
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first
    calls = [lambda t: L.lf_mkd_verify_homography(None, kp.ctypes.data, 8, kp.ctypes.data, 8, m.ctypes.data, 64, t, 0, 0,
                                                  H.ctypes.data, ver.ctypes.data, st.ctypes.data),
             lambda t: L.lf_mkd_verify_homography_device(None, p, p, p, p, p, 4, 64, t, 0, 0, p, p, p, None)]
    refused = [np.nextafter(lo, f32(0)), f32(1e-20), f32(1e-30), np.finfo(f32).tiny, f32(1.4e-45),
               np.nextafter(hi, f32(np.inf)), f32(1e20), np.finfo(f32).max]
    accepted = [lo, np.nextafter(lo, f32(1)), f32(1e-3), f32(1.0), f32(3.0), f32(3.5), f32(8.0), f32(1e10),
                np.nextafter(hi, f32(0)), hi]
    for call in calls:
        for t in refused:
            assert call(float(t)) == -1, t
            assert b"threshold" in L.lf_mkd_last_error(None), (t, L.lf_mkd_last_error(None))
        for t in accepted:
            assert call(float(t)) == -1, t
            assert b"null handle" in L.lf_mkd_last_error(None), (t, L.lf_mkd_last_error(None))
