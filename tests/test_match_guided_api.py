"""CPU tests of guided matching (lf_mkd_match_guided_pairs_device): the symbol, the constants and the Python methods exist; bad
arguments are refused without a device; and the kernel's predicate header (csrc/mkd_guided_math.h, through the host twin
tests/cpp/guided_twin.cpp) is the verifiers' inlier test -- against f_inlier() itself, against tests/homography_f32.py's
restatement of inlier(), against a float64 evaluation, and symmetric between the two directions -- on the batch the GPU tests
use, which has the coverage they need."""
import ctypes

import numpy as np
import pytest

import homography_f32 as h32
import match_guided_cases as cases
import local_features_python as lfp


def test_the_symbol_the_constants_and_the_methods_exist():
    L = lfp.load_library()
    assert "lf_mkd_match_guided_pairs_device" in lfp.SYMBOLS and hasattr(L, "lf_mkd_match_guided_pairs_device")
    assert (lfp.GUIDE_HOMOGRAPHY, lfp.GUIDE_FUNDAMENTAL) == (0, 1) == (cases.HOMOGRAPHY, cases.FUNDAMENTAL)
    assert hasattr(lfp.MkdHandle, "match_guided_pairs_device")
    assert hasattr(lfp.LocalFeatures, "match_guided_batch") and hasattr(lfp.LocalFeatures, "match_guided")


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first

    def call(**kw):
        a = dict(a=p, ka=p, oa=p, na=64, b=p, kb=p, ob=p, nb=64, model=p, n=4, kind=0, thr=3.0, flags=0, ab=p, ba=p)
        a.update(kw)
        return L.lf_mkd_match_guided_pairs_device(None, a["a"], a["ka"], a["oa"], a["na"], a["b"], a["kb"], a["ob"], a["nb"],
                                                  a["model"], a["n"], a["kind"], a["thr"], 0.8, a["flags"], a["ab"], a["ba"],
                                                  None, None, None)

    big = (1 << 31) - 1
    bad = [({}, b"null handle"), ({"n": 0}, b"null handle"), ({"kind": 1}, b"null handle")]
    bad += [({k: None}, b"null pointer") for k in ("a", "b", "ka", "kb", "oa", "ob", "model", "ab")]
    bad += [({"ba": None}, b"null handle"),                                  # one direction: d_match_ba may be NULL
            ({"ba": None, "flags": lfp.MATCH_MUTUAL}, b"d_match_ba"), ({"flags": 2}, b"unknown flag"),
            ({"flags": 0x80000001}, b"unknown flag"), ({"kind": 2}, b"kind"), ({"kind": 0xFFFFFFFF}, b"kind"),
            ({"thr": 0.0}, b"threshold_px"), ({"thr": -3.0}, b"threshold_px"), ({"thr": float("nan")}, b"threshold_px"),
            ({"thr": float("inf")}, b"threshold_px"), ({"thr": 1e-20}, b"threshold_px"), ({"thr": 1e20}, b"threshold_px"),
            ({"thr": 2e-19}, b"null handle"), ({"thr": 1e19}, b"null handle"),       # the square is a normal number
            ({"a": ctypes.c_void_p(24)}, b"aligned"), ({"b": ctypes.c_void_p(20)}, b"aligned"),
            ({"ka": ctypes.c_void_p(20)}, b"null handle"),                           # keypoint rows are 4-byte aligned
            ({"na": big + 1}, b"2^31"), ({"nb": 1 << 40}, b"2^31"),
            ({"na": big, "nb": big, "n": 1 << 30}, b"workgroups"),                   # 2 x (2^27 + 2^30) slots
            ({"na": big, "n": 0xFFFFFFFF, "ba": None}, b"workgroups"),
            ({"na": big, "nb": big, "n": 1 << 20}, b"null handle")]                  # a grid that fits is no error
    for kw, what in bad:
        assert call(**kw) == -1, kw
        msg = L.lf_mkd_last_error(None)
        assert what in msg and msg.startswith(b"match_guided_pairs_device"), (kw, msg)


@pytest.fixture(scope="module")
def masks(tmp_path_factory):
    d = tmp_path_factory.mktemp("guided_twin")
    exe = cases.build(d)
    return {(kind, thr): cases.batch_masks(exe, d, kind, thr) for kind in (cases.HOMOGRAPHY, cases.FUNDAMENTAL)
            for thr in cases.THRESHOLDS[kind]}


def test_the_batch_covers_what_the_gpu_tests_need(masks):
    found = cases.coverage(masks)
    print("[match_guided] rows by candidates, tiles:", found)
    for kind in (cases.HOMOGRAPHY, cases.FUNDAMENTAL):
        B = cases.batch(kind)
        assert not B.model[cases.ZERO_MODEL].any() and np.isnan(B.model[cases.NAN_MODEL]).sum() == 1
        assert np.isnan(B.ka[:, 2:]).all() and np.isnan(B.kb[:, 2:]).all()       # only x and y may be read
        assert B.ka[:, 0].max() < cases.W and B.ka[:, 1].max() < cases.H and B.ka[:, :2].min() >= 0
        for thr in cases.THRESHOLDS[kind]:
            for p in (cases.ZERO_MODEL, cases.NAN_MODEL, 6, 7):
                assert not masks[(kind, thr)][p][0].any()                         # nothing admissible / an empty side


def test_hoisted_equals_the_verifiers_own_test_and_both_directions_agree(masks):
    for (kind, thr), per_pair in masks.items():
        B = cases.batch(kind)
        for p, (fwd, rev, ref) in enumerate(per_pair):
            assert np.array_equal(fwd, ref), (kind, thr, p)                       # f_inlier() itself / inlier() restated in C++
            assert np.array_equal(rev, fwd.T), (kind, thr, p)                     # the b -> a mask is the transpose
            if kind == cases.HOMOGRAPHY and fwd.size:
                sa, sb = B.pair(p)
                a, b = B.ka[sa, :2], B.kb[sb, :2]
                ax, ay = np.repeat(a[:, 0], len(b)), np.repeat(a[:, 1], len(b))
                bx, by = np.tile(b[:, 0], len(a)), np.tile(b[:, 1], len(a))
                inl, _ = h32.inlier_cost(B.model[p], ax, ay, bx, by, h32.thr_square(thr))
                assert np.array_equal(inl.reshape(fwd.shape), fwd), (thr, p)      # homography_f32.py's inlier rule
        # a larger threshold only adds candidates (thr2 * den is monotone in thr2)
    for kind in (cases.HOMOGRAPHY, cases.FUNDAMENTAL):
        lo, hi = cases.THRESHOLDS[kind]
        for (f_lo, _, _), (f_hi, _, _) in zip(masks[(kind, lo)], masks[(kind, hi)]):
            assert not (f_lo & ~f_hi).any()


def test_masks_against_float64(masks):
    """The twin's masks equal a float64 evaluation of the predicates wherever the float64 num / (thr2 den) is not within
    1 +- 1e-3 -- about 40 times the f32 rounding of the residual at 640 px coordinates, 2^-24 * 640 / 1.5 = 2.5e-5 -- and no
    more than 1 % of the pairs of points are set aside for it."""
    total = aside = 0
    for (kind, thr), per_pair in masks.items():
        B = cases.batch(kind)
        for p, (fwd, _, _) in enumerate(per_pair):
            sa, sb = B.pair(p)
            ok, res = cases.f64_residual(kind, B.model[p], B.ka[sa, :2], B.kb[sb, :2], thr)
            near = np.abs(res - 1.0) <= 1e-3                                      # (NaN -- a zero or NaN model -- is not near)
            assert np.array_equal(ok[~near], fwd[~near]), (kind, thr, p)
            total += fwd.size
            aside += int(near.sum())
    print(f"[match_guided] {aside} of {total} point pairs within 1e-3 of the threshold in float64 ({aside / total:.3%})")
    assert total > 100000 and aside <= 0.01 * total, (aside, total)
