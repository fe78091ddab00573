"""CPU tests of guided matching over 8-bit rows (lf_mkd_match_q8_guided_pairs_device): the symbol exists and refuses bad
arguments without a device, and what the GPU tests rest on (tests/q8_guided_cases.py) is right about itself -- the shared batch
covers every path of the kernel, its planted rows are what they claim to be, the masked integer decision follows the header's
sentences, and the host twin's masks are the float64 predicate away from its boundary."""
import ctypes

import numpy as np
import pytest

import match_guided_cases as gcases
import q8_cases as qcases
import q8_guided_cases as cases
import local_features_python as lfp

BIG = (1 << 31) - 1


@pytest.fixture(scope="module")
def masks(tmp_path_factory):
    d = tmp_path_factory.mktemp("q8_guided_twin")
    return cases.all_masks(gcases.build(d), d)


def test_the_symbol_is_exported_and_the_methods_exist():
    L = lfp.load_library()
    name = "lf_mkd_match_q8_guided_pairs_device"
    assert name in lfp.SYMBOLS and hasattr(L, name)
    assert len(getattr(L, name).argtypes) == 20
    assert hasattr(lfp.MkdHandle, "match_q8_guided_pairs_device")
    assert hasattr(lfp.LocalFeatures, "match_q8_guided_batch") and hasattr(lfp.LocalFeatures, "match_q8_guided")
    assert lfp.match_q8_pairs_plan(0, 0, 0)[0] == cases.R            # the grid is the q8 pairs plan's: the batch is built for its R


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first

    def call(**kw):
        a = dict(a=p, ka=p, oa=p, na=64, b=p, kb=p, ob=p, nb=64, model=p, n=4, kind=0, thr=3.0, flags=0, ab=p, ba=p)
        a.update(kw)
        return L.lf_mkd_match_q8_guided_pairs_device(None, a["a"], a["ka"], a["oa"], a["na"], a["b"], a["kb"], a["ob"], a["nb"],
                                                     a["model"], a["n"], a["kind"], a["thr"], 0.8, a["flags"], a["ab"], a["ba"],
                                                     None, None, None)

    cases_ = [({}, b"null handle"), ({"n": 0}, b"null handle"), ({"kind": 1, "thr": 1.5}, b"null handle"),
              ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"), ({"ka": None}, b"null pointer"),
              ({"kb": None}, b"null pointer"), ({"oa": None}, b"null pointer"), ({"ob": None}, b"null pointer"),
              ({"model": None}, b"null pointer"), ({"ab": None}, b"null pointer"),
              ({"ba": None}, b"null handle"),                                  # one direction: d_match_ba may be NULL
              ({"ba": None, "flags": lfp.MATCH_MUTUAL}, b"d_match_ba"), ({"flags": 2}, b"unknown flag"),
              ({"flags": 0x80000001}, b"unknown flag"), ({"kind": 2}, b"kind"), ({"kind": 0xFFFFFFFF}, b"kind"),
              ({"thr": 0.0}, b"threshold_px"), ({"thr": -3.0}, b"threshold_px"), ({"thr": float("nan")}, b"threshold_px"),
              ({"thr": float("inf")}, b"threshold_px"), ({"thr": 1e-20}, b"threshold_px"), ({"thr": 1e20}, b"threshold_px"),
              ({"thr": 1e-19 * 1.2}, b"null handle"), ({"thr": 1.8e19}, b"null handle"),   # the square is normal: fine
              ({"a": ctypes.c_void_p(24)}, b"aligned"), ({"b": ctypes.c_void_p(20)}, b"aligned"),
              ({"ka": ctypes.c_void_p(20)}, b"null handle"),                   # keypoints need no more than a float's alignment
              ({"na": BIG + 1}, b"2^31"), ({"nb": 1 << 40}, b"2^31"),
              ({"na": BIG, "nb": BIG, "n": 1 << 30}, b"workgroups"),           # 2 x (at least 2^30) slots
              ({"na": BIG, "n": 0xFFFFFFFF, "ba": None}, b"workgroups"),
              ({"na": BIG, "nb": BIG, "n": 1 << 20}, b"null handle")]          # a grid that fits is no error
    for kw, what in cases_:
        assert call(**kw) == -1, kw
        msg = L.lf_mkd_last_error(None)
        assert what in msg and msg.startswith(b"match_q8_guided_pairs_device"), (kw, msg)


def test_the_batch_has_the_sizes_and_the_layout():
    assert cases.SIZES[:2] == [(37, 300), (300, 37)] and (128, 128) in cases.SIZES and (129, 257) in cases.SIZES
    for s in [(1, 1), (1, 2), (2, 1), (0, 9), (5, 0), (33, 129), (130, 31), (600, 1003)]:
        assert s in cases.SIZES, s
    assert cases.SIZES[cases.ZERO_MODEL] == (40, 50) and cases.SIZES[cases.NAN_MODEL] == (30, 20)
    for kind in cases.KINDS:
        B = cases.batch(kind)
        assert [(int(B.oa[p + 1] - B.oa[p]), int(B.ob[p + 1] - B.ob[p])) for p in range(B.n_pairs)] == cases.SIZES
        assert int(B.oa[0]) == cases.LEAD[0] and int(B.ob[0]) == cases.LEAD[1]
        assert len(B.qa) - int(B.oa[-1]) == cases.TRAIL[0] and len(B.qb) - int(B.ob[-1]) == cases.TRAIL[1]
        assert np.array_equal(B.qa, qcases.quantize(B.a)) and B.qa.dtype == np.uint8
        assert not B.model[cases.ZERO_MODEL].any() and np.isnan(B.model[cases.NAN_MODEL]).sum() == 1
        assert np.isnan(B.ka[:, 2:]).all() and np.isnan(B.kb[:, 2:]).all() and not np.isnan(B.ka[:, :2]).any()
    assert len(cases.PLANTS) >= 2 and {P["rev"] for P in cases.PLANTS.values()} == {False, True}


def test_the_batch_covers_what_the_gpu_tests_need(masks):
    found = cases.coverage(masks)
    for key, c in found.items():
        print(f"[q8_guided] {key}: {c}")
    # no candidate at all under the all-zero and the NaN model
    for (kind, thr), m in masks.items():
        for p in (cases.ZERO_MODEL, cases.NAN_MODEL):
            assert not m[p][0].any() and not m[p][1].any() and m[p][0].size
        for fwd, rev, ref in m:
            assert np.array_equal(fwd, rev.T) and np.array_equal(fwd, ref)     # one relation, both directions; = the verifiers' test


def test_decide_follows_the_headers_sentences_on_tiny_inputs():
    rng = np.random.default_rng(31)
    x = rng.integers(1, 256, (6, 128)).astype(np.uint8)
    y = rng.integers(1, 256, (9, 128)).astype(np.uint8)
    y[7] = y[2]                                                                # a duplicated candidate
    x[0] = y[2]                                                                # ... that is row 0's best
    mask = rng.random((6, 9)) < 0.5
    mask[0] = True                                                             # both copies admissible: second == best, 7 wins
    mask[1] = False                                                            # no candidate
    mask[2] = False
    mask[2, 4] = True                                                          # one candidate
    x[3] = y[2]
    mask[3] = True
    mask[3, 7] = False                                                         # the higher copy inadmissible: 2 wins
    for ratio in (np.float32(0.8), np.float32(0.0)):
        got = cases.decide(x, y, mask, ratio)
        lo, hi = np.zeros(6, np.uint32), np.zeros(6, np.uint32)
        for i in range(6):                                                     # the loops of q8_cases over the gathered rows
            cand = np.flatnonzero(mask[i])
            if len(cand) == 0:
                want = (-1, cases.INT32_MIN, cases.INT32_MIN)
            else:
                m, s1, s2 = qcases.match_loops(x[i:i + 1], y[cand], ratio)
                want = (cand[m[0]] if m[0] >= 0 else -1, s1[0], s2[0])
            assert (got[0][i], got[1][i], got[2][i]) == want, (ratio, i)
    m, s1, s2 = cases.decide(x, y, mask, np.float32(0.0))
    assert m[0] == 7 and s1[0] == s2[0] and m[1] == -1 and s1[1] == s2[1] == cases.INT32_MIN
    assert m[2] == 4 and s2[2] == cases.INT32_MIN and m[3] == 2 and s2[3] < s1[3]
    m = cases.decide(x, y, mask, np.float32(0.8))[0]
    assert m[0] == -1 and m[2] == 4 and m[3] == 2                              # a tie fails the ratio test; one candidate passes
    # an empty and a one-row y side
    e = cases.decide(x, y[:0], np.zeros((6, 0), bool))
    assert (e[0] == -1).all() and (e[1] == cases.INT32_MIN).all() and (e[2] == cases.INT32_MIN).all()
    one = cases.decide(x, y[:1], np.array([[True], [False]] * 3))
    assert one[0].tolist() == [0, -1] * 3 and (one[2] == cases.INT32_MIN).all() and (one[1][1::2] == cases.INT32_MIN).all()
    assert cases.decide(x[:0], y, np.zeros((0, 9), bool))[0].shape == (0,)


def test_the_twins_masks_are_the_float64_predicate_away_from_the_boundary(masks):
    checked = near = 0
    for (kind, thr), m in masks.items():
        B = cases.batch(kind)
        for p in range(B.n_pairs):
            sa, sb = B.pair(p)
            if p in (cases.ZERO_MODEL, cases.NAN_MODEL) or m[p][0].size == 0:
                continue
            ok, res = gcases.f64_residual(kind, B.model[p], B.ka[sa, :2], B.kb[sb, :2], thr)
            clear = ~(np.abs(res - 1) <= 1e-5)
            assert np.array_equal(m[p][0][clear], ok[clear]), (kind, thr, p)
            checked += int(clear.sum())
            near += int((~clear).sum())
    print(f"[q8_guided] twin against float64: {checked} point pairs, {near} within 1e-5 of the boundary left out")
    assert checked > 1_000_000 and near < checked // 1000
