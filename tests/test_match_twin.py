"""The screen matcher's host twin (tests/cpp/match_twin.cpp: an exhaustive scan with match_verify's f32 dot product) against
the oracle and float64, and the conditions that prove tests/match_cases.py's inputs reach what they are meant to reach --
all on the CPU.  The device is held to the twin bit for bit by tests/test_gpu_match_exact.py; this module is what ties the
twin to the reference's match_features, and what keeps that module's cases from going vacuous unnoticed.

Bounds:
  * twin against oracle.match: 2e-6 on the similarities, identical decisions outside near-ties (test_gpu_match.compare,
    the bound the device's three-term forms are held to);
  * twin against float64: 128 x 2^-24 x sum |a_k b_k| -- the chain of 8 and the tree of 4 are 11 roundings deep, each of
    at most 2^-24 of the partial sums' magnitude, which sum |a_k b_k| bounds; 128 is the serial sum's depth and leaves room;
  * the dot product's order: a numpy restatement, lane by lane (f32 fma emulated as the f32 rounding of the float64
    a * b + c, the product exact), must give the twin's bits on 300 rows with a wide dynamic range.

margin_inversion reaches an inversion of 0.623 to 0.629 of the margin on its 12 queries (the construction's limit is
0.65 |b_t| / max|b| and the planted norms are ~0.98 of the ordinary rows'); the check's lower cap is the issue's 0.55."""
import numpy as np
import pytest

import match_cases as mc
import match_twin as mt
from test_gpu_match import compare, descriptor_sets, unit


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """(program, scratch directory): one g++ build for the module"""
    tmp = tmp_path_factory.mktemp("match_twin")
    return mt.build(tmp), tmp


def test_twin_agrees_with_the_oracle(twin, oracle):
    a, b = descriptor_sets(1500, 3000, 4500)
    want, s1, s2 = oracle.match(a, b)
    assert 0.1 < (want >= 0).mean() < 0.95
    got = mt.scan(*twin, a, b, 0.8)
    compare(got.match, got.best, got.second, want, s1, s2, np.float32(0.8), "twin, 1500 x 3000")
    # cross-image exclusion (test_gpu_match.test_cross_image_exclusion's input)
    rng = np.random.default_rng(2)
    sizes = [300, 17, 450, 233, 64, 1]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    nb = int(starts[-1])
    base = unit(rng.normal(size=(500, 128)))
    b = unit(base[rng.integers(0, 500, nb)] + 0.08 * rng.normal(size=(nb, 128)))
    img = np.repeat(np.arange(len(sizes)), sizes)
    lo, hi = starts[img].astype(np.uint32), starts[img + 1].astype(np.uint32)
    want, s1, s2 = oracle.match(b, b, exclude=(lo, hi))
    got = mt.scan(*twin, b, b, 0.8, lo, hi)
    assert (img[got.match[got.match >= 0]] != img[got.match >= 0]).all()
    compare(got.match, got.best, got.second, want, s1, s2, np.float32(0.8), "twin, cross-image")


@pytest.mark.parametrize("which", ["unit", "scaled", "signs"])
def test_twin_agrees_with_float64(twin, which):
    if which == "unit":
        a, b = descriptor_sets(400, 900, 7)
        lo = hi = None
    elif which == "scaled":
        a, b, lo, hi, _ = mc.scaled(3e-5, 2e-4, 300, 600)
    else:
        a, b, lo, hi, _ = mc.signs_and_zeros()
    got = mt.scan(*twin, a, b, 0.0, lo, hi, wide=True)
    bound = 128 * 2.0 ** -24 * got.sabs
    e1, e2 = np.abs(got.best - got.best64), np.abs(got.second - got.second64)
    print(f"{which}: worst |f32 - f64| / bound: best {np.max(e1 / np.maximum(bound, 1e-300)):.3f}, "
          f"second {np.max(e2 / np.maximum(bound, 1e-300)):.3f}")
    assert (e1 <= bound).all() and (e2 <= bound).all()
    s = mc.mask_excluded(mc.exact(a, b), lo, hi)
    _, s1, s2 = mc.top2(s)
    assert np.allclose(got.best64, s1, rtol=1e-12, atol=0) and np.allclose(got.second64, s2, rtol=1e-12, atol=0)


def _f32_fma(x, y, acc):
    return (x.astype(np.float64) * y.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def test_the_twin_takes_the_kernels_order(twin):
    """lane l: a[8l] * b[8l], then fmaf over j = 1 .. 7; then p += p[l ^ 8], ^ 4, ^ 2, ^ 1 -- restated in numpy"""
    rng = np.random.default_rng(9)
    n = 300
    a = (rng.normal(size=(n, 128)) * 10.0 ** rng.uniform(-3, 3, (n, 128))).astype(np.float32)
    b = (rng.normal(size=(1, 128)) * 10.0 ** rng.uniform(-3, 3, (1, 128))).astype(np.float32)
    got = mt.scan(*twin, a, b.repeat(2, axis=0), 0.0)     # (the same candidate twice: best = second, the later index)
    al, bl = a.reshape(n, 16, 8), b[0].reshape(16, 8)
    p = al[:, :, 0] * bl[None, :, 0]
    for j in range(1, 8):
        p = _f32_fma(al[:, :, j], np.broadcast_to(bl[None, :, j], p.shape), p)
    for m in (8, 4, 2, 1):
        p = p + p[:, np.arange(16) ^ m]
    assert p.dtype == np.float32 and (p == p[:, :1]).all()
    assert np.array_equal(got.best.view(np.int32), p[:, 0].view(np.int32))
    assert np.array_equal(got.second.view(np.int32), p[:, 0].view(np.int32)) and (got.match == 1).all()
    serial = (a.astype(np.float64) @ b[0].astype(np.float64)).astype(np.float32)
    assert (serial != p[:, 0]).any(), "the input tells the orders apart"


def test_ties_and_ratios(twin):
    rng = np.random.default_rng(1)
    b = unit(rng.normal(size=(300, 128)))
    b[250] = b[17]
    b[299] = b[40]
    a = np.concatenate([b[17:18], b[40:41], b[5:6], unit(rng.normal(size=(5, 128)))])
    got = mt.scan(*twin, a, b, 0.8)
    assert got.match[0] == -1 and got.match[1] == -1 and got.match[2] == 5
    assert got.best[0] == got.second[0] and got.best[1] == got.second[1]
    one = mt.scan(*twin, a, b, 1.0)
    assert one.match[0] == -1 and one.match[1] == -1 and (one.match[2:] >= 0).all()     # a strict best passes ratio 1
    raw = mt.scan(*twin, a, b, 0.0)
    assert raw.match[0] == 250 and raw.match[1] == 299 and (raw.match >= 0).all()        # the highest index among equals
    assert np.array_equal(raw.match[2:], one.match[2:])
    for r in (got, one, raw):
        assert np.array_equal(r.best.view(np.int32), raw.best.view(np.int32))
    # an excluded duplicate leaves the other; everything excluded leaves nothing
    lo, hi = np.zeros(len(a), np.uint32), np.zeros(len(a), np.uint32)
    lo[0], hi[0] = 250, 251
    lo[1], hi[1] = 0, 300
    ex = mt.scan(*twin, a, b, 0.0, lo, hi)
    assert ex.match[0] == 17 and ex.match[1] == -1 and ex.best[1] == -np.inf and ex.second[1] == -np.inf


CASES = {
    "margin_inversion": (mc.margin_inversion, mc.check_margin_inversion),
    "floor_mixup stride 1": (lambda: mc.floor_mixup(1), mc.check_floor_mixup),
    "floor_mixup stride 16": (lambda: mc.floor_mixup(16), mc.check_floor_mixup),
    "floor_mixup stride 64": (lambda: mc.floor_mixup(64), mc.check_floor_mixup),
    "ring_ladder 64 tight": (lambda: mc.ring_ladder(64, True), mc.check_ring_ladder),
    "ring_ladder 64 tight descending": (lambda: mc.ring_ladder(64, True, True), mc.check_ring_ladder),
    "ring_ladder 65 tight": (lambda: mc.ring_ladder(65, True), mc.check_ring_ladder),
    "ring_ladder 100 steps": (lambda: mc.ring_ladder(100, False), mc.check_ring_ladder),
    "crowded_with_exclusion 4": (lambda: mc.crowded_with_exclusion(4), mc.check_crowded_with_exclusion),
    "crowded_with_exclusion 16400": (lambda: mc.crowded_with_exclusion(16400), mc.check_crowded_with_exclusion),
    "signs_and_zeros": (mc.signs_and_zeros, mc.check_signs_and_zeros),
    **{f"scaled {sa:g} x {sb:g}": (lambda sa=sa, sb=sb: mc.scaled(sa, sb), mc.check_scaled) for sa, sb in mc.SCALES},
}


@pytest.mark.parametrize("name", list(CASES))
def test_a_case_reaches_what_it_is_meant_to(name):
    make, check = CASES[name]
    case = make()
    a, b, lo, hi, what = case
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape[1] == 128 and b.shape[1] == 128
    assert (lo is None) == (hi is None) and (lo is None or (lo.dtype == np.uint32 and hi.dtype == np.uint32 and len(lo) == len(a)))
    print(name, "->", check(case))


def test_the_twin_sees_what_the_cases_plant(twin):
    """the planted answers, as the twin finds them: the true best of margin_inversion's queries, the low rows' candidates of
    floor_mixup, the ladder's top, the zero row's last index"""
    a, b, _, _, what = mc.margin_inversion()
    got = mt.scan(*twin, a, b, 0.0)
    for q, t, ds in what["planted"]:
        assert got.match[q] == t and 1e-5 <= got.best[q] - got.second[q] <= 1e-4
    a, b, _, _, what = mc.floor_mixup(1)
    got = mt.scan(*twin, a, b, 0.8)
    assert all(got.match[i] == r[0] or got.match[i] == -1 for i, r in what["plan"].items())
    assert (mt.scan(*twin, a, b, 0.0).match == np.array([what["plan"][i][0] for i in range(len(a))])).all()
    a, b, _, _, what = mc.ring_ladder(100, False)
    got = mt.scan(*twin, a, b, 0.0)
    assert got.match[what["query"]] == what["rows"][-1]
    a, b, lo, hi, what = mc.signs_and_zeros()
    got = mt.scan(*twin, a, b, 0.0, lo, hi)
    assert got.match[what["zero_a"]] == len(b) - 1 and got.match[what["dup"][0]] == what["dup"][2]
    assert (got.best[what["negated"]] <= 0).all() and (got.best[what["negated"][::2]] < -0.1).all()
