"""CPU tests of the 8-bit descriptors (include/lf_mkd.h, "8-bit descriptors"): the five symbols exist and refuse bad
arguments without a device, the launch plan keeps its invariants, the numpy restatements the GPU tests compare against
(tests/q8_cases.py) are right about themselves, and quantisation stays within its derived error bound."""
import ctypes
import glob
import os

import numpy as np
import pytest

import match_pairs_cases as pcases
import q8_cases as cases
from conftest import GOLDEN

import local_features_python as lfp

NAMES = ("lf_mkd_quantize_descriptors_device", "lf_mkd_quantize_descriptors", "lf_mkd_match_q8_device", "lf_mkd_match_q8",
         "lf_mkd_match_q8_plan")


def test_the_symbols_are_exported():
    L = lfp.load_library()
    for name in NAMES:
        assert name in lfp.SYMBOLS and hasattr(L, name), name
    for method in ("quantize", "dequantize", "match_q8"):
        assert hasattr(lfp.LocalFeatures, method), method
    for method in ("quantize", "match_q8", "quantize_descriptors_device", "match_q8_device"):
        assert hasattr(lfp.MkdHandle, method), method
    assert lfp.Q8_SCALE == 256.0


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(64)   # never dereferenced: the arguments are refused first
    big = (1 << 31) - 1
    sub = float(np.float32(1e-40))

    def refused(rc, who, what, kw):
        assert rc == -1, (who, kw)
        msg = L.lf_mkd_last_error(None)
        assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)

    # the quantiser, both forms
    for who, device in ((b"quantize_descriptors_device", True), (b"quantize_descriptors", False)):
        def call(x=p, n=8, scale=256.0, q=p):
            if device:
                return L.lf_mkd_quantize_descriptors_device(None, x, n, scale, q, None)
            return L.lf_mkd_quantize_descriptors(None, x, n, scale, q)
        table = [({}, b"null handle"), ({"n": 0}, b"null handle"), ({"scale": 0.0}, b"null handle"), ({"x": None}, b"null pointer"),
                 ({"q": None}, b"null pointer"), ({"scale": -1.0}, b"scale"), ({"scale": float("nan")}, b"scale"),
                 ({"scale": float("inf")}, b"scale"), ({"scale": sub}, b"scale"), ({"n": big + 1}, b"2^31")]
        if device:
            table += [({"x": ctypes.c_void_p(72)}, b"aligned"), ({"q": ctypes.c_void_p(66)}, b"aligned")]
        for kw, what in table:
            refused(call(**kw), who, what, kw)

    # the matcher, both forms
    def device_call(a=p, na=64, b=p, nb=64, lo=None, hi=None, m=p):
        return L.lf_mkd_match_q8_device(None, a, na, b, nb, lo, hi, 0.8, m, None, None, None)

    for kw, what in [({}, b"null handle"), ({"na": 0}, b"null handle"), ({"lo": p, "hi": p}, b"null handle"), ({"a": None}, b"null pointer"),
                     ({"b": None}, b"null pointer"), ({"m": None}, b"null pointer"), ({"lo": p}, b"go together"),
                     ({"hi": p}, b"go together"), ({"a": ctypes.c_void_p(72)}, b"aligned"), ({"b": ctypes.c_void_p(68)}, b"aligned"),
                     ({"nb": 1}, b"two candidates"), ({"nb": 0}, b"two candidates"), ({"na": big + 1}, b"2^31"),
                     ({"nb": 1 << 40}, b"2^31"), ({"na": big, "nb": big}, b"null handle")]:
        refused(device_call(**kw), b"match_q8_device", what, kw)

    def host_call(a=p, na=64, b=p, nb=64, m=p):
        return L.lf_mkd_match_q8(None, a, na, b, nb, 0.8, m)

    for kw, what in [({}, b"null handle"), ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"), ({"m": None}, b"null pointer"),
                     ({"a": ctypes.c_void_p(65)}, b"null handle"),           # host rows need no alignment
                     ({"nb": 1}, b"two candidates"), ({"na": big + 1}, b"2^31"), ({"nb": big + 1}, b"2^31")]:
        refused(host_call(**kw), b"match_q8", what, kw)

    # the plan
    for na, nb, what in ((5, 1, b"two candidates"), (5, 0, b"two candidates"), (big + 1, 5, b"2^31"), (5, big + 1, b"2^31")):
        refused(L.lf_mkd_match_q8_plan(na, nb, 0, None, None, None), b"match_q8_plan", what, (na, nb))
    assert L.lf_mkd_match_q8_plan(big, big, 0, None, None, None) == 0         # the largest problem, no output wanted


SIZES = [(1, 2), (1, 128), (1, 129), (31, 33), (32, 32), (513, 1025), (1024, 2000), (1025, 129), (2000, 2000), (300, 6000),
         (10000, 10000), (65536, 65536), (1 << 20, 1 << 20), (1, 1 << 20), (1 << 20, 2), ((1 << 31) - 1, (1 << 31) - 1)]


@pytest.mark.parametrize("num_cus", [0, 256, 1, 304])
def test_plan_invariants(num_cus):
    # rows per a block, from the plan itself: the largest na that is still one block
    rows = next(n for n in range(1, 1 << 16) if lfp.match_q8_plan(n + 1, 2, num_cus)[0] >= 2)
    for na, nb in SIZES:
        a_blocks, splits, scratch = lfp.match_q8_plan(na, nb, num_cus)
        b_tiles = (nb + 31) // 32
        assert a_blocks * rows >= na > (a_blocks - 1) * rows, (na, nb)
        assert 1 <= splits <= b_tiles, (na, nb, splits)
        assert a_blocks < (1 << 31) and splits < (1 << 16), (na, nb)          # a launchable grid
        assert (scratch == 0) == (splits == 1), (na, nb, splits, scratch)
        assert scratch == 0 or splits * na * 12 <= scratch <= 2 * 12 * splits * a_blocks * rows, (na, nb, splits, scratch)
    assert lfp.match_q8_plan(0, 5, num_cus) == (0, 1, 0)
    if num_cus == 0:
        assert [lfp.match_q8_plan(na, nb, 0) for na, nb in SIZES] == [lfp.match_q8_plan(na, nb, 256) for na, nb in SIZES]
    # the scratch is monotone in na: a handle warmed up on the largest a never allocates for a smaller one
    for nb in (2, 128, 129, 2000, 65536, 1 << 20):
        nas = sorted(set([1, 2, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5000, 65536, 1 << 18, (1 << 18) + 1,
                          1 << 19, (1 << 19) + 1, 1 << 20, (1 << 21) + 5, (1 << 31) - 1] + list(range(1, 1 << 20, 37 * 1024 + 1))))
        scratch = [lfp.match_q8_plan(na, nb, num_cus)[2] for na in nas]
        assert all(x <= y for x, y in zip(scratch, scratch[1:])), (nb, num_cus)


def test_the_restatement_against_loops():
    rng = np.random.default_rng(11)
    qa = rng.integers(1, 256, (7, 128)).astype(np.uint8)
    qb = rng.integers(1, 256, (9, 128)).astype(np.uint8)
    qb[6] = qb[2]                      # a duplicated b row ...
    qa[3] = qb[2]                      # ... that is row 3's best: best == second, the higher index wins
    qa[4] = 255                        # the extreme sums, both signs
    qb[0], qb[8] = 255, 1
    lo = np.array([0, 0, 3, 0, 1, 0, 4], np.uint32)
    hi = np.array([0, 8, 5, 0, 9, 9, 4], np.uint32)   # row 1: one candidate left (b row 8); row 4: one (row 0); row 5: none
    for ratio in (0.8, 0.0, 1.0):
        for ranges in ((None, None), (lo, hi)):
            got, want = cases.match_q8(qa, qb, ratio, *ranges), cases.match_loops(qa, qb, ratio, *ranges)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (ratio, ranges[0] is None)
    m, best, second = cases.match_q8(qa, qb, 0.8)
    assert best[3] == second[3] and cases.match_q8(qa, qb, 0.0)[0][3] == 6 and m[3] == -1
    assert best[4] == 128 * 127 * 127 == 2064512 and cases.similarities(qa[4:5], qb[8:9])[0, 0] == -2064512
    m, best, second = cases.match_q8(qa, qb, 0.8, lo, hi)
    assert m[1] == 8 and second[1] == cases.INT32_MIN and best[1] > cases.INT32_MIN          # one candidate: accepted
    assert m[4] == 0 and second[4] == cases.INT32_MIN
    assert m[5] == -1 and best[5] == second[5] == cases.INT32_MIN                             # none
    assert cases.match_q8(qa, qb, 0.0, lo, hi)[0][5] == -1


def test_the_quantiser_restatement():
    x = cases.edge_values()
    q = cases.quantize(x).astype(np.int32) - 128
    v = dict(zip(x[0].tolist(), q[0].tolist()))
    f = lambda m: float(np.float32(m) / np.float32(256))
    assert (v[f(0.5)], v[f(-0.5)], v[f(1.5)], v[f(-1.5)], v[f(2.5)]) == (0, 0, 2, -2, 2)     # ties to even
    assert (v[f(126.5)], v[f(127.5)], v[f(-127.5)], v[f(128.0)], v[f(127.49)]) == (126, 127, -127, 127, 127)
    assert (v[float(np.float32(0.496))], v[float(np.float32(-0.476))], v[1.0], v[-1.0]) == (127, -122, 127, -127)
    assert (v[float("inf")], v[float("-inf")], v[float(np.float32(3e38))]) == (127, -127, 127)
    assert q[0][np.isnan(x[0])].tolist() == [0] and (q[0][x[0] == 0] == 0).all()
    assert cases.quantize(x).min() >= 1                                                       # byte 0 never occurs
    assert np.array_equal(cases.quantize(x[:, :4], 100.0), cases.quantize(x, 100.0)[:, :4])
    d = lfp.LocalFeatures.dequantize(cases.quantize(x))
    ok = np.abs(x) < 0.49
    assert d.dtype == np.float32 and np.abs(d - x)[ok].max() <= 0.5 / 256


def _golden_rows():
    rows = [np.load(f)["desc_shader"] for f in sorted(glob.glob(os.path.join(GOLDEN, "patches_*.npz")))]
    assert len(rows) == 3
    return np.concatenate(rows).astype(np.float32)


def test_quantisation_error_bound():
    """|s / scale^2 - a.b| <= (|a|_1 + |b|_1) / (2 scale) + 128 / (4 scale^2) for every pair of unsaturated rows
    (q8_cases.error_bound derives it).  At scale 256 no synthetic row saturates; two of the 78 golden rows hold an element
    near 0.59 (above 127.5 / 256 = 0.498) and are outside the bound's premise."""
    a, b = pcases.descriptor_sets(513, 1025, 1002)
    g = _golden_rows()
    assert g.shape == (78, 128)
    assert not cases.saturated(a).any() and not cases.saturated(b).any()
    keep = ~cases.saturated(g)
    assert keep.sum() >= 76, int(keep.sum())
    for what, x, y in (("synthetic", a, b), ("golden", g[keep], g[keep])):
        s = cases.similarities(cases.quantize(x), cases.quantize(y)).astype(np.float64) / 256.0 ** 2
        true = x.astype(np.float64) @ y.astype(np.float64).T
        bound = cases.error_bound(np.abs(x.astype(np.float64)).sum(1)[:, None], np.abs(y.astype(np.float64)).sum(1)[None, :])
        err = np.abs(s - true)
        print(f"[q8] {what}: largest |s / scale^2 - a.b| = {err.max():.4f}, smallest bound {bound.min():.4f}")
        assert (err <= bound).all(), (what, err.max())
    # a coarser scale: the bound scales with it
    s = cases.similarities(cases.quantize(a, 100.0), cases.quantize(b, 100.0)).astype(np.float64) / 100.0 ** 2
    bound = cases.error_bound(np.abs(a.astype(np.float64)).sum(1)[:, None], np.abs(b.astype(np.float64)).sum(1)[None, :], 100.0)
    assert (np.abs(s - a.astype(np.float64) @ b.astype(np.float64).T) <= bound).all()


@pytest.mark.parametrize("p", [0, 2, 3, 6])
def test_quantised_decisions_on_the_shared_inputs(p):
    """On match_pairs_cases' clearly decided sets (seeds 1000, 1002, 1003, 1006) the 8-bit matcher takes the f64 matcher's
    decision for every row, and its similarities are within the bound of the f64 ones."""
    na, nb = pcases.SIZED[p]
    a, b = pcases.descriptor_sets(na, nb, 1000 + p)
    want, s1, s2 = pcases.match_f64(a, b)
    got, best, second = cases.match_q8(cases.quantize(a), cases.quantize(b))
    assert np.array_equal(got, want), (p, int((got != want).sum()))
    e = cases.error_bound(np.abs(a).sum(1), np.abs(b).sum(1).max())
    assert (np.abs(best / 256.0 ** 2 - s1) <= e).all() and (np.abs(second / 256.0 ** 2 - s2) <= e).all()
