"""CPU tests of the batched int8 matcher (lf_mkd_match_q8_pairs_device, lf_mkd_match_q8_pairs_plan): the symbols exist and
refuse bad arguments without a device, the plan function is the stated formula, and the numpy restatements the GPU tests
use (tests/q8_pairs_cases.py) -- the per-pair decision, the slot map at the plan's block size, the decoys of the shared
batch -- are right about themselves."""
import ctypes

import numpy as np
import pytest

import match_pairs_cases as pcases
import q8_cases as qcases
import q8_pairs_cases as cases
import local_features_python as lfp

BIG = (1 << 31) - 1


def block_rows():
    return lfp.match_q8_pairs_plan(0, 0, 0)[0]


def test_the_symbols_are_exported():
    L = lfp.load_library()
    for name in ("lf_mkd_match_q8_pairs_device", "lf_mkd_match_q8_pairs_plan"):
        assert name in lfp.SYMBOLS and hasattr(L, name), name
    assert hasattr(lfp.MkdHandle, "match_q8_pairs_device") and hasattr(lfp.LocalFeatures, "match_q8_batch")
    assert "match_q8_pairs_plan" in lfp.__all__ and callable(lfp.match_q8_pairs_plan)


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first

    def call(**kw):
        a = dict(a=p, oa=p, na=64, b=p, ob=p, nb=64, n=4, flags=0, ab=p, ba=p, best=None, second=None)
        a.update(kw)
        return L.lf_mkd_match_q8_pairs_device(None, a["a"], a["oa"], a["na"], a["b"], a["ob"], a["nb"], a["n"], 0.8, a["flags"],
                                              a["ab"], a["ba"], a["best"], a["second"], None)

    cases_ = [({}, b"null handle"), ({"n": 0}, b"null handle"), ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"),
              ({"oa": None}, b"null pointer"), ({"ob": None}, b"null pointer"), ({"ab": None}, b"null pointer"),
              ({"ba": None}, b"null handle"),                                  # one direction: d_match_ba may be NULL
              ({"ba": None, "flags": lfp.MATCH_MUTUAL}, b"d_match_ba"), ({"flags": 2}, b"unknown flag"),
              ({"flags": 0x80000001}, b"unknown flag"), ({"a": ctypes.c_void_p(24)}, b"aligned"),
              ({"b": ctypes.c_void_p(20)}, b"aligned"), ({"na": BIG + 1}, b"2^31"), ({"nb": 1 << 40}, b"2^31"),
              ({"na": BIG, "nb": BIG, "n": 1 << 30}, b"workgroups"),           # 2 x (at least 2^30) slots
              ({"na": BIG, "n": 0xFFFFFFFF, "ba": None}, b"workgroups"),
              ({"na": BIG, "nb": BIG, "n": 1 << 20}, b"null handle")]          # a grid that fits is no error
    for kw, what in cases_:
        assert call(**kw) == -1, kw
        msg = L.lf_mkd_last_error(None)
        assert what in msg and msg.startswith(b"match_q8_pairs_device"), (kw, msg)


def test_plan_is_the_formula():
    L = lfp.load_library()
    R = block_rows()
    assert R in (128, 256, 512) and R & (R - 1) == 0
    rng = np.random.default_rng(12)
    for _ in range(300):
        na, nb = int(rng.integers(0, 1 << int(rng.integers(1, 31)))), int(rng.integers(0, 1 << int(rng.integers(1, 31))))
        n = int(rng.integers(0, 1 << int(rng.integers(1, 20))))
        r1, one = lfp.match_q8_pairs_plan(na, nb, n)
        r2, both = lfp.match_q8_pairs_plan(na, nb, n, True)
        assert r1 == r2 == R                                                 # a constant of the build: no size changes it
        assert one == na // R + n and both == one + nb // R + n, (na, nb, n)
        assert one == cases.grid_slots(na, n, R)
    # the totals' and the grid's limits, as the launch refuses them; a grid of exactly 2^31 - 1 workgroups fits
    assert lfp.match_q8_pairs_plan(BIG, BIG, 0, True) == (R, 2 * (BIG // R))
    fits = BIG - BIG // R
    assert lfp.match_q8_pairs_plan(BIG, 0, fits) == (R, BIG)
    for args, what in (((BIG + 1, 0, 1, False), "2^31"), ((0, BIG + 1, 1, False), "2^31"), ((0, 1 << 40, 1, True), "2^31"),
                       ((BIG, 0, fits + 1, False), "workgroups"), ((BIG, BIG, 1 << 30, True), "workgroups"),
                       ((0, 0, 0xFFFFFFFF, True), "workgroups")):
        with pytest.raises(RuntimeError, match="match_q8_pairs_plan") as e:
            lfp.match_q8_pairs_plan(*args)
        assert what in str(e.value), (args, str(e.value))
    # output pointers may be NULL
    assert L.lf_mkd_match_q8_pairs_plan(1000, 1000, 3, 1, None, None) == 0
    w = ctypes.c_uint64()
    assert L.lf_mkd_match_q8_pairs_plan(1000, 1000, 3, 1, None, ctypes.byref(w)) == 0 and w.value == 2 * (1000 // R + 3)


def test_slot_map_covers_every_block_once_within_the_grid():
    R = block_rows()
    rng = np.random.default_rng(8)
    for trial in range(300):
        n_pairs = int(rng.integers(1, 12))
        sizes = rng.integers(0, 5 * R, n_pairs) * rng.integers(0, 2, n_pairs)        # about half of the pairs are empty
        if trial % 5 == 0:
            sizes = rng.integers(0, 40 * R, n_pairs)
        if trial % 7 == 0:
            sizes = rng.integers(0, 4, n_pairs) * R + rng.integers(-1, 2, n_pairs) * rng.integers(0, 2, n_pairs)   # around multiples of R
            sizes = np.maximum(sizes, 0)
        first = int(rng.integers(0, 3 * R)) if trial % 2 else 0                       # offsets[0] above zero
        offsets = first + np.concatenate([[0], np.cumsum(sizes)])
        n_total = int(offsets[-1]) + (int(rng.integers(0, 3 * R)) if trial % 3 else 0)   # rows behind the last pair
        grid = lfp.match_q8_pairs_plan(n_total, 0, n_pairs)[1]
        assert grid == cases.grid_slots(n_total, n_pairs, R)
        seen = {}
        for slot in range(grid + 20):                                                 # beyond the grid nothing is owed
            pb = cases.slot_to_block(offsets, n_total, slot, R)
            if pb is not None:
                assert pb not in seen, (offsets, slot, pb, seen[pb])                  # no block is served twice
                assert slot < grid, (offsets, n_total, slot, grid)                    # the grid bound suffices
                seen[pb] = slot
        want = {(p, k) for p in range(n_pairs) for k in range((int(sizes[p]) + R - 1) // R)}
        assert set(seen) == want, (offsets, set(seen) ^ want)
    # offsets beyond the total are read as the total, an inverted pair is empty: never a row at or beyond the total
    offsets, n_total = np.array([0, 2 * R + 40, 30, 100 * R, R + 90]), 3 * R + 64
    served = 0
    for slot in range(cases.grid_slots(n_total, 4, R) + 5):
        pb = cases.slot_to_block(offsets, n_total, slot, R)
        if pb is not None:
            lo = min(int(offsets[pb[0]]), n_total)
            assert lo + pb[1] * R < n_total
            served += 1
    assert served >= 4


def test_match_pairs_restatement_on_tiny_inputs():
    rng = np.random.default_rng(21)
    sizes = [(3, 4), (0, 5), (4, 1), (2, 2), (5, 0), (1, 3)]
    qa = rng.integers(1, 256, (2 + sum(s[0] for s in sizes) + 1, 128)).astype(np.uint8)
    qb = rng.integers(1, 256, (1 + sum(s[1] for s in sizes) + 2, 128)).astype(np.uint8)
    qb[3] = qb[2]                                                             # a duplicated maximum candidate in pair 0
    oa = 2 + np.cumsum([0] + [s[0] for s in sizes])
    ob = 1 + np.cumsum([0] + [s[1] for s in sizes])
    for ratio in (np.float32(0.8), np.float32(0.0)):
        ab, ba, best, second = cases.match_pairs(qa, oa, qb, ob, ratio)
        for p, (na, nb) in enumerate(sizes):
            x, y = qa[oa[p]:oa[p + 1]], qb[ob[p]:ob[p + 1]]
            sa, sb = slice(oa[p], oa[p + 1]), slice(ob[p], ob[p + 1])
            if nb >= 2:
                m, s1, s2 = qcases.match_loops(x, y, ratio) if na else (np.zeros(0, np.int32),) * 3
                assert np.array_equal(ab[sa], m) and np.array_equal(best[sa], s1) and np.array_equal(second[sa], s2), (p, ratio)
            else:                                                             # too few candidates: -1 / INT32_MIN whatever the ratio
                assert (ab[sa] == -1).all() and (best[sa] == cases.INT32_MIN).all() and (second[sa] == cases.INT32_MIN).all(), p
            if na >= 2:
                m = qcases.match_loops(y, x, ratio)[0] if nb else np.zeros(0, np.int32)
                assert np.array_equal(ba[sb], m), (p, ratio)
            else:
                assert (ba[sb] == -1).all(), p
        # rows outside every pair keep the fill
        assert (ab[:2] == cases.SENTINEL).all() and (ab[oa[-1]:] == cases.SENTINEL).all() and (best[:2] == cases.SENTINEL).all()
        assert (ba[:1] == cases.SENTINEL).all() and (ba[ob[-1]:] == cases.SENTINEL).all()
    # offsets beyond the totals and an inverted pair
    ab, ba, _, _ = cases.match_pairs(qa[:6], [0, 4, 2, 2], qb[:7], [0, 3, 7, 900], np.float32(0.0))
    assert (ab[:4] >= 0).all() and (ab[4:] == cases.SENTINEL).all()           # pair 1 is inverted on the a side: no a row
    assert (ba[:3] >= 0).all() and (ba[3:7] == -1).all()                      # ... and its b rows find no candidates


def test_the_ragged_batch_decides_both_ways_and_its_decoys_bite():
    R = block_rows()
    qa, oa, qb, ob, sizes = cases.ragged_q8_batch(R)
    ab, ba, best, second = cases.ragged_reference(R)
    assert len(sizes) == len(pcases.ragged_batch()) + len(cases.edge_sizes(R)) and len(oa) == len(sizes) + 1
    assert all(s in sizes for s in pcases.DEGENERATE + [pcases.BEYOND] + cases.edge_sizes(R))
    assert int(oa[0]) == cases.LEAD[0] and int(ob[0]) == cases.LEAD[1]
    assert len(qa) - int(oa[-1]) == cases.TRAIL[0] and len(qb) - int(ob[-1]) == cases.TRAIL[1]
    assert (oa[:-1][np.diff(oa) > 0] % 32 != 0).all() and (ob[:-1][np.diff(ob) > 0] % 32 != 0).all()   # no pair starts on a tile border
    assert qa.min() >= 1 and qb.min() >= 1                                                    # the format: byte 0 never occurs
    inside = slice(int(oa[0]), int(oa[-1]))
    assert (ab[inside] >= 0).sum() > 1000 and (ab[inside] == -1).sum() > 1000                 # both outcomes of the ratio test
    assert (best[inside][ab[inside] >= 0].astype(np.float32) * cases.RATIO > second[inside][ab[inside] >= 0].astype(np.float32)).all()
    m_ab, m_ba = pcases.mutual(ab, ba, oa, ob)
    kept = (m_ab[inside] >= 0).sum()
    assert 0 < kept < (ab[inside] >= 0).sum() and kept == (m_ba[int(ob[0]):int(ob[-1])] >= 0).sum()
    # the decoys: letting three more rows in on either side of a pair's b rows changes the pair's result
    hit = cases.decoys_bite(R)
    assert len(hit) >= 1, "the decoys prove nothing"
    print(f"[q8_pairs] R = {R}: {len(sizes)} pairs, {len(qa)} x {len(qb)} rows, {(ab[inside] >= 0).sum()} accepted, {kept} mutual; "
          f"widening the b rows changes {len(hit)} pairs: {hit}")
