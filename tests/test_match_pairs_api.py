"""CPU tests of the batched pair matcher (lf_mkd_match_pairs_device): the symbol exists and refuses bad arguments without a
device, and the numpy restatements the GPU tests use (tests/match_pairs_cases.py) -- the mutual rule, the slot map -- are
right about themselves; the shared inputs have the decision margins the oracle comparison relies on."""
import ctypes

import numpy as np

import match_pairs_cases as cases
import local_features_python as lfp


def test_the_symbol_is_exported():
    L = lfp.load_library()
    assert "lf_mkd_match_pairs_device" in lfp.SYMBOLS and hasattr(L, "lf_mkd_match_pairs_device")
    assert lfp.MATCH_MUTUAL == 1 and hasattr(lfp.MkdHandle, "match_pairs_device") and hasattr(lfp.LocalFeatures, "match_batch")


def test_bad_arguments_are_refused_without_a_device():
    L = lfp.load_library()
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first

    def call(**kw):
        a = dict(a=p, oa=p, na=64, b=p, ob=p, nb=64, n=4, flags=0, ab=p, ba=p, best=None, second=None)
        a.update(kw)
        return L.lf_mkd_match_pairs_device(None, a["a"], a["oa"], a["na"], a["b"], a["ob"], a["nb"], a["n"], 0.8, a["flags"],
                                           a["ab"], a["ba"], a["best"], a["second"], None)

    big = (1 << 31) - 1
    cases_ = [({}, b"null handle"), ({"n": 0}, b"null handle"), ({"a": None}, b"null pointer"), ({"b": None}, b"null pointer"),
              ({"oa": None}, b"null pointer"), ({"ob": None}, b"null pointer"), ({"ab": None}, b"null pointer"),
              ({"ba": None}, b"null handle"),                                  # one direction: d_match_ba may be NULL
              ({"ba": None, "flags": lfp.MATCH_MUTUAL}, b"d_match_ba"), ({"flags": 2}, b"unknown flag"),
              ({"flags": 0x80000001}, b"unknown flag"), ({"a": ctypes.c_void_p(24)}, b"aligned"),
              ({"b": ctypes.c_void_p(20)}, b"aligned"), ({"na": big + 1}, b"2^31"), ({"nb": 1 << 40}, b"2^31"),
              ({"na": big, "nb": big, "n": 1 << 30}, b"workgroups"),           # 2 x (2^27 + 2^30) slots
              ({"na": big, "n": 0xFFFFFFFF, "ba": None}, b"workgroups"),
              ({"na": big, "nb": big, "n": 1 << 20}, b"null handle")]          # a grid that fits is no error
    for kw, what in cases_:
        assert call(**kw) == -1, kw
        msg = L.lf_mkd_last_error(None)
        assert what in msg and msg.startswith(b"match_pairs_device"), (kw, msg)


def test_mutual_rule_restatement():
    oa, ob = np.array([0, 4, 4, 7]), np.array([2, 5, 6, 8])          # pair 1 has no a rows; b starts at row 2
    ab = np.array([0, 2, 2, -1, 1, 0, 5], np.int32)                  # (last: an index outside the pair's b rows)
    ba = np.array([-7, -7, 0, 3, 1, 0, 2, 0], np.int32)
    got_ab, got_ba = cases.mutual(ab, ba, oa, ob)
    # pair 0: a0 <-> b0 agree; a1 -> b2 and b2 -> a1 agree; a2 -> b2 does not (b2 -> a1); b1 -> a3 does not (a3 -> -1)
    assert got_ab.tolist() == [0, 2, -1, -1, 1, -1, -1]
    # pair 1 has a b row and no a row: nothing survives.  Pair 2 (a rows 4..6, b rows 6..7): row 4 -> b1 and b1 -> a0 (= row
    # 4) agree; row 5 -> b0 but b0 -> a2, and a2 -> 5 points outside the pair: none of the three survives
    assert got_ba.tolist() == [-7, -7, 0, -1, 1, -1, -1, 0]
    # every survivor is mutual, and filtering twice changes nothing
    again_ab, again_ba = cases.mutual(got_ab, got_ba, oa, ob)
    assert np.array_equal(again_ab, got_ab) and np.array_equal(again_ba, got_ba)
    # the two-launch order of the kernel: ab against the untouched ba, then ba against the FILTERED ab
    rng = np.random.default_rng(3)
    for _ in range(50):
        sizes = rng.integers(0, 9, (5, 2))
        oa, ob = np.concatenate([[0], np.cumsum(sizes[:, 0])]), np.concatenate([[0], np.cumsum(sizes[:, 1])])
        ab = np.concatenate([rng.integers(-1, max(nb, 1), na) if nb else np.full(na, -1) for na, nb in sizes]).astype(np.int32)
        ba = np.concatenate([rng.integers(-1, max(na, 1), nb) if na else np.full(nb, -1) for na, nb in sizes]).astype(np.int32)
        want_ab, want_ba = cases.mutual(ab, ba, oa, ob)
        step1, _ = cases.mutual(ab, ba, oa, ob)
        _, step2 = cases.mutual(step1, ba, oa, ob)
        assert np.array_equal(step2, want_ba)
        for p in range(5):
            x, y = want_ab[oa[p]:oa[p + 1]], want_ba[ob[p]:ob[p + 1]]
            assert all(y[j] == i for i, j in enumerate(x) if j >= 0) and all(x[i] == j for j, i in enumerate(y) if i >= 0)


def test_slot_map_covers_every_block_once_within_the_grid():
    rng = np.random.default_rng(8)
    for trial in range(300):
        n_pairs = int(rng.integers(1, 12))
        sizes = rng.integers(0, 70, n_pairs) * rng.integers(0, 2, n_pairs)           # about half of the pairs are empty
        if trial % 5 == 0:
            sizes = rng.integers(0, 3000, n_pairs)
        first = int(rng.integers(0, 40)) if trial % 2 else 0                         # offsets[0] above zero
        offsets = first + np.concatenate([[0], np.cumsum(sizes)])
        n_total = int(offsets[-1]) + (int(rng.integers(0, 40)) if trial % 3 else 0)  # rows behind the last pair
        grid = cases.grid_slots(n_total, n_pairs)
        seen = {}
        for slot in range(grid + 20):                                                 # beyond the grid nothing is owed
            pb = cases.slot_to_block(offsets, n_total, slot)
            if pb is not None:
                assert pb not in seen, (offsets, slot, pb, seen[pb])                  # no block is served twice
                assert slot < grid, (offsets, n_total, slot, grid)                    # the grid bound suffices
                seen[pb] = slot
        want = {(p, k) for p in range(n_pairs) for k in range((int(sizes[p]) + 15) // 16)}
        assert set(seen) == want, (offsets, set(seen) ^ want)
    # offsets beyond the total are read as the total, an inverted pair is empty: never a row at or beyond the total
    offsets, n_total = np.array([0, 40, 30, 1000, 90]), 64
    for slot in range(cases.grid_slots(n_total, 4) + 5):
        pb = cases.slot_to_block(offsets, n_total, slot)
        if pb is not None:
            lo = min(int(offsets[pb[0]]), n_total)
            assert lo + pb[1] * 16 < n_total


def test_the_shared_inputs_decide_clearly():
    """In float64 no row of a sized pair (or of the pair beyond the one-launch form) has best * 0.8 or best within 4e-6 of
    second -- twice the band the oracle comparison excuses; in the b -> a direction the second condition holds for the
    accepted rows (a rejected row is -1 whichever candidate is best), so no decision of either direction is excusable;
    both outcomes of the ratio test occur, and the mutual rule keeps some matches and drops others."""
    for a, b, kind in cases.ragged_batch():
        if kind == "degenerate":
            continue
        res = {}
        for name, (x, y) in (("ab", (a, b)), ("ba", (b, a))):
            if len(y) < 2:
                res[name] = np.full(len(x), -1, np.int32)
                continue
            m, s1, s2 = cases.match_f64(x, y)
            gap = np.abs(s1 - s2)
            if name == "ba":        # descriptor_sets gives a fifth of a's rows ONE unrelated vector, so b rows do meet two equal or
                gap = gap[m >= 0]   # nearly equal candidates in a -- and reject them: -1 whichever of the two is called best
            assert np.abs(0.8 * s1 - s2).min() >= 4e-6 and gap.min(initial=1.0) >= 4e-6, (len(a), len(b), name)
            res[name] = m
        if len(a) >= 250:
            acc = (res["ab"] >= 0).mean()
            assert 0.1 < acc <= 1.0, (len(a), len(b), acc)
            o = np.array([0, len(a)]), np.array([0, len(b)])
            kept = (cases.mutual(res["ab"], res["ba"], *o)[0] >= 0).sum()
            assert 0 < kept < (res["ab"] >= 0).sum(), (len(a), len(b), kept)
