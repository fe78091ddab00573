"""RANSAC fundamental-matrix verification on the GPU held to its host twin bit for bit.  The twin
(tests/cpp/fundamental_twin.cpp, driven by tests/fundamental_twin.py) is the kernel's own math header,
local-features_amd/csrc/mkd_fundamental_math.h, compiled by g++, under a serial restatement of the two kernels; it is tied
to the algorithm of include/lf_mkd.h by tests/test_fundamental_twin.py on the CPU.  No tolerance anywhere here: F, verified
and stats are compared as uint32 / int32 words -- every sample of five problem families, whole calls with and without the
refit across the hypothesis-block and row-slice edges, the ragged batch, and the edge cases of tests/fundamental_cases.py."""
import numpy as np
import pytest

import fundamental_cases as fc
import fundamental_twin as ft
from fundamental_cases import FAMILIES, THR, two_view

import local_features_python as lfp

pytestmark = pytest.mark.gpu

NO_REFINE = lfp.VERIFY_NO_REFINE
INVALID = ft.INVALID


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """(program, scratch directory): one g++ build for the module"""
    tmp = tmp_path_factory.mktemp("fundamental_twin")
    return ft.build(tmp), tmp


def _device_batch(handle, pairs, n_hyp, seed, flags=0, thr=THR):
    """Pairs in one lf_mkd_verify_fundamental_device call: (F [n, 9] f32, verified [Na] int32, stats [n, 4] uint32, a offsets)."""
    import torch
    oa = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ob = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    ka = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[0] for p in pairs]), np.float32).reshape(-1, 5)).cuda()
    kb = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[1] for p in pairs]), np.float32).reshape(-1, 5)).cuda()
    mt = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[2] for p in pairs]), np.int32)).cuda()
    d_oa, d_ob = torch.from_numpy(oa).cuda(), torch.from_numpy(ob).cuda()
    n = len(pairs)
    F = torch.full((n, 9), np.nan, device="cuda")
    ver = torch.full((max(len(mt), 1),), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    handle.verify_fundamental_device(ka.data_ptr(), d_oa.data_ptr(), kb.data_ptr(), d_ob.data_ptr(), mt.data_ptr(), n,
                                     F.data_ptr(), ver.data_ptr(), st.data_ptr(), n_hyp, thr, seed, flags,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return F.cpu().numpy(), ver.cpu().numpy()[:len(mt)], st.cpu().numpy().view(np.uint32), oa


def _assert_equal_to_twin(want, F, ver, st, what):
    got = np.ascontiguousarray(F, np.float32).reshape(-1).view(np.uint32)
    assert np.array_equal(got, want["F"].reshape(-1).view(np.uint32)), (what, np.asarray(F).reshape(-1), want["F"].reshape(-1))
    assert np.array_equal(np.asarray(st).view(np.uint32), want["stats"]), (what, st, want["stats"])
    assert np.array_equal(ver, want["verified"]), (what, int((ver != want["verified"]).sum()))


def _assert_outcome(F, ver, st, mt, what):
    """What include/lf_mkd.h promises of any call: no candidate -> all zero / -1 / 0xFFFFFFFF; else a finite F whose largest
    entry is exactly +1, and verified = match on as many rows as stats[0] says and -1 elsewhere."""
    F, st = np.asarray(F, np.float32).reshape(-1), np.asarray(st).view(np.uint32).astype(np.int64)
    if st[2] == INVALID:
        assert st[0] == 0 and st[1] == 0 and (F == 0).all() and (ver == -1).all(), (what, st)
        return
    assert np.isfinite(F).all() and np.abs(F).max() == 1.0 and F[int(np.argmax(np.abs(F)))] == 1.0, (what, F)
    keep = ver >= 0
    assert keep.sum() == st[0] and np.array_equal(ver[keep], np.asarray(mt)[keep]) and (ver[~keep] == -1).all(), (what, st)


# ---- every sample, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_every_sample_bit_for_bit(handle, twin, family):
    """N copies of one problem, n_hypotheses = 1, no refit: pair p reports the best candidate of sample 0 of seed s + p."""
    n = 512 if family == "general" else 256
    ka, kb, mt, _ = two_view(200, 0.4, 900 + len(family), family)
    seed = 0xF00D + 131 * len(family)
    F, ver, st, oa = _device_batch(handle, [(ka, kb, mt)] * n, 1, seed, NO_REFINE)
    want = ft.run_calls(twin[0], [ft.Call(ka, kb, mt, seed + np.arange(n), 1, THR, NO_REFINE, records=True)], twin[1])[0]
    assert len(want) == n
    want_F = np.stack([w["F"].reshape(-1) for w in want])
    want_st = np.stack([w["stats"] for w in want])
    want_ver = np.stack([w["verified"] for w in want])
    bad = np.flatnonzero((F.view(np.uint32) != want_F.view(np.uint32)).any(axis=1) | (st != want_st).any(axis=1)
                         | (ver.reshape(n, -1) != want_ver).any(axis=1))
    assert len(bad) == 0, (family, len(bad), bad[:8], st[bad[:4]], want_st[bad[:4]])
    # the twin's answer is its record of that sample: the largest count, the first slot on a tie
    slots = set()
    for p, w in enumerate(want):
        rec = w["records"][0]
        cnt = np.where(rec["count"] == INVALID, -1, rec["count"].astype(np.int64))
        if cnt.max() < 0:
            assert st[p].tolist() == [0, 0, INVALID, 200], p
            continue
        j = int(np.argmax(cnt))
        slots.add(j)
        assert st[p, 2] == j and st[p, 1] == cnt[j] and st[p, 0] == cnt[j], (p, st[p], cnt)
        f = rec["f"][j]
        assert np.array_equal(F[p].view(np.uint32), (f / f[int(np.argmax(np.abs(f)))]).view(np.uint32)), p
    assert slots == {0, 1, 2}, (family, slots)     # the family reaches every slot


# ---- whole calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("m,n_hyp", [(7, 1), (50, 255), (1000, 256), (1000, 257), (2000, 512)])
def test_whole_calls(handle, twin, family, m, n_hyp):
    ka, kb, mt, _ = two_view(m, 0.0 if m == 7 else 0.4, 700 + m + n_hyp, family)
    calls = [ft.Call(ka, kb, mt, 29, n_hyp, THR, flags) for flags in (0, NO_REFINE)]
    for (want,), flags in zip(ft.run_calls(twin[0], calls, twin[1]), (0, NO_REFINE)):
        F, ver, st = handle.verify_fundamental(ka, kb, mt, n_hyp, THR, 29, flags)
        _assert_equal_to_twin(want, F, ver, st, (family, m, n_hyp, flags))
        _assert_outcome(F, ver, st, mt, (family, m, n_hyp, flags))


def test_most_row_slices_and_fewest(handle, twin):
    """20000 rows: alone the pair is scored in the most row slices a call takes, inside a 48-pair batch in few."""
    ka, kb, mt, _ = two_view(20000, 0.4, 77)
    seed, at = 61, 5
    (want,), (plain,) = ft.run_calls(twin[0], [ft.Call(ka, kb, mt, seed + at, 256, THR, 0),
                                                ft.Call(ka, kb, mt, seed + at, 256, THR, NO_REFINE)], twin[1])
    assert want["stats"][0] > 10000 and want["stats"][2] != INVALID
    F, ver, st = handle.verify_fundamental(ka, kb, mt, 256, THR, seed + at, 0)
    _assert_equal_to_twin(want, F, ver, st, "single")
    F, ver, st = handle.verify_fundamental(ka, kb, mt, 256, THR, seed + at, NO_REFINE)
    _assert_equal_to_twin(plain, F, ver, st, "single, no refit")
    pairs = fc.pairs(48)
    pairs[at] = (ka, kb, mt)
    F, ver, st, oa = _device_batch(handle, pairs, 256, seed)
    _assert_equal_to_twin(want, F[at], ver[oa[at]:oa[at + 1]], st[at], "in a batch")


# ---- the ragged batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, NO_REFINE])
def test_ragged_batch(handle, twin, flags):
    """-1 and out-of-range matches, unmatched b rows, empty pairs, M < 7 and M = 7, every family: pair by pair."""
    pairs = fc.pairs()
    F, ver, st, oa = _device_batch(handle, pairs, 512, 40, flags)
    want = ft.run_calls(twin[0], [ft.Call(*p, 40 + i, 512, THR, flags) for i, p in enumerate(pairs)], twin[1])
    for p, ((w,), (ka, kb, mt)) in enumerate(zip(want, pairs)):
        _assert_equal_to_twin(w, F[p], ver[oa[p]:oa[p + 1]], st[p], (p, flags))
        _assert_outcome(F[p], ver[oa[p]:oa[p + 1]], st[p], mt, (p, flags))
        assert (st[p, 2] == INVALID) == (p % 8 in (0, 1)), (p, st[p])     # empty, M < 7: no valid sample


# ---- edge cases -------------------------------------------------------------------------------------------------------
def test_edge_cases(handle, twin):
    cases = fc.edge_cases()
    calls = [ft.Call(ka, kb, mt, 17, 256, thr, flags) for _, ka, kb, mt, thr in cases for flags in (0, NO_REFINE)]
    want = iter(ft.run_calls(twin[0], calls, twin[1]))
    for name, ka, kb, mt, thr in cases:
        for flags in (0, NO_REFINE):
            (w,) = next(want)
            F, ver, st = handle.verify_fundamental(ka, kb, mt, 256, thr, 17, flags)
            _assert_equal_to_twin(w, F, ver, st, (name, flags))
            _assert_outcome(F, ver, st, mt, (name, flags))
            if name in ("collinear_a", "identical_rows", "seven_repeated"):   # every 7 x 9 system is rank deficient
                assert st[2] == INVALID, (name, st)
            if name in ("plane_noisy", "pure_rotation", "large_offset", "threshold_max"):
                assert st[2] != INVALID and st[0] >= 7, (name, st)
            if name == "threshold_max":                                      # every considered match is within it
                assert st[0] == len(mt) and st[1] == len(mt), st
    # one call holding them all (another slicing, seeds 17 - p + p): the same bits
    same_thr = [(n, ka, kb, mt) for n, ka, kb, mt, thr in cases if thr == THR]
    F, ver, st, oa = _device_batch(handle, [c[1:] for c in same_thr], 256, 17)
    singles = ft.run_calls(twin[0], [ft.Call(ka, kb, mt, 17 + p, 256, THR, 0) for p, (_, ka, kb, mt) in enumerate(same_thr)],
                           twin[1])
    for p, (w,) in enumerate(singles):
        _assert_equal_to_twin(w, F[p], ver[oa[p]:oa[p + 1]], st[p], ("batched", same_thr[p][0]))


def test_threshold_zero_is_refused(handle):
    ka, kb, mt, _ = two_view(50, 0.2, 3)
    for thr in (0.0, 1e-20, 1e20):
        with pytest.raises(RuntimeError, match="threshold"):
            handle.verify_fundamental(ka, kb, mt, 64, thr, 0, 0)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinates(handle, twin, bad):
    ka, kb, mt, _ = two_view(300, 0.4, 43)
    mt = mt.copy()
    mt[[10, 20, 30]] = -1
    (clean,) = ft.run_calls(twin[0], [ft.Call(ka, kb, mt, 4, 256, THR, 0)], twin[1])[0]
    assert clean["stats"][2] != INVALID
    # in rows that do not count: nothing changes, bit for bit
    ka2 = ka.copy()
    ka2[10, 0], ka2[20, 1] = bad, bad
    kb2 = np.concatenate([kb, np.full((1, 5), bad, np.float32)])      # an unmatched b row
    mt2 = mt.copy()
    mt2[30] = len(kb2) - 1 + 1000                                        # out of range: does not count either
    F, ver, st = handle.verify_fundamental(ka2, kb2, mt2, 256, THR, 4, 0)
    _assert_equal_to_twin(clean, F, ver, st, "non-considered")
    # in a considered row (a or b, x or y): no candidate for that pair, the other pairs of the call unaffected
    broken = fc.non_finite(bad)
    clean_pair = (broken[0][0].copy(), broken[0][1].copy(), broken[0][2])
    clean_pair[0][fc.BAD_ROW, 0] = 100.0
    assert np.isfinite(clean_pair[0]).all() and np.isfinite(clean_pair[1]).all()
    pairs = [clean_pair] + broken + [clean_pair]
    F, ver, st, oa = _device_batch(handle, pairs, 256, 4)
    want = ft.run_calls(twin[0], [ft.Call(*p, 4 + i, 256, THR, 0) for i, p in enumerate(pairs)], twin[1])
    for p, (w,) in enumerate(want):
        _assert_equal_to_twin(w, F[p], ver[oa[p]:oa[p + 1]], st[p], ("pair", p))
        _assert_outcome(F[p], ver[oa[p]:oa[p + 1]], st[p], pairs[p][2], ("pair", p))
        if 0 < p < len(pairs) - 1:
            assert st[p].tolist() == [0, 0, INVALID, 300] and (F[p] == 0).all() and (ver[oa[p]:oa[p + 1]] == -1).all(), p
        else:
            assert st[p, 2] != INVALID and st[p, 0] > 100, (p, st[p])
