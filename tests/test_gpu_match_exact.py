"""The screen matcher (match_screen + match_verify, LF_MKD_MATCH=screen) against its host twin, bit for bit.

include/lf_mkd.h promises that the screen form's best, second and match are, for every row the fallback scan does not
redo, those of an exhaustive scan with verify's own f32 dot product.  tests/cpp/match_twin.cpp is that scan, so the promise
is tested as an equality: match, and the bits of best and second, with no allowance for near-ties.  A candidate that the
screening margin, the record ring, the splits' shared floor, a tile or split seam or an exclusion mask loses changes a bit.
tests/test_gpu_match.py's tolerance compare stays what holds the three-term forms, and it holds the rows redone here:
their number is lf_mkd_match_overflowed(), asserted per case, and at most that many rows may differ from the twin in a bit.

The inputs are tests/match_cases.py's; tests/test_match_twin.py proves on the CPU that each reaches what it is meant to.
Measured on the MI355X (NOTEBOOK.md): rows redone 0 wherever 0 is asserted, 1 for the tight ladder of 65, 1 for the zero
query, 4 and 16400 for the crowded rows."""
import numpy as np
import pytest

import match_cases as mc
import match_twin as mt
from test_gpu_match import compare, descriptor_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def screen_form(monkeypatch):
    monkeypatch.setenv("LF_MKD_MATCH", "screen")
    monkeypatch.delenv("LF_MKD_MATCH_SPLITS", raising=False)
    monkeypatch.delenv("LF_MKD_MATCH_SHARE", raising=False)


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """scan(key, a, b, ratio, lo, hi): the twin's answer, computed once per key for the module"""
    tmp = tmp_path_factory.mktemp("match_twin")
    exe = mt.build(tmp)
    seen = {}

    def scan(key, a, b, ratio, lo=None, hi=None):
        if key not in seen:
            seen[key] = mt.scan(exe, tmp, a, b, ratio, lo, hi)
        return seen[key]
    return scan


class Got:
    def __init__(self, match, best, second, overflowed):
        self.match, self.best, self.second, self.overflowed = match, best, second, overflowed

    def bits(self):
        return self.match, self.best.view(np.int32), self.second.view(np.int32)


def device(lfp, torch, a, b, ratio, lo=None, hi=None, handle=None):
    h = handle or lfp.MkdHandle(max_features=64)
    na = len(a)
    d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d_lo = torch.from_numpy(lo.view(np.int32)).cuda() if lo is not None else None
    d_hi = torch.from_numpy(hi.view(np.int32)).cuda() if hi is not None else None
    d_m = torch.full((na,), -7, dtype=torch.int32, device="cuda")
    d_1, d_2 = torch.full((na,), np.nan, device="cuda"), torch.full((na,), np.nan, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    h.match_device(d_a.data_ptr(), na, d_b.data_ptr(), len(b), d_m.data_ptr(), ratio,
                   d_lo.data_ptr() if d_lo is not None else None, d_hi.data_ptr() if d_hi is not None else None,
                   d_1.data_ptr(), d_2.data_ptr(), s)
    torch.cuda.synchronize()
    return Got(d_m.cpu().numpy(), d_1.cpu().numpy(), d_2.cpu().numpy(), h.match_overflowed(s))


def differing(got, want):
    """rows whose (best, second) bits differ from the twin's"""
    return np.flatnonzero((got.best.view(np.int32) != want.best.view(np.int32)) |
                          (got.second.view(np.int32) != want.second.view(np.int32)))


def assert_exact(got, want, what):
    rows = np.union1d(differing(got, want), np.flatnonzero(got.match != want.match))
    detail = [(int(i), int(got.match[i]), int(want.match[i]), hex(got.best.view(np.uint32)[i]), hex(want.best.view(np.uint32)[i]),
               hex(got.second.view(np.uint32)[i]), hex(want.second.view(np.uint32)[i])) for i in rows[:8]]
    assert len(rows) == 0, (what, len(rows), "row, match got / twin, best bits got / twin, second bits got / twin", detail)


def assert_redone(got, want, ratio, what):
    """at most `overflowed` rows differ from the twin in a bit or in the decision, and those agree as the three-term forms must"""
    diff = np.union1d(differing(got, want), np.flatnonzero(got.match != want.match))
    print(f"{what}: rows redone {got.overflowed}, rows that differ from the twin {len(diff)}")
    assert len(diff) <= got.overflowed, (what, diff[:8], got.overflowed)
    compare(got.match, got.best, got.second, want.match, want.best, want.second, np.float32(ratio), what)


def run_case(lfp, torch, twin, monkeypatch, case, ratio=None, handle=None):
    a, b, lo, hi, what = case
    ratio = what["ratio"] if ratio is None else ratio
    if what["splits"] is not None:
        monkeypatch.setenv("LF_MKD_MATCH_SPLITS", str(what["splits"]))
    got = device(lfp, torch, a, b, ratio, lo, hi, handle)
    return got, twin((what["name"], ratio), a, b, ratio, lo, hi)


def _ranges(na, nb, seed):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, max(1, nb - 1), na).astype(np.uint32)
    hi = lo + rng.integers(0, min(nb, 40), na).astype(np.uint32)
    return lo, hi


@pytest.mark.parametrize("splits", [None, 1, 3])
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("na,nb", [(1, 2), (17, 33), (70, 1000), (1500, 3000)])
def test_random_rows(lfp, torch, twin, monkeypatch, na, nb, exclude, splits):
    a, b = descriptor_sets(na, nb, 5 * na + nb)
    lo, hi = _ranges(na, nb, na) if exclude else (None, None)
    if splits is not None:
        monkeypatch.setenv("LF_MKD_MATCH_SPLITS", str(splits))
    got = device(lfp, torch, a, b, 0.8, lo, hi)
    want = twin(("random", na, nb, exclude), a, b, 0.8, lo, hi)
    if na >= 1000:
        assert 0.1 < (want.match >= 0).mean() < 0.95
    assert got.overflowed == 0
    assert_exact(got, want, ("random", na, nb, exclude, splits))


def test_the_margin_keeps_a_best_the_screen_ranks_third(lfp, torch, twin, monkeypatch):
    """margin_inversion: the true best is 0.62 of the margin below the screen's second largest"""
    case = mc.margin_inversion()
    for splits in (4, None):
        case[4]["splits"] = splits
        got, want = run_case(lfp, torch, twin, monkeypatch, case)
        monkeypatch.delenv("LF_MKD_MATCH_SPLITS", raising=False)
        assert [int(want.match[q]) for q, _, _ in case[4]["planted"]] == [t for _, t, _ in case[4]["planted"]]
        assert got.overflowed == 0
        assert_exact(got, want, ("margin_inversion", splits))


def test_both_directions_under_the_screen(lfp, torch, twin):
    a, b, _, _, what = mc.margin_inversion()
    d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m_ab = torch.full((len(a),), -7, dtype=torch.int32, device="cuda")
    m_ba = torch.full((len(b),), -7, dtype=torch.int32, device="cuda")
    h = lfp.MkdHandle(max_features=64)
    s = torch.cuda.current_stream().cuda_stream
    h.match_both_device(d_a.data_ptr(), len(a), d_b.data_ptr(), len(b), m_ab.data_ptr(), m_ba.data_ptr(), 0.0, s)
    torch.cuda.synchronize()
    assert h.match_overflowed(s) == 0
    assert np.array_equal(m_ab.cpu().numpy(), twin((what["name"], 0.0), a, b, 0.0).match)
    assert np.array_equal(m_ba.cpu().numpy(), twin((what["name"], "reverse"), b, a, 0.0).match)


@pytest.mark.parametrize("stride", [1, 16, 64])
def test_a_floor_reaches_its_own_row_only(lfp, torch, twin, monkeypatch, stride):
    """floor_mixup: rows whose splits share a floor of 0.95 beside rows whose best is 0.10; every sharing period gives the
    twin's bits (and so each other's)"""
    case = mc.floor_mixup(stride)
    for share in (None, "2", "0"):
        if share is not None:
            monkeypatch.setenv("LF_MKD_MATCH_SHARE", share)
        got, want = run_case(lfp, torch, twin, monkeypatch, case)
        assert got.overflowed == 0
        assert_exact(got, want, ("floor_mixup", stride, share))
        raw, want0 = run_case(lfp, torch, twin, monkeypatch, case, ratio=0.0)
        assert_exact(raw, want0, ("floor_mixup, ratio 0", stride, share))


@pytest.mark.parametrize("k,tight,descending", [(64, True, False), (64, True, True), (65, True, False), (100, False, False)])
def test_the_record_ring(lfp, torch, twin, monkeypatch, k, tight, descending):
    """ring_ladder: 64 records fill a stream's ring and nothing is redone; the 65th within the margin costs one redone row;
    100 in steps of 2.5 margins wrap the ring and verify still decides"""
    case = mc.ring_ladder(k, tight, descending)
    got, want = run_case(lfp, torch, twin, monkeypatch, case)
    print(case[4]["name"], "rows redone", got.overflowed)
    assert got.overflowed == case[4]["overflowed"]
    assert want.match[case[4]["query"]] == case[4]["rows"][0 if descending else -1]
    if got.overflowed:
        assert_redone(got, want, case[4]["ratio"], case[4]["name"])
        assert differing(got, want).tolist() in ([], [case[4]["query"]])
    else:
        assert_exact(got, want, case[4]["name"])


@pytest.mark.parametrize("n_over", [4, 16400])
def test_redone_rows_keep_their_exclusion_ranges(lfp, torch, twin, monkeypatch, n_over):
    """crowded_with_exclusion: the fallback scan of a few rows (match_split_rows gathers lo and hi) and of every row"""
    case = mc.crowded_with_exclusion(n_over)
    got, want = run_case(lfp, torch, twin, monkeypatch, case)
    lo_n, hi_n = case[4]["overflowed"]
    assert lo_n <= got.overflowed <= hi_n, got.overflowed
    assert_redone(got, want, case[4]["ratio"], case[4]["name"])
    if n_over == 4:
        assert set(differing(got, want).tolist()) <= set(case[4]["crowded"].tolist())
        # what the exclusion is for: with ratio 0 a crowded row's answer lies outside its range
        raw, want0 = run_case(lfp, torch, twin, monkeypatch, case, ratio=0.0)
        assert_redone(raw, want0, 0.0, case[4]["name"] + ", ratio 0")
        rows = case[4]["crowded"]
        assert ((raw.match[rows] < case[2][rows]) | (raw.match[rows] >= case[3][rows])).all()


@pytest.mark.parametrize("ratio", [0.0, 0.8])
def test_signs_and_zeros(lfp, torch, twin, monkeypatch, ratio):
    case = mc.signs_and_zeros()
    got, want = run_case(lfp, torch, twin, monkeypatch, case, ratio=ratio)
    what = case[4]
    assert what["overflowed"][0] <= got.overflowed <= what["overflowed"][1], got.overflowed
    assert_redone(got, want, ratio, what["name"])
    assert differing(got, want).tolist() in ([], [what["zero_a"]])
    if ratio == 0.0:
        assert got.match[what["zero_a"]] == len(case[1]) - 1 and got.match[what["dup"][0]] == what["dup"][2]
        assert (got.best[what["negated"]] <= 0).all()


@pytest.mark.parametrize("scale_a,scale_b", mc.SCALES)
def test_rows_far_from_unit_norm(lfp, torch, twin, monkeypatch, scale_a, scale_b):
    case = mc.scaled(scale_a, scale_b)
    got, want = run_case(lfp, torch, twin, monkeypatch, case)
    assert got.overflowed == 0
    assert_exact(got, want, case[4]["name"])


def test_a_handle_carries_nothing_over(lfp, torch, twin, monkeypatch):
    """one handle: a case, a crowded call (records, floors and the redone-rows count all in use), the case again"""
    h = lfp.MkdHandle(max_features=64)
    case, crowd = mc.floor_mixup(1), mc.crowded_with_exclusion(4)
    monkeypatch.setenv("LF_MKD_MATCH_SHARE", "2")
    first, want = run_case(lfp, torch, twin, monkeypatch, case, handle=h)
    mid, want_mid = run_case(lfp, torch, twin, monkeypatch, crowd, handle=h)
    again, _ = run_case(lfp, torch, twin, monkeypatch, case, handle=h)
    assert first.overflowed == 0 and again.overflowed == 0 and mid.overflowed == 4
    assert_redone(mid, want_mid, crowd[4]["ratio"], "crowded, between the two")
    assert_exact(first, want, "first call")
    assert all(np.array_equal(x, y) for x, y in zip(first.bits(), again.bits()))
