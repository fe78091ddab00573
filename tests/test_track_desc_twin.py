"""The host twin of the track descriptor call (tests/cpp/track_desc_twin.cpp: csrc/mkd_track_desc_math.h under g++, built as
a stand-alone program with -fsanitize=address,undefined) against the numpy restatement of the contract
(tests/track_desc_cases.py): every byte and word equal, on every case the GPU tests use."""
import numpy as np
import pytest

import track_desc_cases as cases


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("track_desc_twin")
    exe = cases.build(tmp)
    return lambda calls: cases.run_calls(exe, tmp, calls)


def test_the_twin_equals_the_restatement_on_every_case(twin):
    named = cases.cpu_cases()
    got = twin([c for _, c in named])
    for (name, c), (desc, stats) in zip(named, got):
        want_desc, want_stats = cases.restate(c)
        assert np.array_equal(desc, want_desc), (name, np.argwhere(desc != want_desc)[:5].tolist())
        if c["stats"]:
            assert np.array_equal(stats, want_stats), (name, np.argwhere(stats != want_stats)[:5].tolist())
        else:
            assert stats is None


def test_what_the_cases_hold(twin):
    """the cases reach what they are meant to reach: the cap, the clamp, the cancelling pair, the filters"""
    c = cases.lengths()
    (desc, stats), = twin([c])
    lens = np.diff(c["track_offsets"].astype(np.int64))[:int(c["counts"][0])]
    long = int(np.argmax(lens))
    assert lens[long] == cases.LONG and stats[long, 0] == cases.MAX_OBS
    n = len(cases.LENGTHS) + 1
    assert stats[n:n + 7, 0].tolist() == [0, 1, 2, 3, 3, 0, 20]
    assert (desc[n] == 128).all() and stats[n, 1] == cases.INT32_MIN                      # the empty track
    assert desc[n + 1, 37] == 255 and (np.delete(desc[n + 1], 37) == 128).all()           # the spike: the clamp at 127
    assert stats[n + 1, 1] == 127 * 127
    assert (desc[n + 2] == 128).all() and stats[n + 2].tolist() == [2, cases.INT32_MIN]   # the pair that cancels
    assert (desc[n + 5] == 128).all()                                                     # rows that are no row
    T = int(c["counts"][0])
    assert (desc[T:] == 128).all() and (stats[T:] == [0, cases.INT32_MIN]).all() and len(desc) == T + 5
    # unit rows again: the quantised row's norm is the scale, up to the rounding of 128 values
    real = (stats[:T, 1] != cases.INT32_MIN) & (desc[:T] != 255).all(1) & (desc[:T] != 1).all(1)
    assert real.sum() >= len(cases.LENGTHS)
    norm = np.linalg.norm(desc[:T][real].astype(np.float64) - 128, axis=1)
    assert np.abs(norm - 256).max() < 128 ** 0.5
    by_state = [twin([cases.states(m)])[0][1] for m in (0, 1, 2)]
    assert by_state[0][5, 0] == 9 and by_state[1][5].tolist() == by_state[2][5].tolist() == [0, cases.INT32_MIN]
    assert (by_state[0][:11, 0] >= by_state[1][:11, 0]).all() and (by_state[1][:11, 0] >= by_state[2][:11, 0]).all()
    assert by_state[2][:11, 0].sum() < by_state[0][:11, 0].sum()
    (desc0, st0), = twin([cases.point_filter(0.0)])
    zero = [bool((desc0[i] == 128).all()) for i in range(11)]
    assert zero == [True, True, True, True, False, True, False, True, False, False, True]
    assert (st0[:11, 0] == cases.LENGTHS).all()                                           # C is counted for them all the same
    t0, t1, t2 = twin(cases.ties())
    assert t0[0][0, 3] == 128 + 2 and t0[0][0, 90] == 128 + 6 and t1[0][1, 0] == 128 + 2 and t1[0][1, 127] == 128 - 2
    assert t2[0][0, 3] == 128 + 1 and t2[0][1, 0] == 128 + 2                              # 17.5 / 13 = 1.35, 10.5 / 5 = 2.1


def test_a_permutation_of_the_tracks_permutes_the_rows(twin):
    q, tracks = cases.length_tracks(long=0)
    order = np.random.default_rng(9).permutation(len(tracks))
    (a, sa), (b, sb) = twin([cases.call(q, tracks), cases.permuted(tracks, q, order)])
    assert np.array_equal(a[order], b) and np.array_equal(sa[order], sb)
