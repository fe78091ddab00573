"""CPU tests of track tables (include/lf_mkd.h: lf_mkd_track_table_plan, lf_mkd_track_table_device,
lf_mkd_gather_track_rows_device): the symbols exist and refuse bad arguments without a device, the plan reports what the
header says, and the two formulations of the numpy restatement the GPU tests compare against (tests/track_table_cases.py)
agree -- on the shared track cases, on small random pools and on every capacity cut."""
import ctypes
import os
import re

import numpy as np

import tracks_cases as tcases
import track_table_cases as cases
from conftest import ROOT

import local_features_python as lfp

BIG = (1 << 31) - 1
TILE = lfp.TRACKS_DUP_TILE


def test_the_symbols_are_exported():
    L = lfp.load_library()
    header = open(os.path.join(ROOT, "include", "lf_mkd.h")).read()
    for name, arity in (("lf_mkd_track_table_plan", 6), ("lf_mkd_track_table_device", 17), ("lf_mkd_gather_track_rows_device", 9)):
        assert name in lfp.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
        proto = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert len(proto.split(",")) == arity
    assert hasattr(lfp.LocalFeatures, "track_table") and hasattr(lfp.LocalFeatures, "gather_track_rows")
    assert hasattr(lfp.MkdHandle, "track_table_device") and hasattr(lfp.MkdHandle, "gather_track_rows_device")
    assert int(re.search(r"#define LF_MKD_TRACK_TABLE_CONSISTENT \((\d+)u\)", header).group(1)) == lfp.TRACK_TABLE_CONSISTENT == 1


def _refused(L, rc, who, what, kw):
    assert rc == -1, (who, kw)
    msg = L.lf_mkd_last_error(None)
    assert msg.startswith(who + b": ") and what in msg, (who, kw, msg)


def test_the_table_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)
    C = lfp.TRACK_TABLE_CONSISTENT

    def call(io=p, n_images=3, total=64, track=p, length=p, dup=p, min_len=2, flags=C, t_cap=32, o_cap=64, offsets=p, rows=p,
             images=p, row_track=p, counts=p):
        return L.lf_mkd_track_table_device(None, io, n_images, total, track, length, dup, min_len, flags, t_cap, o_cap, offsets, rows,
                                           images, row_track, counts, None)

    for kw, what in [({}, b"null handle"), ({"flags": 0}, b"null handle"), ({"flags": 0, "dup": None}, b"null handle"),
                     ({"images": None}, b"null handle"), ({"images": None, "io": None}, b"null handle"),
                     ({"row_track": None}, b"null handle"), ({"total": 0}, b"null handle"), ({"t_cap": 0, "o_cap": 0}, b"null handle"),
                     ({"o_cap": 0, "rows": None}, b"null handle"), ({"min_len": 1}, b"null handle"),
                     ({"total": BIG, "t_cap": BIG, "o_cap": BIG}, b"null handle"),
                     ({"offsets": None}, b"null pointer"), ({"counts": None}, b"null pointer"),
                     ({"track": None}, b"null track or length array"), ({"length": None}, b"null track or length array"),
                     ({"rows": None}, b"null d_obs_row"), ({"io": None}, b"d_obs_image needs d_image_offsets"),
                     ({"min_len": 0}, b"min_len"), ({"dup": None}, b"LF_MKD_TRACK_TABLE_CONSISTENT needs d_track_dup"),
                     ({"flags": 2}, b"unknown flag bits"), ({"flags": 0x80000001}, b"unknown flag bits"),
                     ({"io": odd8}, b"8-byte aligned"), ({"offsets": odd8}, b"8-byte aligned"),
                     ({"track": odd4}, b"4-byte aligned"), ({"length": odd4}, b"4-byte aligned"), ({"dup": odd4}, b"4-byte aligned"),
                     ({"rows": odd4}, b"4-byte aligned"), ({"images": odd4}, b"4-byte aligned"), ({"row_track": odd4}, b"4-byte aligned"),
                     ({"counts": odd4}, b"4-byte aligned"),
                     ({"total": BIG + 1}, b"2^31 - 1"), ({"t_cap": BIG + 1}, b"2^31 - 1"), ({"o_cap": BIG + 1}, b"2^31 - 1"),
                     ({"total": 1 << 40}, b"2^31 - 1")]:
        _refused(L, call(**kw), b"track_table_device", what, kw)


def test_the_gather_call_refuses_bad_arguments_without_a_device():
    L = lfp.load_library()
    p, odd4 = ctypes.c_void_p(64), ctypes.c_void_p(66)

    def call(src=p, row_bytes=20, total=64, rows=p, counts=p, o_cap=64, dst=p):
        return L.lf_mkd_gather_track_rows_device(None, src, row_bytes, total, rows, counts, o_cap, dst, None)

    for kw, what in [({}, b"null handle"), ({"row_bytes": 4}, b"null handle"), ({"row_bytes": 512}, b"null handle"),
                     ({"row_bytes": 128}, b"null handle"), ({"o_cap": 0, "rows": None, "dst": None}, b"null handle"),
                     ({"total": 0, "src": None}, b"null handle"), ({"total": BIG, "o_cap": BIG}, b"null handle"),
                     ({"src": None}, b"null pointer"), ({"rows": None}, b"null pointer"), ({"counts": None}, b"null pointer"),
                     ({"dst": None}, b"null pointer"),
                     ({"row_bytes": 0}, b"row_bytes"), ({"row_bytes": 2}, b"row_bytes"), ({"row_bytes": 22}, b"row_bytes"),
                     ({"row_bytes": 516}, b"row_bytes"), ({"row_bytes": 0xFFFFFFFC}, b"row_bytes"),
                     ({"src": odd4}, b"4-byte aligned"), ({"dst": odd4}, b"4-byte aligned"), ({"rows": odd4}, b"4-byte aligned"),
                     ({"counts": odd4}, b"4-byte aligned"),
                     ({"total": BIG + 1}, b"2^31 - 1"), ({"o_cap": BIG + 1}, b"2^31 - 1")]:
        _refused(L, call(**kw), b"gather_track_rows_device", what, kw)


def test_the_plan():
    L = lfp.load_library()
    assert L.lf_mkd_track_table_plan(64, 0, None, None, None, None) == -1
    assert L.lf_mkd_last_error(None).startswith(b"track_table_plan: ") and b"min_len" in L.lf_mkd_last_error(None)
    assert L.lf_mkd_track_table_plan(BIG + 1, 1, None, None, None, None) == -1
    assert L.lf_mkd_last_error(None).startswith(b"track_table_plan: ") and b"2^31 - 1" in L.lf_mkd_last_error(None)
    assert L.lf_mkd_track_table_plan(BIG, 1, None, None, None, None) == 0      # every output is optional
    assert lfp.track_table_plan(0, 1)[3] == 0 and lfp.track_table_plan(0, 5)[:2] == (0, 0)
    block = lfp.track_table_plan(1, 1)[2]
    assert 64 <= block <= 8192 and block % 64 == 0
    widths = set()
    last = (0, 0, 0)
    for n in [1, 2, 3, 63, 64, 65, 255, 256, 257, 3197, 4095, 4096, 4097, 65535, 65536, 3 * 2 ** 16 + 5, 2 ** 20, 2 ** 24 + 1, BIG]:
        for min_len in (1, 2, 3, 7):
            bits, passes, rows, scratch = lfp.track_table_plan(n, min_len)
            assert bits == (n // min_len).bit_length() and rows == block, (n, min_len)
            assert scratch > 0
            if bits:
                # the passes cover the bits at one digit width, whatever it is: 1 .. 16 bits
                ws = {w for w in range(1, 17) if passes == -(-bits // w)}
                assert ws, (n, min_len, bits, passes)
                widths.add(frozenset(ws))
            else:
                assert passes == 0
        bits, passes, rows, scratch = lfp.track_table_plan(n, 1)
        assert bits >= last[0] and passes >= last[1] and scratch >= last[2], n   # monotone in N
        last = (bits, passes, scratch)
    common = frozenset.intersection(*widths)
    assert common, "no single digit width explains every plan"
    assert lfp.track_table_plan(3 * 2 ** 16 + 5, 1)[1] > lfp.track_table_plan(3197, 1)[1]    # what the GPU tests' large pool is for


def shared_cases():
    p = tcases.pool(TILE)[:2]
    return [("chain", tcases.chain(TILE, False)), ("star", tcases.stars(TILE, False)), ("two stars", tcases.stars(TILE, True)),
            ("cycles", tcases.cycles(TILE)), ("random", tcases.random_case(p, 40, 5))]


def test_the_two_formulations_agree_on_the_shared_cases():
    """and the figures the GPU tests name hold"""
    io = tcases.pool(TILE)[0]
    figures = {}
    for name, case in shared_cases():
        track, length, dup = case.reference()
        for min_len in (1, 2, 3):
            for consistent in (False, True):
                a = cases.track_table(track, length, dup, min_len, consistent, image_offsets=io)
                b = cases.track_table_by_groups(track, length, dup, min_len, consistent, image_offsets=io)
                assert a.same(b), (name, min_len, consistent)
                figures[name, min_len, consistent] = (a.counts[0], a.counts[1], int(np.diff(a.offsets[:a.counts[0] + 1].astype(np.int64)).max(initial=0)))
                assert a.counts[0] == a.counts[2] and a.counts[1] == a.counts[3]     # the default capacities cut nothing
    assert case.total == 3197
    assert figures["star", 2, False] == (1, 2379, 2379)                      # one track: every key equal
    assert figures["star", 1, True][:2] == (818, 818)                        # the star is inconsistent: what is left are single rows
    assert figures["cycles", 2, True][:2] == (100, 300) and figures["cycles", 2, False][:2] == (152, 506)
    assert figures["random", 2, False] == (64, 322, 61)
    # rows of no image, in front of and behind the images, are observations of their own tracks at min_len 1
    track, length, dup = shared_cases()[0][1].reference()
    a = cases.track_table(track, length, dup, 1, False, image_offsets=io)
    assert (a.obs_image[:tcases.LEAD] == cases.NO_IMAGE).all() and (a.obs_image[-tcases.TRAIL:] == cases.NO_IMAGE).all()
    assert (a.obs_image != cases.NO_IMAGE).sum() == case.total - tcases.LEAD - tcases.TRAIL


def test_the_two_formulations_agree_on_small_random_pools_and_every_capacity_cut():
    cut_somewhere = 0
    for seed in range(24):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(0, 61))
        track, length, dup = cases.random_groups(n, max(n // int(rng.integers(1, 5)), 1), seed)
        dup[rng.random(n) < 0.2] = 1
        dup[length == 0] = 0
        if n > 4:
            track[rng.integers(0, n, 2)] = (-3, n + 2)                        # members of nothing (their labels' lengths now overstate)
            roots = track == np.arange(n)
            length = np.where(roots, np.bincount(track[(track >= 0) & (track < n)], minlength=n), 0).astype(np.uint32)
        sizes = rng.integers(0, 9, 6)
        io = 2 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        for min_len in (1, 2, 3):
            for consistent in (False, True):
                full = cases.track_table(track, length, dup, min_len, consistent, image_offsets=io)
                assert full.same(cases.track_table_by_groups(track, length, dup, min_len, consistent, image_offsets=io)), (seed, min_len)
                s, w = full.counts[2], full.counts[3]
                assert full.counts[:2] == [s, w] and s <= n // min_len and w <= n
                for t_cap in range(0, s + 2):
                    a = cases.track_table(track, length, dup, min_len, consistent, t_cap, n)
                    assert a.same(cases.track_table_by_groups(track, length, dup, min_len, consistent, t_cap, n)), (seed, min_len, t_cap)
                    assert a.counts == [min(t_cap, s), int(full.offsets[min(t_cap, s)]), s, w] and len(a.offsets) == t_cap + 1
                for o_cap in range(0, w + 2):
                    a = cases.track_table(track, length, dup, min_len, consistent, None, o_cap)
                    assert a.same(cases.track_table_by_groups(track, length, dup, min_len, consistent, None, o_cap)), (seed, min_len, o_cap)
                    t = a.counts[0]
                    assert a.counts[1] <= o_cap and a.counts[2:] == [s, w] and (a.offsets[t:] == a.counts[1]).all()
                    assert t == s or int(full.offsets[t + 1]) > o_cap             # the next track did not fit: never cut in the middle
                    assert np.array_equal(a.obs_row, full.obs_row[:a.counts[1]])
                    cut_somewhere += t < s and a.counts[1] < o_cap
    assert cut_somewhere > 100                                                # capacities that end inside a track


def test_relabelling_keeps_the_tracks():
    track, length, dup = shared_cases()[3][1].reference()
    n = len(track)
    perm = np.random.default_rng(9).permutation(n)
    t2, l2, d2 = cases.relabelled(track, length, dup, perm)
    a, b = cases.track_table(track, length, dup, 2, True), cases.track_table(t2, l2, d2, 2, True)
    assert a.counts == b.counts
    inv = np.argsort(perm)
    sets = lambda tab, back: sorted(tuple(sorted(back[tab.obs_row[int(tab.offsets[i]):int(tab.offsets[i + 1])]].tolist())) for i in range(tab.counts[0]))
    assert sets(a, np.arange(n)) == sets(b, inv)


def test_the_gather_restatement():
    src = np.arange(40, dtype=np.float32).reshape(8, 5)
    dst = np.full((6, 5), -1, np.float32)
    cases.gather_track_rows(src, np.array([7, 0, -1, 8, 3, 2], np.int32), 5, dst)
    assert np.array_equal(dst[:2], src[[7, 0]]) and (dst[2:4] == 0).all() and np.array_equal(dst[4], src[3]) and (dst[5] == -1).all()
