"""CPU tests of tests/keypoint_list_cases.py, with the oracle alone: every premise the GPU tests of the keypoint lists rest on
(list lengths on both sides of the 8192 seam, runs of extrema without a keypoint aligned to blocks of 1024, frames whose
extremum counts pass 8192, 4096 and the batch's former shared cap, or are zero), and that the cases have teeth: a numpy model
of the batched call's former arithmetic -- one list of 2 * cap_f * n_frames rows for the batch, frame starts clamped to it --
gives another result than the contract on every shared-cap batch and the same on every long-segment batch, and a Part 1
expectation fails when one block's offset is dropped from it."""
import numpy as np
import pytest

import keypoint_list_cases as cases


@pytest.fixture(scope="module")
def orient_stack(oracle):
    return oracle.build_coarse_stack(cases.orient_frame())


@pytest.fixture(scope="module")
def long_rows(oracle):
    return {name: cases.oracle_extrema(oracle, img) for name, img in cases.long_frames().items()}


@pytest.fixture(scope="module")
def cap_rows(oracle):
    return {name: cases.oracle_extrema(oracle, img) for name, img in cases.cap_frames().items()}


def test_the_strip_holds_extrema_without_a_keypoint(oracle, orient_stack):
    """dead extrema are chosen by asking the oracle; the sample the builder's ranges were read from: x = 10, size 2.5 -> no
    keypoint, size 4 -> one"""
    probe = np.array([[10.0, 120.0, 2.5, 0.1], [10.0, 120.0, 4.0, 0.1]], np.float32)
    assert len(oracle.orient(orient_stack, probe[:1])) == 0 and len(oracle.orient(orient_stack, probe[1:])) == 1
    dead = cases.dead_extrema(oracle, orient_stack, 1500, 5)
    assert dead.shape == (1500, 4) and len(oracle.orient(orient_stack, dead)) == 0


@pytest.mark.parametrize("n", list(cases.ORIENT_LISTS))
def test_orientation_lists(oracle, orient_stack, n):
    assert sorted(cases.ORIENT_LISTS) == [8192, 8193, 9216, 20000]
    assert 8192 == cases.KERNEL_FORM and 8193 % cases.BLOCK == 1 and 9216 % cases.BLOCK == 0 and 20000 > 16 * cases.BLOCK
    ex = cases.orient_list(oracle, orient_stack, n)
    assert ex.shape == (n, 4) and len(np.unique(ex[:, 3])) == n
    kps = oracle.orient(orient_stack, ex)
    counts = cases.peaks_per_extremum(ex, kps)
    assert counts.sum() == len(kps) > n and counts.max() >= 3
    # the run of dead extrema: whole blocks whose counts sum to zero, at the head, in the middle, at the tail
    b0, nb = cases.ORIENT_LISTS[n]
    assert nb >= 1 and counts[b0 * cases.BLOCK:(b0 + nb) * cases.BLOCK].sum() == 0
    last_block = (n - 1) // cases.BLOCK
    assert {8192: b0 == 0, 8193: 0 < b0 < last_block, 9216: b0 + nb - 1 == last_block, 20000: 0 < b0 < last_block}[n]
    assert (counts == 0).sum() == nb * cases.BLOCK                      # everything else yields a keypoint
    # the cuts: one keypoint, inside an extremum's peaks, at a block's base, around the total
    cuts = cases.orient_cuts(counts)
    first = np.concatenate([[0], np.cumsum(counts)])
    total = len(kps)
    assert len(cuts) == 6 and cuts[0] == 1 and cuts[-3:] == [total - 1, total, total + 1]
    inside = [c for c in cuts[1:-3] if c not in first and counts[np.searchsorted(first, c, side="right") - 1] >= 3]
    assert inside, cuts                                                  # a cut that splits an extremum's peaks
    mid = n // cases.BLOCK // 2
    assert int(first[mid * cases.BLOCK]) in cuts and 0 < mid < last_block
    # teeth: an expectation with one block's offset dropped is told from the right one
    cases.check_keypoints(kps, kps)
    blocks = [b for b in range(last_block + 1) if first[b * cases.BLOCK] > 0 and counts[b * cases.BLOCK:(b + 1) * cases.BLOCK].sum()]
    assert len(blocks) >= last_block - nb                                # (all but the dead ones and those with nothing before them)
    for block in blocks:
        with pytest.raises(AssertionError):
            cases.check_keypoints(cases.drop_block_offset(kps, counts, block), kps)
    off = kps.copy()
    off[len(off) // 2, 3] = (off[len(off) // 2, 3] + 0.002) % 360
    with pytest.raises(AssertionError):
        cases.check_keypoints(off, kps)                                   # EVERY angle, not most of them


def test_interleaved_frames_list(oracle):
    ex, frame_of = cases.interleaved_extrema()
    assert len(ex) == 9000 > cases.KERNEL_FORM and set(frame_of) == {0, 1, 2}
    assert (np.diff(frame_of.astype(np.int64)) != 0).mean() > 0.5       # interleaved, not frame after frame
    stacks = [oracle.build_coarse_stack(img) for img in cases.interleaved_frames()]
    kps, frame_of_kp = cases.expected_interleaved(oracle, stacks, ex, frame_of)
    assert len(kps) == len(frame_of_kp) > len(ex)
    counts = cases.peaks_per_extremum(ex, kps)                           # by extremum, in index order
    assert np.array_equal(np.repeat(frame_of, counts), frame_of_kp)
    # the frames differ: orienting everything on frame 0 gives another list
    with pytest.raises(AssertionError):
        cases.check_keypoints(oracle.orient(stacks[0], ex), kps)


def test_the_single_frame_passes_8192(oracle):
    st, rows = cases.oracle_extrema(oracle, cases.detect_frame())
    assert cases.KERNEL_FORM < len(rows) < cases.DETECT_BLOBS == 16384
    total = len(oracle.orient(st, rows))
    requests = cases.detect_requests(rows, total)
    assert [r[0] for r in requests] == [0, 0, 10000, 9000]
    assert requests[0][2] > total > requests[1][2] > 0                   # a capacity above the total, one that cuts
    assert cases.KERNEL_FORM < 10000 < len(rows)                         # the selection cuts, and stays a long list
    top_n, min_size, _ = requests[3]
    left = int((rows[:, 2] >= np.float32(min_size)).sum())
    assert 1000 <= left <= 8191 < top_n                                  # n_dev < 8192 < n_host
    assert len(cases.select(oracle, rows, 16384, top_n, min_size)) == left
    k, fo, db, df, _ = cases.expected_frames(oracle, [st], [rows], 16384, 0, 0.0, requests[1][2])
    assert len(k) == requests[1][2] and df == total - requests[1][2] and db == 0


def test_long_segment_batches(oracle, long_rows):
    n = {name: len(rows) for name, (_, rows) in long_rows.items()}
    assert n["dense"] > cases.KERNEL_FORM and n["dense2"] > cases.KERNEL_FORM      # segments longer than 8192 (and a sweep step)
    assert 0 < n["sparse"] < cases.SWEEP and n["flat"] == 0
    assert max(n.values()) < cases.LONG_BLOBS
    assert [o.index("flat") for o in cases.LONG_ORDERS] == [0, 1, 3]               # empty segment in front, between, behind
    min_size = cases.pick_min_size(long_rows["dense"][1], 9000)
    for order in cases.LONG_ORDERS:
        stacks, rows = [long_rows[x][0] for x in order], [long_rows[x][1] for x in order]
        for top_n in cases.LONG_TOP_N:
            for ms in (0.0, min_size):
                want = cases.expected_frames(oracle, stacks, rows, cases.LONG_BLOBS, top_n, ms, 1 << 20)
                model = cases.model_frames(oracle, stacks, rows, cases.LONG_BLOBS, top_n, ms, 1 << 20)
                # these cases do not rest on the shares: the former arithmetic gives the same list and counters
                assert np.array_equal(want[0], model[0]) and np.array_equal(want[1], model[1]) and want[2:4] == model[2:4] == (0, 0)
                per = np.bincount(want[1], minlength=4)
                assert per[order.index("flat")] == 0 and per[order.index("sparse")] > 0
                if top_n:
                    picked = want[4][order.index("dense")]
                    assert len(picked) == (top_n if not ms else min(top_n, int((long_rows["dense"][1][:, 2] >= np.float32(ms)).sum())))
    # the builder-chosen min_size leaves a dense frame a segment's worth below 8192 and above top_n = 2000
    assert 2000 < int((long_rows["dense"][1][:, 2] >= np.float32(min_size)).sum()) < cases.KERNEL_FORM


def test_shared_cap_batches_tell_the_former_arithmetic_from_the_contract(oracle, cap_rows):
    cap_f = cases.CAP_BLOBS
    # the worked example: two frames of 4231 extrema, max_blobs = 256
    spans, dropped = cases.shared_cap_model([4231, 4231], 256)
    assert spans == [(0, 256), (0, 0)] and dropped == 7438 + 768 == 8206 != 2 * 3975
    n = {name: len(rows) for name, (_, rows) in cap_rows.items()}
    for name in ("dense", "dense2", "dense3"):
        assert n[name] > 2 * cap_f * 3                                   # alone beyond the whole batch's former list
    assert 100 < n["sparse"] <= cap_f and n["flat"] == 0
    for batch in cases.CAP_BATCHES:
        stacks, rows = [cap_rows[x][0] for x in batch], [cap_rows[x][1] for x in batch]
        for top_n in cases.CAP_TOP_N:
            want = cases.expected_frames(oracle, stacks, rows, cap_f, top_n, 0.0, 1 << 20)
            model = cases.model_frames(oracle, stacks, rows, cap_f, top_n, 0.0, 1 << 20)
            assert want[2] == sum(max(0, len(r) - cap_f) for r in rows)
            assert want[2] != model[2], (batch, top_n)                   # another dropped_blobs ...
            assert want[0].shape != model[0].shape or not np.array_equal(want[0], model[0]), (batch, top_n)   # ... another list
            per = np.bincount(want[1], minlength=len(batch))
            for f, name in enumerate(batch):                             # every frame keeps the head of its own list
                assert len(want[4][f]) == min(n[name], top_n or cap_f, cap_f)
                assert (per[f] > 0) == (n[name] > 0)
            if "sparse" in batch and not top_n:
                assert len(want[4][batch.index("sparse")]) == n["sparse"]   # all of its roughly 140


def test_small_frames_share_a_workgroup(oracle):
    assert 0 < cases.small_cubes() < cases.BLOCK // 4 and cases.BLOCK % cases.small_cubes() != 0     # frames begin inside workgroups
    assert cases.small_cubes() * cases.SMALL_FRAMES > 2 * cases.BLOCK                               # and more than one workgroup
    n = [len(cases.oracle_extrema(oracle, img)[1]) for img in cases.small_frames()]
    assert n[5] == 0 and all(5 < c < cases.SMALL_BLOBS for i, c in enumerate(n) if i != 5), n
