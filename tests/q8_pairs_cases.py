"""Inputs and numpy restatements for the batched int8 matcher (lf_mkd_match_q8_pairs_device): the per-pair decision built
from tests/q8_cases.py, the workgroup-to-pair slot map at a block size R, and the ragged batch of quantised pairs -- with
decoy rows around every pair -- that the CPU and GPU tests share."""
import functools

import numpy as np

import match_pairs_cases as pcases
import q8_cases as qcases

INT32_MIN = qcases.INT32_MIN
RATIO = qcases.RATIO
SENTINEL = -7
LEAD, TRAIL = (5, 19), (7, 3)
WIDEN = 3                       # rows on either side of a pair's b rows that the decoy check lets in


def pair_bounds(offsets, n_total, p):
    """(first row, rows) of pair p: an offset beyond the total is read as the total, an inverted pair is empty"""
    o0, o1 = min(int(offsets[p]), n_total), min(int(offsets[p + 1]), n_total)
    return o0, max(o1 - o0, 0)


def match_one(x, y, ratio=RATIO):
    """lf_mkd_match_q8_device on one pair's rows, with the too-few rule: fewer than two candidates give -1 / INT32_MIN"""
    if len(y) < 2 or len(x) == 0:
        return (np.full(len(x), -1, np.int32), np.full(len(x), INT32_MIN, np.int32), np.full(len(x), INT32_MIN, np.int32))
    return qcases.match_q8(x, y, ratio)


def match_pairs(qa, oa, qb, ob, ratio=RATIO, fill=SENTINEL):
    """(match_ab [Na], match_ba [Nb], best [Na], second [Na]) of lf_mkd_match_q8_pairs_device without the mutual filter: per
    pair q8_cases.match_q8 in both directions, match values local to the pair; rows outside every pair hold `fill`."""
    na_total, nb_total = len(qa), len(qb)
    ab, ba = np.full(na_total, fill, np.int32), np.full(nb_total, fill, np.int32)
    best, second = np.full(na_total, fill, np.int32), np.full(na_total, fill, np.int32)
    for p in range(len(oa) - 1):
        a0, na = pair_bounds(oa, na_total, p)
        b0, nb = pair_bounds(ob, nb_total, p)
        x, y = qa[a0:a0 + na], qb[b0:b0 + nb]
        ab[a0:a0 + na], best[a0:a0 + na], second[a0:a0 + na] = match_one(x, y, ratio)
        ba[b0:b0 + nb] = match_one(y, x, ratio)[0]
    return ab, ba, best, second


# --- the slot map at block size R: which workgroup serves which R rows of which pair ----------------------------------
def grid_slots(n_total, n_pairs, R):
    """workgroups one direction is launched with: sized from the total alone, the host never reads the offsets"""
    return n_total // R + n_pairs


def slot_start(offsets, n_total, p, R):
    return min(int(offsets[p]), n_total) // R + p


def slot_to_block(offsets, n_total, slot, R):
    """(pair, block of R rows) the workgroup in `slot` works on, or None if it is idle: the kernel's binary search for the
    last pair whose first slot is at or before `slot`"""
    lo, hi = 0, len(offsets) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if slot_start(offsets, n_total, mid, R) <= slot:
            lo = mid
        else:
            hi = mid
    if slot_start(offsets, n_total, lo, R) > slot:
        return None
    block = slot - slot_start(offsets, n_total, lo, R)
    return (lo, block) if block * R < pair_bounds(offsets, n_total, lo)[1] else None


# --- the ragged batch -------------------------------------------------------------------------------------------------
def edge_sizes(R):
    """(na, nb) where this kernel can go wrong: around a 32-row tile; around an LDS stage of 4 tiles and the double buffer
    (b of 1, 4, 4, 5, 8, 9, 9 tiles); around a block of R rows; two candidates"""
    return ([(31, 33), (32, 32), (33, 31)] +
            [(37, 30), (64, 127), (65, 128), (33, 129), (96, 255), (70, 257), (50, 288)] +
            [(R - 1, 40), (R, 40), (R + 1, 40), (2 * R + 1, 70)] + [(20, 2)])


def _interior(n, k):
    """a row of an n-row pair for decoy k, away from the pair's first and last WIDEN rows where there are that many"""
    return (WIDEN + 5 * k) % (n - 2 * WIDEN) + WIDEN if n > 2 * WIDEN else k % n


@functools.lru_cache(maxsize=None)
def ragged_q8_batch(R):
    """(qa, oa, qb, ob, sizes): the quantised pairs of match_pairs_cases.ragged_batch() -- the degenerate ones and the
    (300, 6000) pair among them -- then edge_sizes(R), back to back behind LEAD rows and in front of TRAIL rows.
    Decoys: the WIDEN rows in front of and behind every pair's b rows (rows of the neighbouring pairs, or lead / trail rows)
    are exact copies of a rows of that pair, and likewise on the a side with copies of the pair's b rows; all lead and trail
    rows are such copies.  A candidate leaking across a pair boundary then meets a row's own copy.  Arrays are read-only."""
    pairs = [(qcases.quantize(a), qcases.quantize(b)) for a, b, _ in pcases.ragged_batch()]
    pairs += [qcases.quantized_sets(na, nb, 5000 + k) for k, (na, nb) in enumerate(edge_sizes(R))]
    rng = np.random.default_rng(77)
    pad = lambda n: qcases.quantize(pcases.unit(rng.normal(size=(n, 128))))
    qa = np.concatenate([pad(LEAD[0])] + [p[0] for p in pairs] + [pad(TRAIL[0])])
    qb = np.concatenate([pad(LEAD[1])] + [p[1] for p in pairs] + [pad(TRAIL[1])])
    oa = LEAD[0] + np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ob = LEAD[1] + np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    sizes = [(len(p[0]), len(p[1])) for p in pairs]
    n = len(pairs)
    for x, ox, y, oy in ((qa, oa, qb, ob), (qb, ob, qa, oa)):       # b's decoys copy a rows, then a's copy b rows
        for p in range(n):
            nx = int(ox[p + 1] - ox[p])
            if nx == 0:
                continue
            before = range(0 if p == 0 else max(int(oy[p]) - WIDEN, 0), int(oy[p]))
            after = range(int(oy[p + 1]), len(y) if p == n - 1 else min(int(oy[p + 1]) + WIDEN, len(y)))
            for k, row in enumerate(list(before) + list(after)):
                y[row] = x[int(ox[p]) + _interior(nx, k)]
    for arr in (qa, qb, oa, ob):
        arr.setflags(write=False)
    return qa, oa, qb, ob, sizes


@functools.lru_cache(maxsize=None)
def ragged_reference(R):
    """match_pairs of the ragged batch at RATIO: computed once, shared, never changed"""
    qa, oa, qb, ob, _ = ragged_q8_batch(R)
    out = match_pairs(qa, oa, qb, ob)
    for arr in out:
        arr.setflags(write=False)
    return out


def decoys_bite(R, limit=1 << 20):
    """pairs (of those with at most `limit` similarities) whose a -> b result changes when the pair's b rows are widened by
    WIDEN rows on either side: were a kernel to let those rows in, these pairs would show it"""
    qa, oa, qb, ob, sizes = ragged_q8_batch(R)
    ab, _, best, second = ragged_reference(R)
    hit = []
    for p, (na, nb) in enumerate(sizes):
        if na == 0 or na * nb > limit:
            continue
        a0, b0 = int(oa[p]), int(ob[p])
        lo, hi = max(b0 - WIDEN, 0), min(b0 + nb + WIDEN, len(qb))
        m, s1, s2 = match_one(qa[a0:a0 + na], qb[lo:hi])
        m = np.where(m >= 0, m - (b0 - lo), -1)                      # back to indices local to the pair
        if not (np.array_equal(m, ab[a0:a0 + na]) and np.array_equal(s1, best[a0:a0 + na]) and np.array_equal(s2, second[a0:a0 + na])):
            hit.append(p)
    return hit
