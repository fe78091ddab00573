"""Inputs and numpy restatements for the batched pair matcher (lf_mkd_match_pairs_device): the ragged batch the CPU and
GPU tests share, the mutual (cross-check) rule, the workgroup-to-pair slot map, and the oracle comparison's rule."""
import numpy as np


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def descriptor_sets(na, nb, seed, noise=0.25):
    """b random unit vectors; a = noisy copies of some b rows plus unrelated ones: a mix of accepted and rejected."""
    rng = np.random.default_rng(seed)
    b = unit(rng.normal(size=(nb, 128)))
    src = rng.integers(0, nb, na)
    a = b[src] + noise * rng.normal(size=(na, 128)) / np.sqrt(128) * rng.uniform(0, 4, (na, 1))
    a[rng.random(na) < 0.2] = rng.normal(size=(128,))
    return unit(a), b


# (na, nb) of pair p, seed 1000 + p: both directions of every one fit the single-pair call's one-launch form
SIZED = [(2000, 2000), (31, 33), (513, 1025), (3000, 700), (1, 2), (1900, 2100), (500, 4000), (16, 16), (17, 130),
         (2048, 4096), (250, 250), (1000, 1200)]
BEYOND = (300, 6000)            # seed 1012: nb beyond the one-launch form's 4096
DEGENERATE = [(0, 50), (40, 0), (17, 1), (0, 0)]   # a side the single-pair call refuses
RATIO = np.float32(0.8)


def small_fits(na, nb):
    """match_small_fits of csrc/mkd_match.hip: where lf_mkd_match_device takes its one-launch form by default"""
    return na > 0 and 2 <= nb <= 4096 and na * nb <= 8388608 and (nb >= 128 or na <= 4096)


def ragged_batch():
    """[(a, b, kind)] with kind "sized" / "beyond" / "degenerate": the twelve sized pairs with the degenerate ones
    interleaved, then the pair beyond the one-launch form."""
    out = []
    deg = list(DEGENERATE)
    for p, (na, nb) in enumerate(SIZED):
        out.append(descriptor_sets(na, nb, 1000 + p) + ("sized",))
        if p % 3 == 1 and deg:
            da, db = deg.pop(0)
            rng = np.random.default_rng(2000 + p)
            out.append((unit(rng.normal(size=(da, 128))), unit(rng.normal(size=(db, 128))), "degenerate"))
    assert not deg
    out.append(descriptor_sets(BEYOND[0], BEYOND[1], 1012) + ("beyond",))
    return out


def concatenate(pairs, lead=(0, 0), trail=(0, 0), seed=77):
    """(a rows, offsets_a, b rows, offsets_b) of the pairs back to back, with `lead` / `trail` rows of neither pair in
    front of and behind them (the offsets then start above 0 and end below the totals)."""
    rng = np.random.default_rng(seed)
    pad = lambda n: unit(rng.normal(size=(n, 128))) if n else np.zeros((0, 128), np.float32)
    a = np.concatenate([pad(lead[0])] + [p[0] for p in pairs] + [pad(trail[0])])
    b = np.concatenate([pad(lead[1])] + [p[1] for p in pairs] + [pad(trail[1])])
    oa = lead[0] + np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ob = lead[1] + np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    return np.ascontiguousarray(a), oa, np.ascontiguousarray(b), ob


# --- the mutual rule (LF_MKD_MATCH_MUTUAL) ---------------------------------------------------------------------------
def mutual(ab, ba, oa, ob):
    """match_ab[i] = j survives iff match_ba[j] == i, match_ba[j] = i survives iff match_ab[i] == j, both read from the
    unfiltered arrays (indices local to the pair); everything else becomes -1.  Rows outside the pairs are left alone."""
    ab, ba = np.asarray(ab), np.asarray(ba)
    out_ab, out_ba = ab.copy(), ba.copy()
    for p in range(len(oa) - 1):
        x, y = ab[oa[p]:oa[p + 1]], ba[ob[p]:ob[p + 1]]
        i = np.arange(len(x))
        ok = (x >= 0) & (x < len(y))
        keep = ok.copy()
        keep[ok] = y[x[ok]] == i[ok]
        out_ab[oa[p]:oa[p + 1]] = np.where(keep, x, -1)
        j = np.arange(len(y))
        ok = (y >= 0) & (y < len(x))
        keep = ok.copy()
        keep[ok] = x[y[ok]] == j[ok]
        out_ba[ob[p]:ob[p + 1]] = np.where(keep, y, -1)
    return out_ab, out_ba


# --- the slot map: which workgroup serves which 16 rows of which pair -------------------------------------------------
def grid_slots(n_total, n_pairs):
    """workgroups one direction is launched with: sized from the total alone, the host never reads the offsets"""
    return n_total // 16 + n_pairs


def slot_start(offsets, n_total, p):
    return min(int(offsets[p]), n_total) // 16 + p


def slot_to_block(offsets, n_total, slot):
    """(pair, block of 16 rows) the workgroup in `slot` works on, or None if it is idle: the kernel's binary search for
    the last pair whose first slot is at or before `slot`."""
    n_pairs = len(offsets) - 1
    lo, hi = 0, n_pairs
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if slot_start(offsets, n_total, mid) <= slot:
            lo = mid
        else:
            hi = mid
    if slot_start(offsets, n_total, lo) > slot:
        return None
    o0, o1 = min(int(offsets[lo]), n_total), min(int(offsets[lo + 1]), n_total)
    block = slot - slot_start(offsets, n_total, lo)
    return (lo, block) if block * 16 < max(o1 - o0, 0) else None


# --- the oracle comparison (compare() of tests/test_gpu_match.py, restated) ------------------------------------------
def compare(got, got_s1, got_s2, want, s1, s2, ratio, what):
    if got_s1 is not None:
        assert np.abs(got_s1 - s1).max(initial=0.0) < 2e-6 and np.abs(got_s2 - s2).max(initial=0.0) < 2e-6, what
    diff = np.flatnonzero(got != want)
    # a differing decision must be a near-tie: best vs second (index choice) or best*ratio vs second (acceptance)
    for i in diff:
        near_accept = abs(s1[i] * ratio - s2[i]) < 2e-6
        near_index = abs(s1[i] - s2[i]) < 2e-6
        assert near_accept or near_index, (what, i, got[i], want[i], s1[i], s2[i])
    assert len(diff) <= max(2, len(want) // 500), (what, len(diff))
    return len(diff)


def match_f64(a, b, ratio=0.8):
    """match_features in float64 (the decision margins of the inputs are checked with it): (match, best, second)"""
    s = a.astype(np.float64) @ b.astype(np.float64).T
    order = np.argsort(s, axis=1, kind="stable")
    idx = order[:, -1]
    rows = np.arange(len(a))
    best, second = s[rows, idx], s[rows, order[:, -2]]
    return np.where(best * ratio > second, idx, -1).astype(np.int32), best, second
