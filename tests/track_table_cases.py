"""The numpy restatement of lf_mkd_track_table_device and lf_mkd_gather_track_rows_device (include/lf_mkd.h), read literally:
a mask, np.flatnonzero, a cumsum and a stable argsort of every row's table index -- and a second, independent formulation that
groups the rows label by label in a Python dict.  N = len(track); track / length / dup are what lf_mkd_build_tracks_device
leaves."""
import numpy as np

import q8_edges_cases as ecases

NO_IMAGE = 0xFFFFFFFF
U32_MAX = 2 ** 32 - 1


class Table:
    """counts [4] (Python ints), offsets uint64 [track_capacity + 1], obs_row int32 [O], obs_image uint32 [O] or None, row_track
    int32 [N]"""

    def __init__(self, counts, offsets, obs_row, obs_image, row_track):
        self.counts, self.offsets, self.obs_row, self.obs_image, self.row_track = counts, offsets, obs_row, obs_image, row_track

    def same(self, other):
        return (self.counts == other.counts and np.array_equal(self.offsets, other.offsets) and np.array_equal(self.obs_row, other.obs_row)
                and (self.obs_image is None) == (other.obs_image is None)
                and (self.obs_image is None or np.array_equal(self.obs_image, other.obs_image))
                and np.array_equal(self.row_track, other.row_track))


def image_of(image_offsets, total, rows):
    """per row the image whose range, read against the total as lf_mkd_build_tracks_device reads it, holds it, or NO_IMAGE
    (offsets that do not decrease: at most one image holds a row)"""
    rows = np.asarray(rows, np.int64)
    out = np.full(len(rows), NO_IMAGE, np.uint32)
    for m in range(len(image_offsets) - 1):
        first, n = ecases.image_bounds(image_offsets, total, m)
        out[(rows >= first) & (rows < first + n)] = m
    return out


def selected_labels(track, length, dup, min_len, consistent):
    """the selected roots in ascending order: 0 <= t < N, track[t] == t, length[t] >= min_len and, if consistent, dup[t] == 0"""
    n = len(track)
    mask = (np.asarray(track, np.int64) == np.arange(n)) & (np.asarray(length).astype(np.uint32) >= min_len)
    if consistent:
        mask &= np.asarray(dup).astype(np.uint32) == 0
    return np.flatnonzero(mask)


def counts_of(track, length, dup, min_len, consistent, track_capacity, obs_capacity):
    """(counts, labels, W): d_counts, the selected labels and W [S + 1] (Python ints) -- specified whatever the arrays hold"""
    labels = selected_labels(track, length, dup, min_len, consistent)
    lens = [int(x) for x in np.asarray(length).astype(np.uint32)[labels]]
    w = [0]
    for v in lens:
        w.append(w[-1] + v)
    kept = [i < track_capacity and w[i + 1] <= obs_capacity for i in range(len(labels))]
    t = sum(kept)
    assert kept == [True] * t + [False] * (len(labels) - t)                  # W does not decrease: a prefix
    return [t, w[t], len(labels), min(w[-1], U32_MAX)], labels, w


def track_table(track, length, dup, min_len=2, consistent=True, track_capacity=None, obs_capacity=None, image_offsets=None):
    """the Table of lf_mkd_track_table_device for arrays as lf_mkd_build_tracks_device leaves them"""
    track = np.asarray(track, np.int64)
    n = len(track)
    track_capacity = n // min_len if track_capacity is None else track_capacity
    obs_capacity = n if obs_capacity is None else obs_capacity
    counts, labels, w = counts_of(track, length, dup, min_len, consistent, track_capacity, obs_capacity)
    t, o = counts[0], counts[1]
    offsets = np.full(track_capacity + 1, o, np.uint64)
    offsets[:t + 1] = np.array(w[:t + 1], np.uint64)
    index = np.full(n, -1, np.int64)                                         # label -> table index
    index[labels[:t]] = np.arange(t)
    valid = (track >= 0) & (track < n)
    row_track = np.where(valid, index[np.where(valid, track, 0)], -1)
    rows = np.flatnonzero(row_track >= 0)
    obs_row = rows[np.argsort(row_track[rows], kind="stable")]
    assert len(obs_row) == o, "a track's member count must equal its length (arrays not from lf_mkd_build_tracks_device?)"
    obs_image = image_of(image_offsets, n, obs_row) if image_offsets is not None else None
    return Table(counts, offsets, obs_row.astype(np.int32), obs_image, row_track.astype(np.int32))


def track_table_by_groups(track, length, dup, min_len=2, consistent=True, track_capacity=None, obs_capacity=None, image_offsets=None):
    """the same Table, label by label: the rows grouped in a dict, the tracks walked in the order of their labels"""
    n = len(track)
    track_capacity = n // min_len if track_capacity is None else track_capacity
    obs_capacity = n if obs_capacity is None else obs_capacity
    members = {}
    for r in range(n):
        t = int(track[r])
        if 0 <= t < n:
            members.setdefault(t, []).append(r)
    offsets, obs_row, row_track = [0], [], [-1] * n
    selected = wanted = 0
    cut = False
    for t in sorted(members):
        if int(track[t]) != t or int(np.uint32(length[t])) < min_len or (consistent and int(np.uint32(dup[t])) != 0):
            continue
        selected += 1
        wanted += int(np.uint32(length[t]))
        if cut or len(offsets) - 1 >= track_capacity or offsets[-1] + int(np.uint32(length[t])) > obs_capacity:
            cut = True                                                       # a track is never cut in the middle, nor skipped
            continue
        for r in members[t]:
            row_track[r] = len(offsets) - 1
        obs_row += members[t]
        offsets.append(offsets[-1] + int(np.uint32(length[t])))
    t_kept, o = len(offsets) - 1, offsets[-1]
    assert o == len(obs_row)
    offsets += [o] * (track_capacity - t_kept)
    obs_image = None
    if image_offsets is not None:
        owner = {}                                                           # row -> the image whose range holds it
        for m in range(len(image_offsets) - 1):
            for r in range(min(int(image_offsets[m]), n), min(int(image_offsets[m + 1]), n)):
                assert r not in owner                                        # (offsets that do not decrease: one image a row)
                owner[r] = m
        obs_image = np.array([owner.get(r, NO_IMAGE) for r in obs_row], np.uint32)
    return Table([t_kept, o, selected, min(wanted, U32_MAX)], np.array(offsets, np.uint64), np.array(obs_row, np.int32), obs_image,
                 np.array(row_track, np.int32))


def gather_track_rows(src, obs_row, count, dst):
    """lf_mkd_gather_track_rows_device into `dst` (changed in place): dst row k = src row obs_row[k] for k < count; an index
    outside the pool gives a zero row"""
    for k in range(count):
        r = int(obs_row[k])
        dst[k] = src[r] if 0 <= r < len(src) else 0
    return dst


# --- inputs with no edge list -------------------------------------------------------------------------------------------
def from_groups(group):
    """(track, length, dup) for rows whose group ids are given: the label is the group's smallest row, dup 0"""
    group = np.asarray(group, np.int64)
    n = len(group)
    first = np.full(int(group.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(first, group, np.arange(n))
    track = first[group]
    length = np.bincount(track, minlength=n).astype(np.uint32)
    return track.astype(np.int32), length, np.zeros(n, np.uint32)


def random_groups(n, n_groups, seed):
    return from_groups(np.random.default_rng(seed).integers(0, max(n_groups, 1), n))


def relabelled(track, length, dup, perm):
    """the same tracks with the rows renamed: row r becomes row perm[r].  Labels are smallest rows again, the statistics move to
    the new labels."""
    n = len(track)
    perm = np.asarray(perm, np.int64)
    group = np.empty(n, np.int64)
    group[perm] = np.asarray(track, np.int64)                                # new row perm[r] is in the group old label names
    t2, l2, _ = from_groups(group)
    d2 = np.zeros(n, np.uint32)
    old_label_of_new = np.empty(n, np.int64)
    old_label_of_new[perm] = np.asarray(track, np.int64)
    roots = np.flatnonzero(t2 == np.arange(n))
    d2[roots] = np.asarray(dup).astype(np.uint32)[old_label_of_new[roots]]
    return t2, l2, d2
