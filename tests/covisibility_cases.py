"""The numpy restatement of lf_mkd_covisibility_device (include/lf_mkd.h), read literally, in two formulations -- the loop over
counted positions, and the incidence matrix B[t][i] = counted positions of track t with image i, C = B.T @ B with the diagonal
replaced by B's column sums (for tracks whose images do not decrease B is 0/1 after the de-duplication and the diagonal of
B.T @ B is those sums already) -- and the generator of the tables the CPU and GPU tests share."""
import numpy as np

ACCUMULATE = 1
PAD = 0xFFFFFFFF
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 128, 129)
IMAGES = (1, 2, 3, 64, 65, 200)


class Table:
    """a track table as lf_mkd_track_table_device leaves it: offsets uint64 [track_capacity + 1], images uint32 [obs_capacity],
    counts uint32 [4]"""

    def __init__(self, offsets, images, counts=None, track_capacity=None, obs_capacity=None):
        self.offsets = np.asarray(offsets, np.uint64)
        self.images = np.asarray(images, np.uint32)
        self.track_capacity = len(self.offsets) - 1 if track_capacity is None else track_capacity
        self.obs_capacity = len(self.images) if obs_capacity is None else obs_capacity
        assert len(self.offsets) >= self.track_capacity + 1 and len(self.images) >= self.obs_capacity
        self.counts = np.asarray([self.track_capacity, self.obs_capacity, 0, 0] if counts is None else counts, np.uint32)


def from_tracks(tracks, **kw):
    """the Table of a list of image lists"""
    lens = [len(t) for t in tracks]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    images = np.concatenate([np.asarray(t, np.uint64) for t in tracks] + [np.zeros(0, np.uint64)]).astype(np.uint32)
    return Table(offsets, images, **kw)


def counted_lists(tab, n_images):
    """per track t < T the images of its counted positions, in order"""
    T = min(int(tab.counts[0]), tab.track_capacity)
    O = min(int(tab.counts[1]), tab.obs_capacity)
    im = tab.images
    out = []
    for t in range(T):
        lo, hi = min(int(tab.offsets[t]), O), min(int(tab.offsets[t + 1]), O)
        out.append([int(im[k]) for k in range(lo, max(lo, hi)) if (k == lo or im[k] != im[k - 1]) and im[k] < n_images])
    return out


def pairs(tab, n_images, matrix=False):
    """the table as a dict {(i, j): count} of its non-zero entries (before the reduction mod 2^32 and the mask)"""
    lists = counted_lists(tab, n_images)
    C = {}
    if matrix:
        for D in lists:
            ids, cnt = np.unique(np.asarray(D, np.int64), return_counts=True)
            outer = np.outer(cnt, cnt)
            outer[np.diag_indices(len(ids))] = cnt
            for a, i in enumerate(ids.tolist()):
                for b, j in enumerate(ids.tolist()):
                    C[i, j] = C.get((i, j), 0) + int(outer[a, b])
        return C
    for D in lists:
        for p, i in enumerate(D):
            C[i, i] = C.get((i, i), 0) + 1
            for q, j in enumerate(D):
                if p != q and i != j:
                    C[i, j] = C.get((i, j), 0) + 1
    return C


def covisibility(tab, n_images, edges=None, into=None, matrix=False):
    """d_covis uint32 [n_images][n_images]; into: what the table held (LF_MKD_COVIS_ACCUMULATE); edges: (edge_a, edge_b)"""
    C = np.zeros((n_images, n_images), np.uint64) if into is None else np.asarray(into).astype(np.uint32).astype(np.uint64)
    if matrix:
        lists = counted_lists(tab, n_images)
        B = np.zeros((len(lists), n_images), np.uint64)
        for t, D in enumerate(lists):
            np.add.at(B[t], np.asarray(D, np.int64), 1)
        P = B.T @ B
        P[np.diag_indices(n_images)] = B.sum(0)
        C = C + P
    else:
        for (i, j), v in pairs(tab, n_images).items():
            C[i, j] += v
    C = (C & 0xFFFFFFFF).astype(np.uint32)
    if edges is not None:
        for a, b in zip(np.asarray(edges[0]).astype(np.uint32).tolist(), np.asarray(edges[1]).astype(np.uint32).tolist()):
            if a < n_images and b < n_images:
                C[a, b] = C[b, a] = 0
    return C


def split(tab, parts):
    """the Table cut into `parts` Tables of consecutive tracks over the same image array (a call per part, ACCUMULATE from the
    second on, must give the whole table's result)"""
    T = min(int(tab.counts[0]), tab.track_capacity)
    cuts = [T * p // parts for p in range(parts + 1)]
    return [Table(tab.offsets[a:b + 1].copy(), tab.images, counts=[b - a, tab.counts[1], 0, 0], obs_capacity=tab.obs_capacity)
            for a, b in zip(cuts[:-1], cuts[1:])]


def consistent(rng, n_images, lengths):
    return [np.sort(rng.choice(n_images, min(l, n_images), replace=False)) for l in lengths]


def duplicated(rng, n_images, lengths):
    """sorted with adjacent duplicates, as a table made without LF_MKD_TRACK_TABLE_CONSISTENT holds them"""
    return [np.sort(rng.integers(0, n_images, l)) for l in lengths]


def unsorted(rng, n_images, lengths):
    return [rng.integers(0, n_images, l) for l in lengths]


def outside(rng, n_images, lengths):
    """ids at n_images, n_images + 1, 2^31 and 0xFFFFFFFF among the images, at track starts and after an equal raw neighbour"""
    bad = np.array([n_images, n_images + 1, 1 << 31, PAD], np.uint64)
    out = []
    for t, l in enumerate(lengths):
        x = np.sort(rng.integers(0, n_images, l)).astype(np.uint64)
        if l:
            hit = rng.random(l) < 0.3
            x[hit] = bad[rng.integers(0, 4, int(hit.sum()))]
            x[0] = bad[t % 4] if t % 2 else x[0]
            if l > 2:
                x[2] = x[1]                                                      # an equal raw neighbour, in or out of range
        out.append(x)
    return out


KINDS = {"consistent": consistent, "duplicated": duplicated, "unsorted": unsorted, "outside": outside}


def lengths_for(n_images, rng, extra=40):
    """every length of LENGTHS, n_images itself, and a crowd of short tracks (several groups to a wave, several waves)"""
    return list(LENGTHS) + [n_images, n_images + 1] + rng.integers(0, 7, extra).tolist()


def cases():
    """(name, Table, n_images) over every kind, every n_images of IMAGES and the values either side of the plan's thresholds"""
    out = []
    rng = np.random.default_rng(20261020)
    for n in sorted(set(IMAGES) | {4, 5, 8, 9, 16, 17, 32, 33}):
        for kind, make in KINDS.items():
            out.append(("%s-%d" % (kind, n), from_tracks(make(rng, n, lengths_for(n, rng))), n))
    out.append(("by-hand", from_tracks([[0, 0, 1, 1, 1, 2], [2], [], [1, 2]]), 3))
    return out


def capacity_cases():
    """counts beyond the capacities, offsets beyond O, an inverted range between ordered neighbours"""
    rng = np.random.default_rng(7)
    base = from_tracks(consistent(rng, 9, [3, 4, 0, 5, 2, 9, 1, 6]))
    T, O = base.track_capacity, base.obs_capacity
    over_t = Table(base.offsets, base.images, counts=[T + 5, O, 0, 0], track_capacity=T - 2)
    over_o = Table(base.offsets, base.images, counts=[T, O + 100, 0, 0], obs_capacity=O - 4)
    cut = Table(base.offsets, base.images, counts=[T, O - 7, 0, 0])              # the last offsets lie beyond O
    beyond = base.offsets.copy()
    beyond[-1] = (1 << 40) + 5
    beyond[-2] = 1 << 33
    far = Table(beyond, base.images)
    inv = base.offsets.copy()
    inv[2] = inv[2] + 2                                                          # track 1 longer, [lo, hi) of track 2 inverted: empty
    inverted = Table(inv, base.images)
    return [("counts[0] > track_capacity", over_t, 9), ("counts[1] > obs_capacity", over_o, 9), ("offsets beyond O", cut, 9),
            ("huge offsets", far, 9), ("inverted range", inverted, 9)]
