"""The numpy restatement of lf_mkd_build_tracks_device (include/lf_mkd.h) and the inputs its tests share: a pool is image
offsets over `total` rows, an edge is two image ids of that ONE pool, the match array lives in the a side's edge layout, and an
entry is a link between two pool rows iff its value is a row of the edge's b image.  Tracks are the connected components of the
links; a track's label is its smallest row."""
import functools

import numpy as np

import q8_edges_cases as ecases
import q8_pairs_cases as pq

INT32_MAX = 2 ** 31 - 1
NO_IMAGE = ecases.NO_IMAGE
SENTINEL = -77
LEAD, TRAIL = 5, 7              # rows in front of the first and behind the last image that belong to no image


def links(image_offsets, total, edge_a, edge_b, layout_a, capacity, match):
    """(u, v) int64 arrays, the links: for edge e with (lo, len) its range of the layout against the capacity and (firstA, nA) /
    (firstB, nB) its two images' rows against the total, entry lo + r (r < min(nA, len)) links rows firstA + r and firstB + j,
    j = match[lo + r], iff 0 <= j < nB"""
    us, vs = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for e in range(len(edge_a)):
        lo, length = pq.pair_bounds(layout_a, capacity, e)
        first_a, na = ecases.image_bounds(image_offsets, total, edge_a[e])
        first_b, nb = ecases.image_bounds(image_offsets, total, edge_b[e])
        k = min(na, length)
        j = np.asarray(match[lo:lo + k], np.int64)
        r = np.flatnonzero((j >= 0) & (j < nb))
        us.append(first_a + r)
        vs.append(first_b + j[r])
    return np.concatenate(us), np.concatenate(vs)


def forest(total, into=None):
    """every row's root in the forest `into` holds (None: every row its own): an entry p at index r with p < 0 or p > r is read
    as r, so parents never exceed their index and jumping to the parent's parent ends"""
    r = np.arange(total, dtype=np.int64)
    if into is None:
        return r
    p = np.asarray(into, np.int64)[:total]
    p = np.where((p < 0) | (p > r), r, p)
    while True:
        pp = p[p]
        if np.array_equal(pp, p):
            return p
        p = pp


def components(root, u, v):
    """the smallest row of every row's connected component when the links (u, v) are added to the trees `root` describes
    (root[r] = the smallest row of r's tree): lower the larger of two linked roots to the smaller, flatten, repeat until every
    link's ends agree"""
    p = root.copy()
    while len(u):
        ru, rv = p[u], p[v]
        open_ = ru != rv
        if not open_.any():
            break
        u, v, ru, rv = u[open_], v[open_], ru[open_], rv[open_]
        np.minimum.at(p, np.maximum(ru, rv), np.minimum(ru, rv))
        while True:
            pp = p[p]
            if np.array_equal(pp, p):
                break
            p = pp
    return p


def statistics(image_offsets, total, track):
    """(len, dup): len[t] = rows with label t; dup[t] = the sum over images m of max(c(m, t) - 1, 0), c(m, t) = the rows of image
    m (its range against the total) with label t"""
    length = np.bincount(track, minlength=total).astype(np.uint32)
    dup = np.zeros(total, np.uint32)
    for m in range(len(image_offsets) - 1):
        first, n = ecases.image_bounds(image_offsets, total, m)
        t, c = np.unique(track[first:first + n], return_counts=True)
        dup[t] += (c - 1).astype(np.uint32)
    return length, dup


def build_tracks(image_offsets, total, edge_a, edge_b, layout_a, capacity, match, into=None):
    """(track int32 [total], len uint32 [total], dup uint32 [total]) of lf_mkd_build_tracks_device; `into`: the array the call
    accumulates onto (LF_MKD_TRACKS_ACCUMULATE), not changed"""
    u, v = links(image_offsets, total, edge_a, edge_b, layout_a, capacity, match)
    track = components(forest(total, into), u, v)
    length, dup = statistics(image_offsets, total, track)
    return track.astype(np.int32), length, dup


def closure(total, u, v):
    """the same labels by brute force: the reflexive, symmetric, transitive closure of the links as boolean matrix powers"""
    reach = np.eye(total, dtype=bool)
    reach[u, v] = reach[v, u] = True
    while True:
        more = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        if np.array_equal(more, reach):
            return np.argmax(reach, axis=1).astype(np.int32)           # the first True of a row: the smallest row it reaches
        reach = more


# --- cases ------------------------------------------------------------------------------------------------------------
class Case:
    """an edge list with its a side's layout (made from the ids unless `layout_from` gives others) and a match array built from
    (edge, row of its a image, value) triples; entries of no triple hold `fill`"""

    def __init__(self, pool, edges, triples, fill=-1, layout_from=None, capacity=None, extra=0):
        self.io, self.total = pool
        self.ea = np.array([e[0] for e in edges], np.uint32)
        self.eb = np.array([e[1] for e in edges], np.uint32)
        self.la = ecases.edge_layout(self.io, self.total, self.ea if layout_from is None else np.asarray(layout_from, np.uint32))
        self.size = int(self.la[-1]) + extra                              # the match array's entries
        self.cap = self.size if capacity is None else capacity
        self.match = np.full(self.size, fill, np.int32)
        for e, r, j in triples:
            assert 0 <= int(self.la[e]) + r < self.size, (e, r)
            self.match[int(self.la[e]) + r] = j

    def reference(self, into=None, match=None):
        return build_tracks(self.io, self.total, self.ea, self.eb, self.la, self.cap, self.match if match is None else match, into)

    def links(self):
        return links(self.io, self.total, self.ea, self.eb, self.la, self.cap, self.match)

    def permuted(self, order):
        """the same links with the edges in another order (the layout and the match array move with them)"""
        c = Case((self.io, self.total), [(self.ea[e], self.eb[e]) for e in order], [])
        assert self.size == int(self.la[-1]) == c.size and self.cap == self.size
        for k, e in enumerate(order):
            n = int(self.la[e + 1] - self.la[e])
            c.match[int(c.la[k]):int(c.la[k]) + n] = self.match[int(self.la[e]):int(self.la[e]) + n]
        return c


SMALL = 300                     # one-to-two-row images the chains run through


def pool_sizes(tile):
    """(sizes, names): images of 0, 1, 2, 63 .. 65, 255 .. 257 rows, a few of about 300, one of 2 x (the dup tile) + 1, SMALL
    images of one or two rows, and images on no edge between them ("gap")"""
    sizes, names = [], {}
    for name, n in (("e0", 0), ("e1", 1), ("e2", 2), ("gap0", 11), ("s63", 63), ("s64", 64), ("s65", 65), ("gap1", 3), ("s255", 255),
                    ("s256", 256), ("s257", 257), ("X", 300), ("Y", 310), ("gap2", 40), ("Z", 290), ("L", 2 * tile + 1)):
        names[name] = len(sizes)
        sizes.append(n)
    names["small"] = len(sizes)
    sizes += [1 + (k % 2) for k in range(SMALL)]
    names["W"] = len(sizes)
    sizes.append(305)
    return sizes, names


@functools.lru_cache(maxsize=None)
def pool(tile):
    """(image_offsets int64, total, names): the images of pool_sizes behind LEAD and in front of TRAIL rows of no image"""
    sizes, names = pool_sizes(tile)
    io = LEAD + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    io.setflags(write=False)
    return io, int(io[-1]) + TRAIL, names


def rows_of(p, m):
    return ecases.image_bounds(p[0], p[1], m)[1]


def chain(tile, descending):
    """row 0 of small image k linked to row 0 of small image k + 1, edge after edge: one track through all of them, the second
    rows on no link; descending: the edges from the far end, each from the higher image to the lower one"""
    io, total, names = pool(tile)
    s = names["small"]
    if descending:
        edges = [(s + k + 1, s + k) for k in range(SMALL - 2, -1, -1)]
    else:
        edges = [(s + k, s + k + 1) for k in range(SMALL - 1)]
    return Case((io, total), edges, [(i, 0, 0) for i in range(len(edges))])


def stars(tile, two):
    """every row of many images matched to ONE row of one image (row 5 of X); `two`: the images split between that hub and a
    second one, the single row of e1, and ONE link between the two hubs, on the last edge -- the last slot of the link grid"""
    io, total, names = pool(tile)
    leaves = [names[k] for k in ("s255", "s63", "s256", "Y", "s64", "Z", "s257", "L", "s65", "W")]
    hub_x, hub_1 = names["X"], names["e1"]
    edges, triples = [], []
    for i, m in enumerate(leaves):
        second = two and i % 2 == 1
        edges.append((m, hub_1 if second else hub_x))
        triples += [(i, r, 0 if second else 5) for r in range(rows_of((io, total), m))]
    if two:
        edges.append((hub_1, hub_x))
        triples.append((len(edges) - 1, 0, 5))
    return Case((io, total), edges, triples)


def cycles(tile):
    """consistent 3-cycles X -> Y -> Z -> X; cycles that come back to ANOTHER row of X (dup 1 there); a self edge linking two
    rows of X (dup 1); three rows of L, one in each of its dup tiles, on one row of W (dup 2)"""
    io, total, names = pool(tile)
    X, Y, Z, L, W = (names[k] for k in "XYZLW")
    edges = [(X, Y), (Y, Z), (Z, X), (X, X), (L, W)]
    triples = []
    for k in range(100):
        triples += [(0, k, k + 3), (1, k + 3, k + 1), (2, k + 1, k)]
    for k in range(100, 150):
        triples += [(0, k, k + 50), (1, k + 50, k + 10), (2, k + 10, k + 100)]
    triples += [(3, 270, 280)]
    triples += [(4, 3, 77), (4, tile + 44, 77), (4, 2 * tile, 77)]
    return Case((io, total), edges, triples)


def random_case(p, n_edges, seed, share=0.4, layout_from_b=False, extra=0):
    """random edges over the images of pool p -- ids at and beyond n_images, self edges and a repeated edge among them -- and a
    match array of which about `share` of the entries are links; the others hold -1, -7, nB, nB + 3 and INT32_MAX"""
    io, total = p[0], p[1]
    rng = np.random.default_rng(seed)
    n_images = len(io) - 1
    ea = rng.integers(0, n_images, n_edges)
    eb = rng.integers(0, n_images, n_edges)
    for k, bad in zip(rng.choice(n_edges, 4, replace=False), (n_images, NO_IMAGE, n_images + 7, 1 << 31)):
        (ea if k % 2 else eb)[k] = bad
    ea[-1], eb[-1] = ea[0], eb[0]                                          # a repeated edge
    ea[1] = eb[1]                                                          # a self edge
    edges = list(zip(ea.tolist(), eb.tolist()))
    c = Case((io, total), edges, [], layout_from=eb if layout_from_b else None, extra=extra)
    for e in range(n_edges):
        lo, length = pq.pair_bounds(c.la, c.size, e)
        nb = ecases.image_bounds(io, total, eb[e])[1]
        v = rng.integers(0, max(nb, 1), length)
        junk = rng.choice(np.array([-1, -7, nb, nb + 3, INT32_MAX], np.int64), length)
        c.match[lo:lo + length] = np.where(rng.random(length) < share, v, junk)
    return c


def odd_pool():
    """image offsets of 40 images with one inverted range, behind 9 rows of no image; the pool is told 6 rows fewer than the
    last offset says, so the last image's offset lies beyond the total (test_gpu_q8_edges.py's)"""
    rng = np.random.default_rng(77)
    sizes = rng.integers(0, 50, 40)
    sizes[39] = 20
    io = 9 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    io[17] = io[18] + 4                                        # image 17 inverted: empty; image 16 longer, over image 18's first rows
    return io, int(io[-1]) - 6
