"""The numpy restatement of lf_mkd_link_table_device (include/lf_mkd.h), in two independent formulations: a literal loop over
the edges on tracks_cases.links' rule, and a vectorised one (the edge ids repeated over the layout, one mask, flatnonzero,
cumsum) that the large GPU cases can afford.  An edge's links are the entries of its range of the a side's layout whose value
is a row of its b image; an edge is selected iff it has min_links of them, kept iff the selected edges up to and including it
fit link_capacity; the table lists the kept edges' links in edge order, then row order."""
import numpy as np

import q8_edges_cases as ecases
import q8_pairs_cases as pq
import tracks_cases as tcases

U32_MAX = 2 ** 32 - 1
INT32_MIN = -2 ** 31


class Table:
    """offsets uint64 [n_edges + 1]; link_a, link_b int32 [O]; link_edge uint32 [O]; edge_links uint32 [n_edges]; match_kept:
    `into` after the call (None without); counts [4] python ints"""

    def __init__(self, offsets, link_a, link_b, link_edge, edge_links, match_kept, counts):
        self.offsets, self.link_a, self.link_b, self.link_edge = offsets, link_a, link_b, link_edge
        self.edge_links, self.match_kept, self.counts = edge_links, match_kept, counts

    def same(self, other):
        both = self.match_kept is not None and other.match_kept is not None
        return (self.counts == other.counts and all(
            a.dtype == b.dtype and np.array_equal(a, b)
            for a, b in ((self.offsets, other.offsets), (self.link_a, other.link_a), (self.link_b, other.link_b),
                         (self.link_edge, other.link_edge), (self.edge_links, other.edge_links)))
                and (self.match_kept is None) == (other.match_kept is None)
                and (not both or np.array_equal(self.match_kept, other.match_kept)))

    def edge(self, e):
        """the (a, b) lists of edge e"""
        lo, hi = int(self.offsets[e]), int(self.offsets[e + 1])
        return self.link_a[lo:hi], self.link_b[lo:hi]


def _finish(n_edges, L, min_links, link_capacity):
    """(selected, kept, W [n_edges + 1], O) from the per-edge link counts, one edge at a time"""
    selected, kept, W = np.zeros(n_edges, bool), np.zeros(n_edges, bool), [0]
    for e in range(n_edges):
        selected[e] = int(L[e]) >= min_links
        W.append(W[-1] + (int(L[e]) if selected[e] else 0))
        kept[e] = selected[e] and W[-1] <= link_capacity
    return selected, kept, W, sum(int(L[e]) for e in range(n_edges) if kept[e])


def link_table(image_offsets, total, edge_a, edge_b, layout_a, capacity, match, min_links=0, link_capacity=None, local=False,
               into=None):
    """the literal loop.  link_capacity None: capacity, which always suffices.  into: what d_match_kept holds before the call
    (a copy is written and returned; `match` itself for the in-place form)"""
    n_edges = len(edge_a)
    link_capacity = capacity if link_capacity is None else link_capacity
    per_edge = []
    for e in range(n_edges):
        lo, length = pq.pair_bounds(layout_a, capacity, e)
        first_a, na = ecases.image_bounds(image_offsets, total, edge_a[e])
        first_b, nb = ecases.image_bounds(image_offsets, total, edge_b[e])
        k = min(na, length)
        j = np.asarray(match[lo:lo + k], np.int64)
        r = np.flatnonzero((j >= 0) & (j < nb))
        per_edge.append((lo, k, first_a, first_b, r, j[r]))
    L = np.array([len(p[4]) for p in per_edge], np.uint32).reshape(n_edges)
    selected, kept, W, O = _finish(n_edges, L, min_links, link_capacity)
    a, b, ed = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    out = None if into is None else np.array(into, np.int32)
    for e, (lo, k, first_a, first_b, r, j) in enumerate(per_edge):
        if out is not None:
            keep = np.full(k, -1, np.int32)
            if kept[e]:
                keep[r] = j
            out[lo:lo + k] = keep
        if kept[e]:
            a.append(r if local else first_a + r)
            b.append(j if local else first_b + j)
            ed.append(np.full(len(r), e, np.int64))
    offsets = np.minimum(np.array(W, np.uint64), np.uint64(O))
    counts = [int(kept.sum()), O, int(selected.sum()), min(W[-1], U32_MAX)]
    return Table(offsets, np.concatenate(a).astype(np.int32), np.concatenate(b).astype(np.int32),
                 np.concatenate(ed).astype(np.uint32), L, out, counts)


def _bounds(offsets, total, ids):
    """ecases.image_bounds for an array of ids: (first, rows) int64 arrays"""
    offsets = np.asarray(offsets, np.int64)
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(offsets) - 1)
    m = np.where(ok, ids, 0)
    o0, o1 = np.minimum(offsets[m], total), np.minimum(offsets[m + 1], total)
    return np.where(ok, o0, 0), np.where(ok, np.maximum(o1 - o0, 0), 0)


def link_table_vectorised(image_offsets, total, edge_a, edge_b, layout_a, capacity, match, min_links=0, link_capacity=None,
                          local=False, into=None):
    """the same table without a loop over the edges"""
    n_edges = len(edge_a)
    link_capacity = capacity if link_capacity is None else link_capacity
    la = np.minimum(np.asarray(layout_a).astype(np.int64), capacity)
    lo, length = la[:-1], np.maximum(la[1:] - la[:-1], 0)
    first_a, na = _bounds(image_offsets, total, edge_a)
    first_b, nb = _bounds(image_offsets, total, edge_b)
    k = np.minimum(na, length)
    edge_of = np.repeat(np.arange(n_edges, dtype=np.int64), k)
    r = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(np.cumsum(k) - k, k)
    at = lo[edge_of] + r
    j = np.asarray(match, np.int32)[at].astype(np.int64)
    mask = (j >= 0) & (j < nb[edge_of])
    L = np.bincount(edge_of[mask], minlength=n_edges).astype(np.int64)
    selected = L >= min_links
    W = np.concatenate([[0], np.cumsum(np.where(selected, L, 0))])
    kept = selected & (W[1:] <= link_capacity)
    O = int(L[kept].sum())
    idx = np.flatnonzero(mask & kept[edge_of])
    e, rr, jj = edge_of[idx], r[idx], j[idx]
    out = None
    if into is not None:
        out = np.array(into, np.int32)
        out[at] = np.where(mask & kept[edge_of], j, -1).astype(np.int32)
    counts = [int(kept.sum()), O, int(selected.sum()), min(int(W[-1]), U32_MAX)]
    return Table(np.minimum(W, O).astype(np.uint64), (rr if local else first_a[e] + rr).astype(np.int32),
                 (jj if local else first_b[e] + jj).astype(np.int32), e.astype(np.uint32), L.astype(np.uint32), out, counts)


def of_case(case, vectorised=False, **kw):
    f = link_table_vectorised if vectorised else link_table
    return f(case.io, case.total, case.ea, case.eb, case.la, case.cap, case.match, **kw)


# --- cases ----------------------------------------------------------------------------------------------------------------
def shared_cases(tile):
    """tracks_cases' shared cases: chains, stars, cycles, random, the odd pool, a layout from other ids, capacities below the
    layout"""
    p = tcases.pool(tile)[:2]
    odd = tcases.odd_pool()
    below = tcases.random_case(p, 30, 8)
    below.cap = below.size - 41
    return [("chain", tcases.chain(tile, False)), ("chain, descending", tcases.chain(tile, True)),
            ("star", tcases.stars(tile, False)), ("two stars", tcases.stars(tile, True)), ("cycles", tcases.cycles(tile)),
            ("random", tcases.random_case(p, 40, 5)), ("random, extra", tcases.random_case(p, 25, 6, extra=19)),
            ("odd pool", tcases.random_case(odd, 30, 3)), ("layout from b", tcases.random_case(p, 30, 7, layout_from_b=True)),
            ("capacity below", below)]


def tiny_edges(n_edges, seed):
    """n_edges edges over a pool of 0- to 2-row images, about half of the entries links: many edges, few entries, so that the
    slots are the edges and the scan over them is what is exercised"""
    rng = np.random.default_rng(seed)
    n_images = 301
    sizes = rng.integers(0, 3, n_images)
    io = 3 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(io[-1]) + 2
    ea = rng.integers(0, n_images, n_edges).astype(np.uint32)
    eb = rng.integers(0, n_images, n_edges).astype(np.uint32)
    la = np.concatenate([[0], np.cumsum(sizes[ea])]).astype(np.uint64)
    size = int(la[-1])
    match = np.where(rng.random(size) < 0.5, rng.integers(0, 2, size), -1).astype(np.int32)

    class Tiny:
        pass
    c = Tiny()
    c.io, c.total, c.ea, c.eb, c.la, c.size, c.cap, c.match = io, total, ea, eb, la, size, size, match
    return c
