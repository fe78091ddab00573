"""Inputs and numpy restatements for edge-list matching over 8-bit descriptors (include/lf_mkd.h, "edge lists":
lf_mkd_edge_layout_device, lf_mkd_gather_edge_rows_device, lf_mkd_match_q8_edges_device): a pool is a row array plus image
offsets, an edge is two image ids, the edge layout of a side is the pair layout whose pair e has the rows of that side's image
of edge e.  The per-edge decision is tests/q8_pairs_cases.py's match_one; the shared pool has decoy images around selected
images, so that a candidate leaking past an image boundary changes a decision."""
import functools

import numpy as np

import match_pairs_cases as pcases
import q8_cases as qcases
import q8_pairs_cases as pq

INT32_MIN = qcases.INT32_MIN
RATIO = qcases.RATIO
SENTINEL = pq.SENTINEL
LEAD, TRAIL = 5, 7              # rows in front of the first and behind the last image that belong to no image
DECOY = 3                       # rows of a decoy image
NO_IMAGE = 0xFFFFFFFF


def image_bounds(image_offsets, n_total, m):
    """(first row, rows) of image m of a pool: pair_rows of its two offsets; an id at or beyond n_images names an empty image"""
    if not 0 <= int(m) < len(image_offsets) - 1:
        return 0, 0
    return pq.pair_bounds(image_offsets, n_total, int(m))


def edge_layout(image_offsets, n_total, edge_image):
    """lf_mkd_edge_layout_device, one sentence at a time: out[0] = 0, out[e + 1] = out[e] + rows(edge_image[e])"""
    out = [0]
    for m in edge_image:
        out.append(out[-1] + image_bounds(image_offsets, n_total, m)[1])
    return np.array(out, np.uint64)


def gather_edge_rows(src, image_offsets, n_total, edge_image, edge_offsets, capacity, dst):
    """lf_mkd_gather_edge_rows_device into `dst` (changed in place): dst row lo + r = src row first + r for r < min(n, len)"""
    for e, m in enumerate(edge_image):
        lo, length = pq.pair_bounds(edge_offsets, capacity, e)
        first, n = image_bounds(image_offsets, n_total, m)
        k = min(n, length)
        dst[lo:lo + k] = src[first:first + k]
    return dst


def match_edges(qa, offsets_a, qb, offsets_b, edge_a, edge_b, layout_a, cap_a, layout_b, cap_b, ratio=RATIO, fill=SENTINEL):
    """(match_ab [cap_a], match_ba [cap_b], best [cap_a], second [cap_a]) of lf_mkd_match_q8_edges_device without the mutual
    filter: per edge q8_pairs_cases.match_one on the two WHOLE images in both directions, written for the rows the layout's
    range (cut at the capacity) has room for; entries of no edge hold `fill`."""
    ab, ba = np.full(cap_a, fill, np.int32), np.full(cap_b, fill, np.int32)
    best, second = np.full(cap_a, fill, np.int32), np.full(cap_a, fill, np.int32)
    for e in range(len(edge_a)):
        a0, na = image_bounds(offsets_a, len(qa), edge_a[e])
        b0, nb = image_bounds(offsets_b, len(qb), edge_b[e])
        A, B = qa[a0:a0 + na], qb[b0:b0 + nb]
        lo, length = pq.pair_bounds(layout_a, cap_a, e)
        k = min(na, length)
        m, s1, s2 = pq.match_one(A, B, ratio)
        ab[lo:lo + k], best[lo:lo + k], second[lo:lo + k] = m[:k], s1[:k], s2[:k]
        lo, length = pq.pair_bounds(layout_b, cap_b, e)
        k = min(nb, length)
        ba[lo:lo + k] = pq.match_one(B, A, ratio)[0][:k]
    return ab, ba, best, second


def chain_edges(n_images):
    """frame t against frame t + 1"""
    t = np.arange(n_images - 1, dtype=np.uint32)
    return t, t + 1


# --- the shared pool --------------------------------------------------------------------------------------------------
def image_sizes(R):
    """around the 32-row tile, the 4-tile LDS stage and its double buffer, a block of R rows, and the refusal of fewer than two
    rows"""
    return [0, 1, 2, 31, 32, 33, 127, 128, 129, 257, 300, R - 1, R, R + 1, 2 * R + 1]


PARTNER = 10                    # position (in image_sizes) of the 300-row image the decoys copy rows of
DESIGNATED = (3, 7, 8, 13, 14)  # positions whose image gets a decoy image directly in front of it and one directly behind


def make_pool(sizes, seed, designated=(), partner=None):
    """(q, image_offsets, ids, decoys): images of `sizes` rows, every one a noisy view of one 500-point scene (so that matches
    survive the ratio test and the cross-check), behind LEAD rows and in front of TRAIL rows of no image.  Around every
    position in `designated` sit two DECOY-row images holding exact copies of rows of the image at position `partner`; the
    lead and trail rows are such copies as well.  ids[k] is the image id of position k, decoys [(id in front, id of the
    image, id behind)].  Planted ties: in the partner row 250 is a copy of row 10, and in every image of 129 rows or more row
    128 is a copy of row 0 -- the two sides of an LDS stage border."""
    rng = np.random.default_rng(seed)
    scene = pcases.unit(rng.normal(size=(500, 128)))
    view = lambda n: qcases.quantize(pcases.unit(scene[rng.integers(0, 500, n)] + 0.03 * rng.normal(size=(n, 128)))) \
        if n else np.zeros((0, 128), np.uint8)
    images = [view(n) for n in sizes]
    for im in images:
        if len(im) >= 129:
            im[128] = im[0]
    copies = lambda n, k: np.zeros((n, 128), np.uint8)
    if partner is not None:
        images[partner][250] = images[partner][10]
        P = images[partner]
        copies = lambda n, k: P[[(7 + 11 * (k + i)) % len(P) for i in range(n)]].copy()
    blocks, ids, decoys, count = [copies(LEAD, 0)], [], [], 0
    for k, im in enumerate(images):
        if k in designated:
            blocks += [copies(DECOY, 10 * k), im, copies(DECOY, 10 * k + 5)]
            ids.append(count + 1)
            decoys.append((count, count + 1, count + 2))
            count += 3
        else:
            blocks.append(im)
            ids.append(count)
            count += 1
    blocks.append(copies(TRAIL, 3))
    if partner is None:             # no decoys: the rows of no image are noise
        blocks[0], blocks[-1] = view(LEAD), view(TRAIL)
    q = np.ascontiguousarray(np.concatenate(blocks))
    starts = np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.int64)         # of every block; the images are blocks 1 .. -2
    image_offsets = np.ascontiguousarray(starts[1:])                                # ... and the last image ends where the trail starts
    assert image_offsets[0] == LEAD and image_offsets[-1] == len(q) - TRAIL and len(image_offsets) == count + 1
    return q, image_offsets, ids, decoys


def all_edges(n_images):
    """every ordered pair of images, self edges included; one repeated edge; one edge with id n_images and one with NO_IMAGE"""
    i, j = np.divmod(np.arange(n_images * n_images, dtype=np.int64), n_images)
    ea = np.concatenate([i, [i[n_images + 2]], [n_images, 1]]).astype(np.uint32)
    eb = np.concatenate([j, [j[n_images + 2]], [2, NO_IMAGE]]).astype(np.uint32)
    return ea, eb


@functools.lru_cache(maxsize=None)
def shared_pool(R):
    """(q, image_offsets, ids, decoys, edge_a, edge_b): the pool of image_sizes(R) with its decoys, and all_edges over every
    image of it (the decoy images are images too).  Arrays are read-only."""
    q, image_offsets, ids, decoys = make_pool(image_sizes(R), 9100, DESIGNATED, PARTNER)
    ea, eb = all_edges(len(image_offsets) - 1)
    for arr in (q, image_offsets, ea, eb):
        arr.setflags(write=False)
    return q, image_offsets, tuple(ids), tuple(decoys), ea, eb


@functools.lru_cache(maxsize=None)
def shared_reference(R):
    """(layout_a, layout_b, match_edges(...)) of the shared pool against itself at RATIO with capacities = the layouts' totals:
    computed once, shared, never changed"""
    q, io, _, _, ea, eb = shared_pool(R)
    la, lb = edge_layout(io, len(q), ea), edge_layout(io, len(q), eb)
    out = match_edges(q, io, q, io, ea, eb, la, int(la[-1]), lb, int(lb[-1]))
    for arr in (la, lb) + out:
        arr.setflags(write=False)
    return la, lb, out


def decoys_bite(R):
    """per designated image B: the edges (A, B) whose a -> b result changes when B's rows are widened by its two decoy images --
    were a kernel to let the rows next to an image in, these edges would show it"""
    q, io, ids, decoys, ea, eb = shared_pool(R)
    hits = {}
    for front, b, behind in decoys:
        assert io[front + 1] == io[b] and io[b + 1] == io[behind] and io[behind + 1] - io[behind] == DECOY
        b0, nb = image_bounds(io, len(q), b)
        lo, hi = int(io[front]), int(io[behind + 1])
        hits[b] = []
        for a in range(len(io) - 1):
            a0, na = image_bounds(io, len(q), a)
            if na == 0 or nb < 2:
                continue
            want = pq.match_one(q[a0:a0 + na], q[b0:b0 + nb])
            m, s1, s2 = pq.match_one(q[a0:a0 + na], q[lo:hi])
            m = np.where(m >= 0, m - (b0 - lo), -1)
            if not (np.array_equal(m, want[0]) and np.array_equal(s1, want[1]) and np.array_equal(s2, want[2])):
                hits[b].append(a)
    return hits
