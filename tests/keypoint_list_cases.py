"""Frames, extremum lists and the host-side expectation for the list machinery between the extremum scan and the describe
launch: the ordered compactions, the per-frame top-n filter and the device-side counts (mkd_orient.hip, mkd_detect.hip,
lf_mkd.cpp), at the lengths where they change form.  tests/test_keypoint_list_cases.py checks the premises stated here with the
oracle alone; tests/test_gpu_keypoint_lists.py holds the library to the expectation.

THE EXPECTATION FEEDS EVERY STAGE THE LIBRARY'S OWN BITS.  The oracle's extrema and the library's agree to 1e-3 px, and the
orientation reads its window at int(x), int(y): an end-to-end comparison has to forgive the few positions that land in the other
texel.  Staged, nothing needs forgiving: the extrema are compared with oracle.scan_extrema at the detector's tolerances (counts
exact), the selection is oracle.topk_filter of the LIBRARY's rows (indices equal), the orientation is oracle.orient of the
LIBRARY's selected rows (x, y, size, response bit-equal, every angle within 1e-3 degrees, circular).

    expected_frames   the contract of lf_mkd_detect_frames_device (include/lf_mkd.h), and with one frame that of lf_mkd_detect:
                      per frame the first cap_f rows, filtered if top_n is set, oriented; the frames concatenated; max_out cuts
                      the whole list; dropped_blobs sums the rows beyond cap_f over the frames
    shared_cap_model  the arithmetic the batched call had before each frame got a share of its own: ONE list of
                      2 * cap_f * n_frames rows for the batch, the frames' starts clamped to it -- what the cases must tell
                      from the contract (the shared-cap batches) or must not depend on (the long-segment batches)

Tied contrasts in the segmented filter cannot be injected through any entry point: the contrasts of a frame's extrema are what
the detector computes (a dense frame here holds two or three equal pairs, wherever they fall), so a tie AT the cut of the
segmented form is not constructed here; test_topk_filter_vs_oracle constructs them for the single-list forms.
"""
import numpy as np

KERNEL_FORM = 8192          # launch_orient: n <= 8192 one launch, beyond it three; topk_filter's single-list form ends there too
BLOCK = 1024                # extrema per workgroup of the compactions
SWEEP = 4096                # extrema per sweep step of the segmented topk_filter


# ---- frames ---------------------------------------------------------------------------------------------------------------
def noise_frame(w, h, seed, passes, strip=0):
    """uniform noise, `passes` five-point averages, normalised to [0, 1]; columns [0, strip) flat (the mean)"""
    rng = np.random.default_rng(seed)
    img = rng.random((h, w))
    for _ in range(passes):
        img = (img + np.roll(img, 1, 0) + np.roll(img, -1, 0) + np.roll(img, 1, 1) + np.roll(img, -1, 1)) / 5
    img = (img - img.min()) / (img.max() - img.min())
    if strip:
        img[:, :strip] = img.mean()
    return np.ascontiguousarray(img, np.float32)


def flat_frame(w, h):
    return np.full((h, w), 0.4, np.float32)


def dense(w, h, seed):      # thousands of extrema
    return noise_frame(w, h, seed, 2)


def sparse(w, h, seed):     # the noise itself: few extrema survive the contrast threshold and the edge test
    return noise_frame(w, h, seed, 0)


def oracle_extrema(oracle, img, n_scales=4):
    """(a-trous stack, every extremum of the frame in the detector's order)"""
    st = oracle.build_coarse_stack(img, n_scales)
    ex, total = oracle.scan_extrema(oracle.dog(st))
    assert total == len(ex)
    return st, ex


# ---- Part 1: orientation lists ----------------------------------------------------------------------------------------------
ORIENT_W, ORIENT_H, STRIP = 320, 240, 48


def orient_frame():
    """test_gpu_orientation.py's smooth_image with a flat strip on the left"""
    return noise_frame(ORIENT_W, ORIENT_H, 320, 3, STRIP)


def random_extrema(n, w, h, seed, n_scales=4, x_lo=0.0):
    """test_gpu_orientation.py's random_extrema right of x_lo, with pairwise distinct responses: a keypoint then names its extremum"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, n_scales + 0.45, n)
    ex = np.stack([rng.uniform(x_lo, w, n), rng.uniform(0, h, n), 0.82 * np.sqrt(2.0) * 2.0 ** z,
                   rng.uniform(0.04, 0.4, n)], axis=1).astype(np.float32)
    return distinct_responses(ex)


def distinct_responses(ex):
    """responses 0.04 + i * 2^-18 in a shuffled order: exact in f32 and pairwise distinct up to 2^16 rows and beyond"""
    n = len(ex)
    assert n < 1 << 17
    perm = np.random.default_rng(n).permutation(n)
    ex[:, 3] = (np.float32(0.04) + perm.astype(np.float32) * np.float32(2.0 ** -18)).astype(np.float32)
    assert len(np.unique(ex[:, 3])) == n
    return ex


def dead_extrema(oracle, stack, n, seed):
    """n extrema in the flat strip for which the ORACLE returns no keypoint (asked, not inferred from the geometry)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 4), np.float32)
    while len(out) < n:
        m = 2 * n
        cand = np.stack([rng.uniform(8.0, 12.0, m), rng.uniform(0, ORIENT_H, m), rng.uniform(2.4, 2.6, m),
                         rng.uniform(0.04, 0.4, m)], axis=1).astype(np.float32)
        cand = distinct_responses(cand)
        alive = np.isin(cand[:, 3], oracle.orient(stack, cand)[:, 4])
        out = np.concatenate([out, cand[~alive]])
    return out[:n]


def peaks_per_extremum(ex, kps):
    """[n] keypoints of each extremum, from the responses (distinct); the keypoints must come by extremum, in index order"""
    order = np.argsort(ex[:, 3], kind="stable")
    idx = order[np.searchsorted(ex[order, 3], kps[:, 4])]
    assert np.array_equal(ex[idx, 3], kps[:, 4]) and np.all(np.diff(idx) >= 0)
    return np.bincount(idx, minlength=len(ex))


# (length, where the run of dead extrema lies: first block of it, blocks)
ORIENT_LISTS = {8192: (0, 1), 8193: (3, 1), 9216: (8, 1), 20000: (9, 2)}


def orient_list(oracle, stack, n):
    """n extrema with a run of dead ones aligned to a block of 1024: at the head (8192), in the middle (8193, 20000: two
    blocks there), at the tail (9216, an exact multiple of 1024)"""
    b0, nb = ORIENT_LISTS[n]
    ex = random_extrema(n, ORIENT_W, ORIENT_H, n, x_lo=STRIP + 30.0)
    ex[b0 * BLOCK:(b0 + nb) * BLOCK] = dead_extrema(oracle, stack, nb * BLOCK, n + 1)
    return distinct_responses(ex)


def orient_cuts(counts):
    """the max_out values of Part 1 from the oracle's per-extremum counts"""
    first = np.concatenate([[0], np.cumsum(counts)])         # offset of each extremum's first keypoint; first[n] = total
    total = int(first[-1])
    j = int(np.flatnonzero((counts >= 3) & (first[:-1] > 1))[0])   # a cut inside an extremum's peaks
    b = len(counts) // BLOCK // 2                            # a cut at a block's base, a middle block
    return sorted({1, int(first[j]) + 1, int(first[BLOCK * b]), total - 1, total, total + 1})


def drop_block_offset(kps, counts, block):
    """the keypoint list a scatter would leave that forgot the offset of `block` (its keypoints written from row 0, the rows it
    should have filled left as they were: zero)"""
    first = np.concatenate([[0], np.cumsum(counts)])
    lo, hi = int(first[block * BLOCK]), int(first[min((block + 1) * BLOCK, len(counts))])
    bad = kps.copy()
    bad[lo:hi] = 0
    bad[:hi - lo] = kps[lo:hi]
    return bad


def interleaved_frames():
    return [noise_frame(ORIENT_W, ORIENT_H, 20 + f, 3) for f in range(3)]


def interleaved_extrema():
    """9000 extrema of three frames, interleaved: (extrema [n,4], frame_of [n])"""
    n = 9000
    ex = random_extrema(n, ORIENT_W, ORIENT_H, 31, x_lo=3.0)
    frame_of = np.random.default_rng(32).integers(0, 3, n).astype(np.uint32)
    return ex, frame_of


def expected_interleaved(oracle, stacks, ex, frame_of):
    """each extremum oriented on its own frame, the keypoints by extremum in index order: (keypoints, frame_of_kp)"""
    kps = np.concatenate([oracle.orient(st, ex[frame_of == f]) for f, st in enumerate(stacks)])
    order = np.argsort(ex[:, 3], kind="stable")
    idx = order[np.searchsorted(ex[order, 3], kps[:, 4])]          # the extremum of every keypoint
    by_extremum = np.argsort(idx, kind="stable")                   # (an extremum's peaks stay in bin order)
    return kps[by_extremum], frame_of[idx[by_extremum]]


def check_keypoints(got, want, what=""):
    """the bar of assert_same_keypoints in test_gpu_orientation.py: the same list, x, y, size, response bit-equal, EVERY angle
    within 1e-3 degrees (circular)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = np.all(got[:, [0, 1, 2, 4]] == want[:, [0, 1, 2, 4]], axis=1)
    assert same.all(), (what, "first row that differs", int(np.argmin(same)), int((~same).sum()))
    d = np.abs(got[:, 3].astype(np.float64) - want[:, 3].astype(np.float64))
    d = np.minimum(d, 360 - d)
    assert d.max(initial=0.0) < 1e-3, (what, "angle", int(d.argmax()), float(d.max()))


def check_extrema(got, want, what=""):
    """the bar of assert_same_extrema in test_gpu_detector.py: the same count, 1e-3 px, 1e-4 relative size, 1e-6 contrast"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if len(want):
        assert np.abs(got[:, :2] - want[:, :2]).max() < 1e-3, (what, np.abs(got[:, :2] - want[:, :2]).max())
        assert np.abs(got[:, 2] / want[:, 2] - 1).max() < 1e-4, what
        assert np.abs(got[:, 3] - want[:, 3]).max() < 1e-6, what


# ---- the staged expectation -------------------------------------------------------------------------------------------------
def select(oracle, rows, cap_f, top_n, min_size):
    """indices (into the frame's rows) of the extrema that reach orientation"""
    head = rows[:cap_f]
    if not top_n:
        return np.arange(len(head), dtype=np.uint32)
    return oracle.topk_filter(head, min(top_n, cap_f), min_size) if len(head) else np.zeros(0, np.uint32)


def expected_frames(oracle, stacks, rows_per_frame, cap_f, top_n, min_size, max_out):
    """-> (keypoints [m,5], frame_of_kp [m], dropped_blobs, dropped_features, [indices selected per frame])"""
    kps, frame_of, picks, dropped_blobs = [], [], [], 0
    for f, (st, rows) in enumerate(zip(stacks, rows_per_frame)):
        idx = select(oracle, rows, cap_f, top_n, min_size)
        k = oracle.orient(st, rows[idx]) if len(idx) else np.zeros((0, 5), np.float32)
        kps.append(k)
        frame_of.append(np.full(len(k), f, np.uint32))
        picks.append(idx)
        dropped_blobs += max(0, len(rows) - cap_f)
    kps, frame_of = np.concatenate(kps), np.concatenate(frame_of)
    total = len(kps)
    kept = min(total, max_out)
    return kps[:kept], frame_of[:kept], dropped_blobs, total - kept, picks


def shared_cap_model(counts, cap_f):
    """the batched call's arithmetic before every frame had a share of its own: the extrema of the batch in ONE list of
    2 * cap_f * n_frames rows, frame_start clamped to it.  -> ([(lo, hi) rows of frame f's own list that survive], dropped_blobs)"""
    counts = np.asarray(counts, np.int64)
    all_cap = 2 * cap_f * len(counts)
    start = np.minimum(np.concatenate([[0], np.cumsum(counts)]), all_cap)        # clamped starts, then the clamped total
    seg = np.diff(start)
    kept = np.minimum(seg, cap_f)
    dropped = max(0, int(counts.sum()) - all_cap) + int((seg - kept).sum())
    return [(0, int(k)) for k in kept], dropped


def model_frames(oracle, stacks, rows_per_frame, cap_f, top_n, min_size, max_out):
    """expected_frames under shared_cap_model"""
    spans, dropped = shared_cap_model([len(r) for r in rows_per_frame], cap_f)
    k, fo, _, df, picks = expected_frames(oracle, stacks, [r[lo:hi] for r, (lo, hi) in zip(rows_per_frame, spans)], cap_f, top_n,
                                          min_size, max_out)
    return k, fo, dropped, df, picks


# ---- Part 2: one frame whose device-side counts pass 8192 ------------------------------------------------------------------
DETECT_W, DETECT_H, DETECT_BLOBS, DETECT_MAX_OUT = 1024, 768, 16384, 20000


def detect_frame():
    return dense(DETECT_W, DETECT_H, 1024)


def pick_min_size(rows, top_n, lo=1000, hi=KERNEL_FORM - 1):
    """a min_size that leaves between lo and hi of the rows (fewer than top_n, so that the count after the filter is theirs)"""
    sizes = np.sort(rows[:, 2])
    want = (lo + min(hi, top_n - 1)) // 2
    min_size = float(np.float32(sizes[len(sizes) - want] if want < len(sizes) else sizes[0]))
    left = int((rows[:, 2] >= np.float32(min_size)).sum())
    assert lo <= left <= min(hi, top_n - 1), (left, lo, hi, top_n)
    return min_size


def detect_requests(rows, kps_total):
    """(top_n, min_size, max_out): untruncated, a capacity that cuts, a long selection, and one with n_dev < 8192 < n_host"""
    assert kps_total + 100 <= DETECT_MAX_OUT
    return [(0, 0.0, kps_total + 100), (0, 0.0, kps_total - 1234), (10000, 0.0, DETECT_MAX_OUT),
            (9000, pick_min_size(rows, 9000), DETECT_MAX_OUT)]


# ---- Part 3: batches ---------------------------------------------------------------------------------------------------------
LONG_W, LONG_H, LONG_BLOBS = 1024, 768, 16384
CAP_W, CAP_H, CAP_BLOBS = 640, 480, 256


def long_frames():
    return {"dense": dense(LONG_W, LONG_H, 1024), "flat": flat_frame(LONG_W, LONG_H), "sparse": sparse(LONG_W, LONG_H, 7),
            "dense2": dense(LONG_W, LONG_H, 2048)}


LONG_ORDERS = [("flat", "dense", "sparse", "dense2"), ("dense", "flat", "sparse", "dense2"), ("dense", "sparse", "dense2", "flat")]
LONG_TOP_N = (0, 2000, 9000)


def cap_frames():
    return {"dense": dense(CAP_W, CAP_H, 640), "dense2": dense(CAP_W, CAP_H, 641), "dense3": dense(CAP_W, CAP_H, 642),
            "flat": flat_frame(CAP_W, CAP_H), "sparse": sparse(CAP_W, CAP_H, 9)}


CAP_BATCHES = [("dense", "dense2"), ("dense", "dense2", "dense3"), ("flat", "dense", "dense2"), ("dense", "flat", "sparse")]
CAP_TOP_N = (0, 100)


# frames so small that several share one workgroup of the extremum compaction (scan cubes of 4 x 4 texels inside a border of 5,
# one cube layer at n_scales = 4: 16 x 12 = 192 cubes a frame, five frames and a part of the sixth in 1024)
SMALL_W, SMALL_H, SMALL_BLOBS, SMALL_FRAMES = 72, 56, 256, 12


def small_cubes():
    return ((SMALL_W - 10 + 3) // 4) * ((SMALL_H - 10 + 3) // 4)


def small_frames():
    return [flat_frame(SMALL_W, SMALL_H) if f == 5 else dense(SMALL_W, SMALL_H, 70 + f) for f in range(SMALL_FRAMES)]
