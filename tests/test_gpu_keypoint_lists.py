"""GPU tests of the list machinery between the extremum scan and the describe launch -- the ordered compactions, the per-frame
top-n filter and the device-side counts (mkd_orient.hip, mkd_detect.hip, lf_mkd.cpp) -- on lists long enough to take the
forms the short test frames never reach: orientation's three-launch form (more than 8192 extrema), lf_mkd_detect with
device-side counts beyond 8192, and lf_mkd_detect_frames_device with segments longer than a sweep step, empty segments, and
frames that alone hold more extrema than the whole batch is allowed to keep.

Every stage is held to the oracle ON THE LIBRARY'S OWN BITS of the stage before (tests/keypoint_list_cases.py): extremum
counts exact, selected indices equal, keypoints x, y, size, response bit-equal, EVERY angle within 1e-3 degrees.  Tied
contrasts at a cut of the segmented filter cannot be injected through an entry point and are not covered (see the cases)."""
import numpy as np
import pytest

import keypoint_list_cases as cases
from conftest import assert_same_descriptors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


# ---- Part 1: orientation, one-launch and three-launch form ------------------------------------------------------------------
@pytest.fixture(scope="module")
def orient_handle(lfp, oracle):
    img = cases.orient_frame()
    h = lfp.MkdHandle(max_features=256, max_image_width=cases.ORIENT_W, max_image_height=cases.ORIENT_H)
    h.set_image(img)
    st = oracle.build_coarse_stack(img)
    for l in range(len(st)):                    # the stack the two sides orient on is the same, bit for bit
        assert np.array_equal(h.coarse_layer(l, cases.ORIENT_W, cases.ORIENT_H), st[l]), l
    return h, st


@pytest.mark.parametrize("n", list(cases.ORIENT_LISTS))
def test_orientation_lists_vs_oracle(oracle, orient_handle, n):
    """8192: the last one-launch length; 8193, 9216, 20000: three launches (a one-element last block, whole blocks, many
    blocks); each list with a run of whole blocks whose counts sum to zero, at the head, in the middle or at the tail"""
    h, st = orient_handle
    ex = cases.orient_list(oracle, st, n)
    want = oracle.orient(st, ex)
    counts = cases.peaks_per_extremum(ex, want)
    got, dropped = h.orient_keypoints(ex)
    assert dropped == 0
    cases.check_keypoints(got, want, n)
    assert np.array_equal(cases.peaks_per_extremum(ex, got), counts)     # the peaks extremum by extremum
    # max_out cuts the ordered list: the head of the library's own untruncated list, bit for bit, the rest counted
    total = len(want)
    for cut in cases.orient_cuts(counts):
        head, dropped = h.orient_keypoints(ex, max_out=cut)
        assert len(head) == min(cut, total) and dropped == total - min(cut, total), (n, cut, len(head), dropped)
        assert np.array_equal(head, got[:cut]), (n, cut)


def test_orientation_device_entry_point_interleaved_frames(lfp, torch, oracle):
    """lf_mkd_orient_keypoints_device on 9000 extrema of three frames, interleaved: frame_of read by the three-launch form"""
    imgs = np.stack(cases.interleaved_frames())
    ex, frame_of = cases.interleaved_extrema()
    want, want_frame = cases.expected_interleaved(oracle, [oracle.build_coarse_stack(i) for i in imgs], ex, frame_of)
    h = lfp.MkdHandle(max_features=256, max_image_width=cases.ORIENT_W, max_image_height=cases.ORIENT_H, max_frames=3)
    d_img = torch.from_numpy(imgs).cuda().contiguous()
    d_ex, d_fo = torch.from_numpy(ex).cuda(), torch.from_numpy(frame_of.view(np.int32)).cuda()
    cap = 18 * len(ex)
    d_k = torch.zeros((cap, 5), device="cuda")
    d_fk = torch.zeros((cap,), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    h.set_images_device(d_img.data_ptr(), 3, cases.ORIENT_W, cases.ORIENT_H, s)
    m, dropped = h.orient_keypoints_device(d_ex.data_ptr(), d_fo.data_ptr(), len(ex), d_k.data_ptr(), d_fk.data_ptr(), cap, s)
    assert dropped == 0
    cases.check_keypoints(d_k[:m].cpu().numpy(), want, "interleaved")
    assert np.array_equal(d_fk[:m].cpu().numpy().view(np.uint32), want_frame)
    # a capacity that cuts: the head of that list and of its frame ids
    cut = len(want) // 2 + 1
    d_k2 = torch.zeros((cut, 5), device="cuda")
    d_fk2 = torch.zeros((cut,), dtype=torch.int32, device="cuda")
    m2, dropped = h.orient_keypoints_device(d_ex.data_ptr(), d_fo.data_ptr(), len(ex), d_k2.data_ptr(), d_fk2.data_ptr(), cut, s)
    assert m2 == cut and dropped == len(want) - cut
    assert torch.equal(d_k2, d_k[:cut]) and torch.equal(d_fk2, d_fk[:cut])


# ---- Part 2: lf_mkd_detect, device-side counts above 8192 -------------------------------------------------------------------
def test_detect_with_counts_beyond_8192(lfp, oracle):
    """One 1024 x 768 frame of more than 8192 extrema through the recorded pipeline (first sighting, recording, replay) and
    through the stage-by-stage form: every extremum, a capacity that cuts, a selection of 10000, and a selection whose
    min_size leaves fewer than 8192 on the device while the host sized the launch for 9000."""
    w, hgt, img = cases.DETECT_W, cases.DETECT_H, cases.detect_frame()
    kw = dict(max_features=cases.DETECT_MAX_OUT, max_image_width=w, max_image_height=hgt, max_blobs=cases.DETECT_BLOBS)
    rec, step = lfp.MkdHandle(**kw), lfp.MkdHandle(flags=lfp.FLAG_DETECT_STEPWISE, **kw)
    st, o_rows = cases.oracle_extrema(oracle, img)
    requests = cases.detect_requests(o_rows, len(oracle.orient(st, o_rows)))
    results = []
    for top_n, min_size, max_out in requests:
        want = step.detect(img, top_n, min_size, max_out)
        for sighting in range(3):                                  # first sighting, recording, replay
            got = rec.detect(img, top_n, min_size, max_out)
            assert got[2:] == want[2:], (top_n, min_size, max_out, sighting, got[2:], want[2:])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (top_n, min_size, max_out, sighting)
        results.append(want)
    # the library's extrema (the handle holds the frame): the oracle's, counts exact
    rows, dropped = rec.detect_extrema(max_out=cases.DETECT_BLOBS)
    assert dropped == 0 and cases.KERNEL_FORM < len(rows) < cases.DETECT_BLOBS
    cases.check_extrema(rows, o_rows, "extrema")
    rows2, _ = step.detect_extrema(max_out=cases.DETECT_BLOBS)
    assert np.array_equal(rows, rows2)
    for l in range(len(st)):
        assert np.array_equal(rec.coarse_layer(l, w, hgt), st[l]), l
    # every request against the staged expectation
    for (top_n, min_size, max_out), (k, d, db, df) in zip(requests, results):
        want_k, _, want_db, want_df, picks = cases.expected_frames(oracle, [st], [rows], cases.DETECT_BLOBS, top_n, min_size, max_out)
        print(f"detect top_n={top_n} min_size={min_size:.4f} max_out={max_out}: extrema {len(rows)}, selected {len(picks[0])}, "
              f"keypoints {len(k)} (expected {len(want_k)}), dropped_features {df} (expected {want_df})")
        assert (db, df) == (want_db, want_df), (top_n, min_size, max_out, db, df, want_db, want_df)
        cases.check_keypoints(k, want_k, (top_n, min_size, max_out))
        assert_same_descriptors(d, rec.describe_keypoints(k), f"detect top_n={top_n} max_out={max_out} vs describe_keypoints")
    top_n, min_size, _ = requests[3]
    assert 1000 <= int((rows[:, 2] >= np.float32(min_size)).sum()) < cases.KERNEL_FORM < top_n     # n_dev < 8192 < n_host
    assert results[1][3] > 0 and len(results[1][0]) == requests[1][2]


# ---- Part 3: lf_mkd_detect_frames_device ------------------------------------------------------------------------------------
class Batch:
    """a handle, the frames of one batch on the device, and room for the results"""

    def __init__(self, lfp, torch, imgs, max_blobs, max_out):
        self.torch, self.n, (self.hgt, self.w) = torch, len(imgs), imgs[0].shape
        self.h = lfp.MkdHandle(max_features=4096, max_image_width=self.w, max_image_height=self.hgt, max_blobs=max_blobs,
                               max_frames=self.n)
        self.d_img = torch.from_numpy(np.stack(imgs)).cuda().contiguous()
        self.max_out = max_out
        self.d_k = torch.zeros((max_out, 5), device="cuda")
        self.d_f = torch.zeros((max_out,), dtype=torch.int32, device="cuda")
        self.d_d = torch.zeros((max_out, 128), device="cuda")
        self.s = torch.cuda.current_stream().cuda_stream

    def detect(self, top_n, min_size, max_out=None):
        """-> (keypoints, frame_of_kp, descriptors, dropped_blobs, dropped_features)"""
        m, db, df = self.h.detect_frames_device(self.d_img.data_ptr(), self.n, self.w, self.hgt, top_n, min_size,
                                                self.d_k.data_ptr(), self.d_f.data_ptr(), self.d_d.data_ptr(),
                                                self.max_out if max_out is None else max_out, self.s)
        self.torch.cuda.synchronize()
        return (self.d_k[:m].cpu().numpy(), self.d_f[:m].cpu().numpy().view(np.uint32), self.d_d[:m].cpu().numpy(), db, df)

    def rows_per_frame(self, max_rows):
        """the library's extrema of the frames the handle holds after a call, frame by frame (the same handle: the scan's
        template follows the batch's size)"""
        d_ex = self.torch.zeros((max_rows, 4), device="cuda")
        d_fo = self.torch.zeros((max_rows,), dtype=self.torch.int32, device="cuda")
        m, dropped = self.h.detect_extrema_device(d_ex.data_ptr(), d_fo.data_ptr(), max_rows, self.s)
        assert dropped == 0
        ex, fo = d_ex[:m].cpu().numpy(), d_fo[:m].cpu().numpy()
        assert np.all(np.diff(fo) >= 0)
        return [ex[fo == f] for f in range(self.n)]

    def describe(self, k, frame_of):
        d_k = self.torch.from_numpy(np.ascontiguousarray(k)).cuda()
        d_f = self.torch.from_numpy(np.ascontiguousarray(frame_of.view(np.int32))).cuda()
        d_o = self.torch.zeros((len(k), 128), device="cuda")
        self.h.describe_keypoints_frames_device(d_k.data_ptr(), d_f.data_ptr(), len(k), d_o.data_ptr(), self.s)
        self.torch.cuda.synchronize()
        return d_o.cpu().numpy()


def check_batch(oracle, batch, stacks, oracle_rows, cap_f, requests, what):
    """every request (top_n, min_size, max_out) of one batch against the staged expectation"""
    results = [batch.detect(*r) for r in requests]
    rows = batch.rows_per_frame(1 << 16)
    for f, (got, want) in enumerate(zip(rows, oracle_rows)):
        cases.check_extrema(got, want, (what, "extrema of frame", f))
    for (top_n, min_size, max_out), (k, fo, d, db, df) in zip(requests, results):
        want_k, want_fo, want_db, want_df, picks = cases.expected_frames(oracle, stacks, rows, cap_f, top_n, min_size, max_out)
        tag = (what, top_n, min_size, max_out)
        print(f"{what} top_n={top_n} min_size={min_size:.4f} max_out={max_out}: extrema per frame {[len(r) for r in rows]}, selected "
              f"{[len(p) for p in picks]}, keypoints per frame {np.bincount(fo, minlength=len(rows)).tolist()} (expected "
              f"{np.bincount(want_fo, minlength=len(rows)).tolist()}), dropped_blobs {db} (expected {want_db}), dropped_features {df} "
              f"(expected {want_df})")
        assert db == want_db, (tag, "dropped_blobs", db, want_db)
        assert df == want_df, (tag, "dropped_features", df, want_df)
        assert np.array_equal(np.bincount(fo, minlength=len(rows)), np.bincount(want_fo, minlength=len(rows))), tag
        assert np.array_equal(fo, want_fo), tag
        cases.check_keypoints(k, want_k, tag)
        if len(k):
            assert_same_descriptors(d, batch.describe(k, fo), f"{what} top_n={top_n} min_size={min_size:.2f}: batch vs describe_keypoints_frames")
    return rows, results


@pytest.fixture(scope="module")
def long_oracle(oracle):
    return {name: (img,) + cases.oracle_extrema(oracle, img) for name, img in cases.long_frames().items()}


@pytest.mark.parametrize("order", cases.LONG_ORDERS, ids=["flat_first", "flat_inner", "flat_last"])
def test_batches_with_long_and_empty_segments(lfp, torch, oracle, long_oracle, order):
    """4 frames of 1024 x 768: two with more than 8192 extrema (segments longer than two sweep steps of the per-frame filter),
    one with a few hundred, one flat (an empty segment in front of, between or behind the others)"""
    imgs, stacks, o_rows = ([long_oracle[x][i] for x in order] for i in range(3))
    batch = Batch(lfp, torch, imgs, cases.LONG_BLOBS, 40000)
    min_size = cases.pick_min_size(long_oracle["dense"][2], 9000)
    requests = [(top_n, ms, 40000) for top_n in cases.LONG_TOP_N for ms in (0.0, min_size)]
    requests.append((0, 0.0, 12345))                                # a budget for the whole batch that cuts inside a frame
    rows, results = check_batch(oracle, batch, stacks, o_rows, cases.LONG_BLOBS, requests, "/".join(order))
    assert max(len(r) for r in rows) > cases.KERNEL_FORM and len(rows[order.index("flat")]) == 0
    assert results[-1][4] > 0 and len(results[-1][0]) == 12345


def test_a_batch_of_flat_frames(lfp, torch):
    batch = Batch(lfp, torch, [cases.flat_frame(cases.LONG_W, cases.LONG_H)] * 4, cases.LONG_BLOBS, 1024)
    for top_n in (0, 2000):
        k, fo, d, db, df = batch.detect(top_n, 0.0)                 # (status OK: the binding raises otherwise)
        assert len(k) == 0 and len(fo) == 0 and d.shape == (0, 128) and (db, df) == (0, 0)


def test_small_frames_share_a_workgroup(lfp, torch, oracle):
    """12 frames of 72 x 56 (192 scan cubes each): a workgroup of the extremum compaction holds five frames and parts of two,
    so frames begin inside workgroups and one of them is flat"""
    imgs = cases.small_frames()
    stacks, o_rows = zip(*[cases.oracle_extrema(oracle, img) for img in imgs])
    batch = Batch(lfp, torch, imgs, cases.SMALL_BLOBS, 4096)
    rows, results = check_batch(oracle, batch, stacks, o_rows, cases.SMALL_BLOBS, [(0, 0.0, 4096), (10, 0.0, 4096), (0, 0.0, 100)],
                                "small frames")
    assert len(rows[5]) == 0 and min(len(r) for i, r in enumerate(rows) if i != 5) > 5 and results[2][4] > 0


@pytest.fixture(scope="module")
def cap_oracle(oracle):
    return {name: (img,) + cases.oracle_extrema(oracle, img) for name, img in cases.cap_frames().items()}


@pytest.mark.parametrize("names", cases.CAP_BATCHES, ids=["+".join(b) for b in cases.CAP_BATCHES])
def test_every_frame_keeps_the_head_of_its_own_list(lfp, torch, oracle, cap_oracle, names):
    """640 x 480 frames of about 4200 extrema each, max_blobs = 256: each alone holds more than 2 * 256 * n_frames.  Every frame
    keeps its own first 256 (include/lf_mkd.h), whatever the frames before it hold, and dropped_blobs sums the rest per frame."""
    imgs, stacks, o_rows = ([cap_oracle[x][i] for x in names] for i in range(3))
    cap_f = cases.CAP_BLOBS
    batch = Batch(lfp, torch, imgs, cap_f, 4096)
    requests = [(top_n, 0.0, 4096) for top_n in cases.CAP_TOP_N]
    rows, results = check_batch(oracle, batch, stacks, o_rows, cap_f, requests, "+".join(names))
    for name, r in zip(names, rows):
        assert len(r) > 2 * cap_f * len(names) if name.startswith("dense") else len(r) <= cap_f
    for (top_n, _, _), (k, fo, d, db, df) in zip(requests, results):
        assert db == sum(max(0, len(r) - cap_f) for r in rows) and df == 0
        per = np.bincount(fo, minlength=len(names))
        assert all((per[f] > 0) == (len(rows[f]) > 0) for f in range(len(names))), per
    if "sparse" in names:                                           # the sparse frame keeps all of its extrema
        f = names.index("sparse")
        k, fo = results[0][0], results[0][1]
        want = oracle.orient(stacks[f], rows[f])
        cases.check_keypoints(k[fo == f], want, "sparse frame")
