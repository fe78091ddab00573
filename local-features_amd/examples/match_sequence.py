#!/usr/bin/env python3
"""match_sequence [--fundamental] [--guided] [--q8] [--guided-q8] IMAGE_1 IMAGE_2 [IMAGE_3 ...] -- N images of one size through the whole pipeline on the
device, every stage launched once for all of them and nothing copied to the host in between:

  detect_top_n(2000, min_size 0) on all frames      lf_mkd_detect_frames_device
  frame offsets from the keypoints' frame ids        torch.bincount / cumsum
  frame t against frame t + 1, both directions,      LocalFeatures.match_batch(mutual=True): one matcher launch and two
  0.8 ratio test, cross-check                        filter launches for all pairs (lf_mkd_match_pairs_device)
  RANSAC homography (3 px) per pair, or with         LocalFeatures.verify_homography_batch / verify_fundamental_batch
  --fundamental epipolar geometry (1.5 px)
  with --guided: every pair matched again under its   LocalFeatures.match_guided_batch (lf_mkd_match_guided_pairs_device):
  model, then verified once more with the same seed   candidates restricted to the model's transfer disc / epipolar band

  with --q8: the descriptors quantised once to 8 bits  LocalFeatures.quantize, then LocalFeatures.match_q8_batch(mutual=True)
  and the first pass matched on exact integer sums    (lf_mkd_match_q8_pairs_device); a --guided second pass stays on f32
  with --guided-q8: both passes on the 8-bit rows --   LocalFeatures.match_q8_batch, then LocalFeatures.match_q8_guided_batch
  quantised once, matched, verified, matched again     (lf_mkd_match_q8_guided_pairs_device) and verified once more with the
  under each pair's model on the same bytes            same seed; the f32 rows are not read after the quantiser

and prints one line per pair: ratio-test matches t -> t + 1, those the other direction confirms, those the geometry keeps
(and with --guided or --guided-q8: the guided mutual matches -- never fewer than the geometry kept -- and those the second verification keeps).
The frames are ONE descriptor array; the matcher is given it twice -- with the offsets of frames 0 .. N-2 as the a side and
with the offsets of frames 1 .. N-1 as the b side -- so no row is duplicated.

Image decoding as in match_images.py (8-bit luma, then f32 / 255).  Needs Pillow and torch."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import local_features_python as lfp  # noqa: E402


def load_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.float32) / 255.0


def match_sequence(frames, top_n=2000, min_size=0.0, fundamental=False, ratio=0.8, seed=0, feats=None, guided=False, q8=False,
                   guided_q8=False):
    """frames [n, h, w] float32 in [0, 1].  Returns device tensors (keypoints [m,5], descriptors [m,128], frame offsets
    [n + 1], mutual matches t -> t + 1 [m] local to frame t + 1, verified matches [m], model [n - 1,3,3], per pair
    [n - 1, 3]: ratio-test matches, mutual matches, verified inliers).  guided: the matches, the verified matches and the
    model are those of the guided second pass, and per pair has two more columns: guided mutual matches, verified again.
    q8: the first-pass matches come from the 8-bit rows (quantised once, on the device); the guided pass, if any, from `desc`.
    guided_q8: both passes on the 8-bit rows (it implies q8's first pass); the returns and the columns are those of `guided`."""
    import torch
    n, hgt, w = frames.shape
    if feats is None:
        feats = lfp.LocalFeatures(w, hgt, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=n)
    dev = torch.device("cuda", feats.device)
    cap = feats.max_features * n
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev)
        d_img = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).to(dev)
        kps = torch.empty((cap, 5), device=dev)
        frame_of = torch.empty((cap,), dtype=torch.int32, device=dev)
        desc = torch.empty((cap, 128), device=dev)
        m, _, _ = feats._inner.detect_frames_device(d_img.data_ptr(), n, w, hgt, top_n, min_size, kps.data_ptr(),
                                                    frame_of.data_ptr(), desc.data_ptr(), cap, s.cuda_stream)
        kps, frame_of, desc = kps[:m], frame_of[:m].long(), desc[:m]
        o = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(frame_of, minlength=n), 0)])
        # frame t against frame t + 1: the a side is `desc` with the offsets of frames 0 .. n-2, the b side the same array
        # with the offsets of frames 1 .. n-1 -- no row is copied and no offset is read back to the host
        oa, ob = o[:n], o[1:]
        if q8 or guided_q8:
            q = feats.quantize(desc)
            m_ab, m_ba, best, second = feats.match_q8_batch(q, oa, q, ob, ratio=ratio, mutual=True)
            # the int32 scores as floats (exact: |sums| < 2^24), "no candidate" (INT32_MIN) as the f32 path's -inf
            best, second = (torch.where(x == -2 ** 31, float("-inf"), x.float()) for x in (best, second))
        else:
            m_ab, m_ba, best, second = feats.match_batch(desc, oa, desc, ob, ratio=ratio, mutual=True)
        verify = feats.verify_fundamental_batch if fundamental else feats.verify_homography_batch
        model, ver, stats = verify(kps, oa, kps, ob, m_ab, seed=seed)
        # per pair: a row of frame t belongs to pair t; the ratio-test matches are told by best / second, which the
        # cross-check leaves as the a -> b direction found them
        in_pair = frame_of < n - 1
        count = lambda mask: torch.bincount(frame_of[mask & in_pair], minlength=n)[:n - 1]
        columns = [count(best * ratio > second), count(m_ab >= 0), count(ver >= 0)]
        if guided or guided_q8:
            # the verifier's model, threshold (the defaults of both calls) and ratio: every verified match is found again
            kind = "fundamental" if fundamental else "homography"
            if guided_q8:
                m_ab, _, _, _ = feats.match_q8_guided_batch(q, kps, oa, q, kps, ob, model, kind=kind, ratio=ratio, mutual=True)
            else:
                m_ab, _, _, _ = feats.match_guided_batch(desc, kps, oa, desc, kps, ob, model, kind=kind, ratio=ratio, mutual=True)
            model, ver, stats = verify(kps, oa, kps, ob, m_ab, seed=seed)
            columns += [count(m_ab >= 0), count(ver >= 0)]
        per_pair = torch.stack(columns, dim=1)
    return kps, desc, o, m_ab, ver, model, per_pair


def main():
    args = sys.argv[1:]
    flags = ("--fundamental", "--guided", "--q8", "--guided-q8")
    fundamental, guided, q8, guided_q8 = (f in args for f in flags)
    args = [a for a in args if a not in flags]
    if len(args) < 2:
        print("Required arguments: [--fundamental] [--guided] [--q8] [--guided-q8] IMAGE_1 IMAGE_2 [IMAGE_3 ...]", file=sys.stderr)
        return 1
    imgs = [load_gray(a) for a in args]
    if any(i.shape != imgs[0].shape for i in imgs):
        print("the images must have one size", file=sys.stderr)
        return 1
    _, _, o, _, _, _, per_pair = match_sequence(np.stack(imgs), fundamental=fundamental, guided=guided, q8=q8, guided_q8=guided_q8)
    o, per_pair = o.cpu().tolist(), per_pair.cpu().tolist()
    print("Extracted " + ", ".join(str(o[t + 1] - o[t]) for t in range(len(imgs))) + " keypoints")
    what = "one epipolar geometry" if fundamental else "one homography"
    for t, (raw, mutual, inl, *again) in enumerate(per_pair):
        more = f", {again[0]} guided, {again[1]} agree after re-verification" if guided or guided_q8 else ""
        print(f"Pair {t + 1} -> {t + 2}: {raw} matches, {mutual} mutual, {inl} agree with {what}{more}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
