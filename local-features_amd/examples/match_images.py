#!/usr/bin/env python3
"""match_images [--homography | --fundamental] [--q8] IMAGE_1 IMAGE_2 IMAGE_OUT -- the reference's example (examples/match_images/src/main.rs) on the
MI355X path: load two images, detect_top_n(2000, min_size 0) on each, brute-force match 1->2 and 2->1 with the
0.8 ratio test, draw keypoints and the 1->2 matches side by side.  With --homography the 1->2 matches are verified on the
device first (RANSAC homography, 3 px: LocalFeatures.verify_homography) and only the inliers are drawn; with --fundamental
they are verified by epipolar geometry instead (7-point RANSAC, 1.5 px Sampson distance: LocalFeatures.verify_fundamental),
which keeps the correct matches of a 3-D scene seen from two places, not only those of its dominant plane.  With --q8 both
descriptor sets are quantised to one byte per dimension first and matched on exact integer similarities
(LocalFeatures.quantize / match_q8); the printed lines are the same.

Image decoding follows main.rs:44-60: 8-bit luma, then f32 / 255 (Pillow's "L" conversion stands in for the `image`
crate's grayscale(); they may differ by one LSB).  Needs Pillow."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import local_features_python as lfp  # noqa: E402


def load_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.float32) / 255.0


def features(img1, img2):
    """The example's LocalFeatures handle for two images (main.rs:62-76)."""
    return lfp.LocalFeatures(max(img1.shape[1], img2.shape[1]), max(img1.shape[0], img2.shape[0]), 3000,
                             max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3)


def match_images(img1, img2, top_n=2000, min_size=0.0, feats=None, q8=False):
    """Returns (keypoints1, keypoints2, matches 1->2, matches 2->1) as the example computes them (main.rs:62-121), with
    `feats` (default: a new handle from `features`).  q8: the descriptors are quantised to 8 bits and matched as such."""
    if feats is None:
        feats = features(img1, img2)
    kp1, d1 = feats.detect_top_n(img1, top_n, min_size)
    kp2, d2 = feats.detect_top_n(img2, top_n, min_size)
    if q8:
        q1, q2 = feats.quantize(d1), feats.quantize(d2)
        m12 = feats.match_q8(q1, q2) if len(q2) >= 2 else []
        m21 = feats.match_q8(q2, q1) if len(q1) >= 2 else []
    else:
        m12, m21 = feats.match_both(d1, d2)        # main.rs:113-116: both directions, one launch on the device
    return kp1, kp2, d1, d2, m12, m21




def draw(img1, img2, kp1, kp2, matches, out_path):
    from PIL import Image, ImageDraw
    h = max(img1.shape[0], img2.shape[0])
    canvas = Image.new("L", (img1.shape[1] + img2.shape[1], h))
    canvas.paste(Image.fromarray((img1 * 255).astype(np.uint8)), (0, 0))
    canvas.paste(Image.fromarray((img2 * 255).astype(np.uint8)), (img1.shape[1], 0))
    d = ImageDraw.Draw(canvas)
    for k in kp1:
        d.ellipse([k.x - k.size, k.y - k.size, k.x + k.size, k.y + k.size], outline=255)
    for k in kp2:
        ox = img1.shape[1]
        d.ellipse([ox + k.x - k.size, k.y - k.size, ox + k.x + k.size, k.y + k.size], outline=255)
    for i, j in matches:
        d.line([kp1[i].x, kp1[i].y, img1.shape[1] + kp2[j].x, kp2[j].y], fill=255)
    canvas.save(out_path)


def main():
    args = sys.argv[1:]
    homography, fundamental = "--homography" in args, "--fundamental" in args
    q8 = "--q8" in args
    args = [a for a in args if a not in ("--homography", "--fundamental", "--q8")]
    if len(args) != 3 or (homography and fundamental):
        print("Required arguments: [--homography | --fundamental] [--q8] IMAGE_1 IMAGE_2 IMAGE_OUT", file=sys.stderr)
        return 1
    img1, img2 = load_gray(args[0]), load_gray(args[1])
    feats = features(img1, img2)
    kp1, kp2, _, _, m12, m21 = match_images(img1, img2, feats=feats, q8=q8)
    print(f"Extracted {len(kp1)} and {len(kp2)} keypoints")
    print(f"Matching 1 -> 2: {len(m12)} matches")
    print(f"Matching 2 -> 1: {len(m21)} matches")
    if homography:
        _, m12 = feats.verify_homography(kp1, kp2, m12, 3.0)   # on the device that detected and matched them
        print(f"Verified 1 -> 2: {len(m12)} matches agree with one homography")
    if fundamental:
        _, m12 = feats.verify_fundamental(kp1, kp2, m12, 1.5)
        print(f"Verified 1 -> 2: {len(m12)} matches agree with one epipolar geometry")
    draw(img1, img2, kp1, kp2, m12, args[2])
    return 0


if __name__ == "__main__":
    sys.exit(main())
