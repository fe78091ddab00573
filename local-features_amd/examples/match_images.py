#!/usr/bin/env python3
"""match_images [--homography | --fundamental [--pose FOCAL]] [--q8] IMAGE_1 IMAGE_2 IMAGE_OUT -- the reference's example (examples/match_images/src/main.rs) on the
MI355X path: load two images, detect_top_n(2000, min_size 0) on each, brute-force match 1->2 and 2->1 with the
0.8 ratio test, draw keypoints and the 1->2 matches side by side.  With --homography the 1->2 matches are verified on the
device first (RANSAC homography, 3 px: LocalFeatures.verify_homography) and only the inliers are drawn; with --fundamental
they are verified by epipolar geometry instead (7-point RANSAC, 1.5 px Sampson distance: LocalFeatures.verify_fundamental),
which keeps the correct matches of a 3-D scene seen from two places, not only those of its dominant plane.  With --q8 both
descriptor sets are quantised to one byte per dimension first and matched on exact integer similarities
(LocalFeatures.quantize / match_q8); the printed lines are the same.  With --fundamental --pose FOCAL (a pinhole camera of
that focal length in pixels for both images, the principal point in the middle of each) the verified matches and F are
turned into the relative pose of camera 2 (LocalFeatures.two_view_pose): the rotation angle, the direction of t, the links
in front of both cameras, those with at least 1 degree of parallax, and s2/s1 of the essential matrix.

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
    focal = None
    if "--pose" in args:
        at = args.index("--pose")
        try:
            focal = float(args[at + 1])
        except (IndexError, ValueError):
            focal = -1.0
        del args[at:at + 2]
    args = [a for a in args if a not in ("--homography", "--fundamental", "--q8")]
    if len(args) != 3 or (homography and fundamental) or (focal is not None and not (fundamental and focal > 0)):
        print("Required arguments: [--homography | --fundamental [--pose FOCAL]] [--q8] IMAGE_1 IMAGE_2 IMAGE_OUT", file=sys.stderr)
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
        F, m12 = feats.verify_fundamental(kp1, kp2, m12, 1.5)
        print(f"Verified 1 -> 2: {len(m12)} matches agree with one epipolar geometry")
        if focal is not None and F is not None:
            K1, K2 = ((focal, focal, i.shape[1] / 2.0, i.shape[0] / 2.0) for i in (img1, img2))
            R, t, st, sg, _ = feats.two_view_pose(F, (K1, K2), (kp1, kp2), links=m12, points=False)
            if st[2] < 0:
                print("Pose 1 -> 2: none")
            else:
                angle = np.degrees(np.arccos(np.clip((np.trace(R.astype(np.float64)) - 1) / 2, -1, 1)))
                print(f"Pose 1 -> 2: rotation {angle:.2f} deg, t {t[0]:+.3f} {t[1]:+.3f} {t[2]:+.3f}, {st[0]} / {len(m12)} links in "
                      f"front, {st[3]} with parallax, s2/s1 {sg[1]:.3f}")
    draw(img1, img2, kp1, kp2, m12, args[2])
    return 0


if __name__ == "__main__":
    sys.exit(main())
