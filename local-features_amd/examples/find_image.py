#!/usr/bin/env python3
"""find_image QUERY DB_1 [DB_2 ...] -- which database image shows what the query shows?  Retrieval against a pooled database,
the ratio test taken against the best neighbour from ANOTHER image: what a top-2 matcher cannot express.

Every image goes through detect_top_n(2000, min_size 0) and its descriptors are quantised to one byte per dimension
(LocalFeatures.quantize).  The database descriptors are pooled into one array with image offsets, and ONE
LocalFeatures.knn_q8 call with k = 8 gives every query row its eight nearest pool rows on exact integer similarities.  A
query row votes for the image of its nearest neighbour; the vote counts iff (float)best * 0.8 > (float)rival, rival being the
first of its k neighbours that lies in a different image (none among the k, or fewer than two candidates: the vote counts).
The database images are printed ranked by votes.

Image decoding is match_images.py's (8-bit luma, then f32 / 255).  Needs Pillow."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import local_features_python as lfp  # noqa: E402

K = 8
RATIO = 0.8


def load_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.float32) / 255.0


def rank_images(index, score, image_offsets, ratio=RATIO):
    """index / score [n, k] int32 as knn_q8 returns them against a pool in which image m owns the rows
    image_offsets[m] .. image_offsets[m + 1] - 1 -> votes [n_images] int64.  Row i votes for the image of index[i, 0]; the vote
    counts iff (float)score[i, 0] * ratio > (float)score[i, c], c the first column whose neighbour lies in another image (one
    f32 multiplication, both conversions exact); no such column, or fewer than two candidates: it counts.  A row without a
    candidate (index -1) does not vote."""
    index, score = np.asarray(index, np.int64), np.asarray(score, np.int32)
    offsets = np.asarray(image_offsets, np.int64)
    n_images = len(offsets) - 1
    votes = np.zeros(n_images, np.int64)
    if index.size == 0:
        return votes
    image = np.where(index >= 0, np.searchsorted(offsets, index, side="right") - 1, -1)     # [n, k], -1: no neighbour
    rows = np.arange(len(index))
    other = (image != image[:, :1]) & (image >= 0)
    has_rival = other.any(axis=1)
    rival = score[rows, np.argmax(other, axis=1)]                                            # the first such column
    passes = score[:, 0].astype(np.float32) * np.float32(ratio) > rival.astype(np.float32)
    counts = (image[:, 0] >= 0) & (~has_rival | passes)
    np.add.at(votes, image[counts, 0], 1)
    return votes


def find_image(query, database, top_n=2000, min_size=0.0, feats=None, k=K, ratio=RATIO):
    """query and database: f32 images.  Returns (votes [n_images], image_offsets, query rows, pool rows, index, score)."""
    images = [query] + list(database)
    if feats is None:
        feats = lfp.LocalFeatures(max(i.shape[1] for i in images), max(i.shape[0] for i in images), 3000, max_blobs=8000,
                                  n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3)
    rows = [feats.quantize(feats.detect_top_n(img, top_n, min_size)[1]) for img in images]
    q, pool = rows[0], np.concatenate(rows[1:]) if len(rows) > 1 else np.zeros((0, 128), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows[1:]])]).astype(np.int64)
    if len(pool) == 0 or len(q) == 0:
        empty = np.zeros((len(q), k), np.int32)
        return np.zeros(len(database), np.int64), offsets, q, pool, empty - 1, empty + np.int32(-2 ** 31)
    index, score = feats.knn_q8(q, pool, k)
    return rank_images(index, score, offsets, ratio), offsets, q, pool, index, score


def main():
    args = sys.argv[1:]
    if len(args) < 2:
        print("Required arguments: QUERY DB_1 [DB_2 ...]", file=sys.stderr)
        return 1
    votes, offsets, q, _, _, _ = find_image(load_gray(args[0]), [load_gray(p) for p in args[1:]])
    print(f"Query: {len(q)} keypoints against {int(offsets[-1])} in {len(args) - 1} images")
    for rank, m in enumerate(sorted(range(len(votes)), key=lambda m: (-votes[m], m)), 1):
        print(f"{rank}. {args[1 + m]}: {int(votes[m])} votes ({int(offsets[m + 1] - offsets[m])} keypoints)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
