#!/usr/bin/env python3
"""find_image QUERY DB_1 [DB_2 ...] -- which database image shows what the query shows?  Retrieval against a pooled database,
the ratio test taken against the best neighbour from ANOTHER image: what a top-2 matcher cannot express.

Every image goes through detect_top_n(2000, min_size 0) and its descriptors are quantised to one byte per dimension
(LocalFeatures.quantize).  The database descriptors are pooled into one array with image offsets, and ONE
LocalFeatures.knn_q8 call with k = 8 gives every query row its eight nearest pool rows on exact integer similarities.  A
query row votes for the image of its nearest neighbour; the vote counts iff (float)best * 0.8 > (float)rival, rival being the
first of its k neighbours that lies in a different image (none among the k, or fewer than two candidates: the vote counts).
The database images are printed ranked by votes.

--exact asks the device for that rule itself instead of approximating it from k neighbours: the pool carries one image id per
row, ONE LocalFeatures.match_q8_grouped call (ratio 0.8) accepts a query row's nearest neighbour iff it beats the best pool
row of any other image -- however many near-duplicates the matched image holds -- and ONE LocalFeatures.vote_groups call counts
the accepted rows per image.  Nothing but the vote table comes back to the host.  The ranking lines are the same.

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


def rank_images_exact(match, groups, n_images):
    """match [n] int32 as match_q8_grouped returns it (a pool row or -1) and groups [n_pool], the image of every pool row
    -> votes [n_images] int64: the numpy statement of vote_groups with one group of query rows.  Row i votes for
    groups[match[i]] iff 0 <= match[i] < n_pool and that image id is below n_images."""
    match, groups = np.asarray(match, np.int64).reshape(-1), np.asarray(groups, np.int64).reshape(-1)
    votes = np.zeros(n_images, np.int64)
    ok = (match >= 0) & (match < len(groups))
    image = groups[match[ok]]
    np.add.at(votes, image[image < n_images], 1)
    return votes


def describe_all(query, database, top_n=2000, min_size=0.0, feats=None):
    """(feats, query rows, pool rows, image_offsets): the quantised descriptors of the query and of the pooled database"""
    images = [query] + list(database)
    if feats is None:
        feats = lfp.LocalFeatures(max(i.shape[1] for i in images), max(i.shape[0] for i in images), 3000, max_blobs=8000,
                                  n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3)
    rows = [feats.quantize(feats.detect_top_n(img, top_n, min_size)[1]) for img in images]
    q, pool = rows[0], np.concatenate(rows[1:]) if len(rows) > 1 else np.zeros((0, 128), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows[1:]])]).astype(np.int64)
    return feats, q, pool, offsets


def find_image_exact(query, database, top_n=2000, min_size=0.0, feats=None, ratio=RATIO):
    """query and database: f32 images.  Returns (votes [n_images], image_offsets, query rows, pool rows, groups, match): the
    exact rule, one match_q8_grouped call and one vote_groups call on the device."""
    import torch
    feats, q, pool, offsets = describe_all(query, database, top_n, min_size, feats)
    n_images = len(database)
    groups = np.repeat(np.arange(n_images, dtype=np.uint32), np.diff(offsets))
    if len(pool) == 0 or len(q) == 0:
        return np.zeros(n_images, np.int64), offsets, q, pool, groups, np.full(len(q), -1, np.int32)
    dev = torch.device("cuda", feats.device)
    d_groups = torch.from_numpy(groups.view(np.int32)).to(dev)
    match = feats.match_q8_grouped(torch.from_numpy(q).to(dev), torch.from_numpy(pool).to(dev), d_groups, ratio)
    votes = feats.vote_groups(match, d_groups, n_images)
    return votes.cpu().numpy().reshape(-1).astype(np.int64), offsets, q, pool, groups, match.cpu().numpy()


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
    args = [a for a in sys.argv[1:] if a != "--exact"]
    exact = len(args) != len(sys.argv) - 1
    if len(args) < 2:
        print("Required arguments: [--exact] QUERY DB_1 [DB_2 ...]", file=sys.stderr)
        return 1
    votes, offsets, q, _, _, _ = (find_image_exact if exact else find_image)(load_gray(args[0]), [load_gray(p) for p in args[1:]])
    print(f"Query: {len(q)} keypoints against {int(offsets[-1])} in {len(args) - 1} images")
    for rank, m in enumerate(sorted(range(len(votes)), key=lambda m: (-votes[m], m)), 1):
        print(f"{rank}. {args[1 + m]}: {int(votes[m])} votes ({int(offsets[m + 1] - offsets[m])} keypoints)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
