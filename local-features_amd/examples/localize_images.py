#!/usr/bin/env python3
"""localize_images --pose FOCAL[,CX,CY] [--model MODEL.npz] [--register ROUNDS] [--bundle ITERS] FOLDER QUERY_1 [QUERY_2 ...]
-- where were photographs taken that were not part of a reconstruction?

  the model:  the images of FOLDER (one size, sorted by name) go through match_collection.py's route -- detect, quantise,
              match a window of 2, verify the epipolar geometry, two-view poses, tracks and their table, an initial pair,
              ROUNDS (default 3) rounds of resection and triangulation, ITERS (default 10) iterations of bundle adjustment
              -- and then ONE LocalFeatures.track_descriptors call (lf_mkd_track_descriptors_device) gives every track
              with a point one 8-bit descriptor from its inlier observations (state 2).  What is kept of the collection is
              model_desc [tracks, 128] uint8, points [tracks, 4] float32 and the table's counts: with --model they are saved
              to MODEL.npz, and a MODEL.npz that exists is loaded instead of building anything (FOLDER is then not read).
  a query:    detect_top_n(2000, min_size 0) and the descriptors quantised, all queries pooled; ONE LocalFeatures.localize
              call: lf_mkd_match_q8_device of all query rows against the model's rows -- its answer is the row_track that
              resection reads -- and lf_mkd_resect_cameras_device with all-zero poses (512 samples, at least 12 inliers at
              4 px).  Neither the collection's descriptors nor its track table are needed for it.

Prints per query its pose (R row-major, then t; world to camera; the world is the model's: its first camera at [I | 0]), its
correspondences, its inliers and the rms reprojection error, or why there is no pose.  One pinhole camera for every image, the
principal point in the middle of the frame unless given.  Image decoding as in match_images.py.  Needs Pillow and torch."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import local_features_python as lfp  # noqa: E402
import match_collection as mc  # noqa: E402

REASONS = ("pose", "not a candidate", "fewer than three correspondences or no candidate pose", "too few inliers")


def build_model(frames, pose, register=3, bundle=10, seed=0, feats=None):
    """frames [n, h, w] float32 in [0, 1], pose = (focal, cx, cy).  Returns (built, out): out = what match_collection returned,
    built = what describe_model reads of it, device tensors all: the pool's quantised rows q8, the track table, the
    observations' states after the last stage that wrote them, the tracks' points and the table's counts."""
    out = mc.match_collection(frames, "window", 2, fundamental=True, pose=pose, register=register, bundle=bundle, seed=seed,
                              feats=feats)
    state = out["bundle_obs_state"] if out["bundle_obs_state"] is not None else out["tri_obs_state"]
    table = (out["table_offsets"], out["table_rows"], out["table_images"], out["table_counts"])
    return dict(table=table, state=state, points=out["tri_points"], counts=out["table_counts"], q8=out["q8"]), out


def describe_model(feats, built):
    """the one call: per track with a point one descriptor from its inlier observations.  Returns the model, a dict of device
    tensors: model_desc [track_capacity, 128] uint8, points [track_capacity, 4] float32, counts [4] int32, and desc_stats
    [track_capacity, 2] int32 (contributors, smallest similarity)."""
    import torch
    desc, stats = feats.track_descriptors(built["q8"], built["table"], built["state"], 2, built["points"], stats=True)
    # triangulation leaves the rows beyond the table's tracks as allocated: the model says "no point" there
    pts, none = built["points"], torch.tensor([0, 0, 0, 2], dtype=torch.float32, device=desc.device)
    live = torch.arange(pts.shape[0], device=desc.device)[:, None] < built["counts"][0]
    return dict(model_desc=desc, points=torch.where(live, pts, none), counts=built["counts"], desc_stats=stats)


def save_model(path, model):
    np.savez(path, model_desc=model["model_desc"].cpu().numpy(), points=model["points"].cpu().numpy(),
             counts=model["counts"].cpu().numpy())


def load_model(path, device):
    import torch
    with np.load(path) as z:
        return {k: torch.from_numpy(np.ascontiguousarray(z[k])).to(device) for k in ("model_desc", "points", "counts")}


def localize_images(feats, model, images, pose, top_n=2000, min_size=0.0, ratio=mc.RATIO, seed=0):
    """images: f32 frames of the handle's size.  Returns (poses [n, 12], stats [n, 4], err [n, 2], row_state, row_track,
    offsets) as LocalFeatures.localize returns them, on the device, and the queries' image offsets."""
    import torch
    dev = torch.device("cuda", feats.device)
    kps, rows = [], []
    for img in images:
        k, d = feats.detect_top_n(img, top_n, min_size)
        kps.append(np.array([(p.x, p.y, p.size, p.angle, p.response) for p in k], np.float32).reshape(-1, 5))
        rows.append(feats.quantize(d))
    offsets = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    intr = torch.tensor([[pose[0], pose[0], pose[1], pose[2]]], dtype=torch.float32, device=dev).repeat(len(images), 1)
    got = feats.localize(up(np.concatenate(rows)), up(np.concatenate(kps)), up(offsets), model["model_desc"], model["points"],
                         model["counts"], intr, ratio=ratio, seed=seed)
    return got + (offsets,)


def pose_lines(names, poses, stats, err):
    lines = []
    for name, P, st, e in zip(names, poses.cpu().numpy(), stats.cpu().numpy(), err.cpu().numpy()):
        if st[2] == 0:
            lines.append(f"{name}: R = [{' '.join('%.5f' % v for v in P[:9])}] t = [{' '.join('%.4f' % v for v in P[9:])}]; "
                         f"{st[1]} inliers of {st[0]} correspondences, rms {e[0]:.2f} px")
        else:
            lines.append(f"{name}: no pose ({REASONS[st[2]]}; {st[0]} correspondences)")
    return lines


def main():
    args, opt = [], {"--pose": None, "--model": None, "--register": "3", "--bundle": "10"}
    it = iter(sys.argv[1:])
    for a in it:
        if a in opt:
            opt[a] = next(it, None)
        else:
            args.append(a)
    if opt["--pose"] is None or len(args) < 2:
        print("Required arguments: --pose FOCAL[,CX,CY] [--model MODEL.npz] [--register ROUNDS] [--bundle ITERS] FOLDER QUERY_1 "
              "[QUERY_2 ...]", file=sys.stderr)
        return 1
    import torch
    queries = [mc.load_gray(p) for p in args[1:]]
    hgt, w = queries[0].shape
    focal, cx, cy = mc.parse_pose(opt["--pose"])
    pose = (focal, w / 2 if cx is None else cx, hgt / 2 if cy is None else cy)
    have = opt["--model"] is not None and os.path.exists(opt["--model"])
    names = [] if have else sorted(f for f in os.listdir(args[0]) if f.lower().endswith((".png", ".jpg", ".jpeg", ".pgm", ".bmp")))
    feats = lfp.LocalFeatures(w, hgt, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3,
                              max_frames=max(len(names), 1))
    if have:
        model = load_model(opt["--model"], torch.device("cuda", feats.device))
        print(f"Model {opt['--model']}: {int(model['counts'][0])} tracks")
    else:
        frames = np.stack([mc.load_gray(os.path.join(args[0], f)) for f in names])
        built, out = build_model(frames, pose, int(opt["--register"]), int(opt["--bundle"]), feats=feats)
        model = describe_model(feats, built)
        n_tracks = int(model["counts"][0])
        described = int((model["desc_stats"][:n_tracks, 0] > 0).logical_and(model["desc_stats"][:n_tracks, 1] > -2 ** 31).sum())
        registered = int((out["tri_poses"][:, :9] != 0).any(1).sum())
        print(f"Model of {len(names)} images ({registered} registered): {n_tracks} tracks, {described} with a descriptor")
        if opt["--model"] is not None:
            save_model(opt["--model"], model)
    poses, stats, err, _, _, _ = localize_images(feats, model, queries, pose)
    for line in pose_lines(args[1:], poses, stats, err):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
