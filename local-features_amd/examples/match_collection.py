#!/usr/bin/env python3
"""match_collection [--window W | --all | --retrieve K | --select K] [--fundamental] [--tracks] [--table] [--pairs] [--min-inliers M] [--expand K [--min-shared M]] [--pose FOCAL[,CX,CY]] [--view-graph DEG] [--global SWEEPS] [--triangulate [POSES.npy]] [--register ROUNDS] [--bundle ITERS [--refine-focal] [--refine-principal]] IMAGE_1 IMAGE_2 [IMAGE_3 ...] -- N images of one size,
matched along any list of image pairs ("edges") on the device: an image sits on as many edges as the list says, and no
descriptor row is copied for it.

  detect_top_n(2000, min_size 0) on all frames       lf_mkd_detect_frames_device
  the descriptors quantised once to 8 bits           LocalFeatures.quantize
  the edges:  --window W  t against t + 1 .. t + W   (the default, W = 2)
              --all       every i < j
              --retrieve K  every image against the K images that share most exact votes with it, chosen on the device:
                          LocalFeatures.match_q8_grouped of the pool against itself with every row's own image excluded,
                          LocalFeatures.vote_groups into an [N][N] table, torch.topk per image
              --select K  the same vote table, the edges chosen by LocalFeatures.select_edges (lf_mkd_select_edges_device)
                          with skip_self, unique and min_votes = 1: ties go to the lower image, a pair two images picked
                          mutually is ONE edge (smaller, larger), an image nobody voted for is not picked; the list has
                          N * K entries, the ones behind the edges name no image and have empty ranges everywhere
  both sides' edge layouts                           lf_mkd_edge_layout_device (inside match_q8_edges)
  every edge, both directions, 0.8 ratio test,       LocalFeatures.match_q8_edges(mutual=True): one matcher launch and two
  cross-check                                        filter launches for all edges (lf_mkd_match_q8_edges_device)
  the keypoints brought into the edge layouts        LocalFeatures.gather_edge_rows (20-byte rows: the only rows copied)
  RANSAC homography (3 px) per edge, or with         LocalFeatures.verify_homography_batch / verify_fundamental_batch, on the
  --fundamental epipolar geometry (1.5 px)           edge layouts as they are
  with --tracks the tracks of the verified matches:  LocalFeatures.build_tracks (lf_mkd_build_tracks_device): per keypoint the
  the keypoints the edges tie together               track it belongs to, per track its length and its conflicting keypoints
  with --table (which implies --tracks) the track    LocalFeatures.track_table (lf_mkd_track_table_device): the consistent tracks
  table, and the keypoints in its order              of two or more keypoints as a CSR table; LocalFeatures.gather_track_rows
  with --pairs the link table: per edge the list     LocalFeatures.link_table (lf_mkd_link_table_device) on the verified matches,
  of its verified correspondences, and both          and LocalFeatures.gather_track_rows once per side
  sides' keypoints in its order
  with --min-inliers M (which implies the link       the same call with min_links = M: edges with fewer verified matches are
  table) the tracks of the supported edges only      dropped on the device, and --tracks / --table build from its pruned matches
  with --expand K (which implies --table) a second   LocalFeatures.covisibility (lf_mkd_covisibility_device) of the track table with
  round: per image the K images it shares most       the first round's edges zeroed -- tracks tie together images that were never
  tracks with without having been matched against    matched against each other --, LocalFeatures.select_edges on that table
  them (at least --min-shared M of them, default     (min_votes = M, skip_self, unique), the same matcher and verifier on the
  8), matched and verified like the first round,     proposed edges, their links ADDED to the forest (build_tracks(into=track)),
  and the tracks of both rounds together             then the statistics and the table once more
  with --pose FOCAL[,CX,CY] (one pinhole camera for  LocalFeatures.two_view_pose (lf_mkd_two_view_pose_device) after the link
  every image, the principal point in the middle     table: E = K^T F K per edge, its four (R, t) candidates voted by the edge's
  of the frame unless given; implies --fundamental   links, the links triangulated; nothing leaves the device before the lines
  and --pairs) the relative pose of every edge       are printed
  with --view-graph DEG (needs --pose) the posed      LocalFeatures.view_graph (lf_mkd_view_graph_device) after the poses: an edge
  edges checked against each other and a global      none of whose triangles closes within DEG degrees is dropped, its matches
  rotation per image                                 go to -1 before build_tracks, and the initial pair is a supported edge
  with --triangulate [POSES.npy] (needs --pose;       LocalFeatures.triangulate_tracks (lf_mkd_triangulate_tracks_device) on the track
  implies --table) a 3-D point per track under the   table: pair hypotheses, least squares over the winner's inliers, two trimming
  [images][12] poses of the file (R row-major, then  rounds at 4 px; without a file the edge with the most links with parallax is
  t; world to camera)                                the initial pair, [I | 0] and its [R | t], chosen on the device, and every
                                                     other image stays all zero: not registered
  with --global SWEEPS (needs --pose and              LocalFeatures.tree_poses (lf_mkd_tree_poses_device) on the view graph's rotations
  --view-graph; implies --triangulate) every image    and tree, then LocalFeatures.global_positions (lf_mkd_global_positions_device) in
  posed at once: no initial pair, no rounds           place: all centres and points by SWEEPS alternating solves; then the
                                                     triangulation, and with --bundle the bundle with two images held
  with --register ROUNDS (needs --pose; implies       ROUNDS times LocalFeatures.resect_cameras (lf_mkd_resect_cameras_device) in
  --triangulate) the other images registered from     place on the pose array -- P3P samples over the keypoints an image owns in
  the points and the points triangulated again       tracks with a point, 512 samples, at least 12 inliers at 4 px -- and then
                                                     triangulate_tracks again, nothing read back in between
  with --bundle ITERS (1 .. 64; needs --pose; implies LocalFeatures.bundle_adjust (lf_mkd_bundle_adjust_device) after the rounds, in
  --triangulate) poses and points refined jointly     place: ITERS Levenberg-Marquardt iterations of 10 CG steps over the
                                                     triangulation's inlier observations, the images posed before the rounds held
  with --refine-focal / --refine-principal (need      LocalFeatures.bundle_adjust_intrinsics (lf_mkd_bundle_adjust_intrinsics_device)
  --bundle) the one lens of the images refined too    in its place: one group, the focal scale and / or the principal point's shift;
                                                     the refined focal is printed beside the bundle lines

and prints one line per edge, ranked by the matches the geometry keeps; with --tracks also how many tracks of two and of three
or more keypoints there are, how many of them are consistent (no two keypoints of one image), the longest one, and the share
of the keypoints that sit in a consistent track; with --table also the number of tracks and observations in the table and the
first three tracks as image:x,y lists; with --pairs also the number of edges and correspondences in the link table and the
first three correspondences of the best edge as x,y -> x,y; with --expand also one line with the proposed edges and how many of
them kept a verified match, and the track lines once more for the expanded forest; with --pose per edge the rotation angle,
the direction of t, the links in front of both cameras out of the edge's links, those with at least 1 degree of parallax and
s2/s1 of the essential matrix (1 for a true one); with --view-graph the usable, supported, rejected, unchecked and kept edges
and the images that got a rotation; with --triangulate the tracks, the registered images, the points, the inlier
observations and the median parallax; with --register per round the images registered so far, those the round added and the
points; with --bundle the counts, one line per iteration of the trace and the rms reprojection error before and after.  Nothing is read back before those counts: the
output arrays are sized from a bound the host knows -- an image sits on at most D edges of a side, so D times the number of
keypoints bounds that side's layout.

Image decoding as in match_images.py (8-bit luma, then f32 / 255).  Needs Pillow and torch."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import local_features_python as lfp  # noqa: E402

RATIO = 0.8


def load_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.float32) / 255.0


def window_edges(n, w):
    """(edge_a, edge_b, degree): t against t + 1 .. t + w; no image is on more than w edges of a side"""
    pairs = [(t, t + d) for d in range(1, w + 1) for t in range(n - d)]
    return [p[0] for p in pairs], [p[1] for p in pairs], min(w, n - 1)


def all_edges(n):
    """(edge_a, edge_b, degree): every i < j"""
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return [p[0] for p in pairs], [p[1] for p in pairs], n - 1


def vote_table(feats, q, o, frame_of, n, ratio=RATIO):
    """votes [n, n] int32 on the device: votes[i, j] = the rows of image i whose best match among the rows of all OTHER images
    lies in image j and beats the best row of any third image by `ratio`"""
    lo, hi = o[frame_of], o[frame_of + 1]                      # every row's own image is no candidate
    match = feats.match_q8_grouped(q, q, frame_of.int(), ratio=ratio, exclude=(lo.int(), hi.int()))
    return feats.vote_groups(match, frame_of.int(), n, groups_a=frame_of.int(), n_groups_a=n)


def retrieved_edges(feats, q, o, frame_of, n, k, ratio=RATIO):
    """(edge_a, edge_b) as device tensors [n * k]: image i against the k images with most votes for it -- a row votes for the
    image of its best match among the rows of all OTHER images if that beats the best row of any other image by `ratio`"""
    import torch
    votes = vote_table(feats, q, o, frame_of, n, ratio)
    votes = votes.masked_fill(torch.eye(n, dtype=torch.bool, device=votes.device), -1)
    top = torch.topk(votes.long(), k, dim=1).indices            # [n, k]
    return torch.arange(n, dtype=torch.int32, device=top.device).repeat_interleave(k), top.reshape(-1).int()


def match_collection(frames, mode="window", arg=2, top_n=2000, min_size=0.0, fundamental=False, ratio=RATIO, seed=0, feats=None, tracks=False,
                     table=False, pairs=False, min_inliers=None, expand=None, min_shared=8, pose=None, triangulate=None, register=0, bundle=0,
                     refine_focal=False, refine_principal=False, view_graph=None, global_sweeps=0):
    """frames [n, h, w] float32 in [0, 1]; mode "window" (arg = W), "all", "retrieve" or "select" (arg = K).  Returns a dict of device
    tensors: edge_a / edge_b [E]; offsets [n + 1] of the frames; keypoints [m,5] and q8 [m,128], the pool; layout_a / layout_b
    [E + 1], the two edge layouts; match and verified, the mutual and the verified matches in the a side's layout; model
    [E,3,3] and stats [E,4] as the verifier returns them; per_edge [E,3]: ratio-test matches a -> b, mutual, verified.  With
    `tracks` also track [m] (per keypoint the smallest keypoint of its track under the verified matches), track_len and
    track_dup [m] (at a track's label its keypoints and its conflicting keypoints), and track_counts [6] int64: tracks of
    length >= 2, the consistent ones among them, tracks of length >= 3, the consistent ones, the longest track, the keypoints
    in a consistent track of length >= 2; without, those four are None.  With `table` (which implies `tracks`) also the table of
    the consistent tracks of length >= 2 as LocalFeatures.track_table returns it -- table_offsets [m // 2 + 1], table_rows [m],
    table_images [m], table_row_track [m], table_counts [4] -- and table_keypoints [m,5], the keypoints in the table's order
    (LocalFeatures.gather_track_rows); without, those six are None.  With `pairs`, or with min_inliers (an int: edges with
    fewer verified matches are left out), also the link table of the verified matches as LocalFeatures.link_table returns it
    -- link_offsets [E + 1], link_a / link_b / link_edge [layout capacity], edge_links [E], link_counts [4] --, link_keypoints_a /
    link_keypoints_b, both sides' keypoints in the table's order, and with min_inliers match_kept, the verified matches of the
    kept edges alone, from which the tracks are then built; without, those nine are None.  In mode "select" edge_a / edge_b have
    n * K entries, -1 behind the edges (an empty image to every call here), and votes [n, n], edge_votes [n * K], rank and
    rank_votes [n, K] and select_counts [4] are what LocalFeatures.select_edges took and returned; otherwise those five are
    None.  With `expand` (an int K; implies `table`) a second round of edges: covisibility [n, n], the tracks every two images
    share in the first round's table with the first round's edges zeroed (LocalFeatures.covisibility); expand_edge_a /
    expand_edge_b [n * K] and expand_counts [4], what LocalFeatures.select_edges proposes from it (min_votes = min_shared,
    skip_self, unique); expand_layout_a, expand_verified and expand_per_edge, the proposed edges matched and verified like the
    first round's; first_round, a dict with the first round's track_counts and table_* entries -- and track, track_len,
    track_dup, track_counts and the table_* entries are then those of the forest with both rounds' links (the second round's
    are added in place: build_tracks(into=track)).  Without, those seven are None.  With `pose` = (focal, cx, cy), one pinhole
    camera for every image (implies `pairs`; it wants `fundamental`), also the relative pose of every edge from its F and its
    links as LocalFeatures.two_view_pose returns it -- pose_R [E,3,3], pose_t [E,3], pose_stats [E,4], pose_sigma [E,3] and
    pose_points [layout capacity,4], the links triangulated in the a camera's frame; without, those five are None.  With
    `triangulate` (it wants `pose` and implies `table`) also the 3-D point of every track of the table as
    LocalFeatures.triangulate_tracks returns it -- tri_poses [n,12] (R row-major, then t; world to camera), tri_points
    [tracks,4], tri_stats [tracks,4], tri_err [tracks,2] and tri_obs_state [observations] (with `register` = ROUNDS > 0, which
    implies `triangulate`, those after ROUNDS rounds of resect_cameras in place on tri_poses and triangulate_tracks, and
    register_rounds = per round (the resection's stats [n,4], the triangulation's stats [tracks,4])); `triangulate` is an [n,12] array of
    poses, or True: the edge with the most links with parallax is the initial pair, [I | 0] and its [R | t], and every other
    image stays all zero, which says "not registered"; without, those five are None.  `bundle` = ITERS > 0 (needs `triangulate`)
    then runs LocalFeatures.bundle_adjust in place on tri_poses and tri_points and adds bundle_trace [ITERS,8], bundle_counts [4],
    bundle_obs_state and bundle_rms [2] (before, after); None without.  With `refine_focal` / `refine_principal` the bundle step
    is LocalFeatures.bundle_adjust_intrinsics with every image in one group: the shared focal length (its scale) and / or the
    principal point (its shift) are refined too, bundle_trace is [ITERS,9] and bundle_counts [5], bundle_groups [1,3] = (s, dx,
    dy), and `intrinsics` [n,4] (what `pose` gave, per image) is updated in place for everything after.  With `view_graph` =
    DEG (the loop threshold in degrees; it wants `pose`) LocalFeatures.view_graph runs after the poses: vg_rotations [n,3,3],
    vg_edge_stats [E,4], vg_residual [E], vg_image_stats [n,4], vg_counts [8] and vg_match, the matches with the entries of the
    edges it does not keep at -1 -- the tracks are then built from vg_match, and the initial pair is chosen among the supported
    edges only; None without, and nothing else changes."""
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
        kps, frame_of, desc = kps[:m].contiguous(), frame_of[:m].long(), desc[:m]
        o = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(frame_of, minlength=n), 0)])
        q = feats.quantize(desc)                                # once; the f32 rows are not read again
        votes = e_votes = rank = rank_votes = s_counts = None
        if mode == "retrieve":
            ea, eb = retrieved_edges(feats, q, o, frame_of, n, arg, ratio)
            deg_a, deg_b = arg, n - 1                           # image i is the a side of its own k edges, the b side of at most n - 1
        elif mode == "select":
            votes = vote_table(feats, q, o, frame_of, n, ratio)
            ea, eb, e_votes, rank, rank_votes, s_counts = feats.select_edges(votes, arg, min_votes=1, skip_self=True, unique=True,
                                                                             capacity=n * arg)
            deg_a = deg_b = n - 1                               # (smaller, larger): an image meets every other one at most once
        else:
            ea, eb, deg = window_edges(n, arg) if mode == "window" else all_edges(n)
            ea, eb = torch.tensor(ea, dtype=torch.int32, device=dev), torch.tensor(eb, dtype=torch.int32, device=dev)
            deg_a = deg_b = deg
        n_edges = int(ea.numel())
        cap_a, cap_b = deg_a * m, deg_b * m                     # bounds of the two layouts that need no look at the device
        m_ab, m_ba, best, second, la, lb = feats.match_q8_edges(q, o, q, o, ea, eb, ratio=ratio, mutual=True, capacity_a=cap_a,
                                                               capacity_b=cap_b)
        ka = feats.gather_edge_rows(kps, o, ea, la, capacity=cap_a)
        kb = feats.gather_edge_rows(kps, o, eb, lb, capacity=cap_b)
        verify = feats.verify_fundamental_batch if fundamental else feats.verify_homography_batch
        model, ver, stats = verify(ka, la, kb, lb, m_ab, seed=seed)
        # per edge: which edge an entry of the a side's layout belongs to (entries behind the last edge: none)
        edge_of = torch.searchsorted(la, torch.arange(cap_a, device=dev), right=True) - 1
        count = lambda mask: torch.bincount(edge_of[mask], minlength=n_edges + 1)[:n_edges]
        raw = (best != -2 ** 31) & ((ratio <= 0) | (best.float() * ratio > second.float()))   # (both conversions are exact)
        per_edge = torch.stack([count(raw), count(m_ab >= 0), count(ver >= 0)], dim=1)
        l_off = l_a = l_b = l_edge = l_links = l_kept = l_counts = l_ka = l_kb = None
        if pairs or min_inliers is not None or pose is not None:
            l_off, l_a, l_b, l_edge, l_links, l_kept, l_counts = feats.link_table(
                o, ea, eb, la, ver, min_links=min_inliers or 0, capacity=cap_a, n_rows=m, kept_match=min_inliers is not None)
            l_ka, l_kb = feats.gather_track_rows(kps, l_a, l_counts), feats.gather_track_rows(kps, l_b, l_counts)
        p_R = p_t = p_stats = p_sigma = p_points = None
        if pose is not None:
            intr = torch.tensor([[pose[0], pose[0], pose[1], pose[2]]], dtype=torch.float32, device=dev).repeat(n, 1)
            p_R, p_t, p_stats, p_sigma, p_points = feats.two_view_pose(model.contiguous(), intr, kps, (ea, eb), (l_off, l_a, l_b))
        vg_rot = vg_es = vg_res = vg_ims = vg_counts = vg_match = None
        links_for_tracks = ver if l_kept is None else l_kept
        if view_graph is not None:
            if pose is None:
                raise RuntimeError("match_collection: view_graph needs pose (the edges' relative rotations)")
            vg_rot, vg_es, vg_res, vg_ims, vg_counts, vg_match = feats.view_graph((ea, eb), p_R, p_stats, n, max_loop_deg=view_graph,
                                                                                  layout=la, match=links_for_tracks)
            links_for_tracks = vg_match
        track = track_len = track_dup = track_counts = None
        t_off = t_rows = t_img = t_row_track = t_counts = t_kps = None
        if global_sweeps and view_graph is None:
            raise RuntimeError("match_collection: global_sweeps needs view_graph (the images' global rotations and the tree)")
        if (register or bundle or global_sweeps) and triangulate is None:
            triangulate = True
        if tracks or table or expand or triangulate is not None:
            track, track_len, track_dup = feats.build_tracks(o, ea, eb, la, links_for_tracks, capacity=cap_a, n_rows=m)
            two, three, ok = track_len >= 2, track_len >= 3, track_dup == 0
            track_counts = torch.stack([two.sum(), (two & ok).sum(), three.sum(), (three & ok).sum(), track_len.max().long(),
                                        (track_len * (two & ok)).sum()])
        if table or expand or triangulate is not None:
            t_off, t_rows, t_img, t_row_track, t_counts = feats.track_table(track, track_len, track_dup, image_offsets=o, min_len=2,
                                                                            consistent=True)
            t_kps = feats.gather_track_rows(kps, t_rows, t_counts)
        covis = x_ea = x_eb = x_counts = x_la = x_ver = x_per_edge = first = None
        if expand:
            first = dict(track_counts=track_counts, table_offsets=t_off, table_rows=t_rows, table_images=t_img,
                         table_row_track=t_row_track, table_counts=t_counts, table_keypoints=t_kps)
            # the tracks two images share, the pairs already matched zeroed: what is left was never tried
            covis = feats.covisibility(t_off, t_img, t_counts, n, edges=(ea, eb))
            x_ea, x_eb, _, _, _, x_counts = feats.select_edges(covis, expand, min_votes=min_shared, skip_self=True, unique=True,
                                                               capacity=n * expand)
            x_edges = int(x_ea.numel())
            cap_x = (n - 1) * m                                 # (smaller, larger): an image meets every other one at most once
            x_ab, _, _, _, x_la, x_lb = feats.match_q8_edges(q, o, q, o, x_ea, x_eb, ratio=ratio, mutual=True, capacity_a=cap_x,
                                                             capacity_b=cap_x)
            x_ka = feats.gather_edge_rows(kps, o, x_ea, x_la, capacity=cap_x)
            x_kb = feats.gather_edge_rows(kps, o, x_eb, x_lb, capacity=cap_x)
            _, x_ver, _ = verify(x_ka, x_la, x_kb, x_lb, x_ab, seed=seed)
            x_edge_of = torch.searchsorted(x_la, torch.arange(cap_x, device=dev), right=True) - 1
            x_count = lambda mask: torch.bincount(x_edge_of[mask], minlength=x_edges + 1)[:x_edges]
            x_per_edge = torch.stack([x_count(x_ab >= 0), x_count(x_ver >= 0)], dim=1)
            x_links = x_ver
            if min_inliers is not None:
                x_links = feats.link_table(o, x_ea, x_eb, x_la, x_ver, min_links=min_inliers, capacity=cap_x, n_rows=m,
                                           kept_match=True)[5]
            track, track_len, track_dup = feats.build_tracks(o, x_ea, x_eb, x_la, x_links, capacity=cap_x, into=track)
            two, three, ok = track_len >= 2, track_len >= 3, track_dup == 0
            track_counts = torch.stack([two.sum(), (two & ok).sum(), three.sum(), (three & ok).sum(), track_len.max().long(),
                                        (track_len * (two & ok)).sum()])
            t_off, t_rows, t_img, t_row_track, t_counts = feats.track_table(track, track_len, track_dup, image_offsets=o, min_len=2,
                                                                            consistent=True)
            t_kps = feats.gather_track_rows(kps, t_rows, t_counts)
        tri_poses = tri_points = tri_stats = tri_err = tri_state = None
        register_rounds = [] if register else None       # (None without `register`, like every output that was not asked for)
        bundle_trace = bundle_counts = bundle_state = bundle_rms = bundle_groups = None
        gp_points = gp_state = gp_ims = gp_counts = None
        if triangulate is not None and triangulate is not False:
            if pose is None:
                raise RuntimeError("match_collection: triangulate needs pose (the cameras' intrinsics)")
            if global_sweeps:
                # the global route: no initial pair and no rounds -- the view graph's rotations, unit steps along its tree,
                # then every centre and every point at once, in place on the pose array
                tri_poses = feats.tree_poses((ea, eb), p_t, vg_rot, vg_ims)
                tri_poses, gp_points, gp_state, gp_ims, _, gp_counts = feats.global_positions(
                    kps, o, (t_off, t_rows, t_img, t_row_track, t_counts), intr, tri_poses, sweeps=global_sweeps, out_poses=tri_poses)
            elif triangulate is True:
                # the initial pair, chosen on the device: nothing is read back
                with_pose = torch.where(p_stats[:, 2] >= 0, p_stats[:, 3], torch.full_like(p_stats[:, 3], -1))
                if vg_es is not None:                           # ... among the edges the view graph supports
                    with_pose = torch.where(vg_es[:, 2] == 3, with_pose, torch.full_like(with_pose, -1))
                e = torch.argmax(with_pose).reshape(1)
                eye = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32, device=dev)
                tri_poses = torch.zeros((n, 12), dtype=torch.float32, device=dev)
                tri_poses.index_copy_(0, ea[e].long(), eye)
                tri_poses.index_copy_(0, eb[e].long(), torch.cat([p_R[e].reshape(1, 9), p_t[e].reshape(1, 3)], 1))
            else:
                tri_poses = torch.as_tensor(np.ascontiguousarray(triangulate, np.float32).reshape(n, 12), device=dev)
            tri_points, tri_stats, tri_err, tri_state = feats.triangulate_tracks(kps, (t_off, t_rows, t_img, t_counts), intr, tri_poses)
            held = (tri_poses[:, :9] != 0).any(1).to(torch.int32)
            if global_sweeps:
                # every image has a pose: the two with the most weighted rows hold the bundle's gauge
                held = torch.zeros_like(held).index_fill_(0, torch.topk(gp_ims[:, 1], min(2, n)).indices, 1)
            for _ in range(register or 0):
                # the images without a pose from the points there are, in place; then the points under every pose there is
                _, r_stats, _, _ = feats.resect_cameras(kps, o, t_row_track, tri_points, t_counts, intr, tri_poses, seed=seed,
                                                        out=tri_poses)
                tri_points, tri_stats, tri_err, tri_state = feats.triangulate_tracks(kps, (t_off, t_rows, t_img, t_counts), intr,
                                                                                     tri_poses)
                register_rounds.append((r_stats, tri_stats))
            if bundle:
                # poses and points jointly, in place; the images that had a pose before the rounds hold theirs (the gauge)
                before = (tri_poses.clone(), tri_points.clone(), intr.clone())
                if refine_focal or refine_principal:
                    # ... and the one lens all the images share, in place too
                    tri_poses, tri_points, intr, bundle_groups, bundle_state, bundle_trace, bundle_counts = feats.bundle_adjust_intrinsics(
                        kps, o, (t_off, t_rows, t_img, t_counts), tri_points, intr, tri_poses, obs_state=tri_state, camera_fixed=held,
                        refine_focal=refine_focal, refine_principal=refine_principal, iterations=bundle, out_poses=tri_poses,
                        out_points=tri_points, out_intrinsics=intr)
                else:
                    tri_poses, tri_points, bundle_state, bundle_trace, bundle_counts = feats.bundle_adjust(
                        kps, o, (t_off, t_rows, t_img, t_counts), tri_points, intr, tri_poses, obs_state=tri_state, camera_fixed=held,
                        iterations=bundle, out_poses=tri_poses, out_points=tri_points)
                active = bundle_state >= 1
                bundle_rms = torch.stack([reprojection_rms(kps, t_off, t_rows, t_img, K, P, X, active) for P, X, K in
                                          (before, (tri_poses, tri_points, intr))])
    return dict(gp_points=gp_points, gp_obs_state=gp_state, gp_image_stats=gp_ims, gp_counts=gp_counts, bundle_groups=bundle_groups, intrinsics=intr if pose is not None else None, bundle_trace=bundle_trace, bundle_counts=bundle_counts, bundle_obs_state=bundle_state, bundle_rms=bundle_rms,
                register_rounds=register_rounds, tri_poses=tri_poses, tri_points=tri_points, tri_stats=tri_stats, tri_err=tri_err, tri_obs_state=tri_state,
                edge_a=ea, edge_b=eb, offsets=o, keypoints=kps, q8=q, layout_a=la, layout_b=lb, match=m_ab, verified=ver, model=model,
                stats=stats, per_edge=per_edge, track=track, track_len=track_len, track_dup=track_dup, track_counts=track_counts,
                table_offsets=t_off, table_rows=t_rows, table_images=t_img, table_row_track=t_row_track, table_counts=t_counts,
                table_keypoints=t_kps, link_offsets=l_off, link_a=l_a, link_b=l_b, link_edge=l_edge, edge_links=l_links,
                link_counts=l_counts, link_keypoints_a=l_ka, link_keypoints_b=l_kb, match_kept=l_kept, votes=votes,
                edge_votes=e_votes, rank=rank, rank_votes=rank_votes, select_counts=s_counts, covisibility=covis,
                expand_edge_a=x_ea, expand_edge_b=x_eb, expand_counts=x_counts, expand_layout_a=x_la, expand_verified=x_ver,
                expand_per_edge=x_per_edge, first_round=first, pose_R=p_R, pose_t=p_t, pose_stats=p_stats,
                pose_sigma=p_sigma, pose_points=p_points, vg_rotations=vg_rot, vg_edge_stats=vg_es, vg_residual=vg_res,
                vg_image_stats=vg_ims, vg_counts=vg_counts, vg_match=vg_match)


def reprojection_rms(kps, t_off, t_rows, t_img, intr, poses, points, active, max_reproj_px=4.0):
    """the rms reprojection error (px) of the observations in `active` that are inliers at max_reproj_px, on the device"""
    import torch
    n_obs = t_rows.numel()
    track = torch.searchsorted(t_off[1:].contiguous(), torch.arange(n_obs, device=t_off.device), right=True).clamp_(max=points.shape[0] - 1)
    at = torch.nonzero(active).reshape(-1)
    img, row, X = t_img[at].long(), t_rows[at].long(), points[track[at], :3].double()
    P = poses[img].double()
    p = torch.einsum("nij,nj->ni", P[:, :9].reshape(-1, 3, 3), X) + P[:, 9:]
    K = intr[img].double()
    e = K[:, :2] * p[:, :2] / p[:, 2:3] + K[:, 2:] - kps[row, :2].double()
    e2 = (e * e).sum(1)
    inl = (p[:, 2] > 0) & (e2 <= max_reproj_px * max_reproj_px)
    return torch.sqrt((e2 * inl).sum() / inl.sum().clamp(min=1))


def bundle_lines(out):
    """one line per Levenberg-Marquardt iteration of `bundle`, then the rms before and after"""
    if out["bundle_trace"] is None:
        return []
    free_c, free_p, active, accepted = out["bundle_counts"].cpu().tolist()[:4]
    lines = [f"{free_c} free cameras, {free_p} free points, {active} active observations, {accepted} steps accepted"]
    for k, (cost, new, lam, ok, steps, inl, hc, hp, *hg) in enumerate(out["bundle_trace"].cpu().tolist()):
        lines.append(f"iteration {k + 1}: cost {cost:.1f} -> {new:.1f} at lambda {lam:.2e}, {'accepted' if ok else 'rejected'}, "
                     f"{int(steps)} CG steps, {int(inl)} inliers, {int(hc)} cameras and {int(hp)} points held"
                     + (f", {int(hg[0])} lenses held" if hg else ""))
    if out.get("bundle_groups") is not None:
        (s, dx, dy), K = out["bundle_groups"].cpu().tolist()[0], out["intrinsics"].cpu().tolist()[0]
        lines.append(f"refined focal {K[0]:.2f} (x {s:.5f}), principal point ({K[2]:.2f}, {K[3]:.2f}) (moved by ({dx:.2f}, {dy:.2f}))")
    before, after = out["bundle_rms"].cpu().tolist()
    lines.append(f"rms reprojection error {before:.3f} px -> {after:.3f} px")
    return lines


def view_graph_lines(out):
    """one line of `view_graph`'s counts"""
    if out.get("vg_counts") is None:
        return []
    usable, supported, rejected, unchecked, kept, labelled, root = out["vg_counts"].cpu().tolist()[:7]
    return [f"{usable} usable edges: {supported} supported, {rejected} rejected, {unchecked} unchecked, {kept} kept; "
            f"{labelled} of {out['vg_image_stats'].shape[0]} images with a rotation, root {root + 1}"]


def global_lines(out):
    """one line of `global_sweeps`' counts"""
    if out.get("gp_counts") is None:
        return []
    reg, solved, usable, weighted, held, failed, tracks, sweeps = out["gp_counts"].cpu().tolist()
    return [f"global positions, {sweeps} sweeps: {reg} images, {solved} of {tracks} points solved, {weighted} of {usable} observations "
            f"weighted at least 1/2, {held} cameras held in the last sweep"]


def register_lines(out):
    """one line per round of `register`: the images registered after it, those it added, and the points"""
    n_tracks = out["table_counts"].cpu().tolist()[0]
    lines, registered = [], None
    for k, (r_stats, t_stats) in enumerate(out["register_rounds"] or []):
        reason = r_stats[:, 2].cpu().numpy()
        if registered is None:
            registered = int((reason == 1).sum())
        added = int((reason == 0).sum())
        registered += added
        points = int((t_stats[:n_tracks, 2].cpu().numpy() == 0).sum())
        lines.append(f"round {k + 1}: {registered} of {len(reason)} images registered ({added} added), {points} points")
    return lines


def parse_pose(text):
    """FOCAL or FOCAL,CX,CY -> (focal, cx, cy), cx and cy None if not given; None if the text is neither."""
    try:
        v = [float(x) for x in text.split(",")]
    except ValueError:
        return None
    if len(v) not in (1, 3) or not v[0] > 0:
        return None
    return (v[0], v[1], v[2]) if len(v) == 3 else (v[0], None, None)


def main():
    args = sys.argv[1:]
    mode, arg, fundamental, tracks, table, pairs, min_inliers, paths = "window", 2, False, False, False, False, None, []
    expand, min_shared, pose, triangulate, register, bundle = None, 8, None, None, 0, 0
    refine_focal = refine_principal = False
    view_graph, global_sweeps = None, 0
    while args:
        a = args.pop(0)
        if a == "--fundamental":
            fundamental = True
        elif a == "--tracks":
            tracks = True
        elif a == "--table":
            tracks = table = True
        elif a == "--pairs":
            pairs = True
        elif a == "--min-inliers" and args and args[0].isdigit():
            min_inliers = int(args.pop(0))
        elif a == "--expand" and args and args[0].isdigit() and int(args[0]) > 0:
            tracks = table = True
            expand = int(args.pop(0))
        elif a == "--min-shared" and args and args[0].isdigit():
            min_shared = int(args.pop(0))
        elif a == "--pose" and args and parse_pose(args[0]) is not None:
            pose = parse_pose(args.pop(0))
            fundamental = pairs = True
        elif a == "--view-graph" and args and parse_pose(args[0]) is not None and "," not in args[0] and float(args[0]) <= 180:
            view_graph = float(args.pop(0))
        elif a == "--triangulate":
            tracks = table = True
            triangulate = np.load(args.pop(0)) if args and args[0].endswith(".npy") else True
        elif a == "--global" and args and args[0].isdigit() and 0 < int(args[0]) <= 4096:
            tracks = table = True
            global_sweeps = int(args.pop(0))
            triangulate = True if triangulate is None else triangulate
        elif a == "--register" and args and args[0].isdigit() and int(args[0]) > 0:
            tracks = table = True
            register = int(args.pop(0))
            triangulate = True if triangulate is None else triangulate
        elif a == "--bundle" and args and args[0].isdigit() and 0 < int(args[0]) <= 64:
            tracks = table = True
            bundle = int(args.pop(0))
            triangulate = True if triangulate is None else triangulate
        elif a == "--refine-focal":
            refine_focal = True
        elif a == "--refine-principal":
            refine_principal = True
        elif a == "--all":
            mode = "all"
        elif a in ("--window", "--retrieve", "--select") and args and args[0].isdigit() and int(args[0]) > 0:
            mode, arg = a[2:], int(args.pop(0))
        elif a.startswith("--"):
            paths = []
            break
        else:
            paths.append(a)
    if len(paths) < 2 or (triangulate is not None and pose is None) or (view_graph is not None and pose is None) or (global_sweeps and view_graph is None) or ((refine_focal or refine_principal) and not bundle) or (mode in ("retrieve", "select") and arg > len(paths) - 1) or (expand or 0) > min(len(paths) - 1, 32):
        print("Required arguments: [--window W | --all | --retrieve K | --select K] [--fundamental] [--tracks] [--table] [--pairs] [--min-inliers M] [--expand K [--min-shared M]] [--pose FOCAL[,CX,CY]] [--view-graph DEG] [--global SWEEPS] [--triangulate [POSES.npy]] [--register ROUNDS] [--bundle ITERS [--refine-focal] [--refine-principal]] IMAGE_1 IMAGE_2 [IMAGE_3 ...]  (K "
              "below "
              "the "
              "number of images; --view-graph, --triangulate, --register and --bundle need --pose, --global --pose and --view-graph, --refine-focal and --refine-principal --bundle)", file=sys.stderr)
        return 1
    imgs = [load_gray(p) for p in paths]
    if any(i.shape != imgs[0].shape for i in imgs):
        print("the images must have one size", file=sys.stderr)
        return 1
    if pose is not None and pose[1] is None:                    # the principal point: the middle of the frame
        pose = (pose[0], imgs[0].shape[1] / 2.0, imgs[0].shape[0] / 2.0)
    out = match_collection(np.stack(imgs), mode, arg, fundamental=fundamental, tracks=tracks, table=table, pairs=pairs,
                           min_inliers=min_inliers, expand=expand, min_shared=min_shared, pose=pose, triangulate=triangulate, register=register, bundle=bundle,
                           refine_focal=refine_focal, refine_principal=refine_principal, view_graph=view_graph, global_sweeps=global_sweeps)
    ea, eb, o, per_edge = (out[k].cpu().tolist() for k in ("edge_a", "edge_b", "offsets", "per_edge"))
    if mode == "select":                                        # the entries behind the edges name no image
        kept = out["select_counts"].cpu().tolist()[0]
        ea, eb, per_edge = ea[:kept], eb[:kept], per_edge[:kept]
    print("Extracted " + ", ".join(str(o[t + 1] - o[t]) for t in range(len(imgs))) + " keypoints")
    what = "one epipolar geometry" if fundamental else "one homography"
    for e in sorted(range(len(ea)), key=lambda e: (-per_edge[e][2], e)):
        raw, mutual, inl = per_edge[e]
        print(f"Edge {ea[e] + 1} -> {eb[e] + 1}: {raw} matches, {mutual} mutual, {inl} agree with {what}")

    def track_lines(r):
        if tracks:
            n2, c2, n3, c3, longest, inside = r["track_counts"].cpu().tolist()
            print(f"Tracks: {n2} of length >= 2 ({c2} consistent), {n3} of length >= 3 ({c3} consistent)")
            print(f"Longest track: {longest} keypoints; {100.0 * inside / max(o[-1], 1):.1f} % of the keypoints sit in a consistent track "
                  "of length >= 2")
        if table:
            n_tracks, n_obs = r["table_counts"].cpu().tolist()[:2]
            print(f"Track table: {n_tracks} tracks, {n_obs} observations (consistent, length >= 2)")
            first = r["table_offsets"][:min(n_tracks, 3) + 1].cpu().tolist()
            images, xy = r["table_images"][:first[-1]].cpu().tolist(), r["table_keypoints"][:first[-1], :2].cpu().tolist()
            for k in range(len(first) - 1):
                print(f"Track {k + 1}: " + " ".join(f"{images[i] + 1}:{xy[i][0]:.1f},{xy[i][1]:.1f}" for i in range(first[k], first[k + 1])))

    track_lines(out["first_round"] if expand else out)
    if pairs:
        n_kept, n_links = out["link_counts"].cpu().tolist()[:2]
        print(f"Link table: {n_kept} edges, {n_links} correspondences")
        best = min(range(len(ea)), key=lambda e: (-per_edge[e][2], e))
        lo, hi = out["link_offsets"][best:best + 2].cpu().tolist()
        hi = min(hi, lo + 3)
        xa, xb = out["link_keypoints_a"][lo:hi, :2].cpu().tolist(), out["link_keypoints_b"][lo:hi, :2].cpu().tolist()
        for a, b in zip(xa, xb):
            print(f"Edge {ea[best] + 1} -> {eb[best] + 1}: {a[0]:.1f},{a[1]:.1f} -> {b[0]:.1f},{b[1]:.1f}")
    if pose is not None:
        R, t, st, sg = (out[k].cpu().numpy() for k in ("pose_R", "pose_t", "pose_stats", "pose_sigma"))
        links = out["edge_links"].cpu().tolist()
        for e in sorted(range(len(ea)), key=lambda e: (-per_edge[e][2], e)):
            if st[e][2] < 0:
                print(f"Pose {ea[e] + 1} -> {eb[e] + 1}: none")
                continue
            angle = np.degrees(np.arccos(np.clip((np.trace(R[e].astype(np.float64)) - 1) / 2, -1, 1)))
            print(f"Pose {ea[e] + 1} -> {eb[e] + 1}: rotation {angle:.2f} deg, t {t[e][0]:+.3f} {t[e][1]:+.3f} {t[e][2]:+.3f}, "
                  f"{st[e][0]} / {links[e]} links in front, {st[e][3]} with parallax, s2/s1 {sg[e][1]:.3f}")
    for line in view_graph_lines(out):
        print("View graph, " + line)
    if triangulate is not None:
        n_tracks = out["table_counts"].cpu().tolist()[0]
        st, pts = out["tri_stats"][:n_tracks].cpu().numpy(), out["tri_points"][:n_tracks].cpu().numpy()
        have = st[:, 2] == 0
        registered = int((out["tri_poses"][:, :9] != 0).any(1).sum())
        median = np.degrees(np.arccos(np.clip(np.median(pts[have, 3]), -1, 1))) if have.any() else 0.0
        print(f"Triangulated: {n_tracks} tracks under {registered} registered images, {int(have.sum())} points, "
              f"{int(st[have, 1].sum())} inlier observations, median parallax {median:.2f} deg")
        for line in global_lines(out):
            print(line)
        for line in register_lines(out):
            print("Registered, " + line)
        for line in bundle_lines(out):
            print("Bundle adjustment, " + line)
    if expand:
        proposed = out["expand_counts"].cpu().tolist()[0]
        kept = int((out["expand_per_edge"][:proposed, 1] > 0).sum())
        print(f"Expanded: {proposed} edges proposed from the tracks two unmatched images share (at least {min_shared}), "
              f"{kept} of them with verified matches")
        track_lines(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
