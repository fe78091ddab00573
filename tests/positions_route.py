"""The global route on the collection of tests/reconstruction_cases.py, composed on the host: what follows the two-view poses of
the chain (reconstruction_cases.run_chain gives the verifier, the link table, the poses, the tracks and the track table) is
view graph -> tree poses -> global positions -> triangulation -> bundle adjustment, every stage through its twin's driver on
the previous stage's output words.  `numpy_route` composes the float64 restatements of the three new stages the same way, for
the truth bounds.  There is no arithmetic here."""
import numpy as np

import positions_cases
import positions_twin as pt
import reconstruction_cases as cases
import view_graph_cases
import view_graph_twin as vgt

HELD = (0, 1)                      # the two cameras that hold the bundle's gauge


def graph_scene(s, pose):
    n = len(s["offsets"]) - 1
    return dict(n_images=n, edge_a=s["edge_a"].astype(np.uint32), edge_b=s["edge_b"].astype(np.uint32),
                R=cases.f32(pose["R"]).reshape(-1, 9), pose_stats=np.asarray(pose["stats"], np.uint32).reshape(-1, 4))


def tree_scene(s, pose, rotations, image_stats):
    return dict(edge_a=s["edge_a"].astype(np.uint32), edge_b=s["edge_b"].astype(np.uint32), t=cases.f32(pose["t"]).reshape(-1, 3),
                rotations=np.asarray(rotations, np.float32).reshape(-1, 9), image_stats=np.asarray(image_stats, np.uint32).reshape(-1, 4))


def positions_scene(s, K, tt, poses):
    return dict(kps=s["kps"], image_offsets=s["offsets"].astype(np.uint64), track_offsets=np.asarray(tt.offsets, np.uint64),
                obs_row=tt.obs_row, obs_image=tt.obs_image, counts=np.array(tt.counts[:2], np.uint32), row_track=tt.row_track,
                intrinsics=K, poses=np.asarray(poses, np.float32).reshape(-1, 12))


def twin_route(twins, exe_vg, exe_gp, tmp, s, K, ch):
    """ch: the host chain of reconstruction_twin.run (its stages up to the track table are used) -> the new stages' words"""
    p, tt = ch["params"], ch["table"]
    vg = vgt.run(exe_vg, tmp, graph_scene(s, ch["pose"]), match=False)
    tree = pt.run_tree(exe_gp, tmp, tree_scene(s, ch["pose"], cases.f32(vg["rotations"]), vg["image_stats"]))
    sc = positions_scene(s, K, tt, cases.f32(tree))
    gp = pt.run(exe_gp, tmp, sc, trace=False)
    poses = cases.f32(gp["poses"]).reshape(-1, 12)
    tri = twins.triangulate(dict(kps=sc["kps"], track_offsets=sc["track_offsets"], obs_row=sc["obs_row"], obs_image=sc["obs_image"],
                                 counts=sc["counts"], intrinsics=K, poses=poses), p["px"], p["tri_rounds"])
    held = np.zeros(len(K), np.uint32)
    held[list(HELD)] = 1
    b = twins.bundle(dict(sc, points=cases.f32(tri["points"]), poses=poses, obs_state=tri["obs_state"], camera_fixed=held), px=p["px"],
                     lambda0=p["lambda0"], iterations=p["iterations"], cg_iterations=p["cg_iterations"], cg_tol=p["cg_tol"])
    return dict(view_graph=vg, tree=tree, positions=gp, tri=tri, bundle=b)


def numpy_route(s, K, ch):
    """the three new stages as their float64 restatements compute them, on the same pose words, then the triangulation and the bundle as
    reconstruction_cases.Reference composes them -> dict(positions, tri, bundle)"""
    vg = view_graph_cases.reference(graph_scene(s, ch["pose"]), match=False)
    rot = np.asarray(vg["rotations"], np.float32).reshape(-1, 9)
    tree = positions_cases.tree_reference(tree_scene(s, ch["pose"], rot, np.asarray(vg["image_stats"]).astype(np.int64) & 0xFFFFFFFF))
    sc = positions_scene(s, K, ch["table"], tree)
    gp = positions_cases.reference(sc, **pt.DEFAULTS)
    p, ref = ch["params"], cases.Reference()
    tri = ref.triangulate(dict(kps=sc["kps"], track_offsets=sc["track_offsets"], obs_row=sc["obs_row"], obs_image=sc["obs_image"],
                               counts=sc["counts"], intrinsics=K, poses=gp["poses"]), p["px"], p["tri_rounds"])
    held = np.zeros(len(K), np.uint32)
    held[list(HELD)] = 1
    b = ref.bundle(dict(sc, points=cases.f32(tri["points"]), poses=gp["poses"], obs_state=tri["obs_state"], camera_fixed=held), px=p["px"],
                   lambda0=p["lambda0"], iterations=p["iterations"], cg_iterations=p["cg_iterations"], cg_tol=p["cg_tol"])
    return dict(positions=gp, tri=tri, bundle=b)


def centre_error(s, poses):
    """the largest centre distance of the registered images from the truth after a similarity fit, in units of the rms radius"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    reg = (P[:, :9] != 0).any(1)
    truth = s["truth_poses"]
    tc = -np.einsum("nji,nj->ni", truth[:, :9].reshape(-1, 3, 3), truth[:, 9:])
    return positions_cases.similarity_error(positions_cases.centres_of(P[reg]), tc[reg]), int(reg.sum())
