"""The global route on the GPU, stage after stage on what the stage before left on the device, through the LocalFeatures
wrappers: verifier -> link table -> two-view poses -> view graph -> tree poses -> tracks and track table -> global positions
in place -> triangulation -> bundle adjustment, against the same route composed from the twins (tests/positions_route.py) word
for word, and against the truth under the bounds of tests/test_positions_route.py."""
import numpy as np
import pytest

import positions_route as route
import positions_twin as pt
import reconstruction_cases as cases
import reconstruction_twin as rtwin
import view_graph_twin as vgt
from test_gpu_reconstruction import device_chain, words
from test_positions_route import BOUND

import local_features_python as lfp

pytestmark = pytest.mark.gpu


def test_the_global_route_equals_the_twins_route_word_for_word(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    tmp = tmp_path_factory.mktemp("positions_route")
    twins, exe_vg, exe_gp = rtwin.Twins(tmp), vgt.build(tmp), pt.build(tmp)
    s, p = cases.scene(), cases.PARAMS
    K = cases.intrinsics(s)
    ch = rtwin.run(twins, s, K)
    want = route.twin_route(twins, exe_vg, exe_gp, tmp, s, K, ch)

    lf = lfp.LocalFeatures(64, 64, 16)
    d = device_chain(torch, lf, s, K, focal=False)                 # (its stages up to the track table are used)
    pool, off, ea, eb = d["keep"][:4]
    p_R, p_t, p_stats = d["pose"][:3]
    t_off, t_rows, t_img, t_row_track, t_counts = d["table"]
    intr = torch.from_numpy(K).cuda()
    n = len(K)
    rot, _, _, v_ims, v_counts, _ = lf.view_graph((ea, eb), p_R.contiguous(), p_stats, n)
    tree = lf.tree_poses((ea, eb), p_t.contiguous(), rot, v_ims)
    poses = tree.clone()
    g_poses, g_points, g_state, g_ims, _, g_counts = lf.global_positions(pool, off, d["table"], intr, poses, out_poses=poses)
    assert g_poses.data_ptr() == poses.data_ptr()
    tri = lf.triangulate_tracks(pool, (t_off, t_rows, t_img, t_counts), intr, poses, p["px"], p["tri_rounds"])
    held = torch.zeros(n, dtype=torch.int32, device="cuda")
    held[list(route.HELD)] = 1
    b_poses, b_points, b_state, b_trace, b_counts = lf.bundle_adjust(
        pool, off, (t_off, t_rows, t_img, t_counts), tri[0], intr, poses.clone(), obs_state=tri[3], camera_fixed=held, max_reproj_px=p["px"],
        lambda0=p["lambda0"], iterations=p["iterations"], cg_iterations=p["cg_iterations"], cg_tol=p["cg_tol"])
    torch.cuda.synchronize()

    T, O = (int(v) for v in words(t_counts)[:2])
    w, u = want, cases.u32
    pairs = [("view_graph rotations", words(rot).reshape(n, 9), w["view_graph"]["rotations"]),
             ("view_graph image_stats", words(v_ims), w["view_graph"]["image_stats"]), ("view_graph counts", words(v_counts), w["view_graph"]["counts"]),
             ("tree poses", words(tree), w["tree"]), ("positions poses", words(g_poses), w["positions"]["poses"]),
             ("positions points", words(g_points)[:T], w["positions"]["points"][:T]),
             ("positions obs_state", words(g_state)[:O], w["positions"]["obs_state"][:O]),
             ("positions image_stats", words(g_ims), w["positions"]["image_stats"]), ("positions counts", words(g_counts), w["positions"]["counts"]),
             ("triangulate points", words(tri[0])[:T], w["tri"]["points"][:T]), ("triangulate stats", words(tri[1])[:T], w["tri"]["stats"][:T]),
             ("triangulate obs_state", words(tri[3])[:O], w["tri"]["obs_state"][:O]),
             ("bundle poses", words(b_poses), w["bundle"]["poses"]), ("bundle points", words(b_points)[:T], w["bundle"]["points"][:T]),
             ("bundle obs_state", words(b_state)[:O], w["bundle"]["obs_state"][:O]), ("bundle counts", words(b_counts), w["bundle"]["counts"]),
             ("bundle trace", words(b_trace).reshape(-1), np.asarray(w["bundle"]["trace_words"]).reshape(-1))]
    for name, got, expect in pairs:
        got, expect = np.asarray(got).reshape(-1), u(np.asarray(expect)).reshape(-1) if np.asarray(expect).dtype.itemsize == 4 else np.asarray(expect).reshape(-1)
        assert got.shape == expect.shape, (name, got.shape, expect.shape)
        bad = np.flatnonzero(got != expect)
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), [hex(int(got[b])) for b in bad[:5]], [hex(int(expect[b])) for b in bad[:5]])
    for stage, x in (("positions", g_poses), ("bundle", b_poses)):
        err, registered = route.centre_error(s, x.cpu().numpy())
        assert registered == cases.N_IMAGES and err <= BOUND[stage], (stage, err)
