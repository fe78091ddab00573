"""examples/localize_images.py on the GPU: a model from three of the example's frames through match_collection's route, its
descriptors by one call, saved and loaded again, two photographs localised against it.  The frames are warps of one picture,
so the geometry means little; this is about the plumbing, and the matches are held to numpy's matcher over the saved rows."""
import os
import sys

import numpy as np
import pytest

import q8_cases

import local_features_python as lfp

pytestmark = pytest.mark.gpu


def test_a_model_is_built_saved_loaded_and_queried(tmp_path):
    import torch
    from conftest import ROOT
    from test_gpu_covisibility import _frames
    sys.path.insert(0, os.path.join(ROOT, "local-features_amd", "examples"))
    import localize_images as ex
    frames = np.stack([np.asarray(f, np.float32) / 255.0 for f in _frames()])
    feats = lfp.LocalFeatures(1024, 768, 3000, max_blobs=8000, n_scales=5, pca="liberty", pool_mode=lfp.POOL_F16X3, max_frames=3)
    pose = (800.0, 512.0, 384.0)
    built, out = ex.build_model(frames[:3], pose, register=2, bundle=0, seed=21, feats=feats)
    model = ex.describe_model(feats, built)
    torch.cuda.synchronize()
    T, tcap = int(model["counts"][0]), model["model_desc"].shape[0]
    desc, stats, points = model["model_desc"].cpu().numpy(), model["desc_stats"].cpu().numpy(), model["points"].cpu().numpy()
    assert desc.shape == (tcap, 128) and stats.shape == (tcap, 2) and 0 < T <= tcap
    zero = (desc == 128).all(1)
    assert (zero[T:]).all() and (stats[T:] == [0, -2 ** 31]).all()
    assert (zero[:T] | (points[:T, 3] < 1.5)).all()                       # a row only where there is a point
    assert ((stats[:T, 1] == -2 ** 31) == zero[:T]).all() and (stats[:T][~zero[:T], 0] >= 2).all()
    path = str(tmp_path / "model.npz")
    ex.save_model(path, model)
    loaded = ex.load_model(path, torch.device("cuda", feats.device))
    assert all(loaded[k].cpu().numpy().tobytes() == model[k].cpu().numpy().tobytes() for k in ("model_desc", "points", "counts"))
    assert (points[T:] == [0, 0, 0, 2]).all()
    poses, st, err, row_state, row_track, offsets = ex.localize_images(feats, loaded, [frames[1], frames[3]], pose)
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert poses.shape == (2, 12) and st.shape == (2, 4) and set(st[:, 2].tolist()) <= {0, 2, 3}
    assert row_track.shape[0] == offsets[-1] == row_state.shape[0]
    # the rows matched are numpy's over the saved model
    k, d = feats.detect_top_n(frames[1], 2000, 0.0)
    want, _, _ = q8_cases.match_q8(feats.quantize(d), desc, 0.8)
    assert np.array_equal(row_track.cpu().numpy()[:offsets[1]], want)
    lines = ex.pose_lines(["a", "b"], poses, torch.from_numpy(st), err)
    assert len(lines) == 2 and lines[0].startswith("a: ") and lines[1].startswith("b: ")
