"""RANSAC homography verification on the GPU (lf_mkd_verify_homography*) against the numpy restatement
(tests/homography_ref.py): the same hypotheses and counts, the same refit, batched = single, bit-stable and capturable,
and end to end on real photographs."""
import os

import numpy as np
import pytest

import homography_ref as ref
from homography_cases import CORNERS, H_TRUE, THR, band, planted
from homography_cases import pairs as _pairs
from conftest import GOLDEN

import local_features_python as lfp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


@pytest.mark.parametrize("m,n_hyp", [(4, 256), (50, 2048), (1000, 2048), (20000, 256)])
@pytest.mark.parametrize("frac", [0.1, 0.5, 0.9])
def test_hypotheses_match_the_restatement(handle, m, n_hyp, frac):
    ka, kb, mt = planted(m, frac, seed=m + int(frac * 10))
    H, ver, st = handle.verify_homography(ka, kb, mt, n_hyp, THR, 11, lfp.VERIFY_NO_REFINE)
    prob = ref.Problem(ka, kb, mt)
    counts, hs = ref.score_all(prob, 11, n_hyp, THR)
    assert st[3] == m
    if counts.max() < 0:
        assert st[2] == ref.INVALID and st[0] == 0 and (H == 0).all() and (ver == -1).all()
        return
    k = int(st[2])
    assert k < n_hyp and counts[k] >= 0, (k, counts[k] if k < n_hyp else None)
    slack_k = int(band(prob, hs[k]).sum())
    assert abs(int(st[1]) - counts[k]) <= slack_k, (st, counts[k], slack_k)
    k_ref = int(np.argmax(counts))
    slack_ref = int(band(prob, hs[k_ref]).sum())
    if k != k_ref:   # only a near tie may choose another hypothesis
        assert counts[k_ref] - counts[k] <= slack_ref + slack_k, (k, k_ref, counts[k], counts[k_ref])
    # without the refit the result is the best hypothesis itself
    assert st[0] == st[1] and (ver >= 0).sum() == st[0]
    mask = prob.inliers(hs[k], THR)
    diff = (ver[prob.rows] >= 0) != mask
    assert not (diff & ~band(prob, hs[k])).any()
    # the same map: within 0.05 px on the corners, relative 1e-5 where a wild hypothesis sends a corner far away
    got, want = ref.map_points(H, CORNERS), ref.map_points(hs[k], CORNERS)
    assert (np.abs(got - want) < 0.05 + 1e-5 * np.abs(want)).all(), (got, want)


@pytest.mark.parametrize("m,frac", [(50, 0.5), (1000, 0.3), (1000, 0.8), (20000, 0.5)])
def test_refit_matches_the_restatement(handle, m, frac):
    ka, kb, mt = planted(m, frac, seed=100 + m)
    n_hyp = 1024 if m < 20000 else 256
    H, ver, st = handle.verify_homography(ka, kb, mt, n_hyp, THR, 5, 0)
    want = ref.verify(ka, kb, mt, n_hyp=n_hyp, thr=THR, seed=5)
    prob = want["problem"]
    diff = (ver[prob.rows] >= 0) != want["mask"]
    assert not (diff & ~band(prob, want["h"])).any(), diff.sum()
    assert abs(int(st[0]) - int(want["stats"][0])) <= int(band(prob, want["h"]).sum())
    assert H[2, 2] == 1.0
    assert np.abs(ref.map_points(H, CORNERS) - ref.map_points(want["H"], CORNERS)).max() < 0.05
    # against the planted map: 1 px on the corners of the square the points fill (25 noisy inliers extrapolate less well)
    assert np.abs(ref.map_points(H, CORNERS) - ref.map_points(H_TRUE, CORNERS)).max() < (1.0 if m >= 1000 else 2.0)


def _batch_call(handle, pairs, n_hyp, seed, flags=0, stream=None, out=None):
    import torch
    oa = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ob = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    ka = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    kb = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    mt = torch.from_numpy(np.concatenate([p[2] for p in pairs])).cuda()
    d_oa, d_ob = torch.from_numpy(oa).cuda(), torch.from_numpy(ob).cuda()
    n = len(pairs)
    if out is None:
        out = (torch.full((n, 9), np.nan, device="cuda"), torch.full((len(ka),), -7, dtype=torch.int32, device="cuda"),
               torch.zeros((n, 4), dtype=torch.int32, device="cuda"))
    args = (ka, d_oa, kb, d_ob, mt)
    return args, out, oa


def _run(handle, args, out, n_pairs, n_hyp, seed, flags=0, stream=None):
    ka, d_oa, kb, d_ob, mt = args
    H, ver, st = out
    handle.verify_homography_device(ka.data_ptr(), d_oa.data_ptr(), kb.data_ptr(), d_ob.data_ptr(), mt.data_ptr(), n_pairs,
                                    H.data_ptr(), ver.data_ptr(), st.data_ptr(), n_hyp, THR, seed, flags, stream)


def test_batched_equals_single_bit_for_bit(handle):
    import torch
    pairs = _pairs()
    for flags in (0, lfp.VERIFY_NO_REFINE):
        args, out, oa = _batch_call(handle, pairs, 512, 40, flags)
        _run(handle, args, out, len(pairs), 512, 40, flags)
        torch.cuda.synchronize()
        H, ver, st = (t.cpu().numpy() for t in out)
        for p, (ka, kb, mt) in enumerate(pairs):
            h1, v1, s1 = handle.verify_homography(ka, kb, mt, 512, THR, 40 + p, flags)
            assert np.array_equal(H[p].view(np.uint32), h1.reshape(-1).view(np.uint32)), p
            assert np.array_equal(ver[oa[p]:oa[p + 1]], v1), p
            assert np.array_equal(st[p].view(np.uint32), s1), p
            if p % 8 in (0, 1, 2):     # empty, M < 4, collinear: no valid hypothesis
                assert s1[2] == ref.INVALID and s1[0] == 0 and (h1 == 0).all() and (v1 == -1).all(), (p, s1)
            else:
                assert s1[2] != ref.INVALID and s1[0] >= 4, (p, s1)


def test_batch_face_on_device_tensors():
    """LocalFeatures.verify_homography_batch: torch tensors in any integer / float dtype, on torch's current stream and on
    a stream of the caller's; pair p equals the single-pair call with seed + p."""
    import torch
    pairs = _pairs(24)
    feats = lfp.LocalFeatures(64, 64, 64)
    oa = torch.tensor(np.cumsum([0] + [len(p[0]) for p in pairs]))                 # int64 on the host: moved and kept
    ob = torch.tensor(np.cumsum([0] + [len(p[1]) for p in pairs]), dtype=torch.int32).cuda()
    ka = torch.from_numpy(np.concatenate([p[0] for p in pairs])).double().cuda()
    kb = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    mt = torch.from_numpy(np.concatenate([p[2] for p in pairs])).long().cuda()
    H, ver, st = feats.verify_homography_batch(ka, oa, kb, ob, mt, seed=70, n_hypotheses=512)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        H2, ver2, st2 = feats.verify_homography_batch(ka, oa, kb, ob, mt, seed=70, n_hypotheses=512, stream=s)
    s.synchronize()
    torch.cuda.synchronize()
    assert H.shape == (24, 3, 3) and ver.shape == (len(ka),) and st.shape == (24, 4) and st.dtype == torch.int64
    assert torch.equal(H, H2) and torch.equal(ver, ver2) and torch.equal(st, st2)
    H, ver, st, o = H.cpu().numpy(), ver.cpu().numpy(), st.cpu().numpy(), oa.numpy()
    for p, (a, b, m) in enumerate(pairs):
        h1, v1, s1 = feats._inner.verify_homography(a, b, m, 512, THR, 70 + p, 0)
        assert np.array_equal(H[p].reshape(-1).view(np.uint32), h1.reshape(-1).view(np.uint32)), p
        assert np.array_equal(ver[o[p]:o[p + 1]], v1), p
        assert st[p].tolist() == [int(s1[0]), int(s1[1]), -1 if s1[2] == ref.INVALID else int(s1[2]), int(s1[3])], p


def test_repeatable_and_capturable(handle):
    import torch
    pairs = _pairs(16)
    args, out, _ = _batch_call(handle, pairs, 2048, 9)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _run(handle, args, out, 16, 2048, 9, 0, s.cuda_stream)
    s.synchronize()
    first = [t.cpu().clone() for t in out]
    for t in out:
        t.fill_(0)
    with torch.cuda.stream(s):
        _run(handle, args, out, 16, 2048, 9, 0, s.cuda_stream)
    s.synchronize()
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, out))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(handle, args, out, 16, 2048, 9, 0, torch.cuda.current_stream().cuda_stream)
    for t in out:
        t.fill_(0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, out))


def _end_to_end(img1, img2, h_true, min_matches, what):
    feats = lfp.LocalFeatures(max(img1.shape[1], img2.shape[1]), max(img1.shape[0], img2.shape[0]), 3000, n_scales=5)
    kp1, d1 = feats.detect_top_n(img1, 2000, 0.0)
    kp2, d2 = feats.detect_top_n(img2, 2000, 0.0)
    m12 = feats.match(d1, d2)
    assert len(m12) > min_matches
    H, inl = feats.verify_homography(kp1, kp2, m12)
    assert H is not None and len(inl) >= 0.5 * len(m12) and set(inl) <= set(m12)
    assert feats.verify_stats["inliers"] == len(inl) and feats.verify_stats["considered"] == len(m12)
    # the verified matches are right: >= 98 % within 3 px of the true map (the ratio test alone: > 80 %, test_gpu_example.py)
    p1 = np.array([[kp1[i].x, kp1[i].y] for i, _ in inl])
    p2 = np.array([[kp2[j].x, kp2[j].y] for _, j in inl])
    err = np.linalg.norm(ref.map_points(h_true, p1) - p2, axis=1)
    raw = np.array([[kp1[i].x, kp1[i].y, kp2[j].x, kp2[j].y] for i, j in m12])
    raw_ok = (np.linalg.norm(ref.map_points(h_true, raw[:, :2]) - raw[:, 2:], axis=1) < 3.0).mean()
    assert (err < 3.0).mean() >= 0.98, ((err < 3.0).mean(), raw_ok)
    # the same H as the restatement computes from the same matches
    ka = np.array([(k.x, k.y, k.size, k.angle, k.response) for k in kp1], np.float32)
    kb = np.array([(k.x, k.y, k.size, k.angle, k.response) for k in kp2], np.float32)
    m = np.full(len(ka), -1, np.int32)
    for i, j in m12:
        m[i] = j
    want = ref.verify(ka, kb, m)
    hgt, w = img1.shape
    corners = np.array([[0, 0], [w, 0], [w, hgt], [0, hgt]], np.float64)
    assert np.abs(ref.map_points(H, corners) - ref.map_points(want["H"], corners)).max() < 0.05
    # the refit is what makes H accurate: it is kept (the 4-point hypothesis alone is several px off at the corners)
    assert want["h"] is not want["hyps"][want["k"]]
    # and the true map: the image's corners within 1.5 px
    img_err = np.abs(ref.map_points(H, corners) - ref.map_points(h_true, corners)).max()
    hyp_err = np.abs(ref.map_points(want["hyps"][want["k"]], corners) - ref.map_points(h_true, corners)).max()
    print(f"[homography] {what}: {len(m12)} ratio-test matches ({raw_ok:.1%} within 3 px of the true map) -> {len(inl)} verified "
          f"({(err < 3.0).mean():.1%} within 3 px); H vs the true map at the image corners: {img_err:.2f} px "
          f"(best 4-point hypothesis: {hyp_err:.2f} px)")
    assert img_err < 1.5, (img_err, hyp_err)
    return kp1, kp2, m12, H, inl


def test_end_to_end_on_a_perspective_warp_of_a_photograph():
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    crop = im.crop((x0, y0, x0 + 1024, y0 + 768))
    h_true = np.array([[0.95, 0.06, 20.0], [-0.04, 0.97, 15.0], [4e-5, -3e-5, 1.0]])   # crop -> warped view
    hi = np.linalg.inv(h_true)
    hi = hi / hi[2, 2]
    warped = crop.transform((1024, 768), Image.PERSPECTIVE, tuple(hi.reshape(-1)[:8]), resample=Image.BICUBIC)
    img1 = np.asarray(crop, np.float32) / 255.0
    img2 = np.asarray(warped, np.float32) / 255.0
    kp1, kp2, m12, H, inl = _end_to_end(img1, img2, h_true, 200, "houses.jpg crop, perspective warp")
    # the C++ face (include/local_features.hpp) on the same keypoints and matches: the same H and inliers, bit for bit
    import subprocess
    import tempfile
    from conftest import MODELS, ROOT
    lib_dir = os.path.join(ROOT, "local-features_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe, pre = os.path.join(tmp, "demo_verify"), os.path.join(tmp, "io")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "demo_verify.cpp"), "-L", lib_dir, "-llf_mkd",
                               f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
        np.array([(k.x, k.y, k.size, k.angle, k.response) for k in kp1], np.float32).tofile(pre + ".ka")
        np.array([(k.x, k.y, k.size, k.angle, k.response) for k in kp2], np.float32).tofile(pre + ".kb")
        np.array(m12, np.int32).tofile(pre + ".m")
        out = subprocess.run([exe, MODELS, pre, pre], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.splitlines()[-1] == "bad match: InvalidParameters", out.stdout
        h_cpp = np.fromfile(pre + ".H", np.float32)
        inl_cpp = [tuple(r) for r in np.fromfile(pre + ".inl", np.int32).reshape(-1, 2).tolist()]
    assert np.array_equal(h_cpp, H.astype(np.float32).reshape(-1)) and inl_cpp == inl


def test_end_to_end_on_the_examples_rotation():
    from PIL import Image
    img1 = np.asarray(Image.open(os.path.join(GOLDEN, "bird.jpg")).convert("L"), np.float32) / 255.0
    hgt, w = img1.shape
    ang = np.deg2rad(17.0)
    c, s = np.cos(ang), np.sin(ang)
    cx, cy = w / 2, hgt / 2
    inv = (c, s, cx - c * cx - s * cy, -s, c, cy + s * cx - c * cy)
    im2 = Image.fromarray((img1 * 255).astype(np.uint8)).transform((w, hgt), Image.AFFINE, inv, resample=Image.BICUBIC)
    img2 = np.asarray(im2, np.float32) / 255.0
    h_true = np.linalg.inv(np.array([inv[:3], inv[3:], [0, 0, 1.0]]))
    _end_to_end(img1, img2, h_true, 150, "bird.jpg, 17 degree rotation")
