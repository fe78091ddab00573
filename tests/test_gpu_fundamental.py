"""RANSAC fundamental-matrix verification on the GPU (lf_mkd_verify_fundamental*) against the numpy restatement
(tests/fundamental_ref.py): the same samples, candidates and counts, the same refit, batched = single, bit-stable and
capturable, sharing the handle with the homography, and end to end on a photograph seen with parallax."""
import os

import numpy as np
import pytest

import fundamental_ref as ref
import homography_ref as href
from conftest import GOLDEN
from fundamental_cases import THR, band, two_view
from fundamental_cases import pairs as _pairs

import local_features_python as lfp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    return lfp.MkdHandle(max_features=64)


def _line_gap(prob, f1, f2, mask):
    """Largest distance between the epipolar lines of the masked matches under F1 and F2 (in view b, over the frame's width)."""
    a = np.concatenate([prob.a[mask], np.ones((int(mask.sum()), 1))], axis=1)
    gaps = []
    for x in (0.0, 512.0, 1024.0):
        ys = []
        for f in (f1, f2):
            l = a @ np.asarray(f, np.float64).reshape(3, 3).T
            ys.append(-(l[:, 0] * x + l[:, 2]) / l[:, 1])
        gaps.append(np.abs(ys[0] - ys[1]))
    return float(np.max(gaps)) if mask.any() else 0.0


@pytest.mark.parametrize("m", [7, 50, 1000, 20000])
@pytest.mark.parametrize("frac", [0.1, 0.5, 0.9])
def test_candidates_match_the_restatement(handle, m, frac):
    n_hyp = 256
    ka, kb, mt, _ = two_view(m, frac, seed=m + int(frac * 10))
    F, ver, st = handle.verify_fundamental(ka, kb, mt, n_hyp, THR, 11, lfp.VERIFY_NO_REFINE)
    prob = ref.Problem(ka, kb, mt)
    counts, cands = ref.score_all(prob, 11, n_hyp, THR)
    assert st[3] == m
    if counts.max() < 0:
        assert st[2] == ref.INVALID and st[0] == 0 and (F == 0).all() and (ver == -1).all()
        return
    c = int(st[2])
    assert c < 3 * n_hyp and cands[c] is not None, (c, counts[c] if c < 3 * n_hyp else None)
    f_c = cands[c][0]
    slack_c = int(band(prob, f_c).sum())
    assert abs(int(st[1]) - counts[c]) <= slack_c, (st, counts[c], slack_c)
    c_ref = int(np.argmax(counts))
    slack_ref = int(band(prob, cands[c_ref][0]).sum())
    if c != c_ref:   # only a near tie may choose another candidate
        assert counts[c_ref] - counts[c] <= slack_ref + slack_c, (c, c_ref, counts[c], counts[c_ref])
    assert st[0] == st[1] and (ver >= 0).sum() == st[0]
    diff = (ver[prob.rows] >= 0) != prob.inliers(f_c, THR)
    assert not (diff & ~band(prob, f_c)).any(), diff.sum()
    assert np.abs(F).max() == 1.0 and (F.reshape(-1) == 1.0).any()


@pytest.mark.parametrize("m,frac", [(50, 0.3), (1000, 0.3), (1000, 0.5), (20000, 0.4)])
def test_refit_matches_the_restatement(handle, m, frac):
    n_hyp = 256
    ka, kb, mt, info = two_view(m, frac, seed=100 + m)
    F, ver, st = handle.verify_fundamental(ka, kb, mt, n_hyp, THR, 5, 0)
    want = ref.verify(ka, kb, mt, n_hyp=n_hyp, thr=THR, seed=5)
    prob = want["problem"]
    b = band(prob, want["f"]) | band(prob, F)
    diff = (ver[prob.rows] >= 0) != want["mask"]
    assert not (diff & ~b).any(), diff.sum()
    assert abs(int(st[0]) - int(want["stats"][0])) <= int(b.sum())
    # the epipolar lines of the inliers agree within 0.05 px
    gap = _line_gap(prob, F, want["F"], want["mask"])
    assert gap < 0.05, gap
    inl = info["inlier"]
    d = ref.epipolar_distance(F, info["a"][inl], info["b"][inl])
    assert np.median(d) < 0.5, np.median(d)


def _batch(pairs):
    import torch
    oa = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ob = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    ka = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    kb = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    mt = torch.from_numpy(np.concatenate([p[2] for p in pairs])).cuda()
    n = len(pairs)
    out = (torch.full((n, 9), np.nan, device="cuda"), torch.full((len(ka),), -7, dtype=torch.int32, device="cuda"),
           torch.zeros((n, 4), dtype=torch.int32, device="cuda"))
    return (ka, torch.from_numpy(oa).cuda(), kb, torch.from_numpy(ob).cuda(), mt), out, oa


def _run(handle, args, out, n_pairs, n_hyp, seed, flags=0, stream=None, fn="fundamental"):
    ka, d_oa, kb, d_ob, mt = args
    M, ver, st = out
    call = handle.verify_fundamental_device if fn == "fundamental" else handle.verify_homography_device
    call(ka.data_ptr(), d_oa.data_ptr(), kb.data_ptr(), d_ob.data_ptr(), mt.data_ptr(), n_pairs, M.data_ptr(), ver.data_ptr(),
         st.data_ptr(), n_hyp, THR, seed, flags, stream)


def test_batched_equals_single_bit_for_bit(handle):
    """Pair p of a ragged batch (48 pairs: few row slices) equals the single-pair call (one pair: up to 16 slices)."""
    import torch
    pairs = _pairs()
    for flags in (0, lfp.VERIFY_NO_REFINE):
        args, out, oa = _batch(pairs)
        _run(handle, args, out, len(pairs), 512, 40, flags)
        torch.cuda.synchronize()
        F, ver, st = (t.cpu().numpy() for t in out)
        for p, (ka, kb, mt) in enumerate(pairs):
            f1, v1, s1 = handle.verify_fundamental(ka, kb, mt, 512, THR, 40 + p, flags)
            assert np.array_equal(F[p].view(np.uint32), f1.reshape(-1).view(np.uint32)), p
            assert np.array_equal(ver[oa[p]:oa[p + 1]], v1), p
            assert np.array_equal(st[p].view(np.uint32), s1), p
            if p % 8 in (0, 1):     # empty, M < 7: no valid sample
                assert s1[2] == ref.INVALID and s1[0] == 0 and (f1 == 0).all() and (v1 == -1).all(), (p, s1)
            else:
                assert s1[2] != ref.INVALID and s1[0] >= 7, (p, s1)


def test_repeatable_capturable_and_shares_scratch_with_the_homography(handle):
    import torch
    pairs = _pairs(16)
    args, out, _ = _batch(pairs)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _run(handle, args, out, 16, 2048, 9, 0, s.cuda_stream)
    s.synchronize()
    first = [t.cpu().clone() for t in out]
    # the homography alone, into its own outputs
    _, h_out, _ = _batch(pairs)
    with torch.cuda.stream(s):
        _run(handle, args, h_out, 16, 2048, 9, 0, s.cuda_stream, fn="homography")
    s.synchronize()
    h_first = [t.cpu().clone() for t in h_out]
    # interleaved on one handle and one stream: each gives the bits it gives alone
    for t in out + h_out:
        t.fill_(0)
    with torch.cuda.stream(s):
        _run(handle, args, h_out, 16, 2048, 9, 0, s.cuda_stream, fn="homography")
        _run(handle, args, out, 16, 2048, 9, 0, s.cuda_stream)
        _run(handle, args, h_out, 16, 256, 9, 0, s.cuda_stream, fn="homography")     # a smaller call in between
        _run(handle, args, h_out, 16, 2048, 9, 0, s.cuda_stream, fn="homography")
    s.synchronize()
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, out))
    assert all(torch.equal(a, b.cpu()) for a, b in zip(h_first, h_out))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(handle, args, out, 16, 2048, 9, 0, torch.cuda.current_stream().cuda_stream)
    for t in out:
        t.fill_(0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, out))


def test_batch_face_on_device_tensors():
    import torch
    pairs = _pairs(24)
    feats = lfp.LocalFeatures(64, 64, 64)
    oa = torch.tensor(np.cumsum([0] + [len(p[0]) for p in pairs]))
    ob = torch.tensor(np.cumsum([0] + [len(p[1]) for p in pairs]), dtype=torch.int32).cuda()
    ka = torch.from_numpy(np.concatenate([p[0] for p in pairs])).double().cuda()
    kb = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    mt = torch.from_numpy(np.concatenate([p[2] for p in pairs])).long().cuda()
    F, ver, st = feats.verify_fundamental_batch(ka, oa, kb, ob, mt, seed=70, n_hypotheses=512)
    torch.cuda.synchronize()
    assert F.shape == (24, 3, 3) and ver.shape == (len(ka),) and st.shape == (24, 4) and st.dtype == torch.int64
    F, ver, st, o = F.cpu().numpy(), ver.cpu().numpy(), st.cpu().numpy(), oa.numpy()
    for p, (a, b, m) in enumerate(pairs):
        f1, v1, s1 = feats._inner.verify_fundamental(a, b, m, 512, THR, 70 + p, 0)
        assert np.array_equal(F[p].reshape(-1).view(np.uint32), f1.reshape(-1).view(np.uint32)), p
        assert np.array_equal(ver[o[p]:o[p + 1]], v1), p
        assert st[p].tolist() == [int(s1[0]), int(s1[1]), -1 if s1[2] == ref.INVALID else int(s1[2]), int(s1[3])], p


# ---- end to end: a "folded card" view of the houses crop -------------------------------------------------------------
FK = np.array([[900.0, 0.0, 512.0], [0.0, 900.0, 384.0], [0.0, 0.0, 1.0]])
Z0 = 6.0                                        # the fold: the 3-D line X = 0, Z = Z0 (view 1's column x = 512)
SLOPES = (-0.45, 0.45)                          # plane i: Z = Z0 + s_i X (left half, right half of view 1)


def _card_homographies():
    ang = np.deg2rad(3.0)
    r = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    t = np.array([-0.9, 0.05, 0.1])
    ki = np.linalg.inv(FK)
    hs = []
    for s in SLOPES:
        n = np.array([-s, 0.0, 1.0])               # n^T X = Z0 on the plane
        h = FK @ (r + np.outer(t, n) / Z0) @ ki
        hs.append(h / h[2, 2])
    f = ki.T @ np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ r @ ki
    return hs, f


def _card_map(hs, pts):
    """view 1 -> view 2, the piecewise true map (left of x = 512: plane 0, else plane 1)."""
    pts = np.asarray(pts, np.float64)
    left = pts[:, 0] < 512.0
    return np.where(left[:, None], href.map_points(hs[0], pts), href.map_points(hs[1], pts))


def _render_card(img, hs):
    from scipy.ndimage import map_coordinates
    hgt, w = img.shape
    yy, xx = np.mgrid[0:hgt, 0:w].astype(np.float64)
    q = np.stack([xx.ravel(), yy.ravel()], axis=1)
    src0, src1 = href.map_points(np.linalg.inv(hs[0]), q), href.map_points(np.linalg.inv(hs[1]), q)
    src = np.where((src0[:, 0] < 512.0)[:, None], src0, src1)
    out = map_coordinates(img.astype(np.float64), [src[:, 1], src[:, 0]], order=3, mode="constant", cval=0.0)
    return np.clip(out, 0.0, 1.0).reshape(hgt, w).astype(np.float32)


def test_end_to_end_on_a_photograph_with_parallax():
    from PIL import Image
    im = Image.open(os.path.join(GOLDEN, "houses.jpg")).convert("L")
    x0, y0 = (im.width - 1024) // 2, (im.height - 768) // 2
    img1 = np.asarray(im.crop((x0, y0, x0 + 1024, y0 + 768)), np.float32) / 255.0
    hs, f_true = _card_homographies()
    # enough parallax: neither plane's homography maps the other half within 10 px
    g = np.random.default_rng(0)
    left = np.stack([g.uniform(0, 400, 500), g.uniform(0, 768, 500)], axis=1)
    right = np.stack([g.uniform(624, 1024, 500), g.uniform(0, 768, 500)], axis=1)
    off_l = np.linalg.norm(href.map_points(hs[1], left) - href.map_points(hs[0], left), axis=1)
    off_r = np.linalg.norm(href.map_points(hs[0], right) - href.map_points(hs[1], right), axis=1)
    assert np.percentile(off_l, 5) > 10 and np.percentile(off_r, 5) > 10, (np.percentile(off_l, 5), np.percentile(off_r, 5))
    img2 = _render_card(img1, hs)
    feats = lfp.LocalFeatures(1024, 768, 3000, n_scales=5)
    kp1, d1 = feats.detect_top_n(img1, 2000, 0.0)
    kp2, d2 = feats.detect_top_n(img2, 2000, 0.0)
    m12 = feats.match(d1, d2)
    assert len(m12) > 200
    p1 = np.array([[kp1[i].x, kp1[i].y] for i, _ in m12])
    p2 = np.array([[kp2[j].x, kp2[j].y] for _, j in m12])
    correct = np.linalg.norm(_card_map(hs, p1) - p2, axis=1) < 3.0
    on_left = p1[:, 0] < 512.0
    F, inl = feats.verify_fundamental(kp1, kp2, m12)
    assert F is not None and set(inl) <= set(m12)
    assert feats.verify_stats["inliers"] == len(inl) and feats.verify_stats["considered"] == len(m12)
    kept = np.array([ij in set(inl) for ij in m12])
    H, inl_h = feats.verify_homography(kp1, kp2, m12)
    kept_h = np.array([ij in set(inl_h) for ij in m12])
    # the true correspondences' symmetric epipolar distance under the recovered F
    q1 = np.stack([g.uniform(0, 1024, 2000), g.uniform(0, 768, 2000)], axis=1)
    q2 = _card_map(hs, q1)
    vis = (q2[:, 0] >= 0) & (q2[:, 0] < 1024) & (q2[:, 1] >= 0) & (q2[:, 1] < 768)
    d = ref.epipolar_distance(F, q1[vis], q2[vis])
    share = lambda k, sel: (k & correct & sel).sum() / max((correct & sel).sum(), 1)
    print(f"[fundamental] houses.jpg crop, folded card: {len(m12)} ratio-test matches ({correct.mean():.1%} correct) -> "
          f"{kept.sum()} kept: {share(kept, np.ones_like(kept)):.1%} of the correct ones (left plane {share(kept, on_left):.1%}, "
          f"right plane {share(kept, ~on_left):.1%}), {(kept & correct).sum() / max(kept.sum(), 1):.1%} of them correct; "
          f"epipolar distance of true correspondences median {np.median(d):.3f} px, p95 {np.percentile(d, 95):.3f} px; "
          f"verify_homography keeps {share(kept_h, np.ones_like(kept)):.1%} of the correct matches")
    assert share(kept, np.ones_like(kept)) >= 0.90
    assert share(kept, on_left) >= 0.80 and share(kept, ~on_left) >= 0.80
    assert (kept & correct).sum() >= 0.95 * kept.sum()
    assert np.median(d) < 0.5 and np.percentile(d, 95) < 1.5, (np.median(d), np.percentile(d, 95))
    assert share(kept_h, np.ones_like(kept)) < 0.70
    # the same F (up to scale) relates the true correspondences: F_true agrees on the same points
    d_true = ref.epipolar_distance(f_true, q1[vis], q2[vis])
    assert np.median(d_true) < 1e-6
    # the C++ face (include/local_features.hpp) on the same keypoints and matches: the same F and inliers, bit for bit
    import subprocess
    import tempfile
    from conftest import MODELS, ROOT
    lib_dir = os.path.join(ROOT, "local-features_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe, pre = os.path.join(tmp, "demo_verify_fundamental"), os.path.join(tmp, "io")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "demo_verify_fundamental.cpp"), "-L", lib_dir, "-llf_mkd",
                               f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
        np.array([(k.x, k.y, k.size, k.angle, k.response) for k in kp1], np.float32).tofile(pre + ".ka")
        np.array([(k.x, k.y, k.size, k.angle, k.response) for k in kp2], np.float32).tofile(pre + ".kb")
        np.array(m12, np.int32).tofile(pre + ".m")
        out = subprocess.run([exe, MODELS, pre, pre], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.splitlines()[-1] == "bad match: InvalidParameters", out.stdout
        f_cpp = np.fromfile(pre + ".F", np.float32)
        inl_cpp = [tuple(r) for r in np.fromfile(pre + ".inl", np.int32).reshape(-1, 2).tolist()]
    assert np.array_equal(f_cpp, F.astype(np.float32).reshape(-1)) and inl_cpp == inl
