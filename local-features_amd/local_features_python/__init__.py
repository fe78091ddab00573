"""Python face of the MI355X MKD descriptor path, mirroring the reference's pyo3 module
`local_features_python` (python/src/lib.rs:11-160) for the part of it this build covers.

The reference class exposes `detect` / `detect_top_n` (detector + describe in one call,
python/src/lib.rs:86-149), both provided here with the same signatures and the
`(list[Keypoint], ndarray[n,128] f32)` result.  The hot path of this build is the describe half
(SURVEY.md section 8), so the class also offers it on its own: `describe` takes the keypoint list the
detector would have produced, `orient` / `describe_extrema` take the detector's refined extrema and run
keypoint orientation first (the whole extract graph, mod.rs:1277-1572), `describe_patches` takes patches.
Nothing here falls back to a CPU path.
"""
import threading

import numpy as np

from ._lib import (ANGLE_EXACT, ANGLE_EXACT_ZERO, ANGLE_SHADER, FLAG_DETECT_STEPWISE, FLAG_KERNEL_TIMING, FLAG_UNFUSED_KEYPOINTS, KEYPOINT_DTYPE, KNN_MAX, LIB_PATH, MODEL_DIR, PCA_NAMES,
                   POOL_DEFAULT, POOL_F16X3, POOL_F32, POOL_F16_FP6, SYMBOLS, COMM_ID_BYTES, GATHER_DIRECT, GATHER_RING, GUIDE_FUNDAMENTAL, GUIDE_HOMOGRAPHY, MATCH_MUTUAL, TRACKS_ACCUMULATE, TRACKS_DUP_TILE, TRACK_TABLE_CONSISTENT, LINK_TABLE_LOCAL, SELECT_SKIP_SELF, SELECT_UNIQUE, SELECT_MAX_K, COVIS_ACCUMULATE, COVIS_FORM_LDS, RESECT_ALL, VIEW_GRAPH_USE_UNCHECKED, VIEW_GRAPH_AUTO_ROOT, BA_REFINE_FOCAL, BA_REFINE_PRINCIPAL, VERIFY_NO_REFINE, Comm,
                   MkdHandle, Q8_SCALE, comm_unique_id, knn_q8_plan, load_library, match_q8_grouped_plan, match_q8_pairs_plan, match_q8_plan, model_path, plan_upload, track_table_plan, link_table_plan, select_edges_plan, covisibility_plan, view_graph_plan, global_positions_plan, GLOBAL_POSITIONS_MAX_SWEEPS)

__all__ = ["Keypoint", "LocalFeatures", "MkdHandle", "ANGLE_SHADER", "ANGLE_EXACT", "ANGLE_EXACT_ZERO", "POOL_DEFAULT", "POOL_F32", "POOL_F16_FP6",
           "POOL_F16X3", "FLAG_KERNEL_TIMING", "FLAG_UNFUSED_KEYPOINTS", "FLAG_DETECT_STEPWISE", "KEYPOINT_DTYPE", "PCA_NAMES", "SYMBOLS", "LIB_PATH", "MODEL_DIR",
           "load_library", "model_path", "plan_upload", "Comm", "comm_unique_id", "COMM_ID_BYTES", "GATHER_DIRECT", "GATHER_RING",
           "VERIFY_NO_REFINE", "MATCH_MUTUAL", "GUIDE_HOMOGRAPHY", "GUIDE_FUNDAMENTAL", "Q8_SCALE", "match_q8_plan", "match_q8_pairs_plan",
           "KNN_MAX", "knn_q8_plan", "match_q8_grouped_plan", "TRACKS_ACCUMULATE", "TRACKS_DUP_TILE", "TRACK_TABLE_CONSISTENT", "track_table_plan",
           "LINK_TABLE_LOCAL", "link_table_plan", "SELECT_SKIP_SELF", "SELECT_UNIQUE", "SELECT_MAX_K", "select_edges_plan",
           "COVIS_ACCUMULATE", "COVIS_FORM_LDS", "RESECT_ALL", "BA_REFINE_FOCAL", "BA_REFINE_PRINCIPAL", "covisibility_plan",
           "VIEW_GRAPH_USE_UNCHECKED", "VIEW_GRAPH_AUTO_ROOT", "view_graph_plan", "GLOBAL_POSITIONS_MAX_SWEEPS",
           "global_positions_plan"]


class Keypoint:
    """python/src/lib.rs:11-23; angle in degrees (keypoint_orientation.glsl:162-167)."""
    __slots__ = ("x", "y", "size", "angle", "response")

    def __init__(self, x, y, size, angle, response=0.0):
        self.x, self.y, self.size, self.angle, self.response = (
            float(x), float(y), float(size), float(angle), float(response))

    def __repr__(self):
        return (f"Keypoint(x={self.x:.3f}, y={self.y:.3f}, size={self.size:.3f}, "
                f"angle={self.angle:.2f}, response={self.response:.4f})")


def _keypoints_to_array(keypoints):
    if isinstance(keypoints, np.ndarray):
        if keypoints.dtype == KEYPOINT_DTYPE:
            return np.ascontiguousarray(keypoints)
        k = np.ascontiguousarray(keypoints, np.float32)
        if k.ndim != 2 or k.shape[1] not in (4, 5):
            raise RuntimeError("keypoints array must be [n,4] (x,y,size,angle) or [n,5] (+response)")
        if k.shape[1] == 4:
            k = np.concatenate([k, np.zeros((k.shape[0], 1), np.float32)], axis=1)
        return np.ascontiguousarray(k)
    return np.array([(k.x, k.y, k.size, k.angle, k.response) for k in keypoints],
                    dtype=np.float32).reshape(-1, 5)


class LocalFeatures:
    """LocalFeatures(max_image_width, max_image_height, max_features, max_blobs, n_scales, pca)
    -- python/src/lib.rs:43-84.  The last detect call's FeaturesResult counters (lib.rs:77-83) are kept in
    `dropped_blobs` / `dropped_features`."""

    def __init__(self, max_image_width, max_image_height, max_features, max_blobs=8000, n_scales=4,
                 pca="liberty", device=0, angle_mode=ANGLE_SHADER, pool_mode=POOL_DEFAULT, max_frames=1, flags=0):
        if pca not in PCA_NAMES:
            raise RuntimeError("Invalid PCA argument")
        try:
            self._inner = MkdHandle(pca=pca, max_features=max_features, max_image_width=max_image_width,
                                    max_image_height=max_image_height, device=device,
                                    angle_mode=angle_mode, pool_mode=pool_mode, n_scales=n_scales,
                                    max_blobs=max_blobs, max_frames=max_frames, flags=flags)
        except RuntimeError as e:   # python/src/lib.rs:77-82
            raise RuntimeError("Failed to initialize local features", str(e)) from e
        self._lock = threading.Lock()   # Mutex<LocalFeaturesVulkan>, python/src/lib.rs:38
        self.max_blobs, self.n_scales, self.max_frames = max_blobs, n_scales, max_frames
        self.max_features, self.device = max_features, device
        self.dropped_blobs = self.dropped_features = 0

    def describe(self, img, keypoints):
        """img: 2-D float32 array in [0,1]; keypoints: list[Keypoint] or [n,4|5] array.
        Returns (list[Keypoint], ndarray[n,128] float32), the reference's result shape."""
        arr = np.asarray(img)
        if arr.ndim != 2:
            raise RuntimeError("Failed to extract features", "image must be 2-dimensional")
        kps = _keypoints_to_array(keypoints)
        with self._lock:
            try:
                self._inner.set_image(arr)
                desc = self._inner.describe_keypoints(kps)
            except RuntimeError as e:   # python/src/lib.rs:97-102
                raise RuntimeError("Failed to extract features", str(e)) from e
        out_k = [Keypoint(*row) for row in kps.reshape(-1, 5)] if not isinstance(keypoints, list) else keypoints
        return out_k, desc

    def orient(self, img, extrema):
        """extrema: [n,4] array (x, y, size, response), the detector's refined extrema.  Returns the
        list[Keypoint] keypoint orientation yields (one per histogram peak, keypoint_orientation.glsl:36-171),
        ordered by extremum then bin."""
        return self.describe_extrema(img, extrema, describe=False)[0]

    def describe_extrema(self, img, extrema, describe=True):
        """The whole extract graph: orientation, then sampling + description of every keypoint found.
        Returns (list[Keypoint], ndarray[m,128] float32)."""
        arr = np.asarray(img)
        if arr.ndim != 2:
            raise RuntimeError("Failed to extract features", "image must be 2-dimensional")
        ex = np.ascontiguousarray(extrema, np.float32)
        if ex.ndim != 2 or ex.shape[1] != 4:
            raise RuntimeError("extrema array must be [n,4] (x, y, size, response)")
        with self._lock:
            try:
                self._inner.set_image(arr)
                kps, _ = self._inner.orient_keypoints(ex)
                desc = self._inner.describe_keypoints(kps) if describe else None
            except RuntimeError as e:
                raise RuntimeError("Failed to extract features", str(e)) from e
        return [Keypoint(*row) for row in kps], desc

    def match(self, desc_a, desc_b, ratio=0.8):
        """match_features of the reference's match_images example (examples/match_images/src/main.rs:8-27):
        list of (i, j) with j the best match of desc_a[i] in desc_b that passes Lowe's ratio test."""
        with self._lock:
            m = self._inner.match(desc_a, desc_b, ratio)
        return [(int(i), int(j)) for i, j in enumerate(m) if j >= 0]

    def match_both(self, desc_a, desc_b, ratio=0.8):
        """Both directions of the example (examples/match_images/src/main.rs:113-116: match_features(f1, f2) and
        match_features(f2, f1)) in one library call -- one launch at the example's own size (lf_mkd_match_both_device).
        Returns (matches a -> b, matches b -> a), each as `match` returns them."""
        import torch
        a = np.ascontiguousarray(desc_a, np.float32).reshape(-1, 128)
        b = np.ascontiguousarray(desc_b, np.float32).reshape(-1, 128)
        if len(a) < 2 or len(b) < 2:
            return self.match(a, b, ratio) if len(a) and len(b) >= 2 else [], self.match(b, a, ratio) if len(b) and len(a) >= 2 else []
        dev = torch.device("cuda", self.device)
        with self._lock, torch.cuda.device(dev):
            d_a, d_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            m_ab = torch.empty((len(a),), dtype=torch.int32, device=dev)
            m_ba = torch.empty((len(b),), dtype=torch.int32, device=dev)
            s = torch.cuda.current_stream(dev)
            self._inner.match_both_device(d_a.data_ptr(), len(a), d_b.data_ptr(), len(b), m_ab.data_ptr(), m_ba.data_ptr(),
                                          ratio, s.cuda_stream)
            s.synchronize()
            self._inner.synchronize()       # (torch's default stream is handle 0 = "the library's own stream" to the ABI)
            m_ab, m_ba = m_ab.cpu().numpy(), m_ba.cpu().numpy()
        return ([(int(i), int(j)) for i, j in enumerate(m_ab) if j >= 0], [(int(i), int(j)) for i, j in enumerate(m_ba) if j >= 0])

    def match_batch(self, desc_a, offsets_a, desc_b, offsets_b, ratio=0.8, mutual=False, both=False, stream=None):
        """Many image pairs in one call (lf_mkd_match_pairs_device: one launch, three with `mutual`) on torch tensors, which
        are moved to the handle's device if they are elsewhere.  desc_a [Na,128] / desc_b [Nb,128] (any float dtype),
        offsets_a / offsets_b [n_pairs + 1] (any integer dtype, non-decreasing): pair p matches a rows
        offsets_a[p]..offsets_a[p+1] against b rows offsets_b[p]..offsets_b[p+1], each pair exactly as `match` decides it alone.
        Two layouts:
          * the verifiers' own -- the pairs' rows back to back on either side, offsets = the running sums of the pairs' sizes;
            the result goes into verify_homography_batch / verify_fundamental_batch with the same offsets;
          * a sequence without a copied row -- one array `desc` of F frames with frame offsets o [F + 1]: desc_a = desc with
            offsets_a = o[0:F], desc_b = desc[o[1]:] (a view) with offsets_b = o[1:F+1] - o[1]; pair t is then frame t against
            frame t + 1.  (desc_b = desc itself with offsets_b = o[1:F+1] says the same without reading o[1] on the host.)
        Returns device tensors (match_ab [Na] int32, match_ba [Nb] int32 or None, best [Na], second [Na]): match_ab[i] is
        the index local to the pair's b rows or -1, match_ba (with `both` or `mutual`) the other direction, local to the
        pair's a rows; rows outside every pair hold -1 / -inf.  `mutual` keeps a match only if both directions agree (best /
        second stay as the a -> b direction found them).  Enqueued on `stream` (default: torch's current stream on the
        handle's device), asynchronously."""
        import torch
        dev = torch.device("cuda", self.device)
        n_pairs = int(offsets_a.numel()) - 1
        if n_pairs < 0 or int(offsets_b.numel()) != n_pairs + 1:
            raise RuntimeError("match_batch: offsets_a and offsets_b need n_pairs + 1 entries each")
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):      # the copies and the fills below are ordered with the call
            a = desc_a.to(dev, torch.float32).reshape(-1, 128).contiguous()
            b = desc_b.to(dev, torch.float32).reshape(-1, 128).contiguous()
            oa, ob = offsets_a.to(dev, torch.int64).contiguous(), offsets_b.to(dev, torch.int64).contiguous()
            na, nb = a.shape[0], b.shape[0]
            m_ab = torch.full((na,), -1, dtype=torch.int32, device=dev)
            m_ba = torch.full((nb,), -1, dtype=torch.int32, device=dev) if (both or mutual) else None
            best = torch.full((na,), float("-inf"), dtype=torch.float32, device=dev)
            second = torch.full((na,), float("-inf"), dtype=torch.float32, device=dev)
            if n_pairs and na and nb:       # (an empty side: every pair is refused, the fills above are the answer)
                with self._lock:
                    self._inner.match_pairs_device(a.data_ptr(), oa.data_ptr(), na, b.data_ptr(), ob.data_ptr(), nb, n_pairs,
                                                   m_ab.data_ptr(), m_ba.data_ptr() if m_ba is not None else None, ratio,
                                                   MATCH_MUTUAL if mutual else 0, best.data_ptr(), second.data_ptr(),
                                                   s.cuda_stream)
        return m_ab, m_ba, best, second

    def match_guided_batch(self, desc_a, kps_a, offsets_a, desc_b, kps_b, offsets_b, model, kind="homography", threshold=None,
                           ratio=0.8, mutual=True, stream=None):
        """Guided matching of many image pairs in one call (lf_mkd_match_guided_pairs_device: one launch, three with
        `mutual`): match_batch once more, with the candidates of every row restricted to the rows of the other side that pass
        the verifier's inlier test with it under the pair's model -- a transfer disc under H, an epipolar band under F.
        Tensors as match_batch takes them (moved to the handle's device, any float / integer dtype), plus kps_a [Na,5] /
        kps_b [Nb,5] (indexed like the descriptor rows; x and y are read) and model [n_pairs,3,3] (or [n_pairs,9]), e.g. what
        verify_homography_batch / verify_fundamental_batch return.  kind: "homography" or "fundamental" (or GUIDE_*);
        threshold in pixels, default the verifier's own (3.0 for H, 1.5 for F).  Returns device tensors (match_ab [Na] int32,
        match_ba [Nb] int32, best [Na], second [Na]) as match_batch does; rows outside every pair hold -1 / -inf.  With the
        verifier's model, threshold and ratio and `mutual`, every verified match is found again (include/lf_mkd.h).
        Enqueued on `stream` (default: torch's current stream on the handle's device), asynchronously."""
        import torch
        kinds = {"homography": GUIDE_HOMOGRAPHY, "fundamental": GUIDE_FUNDAMENTAL, GUIDE_HOMOGRAPHY: GUIDE_HOMOGRAPHY,
                 GUIDE_FUNDAMENTAL: GUIDE_FUNDAMENTAL}
        if kind not in kinds:
            raise RuntimeError('match_guided_batch: kind must be "homography" or "fundamental"')
        kind = kinds[kind]
        if threshold is None:
            threshold = 3.0 if kind == GUIDE_HOMOGRAPHY else 1.5
        dev = torch.device("cuda", self.device)
        n_pairs = int(offsets_a.numel()) - 1
        if n_pairs < 0 or int(offsets_b.numel()) != n_pairs + 1:
            raise RuntimeError("match_guided_batch: offsets_a and offsets_b need n_pairs + 1 entries each")
        if int(model.numel()) != 9 * n_pairs:
            raise RuntimeError("match_guided_batch: model needs 9 entries per pair")
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):      # the copies and the fills below are ordered with the call
            a = desc_a.to(dev, torch.float32).reshape(-1, 128).contiguous()
            b = desc_b.to(dev, torch.float32).reshape(-1, 128).contiguous()
            ka = kps_a.to(dev, torch.float32).reshape(-1, 5).contiguous()
            kb = kps_b.to(dev, torch.float32).reshape(-1, 5).contiguous()
            oa, ob = offsets_a.to(dev, torch.int64).contiguous(), offsets_b.to(dev, torch.int64).contiguous()
            md = model.to(dev, torch.float32).reshape(-1, 9).contiguous()
            na, nb = a.shape[0], b.shape[0]
            if ka.shape[0] != na or kb.shape[0] != nb:
                raise RuntimeError("match_guided_batch: one keypoint per descriptor row on either side")
            m_ab = torch.full((na,), -1, dtype=torch.int32, device=dev)
            m_ba = torch.full((nb,), -1, dtype=torch.int32, device=dev)
            best = torch.full((na,), float("-inf"), dtype=torch.float32, device=dev)
            second = torch.full((na,), float("-inf"), dtype=torch.float32, device=dev)
            if n_pairs and na and nb:       # (an empty side: no row has a candidate, the fills above are the answer)
                with self._lock:
                    self._inner.match_guided_pairs_device(a.data_ptr(), ka.data_ptr(), oa.data_ptr(), na, b.data_ptr(),
                                                          kb.data_ptr(), ob.data_ptr(), nb, md.data_ptr(), n_pairs,
                                                          m_ab.data_ptr(), m_ba.data_ptr(), kind, threshold, ratio,
                                                          MATCH_MUTUAL if mutual else 0, best.data_ptr(), second.data_ptr(),
                                                          s.cuda_stream)
        return m_ab, m_ba, best, second

    def match_guided(self, desc_a, kps_a, desc_b, kps_b, model, kind="homography", threshold=None, ratio=0.8, mutual=True,
                     stream=None):
        """match_guided_batch for one pair (n_pairs = 1: all of desc_a against all of desc_b under `model` [3,3])."""
        import torch
        na, nb = int(desc_a.numel()) // 128, int(desc_b.numel()) // 128
        return self.match_guided_batch(desc_a, kps_a, torch.tensor([0, na]), desc_b, kps_b, torch.tensor([0, nb]), model, kind,
                                       threshold, ratio, mutual, stream)

    def quantize(self, desc, scale=Q8_SCALE):
        """8-bit descriptors (lf_mkd.h): [n,128] f32 -> [n,128] uint8, byte = clamp(rint(x * scale), -127, 127) + 128, a quarter
        of the bytes.  A numpy array goes through the host form and comes back as numpy; a torch tensor is quantised on the
        handle's device (moved there if it is elsewhere) on torch's current stream and comes back as a device tensor."""
        if isinstance(desc, np.ndarray) or not hasattr(desc, "data_ptr"):
            with self._lock:
                return self._inner.quantize(desc, scale)
        import torch
        dev = torch.device("cuda", self.device)
        s = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            d = desc.to(dev, torch.float32).reshape(-1, 128).contiguous()
            q = torch.empty((d.shape[0], 128), dtype=torch.uint8, device=dev)
            if d.shape[0]:
                with self._lock:
                    self._inner.quantize_descriptors_device(d.data_ptr(), d.shape[0], q.data_ptr(), scale, s.cuda_stream)
        return q

    @staticmethod
    def dequantize(q, scale=Q8_SCALE):
        """The f32 values an 8-bit descriptor stands for: (byte - 128) / scale.  numpy in, numpy out; torch in, torch out."""
        if isinstance(q, np.ndarray):
            return (q.astype(np.float32) - np.float32(128)) / np.float32(scale)
        import torch
        return (q.to(torch.float32) - 128.0) / float(scale)

    def match_q8(self, qa, qb, ratio=0.8, exclude=None, scores=False):
        """`match` over 8-bit descriptors (lf_mkd_match_q8_device): every similarity is an exact integer, so the decisions are
        those of an integer matrix product -- no rounding anywhere, ties to the highest index.  qa [na,128] / qb [nb,128]
        uint8, numpy arrays or torch tensors; exclude: None or (lo, hi), uint32 [na] each -- b rows lo[i] .. hi[i] - 1 are no
        candidates for row i.  Returns the list of (i, j) as `match` does; with scores=True (list, best [na] int32,
        second [na] int32) as numpy arrays."""
        import torch
        dev = torch.device("cuda", self.device)

        def rows(x):
            t = torch.from_numpy(np.ascontiguousarray(x, np.uint8)) if not hasattr(x, "data_ptr") else x
            return t.to(dev, torch.uint8).reshape(-1, 128).contiguous()

        with self._lock, torch.cuda.device(dev):
            a, b = rows(qa), rows(qb)
            na, nb = a.shape[0], b.shape[0]
            if na == 0:
                empty = np.zeros(0, np.int32)
                return ([], empty, empty) if scores else []
            lo = hi = None
            if exclude is not None:
                # (the uint32 bounds travel as their int32 bit patterns: torch's uint32 support is partial)
                lo, hi = (torch.from_numpy(np.ascontiguousarray(np.asarray(e.cpu() if hasattr(e, "cpu") else e))
                                           .astype(np.uint32).view(np.int32)).to(dev) for e in exclude)
                if lo.numel() != na or hi.numel() != na:
                    raise RuntimeError("match_q8: exclude needs one (lo, hi) per row of qa")
            m = torch.empty((na,), dtype=torch.int32, device=dev)
            best = torch.empty((na,), dtype=torch.int32, device=dev)
            second = torch.empty((na,), dtype=torch.int32, device=dev)
            s = torch.cuda.current_stream(dev)
            self._inner.match_q8_device(a.data_ptr(), na, b.data_ptr(), nb, m.data_ptr(), ratio,
                                        lo.data_ptr() if lo is not None else None, hi.data_ptr() if hi is not None else None,
                                        best.data_ptr(), second.data_ptr(), s.cuda_stream)
            s.synchronize()
            self._inner.synchronize()       # (torch's default stream is handle 0 = "the library's own stream" to the ABI)
            m, best, second = m.cpu().numpy(), best.cpu().numpy(), second.cpu().numpy()
        pairs = [(int(i), int(j)) for i, j in enumerate(m) if j >= 0]
        return (pairs, best, second) if scores else pairs

    def knn_q8(self, qa, qb, k, exclude=None, stream=None):
        """k-nearest-neighbour search over 8-bit descriptors (lf_mkd_knn_q8_device): for each row of qa its k best rows of qb,
        larger similarity first and among equal similarities the higher index first -- exact integers, one right answer.
        qa [na,128] / qb [nb,128] uint8, numpy arrays or torch tensors; 1 <= k <= KNN_MAX; exclude: None or (lo, hi),
        uint32 [na] each -- b rows lo[i] .. hi[i] - 1 are no candidates for row i.  Returns (index [na,k] int32,
        score [na,k] int32); slots beyond the number of candidates hold -1 / INT32_MIN.  Column 0 is `match_q8`'s answer at
        ratio 0 and its best, column 1's score its second.  With device tensors in, the result is device tensors and the call
        is asynchronous on `stream` (None: torch's current stream) and keeps nothing on the host; otherwise numpy arrays."""
        import torch
        dev = torch.device("cuda", self.device)
        on_device = all(hasattr(x, "data_ptr") and x.is_cuda for x in (qa, qb))

        def rows(x):
            t = torch.from_numpy(np.ascontiguousarray(x, np.uint8)) if not hasattr(x, "data_ptr") else x
            return t.to(dev, torch.uint8).reshape(-1, 128).contiguous()

        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            a, b = rows(qa), rows(qb)
            na, nb = a.shape[0], b.shape[0]
            index = torch.empty((na, int(k)), dtype=torch.int32, device=dev)
            score = torch.empty((na, int(k)), dtype=torch.int32, device=dev)
            lo = hi = None
            if exclude is not None:
                # (the uint32 bounds travel as their int32 bit patterns: torch's uint32 support is partial)
                lo, hi = (e.to(dev).reshape(-1).contiguous().view(torch.int32) if hasattr(e, "data_ptr") and e.is_cuda and e.element_size() == 4
                          else torch.from_numpy(np.ascontiguousarray(np.asarray(e.cpu() if hasattr(e, "cpu") else e))
                                                .astype(np.uint32).view(np.int32)).to(dev) for e in exclude)
                if lo.numel() != na or hi.numel() != na:
                    raise RuntimeError("knn_q8: exclude needs one (lo, hi) per row of qa")
            with self._lock:
                # (with na == 0 the call checks its arguments and writes nothing)
                self._inner.knn_q8_device(a.data_ptr(), na, b.data_ptr(), nb, int(k), index.data_ptr(), score.data_ptr(),
                                          lo.data_ptr() if lo is not None else None, hi.data_ptr() if hi is not None else None,
                                          s.cuda_stream)
            if on_device:
                return index, score
            s.synchronize()
            return index.cpu().numpy(), score.cpu().numpy()

    def match_q8_grouped(self, qa, qb, groups_b, ratio=0.8, exclude=None, scores=False, stream=None):
        """The ratio test against the best neighbour from ANOTHER group over 8-bit descriptors
        (lf_mkd_match_q8_grouped_device): Lowe's object-recognition rule for a pooled database, exact.  qa [na,128] /
        qb [nb,128] uint8 and groups_b [nb] (any uint32 ids: only their equality is used), numpy arrays or torch tensors;
        exclude: None or (lo, hi), uint32 [na] each -- b rows lo[i] .. hi[i] - 1 are no candidates for row i.
        Returns match [na] int32: the row's best row of qb (larger similarity first, among equal ones the higher index) if
        ratio <= 0 or best * ratio > rival, else -1, where rival is the best score among the rows whose group differs from
        the best's (INT32_MIN: none, the row is accepted).  With scores=True: (match, best, rival).  numpy in: numpy out
        (through the host form when there are no exclusion ranges); device tensors in: device tensors out, asynchronously
        on `stream` (None: torch's current stream) with nothing kept on the host."""
        if exclude is None and not any(hasattr(x, "data_ptr") for x in (qa, qb, groups_b)):
            with self._lock:
                m, best, rival = self._inner.match_q8_grouped(qa, qb, groups_b, ratio)
            return (m, best, rival) if scores else m
        import torch
        dev = torch.device("cuda", self.device)
        on_device = all(hasattr(x, "data_ptr") and x.is_cuda for x in (qa, qb))

        def rows(x):
            t = torch.from_numpy(np.ascontiguousarray(x, np.uint8)) if not hasattr(x, "data_ptr") else x
            return t.to(dev, torch.uint8).reshape(-1, 128).contiguous()

        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            a, b = rows(qa), rows(qb)
            na, nb = a.shape[0], b.shape[0]
            g = self._words(groups_b, dev)
            if g.numel() != nb:
                raise RuntimeError("match_q8_grouped: groups_b needs one id per row of qb")
            lo = hi = None
            if exclude is not None:
                lo, hi = (self._words(e, dev) for e in exclude)
                if lo.numel() != na or hi.numel() != na:
                    raise RuntimeError("match_q8_grouped: exclude needs one (lo, hi) per row of qa")
            m = torch.empty((na,), dtype=torch.int32, device=dev)
            best = torch.empty((na,), dtype=torch.int32, device=dev)
            rival = torch.empty((na,), dtype=torch.int32, device=dev)
            with self._lock:
                # (with na == 0 the call checks its arguments and writes nothing)
                self._inner.match_q8_grouped_device(a.data_ptr(), na, b.data_ptr(), nb, g.data_ptr(), m.data_ptr(), ratio,
                                                    lo.data_ptr() if lo is not None else None,
                                                    hi.data_ptr() if hi is not None else None, best.data_ptr(), rival.data_ptr(),
                                                    s.cuda_stream)
            if not on_device:
                s.synchronize()
                m, best, rival = m.cpu().numpy(), best.cpu().numpy(), rival.cpu().numpy()
        return (m, best, rival) if scores else m

    @staticmethod
    def _words(x, dev):
        """uint32 values as a contiguous int32 device tensor of their bit patterns (torch's uint32 support is partial)"""
        import torch
        if hasattr(x, "data_ptr") and x.is_cuda and x.element_size() == 4 and not x.is_floating_point():
            return x.to(dev).reshape(-1).contiguous().view(torch.int32)
        host = np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x)).astype(np.uint32).view(np.int32)
        return torch.from_numpy(host.reshape(-1)).to(dev)

    def vote_groups(self, match, groups_b, n_groups_b, groups_a=None, n_groups_a=1, stream=None):
        """The group-by-group vote table of a match array (lf_mkd_vote_groups_device): votes [n_groups_a, n_groups_b], where
        votes[ga, gb] counts the rows i with 0 <= match[i] < nb, ga = groups_a[i] < n_groups_a (groups_a None: 0) and
        gb = groups_b[match[i]] < n_groups_b; other rows are not counted.  match [na] int32 and the uint32 ids are numpy
        arrays or torch tensors.  With a device tensor `match` the table is an int32 device tensor (a count is at most
        2^31 - 1) and the call is asynchronous on `stream` (None: torch's current stream); otherwise a numpy uint32 array."""
        import torch
        dev = torch.device("cuda", self.device)
        on_device = hasattr(match, "data_ptr") and match.is_cuda
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            m = match if hasattr(match, "data_ptr") else torch.from_numpy(np.ascontiguousarray(match, np.int32))
            m = m.to(dev, torch.int32).reshape(-1).contiguous()
            gb = self._words(groups_b, dev)
            ga = self._words(groups_a, dev) if groups_a is not None else None
            if ga is not None and ga.numel() != m.numel():
                raise RuntimeError("vote_groups: groups_a needs one id per entry of match")
            votes = torch.empty((int(n_groups_a), int(n_groups_b)), dtype=torch.int32, device=dev)
            with self._lock:
                self._inner.vote_groups_device(m.data_ptr(), m.numel(), gb.data_ptr(), gb.numel(), int(n_groups_b),
                                               votes.data_ptr(), ga.data_ptr() if ga is not None else None, int(n_groups_a),
                                               s.cuda_stream)
            if on_device:
                return votes
            s.synchronize()
            return votes.cpu().numpy().view(np.uint32)

    def match_q8_batch(self, qa, offsets_a, qb, offsets_b, ratio=0.8, mutual=False, both=False, stream=None):
        """match_batch over 8-bit descriptors (lf_mkd_match_q8_pairs_device: one launch, three with `mutual`): the same
        layouts, the same offsets (any integer dtype, host or device), each pair decided exactly as `match_q8` decides it
        alone.  qa [Na,128] / qb [Nb,128] must be uint8 (what `quantize` returns); they are moved to the handle's device if
        they are elsewhere.  Returns device tensors (match_ab [Na] int32, match_ba [Nb] int32 or None, best [Na] int32,
        second [Na] int32): the scores are the exact integer similarities of the a -> b direction; rows outside every pair
        hold -1 / INT32_MIN.  Enqueued on `stream` (default: torch's current stream on the handle's device), asynchronously."""
        import torch
        dev = torch.device("cuda", self.device)
        n_pairs = int(offsets_a.numel()) - 1
        if n_pairs < 0 or int(offsets_b.numel()) != n_pairs + 1:
            raise RuntimeError("match_q8_batch: offsets_a and offsets_b need n_pairs + 1 entries each")
        for q in (qa, qb):
            if q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] != 128:
                raise RuntimeError("match_q8_batch: qa and qb must be uint8 [n, 128] (LocalFeatures.quantize)")
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):      # the copies and the fills below are ordered with the call
            a, b = qa.to(dev).contiguous(), qb.to(dev).contiguous()
            oa, ob = offsets_a.to(dev, torch.int64).contiguous(), offsets_b.to(dev, torch.int64).contiguous()
            na, nb = a.shape[0], b.shape[0]
            int32_min = -2 ** 31
            m_ab = torch.full((na,), -1, dtype=torch.int32, device=dev)
            m_ba = torch.full((nb,), -1, dtype=torch.int32, device=dev) if (both or mutual) else None
            best = torch.full((na,), int32_min, dtype=torch.int32, device=dev)
            second = torch.full((na,), int32_min, dtype=torch.int32, device=dev)
            if n_pairs and na and nb:       # (an empty side: every pair has too few candidates, the fills above are the answer)
                with self._lock:
                    self._inner.match_q8_pairs_device(a.data_ptr(), oa.data_ptr(), na, b.data_ptr(), ob.data_ptr(), nb, n_pairs,
                                                      m_ab.data_ptr(), m_ba.data_ptr() if m_ba is not None else None, ratio,
                                                      MATCH_MUTUAL if mutual else 0, best.data_ptr(), second.data_ptr(),
                                                      s.cuda_stream)
        return m_ab, m_ba, best, second

    def edge_layout(self, image_offsets, edge_image, n_rows_total=None, stream=None):
        """The edge layout of one side (lf_mkd_edge_layout_device): edge_offsets [n_edges + 1] int64 on the device, with
        edge_offsets[e + 1] - edge_offsets[e] = the rows of image edge_image[e] of the pool whose image m owns rows
        image_offsets[m] .. image_offsets[m + 1] - 1; an id at or beyond the number of images counts as an empty image.
        image_offsets [n_images + 1] and edge_image [n_edges] are integer tensors (host or device); n_rows_total is the
        pool's row count (None: 2^31 - 1, i.e. the offsets are taken as they are).  Asynchronous on `stream` (None: torch's
        current stream), nothing read back.  Call it once per side; the result is what match_q8_edges, gather_edge_rows, the
        verifiers and the guided calls take as that side's offsets."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            io = image_offsets.to(dev, torch.int64).reshape(-1).contiguous()
            ei = self._words(edge_image, dev)
            if io.numel() < 1:
                raise RuntimeError("edge_layout: image_offsets needs n_images + 1 entries")
            n_edges = ei.numel()
            out = torch.zeros((n_edges + 1,), dtype=torch.int64, device=dev)
            if n_edges:
                with self._lock:
                    self._inner.edge_layout_device(io.data_ptr(), io.numel() - 1, (1 << 31) - 1 if n_rows_total is None else
                                                   int(n_rows_total), ei.data_ptr(), n_edges, out.data_ptr(), s.cuda_stream)
        return out

    def gather_edge_rows(self, src, image_offsets, edge_image, edge_offsets, capacity=None, out=None, stream=None):
        """Rows of a pool brought into an edge layout (lf_mkd_gather_edge_rows_device): for edge e, out rows
        edge_offsets[e] .. get the rows of image edge_image[e] of `src` -- keypoints [N,5] float32 for the verifiers, or
        descriptor rows for a call that has no edges form.  src is a contiguous device tensor [N, ...] whose rows are a
        multiple of 4 bytes, at most 512.  capacity: the rows of the result (None reads the last layout offset back, which
        WAITS for the stream); out: a tensor to write into instead of a new zero-filled one.  Rows of no edge are untouched."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            x = src.to(dev).contiguous()
            n = x.shape[0]
            row_bytes = (x.numel() // n if n else int(np.prod(x.shape[1:]))) * x.element_size()
            io = image_offsets.to(dev, torch.int64).reshape(-1).contiguous()
            ei = self._words(edge_image, dev)
            eo = edge_offsets.to(dev, torch.int64).reshape(-1).contiguous()
            n_edges = ei.numel()
            if eo.numel() != n_edges + 1:
                raise RuntimeError("gather_edge_rows: edge_offsets needs n_edges + 1 entries")
            if out is None:
                cap = int(eo[-1].item()) if capacity is None else int(capacity)       # (.item() waits)
                out = torch.zeros((cap,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
            elif not (out.is_cuda and out.is_contiguous() and out.dtype == x.dtype and tuple(out.shape[1:]) == tuple(x.shape[1:])):
                raise RuntimeError("gather_edge_rows: out must be a contiguous device tensor of src's dtype and row shape")
            if n_edges and n and out.shape[0]:
                with self._lock:
                    self._inner.gather_edge_rows_device(x.data_ptr(), row_bytes, io.data_ptr(), io.numel() - 1, n, ei.data_ptr(),
                                                        eo.data_ptr(), out.shape[0], n_edges, out.data_ptr(), s.cuda_stream)
        return out

    def match_q8_edges(self, qa, offsets_a, qb, offsets_b, edge_a, edge_b, ratio=0.8, mutual=False, capacity_a=None,
                       capacity_b=None, stream=None):
        """Any pairs of images from one pool in one call (lf_mkd_match_q8_edges_device: one launch, three with `mutual`), no
        descriptor row copied.  qa [Na,128] / qb [Nb,128] uint8 device tensors (what `quantize` returns) are the two pools --
        they may be the same tensor --, offsets_a [n_images_a + 1] / offsets_b [n_images_b + 1] their image offsets, and edge e
        matches image edge_a[e] of qa against image edge_b[e] of qb, decided exactly as `match_q8` decides the two images
        alone; an image may sit on any number of edges.  Returns device tensors (match_ab, match_ba, best, second,
        edge_offsets_a, edge_offsets_b): the outputs live in the EDGE LAYOUT of their side (edge_layout) -- match_ab, best,
        second [capacity_a] int32 at edge_offsets_a[e] + r for row r of edge e's a image, match_ba [capacity_b] at
        edge_offsets_b[e] + r, values local to the other image -- which is the pair layout verify_*_batch and the guided calls
        take with those two offset tensors.  Entries of no edge hold -1 / INT32_MIN.
        capacity_a / capacity_b: the sizes of the output arrays, upper bounds of the layouts' totals.  None reads the last
        layout offset back, which WAITS for the stream; a caller who knows a bound (n_edges x its per-image cap) passes it and
        the call is asynchronous on `stream` (default: torch's current stream on the handle's device) from end to end."""
        import torch
        dev = torch.device("cuda", self.device)
        for q in (qa, qb):
            if q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] != 128:
                raise RuntimeError("match_q8_edges: qa and qb must be uint8 [n, 128] (LocalFeatures.quantize)")
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):      # the copies and the fills below are ordered with the call
            a, b = qa.to(dev).contiguous(), qb.to(dev).contiguous()
            oa = offsets_a.to(dev, torch.int64).reshape(-1).contiguous()
            ob = offsets_b.to(dev, torch.int64).reshape(-1).contiguous()
            ea, eb = self._words(edge_a, dev), self._words(edge_b, dev)
            n_edges = ea.numel()
            if eb.numel() != n_edges:
                raise RuntimeError("match_q8_edges: edge_a and edge_b need one id per edge each")
            if oa.numel() < 1 or ob.numel() < 1:
                raise RuntimeError("match_q8_edges: offsets_a and offsets_b need n_images + 1 entries each")
            na, nb = a.shape[0], b.shape[0]
            la = self.edge_layout(oa, ea, na, stream=s)
            lb = self.edge_layout(ob, eb, nb, stream=s)
            cap_a = int(la[-1].item()) if capacity_a is None else int(capacity_a)     # (.item() waits)
            cap_b = int(lb[-1].item()) if capacity_b is None else int(capacity_b)
            int32_min = -2 ** 31
            m_ab = torch.full((cap_a,), -1, dtype=torch.int32, device=dev)
            m_ba = torch.full((cap_b,), -1, dtype=torch.int32, device=dev)
            best = torch.full((cap_a,), int32_min, dtype=torch.int32, device=dev)
            second = torch.full((cap_a,), int32_min, dtype=torch.int32, device=dev)
            if n_edges and na and nb:       # (an empty pool: every edge has too few candidates, the fills above are the answer)
                with self._lock:
                    self._inner.match_q8_edges_device(a.data_ptr(), oa.data_ptr(), oa.numel() - 1, na, b.data_ptr(), ob.data_ptr(),
                                                      ob.numel() - 1, nb, ea.data_ptr(), eb.data_ptr(), la.data_ptr(), cap_a,
                                                      n_edges, m_ab.data_ptr(), lb.data_ptr(), cap_b, m_ba.data_ptr(), ratio,
                                                      MATCH_MUTUAL if mutual else 0, best.data_ptr(), second.data_ptr(),
                                                      s.cuda_stream)
        return m_ab, m_ba, best, second, la, lb

    def build_tracks(self, image_offsets, edge_a, edge_b, layout_a, match, capacity=None, into=None, stats=True, n_rows=None,
                     stream=None):
        """Feature tracks of a matched collection (lf_mkd_build_tracks_device): the connected components of the links a match
        array holds between the rows of one pool.  image_offsets [n_images + 1], edge_a / edge_b [n_edges] and layout_a
        [n_edges + 1] are what match_q8_edges took and returned; match [>= capacity] int32 lives in the a side's edge layout
        -- match_q8_edges' match_ab, the mutual filter's output or a verifier's `verified`, as it is (an entry outside
        0 .. nB - 1 is no link).  capacity: the entries of `match` the layout may use (None: all of them).
        Returns device tensors (track, length, dup): track [n_rows] int32, the smallest pool row of every row's component (a
        row on no link is its own track); length / dup [n_rows] int32, at a label the track's rows and its conflicting rows --
        the rows beyond the first that one image has in it, so dup == 0 is a consistent track -- and 0 elsewhere; both None
        with stats=False.  into: an earlier call's `track`, to which the links are ADDED in place (LF_MKD_TRACKS_ACCUMULATE) and
        which is returned; links given in several calls yield the labels of one call with all of them.  n_rows: the pool's
        rows (None: into's length, else the last image offset read back, which WAITS for the stream).  Otherwise nothing is
        read back: asynchronous on `stream` (default: torch's current stream on the handle's device), capturable."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            io = image_offsets.to(dev, torch.int64).reshape(-1).contiguous()
            ea, eb = self._words(edge_a, dev), self._words(edge_b, dev)
            la = layout_a.to(dev, torch.int64).reshape(-1).contiguous()
            n_edges = ea.numel()
            if eb.numel() != n_edges or la.numel() != n_edges + 1:
                raise RuntimeError("build_tracks: edge_a and edge_b need one id per edge each, layout_a n_edges + 1 entries")
            if io.numel() < 1:
                raise RuntimeError("build_tracks: image_offsets needs n_images + 1 entries")
            if not (hasattr(match, "is_cuda") and match.is_cuda and match.dtype == torch.int32 and match.dim() == 1
                    and match.is_contiguous()):
                raise RuntimeError("build_tracks: match must be a contiguous int32 device tensor in the a side's edge layout")
            cap = match.numel() if capacity is None else int(capacity)
            if cap > match.numel():
                raise RuntimeError("build_tracks: capacity is larger than match")
            if into is not None:
                if not (into.is_cuda and into.dtype == torch.int32 and into.dim() == 1 and into.is_contiguous()):
                    raise RuntimeError("build_tracks: into must be a contiguous int32 device tensor (an earlier call's track)")
                if n_rows is not None and int(n_rows) != into.numel():
                    raise RuntimeError("build_tracks: into needs n_rows entries")
                track, n = into, into.numel()
            else:
                n = int(io[-1].item()) if n_rows is None else int(n_rows)             # (.item() waits)
                track = torch.empty((n,), dtype=torch.int32, device=dev)
            length = torch.empty((n,), dtype=torch.int32, device=dev) if stats else None
            dup = torch.empty((n,), dtype=torch.int32, device=dev) if stats else None
            if n:
                with self._lock:
                    self._inner.build_tracks_device(io.data_ptr(), io.numel() - 1, n, ea.data_ptr(), eb.data_ptr(), la.data_ptr(),
                                                    cap, n_edges, match.data_ptr(), track.data_ptr(),
                                                    length.data_ptr() if stats else None, dup.data_ptr() if stats else None,
                                                    TRACKS_ACCUMULATE if into is not None else 0, s.cuda_stream)
        return track, length, dup

    def track_table(self, track, length, dup=None, image_offsets=None, min_len=2, consistent=True, track_capacity=None,
                    obs_capacity=None, stream=None):
        """The track table of build_tracks' result (lf_mkd_track_table_device): per track the list of its observations, as a
        CSR table made on the device.  track / length / dup [N] are int32 device tensors as build_tracks returned them.  A
        track enters iff its length is at least min_len and, with `consistent`, its dup is 0 (dup is then required); the
        tracks come in the order of their smallest row, a track's rows ascending.
        Returns device tensors (offsets, rows, images, row_track, counts): offsets [track_capacity + 1] int64 -- track i's
        observations are rows[offsets[i] : offsets[i + 1]], entries beyond the last track repeat the number of observations;
        rows [obs_capacity] int32, pool rows (entries beyond the observations are left as allocated); images [obs_capacity]
        int32, the image of each observation (-1: a row of no image), None without image_offsets; row_track [N] int32, per pool
        row the table index of its track or -1; counts [4] int32: the tracks and the observations in the table, and the
        tracks and (saturated at 2^32 - 1, as a bit pattern) the observations wanted -- they differ when a capacity cut the
        table, which keeps whole tracks only.  The default capacities, N // min_len and N, always suffice.
        Nothing is read back: asynchronous on `stream` (default: torch's current stream on the handle's device), capturable
        once a call of this size has been made."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        min_len = int(min_len)
        if min_len < 1:
            raise RuntimeError("track_table: min_len must be at least 1")
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == torch.int32 and x.dim() == 1 and x.is_contiguous()
            if not (ok(track) and ok(length) and (dup is None or ok(dup))):
                raise RuntimeError("track_table: track, length and dup must be contiguous int32 device tensors")
            n = track.numel()
            if length.numel() != n or (dup is not None and dup.numel() != n):
                raise RuntimeError("track_table: length and dup need one entry per row of track")
            if consistent and dup is None:
                raise RuntimeError("track_table: consistent=True needs dup")
            t_cap = n // min_len if track_capacity is None else int(track_capacity)
            o_cap = n if obs_capacity is None else int(obs_capacity)
            io = image_offsets.to(dev, torch.int64).reshape(-1).contiguous() if image_offsets is not None else None
            if io is not None and io.numel() < 1:
                raise RuntimeError("track_table: image_offsets needs n_images + 1 entries")
            offsets = torch.empty((t_cap + 1,), dtype=torch.int64, device=dev)
            rows = torch.empty((o_cap,), dtype=torch.int32, device=dev)
            images = torch.empty((o_cap,), dtype=torch.int32, device=dev) if io is not None else None
            row_track = torch.empty((n,), dtype=torch.int32, device=dev)
            counts = torch.empty((4,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.track_table_device(ptr(io), io.numel() - 1 if io is not None else 0, n, ptr(track), ptr(length),
                                               ptr(dup), min_len, TRACK_TABLE_CONSISTENT if consistent else 0, t_cap, o_cap,
                                               offsets.data_ptr(), ptr(rows), ptr(images), ptr(row_track), counts.data_ptr(),
                                               s.cuda_stream)
        return offsets, rows, images, row_track, counts

    def gather_track_rows(self, src, rows, counts, out=None, stream=None):
        """Rows of a pool brought into a track table's order (lf_mkd_gather_track_rows_device): out[k] = src[rows[k]] for
        k < min(counts[1], len(rows)) -- keypoints [N,5] float32, q8 rows, or any contiguous device tensor [N, ...] whose rows
        are a multiple of 4 bytes, at most 512.  rows / counts are what track_table returned.  out: a tensor of len(rows) rows to
        write into instead of a new zero-filled one; rows beyond the count are untouched, an index outside the pool gives a
        zero row.  One launch, nothing read back."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            x = src.to(dev).contiguous()
            n = x.shape[0]
            row_bytes = int(np.prod(x.shape[1:])) * x.element_size()
            if not (rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous()):
                raise RuntimeError("gather_track_rows: rows must be a contiguous int32 device tensor (track_table's rows)")
            if not (counts.is_cuda and counts.dtype == torch.int32 and counts.numel() == 4 and counts.is_contiguous()):
                raise RuntimeError("gather_track_rows: counts must be track_table's counts")
            cap = rows.numel()
            if out is None:
                out = torch.zeros((cap,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
            elif not (out.is_cuda and out.is_contiguous() and out.dtype == x.dtype and tuple(out.shape[1:]) == tuple(x.shape[1:])
                      and out.shape[0] >= cap):
                raise RuntimeError("gather_track_rows: out must be a contiguous device tensor of src's dtype and row shape with "
                                   "at least len(rows) rows")
            with self._lock:
                self._inner.gather_track_rows_device(x.data_ptr() if n else None, row_bytes, n, rows.data_ptr() if cap else None,
                                                     counts.data_ptr(), cap, out.data_ptr() if cap else None, s.cuda_stream)
        return out

    def link_table(self, image_offsets, edge_a, edge_b, layout_a, match, min_links=0, local=False, capacity=None,
                   link_capacity=None, n_rows=None, kept_match=False, stream=None):
        """The link table of an edge list's matches (lf_mkd_link_table_device): per edge the compact list of its
        correspondences, as a CSR table made on the device.  image_offsets, edge_a / edge_b, layout_a and match are what
        build_tracks takes, read by the same rule: entry lo + r of edge e links rows r of its a image and match[lo + r] of its b
        image iff that value is a row of the b image.  An edge enters iff it has at least min_links links (0: every edge);
        link_capacity keeps whole edges only.  capacity: the entries of `match` the layout may use (None: all of them);
        link_capacity: None is capacity, which always suffices; n_rows: the pool's rows (None: the last image offset read back,
        which WAITS for the stream).
        Returns device tensors (link_offsets, link_a, link_b, link_edge, edge_links, match_kept, counts): link_offsets
        [n_edges + 1] int64 -- edge e's links are link_a / link_b [link_offsets[e] : link_offsets[e + 1]], an edge that is not
        kept has an empty range; link_a / link_b [link_capacity] int32, pool rows -- with local=True rows within their images
        -- in ascending row of a (entries beyond the links are left as allocated); link_edge [link_capacity] int32, the edge of
        each link; edge_links [n_edges] int32, every edge's links, selected or not; match_kept: None, or with kept_match=True a
        new tensor like `match` in which everything but the kept edges' links is -1 (entries of no edge are -1 too), or with
        kept_match=match (or any int32 tensor of its size) that tensor, written in place; counts [4] int32: the kept edges,
        the links in the table, the selected edges and (saturated at 2^32 - 1, as a bit pattern) the links wanted.
        Without local=True, gather_track_rows(keypoints, link_a, counts) and (..., link_b, counts) bring the keypoints into the
        table's order; build_tracks(..., match_kept) builds the tracks of the kept edges alone.  Given n_rows nothing is read
        back: asynchronous on `stream` (default: torch's current stream on the handle's device), capturable once a call of
        this size has been made."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        min_links = int(min_links)
        if not 0 <= min_links < 2 ** 32:
            raise RuntimeError("link_table: min_links must be in [0, 2^32)")
        with torch.cuda.device(dev), torch.cuda.stream(s):
            io = image_offsets.to(dev, torch.int64).reshape(-1).contiguous()
            ea, eb = self._words(edge_a, dev), self._words(edge_b, dev)
            la = layout_a.to(dev, torch.int64).reshape(-1).contiguous()
            n_edges = ea.numel()
            if eb.numel() != n_edges or la.numel() != n_edges + 1:
                raise RuntimeError("link_table: edge_a and edge_b need one id per edge each, layout_a n_edges + 1 entries")
            if io.numel() < 1:
                raise RuntimeError("link_table: image_offsets needs n_images + 1 entries")
            ok = lambda x: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == torch.int32 and x.dim() == 1 and x.is_contiguous()
            if not ok(match):
                raise RuntimeError("link_table: match must be a contiguous int32 device tensor in the a side's edge layout")
            cap = match.numel() if capacity is None else int(capacity)
            if cap > match.numel():
                raise RuntimeError("link_table: capacity is larger than match")
            l_cap = cap if link_capacity is None else int(link_capacity)
            n = int(io[-1].item()) if n_rows is None else int(n_rows)                 # (.item() waits)
            if kept_match is True:
                kept = torch.full_like(match, -1)
            elif kept_match is False or kept_match is None:
                kept = None
            elif ok(kept_match) and kept_match.numel() == match.numel():
                kept = kept_match
            else:
                raise RuntimeError("link_table: kept_match must be a bool or a contiguous int32 device tensor of match's size")
            offsets = torch.empty((n_edges + 1,), dtype=torch.int64, device=dev)
            link_a = torch.empty((l_cap,), dtype=torch.int32, device=dev)
            link_b = torch.empty((l_cap,), dtype=torch.int32, device=dev)
            link_edge = torch.empty((l_cap,), dtype=torch.int32, device=dev)
            edge_links = torch.empty((n_edges,), dtype=torch.int32, device=dev)
            counts = torch.empty((4,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.link_table_device(io.data_ptr(), io.numel() - 1, n, ptr(ea), ptr(eb), la.data_ptr(), cap, n_edges,
                                              ptr(match) if n_edges else None, min_links, LINK_TABLE_LOCAL if local else 0, l_cap,
                                              offsets.data_ptr(), ptr(link_a), ptr(link_b), ptr(link_edge), ptr(edge_links),
                                              ptr(kept), counts.data_ptr(), s.cuda_stream)
        return offsets, link_a, link_b, link_edge, edge_links, kept, counts

    def select_edges(self, votes, k, min_votes=1, skip_self=False, unique=False, capacity=None, stream=None):
        """Candidate edges of a vote table (lf_mkd_select_edges_device): per row of votes [n_a, n_b] -- what vote_groups
        returns, or any 32-bit integer tensor or array, read as uint32 -- the k columns with the most votes among those with
        at least min_votes (0 admits columns without a vote) and, with skip_self, other than the row's own; larger votes
        first, among equal votes the LOWER column first.  Every pick (i, j) is the edge (i, j); with unique=True (one pool,
        n_a == n_b) an unordered pair that either image picked appears once, as (smaller, larger), so a mutual pick is not
        matched twice.  capacity: the edges kept (None: n_a * k, which always suffices).
        Returns device tensors (edge_a, edge_b, edge_votes, rank, rank_votes, counts): edge_a / edge_b [capacity] int32, the
        edges in the order row, then rank, and behind them -1 (the bit pattern 0xFFFFFFFF), which names an empty image to
        edge_layout / match_q8_edges / build_tracks / link_table -- pass them whole; edge_votes [capacity] int32, the votes of
        the pick that made each edge (as a bit pattern), 0 behind them; rank [n_a, k] int32, the picks of every row in order,
        -1 behind them; rank_votes [n_a, k] int32 (bit patterns), their votes; counts [4] int32: the edges kept, the edges
        wanted, the picks and the rows with at least one pick.  Nothing is read back: asynchronous on `stream` (default:
        torch's current stream on the handle's device), capturable once a call of this size has been made."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        k, min_votes = int(k), int(min_votes)
        if not 0 <= min_votes < 2 ** 32:
            raise RuntimeError("select_edges: min_votes must be in [0, 2^32)")
        if not hasattr(votes, "data_ptr"):
            votes = torch.from_numpy(np.ascontiguousarray(np.asarray(votes)).astype(np.uint32).view(np.int32))
        if votes.dim() != 2 or votes.element_size() != 4 or votes.is_floating_point():
            raise RuntimeError("select_edges: votes must be a 32-bit integer [n_a, n_b] table (LocalFeatures.vote_groups)")
        with torch.cuda.device(dev), torch.cuda.stream(s):
            v = votes.to(dev).contiguous()
            n_a, n_b = v.shape
            cap = n_a * max(k, 0) if capacity is None else int(capacity)
            edge_a = torch.empty((cap,), dtype=torch.int32, device=dev)
            edge_b = torch.empty((cap,), dtype=torch.int32, device=dev)
            edge_votes = torch.empty((cap,), dtype=torch.int32, device=dev)
            rank = torch.empty((n_a, max(k, 0)), dtype=torch.int32, device=dev)
            rank_votes = torch.empty((n_a, max(k, 0)), dtype=torch.int32, device=dev)
            counts = torch.empty((4,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x.numel() else None
            with self._lock:
                self._inner.select_edges_device(ptr(v), n_a, n_b, k, min_votes,
                                                (SELECT_SKIP_SELF if skip_self else 0) | (SELECT_UNIQUE if unique else 0), cap,
                                                ptr(rank), ptr(rank_votes), ptr(edge_a), ptr(edge_b), ptr(edge_votes),
                                                counts.data_ptr(), s.cuda_stream)
        return edge_a, edge_b, edge_votes, rank, rank_votes, counts

    def covisibility(self, offsets, images, counts, n_images, edges=None, into=None, stream=None):
        """The covisibility table of a track table (lf_mkd_covisibility_device): per pair of images the number of tracks both
        see, on the diagonal the number of tracks an image sees.  offsets [track_capacity + 1] int64, images [obs_capacity]
        int32 and counts are what track_table returned (with image_offsets given); an observation counts once per run of
        equal images in its track, ids outside 0 .. n_images - 1 (track_table's -1) never.  edges: (edge_a, edge_b), 32-bit
        ids of pairs whose two entries are set to 0 afterwards -- the list a round of matching used, select_edges' padded
        arrays as they are --, so that what is left are the pairs that share tracks without having been matched: the table
        select_edges takes for a second round.  into: an earlier call's table [n_images, n_images], to which the counts are
        ADDED in place (LF_MKD_COVIS_ACCUMULATE; the mask then applies to the sum) and which is returned; the tracks of one
        table given in several calls yield the table of one call with all of them.
        Returns an int32 device tensor [n_images, n_images] (counts as bit patterns of uint32).  Nothing is read back:
        asynchronous on `stream` (default: torch's current stream on the handle's device), capturable once a call of this
        size has been made."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        n = int(n_images)
        if n < 0:
            raise RuntimeError("covisibility: n_images must not be negative")
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.dim() == 1 and x.is_contiguous()
            if not (ok(offsets, torch.int64) and offsets.numel() >= 1 and ok(images, torch.int32) and ok(counts, torch.int32)
                    and counts.numel() >= 2):
                raise RuntimeError("covisibility: offsets (int64), images (int32) and counts (int32) must be contiguous device "
                                   "tensors as track_table returned them")
            ea = eb = None
            if edges is not None:
                ea, eb = self._words(edges[0], dev), self._words(edges[1], dev)
                if ea.numel() != eb.numel():
                    raise RuntimeError("covisibility: edges needs one id per edge in each of its two arrays")
            if into is not None:
                if not (into.is_cuda and into.dtype == torch.int32 and tuple(into.shape) == (n, n) and into.is_contiguous()):
                    raise RuntimeError("covisibility: into must be a contiguous int32 [n_images, n_images] device tensor")
                covis = into
            else:
                covis = torch.empty((n, n), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.covisibility_device(offsets.data_ptr(), offsets.numel() - 1, ptr(images), images.numel(),
                                                counts.data_ptr(), n, ptr(ea), ptr(eb), ea.numel() if ea is not None else 0,
                                                COVIS_ACCUMULATE if into is not None else 0, ptr(covis), s.cuda_stream)
        return covis

    def two_view_pose(self, F, intrinsics, kps, edges=None, links=None, min_parallax_deg=1.0, sigma=True, points=True,
                      stream=None):
        """The relative pose of calibrated image pairs from their fundamental matrices (lf_mkd_two_view_pose_device): x_b =
        R x_a + t with |t| = 1, chosen among the four candidates of E = K_b^T F K_a by a vote of the pair's correspondences,
        and those correspondences triangulated (include/lf_mkd.h states the algorithm).  Two forms:

        * Device tensors, many edges: F [n_edges, 3, 3] (or [n_edges, 9]) float32 as verify_fundamental_batch returns it,
          intrinsics [n_images, 4] float32 (fx, fy, cx, cy per image), kps [rows, 5] float32 (the pool), edges = (edge_a,
          edge_b) 32-bit image ids, links = (link_offsets [n_edges + 1] int64, link_a, link_b int32 pool rows) as
          link_table(local=False) returns them.  Returns device tensors (R [n_edges, 3, 3], t [n_edges, 3], stats
          [n_edges, 4] int32 -- links in front, the best other candidate's, the candidate (-1: no pose), links with at least
          min_parallax_deg of parallax --, sigma [n_edges, 3] or None, points [links, 4] or None: X, Y, Z in camera a's frame
          and the cosine of the parallax angle, (0, 0, 0, 2) where a link is not in front).  Nothing is read back:
          asynchronous on `stream` (default: torch's current stream on the handle's device), capturable.
        * One pair as host arrays: F [3, 3], intrinsics = (K_a, K_b) each (fx, fy, cx, cy), kps = (kp_a, kp_b) keypoint lists
          or [n, 4|5] arrays, links = the (i, j) matches (verify_fundamental's inliers); edges stays None.  Returns numpy (R
          [3, 3], t [3], stats [4] int64, sigma [3] or None, points [len(kp_a), 4] or None), synchronously."""
        if edges is None:
            a, b = _keypoints_to_array(kps[0]), _keypoints_to_array(kps[1])
            m = np.full(len(a), -1, np.int32)
            for i, j in links:
                if not (0 <= i < len(a) and 0 <= j < len(b)):
                    raise RuntimeError("two_view_pose: match (%d, %d) outside the keypoint lists" % (i, j))
                m[i] = j
            with self._lock:
                R, t, st, sg, pts = self._inner.two_view_pose(F, intrinsics[0], intrinsics[1], a.view(np.float32).reshape(-1, 5),
                                                              b.view(np.float32).reshape(-1, 5), m, min_parallax_deg, 0, points)
            st = st.astype(np.int64)
            st[2] = -1 if st[2] == 0xFFFFFFFF else st[2]
            return R, t, st, sg if sigma else None, pts
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            ea, eb = self._words(edges[0], dev), self._words(edges[1], dev)
            n_edges = ea.numel()
            off, la, lb = links
            if not (ok(F, torch.float32) and F.numel() == 9 * n_edges and eb.numel() == n_edges):
                raise RuntimeError("two_view_pose: F must be a contiguous float32 device tensor with 9 values per edge, edges one "
                                   "id per edge in each of its two arrays")
            if not (ok(intrinsics, torch.float32) and intrinsics.dim() == 2 and intrinsics.shape[1] == 4):
                raise RuntimeError("two_view_pose: intrinsics must be a contiguous float32 [n_images, 4] device tensor")
            if not (ok(kps, torch.float32) and kps.dim() == 2 and kps.shape[1] == 5):
                raise RuntimeError("two_view_pose: kps must be a contiguous float32 [rows, 5] device tensor")
            if not (ok(off, torch.int64) and off.numel() == n_edges + 1 and ok(la, torch.int32) and ok(lb, torch.int32)
                    and la.numel() == lb.numel()):
                raise RuntimeError("two_view_pose: links must be (offsets int64 [n_edges + 1], link_a int32, link_b int32) device "
                                   "tensors as link_table returned them")
            cap = la.numel()
            R = torch.empty((n_edges, 3, 3), dtype=torch.float32, device=dev)
            t = torch.empty((n_edges, 3), dtype=torch.float32, device=dev)
            st = torch.empty((n_edges, 4), dtype=torch.int32, device=dev)
            sg = torch.empty((n_edges, 3), dtype=torch.float32, device=dev) if sigma else None
            pts = torch.empty((cap, 4), dtype=torch.float32, device=dev) if points else None
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.two_view_pose_device(ptr(kps), kps.shape[0], ptr(ea), ptr(eb), n_edges, ptr(intrinsics),
                                                 intrinsics.shape[0], ptr(F), off.data_ptr(), ptr(la), ptr(lb), cap, ptr(R), ptr(t),
                                                 ptr(st), ptr(sg), ptr(pts), min_parallax_deg, 0, s.cuda_stream)
        return R, t, st, sg, pts

    def triangulate_tracks(self, kps, table, intrinsics, poses, max_reproj_px=4.0, rounds=2, err=True, obs_state=True,
                           stream=None):
        """The 3-D point of every track of a track table under known camera poses (lf_mkd_triangulate_tracks_device): pair
        hypotheses among a track's first usable observations, a midpoint least squares over the winner's inliers, `rounds`
        (0 .. 4) trimming rounds at max_reproj_px, and the parallax of the inliers (include/lf_mkd.h states the algorithm).
        kps [rows, 5] float32 is the pool; table = (offsets, rows, images, counts) as track_table returned them with
        image_offsets given (its 5-tuple passes as it is); intrinsics [n_images, 4] float32 = fx, fy, cx, cy; poses
        [n_images, 12] float32 = R row-major, then t, world to camera: x_cam = R X + t -- two_view_pose's R and t with camera
        a at [I | 0].  An image whose R is all zero is not
        registered: its observations are not used, so a partial pose array passes as it is.
        Returns device tensors (points [track_capacity, 4] float32: X, Y, Z and the cosine of the parallax angle, (0, 0, 0, 2)
        for no point; stats [track_capacity, 4] int32: usable observations, inliers, reason (0 point, 1 fewer than two usable,
        2 singular, 3 fewer than two inliers), the winning pair ci << 16 | cj or -1; err [track_capacity, 2] float32 (rms and
        largest inlier reprojection error, px) or None; obs_state [obs_capacity] int32 (0 not usable, 1 usable, 2 inlier) or
        None).  Rows beyond the table's tracks and observation entries outside every track are left as allocated.  Nothing is
        read back: asynchronous on `stream` (default: torch's current stream on the handle's device), capturable."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if len(table) == 5:
            offsets, rows, images, _, counts = table
        else:
            offsets, rows, images, counts = table
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            if not (ok(offsets, torch.int64) and offsets.dim() == 1 and offsets.numel() >= 1 and ok(rows, torch.int32)
                    and images is not None and ok(images, torch.int32) and rows.numel() == images.numel()
                    and ok(counts, torch.int32) and counts.numel() >= 2):
                raise RuntimeError("triangulate_tracks: table must be (offsets int64, rows int32, images int32, counts int32) "
                                   "contiguous device tensors as track_table returned them with image_offsets")
            if not (ok(kps, torch.float32) and kps.dim() == 2 and kps.shape[1] == 5):
                raise RuntimeError("triangulate_tracks: kps must be a contiguous float32 [rows, 5] device tensor")
            if not (ok(intrinsics, torch.float32) and intrinsics.dim() == 2 and intrinsics.shape[1] == 4):
                raise RuntimeError("triangulate_tracks: intrinsics must be a contiguous float32 [n_images, 4] device tensor")
            if not (ok(poses, torch.float32) and poses.numel() == 12 * intrinsics.shape[0]):
                raise RuntimeError("triangulate_tracks: poses must be a contiguous float32 [n_images, 12] device tensor")
            tcap, ocap = offsets.numel() - 1, rows.numel()
            pts = torch.empty((tcap, 4), dtype=torch.float32, device=dev)
            st = torch.empty((tcap, 4), dtype=torch.int32, device=dev)
            er = torch.empty((tcap, 2), dtype=torch.float32, device=dev) if err else None
            os_ = torch.empty((ocap,), dtype=torch.int32, device=dev) if obs_state else None
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.triangulate_tracks_device(ptr(kps), kps.shape[0], offsets.data_ptr(), tcap, ptr(rows), ptr(images),
                                                      ocap, counts.data_ptr(), ptr(intrinsics), ptr(poses), intrinsics.shape[0],
                                                      ptr(pts), ptr(st), ptr(er), ptr(os_), max_reproj_px, rounds, 0,
                                                      s.cuda_stream)
        return pts, st, er, os_

    def resect_cameras(self, kps, offsets, row_track, points, table_counts, intrinsics, poses, max_reproj_px=4.0,
                       min_parallax_deg=0.0, n_samples=512, min_inliers=12, rounds=3, seed=0, resect_all=False, out=None,
                       stream=None):
        """The absolute pose of every image that is not registered yet (lf_mkd_resect_cameras_device): P3P samples over the
        keypoints an image owns in tracks that have a 3-D point, scored by reprojection inliers at max_reproj_px, a Gauss-Newton
        refit of `rounds` (0 .. 4) steps, the pose kept with at least max(min_inliers, 3) inliers (include/lf_mkd.h states the
        algorithm).  kps [rows, 5] float32 is the pool and offsets [n_images + 1] int64 its image offsets; row_track [rows]
        int32 is track_table's inverse map; points [track_capacity, 4] float32 and table_counts are triangulate_tracks' points
        and the table's counts; intrinsics [n_images, 4] float32; poses [n_images, 12] float32 = R row-major, then t, world to
        camera, an all-zero R for an image that is not registered -- those are resected, every other image's pose is copied
        (resect_all: every image is resected).  `out` is the pose tensor to write, `poses` itself for an in-place call
        (default: a new tensor).  Returns device tensors (poses [n_images, 12] float32, all zero where no pose was found;
        stats [n_images, 4] int32: correspondences, inliers, reason (0 pose, 1 not a candidate, 2 fewer than three
        correspondences or no candidate, 3 fewer than the minimum inliers), the winning candidate or -1; err [n_images, 2]
        float32: rms and largest inlier reprojection error, px; row_state [rows] int32: 0 no correspondence, 1 correspondence,
        2 inlier, written in the ranges of the resected images only, -1 elsewhere).  Nothing is read back: asynchronous on
        `stream` (default: torch's current stream on the handle's device), capturable once warmed up."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            if not (ok(kps, torch.float32) and kps.dim() == 2 and kps.shape[1] == 5):
                raise RuntimeError("resect_cameras: kps must be a contiguous float32 [rows, 5] device tensor")
            if not (ok(offsets, torch.int64) and offsets.dim() == 1 and offsets.numel() >= 1):
                raise RuntimeError("resect_cameras: offsets must be a contiguous int64 [n_images + 1] device tensor")
            n_images, n_rows = offsets.numel() - 1, kps.shape[0]
            if not (ok(row_track, torch.int32) and row_track.numel() == n_rows):
                raise RuntimeError("resect_cameras: row_track must be a contiguous int32 [rows] device tensor")
            if not (ok(points, torch.float32) and points.dim() == 2 and points.shape[1] == 4 and ok(table_counts, torch.int32)
                    and table_counts.numel() >= 1):
                raise RuntimeError("resect_cameras: points must be float32 [track_capacity, 4] and table_counts int32 device "
                                   "tensors as triangulate_tracks and track_table returned them")
            if not (ok(intrinsics, torch.float32) and intrinsics.numel() == 4 * n_images and ok(poses, torch.float32)
                    and poses.numel() == 12 * n_images):
                raise RuntimeError("resect_cameras: intrinsics must be float32 [n_images, 4] and poses float32 [n_images, 12] "
                                   "contiguous device tensors")
            if out is None:
                out = torch.empty((n_images, 12), dtype=torch.float32, device=dev)
            elif not (ok(out, torch.float32) and out.numel() == 12 * n_images):
                raise RuntimeError("resect_cameras: out must be a contiguous float32 [n_images, 12] device tensor")
            st = torch.empty((n_images, 4), dtype=torch.int32, device=dev)
            er = torch.empty((n_images, 2), dtype=torch.float32, device=dev)
            rs = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.resect_cameras_device(ptr(kps), offsets.data_ptr(), n_images, n_rows, ptr(row_track), ptr(points),
                                                  points.shape[0], table_counts.data_ptr(), ptr(intrinsics), ptr(poses), ptr(out),
                                                  ptr(st), ptr(er), ptr(rs), max_reproj_px, min_parallax_deg, n_samples,
                                                  min_inliers, rounds, seed, RESECT_ALL if resect_all else 0, s.cuda_stream)
        return out, st, er, rs

    def track_descriptors(self, q8, table, obs_state=None, min_state=2, points=None, min_parallax_deg=0.0, scale=Q8_SCALE,
                          stats=False, stream=None):
        """One 8-bit descriptor per track of a track table (lf_mkd_track_descriptors_device): the sum of the centred rows of
        the track's observations, normalised and quantised again with `scale` -- the descriptors a reconstruction exports with
        its points, so that `localize` needs neither the pool's rows nor the table (include/lf_mkd.h states the contract).
        q8 [rows, 128] uint8 is the pool, quantised; table = (offsets, rows, images, counts) or track_table's 5-tuple (the
        images are not read).  obs_state [obs_capacity] int32, triangulate_tracks' or bundle_adjust's: an observation
        contributes iff its state is at least min_state (0 .. 2; None: every observation); points [track_capacity, 4] float32:
        a track is described iff its point is finite with a parallax cosine <= cos(min_parallax_deg), resect_cameras' rule
        (None: every track).  Returns the device tensor desc [track_capacity, 128] uint8 -- the zero row, all bytes 128, for a
        track that is not described, has no contributor or whose rows cancel, and for the rows beyond the table's tracks --
        and with stats=True (desc, stats [track_capacity, 2] int32 = contributors, the smallest similarity of a contributor
        with its track's row; INT32_MIN for a zero row).  Nothing is read back: asynchronous on `stream` (default: torch's
        current stream on the handle's device), capturable."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        offsets, rows, counts = table[0], table[1], table[-1]
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            if not (len(table) in (4, 5) and ok(offsets, torch.int64) and offsets.dim() == 1 and offsets.numel() >= 1
                    and ok(rows, torch.int32) and ok(counts, torch.int32) and counts.numel() >= 2):
                raise RuntimeError("track_descriptors: table must be (offsets int64, rows int32, images, counts int32) contiguous "
                                   "device tensors as track_table returned them")
            if not (ok(q8, torch.uint8) and q8.dim() == 2 and q8.shape[1] == 128):
                raise RuntimeError("track_descriptors: q8 must be a contiguous uint8 [rows, 128] device tensor")
            tcap, ocap = offsets.numel() - 1, rows.numel()
            if obs_state is not None and not (ok(obs_state, torch.int32) and obs_state.numel() == ocap):
                raise RuntimeError("track_descriptors: obs_state must be a contiguous int32 [obs_capacity] device tensor")
            if points is not None and not (ok(points, torch.float32) and points.dim() == 2 and tuple(points.shape) == (tcap, 4)):
                raise RuntimeError("track_descriptors: points must be a contiguous float32 [track_capacity, 4] device tensor")
            desc = torch.empty((tcap, 128), dtype=torch.uint8, device=dev)
            ds = torch.empty((tcap, 2), dtype=torch.int32, device=dev) if stats else None
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.track_descriptors_device(ptr(q8), q8.shape[0], offsets.data_ptr(), tcap, ptr(rows), ocap,
                                                     counts.data_ptr(), ptr(desc), ptr(ds), ptr(obs_state), min_state, ptr(points),
                                                     min_parallax_deg, scale, s.cuda_stream)
        return (desc, ds) if stats else desc

    def localize(self, q8_query, kps_query, query_offsets, model_desc, points, table_counts, intrinsics, ratio=0.8,
                 max_reproj_px=4.0, min_parallax_deg=0.0, n_samples=512, min_inliers=12, rounds=3, seed=0, stream=None):
        """The poses of photographs that were not part of a reconstruction, against the model track_descriptors made: ONE
        lf_mkd_match_q8_device call with all query rows as a and the model's rows as b -- its answer per query row, a table
        index or -1, is the row_track resection reads -- then ONE lf_mkd_resect_cameras_device call over the query pool with
        all-zero poses.  No other kernel, and nothing is read back in between.
        q8_query [rows, 128] uint8 and kps_query [rows, 5] float32 are the query images' pooled rows and query_offsets
        [n_query + 1] int64 their image offsets; model_desc [track_capacity, 128] uint8, points [track_capacity, 4] float32
        and table_counts int32 are the model (at least two tracks); intrinsics [n_query, 4] float32 the query cameras'.  The
        other arguments are resect_cameras'.  A query row matched to a track without a point, or to a zero row, is no
        correspondence there.  Returns device tensors (poses [n_query, 12] float32, all zero where no pose was found; stats
        [n_query, 4] int32, err [n_query, 2] float32 and row_state [rows] int32 as resect_cameras returns them; row_track
        [rows] int32).  Asynchronous on `stream` (default: torch's current stream on the handle's device); capturable once
        warmed up."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            if not (ok(q8_query, torch.uint8) and q8_query.dim() == 2 and q8_query.shape[1] == 128
                    and ok(model_desc, torch.uint8) and model_desc.dim() == 2 and model_desc.shape[1] == 128):
                raise RuntimeError("localize: q8_query and model_desc must be contiguous uint8 [rows, 128] device tensors")
            if not (ok(kps_query, torch.float32) and kps_query.dim() == 2 and tuple(kps_query.shape) == (q8_query.shape[0], 5)):
                raise RuntimeError("localize: kps_query must be a contiguous float32 [rows, 5] device tensor, a row per row of "
                                   "q8_query")
            if not (ok(points, torch.float32) and points.dim() == 2 and tuple(points.shape) == (model_desc.shape[0], 4)):
                raise RuntimeError("localize: points must be a contiguous float32 [track_capacity, 4] device tensor, a row per "
                                   "row of model_desc")
            n_rows, n_query = q8_query.shape[0], query_offsets.numel() - 1 if hasattr(query_offsets, "numel") else -1
            row_track = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
            if n_rows:
                with self._lock:
                    self._inner.match_q8_device(q8_query.data_ptr(), n_rows, model_desc.data_ptr(), model_desc.shape[0],
                                                row_track.data_ptr(), ratio, stream=s.cuda_stream)
            zero = torch.zeros((max(n_query, 0), 12), dtype=torch.float32, device=dev)
        poses, st, er, rs = self.resect_cameras(kps_query, query_offsets, row_track, points, table_counts, intrinsics, zero,
                                                max_reproj_px, min_parallax_deg, n_samples, min_inliers, rounds, seed, stream=s)
        return poses, st, er, rs, row_track

    def view_graph(self, edges, R, pose_stats, n_images, max_loop_deg=3.0, min_front=0, root=None, tree_rounds=16, iterations=10,
                   use_unchecked=False, layout=None, match=None, out_match=None, residual=True, stream=None):
        """View-graph checks and global rotations (lf_mkd_view_graph_device): the relative rotations around every triangle of
        images must compose to the identity within max_loop_deg; an edge none of whose triangles closes is rejected, and the
        images get rotations by a breadth-first tree and `iterations` sweeps of quaternion averaging over the kept edges
        (include/lf_mkd.h states the algorithm).  edges = (edge_a, edge_b) 32-bit image ids, R [n_edges, 3, 3] (or [n_edges,
        9]) float32 and pose_stats [n_edges, 4] int32 as two_view_pose returned them; root is an image id or None (the image
        with the most kept edges); layout / match are edge_layout's offsets int64 [n_edges + 1] and the match array int32, and
        out_match the tensor to write (`match` itself for a call in place; default: a copy of match).  Returns device tensors
        (rotations [n_images, 3, 3] float32, all zero for an image without one; edge_stats [n_edges, 4] int32 = triangles
        closed, consistent, state (0 not usable, 1 rejected, 2 unchecked, 3 supported), the pair's representative (-1: not
        usable); residual [n_edges] float32, the cosine of the angle between R and the final rotations' R_b R_a^T (2: none), or
        None; image_stats [n_images, 4] int32 = kept edges, the round it was labelled in (-1: never), its tree edge, rejected
        edges; counts [8] int32 = usable, supported, rejected, unchecked, kept, labelled, root, 0; the filtered match array,
        build_tracks' input, or None).  Nothing is read back: asynchronous on `stream` (default: torch's current stream on
        the handle's device), capturable once warmed up."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            ea, eb = self._words(edges[0], dev), self._words(edges[1], dev)
            n_edges = ea.numel()
            if not (ok(R, torch.float32) and R.numel() == 9 * n_edges and eb.numel() == n_edges):
                raise RuntimeError("view_graph: R must be a contiguous float32 device tensor with 9 values per edge, edges one id "
                                   "per edge in each of its two arrays")
            if not (ok(pose_stats, torch.int32) and pose_stats.numel() == 4 * n_edges):
                raise RuntimeError("view_graph: pose_stats must be a contiguous int32 [n_edges, 4] device tensor")
            if (layout is None) != (match is None):
                raise RuntimeError("view_graph: layout and match go together")
            if match is not None:
                if not (ok(layout, torch.int64) and layout.numel() == n_edges + 1 and ok(match, torch.int32)):
                    raise RuntimeError("view_graph: layout must be int64 [n_edges + 1] and match int32 contiguous device tensors")
                if out_match is None:
                    out_match = match.clone()
                elif not (ok(out_match, torch.int32) and out_match.numel() == match.numel()):
                    raise RuntimeError("view_graph: out_match must be a contiguous int32 device tensor of match's size")
            rot = torch.empty((n_images, 3, 3), dtype=torch.float32, device=dev)
            es = torch.empty((n_edges, 4), dtype=torch.int32, device=dev)
            res = torch.empty((n_edges,), dtype=torch.float32, device=dev) if residual else None
            ims = torch.empty((n_images, 4), dtype=torch.int32, device=dev)
            counts = torch.empty((8,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.view_graph_device(ptr(ea), ptr(eb), n_edges, ptr(R), ptr(pose_stats), n_images, ptr(rot), ptr(es),
                                              ptr(ims), counts.data_ptr(), ptr(res),
                                              layout.data_ptr() if match is not None else None,
                                              match.numel() if match is not None else 0,
                                              match.data_ptr() if match is not None else None,
                                              out_match.data_ptr() if match is not None else None, max_loop_deg, min_front,
                                              VIEW_GRAPH_AUTO_ROOT if root is None else root, tree_rounds, iterations,
                                              VIEW_GRAPH_USE_UNCHECKED if use_unchecked else 0, s.cuda_stream)
        return rot, es, res, ims, counts, out_match

    def tree_poses(self, edges, t, rotations, image_stats, max_depth=64, stream=None):
        """Initial poses from the view graph's tree (lf_mkd_tree_poses_device): every labelled image gets the rotation
        view_graph gave it and a centre one unit step from its tree parent's, along the tree edge's translation; the root
        gets [R | 0].  edges = (edge_a, edge_b) 32-bit image ids and t [n_edges, 3] float32 as two_view_pose returned them;
        rotations [n_images, 3, 3] (or [n_images, 9]) float32 and image_stats [n_images, 4] int32 as view_graph returned
        them.  Returns poses [n_images, 12] float32 (R row-major, then t; world to camera), the all-zero row for an image
        whose chain of tree edges does not reach the root within max_depth steps: what global_positions starts from.
        Nothing is read back: asynchronous on `stream`, capturable."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, ty: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == ty and x.is_contiguous()
            ea, eb = self._words(edges[0], dev), self._words(edges[1], dev)
            n_edges = ea.numel()
            if not (ok(t, torch.float32) and t.numel() == 3 * n_edges and eb.numel() == n_edges):
                raise RuntimeError("tree_poses: t must be a contiguous float32 device tensor with 3 values per edge, edges one id "
                                   "per edge in each of its two arrays")
            if not (ok(rotations, torch.float32) and rotations.numel() % 9 == 0):
                raise RuntimeError("tree_poses: rotations must be a contiguous float32 [n_images, 9] device tensor")
            n_images = rotations.numel() // 9
            if not (ok(image_stats, torch.int32) and image_stats.numel() == 4 * n_images):
                raise RuntimeError("tree_poses: image_stats must be a contiguous int32 [n_images, 4] device tensor")
            poses = torch.empty((n_images, 12), dtype=torch.float32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.tree_poses_device(ptr(ea), ptr(eb), ptr(t), n_edges, ptr(rotations), ptr(image_stats), n_images,
                                              ptr(poses), max_depth, s.cuda_stream)
        return poses

    def global_positions(self, kps, offsets, table, intrinsics, poses, sweeps=50, warm=3, robust_deg=0.2, min_obs=2,
                         out_poses=None, points=True, obs_state=True, trace=False, stream=None):
        """Global positioning (lf_mkd_global_positions_device): all camera centres and all track points at once under the
        rotations of `poses`, by `sweeps` alternations of the points' and the cameras' weighted 3x3 solves (unit weights for
        the first `warm`, then weights that floor at the sine of robust_deg), each followed by a similarity that puts the
        centres' centroid at 0 and their rms radius at 1 (include/lf_mkd.h states the algorithm).  kps [rows, 5] float32 is
        the pool and offsets [n_images + 1] int64 its image offsets; table = (offsets, rows, images, row_track, counts) as
        track_table returned it with image_offsets; intrinsics [n_images, 4] float32; poses [n_images, 12] float32 as
        tree_poses returned them (an all-zero rotation: the image takes no part).  out_poses names the tensor to write,
        `poses` itself for a call in place.  Returns device tensors (poses [n_images, 12] float32, points [track_capacity, 4]
        float32 = X, Y, Z and the track's smallest cosine ({0, 0, 0, 2}: unsolved) or None, obs_state [obs_capacity] int32 (0
        not usable, 1 usable, 2 final weight at least 1/2; -1 outside every track) or None, image_stats [n_images, 4] int32 =
        usable rows in solved tracks, those of weight at least 1/2, sweeps held, reason; trace [sweeps, 4] float64 = cost,
        weighted observations, held cameras, unsolved points, or None -- THE TRACE'S COST IS SUMMED BY ONE WORKGROUP; counts
        [8] int32).  triangulate_tracks under the returned poses gives the points bundle_adjust takes.  Nothing is read back:
        asynchronous on `stream`, capturable once warmed up."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if len(table) != 5:
            raise RuntimeError("global_positions: table must be track_table's (offsets, rows, images, row_track, counts)")
        t_off, rows, images, row_track, counts = table
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, ty: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == ty and x.is_contiguous()
            if not (ok(t_off, torch.int64) and t_off.dim() == 1 and t_off.numel() >= 1 and ok(rows, torch.int32)
                    and images is not None and ok(images, torch.int32) and rows.numel() == images.numel()
                    and ok(counts, torch.int32) and counts.numel() >= 2):
                raise RuntimeError("global_positions: table must be (offsets int64, rows int32, images int32, row_track int32, "
                                   "counts int32) contiguous device tensors as track_table returned them with image_offsets")
            if not (ok(kps, torch.float32) and kps.dim() == 2 and kps.shape[1] == 5):
                raise RuntimeError("global_positions: kps must be a contiguous float32 [rows, 5] device tensor")
            if not (ok(row_track, torch.int32) and row_track.numel() == kps.shape[0]):
                raise RuntimeError("global_positions: row_track must be a contiguous int32 [rows] device tensor")
            if not (ok(offsets, torch.int64) and offsets.dim() == 1 and offsets.numel() >= 1):
                raise RuntimeError("global_positions: offsets must be a contiguous int64 [n_images + 1] device tensor")
            n_images, tcap, ocap = offsets.numel() - 1, t_off.numel() - 1, rows.numel()
            if not (ok(intrinsics, torch.float32) and intrinsics.numel() == 4 * n_images and ok(poses, torch.float32)
                    and poses.numel() == 12 * n_images):
                raise RuntimeError("global_positions: intrinsics must be float32 [n_images, 4] and poses float32 [n_images, 12] "
                                   "contiguous device tensors")
            if out_poses is None:
                out_poses = torch.empty((n_images, 12), dtype=torch.float32, device=dev)
            elif not (ok(out_poses, torch.float32) and out_poses.numel() == 12 * n_images):
                raise RuntimeError("global_positions: out_poses must be a contiguous float32 [n_images, 12] device tensor")
            xo = torch.zeros((tcap, 4), dtype=torch.float32, device=dev) if points else None
            so = torch.full((ocap,), -1, dtype=torch.int32, device=dev) if obs_state else None
            ims = torch.zeros((n_images, 4), dtype=torch.int32, device=dev)
            tr = torch.zeros((sweeps, 4), dtype=torch.float64, device=dev) if trace else None
            cnt = torch.zeros((8,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.global_positions_device(ptr(kps), offsets.data_ptr(), n_images, kps.shape[0], t_off.data_ptr(), tcap,
                                                    ptr(rows), ptr(images), ocap, counts.data_ptr(), ptr(row_track), ptr(intrinsics),
                                                    ptr(poses), ptr(out_poses), ptr(ims), cnt.data_ptr(), d_points_out=ptr(xo),
                                                    d_obs_state=ptr(so), d_trace=ptr(tr), sweeps=sweeps, warm=warm,
                                                    robust_deg=robust_deg, min_obs=min_obs, stream=s.cuda_stream)
        return out_poses, xo, so, ims, tr, cnt

    def bundle_adjust(self, kps, offsets, table, points, intrinsics, poses, obs_state=None, camera_fixed=None, max_reproj_px=4.0,
                      lambda0=1e-3, iterations=10, cg_iterations=10, cg_tol=0.1, out_poses=None, out_points=None,
                      obs_state_out=True, stream=None):
        """Bundle adjustment (lf_mkd_bundle_adjust_device): Levenberg-Marquardt on the reprojection error over every free
        camera (registered, and not marked in camera_fixed) and every free point (a track with an active observation), the
        reduced camera system solved by `cg_iterations` preconditioned conjugate-gradient steps per iteration
        (include/lf_mkd.h states the algorithm).  kps [rows, 5] float32 is the pool and offsets [n_images + 1] int64 its image
        offsets; table = (offsets, rows, images, counts) as track_table returned them (its 5-tuple passes as it is); points
        [track_capacity, 4] float32 are triangulate_tracks' points; intrinsics [n_images, 4] and poses [n_images, 12] float32
        as the calls before it take them; obs_state [obs_capacity] int32 are triangulate_tracks' states (only its inliers, 2,
        are then used) and camera_fixed [n_images] int32 marks the poses to hold (hold two to fix the gauge).  out_poses /
        out_points name the tensors to write, `poses` / `points` themselves for a call in place (default: new tensors).
        Returns device tensors (poses [n_images, 12] float32, points [track_capacity, 4] float32, obs_state [obs_capacity] int32
        (0 inactive, 1 active, 2 inlier of the result; -1 outside every track) or None, trace [iterations, 8] float64 = cost,
        the candidate's cost, lambda, accepted, CG steps, inliers, held cameras, held points; counts [4] int32 = free cameras,
        free points, active observations, accepted steps).  Nothing is read back: asynchronous on `stream` (default: torch's
        current stream on the handle's device), capturable once warmed up."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if len(table) == 5:
            t_off, rows, images, _, counts = table
        else:
            t_off, rows, images, counts = table
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            if not (ok(t_off, torch.int64) and t_off.dim() == 1 and t_off.numel() >= 1 and ok(rows, torch.int32)
                    and images is not None and ok(images, torch.int32) and rows.numel() == images.numel()
                    and ok(counts, torch.int32) and counts.numel() >= 2):
                raise RuntimeError("bundle_adjust: table must be (offsets int64, rows int32, images int32, counts int32) "
                                   "contiguous device tensors as track_table returned them with image_offsets")
            if not (ok(kps, torch.float32) and kps.dim() == 2 and kps.shape[1] == 5):
                raise RuntimeError("bundle_adjust: kps must be a contiguous float32 [rows, 5] device tensor")
            if not (ok(offsets, torch.int64) and offsets.dim() == 1 and offsets.numel() >= 1):
                raise RuntimeError("bundle_adjust: offsets must be a contiguous int64 [n_images + 1] device tensor")
            n_images, tcap, ocap = offsets.numel() - 1, t_off.numel() - 1, rows.numel()
            if not (ok(points, torch.float32) and points.numel() == 4 * tcap):
                raise RuntimeError("bundle_adjust: points must be a contiguous float32 [track_capacity, 4] device tensor")
            if not (ok(intrinsics, torch.float32) and intrinsics.numel() == 4 * n_images and ok(poses, torch.float32)
                    and poses.numel() == 12 * n_images):
                raise RuntimeError("bundle_adjust: intrinsics must be float32 [n_images, 4] and poses float32 [n_images, 12] "
                                   "contiguous device tensors")
            if obs_state is not None and not (ok(obs_state, torch.int32) and obs_state.numel() == ocap):
                raise RuntimeError("bundle_adjust: obs_state must be a contiguous int32 [obs_capacity] device tensor")
            if camera_fixed is not None and not (ok(camera_fixed, torch.int32) and camera_fixed.numel() == n_images):
                raise RuntimeError("bundle_adjust: camera_fixed must be a contiguous int32 [n_images] device tensor")
            if out_poses is None:
                out_poses = torch.empty((n_images, 12), dtype=torch.float32, device=dev)
            elif not (ok(out_poses, torch.float32) and out_poses.numel() == 12 * n_images):
                raise RuntimeError("bundle_adjust: out_poses must be a contiguous float32 [n_images, 12] device tensor")
            if out_points is None:
                out_points = torch.empty((tcap, 4), dtype=torch.float32, device=dev)
            elif not (ok(out_points, torch.float32) and out_points.numel() == 4 * tcap):
                raise RuntimeError("bundle_adjust: out_points must be a contiguous float32 [track_capacity, 4] device tensor")
            so = torch.full((ocap,), -1, dtype=torch.int32, device=dev) if obs_state_out else None
            trace = torch.zeros((iterations, 8), dtype=torch.float64, device=dev)
            cnt = torch.zeros((4,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            with self._lock:
                self._inner.bundle_adjust_device(ptr(kps), offsets.data_ptr(), n_images, kps.shape[0], t_off.data_ptr(), tcap,
                                                 ptr(rows), ptr(images), ocap, counts.data_ptr(), ptr(points), ptr(intrinsics),
                                                 ptr(poses), ptr(out_poses), ptr(out_points), trace.data_ptr(), cnt.data_ptr(),
                                                 d_obs_state=ptr(obs_state), d_camera_fixed=ptr(camera_fixed),
                                                 d_obs_state_out=ptr(so), max_reproj_px=max_reproj_px, lambda0=lambda0,
                                                 iterations=iterations, cg_iterations=cg_iterations, cg_tol=cg_tol,
                                                 stream=s.cuda_stream)
        return out_poses, out_points, so, trace, cnt

    def bundle_adjust_intrinsics(self, kps, offsets, table, points, intrinsics, poses, obs_state=None, camera_fixed=None,
                                 camera_group=None, n_groups=1, refine_focal=True, refine_principal=False, max_reproj_px=4.0,
                                 lambda0=1e-3, iterations=10, cg_iterations=10, cg_tol=0.1, out_poses=None, out_points=None,
                                 out_intrinsics=None, obs_state_out=True, stream=None):
        """Self-calibrating bundle adjustment (lf_mkd_bundle_adjust_intrinsics_device): bundle_adjust with the intrinsics of the
        images that share a lens refined beside the poses and the points.  The arguments are bundle_adjust's; camera_group
        [n_images] int32 names the lens of every image (None: one lens; an id >= n_groups: that image's intrinsics stay), and
        a group's focal lengths are scaled by one factor s (refine_focal) and its principal points shifted by one (dx, dy)
        (refine_principal).  out_intrinsics names the tensor to write, `intrinsics` itself for a call in place.  Returns device
        tensors (poses, points, intrinsics [n_images, 4] float32, groups [n_groups, 3] float32 = (s, dx, dy), obs_state or
        None, trace [iterations, 9] float64 = bundle_adjust's eight and the held groups, counts [5] int32 = its four and the
        free groups).  With nothing refined every value shared with bundle_adjust is that call's, bit for bit.  Nothing is read
        back: asynchronous on `stream`, capturable once warmed up."""
        import torch
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if len(table) == 5:
            t_off, rows, images, _, counts = table
        else:
            t_off, rows, images, counts = table
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ok = lambda x, t: hasattr(x, "is_cuda") and x.is_cuda and x.dtype == t and x.is_contiguous()
            if not (ok(t_off, torch.int64) and t_off.dim() == 1 and t_off.numel() >= 1 and ok(rows, torch.int32)
                    and images is not None and ok(images, torch.int32) and rows.numel() == images.numel()
                    and ok(counts, torch.int32) and counts.numel() >= 2):
                raise RuntimeError("bundle_adjust_intrinsics: table must be (offsets int64, rows int32, images int32, counts int32) "
                                   "contiguous device tensors as track_table returned them with image_offsets")
            if not (ok(kps, torch.float32) and kps.dim() == 2 and kps.shape[1] == 5):
                raise RuntimeError("bundle_adjust_intrinsics: kps must be a contiguous float32 [rows, 5] device tensor")
            if not (ok(offsets, torch.int64) and offsets.dim() == 1 and offsets.numel() >= 1):
                raise RuntimeError("bundle_adjust_intrinsics: offsets must be a contiguous int64 [n_images + 1] device tensor")
            n_images, tcap, ocap = offsets.numel() - 1, t_off.numel() - 1, rows.numel()
            if not (ok(points, torch.float32) and points.numel() == 4 * tcap):
                raise RuntimeError("bundle_adjust_intrinsics: points must be a contiguous float32 [track_capacity, 4] device tensor")
            if not (ok(intrinsics, torch.float32) and intrinsics.numel() == 4 * n_images and ok(poses, torch.float32)
                    and poses.numel() == 12 * n_images):
                raise RuntimeError("bundle_adjust_intrinsics: intrinsics must be float32 [n_images, 4] and poses float32 "
                                   "[n_images, 12] contiguous device tensors")
            for name, x in (("obs_state", obs_state), ("camera_fixed", camera_fixed), ("camera_group", camera_group)):
                if x is not None and not (ok(x, torch.int32) and x.numel() == (ocap if name == "obs_state" else n_images)):
                    raise RuntimeError("bundle_adjust_intrinsics: %s must be a contiguous int32 device tensor, one entry per %s"
                                       % (name, "observation" if name == "obs_state" else "image"))
            outs = []
            for name, x, width, n in (("out_poses", out_poses, 12, n_images), ("out_points", out_points, 4, tcap),
                                      ("out_intrinsics", out_intrinsics, 4, n_images)):
                if x is None:
                    x = torch.empty((n, width), dtype=torch.float32, device=dev)
                elif not (ok(x, torch.float32) and x.numel() == width * n):
                    raise RuntimeError("bundle_adjust_intrinsics: %s must be a contiguous float32 [., %d] device tensor" % (name, width))
                outs.append(x)
            out_poses, out_points, out_intrinsics = outs
            groups = torch.zeros((n_groups, 3), dtype=torch.float32, device=dev)
            so = torch.full((ocap,), -1, dtype=torch.int32, device=dev) if obs_state_out else None
            trace = torch.zeros((iterations, 9), dtype=torch.float64, device=dev)
            cnt = torch.zeros((5,), dtype=torch.int32, device=dev)
            ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
            refine = (BA_REFINE_FOCAL if refine_focal else 0) | (BA_REFINE_PRINCIPAL if refine_principal else 0)
            with self._lock:
                self._inner.bundle_adjust_intrinsics_device(
                    ptr(kps), offsets.data_ptr(), n_images, kps.shape[0], t_off.data_ptr(), tcap, ptr(rows), ptr(images), ocap,
                    counts.data_ptr(), ptr(points), ptr(intrinsics), ptr(poses), ptr(out_poses), ptr(out_points), ptr(out_intrinsics),
                    trace.data_ptr(), cnt.data_ptr(), d_obs_state=ptr(obs_state), d_camera_fixed=ptr(camera_fixed),
                    d_camera_group=ptr(camera_group), n_groups=n_groups, refine=refine, d_group_out=ptr(groups),
                    d_obs_state_out=ptr(so), max_reproj_px=max_reproj_px, lambda0=lambda0, iterations=iterations,
                    cg_iterations=cg_iterations, cg_tol=cg_tol, stream=s.cuda_stream)
        return out_poses, out_points, out_intrinsics, groups, so, trace, cnt

    def match_q8_guided_batch(self, qa, kps_a, offsets_a, qb, kps_b, offsets_b, model, kind="homography", threshold=None,
                              ratio=0.8, mutual=True, both=False, stream=None):
        """match_guided_batch over 8-bit descriptors (lf_mkd_match_q8_guided_pairs_device: one launch, three with `mutual`):
        match_q8_batch once more, with the candidates of every row restricted to the rows of the other side that pass the
        verifier's inlier test with it under the pair's model -- the relation match_guided_batch uses, bit for bit.  qa
        [Na,128] / qb [Nb,128] must be uint8 (what `quantize` returns); kps_a [Na,5] / kps_b [Nb,5], the offsets and model
        [n_pairs,3,3] (or [n_pairs,9]) as match_guided_batch takes them.  kind: "homography" or "fundamental" (or GUIDE_*);
        threshold in pixels, default the verifier's own (3.0 for H, 1.5 for F).  Returns device tensors (match_ab [Na] int32,
        match_ba [Nb] int32 or None -- given with `mutual` or `both` --, best [Na] int32, second [Na] int32): the scores are
        the exact integer similarities of the a -> b direction over the admissible rows; rows outside every pair hold
        -1 / INT32_MIN.  With the model verification gave on match_q8_batch(mutual=True)'s output, the verifier's threshold and
        the same ratio, every verified match is found again (include/lf_mkd.h).  Enqueued on `stream` (default: torch's
        current stream on the handle's device), asynchronously."""
        import torch
        kinds = {"homography": GUIDE_HOMOGRAPHY, "fundamental": GUIDE_FUNDAMENTAL, GUIDE_HOMOGRAPHY: GUIDE_HOMOGRAPHY,
                 GUIDE_FUNDAMENTAL: GUIDE_FUNDAMENTAL}
        if kind not in kinds:
            raise RuntimeError('match_q8_guided_batch: kind must be "homography" or "fundamental"')
        kind = kinds[kind]
        if threshold is None:
            threshold = 3.0 if kind == GUIDE_HOMOGRAPHY else 1.5
        dev = torch.device("cuda", self.device)
        n_pairs = int(offsets_a.numel()) - 1
        if n_pairs < 0 or int(offsets_b.numel()) != n_pairs + 1:
            raise RuntimeError("match_q8_guided_batch: offsets_a and offsets_b need n_pairs + 1 entries each")
        if int(model.numel()) != 9 * n_pairs:
            raise RuntimeError("match_q8_guided_batch: model needs 9 entries per pair")
        for q in (qa, qb):
            if q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] != 128:
                raise RuntimeError("match_q8_guided_batch: qa and qb must be uint8 [n, 128] (LocalFeatures.quantize)")
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):      # the copies and the fills below are ordered with the call
            a, b = qa.to(dev).contiguous(), qb.to(dev).contiguous()
            ka = kps_a.to(dev, torch.float32).reshape(-1, 5).contiguous()
            kb = kps_b.to(dev, torch.float32).reshape(-1, 5).contiguous()
            oa, ob = offsets_a.to(dev, torch.int64).contiguous(), offsets_b.to(dev, torch.int64).contiguous()
            md = model.to(dev, torch.float32).reshape(-1, 9).contiguous()
            na, nb = a.shape[0], b.shape[0]
            if ka.shape[0] != na or kb.shape[0] != nb:
                raise RuntimeError("match_q8_guided_batch: one keypoint per descriptor row on either side")
            int32_min = -2 ** 31
            m_ab = torch.full((na,), -1, dtype=torch.int32, device=dev)
            m_ba = torch.full((nb,), -1, dtype=torch.int32, device=dev) if (both or mutual) else None
            best = torch.full((na,), int32_min, dtype=torch.int32, device=dev)
            second = torch.full((na,), int32_min, dtype=torch.int32, device=dev)
            if n_pairs and na and nb:       # (an empty side: no row has a candidate, the fills above are the answer)
                with self._lock:
                    self._inner.match_q8_guided_pairs_device(a.data_ptr(), ka.data_ptr(), oa.data_ptr(), na, b.data_ptr(),
                                                             kb.data_ptr(), ob.data_ptr(), nb, md.data_ptr(), n_pairs,
                                                             m_ab.data_ptr(), m_ba.data_ptr() if m_ba is not None else None,
                                                             kind, threshold, ratio, MATCH_MUTUAL if mutual else 0,
                                                             best.data_ptr(), second.data_ptr(), s.cuda_stream)
        return m_ab, m_ba, best, second

    def match_q8_guided(self, qa, kps_a, qb, kps_b, model, kind="homography", threshold=None, ratio=0.8, mutual=True, both=False,
                        stream=None):
        """match_q8_guided_batch for one pair (n_pairs = 1: all of qa against all of qb under `model` [3,3])."""
        import torch
        na, nb = int(qa.numel()) // 128, int(qb.numel()) // 128
        return self.match_q8_guided_batch(qa, kps_a, torch.tensor([0, na]), qb, kps_b, torch.tensor([0, nb]), model, kind,
                                          threshold, ratio, mutual, both, stream)

    def match_ip_distance(self, desc_a, desc_b, factor=0.75):
        """The webcam example's acceptance rule (examples/webcam/src/main.rs:97-104,261-265): nearest and second-nearest
        neighbour of desc_a[i] in desc_b under the inner-product distance d = 1 - <a, b> (usearch MetricKind::IP), accepted
        if d0 < factor * d1.  Built on the same matcher: lf_mkd_match_device with ratio <= 0 returns the best index plus
        the best and second-best similarity, the rule is applied to those.  Returns a list of (i, j)."""
        import torch
        a = np.ascontiguousarray(desc_a, np.float32).reshape(-1, 128)
        b = np.ascontiguousarray(desc_b, np.float32).reshape(-1, 128)
        if len(a) == 0:
            return []
        dev = torch.device("cuda", self.device)
        with self._lock, torch.cuda.device(dev):
            d_a, d_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            d_m = torch.empty((len(a),), dtype=torch.int32, device=dev)
            d_1, d_2 = torch.empty((len(a),), device=dev), torch.empty((len(a),), device=dev)
            s = torch.cuda.current_stream(dev)
            self._inner.match_device(d_a.data_ptr(), len(a), d_b.data_ptr(), len(b), d_m.data_ptr(), 0.0, None, None,
                                     d_1.data_ptr(), d_2.data_ptr(), s.cuda_stream)
            s.synchronize()
            self._inner.synchronize()       # (torch's default stream is handle 0 = "the library's own stream" to the ABI)
            keep = (1.0 - d_1) < (1.0 - d_2) * factor
            m, keep = d_m.cpu().numpy(), keep.cpu().numpy()
        return [(int(i), int(m[i])) for i in np.flatnonzero(keep)]

    def verify_homography(self, kp_a, kp_b, matches, threshold=3.0, n_hypotheses=2048, seed=0, flags=0):
        """Geometric verification of matches (lf_mkd_verify_homography): RANSAC over 4-point homographies on the GPU, then a
        least-squares refit on the inliers (include/lf_mkd.h states the algorithm).  kp_a / kp_b: the keypoint lists (or
        [n,4|5] arrays) the matches index; matches: the (i, j) list `match` / `match_both` return.  Returns (H, inliers):
        H ndarray[3,3] with b ~ H a in pixels and H[2,2] = 1, or None if no hypothesis was valid; inliers the (i, j) pairs
        that agree with H within `threshold` pixels.  Per-call numbers (inlier counts, best hypothesis) are kept in
        `verify_stats`."""
        a, b = _keypoints_to_array(kp_a), _keypoints_to_array(kp_b)
        m = np.full(len(a), -1, np.int32)
        for i, j in matches:
            if not (0 <= i < len(a) and 0 <= j < len(b)):
                raise RuntimeError("verify_homography: match (%d, %d) outside the keypoint lists" % (i, j))
            m[i] = j
        with self._lock:
            H, ver, st = self._inner.verify_homography(a.view(np.float32).reshape(-1, 5), b.view(np.float32).reshape(-1, 5), m,
                                                       n_hypotheses, threshold, seed, flags)
        self.verify_stats = {"inliers": int(st[0]), "best_hypothesis_inliers": int(st[1]), "best_hypothesis": int(st[2]),
                             "considered": int(st[3])}
        if st[2] == 0xFFFFFFFF:
            return None, []
        return H.astype(np.float64), [(int(i), int(j)) for i, j in enumerate(ver) if j >= 0]

    def verify_homography_batch(self, kps_a, offsets_a, kps_b, offsets_b, match, threshold=3.0, n_hypotheses=2048, seed=0,
                                flags=0, stream=None):
        """Many image pairs in one call (lf_mkd_verify_homography_device), on torch device tensors -- e.g. the keypoints of
        detect_top_n_batch frames and a matcher's output per pair.  kps_a [Na,5] / kps_b [Nb,5] float32, offsets_a /
        offsets_b int64 [n_pairs + 1] (pair p: a rows offsets_a[p]..offsets_a[p+1], likewise b), match int32 [Na] with values
        local to the pair's b rows.  Pair p is seeded with seed + p.  Returns device tensors (H [n_pairs,3,3], verified [Na]
        int32, stats [n_pairs,4] int64: final inliers, best hypothesis' inliers, best hypothesis (-1: none), considered).
        Enqueued on `stream` (default: torch's current stream on the handle's device), asynchronously."""
        import torch
        dev = torch.device("cuda", self.device)
        n_pairs = int(offsets_a.numel()) - 1
        if n_pairs < 0 or int(offsets_b.numel()) != n_pairs + 1:
            raise RuntimeError("verify_homography_batch: offsets_a and offsets_b need n_pairs + 1 entries each")
        ka = kps_a.to(dev, torch.float32).reshape(-1, 5).contiguous()
        kb = kps_b.to(dev, torch.float32).reshape(-1, 5).contiguous()
        oa, ob = offsets_a.to(dev, torch.int64).contiguous(), offsets_b.to(dev, torch.int64).contiguous()
        mt = match.to(dev, torch.int32).contiguous()
        if mt.numel() != ka.shape[0]:
            raise RuntimeError("verify_homography_batch: match must have one entry per row of kps_a")
        H = torch.empty((max(n_pairs, 1), 3, 3), dtype=torch.float32, device=dev)
        ver = torch.empty((max(ka.shape[0], 1),), dtype=torch.int32, device=dev)
        st = torch.empty((max(n_pairs, 1), 4), dtype=torch.int32, device=dev)
        with self._lock, torch.cuda.device(dev):
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            self._inner.verify_homography_device(ka.data_ptr(), oa.data_ptr(), kb.data_ptr(), ob.data_ptr(), mt.data_ptr(),
                                                 n_pairs, H.data_ptr(), ver.data_ptr(), st.data_ptr(), n_hypotheses, threshold,
                                                 seed, flags, s.cuda_stream)
        return H[:n_pairs], ver[:ka.shape[0]], st[:n_pairs].to(torch.int64)

    def verify_fundamental(self, kp_a, kp_b, matches, threshold=1.5, n_hypotheses=2048, seed=0, flags=0):
        """Geometric verification of matches by epipolar geometry (lf_mkd_verify_fundamental): 7-point RANSAC on the GPU,
        scored by Sampson distance, then a rank-2 least-squares refit (include/lf_mkd.h states the algorithm).  For pairs with
        parallax, where a homography keeps only one plane; a (nearly) planar scene leaves F underdetermined.  Arguments as
        verify_homography.  Returns (F, inliers): F ndarray[3,3] with b^T F a = 0 in pixels and its largest entry +1, or
        None if no sample was valid; inliers the (i, j) pairs within `threshold` px of Sampson distance.  Per-call numbers
        are kept in `verify_stats` (best_candidate = 3 k + j: sample k, root j)."""
        a, b = _keypoints_to_array(kp_a), _keypoints_to_array(kp_b)
        m = np.full(len(a), -1, np.int32)
        for i, j in matches:
            if not (0 <= i < len(a) and 0 <= j < len(b)):
                raise RuntimeError("verify_fundamental: match (%d, %d) outside the keypoint lists" % (i, j))
            m[i] = j
        with self._lock:
            F, ver, st = self._inner.verify_fundamental(a.view(np.float32).reshape(-1, 5), b.view(np.float32).reshape(-1, 5), m,
                                                        n_hypotheses, threshold, seed, flags)
        self.verify_stats = {"inliers": int(st[0]), "best_candidate_inliers": int(st[1]), "best_candidate": int(st[2]),
                             "considered": int(st[3])}
        if st[2] == 0xFFFFFFFF:
            return None, []
        return F.astype(np.float64), [(int(i), int(j)) for i, j in enumerate(ver) if j >= 0]

    def verify_fundamental_batch(self, kps_a, offsets_a, kps_b, offsets_b, match, threshold=1.5, n_hypotheses=2048, seed=0,
                                 flags=0, stream=None):
        """Many image pairs in one call (lf_mkd_verify_fundamental_device) on torch device tensors, laid out as for
        verify_homography_batch.  Returns device tensors (F [n_pairs,3,3], verified [Na] int32, stats [n_pairs,4] int64:
        final inliers, best candidate's inliers, best candidate 3 k + j (-1: none), considered)."""
        return self._verify_batch(self._inner.verify_fundamental_device, "verify_fundamental_batch", kps_a, offsets_a, kps_b,
                                  offsets_b, match, threshold, n_hypotheses, seed, flags, stream)

    def _verify_batch(self, device_call, what, kps_a, offsets_a, kps_b, offsets_b, match, threshold, n_hypotheses, seed, flags,
                      stream):
        import torch
        dev = torch.device("cuda", self.device)
        n_pairs = int(offsets_a.numel()) - 1
        if n_pairs < 0 or int(offsets_b.numel()) != n_pairs + 1:
            raise RuntimeError(what + ": offsets_a and offsets_b need n_pairs + 1 entries each")
        ka = kps_a.to(dev, torch.float32).reshape(-1, 5).contiguous()
        kb = kps_b.to(dev, torch.float32).reshape(-1, 5).contiguous()
        oa, ob = offsets_a.to(dev, torch.int64).contiguous(), offsets_b.to(dev, torch.int64).contiguous()
        mt = match.to(dev, torch.int32).contiguous()
        if mt.numel() != ka.shape[0]:
            raise RuntimeError(what + ": match must have one entry per row of kps_a")
        M = torch.empty((max(n_pairs, 1), 3, 3), dtype=torch.float32, device=dev)
        ver = torch.empty((max(ka.shape[0], 1),), dtype=torch.int32, device=dev)
        st = torch.empty((max(n_pairs, 1), 4), dtype=torch.int32, device=dev)
        with self._lock, torch.cuda.device(dev):
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            device_call(ka.data_ptr(), oa.data_ptr(), kb.data_ptr(), ob.data_ptr(), mt.data_ptr(), n_pairs, M.data_ptr(),
                        ver.data_ptr(), st.data_ptr(), n_hypotheses, threshold, seed, flags, s.cuda_stream)
        return M[:n_pairs], ver[:ka.shape[0]], st[:n_pairs].to(torch.int64)

    def describe_patches(self, patches):
        """patches: [n,32,32] float32 -> ndarray[n,128] (the CPU twin's Mkd::patch, mkd_ref.rs:57-77)."""
        with self._lock:
            return self._inner.describe_patches(patches)

    def _detect(self, img, n, min_size):
        arr = np.asarray(img)
        if arr.ndim != 2:
            raise RuntimeError("Failed to extract features", "image must be 2-dimensional")
        with self._lock:
            try:
                kps, desc, self.dropped_blobs, self.dropped_features = self._inner.detect(arr, n, min_size)
            except RuntimeError as e:   # python/src/lib.rs:97-102
                raise RuntimeError("Failed to extract features", str(e)) from e
        return [Keypoint(*row) for row in kps], desc

    def detect(self, img):
        """python/src/lib.rs:86-113 (detect_extract_all): every extremum the detector finds, at most max_blobs."""
        return self._detect(img, 0, 0.0)

    def detect_top_n_batch(self, imgs, n, min_size=0.0):
        """detect_top_n over a batch of equally sized frames ([f, h, w] float32, f <= max_frames) with every stage
        launched once for all frames (lf_mkd_detect_frames_device).  Returns one (list[Keypoint], ndarray[k,128]) per
        frame.  The library's keypoint budget is one number for the whole batch (lf_mkd.h): max_features * f here, with
        every frame then cut to its first max_features keypoints -- so each frame's result equals what detect_top_n gives
        for that frame alone as long as the batch total fits the budget (keypoints beyond it are lost to the LAST frames
        and counted, like the per-frame cuts, in dropped_features)."""
        import torch
        arr = np.ascontiguousarray(imgs, np.float32)
        if arr.ndim != 3:
            raise RuntimeError("Failed to extract features", "images must be [frames, height, width]")
        f, h, w = arr.shape
        cap = self.max_features * f
        dev = torch.device("cuda", self.device)      # the handle's device, not torch's current one
        with self._lock:
            try:
                with torch.cuda.device(dev):
                    d_img = torch.from_numpy(arr).to(dev)
                    d_k = torch.empty((cap, 5), device=dev)
                    d_f = torch.empty((cap,), dtype=torch.int32, device=dev)
                    d_d = torch.empty((cap, 128), device=dev)
                    m, self.dropped_blobs, self.dropped_features = self._inner.detect_frames_device(
                        d_img.data_ptr(), f, w, h, int(n), float(min_size), d_k.data_ptr(), d_f.data_ptr(), d_d.data_ptr(),
                        cap, torch.cuda.current_stream(dev).cuda_stream)
                    torch.cuda.synchronize(dev)
            except RuntimeError as e:
                raise RuntimeError("Failed to extract features", str(e)) from e
        kps, fid, desc = d_k[:m].cpu().numpy(), d_f[:m].cpu().numpy(), d_d[:m].cpu().numpy()
        out = []
        for i in range(f):
            sel = np.flatnonzero(fid == i)
            self.dropped_features += max(0, len(sel) - self.max_features)
            sel = sel[:self.max_features]
            out.append(([Keypoint(*row) for row in kps[sel]], desc[sel]))
        return out

    def detect_top_n(self, img, n, min_size):
        """python/src/lib.rs:115-149: the n extrema of largest contrast among those of size >= min_size."""
        return self._detect(img, int(n), float(min_size))
