"""Problems the homography tests share: planted perspective maps and the batches of mixed pairs (tests/test_gpu_homography.py,
tests/test_gpu_homography_exact.py, tests/test_homography_twin.py)."""
import numpy as np

import homography_ref as ref

THR = 3.0
H_TRUE = np.array([[0.92, -0.18, 60.0], [0.12, 1.05, -30.0], [1.2e-4, -1.5e-4, 1.0]])
CORNERS = np.array([[0.0, 0.0], [1000.0, 0.0], [1000.0, 1000.0], [0.0, 1000.0]])


def planted(m, frac, seed, sigma=0.5, h=H_TRUE):
    """m matches (kps as [m,5] f32, identity match array): a fraction `frac` maps by h plus noise, the rest is random."""
    g = np.random.default_rng(seed)
    a = g.uniform(0, 1000, (m, 2))
    b = ref.map_points(h, a) + g.normal(0, sigma, (m, 2))
    out = g.random(m) >= frac
    b[out] = g.uniform(0, 1000, (int(out.sum()), 2))
    ka, kb = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    ka[:, :2], kb[:, :2] = a, b
    ka[:, 2] = kb[:, 2] = 4.0
    return ka, kb, np.arange(m, dtype=np.int32)


def band(prob, h, thr=THR):
    """Considered matches whose squared residual under h lies within 5 % of thr^2 (where f32 and f64 may disagree)."""
    w, e2 = prob.residuals(h)
    return np.abs(e2 - thr * thr) <= 0.05 * thr * thr


def pairs(n_pairs=64):
    """Pairs of differing sizes: empty ones, M < 4, all-collinear ones, and ordinary planted problems (with rows that do
    not count: -1 and out-of-range matches)."""
    g = np.random.default_rng(3)
    pairs = []
    for p in range(n_pairs):
        kind = p % 8
        if kind == 0:
            ka, kb, mt = np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)
        elif kind == 1:
            ka, kb, mt = planted(3, 1.0, p)
        elif kind == 2:
            n = 40
            ka, kb = np.zeros((n, 5), np.float32), np.zeros((n, 5), np.float32)
            ka[:, 0] = np.arange(n) * 9.0
            ka[:, 1] = 5.0 + 0.5 * ka[:, 0]
            kb[:, :2] = ka[:, :2] + 20.0
            mt = np.arange(n, dtype=np.int32)
        else:
            n = int(g.integers(20, 1500))
            ka, kb, mt = planted(n, float(g.uniform(0.2, 0.9)), 1000 + p)
            extra = g.uniform(0, 1000, (n // 3, 5)).astype(np.float32)   # b rows nobody matches
            kb = np.concatenate([kb, extra])
            perm = g.permutation(len(kb))
            inv = np.argsort(perm)
            kb, mt = kb[perm], inv[mt].astype(np.int32)
            drop = g.random(n) < 0.3
            mt[drop] = -1
            mt[g.random(n) < 0.02] = len(kb) + 5                           # out of range: counts as -1
        pairs.append((ka, kb, mt))
    return pairs


def random_perspective(g, width, height):
    """A perspective map of a width x height frame that keeps it in view: its corners moved by up to 15 % of the size."""
    src = np.array([[0, 0], [width, 0], [width, height], [0, height]], np.float64)
    dst = src + g.uniform(-0.15, 0.15, (4, 2)) * [width, height]
    rows = []
    for (x, y), (u, v) in zip(src, dst):
        rows.append([x, y, 1, 0, 0, 0, -x * u, -y * u, u])
        rows.append([0, 0, 0, x, y, 1, -x * v, -y * v, v])
    a = np.array(rows)
    return np.append(np.linalg.solve(a[:, :8], a[:, 8]), 1.0).reshape(3, 3)


def planted_in(g, m, frac, h, width, height, offset=0.0, sigma=0.5):
    """m matches in a width x height frame at `offset` px: a fraction `frac` maps by h (in frame coordinates) plus noise,
    the rest lands anywhere in the frame."""
    a = g.uniform(0, 1, (m, 2)) * [width, height]
    b = ref.map_points(h, a) + g.normal(0, sigma, (m, 2))
    out = g.random(m) >= frac
    b[out] = g.uniform(0, 1, (int(out.sum()), 2)) * [width, height]
    ka, kb = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    ka[:, :2], kb[:, :2] = a + offset, b + offset
    ka[:, 2] = kb[:, 2] = 4.0
    return ka, kb, np.arange(m, dtype=np.int32)


def _rows(a, b):
    ka, kb = np.zeros((len(a), 5), np.float32), np.zeros((len(b), 5), np.float32)
    ka[:, :2], kb[:, :2] = a, b
    ka[:, 2] = kb[:, 2] = 4.0
    return ka, kb


def near_degenerate(g, m, lines=3):
    """m matches on `lines` lines through a 1000 x 1000 frame, b = H_TRUE a, each point jittered off its line by 1e-3 to
    1 px (log-uniform): quads with three points on one line have a normalised |cross| on both sides of 1e-4."""
    ends = g.uniform(0, 1000, (lines, 2, 2))
    which = g.integers(0, lines, m)
    t = g.uniform(0, 1, (m, 1))
    a = ends[which, 0] + t * (ends[which, 1] - ends[which, 0])
    b = ref.map_points(H_TRUE, a)
    jit = lambda: np.exp(g.uniform(np.log(1e-3), 0, (m, 1))) * g.normal(0, 1, (m, 2))
    ka, kb = _rows(a + jit(), b + jit())
    return ka, kb, np.arange(m, dtype=np.int32)


# a strong perspective map whose vanishing line (w = 0: x = 600) crosses the 1000 x 1000 frame
H_VANISH = np.array([[1.0, 0.1, 20.0], [0.05, 1.0, -10.0], [-1.0 / 600.0, 0.0, 1.0]])


def vanishing(g, m):
    """Matches under H_VANISH with noise: points beyond the vanishing line map with w < 0 (so they are never inliers
    of the true map), hypotheses drawn there come out with flipped orientation, mixed ones are invalid."""
    a = g.uniform(0, 1000, (m, 2))
    b = ref.map_points(H_VANISH, a) + g.normal(0, 0.3, (m, 2))
    far = np.abs(b).max(axis=1) > 2e4        # next to the vanishing line: anywhere in the frame instead
    b[far] = g.uniform(0, 1000, (int(far.sum()), 2))
    ka, kb = _rows(a, b)
    return ka, kb, np.arange(m, dtype=np.int32)


def duplicates(g, m):
    """Many a rows matched to one b row (a tenth of the b rows take most matches) and coincident a points."""
    ka, kb, _ = planted(m, 0.6, int(g.integers(1 << 30)))
    mt = np.arange(m, dtype=np.int32)
    hub = g.random(m) < 0.4
    mt[hub] = g.integers(0, max(m // 10, 1), int(hub.sum()))
    same = g.random(m) < 0.2
    ka[same, :2] = ka[g.integers(0, m, int(same.sum())), :2]
    return ka, kb, mt


def exact_integer(g, m, shift=(37.0, -12.0)):
    """Integer pixel coordinates and b = a + an integer shift, exactly: every match is an inlier of the true map."""
    a = g.integers(0, 1000, (m, 2)).astype(np.float64)
    ka, kb = _rows(a, a + shift)
    return ka, kb, np.arange(m, dtype=np.int32)


def two_planes(g, m, shift=500.0):
    """Two exact planes of m / 2 matches each, the second shifted by `shift` px in b: both pure planes' hypotheses tie."""
    a = g.integers(0, 1000, (m, 2)).astype(np.float64)
    b = a + 5.0
    b[m // 2:] += shift
    ka, kb = _rows(a, b)
    return ka, kb, np.arange(m, dtype=np.int32)
