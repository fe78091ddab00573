"""CPU tests of the f32 twin of the verification kernel (tests/homography_f32.py): its fmaf is exact, and on a few hundred
random problems it agrees with the float64 restatement (tests/homography_ref.py) wherever f32 rounding cannot matter.  The
GPU tests then hold the device to the twin bit for bit (tests/test_gpu_homography_exact.py)."""
from fractions import Fraction

import numpy as np

import homography_f32 as tw
import homography_ref as ref
from homography_cases import THR, band, planted_in, random_perspective

F32 = np.float32


def _round_f32(q):
    """An exact rational rounded to the nearest f32, ties to even (subnormals and overflow included)."""
    if q == 0:
        return F32(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(q, quantum)
    if rem * 2 > quantum or (rem * 2 == quantum and n % 2):
        n += 1
    v = n * quantum
    return F32(sign * np.inf) if v >= 2 ** 128 else F32(sign * float(v))


def _exact_fma(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fmaf_matches_exact_rounding_on_random_triples():
    g = np.random.default_rng(0)
    n = 4000
    mant = g.uniform(-2, 2, (3, n))
    exps = g.integers(-70, 40, (3, n))
    a, b, c = (np.ldexp(mant[i], exps[i]).astype(F32) for i in range(3))
    # a third of the triples cancel: c close to -a*b, so that the result is small, of either sign, often subnormal
    k = n // 3
    a[:k] = np.ldexp(g.uniform(-2, 2, k), g.integers(-75, -55, k)).astype(F32)
    b[:k] = np.ldexp(g.uniform(-2, 2, k), g.integers(-75, -55, k)).astype(F32)
    c[:k] = -(a[:k].astype(np.float64) * b[:k]).astype(F32) * F32(1.0 + 2.0 ** -22) ** g.integers(-1, 2, k)
    got = tw.fmaf(a, b, c)
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.abs(want[:k]) < np.finfo(F32).tiny).sum() > 50 and (want[:k] < 0).any() and (want[:k] > 0).any()


def test_fmaf_resolves_double_rounding_at_f32_midpoints():
    """a*b + c lands within an f64 rounding of an f32 midpoint, on either side, at several exponents and in the subnormal
    range: rounding the f64 sum to f32 would pick the wrong neighbour in every case."""
    u = 2.0 ** -23
    cases = []
    for k in (0, -20, 30, -100):
        s = 2.0 ** k
        # 2^-24 (1 - 2^-46) below the midpoint above an odd c: the exact result rounds down to c
        cases.append((F32(s * 2.0 ** -24 * (1 + u)), F32(1 - u), F32(s * (1 + u)), F32(s * (1 + u))))
        # 2^-24 (1 - 2^-46) subtracted from an odd c: the exact result lies just above the midpoint below c -> c
        cases.append((F32(-s * 2.0 ** -24 * (1 + u)), F32(1 - u), F32(s * (1 + 3 * u)), F32(s * (1 + 3 * u))))
    # subnormal: c = 1025 * 2^-149 (odd), plus 2^-150 (1 - 2^-46)
    tiny = 2.0 ** -149
    cases.append((F32(2.0 ** -75 * (1 + u)), F32(2.0 ** -75 * (1 - u)), F32(1025 * tiny), F32(1025 * tiny)))
    cases.append((F32(-2.0 ** -75 * (1 + u)), F32(2.0 ** -75 * (1 - u)), F32(1027 * tiny), F32(1027 * tiny)))
    for a, b, c, want in cases:
        naive = F32(float(a) * float(b) + float(c))
        assert naive != want, (a, b, c)           # the case is one where double rounding goes wrong
        assert _exact_fma(a, b, c) == want, (a, b, c)
        assert tw.fmaf(a, b, c) == want, (a, b, c, tw.fmaf(a, b, c), want)
        assert tw.fmaf(-a, b, -c) == -want        # mixed signs: the mirror image


def test_block_sum_is_the_kernels_tree():
    v = np.arange(256, dtype=np.float64) + 0.5
    assert tw.block_sum(v) == v.sum()
    # non-associative f32 values: the butterfly pairs lane i with lane i ^ 32 first
    x = np.zeros(256, F32)
    x[0], x[1], x[33] = F32(1.0), F32(2.0 ** -24), F32(2.0 ** -24)
    assert tw.block_sum(x) == F32(1.0) + F32(2.0 ** -23)    # lanes 1 and 33 meet first: 2^-23, which 1 then keeps
    assert (F32(1.0) + F32(2.0 ** -24)) + F32(2.0 ** -24) == F32(1.0)   # (in row order both halves would round away)


def _problems():
    """Planted perspective maps at 1000 x 1000 and 4096 x 3072 px, inlier fractions 0.1 .. 0.9, M from 4 to 5000."""
    g = np.random.default_rng(2024)
    for i in range(240):
        wh = (1000.0, 1000.0) if i % 2 else (4096.0, 3072.0)
        m = int(np.exp(g.uniform(np.log(4), np.log(5000))))
        frac = float(g.uniform(0.1, 0.9))
        h = random_perspective(g, *wh)
        yield i, wh, planted_in(g, m, frac, h, *wh)


def _rounding_band(prob, h, thr=THR):
    """Matches whose transfer error under h lies within a forward bound of f32 scoring's rounding of thr: the kernel
    forms u, v, w with fmaf and (bx w - u) / w implicitly, so near h's vanishing line (|w| small against the terms that
    cancel in u, v and w) a fraction of a pixel can be rounding."""
    a, b = prob.a, prob.b
    mag = [np.abs(h[r, 0] * a[:, 0]) + np.abs(h[r, 1] * a[:, 1]) + abs(h[r, 2]) for r in range(3)]
    w = h[2, 0] * a[:, 0] + h[2, 1] * a[:, 1] + h[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = 8 * 2.0 ** -24 * (mag[0] + mag[1] + np.abs(b).sum(axis=1) * mag[2]) / np.abs(w)
        err = np.sqrt(prob.residuals(h)[1])
    return np.abs(err - thr) <= bound + 1e-3


def _min_cross(q):
    return min(abs(ref._cross(q[i], q[j], q[k])) for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)))


def test_twin_agrees_with_the_float64_restatement():
    n_hyp = 256
    straddles = wild = 0
    for i, (w, hgt), (ka, kb, mt) in _problems():
        seed = 1000 + i
        got = tw.verify(ka, kb, mt, n_hyp=n_hyp, thr=THR, seed=seed)
        want = ref.verify(ka, kb, mt, n_hyp=n_hyp, thr=THR, seed=seed)
        prob = want["problem"]
        assert got["stats"][3] == prob.m
        # validity of every hypothesis: the same, except for a quad whose f64 |cross| lies within rounding of 1e-4
        for k in range(n_hyp):
            valid_ref = want["hyps"][k] is not None
            if bool(got["valid"][k]) == valid_ref:
                continue
            pos = ref.sample(seed, k, prob.m)
            near = [abs(_min_cross(q) - ref.DEGENERATE) for q in (prob.an[pos], prob.bn[pos])]
            assert min(near) < 1e-6, (i, k, valid_ref, near)
            straddles += 1
        # every hypothesis both find valid: the twin's count is f64 scoring of the twin's own H within the band and the f32
        # rounding bound; against the f64 hypothesis, also within the matches that the two H themselves classify
        # differently (an ill-conditioned quad, whose last bits move a residual by pixels)
        both = got["valid"] & (want["counts"] >= 0)
        for k in np.flatnonzero(both):
            h32, h64 = got["hyps"][k].astype(np.float64).reshape(3, 3), want["hyps"][k]
            slack = band(prob, h32) | _rounding_band(prob, h32)
            assert abs(int(got["counts"][k]) - int(prob.inliers(h32, THR).sum())) <= int(slack.sum()), (i, k)
            slack |= band(prob, h64) | (prob.inliers(h32, THR) != prob.inliers(h64, THR))
            assert abs(int(got["counts"][k]) - int(want["counts"][k])) <= int(slack.sum()), (i, k)
        if want["k"] is None:
            assert got["k"] is None or got["counts"][got["k"]] <= 4 + int(band(prob, got["hyps"][got["k"]]).sum()), i
            continue
        assert got["k"] is not None, i
        k, k_ref = got["k"], want["k"]
        if k != k_ref:   # only a near tie may choose another hypothesis
            assert want["hyps"][k] is not None, (i, k)
            slack = int(band(prob, want["hyps"][k]).sum()) + int(band(prob, want["hyps"][k_ref]).sum())
            assert want["counts"][k_ref] - want["counts"][k] <= slack, (i, k, k_ref)
            continue
        # the refit: the same map within 0.05 px at the frame's corners.  A wild map (a fit to fewer than 8 matches, or one
        # that sends a corner behind its vanishing line or beyond 3 frame sizes: RANSAC missed the plane) is a 4-point
        # hypothesis of an ill-conditioned quad, whose f32 and f64 solutions part by more: those are counted, not compared.
        at = np.array([[0, 0], [w, 0], [w, hgt], [0, hgt]], np.float64)
        wz = np.concatenate([at, np.ones((4, 1))], axis=1) @ want["H"][2]
        if want["stats"][0] < 8 or (wz <= 0).any() or np.abs(ref.map_points(want["H"], at)).max() > 3 * max(w, hgt):
            wild += 1
            continue
        err = np.abs(ref.map_points(got["H"].astype(np.float64), at) - ref.map_points(want["H"], at)).max()
        assert err < 0.05, (i, err, got["rounds"], got["stats"], want["stats"])
    print(f"[twin] {straddles} validity straddles, {wild} wild maps")
    assert straddles <= 2 and wild < 80, (straddles, wild)


def test_twin_finds_near_degenerate_quads_on_the_f32_side():
    """Points on a few lines plus jitter: some quads' f64 |cross| sits next to 1e-4; the twin decides each with the f32
    cross products the kernel computes, and its decision agrees with f64 everywhere else."""
    from homography_cases import near_degenerate
    ka, kb, mt = near_degenerate(np.random.default_rng(7), 300)
    prob = ref.Problem(ka, kb, mt)
    pair = tw.Pair(ka, kb, mt)
    valid, _ = pair.hypotheses(3, np.arange(4096))
    margins, disagree = [], 0
    for k in range(4096):
        pos = ref.sample(3, k, prob.m)
        qa, qb = prob.an[pos], prob.bn[pos]
        margin = min(abs(_min_cross(qa) - 1e-4), abs(_min_cross(qb) - 1e-4))
        margins.append(margin)
        if valid[k] != (prob.hypothesis(3, k) is not None):
            disagree += 1
            assert margin < 1e-6, (k, margin)
    assert min(margins) < 1e-5          # the family does put quads next to the threshold
    assert 0 < valid.sum() < 4096
