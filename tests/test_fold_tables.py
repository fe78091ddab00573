"""CPU test of the folded pooling tables (csrc/mkd_consts.cpp): the LUT image a handle uploads, the K-slot map of the
kernel's operands and `colmap` together must be the reference's pooling -- embedding_polar / embedding_cartesian times the
rotation by the pixel's angle -- for every one of the 238 descriptor entries.

The kernel folds a patch row about its middle (mkd_consts.hpp): a lane (column c = lane & 15, q = lane >> 4) holds, at K slot
e = 4 half + i, the LUT value of folded pixel x = 4q + i of the column's first / second half, and the stream operands are
    M = [m_e | m_o]    U_k = [cos_e | sin_o]    V_k = [sin_e | -cos_o],    s_e(x) = s(x) + s(31-x),  s_o(x) = s(x) - s(31-x).
Accumulator tile t meets LUT tile ut under operand: t < 3: (t, M); else h = (t-3) // 6, r = (t-3) % 6: (3 + 3h + r // 2, U or V
of harmonic h + 1 as r is even or odd)."""
import ctypes

import numpy as np
import pytest

import local_features_python as lfp

VM_N3_K8 = np.array([0.37872374, 0.51796234, 0.46882015, 0.39798096], np.float32).astype(np.float64)   # mkd_consts.cpp
N_UT, N_T = 12, 21


@pytest.fixture(scope="module")
def tables(oracle):
    L = lfp.load_library()
    ga = np.zeros(1024, np.float32)
    ep = np.zeros(25 * 1024, np.float32)
    ec = np.zeros(9 * 1024, np.float32)
    assert L.lf_mkd_build_constants(oracle.mean.ctypes.data, oracle.eigvals.ctypes.data, oracle.eigvecs.ctypes.data,
                                    ga.ctypes.data, ep.ctypes.data, ec.ctypes.data, None) == 0
    lut = np.zeros(32 * N_UT * 2 * 64 * 4, np.float32)
    colmap = np.zeros(N_T * 16, np.int16)
    defect = ctypes.c_float(0)
    fn = L.lfmkd_test_pool_tables
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.POINTER(ctypes.c_float)]
    fn.restype = ctypes.c_int
    assert fn(oracle.mean.ctypes.data, oracle.eigvals.ctypes.data, oracle.eigvecs.ctypes.data, lut.ctypes.data,
              colmap.ctypes.data, ctypes.byref(defect)) == 0
    return (ga.astype(np.float64).reshape(32, 32), ep.astype(np.float64).reshape(25, 32, 32),
            ec.astype(np.float64).reshape(9, 32, 32), lut.reshape(32, N_UT, 2, 64, 4), colmap, float(defect.value))


def expected_matrix(ga, ep, ec):
    """E[d, stream, y, x]: what descriptor entry d pools of each of the seven streams (0: m, k: m cos k theta, k + 3: m sin k theta);
    shaders/common.glsl's order: polar [in-dim][kernel] (175), then cartesian [in-dim][kernel] (63)."""
    E = np.zeros((238, 7, 32, 32))
    for j in range(25):
        E[j, 0] = VM_N3_K8[0] * ep[j]
        for k in (1, 2, 3):
            pc, ps = VM_N3_K8[k] * ep[j] * np.cos(k * ga), VM_N3_K8[k] * ep[j] * np.sin(k * ga)
            E[k * 25 + j, k], E[k * 25 + j, k + 3] = pc, -ps              # relcos = cos x EPc - sin x EPs
            E[(k + 3) * 25 + j, k + 3], E[(k + 3) * 25 + j, k] = pc, ps   # relsin = sin x EPc + cos x EPs
    for i in range(7):
        for j in range(9):
            E[175 + i * 9 + j, i] = VM_N3_K8[0 if i == 0 else (i if i <= 3 else i - 3)] * ec[j]
    return E


def implied_matrix(lut, colmap):
    """the same from the folded LUT image, the operands' K-slot map and colmap; and how often each entry is produced"""
    P = np.zeros((238, 7, 32, 32))
    seen = np.zeros(238, int)
    lut = lut.astype(np.float64)
    for t in range(N_T):
        if t < 3:
            ut, halves = t, ((0, 1, 1), (0, 1, -1))                   # (stream, weight at x, weight at 31 - x) per half
        else:
            h, r = divmod(t - 3, 6)
            k, ut = h + 1, 3 + 3 * h + r // 2
            halves = ((k, 1, 1), (k + 3, 1, -1)) if r % 2 == 0 else ((k + 3, 1, 1), (k, -1, 1))
        for c in range(16):
            d = int(colmap[t * 16 + c])
            if d == -1:
                assert not lut[:, ut, :, c::16, :].any(), (t, c)   # an unused packed column pools nothing
                continue
            sign = 1.0
            if d < 0:
                d, sign = -2 - d, -1.0
            seen[d] += 1
            for half, (stream, w_x, w_mirror) in enumerate(halves):
                for q in range(4):
                    for i in range(4):
                        x = 4 * q + i
                        P[d, stream, :, x] += sign * w_x * lut[:, ut, half, c + 16 * q, i]
                        P[d, stream, :, 31 - x] += sign * w_mirror * lut[:, ut, half, c + 16 * q, i]
    return P, seen


def parity_errors(col):
    """(largest |L(x) - L(31-x)|, largest |L(x) + L(31-x)|) of a [32, 32] column"""
    m = col[:, ::-1]
    return np.abs(col - m).max(), np.abs(col + m).max()


def test_folded_tables_are_the_reference_pooling(tables):
    ga, ep, ec, lut, colmap, lib_defect = tables
    E = expected_matrix(ga, ep, ec)
    P, seen = implied_matrix(lut, colmap)
    assert (seen == 1).all(), np.flatnonzero(seen != 1)
    # the LUT's own mirror defect, from the unfolded embeddings: how far its columns are from being even or odd in x
    defect, n_cols = 0.0, 0
    worst, worst_at = 0.0, None
    for d in range(238):
        for s in range(7):
            col = E[d, s]
            mx = np.abs(col).max()
            if mx == 0.0:
                assert not P[d, s].any(), (d, s)
                continue
            n_cols += 1
            ev, od = parity_errors(col)
            defect = max(defect, min(ev, od) / mx)
            # the folded image is even or odd by construction: it must be the parity the column has
            pe, po = parity_errors(P[d, s])
            assert (pe < po) == (ev < od), (d, s, "tile assumes the wrong parity")
            assert min(pe, po) == 0.0
            err = np.abs(P[d, s] - col).max() / mx
            if err > worst:
                worst, worst_at = err, (d, s)
    assert n_cols == 25 + 150 * 2 + 63          # polar m | relcos, relsin: two streams each | cartesian
    print(f"LUT mirror defect {defect:.2e} (library: {lib_defect:.2e}); worst folded-vs-reference {worst:.2e} at {worst_at}")
    assert defect < 1e-4                         # f32 rounding of the grid and atan2, not structure
    assert worst <= defect + 2.0 ** -23, (worst, defect, worst_at)
