"""CPU test of the factors LF_MKD_POOL_F16X3 pools the x-odd cartesian kernels with (csrc/mkd_consts.cpp, odd_cart_*).

The kernel spends no matrix instruction on the three x-odd cartesian kernels EC 6, 7, 8: for each of the seven streams it
sums gy_b(y) * sum_{x<16} fx(x) (s(x, y) - s(31-x, y)) and multiplies by the stream's von-Mises coefficient c_k.  That is
the reference's pooling of descriptor entries 175 + 9 i + 6 + b (in-dim i, stream i) exactly when
    c_k EC_{6+b}(x, y) = c_k * fx(min(x, 31-x)) * (+1 for x < 16, -1 otherwise) * gy_b(y),
which is what this file checks, against the same expected matrix tests/test_fold_tables.py builds."""
import ctypes

import numpy as np
import pytest

import local_features_python as lfp
from test_fold_tables import VM_N3_K8, expected_matrix


@pytest.fixture(scope="module")
def factors(oracle):
    L = lfp.load_library()
    ga = np.zeros(1024, np.float32)
    ep = np.zeros(25 * 1024, np.float32)
    ec = np.zeros(9 * 1024, np.float32)
    assert L.lf_mkd_build_constants(oracle.mean.ctypes.data, oracle.eigvals.ctypes.data, oracle.eigvecs.ctypes.data,
                                    ga.ctypes.data, ep.ctypes.data, ec.ctypes.data, None) == 0
    fx = np.full(16, np.nan, np.float32)
    gy = np.full((32, 4), np.nan, np.float32)
    defect = ctypes.c_float(-1)
    fn = L.lfmkd_test_pool_factors
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.POINTER(ctypes.c_float)]
    fn.restype = ctypes.c_int
    assert fn(oracle.mean.ctypes.data, oracle.eigvals.ctypes.data, oracle.eigvecs.ctypes.data, fx.ctypes.data,
              gy.ctypes.data, ctypes.byref(defect)) == 0
    E = expected_matrix(ga.astype(np.float64).reshape(32, 32), ep.astype(np.float64).reshape(25, 32, 32),
                        ec.astype(np.float64).reshape(9, 32, 32))
    return fx.astype(np.float64), gy.astype(np.float64), float(defect.value), E


def implied_column(fx, gy, k, b):
    """[y 32, x 32]: c_k * (+-) fx(folded x) * gy_b(y)"""
    x_profile = np.concatenate([fx, -fx[::-1]])
    return VM_N3_K8[k] * gy[:, b][:, None] * x_profile[None, :]


def test_the_x_odd_cartesian_kernels_are_the_product_of_the_factors(factors):
    fx, gy, lib_defect, E = factors
    assert np.isfinite(fx).all() and np.isfinite(gy).all()
    assert (gy[:, 3] == 0.0).all()                 # the pad
    worst, worst_at, n = 0.0, None, 0
    for i in range(7):                             # in-dim = stream: 0 m | k: cos k | k + 3: sin k
        k = 0 if i == 0 else (i if i <= 3 else i - 3)
        for b in range(3):
            d = 175 + 9 * i + 6 + b
            col = E[d, i]
            assert not np.delete(E[d], i, axis=0).any(), d      # a cartesian entry pools its own stream only
            P = implied_column(fx, gy, k, b)
            assert np.array_equal(P, -P[:, ::-1]), (d, "not exactly odd in x")
            err = np.abs(P - col).max() / np.abs(col).max()
            n += 1
            if err > worst:
                worst, worst_at = err, (d, i)
    assert n == 21
    print(f"x-odd cartesian kernels as c_k fx gy_b: worst error over the column maximum {worst:.2e} at {worst_at} "
          f"(library's defect: {lib_defect:.2e})")
    assert 0.0 <= lib_defect < 1e-6                # f32 rounding of the builder's factors, a few ulp: not structure
    assert worst <= lib_defect + 2.0 ** -23, (worst, lib_defect, worst_at)


def test_the_other_cartesian_kernels_are_even_in_x(factors):
    """what the kernel's choice of EC 6, 7, 8 rests on (build_host_consts refuses otherwise): EC 0..5 are even in x"""
    _, _, _, E = factors
    for j in range(6):
        col = E[175 + j, 0]
        assert np.abs(col - col[:, ::-1]).max() < 1e-5 * np.abs(col).max(), j
    for j in range(6, 9):
        col = E[175 + j, 0]
        assert np.abs(col + col[:, ::-1]).max() < 1e-5 * np.abs(col).max(), j
