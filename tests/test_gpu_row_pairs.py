"""GPU tests of the row pairs of mkd_pool's patch mode in LF_MKD_POOL_F16X3 (run with -m gpu on an MI355X).

That form walks a patch's middle rows two at a time over fixed ring slots (raw row r in slot r mod 6), reads every raw row
from the ring once per pair, replicates rows 0 and 31 from their own slots instead of fetching them again, and requests the
next batch's first rows while the last rows of this one are still being read (csrc/mkd_describe.hip, patch_row).  None of
that may change a bit of a descriptor: tests/golden/pool_f16x3_*_rows.npy are the rows of the build before the change
(tools/dump_f16x3_rows.py)."""
import numpy as np
import pytest

from conftest import assert_patch_parity, golden, rel_l2
from row_pairs_cases import HOT_ROWS, seeded_patches, structured_patches

pytestmark = pytest.mark.gpu

TOL = 2e-5              # tests/test_gpu_parity.py's bound for this mode against the oracle
N_WIDE = 32768 + 128 + 5   # the 8-wave form: 258 batches of 128 on at most 256 workgroups -- a workgroup runs two batches, the
                           # second requested while the first one's last rows are read -- and the last batch is ragged


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def _angle(lfp, angle):
    return lfp.ANGLE_SHADER if angle == "shader" else lfp.ANGLE_EXACT


def _describe(lfp, torch, p, angle, n):
    """descriptors (a device tensor) of the patches p tiled to n, through LF_MKD_POOL_F16X3"""
    reps = -(-n // len(p))
    h = lfp.MkdHandle(max_features=n, angle_mode=_angle(lfp, angle), pool_mode=lfp.POOL_F16X3)
    dp = torch.from_numpy(np.tile(p, (reps, 1, 1))[:n].copy()).cuda()
    out = torch.empty((n, 128), device="cuda")
    h.describe_patches_device(dp.data_ptr(), n, out.data_ptr())
    h.synchronize()
    return out


def _same_bits(got, want):
    got = np.ascontiguousarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), "entries differ, first in row", int(np.argwhere(diff)[0][0]))


@pytest.fixture(scope="module")
def oracle_rows(oracle):
    """the structured patches and the oracle's descriptors of them (the blur contracted, as the kernel's is), per angle mode"""
    from oracle import ATAN_LIBM, ATAN_SHADER, BLUR_CONTRACT
    p = structured_patches()
    ref = {name: oracle.describe_patches(p, atan_mode=mode | BLUR_CONTRACT, nthreads=8)
           for name, mode in (("shader", ATAN_SHADER), ("exact", ATAN_LIBM))}
    for v in ref.values():
        v.setflags(write=False)
    return p, ref


@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_both_workgroup_forms_keep_the_parents_bits(lfp, torch, angle):
    p = seeded_patches()
    want = golden(f"pool_f16x3_{angle}_rows.npy")
    _same_bits(_describe(lfp, torch, p, angle, 256).cpu().numpy(), want)          # one round: the 4-wave form
    wide = _describe(lfp, torch, p, angle, N_WIDE)
    for lo in range(256, N_WIDE, 256):   # every repetition has the bits of the first, the ragged tail included
        hi = min(lo + 256, N_WIDE)
        assert torch.equal(wide[lo:hi], wide[:hi - lo]), (lo, "a repeated block differs")
    _same_bits(wide[:256].cpu().numpy(), want)


@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_rows_that_show_a_wrong_slot(lfp, torch, oracle, oracle_rows, angle):
    from oracle import ATAN_LIBM, ATAN_SHADER
    p, ref = oracle_rows
    got = _describe(lfp, torch, p, angle, len(p)).cpu().numpy()
    assert np.isfinite(got).all()
    e = rel_l2(got, ref[angle])
    print(f"{angle} angle: worst relative L2 against the oracle -- rows constant along x {e[:64].max():.2e}, one row of 1.0 at "
          + ", ".join(f"y={y}: {v:.2e}" for y, v in zip(HOT_ROWS, e[64:72])) + f", random {e[72:].max():.2e}")
    assert e[:72].max() < TOL, (int(e[:72].argmax()), e[:72].max())
    assert assert_patch_parity(oracle, p[72:], got[72:], ATAN_SHADER if angle == "shader" else ATAN_LIBM,
                               what=("row pairs", angle)) < TOL
    _same_bits(got, golden(f"pool_f16x3_{angle}_structured_rows.npy"))


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("angle", ["shader", "exact"])
def test_a_lone_patch_and_a_partly_filled_wave(lfp, torch, oracle_rows, angle, n):
    """n = 1: fifteen lanes of sixteen recompute the last patch; n = 17: the second wave holds one patch"""
    p, ref = oracle_rows
    got = _describe(lfp, torch, p[72:72 + n], angle, n).cpu().numpy()
    e = rel_l2(got, ref[angle][72:72 + n])
    print(f"n = {n}, {angle} angle: worst relative L2 against the oracle {e.max():.2e}")
    assert e.max() < TOL, e.max()
