"""GPU tests of the run-time batch claims of mkd_pool's 8-wave patch mode (run with -m gpu on an MI355X).

A launch of at least four whole batches of 128 patches per workgroup deals only each workgroup's first batch by its id: every
later batch is a ticket drawn from a device counter, one batch ahead of the one being computed (csrc/mkd_describe.hip, the
batch loop of mkd_pool; csrc/lf_mkd.cpp clears the counter on the launch stream).  Which workgroup computes a batch changes
no bit of it, so the reference is the same patches described in chunks of one round of 64-patch workgroups: the 4-wave
form, which never claims and which tests/test_gpu_parity.py::test_full_size_properties holds bit-equal to the 8-wave form."""
import pytest

pytestmark = pytest.mark.gpu

ANGLES = ["shader", "exact"]


@pytest.fixture(scope="module")
def lfp():
    import local_features_python as m
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _n_claim(cus):
    return 128 * (4 * cus + 3) + 5      # 4 CUs + 3 batches, the last one of 5 patches: one claiming launch, ragged end


def _handle(lfp, angle, n):
    return lfp.MkdHandle(max_features=n, angle_mode=lfp.ANGLE_SHADER if angle == "shader" else lfp.ANGLE_EXACT,
                         pool_mode=lfp.POOL_F16X3)


@pytest.fixture(scope="module")
def patches(torch, cus):
    g = torch.Generator(device="cuda")
    g.manual_seed(20260)
    return torch.rand((_n_claim(cus), 32, 32), device="cuda", generator=g)


@pytest.fixture(scope="module")
def chunked(lfp, torch, cus, patches):
    """per angle mode: the descriptors of `patches`, described at most 64 x CUs at a time through a handle of its own"""
    chunk, n = 64 * cus, len(patches)
    ref = {}
    for angle in ANGLES:
        h = _handle(lfp, angle, chunk)
        out = torch.empty((n, 128), device="cuda")
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            h.describe_patches_device(patches[lo:].data_ptr(), m, out[lo:].data_ptr())
        h.synchronize()
        ref[angle] = out
    return ref


def _one_launch(lfp, torch, patches, angle, n, fill=None):
    h = _handle(lfp, angle, n)
    out = torch.empty((n, 128), device="cuda") if fill is None else torch.full((n, 128), fill, device="cuda")
    torch.cuda.synchronize()
    h.describe_patches_device(patches.data_ptr(), n, out.data_ptr())
    h.synchronize()
    return out


@pytest.mark.parametrize("angle", ANGLES)
def test_a_claiming_launch_equals_chunked_launches(lfp, torch, cus, patches, chunked, angle):
    n = _n_claim(cus)
    assert torch.equal(_one_launch(lfp, torch, patches, angle, n), chunked[angle])


@pytest.mark.parametrize("where", ["below", "above"])
@pytest.mark.parametrize("angle", ANGLES)
def test_both_sides_of_the_threshold(lfp, torch, cus, patches, chunked, angle, where):
    """128 (4 CUs) - 1 patches: the last of the 4 CUs batches is short of one patch, the static walk; a batch more claims"""
    n = 128 * (4 * cus) - 1 + (128 if where == "above" else 0)
    assert torch.equal(_one_launch(lfp, torch, patches, angle, n), chunked[angle][:n])


def test_the_counter_is_found_zero_every_time(lfp, torch, cus, patches, chunked):
    n = _n_claim(cus)
    h = _handle(lfp, "shader", n)
    outs = [torch.empty((n, 128), device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for out in outs:                                   # one handle, one stream, nothing waited for in between
        h.describe_patches_device(patches.data_ptr(), n, out.data_ptr())
    h.synchronize()
    for i, out in enumerate(outs):
        assert torch.equal(out, chunked["shader"]), i


def test_two_handles_on_two_streams_at_once(lfp, torch, cus, patches, chunked):
    n = _n_claim(cus)
    hs = [_handle(lfp, "shader", n) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [torch.empty((n, 128), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for h, s, out in zip(hs, streams, outs):           # start both ...
        h.describe_patches_device(patches.data_ptr(), n, out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()                           # ... then wait
    for i, out in enumerate(outs):
        assert torch.equal(out, chunked["shader"]), i


def test_raw_output_of_a_claiming_launch(lfp, torch, cus, patches):
    """the 238-D tap stores from the epilogue and waits with vmcnt(0): against its chunked (4-wave) twin"""
    n, chunk = _n_claim(cus), 64 * cus
    raw = []
    for size in (n, chunk):
        h = _handle(lfp, "shader", size)
        out = torch.empty((n, 238), device="cuda")
        torch.cuda.synchronize()
        for lo in range(0, n, size):
            h.raw_descriptors_device(patches[lo:].data_ptr(), min(size, n - lo), out[lo:].data_ptr())
        h.synchronize()
        raw.append(out)
    assert torch.equal(raw[0], raw[1])


def test_a_recorded_launch_whose_count_is_on_the_device(lfp, torch, cus):
    """lf_mkd_stream_* with the two-launch keypoint form: the describe launch is sized, and claims, by the capacity, the real
    count (a few hundred) is read on the device -- every ticket is beyond the last batch -- and the counter's memset is part
    of the recording: frame after frame the rows are what lf_mkd_detect gives through a small static launch."""
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from gen_golden import blob_image
    w, hgt, cap = 320, 240, 128 * (4 * cus) + 128
    kw = dict(max_image_width=w, max_image_height=hgt, max_blobs=2048, pool_mode=lfp.POOL_F16X3,
              flags=lfp.FLAG_UNFUSED_KEYPOINTS)
    h = lfp.MkdHandle(max_features=cap, **kw)
    ref = lfp.MkdHandle(max_features=1024, **kw)
    d_img = torch.zeros((hgt, w), device="cuda")
    d_k = torch.zeros((cap, 5), device="cuda")
    d_d = torch.zeros((cap, 128), device="cuda")
    d_c = torch.zeros((8,), dtype=torch.int64, device="cuda")
    h.stream_create(w, hgt, 0, 0.0, cap, d_img.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_c.data_ptr())
    for f in range(2):
        img = blob_image(w, hgt, 60 + f, 120 + 60 * f)
        d_img.copy_(torch.from_numpy(img))
        torch.cuda.synchronize()
        h.stream_frame()
        h.synchronize()
        want_k, want_d, _, _ = ref.detect(img, 0, 0.0, 1024)
        n = int(d_c[3].item())
        assert n == len(want_k) > 50, (f, n)
        assert np.array_equal(d_k[:n].cpu().numpy(), want_k)
        assert np.array_equal(d_d[:n].cpu().numpy(), want_d), f


def test_every_batch_is_computed_exactly_once(lfp, torch, cus, patches):
    """no row is left as it was, and every row is a descriptor: unit norm to 1e-5, test_full_size_properties' bound"""
    n = _n_claim(cus)
    out = _one_launch(lfp, torch, patches, "shader", n, fill=float("nan"))
    assert bool(torch.isfinite(out).all())
    norms = out.double().norm(dim=1)
    worst = float((norms - 1).abs().max())
    print(f"worst | |d| - 1 | over {n} rows: {worst:.2e}")
    assert worst < 1e-5
