#!/usr/bin/env python3
"""LF_MKD_POOL_F16X3 descriptors, shader and exact angle, of tests/blur_halo_cases.py's patches, as
tests/golden/blur_halo_f16x3_<angle>_rows.npy (88 KiB each); tests/test_gpu_blur_halo.py holds a build to these bits.  Run on
the build whose bits are to be kept (LF_MKD_LIB=...):
    tools/dump_blur_halo_rows.py OUT_DIR"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import local_features_python as lfp
from blur_halo_cases import halo_patches

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
patches = halo_patches()
n = len(patches)
p = torch.from_numpy(patches).cuda()
for angle, aname in ((lfp.ANGLE_SHADER, "shader"), (lfp.ANGLE_EXACT, "exact")):
    h = lfp.MkdHandle(max_features=n, angle_mode=angle, pool_mode=lfp.POOL_F16X3)
    out = torch.empty((n, 128), device="cuda")
    h.describe_patches_device(p.data_ptr(), n, out.data_ptr())
    h.synchronize()
    np.save(os.path.join(out_dir, f"blur_halo_f16x3_{aname}_rows.npy"), out.cpu().numpy())
    print(f"blur_halo_f16x3_{aname}_rows.npy written ({lfp.LIB_PATH})")
