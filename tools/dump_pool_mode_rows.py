#!/usr/bin/env python3
"""Descriptors of 256 seeded patches in the pooling modes that LF_MKD_POOL_F16X3's changes must leave alone -- LF_MKD_POOL_F32
and LF_MKD_POOL_F16_FP6, shader and exact angle -- as tests/golden/pool_<mode>_<angle>_rows.npy (128 KiB each);
tests/test_gpu_odd_cart.py holds a build to these bits.  Run on the build whose bits are to be kept (LF_MKD_LIB=...):
    tools/dump_pool_mode_rows.py OUT_DIR"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-features_amd"))
import numpy as np
import torch
import local_features_python as lfp

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
p = torch.from_numpy(np.random.default_rng(0xB175).random((256, 32, 32), dtype=np.float32)).cuda()
for pool, pname in ((lfp.POOL_F32, "f32"), (lfp.POOL_F16_FP6, "fp6")):
    for angle, aname in ((lfp.ANGLE_SHADER, "shader"), (lfp.ANGLE_EXACT, "exact")):
        h = lfp.MkdHandle(max_features=256, angle_mode=angle, pool_mode=pool)
        out = torch.empty((256, 128), device="cuda")
        h.describe_patches_device(p.data_ptr(), 256, out.data_ptr())
        h.synchronize()
        np.save(os.path.join(out_dir, f"pool_{pname}_{aname}_rows.npy"), out.cpu().numpy())
        print(f"pool_{pname}_{aname}_rows.npy written")
