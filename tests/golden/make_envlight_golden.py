#!/usr/bin/env python3
"""tests/golden/envlight_ref.npz: the reference's `model/path_tracing_render.py:pdf_fn_constant_2d_light` on a seeded
16 x 32 lognormal map (dynamic range below 1e3), Blender axes, at directions strictly inside texels (build container
only).

    python tests/golden/make_envlight_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()
from model.path_tracing_render import pdf_fn_constant_2d_light  # noqa: E402  (reference)


def main():
    H, W, n = 16, 32, 2048
    g = np.random.Generator(np.random.Philox(23))
    envmap = np.exp(g.normal(size=(H, W, 3)) * 0.9)
    envmap = np.clip(envmap, envmap.max() / 900., None)          # dynamic range of the texel means < 1e3
    # directions at texel-interior (u, v): 5% .. 95% of each texel, Blender mapping (u = (1 - theta/pi) / 2, v = phi/pi)
    i, j = g.integers(0, H, n), g.integers(0, W, n)
    v = (i + g.uniform(0.05, 0.95, n)) / H
    u = (j + g.uniform(0.05, 0.95, n)) / W
    phi, th = np.pi * v, np.pi - 2. * np.pi * u
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], -1)
    lgt = torch.from_numpy(envmap)
    wi = torch.from_numpy(d)
    nrm = torch.zeros_like(wi)
    pdf = pdf_fn_constant_2d_light(wi, nrm, nrm, torch.ones(n, 1, dtype=torch.float64), lgt)
    out = {'envmap': envmap.astype(np.float64), 'dirs': d, 'pdf': pdf.numpy().reshape(-1).astype(np.float64)}
    np.savez_compressed(os.path.join(HERE, 'envlight_ref.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
