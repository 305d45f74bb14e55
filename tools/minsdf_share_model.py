"""Shared first stage of the staged min-SDF search: what the rule (tests/test_minsdf_share_cpu.py) predicts on a bench workload's
own scene and rays, on the CPU - single-pass evaluations per search with and without the sharing.

    python tools/minsdf_share_model.py [workload=cfg3] [pixels=256] [L=2.074] [tau=0.001168]

A ray counts as searching when the lowest of its 100 samples is > 0.01 (a miss); the first searching ray of a pixel leads."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from nefii_amd import synthetic as syn      # noqa: E402
from oracle import nets, renderer as orr    # noqa: E402
import test_minsdf_share_cpu as model       # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
    pixels = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    lip = float(sys.argv[3]) if len(sys.argv) > 3 else 2.074
    tau = float(sys.argv[4]) if len(sys.argv) > 4 else 0.001168
    w = syn.WORKLOADS[name]
    mc, sd = syn.workload_state_dict(name)
    cfg = mc['implicit_network']
    inp, _ = syn.make_inputs(w['num_pixels'], w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=1)
    uv = inp['uv'][0][:pixels].reshape(1, -1, 2)
    dirs, cam = orr.camera_rays(uv.float(), inp['pose'].float(), inp['intrinsics'].float())
    d = dirs[0].double().numpy()
    o = np.repeat(cam.double().numpy(), d.shape[0], 0)

    def sdf(x):
        with torch.no_grad():
            return torch.cat([nets.sdf_forward(sd, cfg, c)[:, 0] for c in torch.from_numpy(x).float().split(1 << 17)]).double().numpy()
    s = torch.rand(100, generator=torch.Generator().manual_seed(1)).double().numpy()
    t = time.time()
    own, shared, fell, ok = model.run_waves(sdf, o, d, s, lip, tau=tau, wave=w['num_rays'], searches=lambda v: v.min(1) > 0.01)
    print('%s, %d pixels x %d rays, L %.3f, tau %.6f: %d searches; single-pass evaluations per search %.2f -> %.2f (x %.3f), '
          'shared: median %d, 90th percentile %d; %.1f %% fell back; %.0f s' % (
              name, pixels, w['num_rays'], lip, tau, len(own), own.mean(), shared.mean(), shared.sum() / own.sum(),
              np.median(shared), np.percentile(shared, 90), 100.0 * fell.mean(), time.time() - t))


if __name__ == '__main__':
    main()
