#!/usr/bin/env python3
"""What a winding-number sign costs Step 1 on one GPU, on the torus meshes of tools/mesh_sdf_bench.py.

    python tools/mesh_winding_bench.py [--faces 2304,36864,262144,1048576] [--samples 16384] [--window 1.0] [--rounds 3]
                                       [--brute_points 1024] [--json out.json]

Per mesh (a closed torus of nu x nu/2 quads, R 0.6, r 0.25), on one SDFSampler.sample() worth of points (47/50 of them next to
the surface, the rest in the unit ball):
  moments    mesh_bvh.build_moments on the device, the one-off cost per mesh on top of the tree
  winding    MeshSDF(method='bvh').winding at beta 0 (every face), 2 and 4: the Morton sort of the queries and the kernel
  parity     the parity pass, as the parent commit runs it: signed minus unsigned MeshSDF.__call__ (one launch runs both passes)
  signed     MeshSDF.__call__ under sign='parity' and under sign='winding' at beta 2: what Step 1 pays per batch
  brute      MeshSDF(method='brute').winding, dense torch, on --brute_points of the points, scaled to --samples
Timing: device events around synchronised work, every shape warmed first, each window repeats the call until --window seconds
have passed, the variants alternate over --rounds rounds in this one process; a figure is the median of the rounds' per-call
times with their min and max.  The brute figures are multiplied by samples / brute_points (dense torch ops in chunks of
MeshSDF.pair_budget pairs: their cost is points x faces) and carry "scaled": true; no kernel figure is scaled.  Results are
compared while they are there: the largest |w - w_brute| on the brute points is printed per beta.  Fails without a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_sdf_bench import alternate, scaled, show, torus_mesh  # noqa: E402

BETAS = (0.0, 2.0, 4.0)


def bench_mesh(a, nu, dev):
    from nefii_amd.datasets.sdf_dataset import MeshSDF, SDFSampler
    from nefii_amd.mesh_bvh import build_moments
    verts, faces = torus_mesh(nu, nu // 2)
    F = len(faces)
    out = {'faces': F, 'samples': a.samples}
    sampler = SDFSampler(None, a.samples, device=dev, mesh=(verts, faces), method='bvh')
    parity = sampler.mesh_sdf
    pts = (sampler.sample(torch.Generator().manual_seed(0))[0] - torch.as_tensor(sampler.center, device=dev)) / sampler.scale
    v, f = (verts - sampler.center) / sampler.scale, faces
    tree = {b: MeshSDF(v, f, device=dev, method='bvh', sign='winding', winding_beta=b) for b in BETAS}
    for m in tree.values():
        m._bvh = parity.bvh                                         # one tree, one set of moments
    brute = MeshSDF(v, f, device=dev, method='brute', sign='winding')

    def moments():
        parity.bvh.node_moment = None
        build_moments(parity.bvh)
    out['moments'] = alternate({'moments': moments}, min(a.window, 0.5), a.rounds)['moments']
    out['levels'] = parity.bvh.levels
    print('%8d faces, %d tree levels: %s' % (F, parity.bvh.levels, show('moments', out['moments'])), flush=True)

    sub = pts[:a.brute_points]
    w_brute = brute.winding(sub)
    out['max_abs_diff'] = {str(b): (tree[b].winding(sub) - w_brute).abs().max().item() for b in BETAS}
    d_w, d_p = tree[2.0](pts), parity(pts)
    out['sign_disagreements'] = int((torch.signbit(d_w) != torch.signbit(d_p)).sum())
    print('          max |w - w_brute| over %d points: %s; signs unlike parity at beta 2: %d of %d' % (
        sub.shape[0], ', '.join('beta %g: %.3g' % (b, out['max_abs_diff'][str(b)]) for b in BETAS),
        out['sign_disagreements'], pts.shape[0]), flush=True)

    fns = {'winding_beta_0': lambda: tree[0.0].winding(pts),
           'winding_beta_2': lambda: tree[2.0].winding(pts),
           'winding_beta_4': lambda: tree[4.0].winding(pts),
           'signed_parity': lambda: parity(pts),
           'unsigned': lambda: parity(pts, signed=False),
           'signed_winding_beta_2': lambda: tree[2.0](pts),
           'brute_winding': lambda: brute.winding(sub)}
    r = alternate(fns, a.window, a.rounds)
    r['brute_winding'] = scaled(r['brute_winding'], pts.shape[0] / sub.shape[0])
    out['timing'] = r
    out['parity_pass_ms'] = r['signed_parity']['median'] - r['unsigned']['median']
    for k in fns:
        print('          %s' % show('%-22s' % k, r[k]), flush=True)
    print('          parity pass (signed - unsigned) %.3f ms; winding beta 2 / parity pass = %.2f' % (
        out['parity_pass_ms'], r['winding_beta_2']['median'] / max(out['parity_pass_ms'], 1e-9)), flush=True)
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--faces', type=str, default='2304,36864,262144,1048576')
    p.add_argument('--samples', type=int, default=16384)
    p.add_argument('--window', type=float, default=1.0)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--brute_points', type=int, default=1024)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print('mesh_winding_bench: no GPU - nothing here can be timed without one', file=sys.stderr)
        return 1
    dev = torch.device('cuda')
    res = []
    for F in (int(x) for x in a.faces.split(',') if x):
        nu = int(round(F ** 0.5))
        if nu * (nu // 2) * 2 != F:
            print('mesh_winding_bench: --faces takes squares of even numbers (nu x nu/2 quads), got %d' % F, file=sys.stderr)
            return 2
        res.append(bench_mesh(a, nu, dev))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'meshes': res}, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
