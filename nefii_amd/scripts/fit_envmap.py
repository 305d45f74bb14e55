"""Fit a spherical-Gaussian light to an HDR environment map (reference code/envmaps/fit_envmap_with_sg.py, with
envmaps/rotate_lightsg.py as --rotate):

    python -m nefii_amd.scripts.fit_envmap --envmap sky.exr [--out_dir sky/] [--num_lobes 128] [--iters 100000] \
        [--height 256 --width 512] [--coordinate_type mitsuba|blender] [--lr 1e-2] [--seed 0] [--log_every 100] \
        [--rotate Y,X,Z]

The map (its first three channels) is resampled to height x width by pixel coverage (cv2.INTER_AREA when shrinking),
the light is resumed from <out_dir>/sg_<M>.npy when that file exists (fresh Adam moments, as the reference does), and
the fit runs on the GPU in chunks of --log_every iterations: one library call and one host read of its losses each.
Writes sg_<M>.npy (float32 [M, 7], for scripts/render.py --light_sg / EnvmapMaterialNetwork.load_light),
log_im_<M>.png (target above fit, x^(1/2.2) clipped) and envmap_<M>.exr (the fitted map); with --rotate also
sg_<M>_rot.npy (Euler angles in degrees, 'yxz' order)."""
import argparse
import os
import sys
import time

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser(description='fit spherical-Gaussian lights to an HDR environment map (GPU)')
    p.add_argument('--envmap', required=True, help='HDR environment map (.exr, lat-long)')
    p.add_argument('--out_dir', default=None, help='output directory (default: the map path without extension)')
    p.add_argument('--num_lobes', type=int, default=128)
    p.add_argument('--iters', type=int, default=100000, help='Adam iterations of this run')
    p.add_argument('--height', type=int, default=256)
    p.add_argument('--width', type=int, default=512)
    p.add_argument('--coordinate_type', choices=['mitsuba', 'blender'], default='mitsuba')
    p.add_argument('--lr', type=float, default=1e-2)
    p.add_argument('--seed', type=int, default=0, help='seed of the initial lobes')
    p.add_argument('--log_every', type=int, default=100, help='iterations per chunk (one loss line each)')
    p.add_argument('--save_every', type=int, default=1000,
                   help='iterations between writes of the image artefacts (sg_<M>.npy is written every chunk)')
    p.add_argument('--rotate', default=None, help='Y,X,Z Euler angles in degrees: also write sg_<M>_rot.npy')
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.num_lobes < 1 or args.num_lobes > 512:
        raise SystemExit('--num_lobes must be in 1..512')
    if args.iters < 0 or args.log_every < 1 or args.save_every < 1 or args.height < 1 or args.width < 1:
        raise SystemExit('--iters must be >= 0; --log_every, --save_every, --height, --width >= 1')
    if args.rotate is not None:
        try:
            args.rotate = [float(v) for v in args.rotate.split(',')]
        except ValueError:
            raise SystemExit('--rotate takes three comma-separated angles, Y,X,Z')
        if len(args.rotate) != 3:
            raise SystemExit('--rotate takes three comma-separated angles, Y,X,Z')
    if args.out_dir is None:
        args.out_dir = os.path.splitext(os.path.abspath(args.envmap))[0]
    return args


def load_target(path, H, W):
    """the map's first three channels (a single-channel map repeated), resampled to [H, W, 3] float32"""
    from ..lighting import load_envmap
    try:
        return load_envmap(path, H, W)
    except ValueError as e:
        raise SystemExit(str(e))


def log_image(target, fit):
    """the reference's log_im: target above fit, x^(1/2.2) clipped to [0, 1], uint8"""
    im = np.concatenate((target, fit), axis=0)
    im = np.clip(np.power(np.maximum(im, 0.), 1. / 2.2), 0., 1.)
    return np.uint8(im * 255.)


def write_artefacts(fitter, target, out_dir, H, W, images=True):
    from PIL import Image
    from ..utils import exr
    M = fitter.num_lobes
    np.save(os.path.join(out_dir, 'sg_%d.npy' % M), fitter.lgtSGs.cpu().numpy().astype(np.float32))
    if images:
        fit = fitter.render().reshape(H, W, 3).cpu().numpy()
        Image.fromarray(log_image(target, fit)).save(os.path.join(out_dir, 'log_im_%d.png' % M))
        exr.imwrite(os.path.join(out_dir, 'envmap_%d.exr' % M), fit)


def main(argv=None):
    args = parse_args(argv)
    from ..lighting import SGEnvmapFitter, rotate_light_sgs
    from ..training.render import envmap_directions
    if not torch.cuda.is_available():
        raise SystemExit('fit_envmap needs a GPU (the fit runs in libnefii_hip.so)')
    H, W, M = args.height, args.width, args.num_lobes
    target = load_target(args.envmap, H, W)
    os.makedirs(args.out_dir, exist_ok=True)
    dirs = envmap_directions(H, W, coordinate_type=args.coordinate_type)
    fitter = SGEnvmapFitter(torch.from_numpy(target), dirs, num_lobes=M, seed=args.seed, lr=args.lr)
    resume = os.path.join(args.out_dir, 'sg_%d.npy' % M)
    if os.path.isfile(resume):
        print('Loading: ', resume)
        fitter.load({'lgtSGs': torch.from_numpy(np.load(resume))})
    print('%s: %d x %d, %d lobes, %s convention -> %s' % (args.envmap, H, W, M, args.coordinate_type, args.out_dir))
    t0, done, last_save = time.time(), 0, 0
    while done < args.iters:
        k = min(args.log_every, args.iters - done)
        losses = fitter.fit(k)
        print('step: %d, loss: %.6g  (step %d: %.6g)  %.1f s' % (
            done, losses[0].item(), done + k - 1, losses[-1].item(), time.time() - t0), flush=True)
        done += k
        images = done - last_save >= args.save_every or done == args.iters
        write_artefacts(fitter, target, args.out_dir, H, W, images=images)
        if images:
            last_save = done
    if args.iters == 0:
        write_artefacts(fitter, target, args.out_dir, H, W)
    loss = fitter.loss_grad()[0].item()
    print('final loss: %.6g' % loss)
    if args.rotate is not None:
        rot = rotate_light_sgs(fitter.lgtSGs.cpu().numpy(), args.rotate, seq='yxz', degrees=True)
        np.save(os.path.join(args.out_dir, 'sg_%d_rot.npy' % M), rot.astype(np.float32))
    return 0


if __name__ == '__main__':
    sys.exit(main())
