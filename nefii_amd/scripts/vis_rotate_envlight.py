"""A turntable of the LIGHT around a trained experiment (reference code/scripts/vis_rotate_envlight.py): every view of the
test split from `--start_index` on is rendered under the light yawed about the up axis by a = 0, D, 2 D, ... < 360 degrees
(`--angle_delta D`, default 15: 24 frames), and for each view index i and angle a these files go to `--plots_dir`:

    <i>-render-<a>.png      the relit frame
    <i>-material-<a>.png    normal | albedo | diffuse | specular
    <i>-env-<a>.png         the rotated light as a lat-long map
    <i>-gt_rgb-<a>.png      the ground truth, at angle 0 only

all tone-mapped with x^(1/2.2) and clamped to [0, 1], as the reference does.

    python -m nefii_amd.scripts.vis_rotate_envlight --conf confs_sg/conf.conf --data_split_dir_test <scene>/test \
        --expname robot --timestamp latest --checkpoint latest --num_rays 256 --plots_dir turntable/
    (+ --light_sg sg_128.npy: the turntable of that SG light instead of the trained one;
     + --light_envmap sky.exr [--envmap_indirect bounce]: of a lat-long HDR map, rotated inside the kernels - DESIGN.md 6i;
     + --denoise [--denoise_levels ... as scripts/render.py]: every angle through the guided a-trous filter - 6j;
     + --denoise_variance [--denoise_sigma_luminance 4]: guided by the per-pixel variance of each angle's rays - 6q)

The light is the one the model renders under: its own SG light, `--light_sg`, or the map of `--light_envmap`.  An SG light's
lobes are rotated (lighting.rotate_light_sgs' arithmetic); a map light keeps its map and its sampling table and the
rotation enters the kernels.  The angles of a view are rendered together (training/render.render_turntable): they share the
primary pass, the material buffers, the random numbers and two of every three secondary rays.

Departure from the reference: its loop rotates the light by D BEFORE it renders, so its file `-0` already shows the light
turned by D (and its last file the light turned by 360).  Here frame a is rotated by a, starting at 0.  Monte-Carlo confs
only, single process."""
import argparse
import os

import numpy as np
import torch

from .. import conf as hocon
from .. import denoise as D
from ..training import render as R
from .render import RenderRunner, add_denoise_args, add_render_args, check_denoise_args, check_light_args, runner_kwargs


def tonemap(x):
    """the reference's clip_img(tonemap_img(x)): x^(1/2.2) clamped to [0, 1]"""
    return torch.clamp(torch.pow(x.clamp_min(0.), 1. / 2.2), 0., 1.)


def turntable_angles(angle_delta):
    """0, D, 2 D, ... < 360 for a D that divides 360"""
    if angle_delta < 1 or 360 % angle_delta != 0:
        raise ValueError('angle_delta must be a positive divisor of 360, not %r' % (angle_delta,))
    return list(range(0, 360, angle_delta))


def save_png(path, img):
    """img [H, W, 3] in [0, 1] -> 8-bit PNG"""
    from PIL import Image
    Image.fromarray((img.detach().clamp(0., 1.).cpu().numpy() * 255.).astype(np.uint8)).save(path)


class TurntableRunner(RenderRunner):
    """scripts/render.py's runner (checkpoint, dataset, lights) with the turntable as its frame loop"""

    def __init__(self, plots_dir='', angle_delta=15, env_height=256, env_width=512, **kwargs):
        self.angles = turntable_angles(angle_delta)
        if kwargs.get('local_rank', -1) > -1:
            raise NotImplementedError('the light turntable runs in a single process (multi-rank turntables are out of scope)')
        super().__init__(**kwargs)
        if plots_dir:
            self.plots_dir = plots_dir
        os.makedirs(self.plots_dir, exist_ok=True)
        self.env_height, self.env_width = env_height, env_width
        self.model.check_turntable()

    def light_maps(self, rotations):
        """the rotated light on a lat-long grid per angle, [A, H, W, 3]: compute_envmap of the rotated lobes (SG light) or
        the rotated map's radiance along envmap_directions (map light)"""
        from ..lighting import turned_light_sgs
        H, W = self.env_height, self.env_width
        light = self.model.envmap_light
        net = self.model.envmap_material_network
        if light is None:
            lgt = net.get_lgtSGs().detach()
            return torch.stack([R.compute_envmap(turned_light_sgs(lgt, rot), H, W,
                                                 upper_hemi=getattr(net, 'upper_hemi', False),
                                                 coordinate_type=self.coordinate_type)
                                for rot in rotations])
        dirs = R.envmap_directions(H, W, False, self.coordinate_type).reshape(-1, 3).to(self.device).contiguous()
        return torch.stack([light.radiance_rotations(rotations[a:a + 1], dirs).reshape(H, W, 3)
                            for a in range(rotations.shape[0])])

    def run(self):
        from ..lighting import turntable_rotations
        ds = self.test_dataset
        ds.change_sampling_idx(-1)
        ds.change_sampling_rays(self.num_rays)
        rotations = turntable_rotations(self.angles, self.coordinate_type)
        with torch.no_grad():
            envs = tonemap(self.light_maps(rotations))
        written = []
        for index in range(self.start_index, len(ds)):
            idx, sample, gt = ds.collate_fn([ds[index]])
            i = int(idx[0])
            model_input = {k: v.to(self.device) for k, v in sample.items()}
            frames = R.render_turntable(self.model, model_input, ds.total_pixels, rotations,
                                        num_rays=max(self.num_rays, 1), memory_capacity_level=self.memory_capacity_level,
                                        extra_keys=self.extra_keys)
            h, w = ds.img_res
            img = lambda t: t.reshape(-1, h * w, t.shape[-1])[0].reshape(h, w, 3).float()
            if self.denoise:            # the angles share the primary pass, hence the guides: packed once per view
                den = D.Denoiser(frames[0]['normal_values'], frames[0]['points'], frames[0]['network_object_mask'], (h, w))
                frames = [D.denoise_outputs(out, (h, w), denoiser=den, variance=self.denoise_variance, **self.denoise_params)
                          for out in frames]
            for a, out, env in zip(self.angles, frames, envs):
                name = lambda kind: os.path.join(self.plots_dir, '%d-%s-%d.png' % (i, kind, a))
                if a == 0:
                    save_png(name('gt_rgb'), tonemap(img(gt['rgb'].to(self.device))))
                save_png(name('render'), tonemap(img(out['sg_rgb_values'])))
                normal = torch.clamp((img(out['normal_values']) + 1.) / 2., 0., 1.)
                save_png(name('material'), torch.cat([normal, tonemap(img(out['sg_diffuse_albedo_values'])),
                                                      tonemap(img(out['sg_diffuse_rgb_values'])),
                                                      tonemap(img(out['sg_specular_rgb_values']))], dim=1))
                save_png(name('env'), env)
            written.append(i)
        return written


def check_turntable_args(opt):
    """--angle_delta divides 360, the conf is a Monte-Carlo one, the light arguments as scripts/render.py: exits with a
    message otherwise"""
    if opt.angle_delta < 1 or 360 % opt.angle_delta != 0:
        raise SystemExit('--angle_delta must be a positive divisor of 360, not %d' % opt.angle_delta)
    if opt.start_index < 0:
        raise SystemExit('--start_index must not be negative')
    if opt.coordinate_type not in ('mitsuba', 'blender'):
        raise SystemExit('--coordinate_type is mitsuba or blender, not %r' % opt.coordinate_type)
    if opt.local_rank > -1 or 'RANK' in os.environ:
        raise SystemExit('the light turntable runs in a single process (multi-rank turntables are out of scope)')
    check_light_args(opt)
    check_denoise_args(opt)
    render_type = hocon.parse_file(opt.conf).get_string('model.render_type', default='sg')
    if render_type not in ('pt_render_indirect_mlp', 'pt_render_indirect_mlp_memsave'):
        raise SystemExit('a light turntable needs a Monte-Carlo conf (render_type pt_render_indirect_mlp), %s has %r'
                         % (opt.conf, render_type))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='render a turntable of the light (DESIGN.md 6i)')
    add_render_args(p)
    p.add_argument('--plots_dir', type=str, default='', help='where the PNGs go (default: <exp>/<new timestamp>/plots)')
    p.add_argument('--angle_delta', type=int, default=15, help='degrees between frames; must divide 360')
    add_denoise_args(p)
    opt, _ignored = p.parse_known_args(argv)
    check_turntable_args(opt)
    return opt


def main(argv=None):
    opt = parse_args(argv)
    TurntableRunner(plots_dir=opt.plots_dir, angle_delta=opt.angle_delta, **runner_kwargs(opt)).run()


if __name__ == '__main__':
    main()
