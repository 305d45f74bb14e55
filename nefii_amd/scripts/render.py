"""Novel-view rendering of a trained experiment (reference code/scripts/render.py:30-521): loads
`<exps>/<expname>/<timestamp>/checkpoints/ModelParameters/<checkpoint>.pth`, renders every view of the test split from
`--start_index` on with `--num_rays` jittered rays per pixel, in chunks of `2^memory_capacity_level // num_rays` pixels,
and writes the per-frame buffers and the light's lat-long map under a new `<timestamp>/plots`.

    python -m nefii_amd.scripts.render --conf confs_sg/conf.conf --data_split_dir_test <scene>/test --expname robot \
        --is_continue --timestamp latest --checkpoint latest --num_rays 256 --memory_capacity_level 18
    (+ torchrun --nproc-per-node N: the chunks of a frame are dealt round-robin to the ranks, rank 0 writes)
    (+ --light_sg sg_128.npy: relight under an SG light; --light_envmap sky.exr: under a lat-long HDR map, importance-sampled,
     Monte-Carlo confs only - DESIGN.md 6g; + --envmap_indirect bounce: the interreflections recomputed under that map, 6h)
    (+ --denoise [--denoise_levels 5 --denoise_sigma_normal 32 --denoise_sigma_position 0.1 --denoise_sigma_color 1]: the
     diffuse and specular light of a Monte-Carlo frame through the guided a-trous filter, so that fewer rays do - 6j;
     + --denoise_variance [--denoise_sigma_luminance 4]: the filter's colour stop guided by the per-pixel variance of the rays - 6q)
    (+ --adaptive [--adaptive_pilot_rays 16 --adaptive_max_rays 256 --adaptive_epsilon 0.01 --no_adaptive_dilate]: --num_rays
     becomes the MEAN rays per pixel; a pilot round estimates each pixel's noise and the rest of the budget goes where it is - 6t)

The frame loop is training/render.py (chunk / shard / gather / merge contract of the reference, one fixed-shape
`dist.gather` per frame instead of pickled object lists); the training-only flags of the reference's run scripts are
accepted and ignored."""
import argparse
import os
import sys
from datetime import datetime

import torch
import torch.distributed as dist

from .. import adaptive as A
from .. import conf as hocon
from .. import denoise as D
from ..training import render as R
from ..utils import general as utils

MONTE_CARLO_RENDER_TYPES = ('pt_render_indirect_mlp', 'pt_render_indirect_mlp_memsave')


DENOISE_EXTRA_KEYS = (('denoise_signals', 8),)          # what --denoise_variance adds to the frame loop's packed outputs


def denoise_params(kwargs):
    """the runners' denoise_* kwargs -> Denoiser.filter's parameters, or Denoiser.filter_variance's with denoise_variance
    (sigma_l in place of sigma_c, which is not read then); ValueError for levels outside 1 .. 8 or a bad sigma"""
    params = dict(levels=D.check_levels(kwargs.get('denoise_levels', D.DEFAULTS['levels'])),
                  sigma_n=float(kwargs.get('denoise_sigma_normal', D.DEFAULTS['sigma_n'])),
                  sigma_x=float(kwargs.get('denoise_sigma_position', D.DEFAULTS['sigma_x'])))
    if kwargs.get('denoise_variance'):
        sigma_l = kwargs.get('denoise_sigma_luminance')
        params['sigma_l'] = float(D.VARIANCE_DEFAULTS['sigma_l'] if sigma_l is None else sigma_l)
    else:
        params['sigma_c'] = float(kwargs.get('denoise_sigma_color', D.DEFAULTS['sigma_c']))
    for k in sorted(params):
        if k == 'levels':
            continue
        if not params[k] >= 0.:
            raise ValueError('denoise %s must not be negative or NaN, got %r' % (k, params[k]))
    return params


def adaptive_params(kwargs, num_rays):
    """the runner's adaptive_* kwargs -> render_frame_adaptive's parameters (the defaults are starting values, not measurements:
    tools/adaptive_rays_sweep.py reports what they do); ValueError naming the parameter"""
    pick = lambda k, default: default if kwargs.get(k) is None else kwargs[k]
    params = dict(pilot_rays=int(pick('adaptive_pilot_rays', A.default_pilot_rays(num_rays))),
                  max_rays=int(pick('adaptive_max_rays', A.default_max_rays(num_rays))),
                  epsilon=float(pick('adaptive_epsilon', A.DEFAULTS['epsilon'])),
                  dilate=bool(pick('adaptive_dilate', A.DEFAULTS['dilate'])))
    A.check_params(num_rays, params['pilot_rays'], params['max_rays'], params['epsilon'])
    return params


def write_rays_image(out, img_res, plots_dir, index):
    """<index>-rays.png: the rays each pixel got over the most a pixel may get, in grey"""
    import numpy as np
    from PIL import Image
    share = out['adaptive_rays'].reshape(img_res[0], img_res[1]).float() / float(out['meta']['max_rays'])
    grey = (share.clamp(0., 1.).cpu().numpy() * 255.).astype(np.uint8)
    Image.fromarray(grey).save(os.path.join(plots_dir, '%03d-rays.png' % index))


class RenderRunner:
    def __init__(self, **kwargs):
        torch.set_default_dtype(torch.float32)
        self.local_rank = kwargs.get('local_rank', -1)
        self.multiprocessing = self.local_rank > -1
        if self.multiprocessing:
            torch.cuda.set_device(self.local_rank)
            if not dist.is_initialized():
                dist.init_process_group(backend=kwargs.get('dist_backend', 'nccl'))
            self.device = torch.device('cuda', self.local_rank)
            self.world_size, self.rank = dist.get_world_size(), dist.get_rank()
        else:
            self.device = torch.device('cuda')
            self.world_size, self.rank = 1, 0
        c = kwargs['conf']
        self.conf = c if isinstance(c, hocon.ConfigTree) else hocon.parse_file(c)
        self.memory_capacity_level = kwargs.get('memory_capacity_level', 18)
        self.start_index = kwargs.get('start_index', 0)
        self.num_rays = kwargs.get('num_rays', 256)
        self.coordinate_type = kwargs.get('coordinate_type', 'mitsuba')
        self.exps_folder_name = kwargs.get('exps_folder_name', 'exps')
        self.expname = kwargs.get('expname', 'default')
        self.expdir = os.path.join(self.exps_folder_name, self.expname)
        old = str(kwargs.get('old_expdir') or '') or self.expdir
        timestamp = kwargs.get('timestamp', 'latest')
        if timestamp == 'latest':                                                   # render.py:75-90
            stamps = sorted(s for s in os.listdir(old) if '.' not in s) if os.path.exists(old) else []
            if not stamps:
                raise FileNotFoundError('no experiment to render under ' + old)
            timestamp = stamps[-1]
        ckpt = os.path.join(old, timestamp, 'checkpoints', 'ModelParameters', str(kwargs.get('checkpoint', 'latest')) + '.pth')
        self.timestamp = kwargs.get('new_timestamp') or '{:%Y_%m_%d_%H_%M_%S}'.format(datetime.now())
        self.plots_dir = os.path.join(self.expdir, self.timestamp, 'plots')
        if self.rank == 0:
            os.makedirs(self.plots_dir, exist_ok=True)
            with open(os.path.join(self.expdir, self.timestamp, 'runcmd.txt'), 'w') as f:
                f.write('shell command : {0}'.format(' '.join(sys.argv)))

        ds_cls = kwargs.get('dataset_class') or self.conf.get_string('train.dataset_class')
        sub = kwargs.get('subsample', 1) * kwargs.get('vis_subsample', 1)
        self.test_dataset = utils.get_class(ds_cls)(kwargs.get('gamma', 1.0), kwargs.get('data_split_dir_test', ''), False,
                                                    sub, **kwargs.get('dataset_kwargs', {}))
        model_cls = kwargs.get('model_class') or self.conf.get_string('train.model_class')
        self.model = utils.get_class(model_cls)(conf=self.conf.get_config('model')).to(self.device)
        saved = torch.load(ckpt, map_location=self.device)
        self.model.load_state_dict(saved['model_state_dict'])
        if kwargs.get('light_sg_path') and os.path.exists(kwargs['light_sg_path']):
            self.model.envmap_material_network.load_light(kwargs['light_sg_path'])
        if kwargs.get('light_envmap_path'):                  # every rank loads the map light
            from ..lighting import EnvmapLight
            self.model.set_envmap_light(EnvmapLight.from_exr(
                kwargs['light_envmap_path'], self.coordinate_type, height=kwargs.get('envmap_height'),
                width=kwargs.get('envmap_width'), scale=kwargs.get('envmap_scale', 1.0), device=self.device),
                indirect=kwargs.get('envmap_indirect') or 'mlp')
        elif (kwargs.get('envmap_indirect') or 'mlp') != 'mlp':
            raise ValueError('envmap_indirect=%r needs a map light (light_envmap_path)' % kwargs['envmap_indirect'])
        self.model.freeze_geometry()
        self.model.eval()
        self.denoise = bool(kwargs.get('denoise', False))                           # off by default
        if self.denoise:
            self.denoise_params = denoise_params(kwargs)
            render_type = self.conf.get_string('model.render_type', default='sg')
            if render_type not in MONTE_CARLO_RENDER_TYPES:
                raise ValueError('denoise needs a Monte-Carlo conf (render_type pt_render_indirect_mlp), this one has %r: '
                                 'closed-form frames carry no noise' % render_type)
        self.denoise_variance = bool(kwargs.get('denoise_variance', False))         # off by default
        if self.denoise_variance and not self.denoise:
            raise ValueError('denoise_variance guides the denoiser: it needs denoise=True')
        if kwargs.get('denoise_sigma_luminance') is not None and not self.denoise_variance:
            raise ValueError('denoise_sigma_luminance is read with denoise_variance=True only')
        if self.denoise_variance and self.num_rays < 2:
            raise ValueError('denoise_variance: a variance needs at least two rays per pixel, num_rays is %d' % self.num_rays)
        self.model.pixel_moments = self.denoise_variance
        self.extra_keys = DENOISE_EXTRA_KEYS if self.denoise_variance else ()
        self.adaptive = bool(kwargs.get('adaptive', False))                         # off by default
        given = [k for k in ('adaptive_pilot_rays', 'adaptive_max_rays', 'adaptive_epsilon') if kwargs.get(k) is not None]
        if kwargs.get('adaptive_dilate') is False:
            given.append('adaptive_dilate')
        if given and not self.adaptive:
            raise ValueError('%s is read with adaptive=True only' % given[0])
        if self.adaptive:
            self.adaptive_params = adaptive_params(kwargs, self.num_rays)
            render_type = self.conf.get_string('model.render_type', default='sg')
            if render_type not in MONTE_CARLO_RENDER_TYPES:
                raise ValueError('adaptive needs a Monte-Carlo conf (render_type pt_render_indirect_mlp), this one has %r: '
                                 'closed-form frames carry no noise' % render_type)
            if self.world_size > 1:
                raise NotImplementedError('adaptive runs on one rank (world_size %d)' % self.world_size)
            if self.denoise_variance:
                raise ValueError('adaptive with denoise_variance: merging the demodulated moments of the rounds is out of scope')
        # tiered sphere tracing: per run (--trace_tier / trace_tier=...), else what the checkpoint was trained with, else the
        # model block / NEFII_TRACE_TIER (off by default)
        tt = kwargs.get('trace_tier')
        if tt is None:
            tt = saved.get('trace_tier')
        rt = getattr(self.model, 'ray_tracer', None)
        if tt is not None and rt is not None and os.environ.get('NEFII_TRACE_TIER', '') == '':
            rt.trace_tier = bool(tt)
        self.trace_tier = bool(rt.tier_for()) if rt is not None and hasattr(rt, 'tier_for') else False
        if kwargs.get('bracket_staged_eval') is not None and rt is not None and os.environ.get('NEFII_BRACKET_STAGED_EVAL', '') == '':
            rt.bracket_staged_eval = bool(kwargs['bracket_staged_eval'])

    def run(self):                                                                  # render.py:262-442
        ds = self.test_dataset
        ds.change_sampling_idx(-1)
        ds.change_sampling_rays(-1 if self.adaptive else self.num_rays)     # adaptive: the pixel centres; the rounds jitter
        written = []
        for index in range(self.start_index, len(ds)):
            idx, sample, gt = ds.collate_fn([ds[index]])
            model_input = {k: v.to(self.device) for k, v in sample.items()}
            if self.adaptive:
                out = A.render_frame_adaptive(self.model, model_input, ds.total_pixels, ds.img_res, budget=self.num_rays,
                                              memory_capacity_level=self.memory_capacity_level, world_size=self.world_size,
                                              **self.adaptive_params)
                write_rays_image(out, ds.img_res, self.plots_dir, int(idx[0]))
                print('adaptive frame %d: %s' % (int(idx[0]), out['meta']), flush=True)
            else:
                out = R.render_frame(self.model, model_input, ds.total_pixels, num_rays=max(self.num_rays, 1),
                                     memory_capacity_level=self.memory_capacity_level, rank=self.rank,
                                     world_size=self.world_size, extra_keys=self.extra_keys)
            if self.rank == 0:
                if self.denoise:
                    out = D.denoise_outputs(out, ds.img_res, variance=self.denoise_variance, **self.denoise_params)
                R.write_frame(self.model, out, gt['rgb'].to(self.device), model_input['pose'], ds.img_res, self.plots_dir,
                              int(idx[0]))
                written.append(int(idx[0]))
        if self.rank == 0:
            R.write_envmap(self.model, self.plots_dir, coordinate_type=self.coordinate_type)
        return written


def check_light_args(opt):
    """--light_envmap excludes --light_sg and needs a Monte-Carlo render_type, --envmap_indirect bounce needs
    --light_envmap: exits with a message otherwise"""
    if not opt.light_envmap:
        if getattr(opt, 'envmap_indirect', 'mlp') != 'mlp':
            raise SystemExit('--envmap_indirect %s recomputes the bounce under a map light: it needs --light_envmap'
                             % opt.envmap_indirect)
        return
    if opt.light_sg:
        raise SystemExit('--light_sg and --light_envmap are exclusive: relight under one light')
    if opt.coordinate_type not in ('mitsuba', 'blender'):
        raise SystemExit('--coordinate_type is mitsuba or blender, not %r' % opt.coordinate_type)
    for k in ('envmap_height', 'envmap_width'):
        if getattr(opt, k) is not None and getattr(opt, k) < 1:
            raise SystemExit('--%s must be positive' % k)
    render_type = hocon.parse_file(opt.conf).get_string('model.render_type', default='sg')
    if render_type not in ('pt_render_indirect_mlp', 'pt_render_indirect_mlp_memsave'):
        raise SystemExit('--light_envmap needs a Monte-Carlo conf (render_type pt_render_indirect_mlp), %s has %r'
                         % (opt.conf, render_type))


def add_denoise_args(p):
    p.add_argument('--denoise', default=False, action='store_true',
                   help='filter the diffuse and specular light of each frame with the guided a-trous denoiser (DESIGN.md 6j; '
                        'Monte-Carlo confs)')
    p.add_argument('--denoise_levels', type=int, default=D.DEFAULTS['levels'], help='filter levels, 1 .. %d' % D.MAX_LEVELS)
    p.add_argument('--denoise_sigma_normal', type=float, default=D.DEFAULTS['sigma_n'], help='exponent of the normal term')
    p.add_argument('--denoise_sigma_position', type=float, default=D.DEFAULTS['sigma_x'],
                   help='width of the tangent-plane term (sine of the angle out of the plane)')
    p.add_argument('--denoise_sigma_color', type=float, default=D.DEFAULTS['sigma_c'],
                   help='width of the relative-luminance term at level 0 (halved per level; inf: off); not read with '
                        '--denoise_variance')
    p.add_argument('--denoise_variance', default=False, action='store_true',
                   help='with --denoise: estimate the variance of each pixel from its rays and let it scale the luminance stop '
                        '(DESIGN.md 6q; --num_rays of at least 2; --denoise_sigma_color is not read in this mode)')
    p.add_argument('--denoise_sigma_luminance', type=float, default=None,
                   help='with --denoise_variance: width of the luminance stop in local standard deviations, the same at every '
                        'level (default %g; inf: off)' % D.VARIANCE_DEFAULTS['sigma_l'])


def check_denoise_args(opt):
    """--denoise needs a Monte-Carlo render_type, 1 .. 8 levels and sigmas that are not negative; --denoise_variance needs
    --denoise and two rays per pixel, --denoise_sigma_luminance needs --denoise_variance: exits with a message otherwise"""
    if opt.denoise_variance and not opt.denoise:
        raise SystemExit('--denoise_variance guides the denoiser: it needs --denoise')
    if opt.denoise_sigma_luminance is not None and not opt.denoise_variance:
        raise SystemExit('--denoise_sigma_luminance is read with --denoise_variance only')
    if opt.denoise_variance and opt.num_rays < 2:
        raise SystemExit('--denoise_variance: a variance needs at least two rays per pixel, --num_rays is %d' % opt.num_rays)
    if not opt.denoise:
        return
    try:
        denoise_params(denoise_kwargs(opt))
    except ValueError as e:
        raise SystemExit('--denoise: %s' % e)
    render_type = hocon.parse_file(opt.conf).get_string('model.render_type', default='sg')
    if render_type not in MONTE_CARLO_RENDER_TYPES:
        raise SystemExit('%s needs a Monte-Carlo conf (render_type pt_render_indirect_mlp), %s has %r: closed-form '
                         'frames carry no noise' % ('--denoise_variance' if opt.denoise_variance else '--denoise', opt.conf,
                                                    render_type))


def add_adaptive_args(p):
    """the flags of --adaptive; a flag that is not given leaves no attribute behind, so that a line without them parses to
    what it always did"""
    p.add_argument('--adaptive', default=argparse.SUPPRESS, action='store_true',
                   help='adaptive sampling (DESIGN.md 6t; Monte-Carlo confs, one rank): --num_rays becomes the MEAN rays per '
                        'pixel, a pilot round estimates the noise of each pixel and the rest goes where it is')
    p.add_argument('--adaptive_pilot_rays', type=int, default=argparse.SUPPRESS,
                   help='rays of a round, the pilot included (default max(2, num_rays // 4))')
    p.add_argument('--adaptive_max_rays', type=int, default=argparse.SUPPRESS,
                   help='the most rays of a pixel, a multiple of the pilot (default 4 * num_rays)')
    p.add_argument('--adaptive_epsilon', type=float, default=argparse.SUPPRESS,
                   help='added to the mean luminance under the relative deviation (default %g)' % A.DEFAULTS['epsilon'])
    p.add_argument('--no_adaptive_dilate', default=argparse.SUPPRESS, action='store_true',
                   help="score a pixel by its own rays alone instead of the largest score of its 3 x 3 neighbourhood")


def adaptive_kwargs(opt):
    """the runner's adaptive_* kwargs: none without --adaptive"""
    if not getattr(opt, 'adaptive', False):
        return {}
    return dict(adaptive=True, adaptive_pilot_rays=getattr(opt, 'adaptive_pilot_rays', None),
                adaptive_max_rays=getattr(opt, 'adaptive_max_rays', None), adaptive_epsilon=getattr(opt, 'adaptive_epsilon', None),
                adaptive_dilate=False if getattr(opt, 'no_adaptive_dilate', False) else None)


def check_adaptive_args(opt, parser, ranks=1):
    """the refusals of --adaptive, each naming its flag, through parser.error (exit status 2) before a runner is built"""
    adaptive = getattr(opt, 'adaptive', False)
    for name in ('adaptive_pilot_rays', 'adaptive_max_rays', 'adaptive_epsilon', 'no_adaptive_dilate'):
        if hasattr(opt, name) and not adaptive:
            parser.error('--%s is read with --adaptive only' % name)
    if not adaptive:
        return
    pilot = getattr(opt, 'adaptive_pilot_rays', A.default_pilot_rays(opt.num_rays))
    most = getattr(opt, 'adaptive_max_rays', A.default_max_rays(opt.num_rays))
    epsilon = getattr(opt, 'adaptive_epsilon', A.DEFAULTS['epsilon'])
    if pilot < 2 or pilot > opt.num_rays:
        parser.error('--adaptive_pilot_rays must lie in 2 .. --num_rays = %d, got %d' % (opt.num_rays, pilot))
    if most < opt.num_rays or most % pilot:
        parser.error('--adaptive_max_rays must be at least --num_rays = %d and a multiple of --adaptive_pilot_rays = %d, got %d'
                     % (opt.num_rays, pilot, most))
    if most // pilot > A.MAX_ROUNDS:
        parser.error('--adaptive_max_rays / --adaptive_pilot_rays: at most %d rounds, got %d' % (A.MAX_ROUNDS, most // pilot))
    if not 0. < epsilon < float('inf'):
        parser.error('--adaptive_epsilon must be positive and finite, got %r' % epsilon)
    try:
        A.check_params(opt.num_rays, pilot, most, epsilon)
    except ValueError as e:
        parser.error('--adaptive: %s' % e)
    render_type = hocon.parse_file(opt.conf).get_string('model.render_type', default='sg')
    if render_type not in MONTE_CARLO_RENDER_TYPES:
        parser.error('--adaptive needs a Monte-Carlo conf (render_type pt_render_indirect_mlp), %s has %r: closed-form frames '
                     'carry no noise' % (opt.conf, render_type))
    if ranks > 1:
        parser.error('--adaptive runs on one rank, this launch has %d' % ranks)
    if opt.denoise_variance:
        parser.error('--adaptive with --denoise_variance: merging the demodulated moments of the rounds is out of scope')


def denoise_kwargs(opt):
    return dict(denoise=opt.denoise, denoise_levels=opt.denoise_levels, denoise_sigma_normal=opt.denoise_sigma_normal,
                denoise_sigma_position=opt.denoise_sigma_position, denoise_sigma_color=opt.denoise_sigma_color,
                denoise_variance=opt.denoise_variance, denoise_sigma_luminance=opt.denoise_sigma_luminance)


def add_render_args(p):
    """the arguments scripts/render.py and scripts/vis_rotate_envlight.py share, the denoiser's aside (add_denoise_args)"""
    p.add_argument('--conf', type=str, required=True)
    p.add_argument('--data_split_dir', type=str, default='')
    p.add_argument('--data_split_dir_test', type=str, default='')
    p.add_argument('--gamma', type=float, default=1.0)
    p.add_argument('--subsample', type=int, default=1)
    p.add_argument('--vis_subsample', type=int, default=1)
    p.add_argument('--expname', type=str, default='')
    p.add_argument('--exps_folder_name', '--exps_folder', dest='exps_folder', type=str, default='exps')
    p.add_argument('--old_expdir', type=str, default='')
    p.add_argument('--is_continue', default=False, action='store_true')
    p.add_argument('--timestamp', default='latest', type=str)
    p.add_argument('--checkpoint', default='latest', type=str)
    p.add_argument('--memory_capacity_level', type=int, default=18)
    p.add_argument('--coordinate_type', type=str, default='mitsuba')
    p.add_argument('--light_sg', type=str, default='')
    p.add_argument('--light_envmap', type=str, default='',
                   help='relight under this lat-long HDR map (.exr), importance-sampled (DESIGN.md 6g; Monte-Carlo confs)')
    p.add_argument('--envmap_height', type=int, default=None, help='resample the map to this height (default: its own)')
    p.add_argument('--envmap_width', type=int, default=None, help='resample the map to this width (default: its own)')
    p.add_argument('--envmap_scale', type=float, default=1.0, help='exposure scale applied to the map when loaded')
    p.add_argument('--envmap_indirect', type=str, default='mlp', choices=('mlp', 'bounce'),
                   help='light at the secondary hits under --light_envmap: the trained radiance network (mlp: the training '
                        "light's interreflections) or one bounce recomputed under the map (bounce, DESIGN.md 6h)")
    p.add_argument('--start_index', type=int, default=0, help='start index')
    p.add_argument('--num_rays', type=int, default=256, help='ray number')
    p.add_argument('--local_rank', type=int, default=-1)
    p.add_argument('--model_class', type=str, default='nefii_amd.model.implicit_differentiable_renderer.IDRNetwork')
    p.add_argument('--dataset_class', type=str, default='')


def runner_kwargs(opt):
    """the keyword arguments both scripts' runners are built with, from the parsed add_render_args / add_denoise_args"""
    return dict(conf=opt.conf, data_split_dir_test=opt.data_split_dir_test or opt.data_split_dir, gamma=opt.gamma,
                subsample=opt.subsample, vis_subsample=opt.vis_subsample, expname=opt.expname or 'default',
                exps_folder_name=opt.exps_folder, old_expdir=opt.old_expdir, timestamp=opt.timestamp,
                checkpoint=opt.checkpoint, memory_capacity_level=opt.memory_capacity_level,
                coordinate_type=opt.coordinate_type, light_sg_path=opt.light_sg, light_envmap_path=opt.light_envmap,
                envmap_height=opt.envmap_height, envmap_width=opt.envmap_width, envmap_scale=opt.envmap_scale,
                envmap_indirect=opt.envmap_indirect, start_index=opt.start_index, num_rays=opt.num_rays,
                model_class=opt.model_class, dataset_class=opt.dataset_class or None, **denoise_kwargs(opt))


def main(argv=None):
    p = argparse.ArgumentParser()
    add_render_args(p)
    p.add_argument('--trace_tier', default=None, action='store_true',
                   help='tiered sphere tracing for this render (DESIGN.md 4f; default: what the checkpoint records, else off)')
    p.add_argument('--bracket_staged_eval', default=None, action='store_true',
                   help='stage the bracket search behind the measured slope bound (DESIGN.md section 4; default off)')
    add_denoise_args(p)
    add_adaptive_args(p)
    opt, _ignored = p.parse_known_args(argv)
    check_light_args(opt)
    check_denoise_args(opt)
    local_rank = opt.local_rank if opt.local_rank > -1 else (int(os.environ['LOCAL_RANK']) if 'RANK' in os.environ else -1)
    check_adaptive_args(opt, p, ranks=int(os.environ.get('WORLD_SIZE', '1')) if local_rank > -1 else 1)
    RenderRunner(trace_tier=opt.trace_tier, bracket_staged_eval=opt.bracket_staged_eval, local_rank=local_rank,
                 **adaptive_kwargs(opt), **runner_kwargs(opt)).run()


if __name__ == '__main__':
    main()
