"""Adaptive sampling of Monte-Carlo frames: the rays go where the variance is.

A frame is rendered in rounds of `pilot_rays` rays per pixel.  Round 1, the pilot, covers every pixel; from each pixel's own
rays it estimates the relative standard deviation of the pixel's luminance (ops.ray_luminance_moments inside the model,
IDRNetwork.ray_stats).  The rest of a budget of `budget` rays per pixel ON AVERAGE is then handed out in whole rounds,
k_p = min(K, max(1, ceil(lambda s_p))) with the largest lambda the budget allows (ops.adaptive_allocate: the two-stage
allocation of Neyman 1934, capped and floored), and round j = 2 .. K renders the pixels with k_p >= j only.  The renderer
draws fresh jitter offsets and fresh secondary uniforms on every call, so a pixel's k_p rounds are one k_p x pilot_rays-ray
render; the rounds are merged in fp64 (ops.adaptive_merge) and averaged once (ops.adaptive_finalise).

Every round goes through training/render.py:render_frame, so the chunking is the frame loop's.  One process only.
The pilot's samples both steer the allocation and enter the mean: the known small bias of adaptive sampling (6t states it)."""
import torch

from . import ops
from .training import render as R

DEFAULTS = dict(epsilon=0.01, dilate=True)
MAX_ROUNDS = 256
EXTRA_KEYS = (('adaptive_stats', 2),)
MASK_KEYS = ('network_object_mask', 'object_mask')          # mean_pixel's all(): 1 only if set for every ray of every round


def default_pilot_rays(num_rays):
    return max(2, int(num_rays) // 4)


def default_max_rays(num_rays):
    return 4 * int(num_rays)


def check_params(budget, pilot_rays, max_rays, epsilon=DEFAULTS['epsilon']):
    """budget = mean rays per pixel, pilot_rays = rays of a round, max_rays = the most rays of a pixel -> K, the most rounds
    of a pixel; ValueError naming the parameter otherwise"""
    budget, pilot_rays, max_rays, epsilon = int(budget), int(pilot_rays), int(max_rays), float(epsilon)
    if pilot_rays < 2:
        raise ValueError('pilot_rays must be at least 2 (a variance needs two samples), got %d' % pilot_rays)
    if pilot_rays > budget:
        raise ValueError('pilot_rays must not exceed the budget of %d rays per pixel, got %d' % (budget, pilot_rays))
    if pilot_rays > ops.MOMENTS_MAX_RAYS:
        raise ValueError('pilot_rays must not exceed %d, got %d' % (ops.MOMENTS_MAX_RAYS, pilot_rays))
    if max_rays < budget:
        raise ValueError('max_rays must be at least the budget of %d rays per pixel, got %d' % (budget, max_rays))
    if max_rays % pilot_rays:
        raise ValueError('max_rays must be a multiple of pilot_rays = %d, got %d' % (pilot_rays, max_rays))
    if max_rays // pilot_rays > MAX_ROUNDS:
        raise ValueError('max_rays / pilot_rays: at most %d rounds, got %d' % (MAX_ROUNDS, max_rays // pilot_rays))
    if not (epsilon > 0. and epsilon != float('inf')):
        raise ValueError('epsilon must be positive and finite, got %r' % epsilon)
    return max_rays // pilot_rays


def uniform_jitter(uv, rays):
    """uv [1, m, 2] -> [1, m, rays, 2]: the datasets' jitter (one draw of `rays` offsets in [-0.5, 0.5)^2, shared by the
    pixels), drawn afresh on every call"""
    return uv[:, :, None, :] + (torch.rand(rays, 2) - 0.5).to(uv.device)[None, None]


def render_frame_adaptive(model, model_input, total_pixels, img_res, jitter=uniform_jitter, budget=64, pilot_rays=None,
                          max_rays=None, epsilon=DEFAULTS['epsilon'], dilate=DEFAULTS['dilate'], memory_capacity_level=18,
                          rank=0, world_size=1):
    """A whole frame at `budget` rays per pixel on average.  model_input['uv'] [1, P, 2] holds the un-jittered pixel centres in
    raster order, P = total_pixels = img_res[0] * img_res[1]; jitter(uv [1, m, 2], rays) -> [1, m, rays, 2] draws fresh
    offsets.  Returns render_frame's dict - normal_values is the pilot's (mean_pixel takes the first ray's normal; a sum of unit
    vectors is not one) - plus adaptive_rays [P] int32, adaptive_variance [P] (of the mean luminance) and meta, a dict of
    rounds run, lambda, rounds granted and left over, rays traced and active pixels per round."""
    if world_size > 1:
        raise NotImplementedError('render_frame_adaptive runs on one rank (world_size %d): a round renders the pixels the '
                                  'allocation names, and dealing those to ranks is out of scope' % world_size)
    pilot_rays = default_pilot_rays(budget) if pilot_rays is None else int(pilot_rays)
    max_rays = default_max_rays(budget) if max_rays is None else int(max_rays)
    K = check_params(budget, pilot_rays, max_rays, epsilon)
    H, W = int(img_res[0]), int(img_res[1])
    uv = model_input['uv']
    if uv.dim() != 3 or uv.shape[0] != 1 or uv.shape[1] != total_pixels or H * W != total_pixels:
        raise ValueError('uv must hold the pixel centres [1, %d, 2] of one %d x %d view, got %s'
                         % (total_pixels, H, W, tuple(uv.shape)))
    P, dev = total_pixels, uv.device
    columns = R.PACK_WIDTH
    sums = torch.zeros(P, columns, dtype=torch.float64, device=dev)
    stat = torch.zeros(P, 3, dtype=torch.float64, device=dev)

    def render_round(active):
        """one round over the pixels `active` (None: all) -> its packed rows [m, columns + 2] and its output dict"""
        data = dict(model_input)
        centres = uv if active is None else uv.index_select(1, active)
        data['uv'] = jitter(centres, pilot_rays)
        if active is not None:
            data['object_mask'] = model_input['object_mask'].index_select(1, active)
        out = R.render_frame(model, data, centres.shape[1], num_rays=pilot_rays, memory_capacity_level=memory_capacity_level,
                             extra_keys=EXTRA_KEYS)
        return R.pack_chunk(out, EXTRA_KEYS).contiguous(), out

    was = getattr(model, 'ray_stats', False)
    model.ray_stats = True
    try:
        rows, pilot = render_round(None)
        ops.adaptive_merge(rows, None, pilot_rays, sums, stat)
        score = ops.adaptive_score(stat, H, W, epsilon, dilate)
        N = budget * P // pilot_rays
        k, lam, T = ops.adaptive_allocate(score, N, K)
        active_per_round = [P]
        for j in range(2, K + 1):
            active = torch.nonzero(k >= j).flatten()
            if active.numel() == 0:
                break
            rows, _ = render_round(active)
            ops.adaptive_merge(rows, active.to(torch.int32), pilot_rays, sums, stat)
            active_per_round.append(int(active.numel()))
    finally:
        model.ray_stats = was
    mask_columns, c = [], 0
    for key, w in R.RENDER_KEYS:
        if key in MASK_KEYS:
            mask_columns.append(c)
        c += w
    merged, rays, variance = ops.adaptive_finalise(sums, stat, mask_columns)
    out = R.unpack_chunk(merged)
    out['normal_values'] = pilot['normal_values']
    out['adaptive_rays'] = rays
    out['adaptive_variance'] = variance
    out['meta'] = dict(rounds=len(active_per_round), pilot_rays=pilot_rays, max_rays=max_rays, lam=float(lam),
                       rounds_budget=int(N), rounds_granted=int(T), rounds_left=int(N - T),
                       rays_traced=pilot_rays * sum(active_per_round), active_pixels=active_per_round)
    return out
