#!/usr/bin/env python3
"""bench.py - training rays/s of the Step-2 material-optimisation step on MI355X (BASELINE.json's metric).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]    (N>1: launched by torch.distributed.run)

Step = one full Step-2 iteration on a synthetic batch already resident in HBM: forward (camera rays, HIP
sphere tracer, SDF value/normal, radiance + material MLPs, SG shading) + IDRLoss + backward + both Adam
updates (idr_train.py:750-776).  N=1 workload = BASELINE.json configs[2] ("cfg3"), the largest single-GPU configuration
(the metric is not quoted on a config): what robot/run_s2.sh runs - conf.conf model, num_pixels 4096 x 64 rays per pixel,
128 SG lobes, MC direct + near-field indirect, a secondary-consistency step every 10th iteration - on the non-convex
stand-in scene.  N>1: every rank gets its own 4096-pixel slice of a 4096*N-pixel global batch (the dataset's contiguous
patch split) and gradients are averaged by one RCCL all-reduce per step: weak scaling, `value` = all ranks' primary rays /
max-over-ranks time.  `python bench.py --gpus N` without a launcher starts its own N ranks (torch.distributed.run, as child
processes, before anything touches a GPU).

A plain run sets up, warms up, times the K steps once and prints ONE JSON line (rank 0), the LAST line of stdout: a flat
record of < 4 KB (compact_line) - metric, value, unit, higher_is_better, dtype, ms_per_step, config.  --dump-outputs DIR also
writes what the last timed step returned (dump_outputs).  Everything else is measured only with --full: the timed region
repeated (--repeats, default 3 there, median reported), roofline, cpu_baseline and parity in the line, and the FULL record
(every definition, the nested shorter measurements of the other BASELINE configs: "cfg1", "cfg2" with its own CPU baseline
and parity, "cfg2_camera_at_1.6", "cfg4", a band of "cfg5", the earlier stand-ins of config 3) written to --full-out (default
bench_full.json beside this file; round 5's 25.8 KB single line was more than the driver parses).  --workload X measures X
alone.

The timed steps cycle over --cycle-batches distinct pixel batches (default 4: hit counts differ from step to step, as in
the runner - the padded-hit-count graphs and the trace prefetch see what they see in training).  The tiered sphere
tracing is a per-run switch: this benchmark turns it ON for every workload (config.trace_tier; NEFII_TRACE_TIER=0
for the untiered run, whose ms_per_step the line also carries as ms_per_step_untiered).

`roofline` (--full; recomputable from the numbers in the line): the tracer's SDF-evaluation kernels (eval_kernel16q: split
precision, 3 fp16 MFMAs per product; eval_kernel16s: the single-pass coarse evaluator) against the dense fp16 MFMA peak
(2.5 PFLOP/s, MI355X_MICROARCH.md) in ALGORITHMIC flops:
  frac = the SDF evaluations the kernels EXECUTED (split precision + single pass, one F_sdf each whatever the arithmetic) x
         flops_per_sdf_eval / kernel_ms_per_step / peak, the time measured live with HIP events on the launch stream over one
         extra un-timed step (rounds 2-5 called this frac_executed);
  frac_credited = the same time against the evaluations the REFERENCE's recurrences would execute (rounds 2-5's "frac"): it
         rises when the staged searches skip work - an algorithm-level figure, not a roofline fraction;
  frac_step = SURVEY.md section 8(d)'s A x rays/s / peak: A excludes the min-SDF search (dead work under frozen
         geometry), the speculative bisection nodes and the reference's repeated SDF passes, and includes the MLP and
         shading work behind the tracer; its terms are listed under roofline.step_model.
  frac_8d = the same kernel time against SURVEY 8(d)'s evaluations only (E_tr + 3 h E_tr2: WITHOUT the min-SDF search);
  sustained_peak: what a bare MFMA loop on random operands reaches on THIS device in THIS run (nefii_mfma_sustained_probe):
         MI355X is power-limited under dense fp16 MFMA work (profiles/r04/slot_probe.txt) - frac is priced against the 2.5
         PFLOP/s spec, frac_of_sustained / issued_frac_of_sustained say how far the kernels are from what the part delivers;
  board_power (N = 1): the device's hwmon power sensor sampled during the timed steps, beside the cap it is limited to.
`cpu_baseline` (--full): the CPU oracle (kind "port": a PyTorch-CPU restatement of the reference, pinned against the
reference's own outputs) running the same step on a bounded sample of the same workload on the host cores: 2 warm-ups,
best of 5, the reference's own 1-thread setting after a warm-up, host CPU model and core count.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_F16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense fp16/bf16 MFMA (never the 2:1-sparse figure)
F_SG_SHADING = 0.2e6             # closed-form SG shading fwd+bwd per hit (M = 128)
F_MC_SHADING = 0.1e6             #                         MC shading + samplers + pdfs fwd+bwd per hit


def mlp_flops(specs):
    return sum(2 * s.k_in * s.n_out for s in specs)


def host_info():
    """CPU model and PHYSICAL core count of the host (lscpu), for the CPU baseline's line."""
    info = {}
    try:
        for ln in subprocess.run(['lscpu'], capture_output=True, text=True, timeout=10).stdout.splitlines():
            k, _, v = ln.partition(':')
            info[k.strip()] = v.strip()
        cores = int(info.get('Core(s) per socket', 0)) * int(info.get('Socket(s)', 1))
        return info.get('Model name', 'unknown'), cores or (os.cpu_count() or 1), int(info.get('CPU(s)', os.cpu_count() or 1))
    except Exception:  # noqa: BLE001
        return 'unknown', os.cpu_count() or 1, os.cpu_count() or 1


def cpu_baseline(workload, sample_rays, steps=5, warmup=2, device=None, parity_pixels=128):
    """Oracle training step on the host cores, bounded sample of the workload (rank 0 only).  Also returns the
    parity of the HIP path against the oracle (identical rays and weights): relative L2 and PSNR (evaluate.py:36-44:
    20 log10(1/sqrt(MSE))) of rendered RGB and albedo over the hit pixels - on its OWN sample of `parity_pixels` pixels
    (the first pixels of the workload's batch), forward only on both sides: the timing sample is kept small for the
    clock's sake (32 pixels of config 3 hold a dozen hit pixels - too few to quote a parity figure on)."""
    from nefii_amd import synthetic as syn
    from oracle import renderer as orr
    w = dict(syn.WORKLOADS[workload])
    mc = syn.model_conf(w['model'])
    lc = syn.loss_conf(w['model'])
    R_ = w['num_rays'] if w['num_rays'] > 0 else 1
    sample_pixels = max(8, sample_rays // R_)       # ~10-30 s of CPU work in all: 2 + 5 steps and 1 + 1 on one thread
    inp, gt = syn.make_inputs(sample_pixels, w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=1)
    n_rays = inp['uv'].shape[1] * R_
    cpu_model, phys_cores, logical = host_info()

    def run(threads, n_steps, n_warm):
        torch.set_num_threads(threads)
        sd = syn.make_state_dict(mc, seed=0, scene=w.get('scene'))
        params = [v for k, v in sd.items() if not k.startswith('implicit')]
        for v in params:
            v.requires_grad_(True)
        opt = torch.optim.Adam(params, lr=5e-4)
        R = orr.Renderer(sd, mc, training=True)
        best = None
        for i in range(n_warm + n_steps):
            t0 = time.perf_counter()
            out = R.forward(inp)
            lo = orr.idr_loss(out, gt, lc)
            opt.zero_grad()
            if lo['loss'].requires_grad:        # (a sample without a single hit has nothing to differentiate)
                lo['loss'].backward()
            opt.step()
            dt = time.perf_counter() - t0
            if i >= n_warm:
                best = dt if best is None else min(best, dt)
        return n_rays / best

    # these small GEMMs stop scaling early: on the 2x64-core EPYC 9575F GPU host 16 threads was the measured
    # optimum (1 thread 253, 8: 848, 16: 1029, 32: 853, 64: 396, 128: 151 rays/s; tools/cpu_threads_probe.py)
    threads = min(16, phys_cores)
    value = run(threads, steps, warmup)
    value1 = run(1, 1, 1)
    res = {'value': value, 'unit': 'rays/s', 'cores': threads, 'kind': 'port',
           'value_1_thread': value1, 'host_cpu': cpu_model, 'host_cores': phys_cores, 'host_logical_cpus': logical,
           'sample': '%d of the workload\'s pixels (%d primary rays), best of %d steps after %d warm-ups, %d torch threads (the '
                     'measured optimum on this host class: more threads are slower; value_1_thread = the reference\'s own '
                     'setting, idr_train.py:26, one step after one warm-up)'
                     % (sample_pixels, n_rays, steps, warmup, threads)}
    parity = None
    if device is not None:
        torch.set_num_threads(threads)
        pp = max(sample_pixels, parity_pixels) // 4 * 4
        parity = parity_of(workload, oracle_reference(workload, pp), device, bench_tier())
    return res, parity


def oracle_reference(workload, pp):
    """The oracle's forward (training mode, seeded draws) on the first pp pixels of the workload's batch: what parity_of compares with."""
    from nefii_amd import synthetic as syn
    from oracle import renderer as orr
    w = dict(syn.WORKLOADS[workload])
    mc = syn.model_conf(w['model'])
    inp, _ = syn.make_inputs(pp, w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=1)
    torch.manual_seed(0)        # the oracle draws the sampler's uniforms and the min-SDF steps here: the same sample every run
    with torch.no_grad():
        out = orr.Renderer(syn.make_state_dict(mc, seed=0, scene=w.get('scene')), mc, training=not w.get('eval')).forward(inp)
    ref = {k: out[k].detach().clone() for k in ('sg_rgb_values', 'sg_diffuse_albedo_values', 'network_object_mask')}
    ref['ray_hit'], ref['secondary_dir'], ref['secondary_mask'] = out.get('_ray_hit'), out.get('secondary_dir'), out.get('secondary_mask')
    ref['uniforms'], ref['steps'], ref['steps2'] = out.get('_uniforms'), out.get('_minsdf_steps'), out.get('_minsdf_steps2')
    ref['inp'], ref['pp'] = inp, pp
    return ref


def parity_of(workload, ref, device, tier, tweak=None):
    """Relative L2 / PSNR of the HIP path's rendered RGB and albedo against `ref` (oracle_reference) on identical rays, weights and
    draws, forward only.  tier: RayTracing.trace_tier for this run; tweak(model): further switches (tools/error_budget.py)."""
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    w = dict(syn.WORKLOADS[workload])
    mc = syn.model_conf(w['model'])
    R_ = w['num_rays'] if w['num_rays'] > 0 else 1
    inp, pp = ref['inp'], ref['pp']
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(syn.make_state_dict(mc, seed=0, scene=w.get('scene')), strict=True)
    m = m.to(device)
    m.freeze_geometry()
    m.train(not w.get('eval'))
    over = [x for x in (ref['steps'], ref['steps2']) if x is not None]
    if over:
        m.ray_tracer.minsdf_steps_override = over
    if ref['uniforms'] is not None:
        m.uniforms_override = ref['uniforms']
    m.ray_tracer.trace_tier = bool(tier)      # the arithmetic the timed steps run (per-run switches)
    m.ray_tracer.split_fp8 = bench_fp8()
    if tweak is not None:
        tweak(m)
    with torch.no_grad():
        out = m({k: v.to(device) for k, v in inp.items()})
    mask = ref['network_object_mask'] & out['network_object_mask'].cpu()
    parity = {'pixels': int(mask.numel()), 'hit_pixels': int(mask.sum()),
              'hit_mask_mismatches': int((ref['network_object_mask'] != out['network_object_mask'].cpu()).sum())}
    if ref.get('ray_hit') is not None and getattr(m, 'last_ray_hit', None) is not None:
        # per RAY (a multi-ray pixel counts as hit only when all its rays hit: one ray's flip moves the pixel's mean, not its mask)
        parity['ray_hit_mismatches'] = int((m.last_ray_hit.cpu().bool() != ref['ray_hit'].bool()).sum())
    for k, name in (('sg_rgb_values', 'rgb'), ('sg_diffuse_albedo_values', 'albedo')):
        a, b = out[k].cpu()[mask], ref[k][mask]
        mse = ((a - b) ** 2).mean().item()
        parity[name + '_rel_l2'] = ((a - b).norm() / (b.norm() + 1e-12)).item()
        parity[name + '_psnr_db'] = float('inf') if mse == 0 else 20.0 * math.log10(1.0 / mse ** 0.5)
    # Monte-Carlo workloads: a primary ray whose sampled direction differs (the SG-mixture sampler picks its lobe by a CDF
    # comparison: a uniform within rounding of a boundary picks the neighbour) or one of whose secondary rays hits on one
    # side only is ANOTHER sample of the integrand, not an error of it: counted, and the colour also given without the
    # pixels that hold such a ray (what the GPU suite asserts the north-star bound on: tests/parity.py)
    if ref.get('secondary_dir') is not None and out.get('secondary_dir') is not None and ref.get('ray_hit') is not None:
        hit, rhit = m.last_ray_hit.cpu().bool(), ref['ray_hit'].bool()

        def spread(x, h):
            full = torch.zeros(3, h.shape[0], x.shape[-1])
            full[:, h] = x.detach().cpu().float()
            return full
        both = hit & rhit
        dflag = ((spread(out['secondary_dir'], hit) - spread(ref['secondary_dir'], rhit)).abs().amax(-1) > 1e-3).any(0) & both
        mflag = (spread(out['secondary_mask'].float(), hit)[..., 0] != spread(ref['secondary_mask'].float(), rhit)[..., 0]).any(0) & both & ~dflag
        flagged_px = (dflag | mflag).reshape(-1, R_).any(1)
        parity['rays_with_another_sampled_direction'] = int(dflag.sum())
        parity['rays_with_another_secondary_hit_flag'] = int(mflag.sum())
        parity['pixels_holding_such_a_ray'] = int((flagged_px & mask).sum())
        keep = mask & ~flagged_px
        if keep.any():
            a, b = out['sg_rgb_values'].cpu()[keep], ref['sg_rgb_values'][keep]
            parity['rgb_rel_l2_same_samples'] = ((a - b).norm() / (b.norm() + 1e-12)).item()
    parity['tolerance_rel_l2'] = 1e-3
    parity['sample'] = 'the first %d pixels of the workload (%d primary rays), forward only, the oracle\'s draws replayed' % (
        pp, pp * R_)
    parity['trace_tier'] = bool(m.ray_tracer.trace_tier)
    parity['split_fp8'] = bool(m.ray_tracer.split_fp8)
    return parity


def bench_tier():
    """The tiered sphere tracing (RayTracing.trace_tier) is a per-run switch, off by default in the library; the
    benchmark runs every workload WITH it unless NEFII_TRACE_TIER=0."""
    return os.environ.get('NEFII_TRACE_TIER', '1') != '0'


def bench_fp8():
    """The split evaluator's correction products on block-scaled fp8 (RayTracing.split_fp8): like the tier a per-run switch,
    off by default in the library - and in the benchmark (NEFII_SPLIT_FP8=1 turns it on): on config 2 it takes the parity figure to
    5.1e-4 / 5.4e-4, past the 5e-4 line of the error budget.  The headline's line carries its figure as ms_per_step_split_fp8."""
    return os.environ.get('NEFII_SPLIT_FP8', '0') == '1'


def run_workload(name, args, steps, warmup, rank, world, dev, backend, lib, side=True, scaling=None, sustained=None,
                 power=False, tier=None, fp8=None, full=True, dump=None):
    """Time `steps` training steps of WORKLOADS[name] (every rank), then - full=True - measure the roofline terms in un-timed
    extra steps.  dump: a directory for what the last timed step returned (dump_outputs).  Returns the result dict on rank 0,
    None elsewhere."""
    import ctypes
    import torch.distributed as dist
    from nefii_amd import conf, ops, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.training.step import TrainStep

    w = dict(syn.WORKLOADS[name])
    # NEFII_BENCH_PIXELS (tests only: the 8-rank launch on a one-GPU box): every training workload at this many pixels instead
    # of its own - the line says so (config.num_pixels_override) and is no measurement of the BASELINE config
    px_override = int(os.environ.get('NEFII_BENCH_PIXELS', '0'))
    if px_override > 0:
        w['num_pixels'] = px_override
    mc = syn.model_conf(w['model'])
    sd = syn.make_state_dict(mc, seed=0, scene=w.get('scene'))
    lc = syn.loss_conf(w['model'])
    torch.manual_seed(1234 + rank)
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)
    model.freeze_geometry()
    model.train()
    model.ray_tracer.trace_tier = bench_tier() if tier is None else bool(tier)
    model.ray_tracer.split_fp8 = bench_fp8() if fp8 is None else bool(fp8)
    # weak scaling (default): global batch = num_pixels * world; --scaling strong: the config's own global batch (config 4:
    # 8192 pixels) - either way the contiguous per-rank slice of the global patch list (scene_dataset.py:268-279)
    strong = (scaling or getattr(args, 'scaling', 'weak')) == 'strong'
    # --cycle-batches C: the steps cycle over C distinct pixel batches (seeds 1 .. C), as tools/long_train.py and the runner
    # do: another hit count every step, so the per-padded-hit-count graphs and the trace lookahead meet what training gives them
    n_cycle = max(1, int(getattr(args, 'cycle_batches', 1)))
    batches = []
    for b in range(n_cycle):
        bi, bg = syn.make_inputs(w['num_pixels'] * (1 if strong else world), w['image_hw'], w['focal'], w['cam_pos'],
                                 w['num_rays'], seed=1 + b, rank=rank, world_size=world)
        batches.append(({k: v.to(dev) for k, v in bi.items()}, {'rgb': bg.to(dev)}))
    inp, gt = batches[0]
    rays_per_rank = inp['uv'].shape[1] * (w['num_rays'] if w['num_rays'] > 0 else 1)
    rays_all_ranks = rays_per_rank * world
    if strong and world > 1:        # the last rank takes the remainder of the patch list
        t = torch.tensor([float(rays_per_rank)], device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
        dist.all_reduce(t)
        rays_all_ranks = int(t.item())
    indirect = mc.get('render_type', 'sg') != 'sg'
    # conf.conf runs: secondary-consistency step every 10 iterations on 1024/world points (robot/run_s2.sh:25-26)
    # closed-form shading: the step's tail replays as a hipGraph after 3 eager iterations (NEFII_BENCH_GRAPH=0: eager)
    use_graph = os.environ.get('NEFII_BENCH_GRAPH', '1') != '0' and not indirect
    step = TrainStep(model, lc, world_size=world, secondary_train_interval=10 if indirect else 0,
                     secondary_batch_size=1024, num_rays=w['num_rays'], graph=use_graph)

    # NEFII_BENCH_PREFETCH=1 (default): every step also enqueues the trace of the next batch (TrainStep.prefetch_trace)
    prefetch = os.environ.get('NEFII_BENCH_PREFETCH', '1') != '0'
    look = max(1, int(os.environ.get('NEFII_BENCH_LOOKAHEAD', str(step.preferred_lookahead(inp))))) if prefetch else 0
    it_no = [0]

    def run_step():
        """the next step of the cycle, with the batches known ahead of it (a dataloader's prefetch queue) as next_input"""
        i = it_no[0]
        it_no[0] = i + 1
        bi, bg = batches[i % n_cycle]
        ahead = [batches[(i + 1 + j) % n_cycle][0] for j in range(look)] if look else None
        return step(bi, bg, ahead)

    nxt = [inp] * look if look else None        # (the un-timed roofline passes below run ONE batch)
    for _ in range(warmup):
        run_step()
    # the graph of the step's tail is captured once per padded hit count, after 3 eager steps: with fewer warm-up steps
    # than that, run the missing ones (still untimed) so that no capture lands in the timed region
    priming = max(0, step.graph_after + 1 - warmup) if use_graph else 0     # the same count on every rank
    for _ in range(priming):
        run_step()
    # the timed region - exactly `steps` steps between barrier + synchronize on both sides, max over ranks - is measured
    # `repeats` times back to back (63 ms of a 20-step config-2 region is a thin basis for a headline: boxes and moments
    # differ by a few percent); the line reports the MEDIAN repetition and lists them all
    reps = []
    import contextlib
    with contextlib.ExitStack() as stack:       # (the headline at N = 1 also reads the board's power sensor meanwhile)
        meter = stack.enter_context(BoardPower()) if power and rank == 0 and world == 1 else None
        for _ in range(max(1, args.repeats)):
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out, lo = run_step()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            elapsed = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([elapsed], device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                elapsed = t.item()
            reps.append(elapsed)
    elapsed = sorted(reps)[len(reps) // 2]
    ms_per_step = elapsed / steps * 1e3
    value = rays_all_ranks / (elapsed / steps)
    nonfinite_timed = int(step.nonfinite_steps.item())      # steps the NaN guard cancelled so far (warm-up + timed)

    def record(lo, ms_skip, param_spread, roofline):
        """the result dict; a plain run (full=False) has no side measurement, rank spread or roofline"""
        return {
            'metric': 'training rays/sec (Step-2 material opt)', 'value': value, 'unit': 'rays/s',
            'n_gpus': world, 'steps': steps, 'warmup': warmup, 'graph_priming_steps': priming,
            'ms_per_step': ms_per_step,
            'ms_per_step_repeats': [e / steps * 1e3 for e in reps],
            'ms_per_step_without_dead_min_sdf_search': ms_skip,
            # the runner's OPT-IN schedule under frozen geometry (min_sdf_every = 50: the search runs on the iterations whose loss
            # line is printed, idr_train.py:784; the losses of the other iterations are then not the reference's): 49 steps
            # without the search and one with it, both measured here
            'ms_per_step_min_sdf_on_reporting_iterations': None if ms_skip is None else (49.0 * ms_skip + ms_per_step) / 50.0,
            'higher_is_better': True, 'scaling': 'strong' if strong else 'weak', 'vs_baseline': None,
            # arithmetic of the dominant kernels: f16x3 = split precision on three fp16 MFMAs per product; f16+fp8x2 = its two correction
            # products on block-scaled fp8 MFMAs (RayTracing.split_fp8 on a 512-wide net); the single-pass evaluator is f16 in both
            'dtype': ('f16+fp8x2' if (model.ray_tracer.split_fp8 and model.implicit_network.specs[0].n_out == 512) else 'f16x3')
            if model.ray_tracer.precision.startswith('f16x3') else 'f32',
            'data': 'synthetic',
            'config': {'workload': '%s: %s, %s model, num_pixels=%d per GPU%s, 128 SG lobes, %s, frozen geometry, '
                                   'fwd+IDRLoss+bwd+2xAdam'
                                   % (name + (' (strong scaling: global batch split over the ranks)' if strong else ''),
                                      'robot-like synthetic scene (geometric-init SDF sphere)' if not w.get('scene') else
                                      {'bowl': 'non-convex synthetic scene (fitted ball-in-bowl SDF embedded at full width, zero-padded)',
                                       'bowl_dense': 'non-convex synthetic scene (fitted ball-in-bowl SDF embedded at full width, no zero weights)',
                                       'bowl_trained': 'non-convex synthetic scene (ball-in-bowl, the full-width SDF network trained by the Step-1 runner)',
                                       'frame_trained': 'thin-feature synthetic scene (cube frame + plate + ball, the full-width SDF network '
                                                        'trained by the Step-1 runner)'}[w['scene']],
                                      {'physg': 'physg.conf', 'conf': 'conf.conf', 'neus': 'conf_neus.conf'}[w['model']],
                                      w['num_pixels'], (' x %d rays/pixel' % w['num_rays']) if w['num_rays'] > 0 else '',
                                      'indirect OFF (closed-form SG)' if not indirect else 'MC direct + near-field indirect ON'),
                       'primary_rays_per_step_per_gpu': rays_per_rank, 'parallelism': 'dp%d' % world,
                       'step_graph': bool(use_graph), 'cycle_batches': n_cycle,
                       'trace_tier': bool(model.ray_tracer.tier_for()),
                       # staged bracket search of eval-mode traces (the MC renderer's secondary rays; renders): opt-in since round 6,
                       # NEFII_BRACKET_STAGED_EVAL=1 - bit-identical while the measured slope bound holds, DESIGN section 4
                       'bracket_staged_eval': bool(model.ray_tracer.bracket_staged_eval),
                       'split_fp8': bool(model.ray_tracer.split_fp8),
                       'synchronous_retraces': int(model.ray_tracer.retraced_calls), 'retraced_steps': int(step.retraced_steps),
                       'num_pixels_override': px_override or None,
                       'rank_param_spread': param_spread,
                       # steps cancelled by TrainStep's NaN guard: in warm-up + timed repetitions / in the whole run.  Any
                       # cancelled step makes the line INVALID (main() flags it and exits non-zero)
                       'nonfinite_steps_timed': nonfinite_timed,
                       'nonfinite_steps': int(step.nonfinite_steps.item()),
                       'trace_prefetch': look,   # batches traced ahead, beside the tail of batch i
                       # MC workloads: does the secondary trace also fill the outputs of rays that MISS (min-SDF search,
                       # argmin fallback)?  Nothing reads them (idr_train.py:819 masks secondary_points with the hit mask);
                       # the default skips them - every consumed output bit-identical
                       # (test_secondary_trace_without_the_miss_search_changes_nothing_that_is_read);
                       # NEFII_SECONDARY_MISS_SEARCH=1 executes them as the reference does
                       'secondary_miss_search': bool(model.secondary_miss_search) if indirect else None,
                       'loss': float(lo['loss'].item())},
            'roofline': roofline,
        }

    if dump and rank == 0:      # now: the steps below reuse the graph's output buffers and update the parameters again
        dump_outputs(dump, {'out': out, 'loss': lo,
                            'param': {k: p for k, p in model.named_parameters() if p.requires_grad}})
    if not full:
        if rank != 0:
            return None
        return record(lo, None, 0.0 if world == 1 else None, None)

    # ---- un-timed side measurements (every rank runs the steps: they contain the gradient all-reduce)
    # (1) the same step without the min-SDF search that is dead work under frozen geometry
    #     (RayTracing.skip_min_sdf_search; same gradients, different mask_loss value), and its SDF-evaluation counters:
    #     E_tr / E_tr2 of SURVEY.md section 8(d) (sphere tracing + bracket search + bisection, primary + secondary rays)
    ms_skip = None
    model.ray_tracer.skip_min_sdf_search = True
    if side:
        step._prefetch = []         # traces enqueued WITH the search: dropped, the loop below starts its own queue
        for _ in range(3):
            run_step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for _ in range(max(steps // 2, 1)):
            run_step()
        torch.cuda.synchronize()
        ms_skip = (time.perf_counter() - t2) / max(steps // 2, 1) * 1e3
    torch.cuda.synchronize()
    step._prefetch.clear()                  # traces enqueued ahead by the loops above: done, not needed
    model.ray_tracer.collect_counters = True
    model.ray_tracer.counter_sum = None
    step(inp, gt)
    torch.cuda.synchronize()
    cnt_live = model.ray_tracer.counter_sum.cpu().long()
    model.ray_tracer.skip_min_sdf_search = False

    # (2) roofline of the dominant kernel: one extra step with per-launch HIP events; only rank 0 instruments it
    model.ray_tracer.counter_sum = None
    model.ray_tracer.stream_groups = 1      # the profiled step runs the rounds back to back on one stream
    model.ray_tracer.concurrent = nxt is not None   # as the timed steps' traces run (TrainStep.prefetch_trace): same rounds per step
    if rank == 0:
        lib.nefii_trace_profile_enable(1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out, lo = step(inp, gt)
    torch.cuda.synchronize()
    prof_step_ms = (time.perf_counter() - t1) * 1e3
    # data-parallel sanity: after identical initialisation and all-reduced gradients every rank must hold the same
    # parameters - the relative spread of a parameter checksum over the ranks is reported (0.0 for one process)
    param_spread = 0.0
    if world > 1:
        chk = torch.stack([p.detach().double().abs().sum() for p in model.parameters()]).sum().reshape(1)
        chk = chk.to(dev if backend == 'nccl' else 'cpu')
        hi, lo_ = chk.clone(), chk.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo_, op=dist.ReduceOp.MIN)
        param_spread = float((hi - lo_).item() / max(abs(hi.item()), 1e-30))
        dist.barrier()
    if rank != 0:
        return None

    eval_ms, n_eval, span_ms = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
    lib.nefii_trace_profile_read(ctypes.byref(eval_ms), ctypes.byref(n_eval), ctypes.byref(span_ms))
    lib.nefii_trace_profile_enable(0)
    cnt = model.ray_tracer.counter_sum.cpu().long()       # primary + secondary traces of the step
    n_steps = model.ray_tracer.n_steps
    # algorithmic evaluations (what the reference's recurrences need) vs executed (incl. the unused nodes of the
    # speculative bisection tree and the coarse pass's refined samples); the roofline credits only the algorithmic ones
    queries = int(ops.algorithmic_evals(cnt, n_steps).sum().item())
    ex_split, ex_coarse = ops.executed_evals(cnt, n_steps)
    executed, executed_coarse = int(ex_split.sum().item()), int(ex_coarse.sum().item())
    launches = int((cnt[:, [0, 1, 2, 4, 5, 9, 11]].sum(dim=1) > 0).sum().item())
    tier_queries, tier_repeats = int(cnt[:, 9].sum().item()), int(cnt[:, 10].sum().item())
    f_eval = mlp_flops(model.implicit_network.specs)
    achieved = queries * f_eval / (eval_ms.value * 1e-3) / 1e12 if eval_ms.value > 0 else 0.0
    ray_hit = model.last_ray_hit
    n_hit = int(ray_hit.sum().item())
    hit_frac = n_hit / max(ray_hit.numel(), 1)
    n_hit2 = int(out['secondary_mask'].sum().item()) if out.get('secondary_mask') is not None else 0
    sec_frac = n_hit2 / max(3 * n_hit, 1) if indirect else None
    prec = model.ray_tracer.precision
    split = prec.startswith('f16x3')
    peak = PEAK_F16_MFMA_TFLOPS if split else PEAK_F32_MFMA_TFLOPS
    pm = model.implicit_network.packed(f16x3=True) if split else None
    kname = {'f32': 'eval_kernel', 'f16x3': 'eval_kernel16', 'f16x3w': 'eval_kernel16w'}[prec]
    coarse_tau = 0.0
    if prec == 'f16x3w' and pm.w_stream is not None:
        # 512- / 256-wide nets: the pipelined stream kernels (mlp_tile.h "16q": 16x16x32 MFMA; "16p": 32x32x16)
        kname = 'eval_kernel16q' if pm.struct.reserved == 1 else 'eval_kernel16p'
        if model.ray_tracer.split_fp8 and ops.fp8corr_supported(pm):
            kname = 'eval_kernel16f'        # (mlp_tile.h "16f": correction products on block-scaled fp8)
        if model.ray_tracer.coarse:
            coarse_tau = model.implicit_network.coarse_tau(model.ray_tracer.object_bounding_sphere)
            if coarse_tau > 0:
                kname += ' + eval_kernel16s'
    # ---- algorithmic flops of the whole step per primary ray
    f_rad = mlp_flops(model.rendering_network.specs)
    f_mat = mlp_flops(model.envmap_material_network.specs)
    evals_live = int(ops.algorithmic_evals(cnt_live, n_steps).sum().item())        # E_tr (+ 3 h E_tr2), whole step
    rad_on = lc.get('idr_rgb_weight', 0.0) > 0
    a_step = evals_live * f_eval + n_hit * (2 * f_eval + (3 * f_rad if rad_on or indirect else 0) + 3 * f_mat +
                                            (F_MC_SHADING if indirect else F_SG_SHADING))
    if indirect:
        a_step += n_hit2 * (2 * f_eval + 3 * f_rad)
    a_ray = a_step / rays_per_rank
    frac_step = a_ray * (value / world) / (peak * 1e12)
    # the evaluators' algorithmic flops over the TIMED step (several traces run beside each other there, so this can
    # exceed frac_kernel, which prices one trace's evaluator launches run back to back on one stream)
    frac_chip = queries * f_eval / (ms_per_step * 1e-3) / (peak * 1e12)
    # SURVEY 8(d)-strict on the same kernel time: only the evaluations 8(d) counts (no min-SDF search)
    frac_8d = evals_live * f_eval / (eval_ms.value * 1e-3) / (peak * 1e12) if eval_ms.value > 0 else 0.0
    # (with RayTracing.split_fp8 the two correction products of a split evaluation are fp8 MFMAs: counted here at their flops, which
    # the fp16 sustained_peak does not price - issued_frac_of_sustained is then an upper bound of the fp16 share)
    issued = (executed * (3 if split else 1) + executed_coarse) * f_eval / (eval_ms.value * 1e-3) / 1e12 if eval_ms.value > 0 else 0.0
    # what the kernels EXECUTED, one F_sdf per evaluation whatever its arithmetic (frac credits the reference's count: samples
    # the windowed searches never evaluated are an algorithmic saving, not kernel efficiency)
    frac_executed = (executed + executed_coarse) * f_eval / (eval_ms.value * 1e-3) / (peak * 1e12) if eval_ms.value > 0 else 0.0
    # HBM traffic of the same kernels: NOT measured by this run - read from the rocprofv3 PMC passes of this command
    # committed under profiles/ (tools/profile_round.sh; separate FETCH_SIZE / WRITE_SIZE runs, gfx950 correction applied
    # by tools/pmc_traffic.py), and only quoted for the workload / kernels it was measured on
    traffic, traffic_source = None, None
    for rnd in ('r06', 'r05', 'r04', 'r03', 'r02', 'r01'):
        tpath = os.path.join(ROOT, 'profiles', rnd, 'pmc_traffic_%s.json' % name)
        if os.path.exists(tpath):
            tj = json.load(open(tpath))
            if tj.get('kernel') and tj['kernel'] in kname:
                traffic = tj['hbm_bytes_per_launch']
                traffic_source = ('profiles/%s/pmc_traffic_%s.json: rocprofv3 --pmc passes of this command on an earlier run '
                                  '(2*FETCH_SIZE + WRITE_SIZE per tracer round, all dispatches of the round\'s evaluation '
                                  'kernels, averaged over all rounds incl. empty ones); not measured by this run' % (rnd, name))
                break
    # algorithmic HBM bytes of one tracer round on the same basis as `traffic` (all rounds of the step, empty ones included):
    # every fragment stream a round's evaluators read, once (split: hi + lo pairs; single pass: hi only), plus ~45 B per query
    # (ray state in, value out)
    traffic_alg = None
    if pm is not None and getattr(pm, 'w_stream', None) is not None and n_eval.value > 0:
        split_bytes = sum(2 * 2 * s_.k_in * s_.n_out for s_ in model.implicit_network.specs)
        rounds_split = int((cnt[:, [0, 1, 4, 7]].sum(dim=1) > 0).sum().item())
        rounds_single = int((cnt[:, [5, 9, 11]].sum(dim=1) > 0).sum().item())
        traffic_alg = (split_bytes * rounds_split + split_bytes // 2 * rounds_single + 45.0 * (executed + executed_coarse)) \
            / n_eval.value
    achieved_executed = frac_executed * peak
    roofline = {'bound': 'mfma',
                'kernel': kname + ' (fused SDF MLP over the tracer work list)',
                # frac = what the kernels EXECUTED (one F_sdf per evaluation whatever its arithmetic) / their launch time / peak
                'achieved': achieved_executed, 'peak': peak, 'unit': 'TFLOP/s', 'frac': frac_executed,
                'frac_executed': frac_executed,
                # the evaluations the REFERENCE's recurrences execute against the same time (rounds 2-5 called this `frac`): rises
                # when a staged search skips work - an algorithm-level figure
                'achieved_credited': achieved, 'frac_credited': achieved / peak,
                'frac_kernel': achieved / peak, 'frac_step': frac_step, 'frac_chip': frac_chip, 'frac_8d': frac_8d,
                'traffic_algorithmic': traffic_alg,
                'issued_tflops': issued,
                'sustained_peak': sustained,
                'board_power': meter.summary() if meter is not None else None,
                'frac_of_sustained': (achieved / sustained['value']) if sustained else None,
                'issued_frac_of_sustained': (issued / sustained['value']) if sustained else None,
                'frac_definitions': 'frac = frac_executed; frac_credited = frac_kernel: the REFERENCE\'s evaluator flops / evaluator launch time of ONE trace run serially (HIP '
                                    'events, an extra un-timed step); frac_chip: the same flops / ms_per_step of the timed '
                                    'steps (traces overlapped); frac_step: SURVEY 8(d) A x rays/s / peak (whole step, dead '
                                    'min-SDF search excluded); frac_8d: evaluations WITHOUT the min-SDF search / the same '
                                    'evaluator launch time as frac_kernel; frac_executed: the evaluations the kernels actually '
                                    'executed (split precision + single pass, one F_sdf each) / that time; issued_tflops: MFMA flops the evaluators issue '
                                    '(3 per split-precision product, refined samples and speculative bisection nodes '
                                    'included) / that time; sustained_peak: a bare fp16 MFMA loop on random operands, '
                                    'measured in this run on this device (the part is power-limited: 2.5 PFLOP/s spec)',
                'traffic': traffic, 'traffic_source': traffic_source,
                'arithmetic': ('split precision: 3x v_mfma_f32_16x16x32_f16 per k-step on fp16 hi/lo operand pairs, fp32 '
                               'accumulate; coarse pass (bracket / min-SDF searches): 1x, decisive samples re-evaluated in '
                               'split precision.  achieved counts ALGORITHMIC flops: evaluations the reference executes x '
                               'flops_per_sdf_eval') if split else 'v_mfma_f32_32x32x2_f32 (exact fp32)',
                'flops_per_sdf_eval': f_eval, 'sdf_evals_per_step': queries,
                'sdf_evals_executed_split_precision': executed, 'sdf_evals_executed_single_pass': executed_coarse,
                'coarse_tau': coarse_tau,
                # tiered sphere tracing (nefii_tracer_params.trace_tier): sphere-tracing queries of this step that ran on the
                # single-pass evaluator, and how many of them had to be repeated in split precision
                'trace_tier': bool(model.ray_tracer.tier_for()),
                'tier_queries_single_pass': tier_queries, 'tier_queries_repeated': tier_repeats,
                # staged searches (nefii_tracer_params.minsdf_lipschitz: the min-SDF search, and the bracket search of eval-mode
                # traces and of rays outside the mask): the measured slope bound in use (0: off), the samples their second stages
                # evaluated one by one (the first stage's are a quarter row per search, counted with the single-pass
                # evaluations), dense searches entered (bracket + min-SDF; the reference evaluates n_steps samples for each), and
                # the audit: the largest amount an evaluated sample lay below the lower bound it was given (0 = the bound held)
                'minsdf_lipschitz': float(model.implicit_network.minsdf_lipschitz(model.ray_tracer.object_bounding_sphere))
                if (model.ray_tracer.minsdf_staged and coarse_tau > 0) else 0.0,
                'minsdf_second_stage_depths': int(cnt[:, 11].sum().item()), 'dense_searches_entered': int(cnt[:, 6].sum().item()),
                # the slope bound's online audit: every second-stage sample is held against the bound it was given; among them the
                # PROBES - samples the search had skipped, evaluated after all (one per search by hash + those whose bound cleared
                # the limit by < 2 tau; counter 13, ABI 15)
                'lipschitz_audited_samples': int(cnt[:, 11].sum().item()),
                'lipschitz_probe_samples': int(cnt[:, 13].sum().item()) if cnt.shape[1] > 13 else None,
                'minsdf_lipschitz_violation': float(cnt[:, 12].contiguous().int().view(torch.float32).max().item()) if cnt.numel() else 0.0,
                # the online audit of that bound (every refined sample is evaluated both ways): the largest |single pass -
                # split| the tracer saw in this run, and what ImplicitNetwork.note_coarse_audit did about it (nothing, if empty)
                'coarse_audit_max': float(model.implicit_network.coarse_audit_max),
                'coarse_audit_events': [list(e) for e in model.implicit_network.coarse_audit_events],
                'sdf_evals_per_primary_ray': queries / rays_per_rank,
                'nonempty_launches_per_step': launches, 'launches_per_step': n_eval.value,
                'kernel_ms_per_step': eval_ms.value, 'tracer_span_ms': span_ms.value,
                'profiled_step_ms': prof_step_ms, 'hit_fraction': hit_frac, 'secondary_hit_fraction': sec_frac,
                'step_model': {'formula': 'SURVEY.md 8(d): A = E*F_sdf + N_hit*(F_nrm + 3 F_rad[if weighted] + 3 F_mat + F_shade)'
                                          ' + N_hit2*(F_nrm + 3 F_rad); frac_step = A/ray * rays/s/GPU / peak',
                               'E_sdf_evals_without_min_sdf_search': evals_live, 'N_hit': n_hit, 'N_hit2': n_hit2,
                               'F_sdf': f_eval, 'F_nrm': 2 * f_eval, 'F_rad': f_rad, 'F_mat': f_mat,
                               'F_shade': F_MC_SHADING if indirect else F_SG_SHADING,
                               'radiance_backward_counted': bool(rad_on or indirect),
                               'A_flops_per_primary_ray': a_ray}}
    return record(lo, ms_skip, param_spread, roofline)


def syn_is_render(name):
    from nefii_amd import synthetic as syn
    return bool(syn.WORKLOADS[name].get('eval'))


def run_render(name, args, frames, rank, world, dev, backend, dump=None):
    """BASELINE config 5: eval-mode full-frame render, the frame's chunks dealt round-robin over the ranks and gathered on
    rank 0 (training/render.py:render_frame <-> scripts/render.py:267-360).  One "step" = one 800 x 800 frame at 256 rays per
    pixel; strong scaling by definition (the frame is the unit).  --frame-rows R renders a band of R rows through the middle of
    the frame only (a bounded run: a whole frame takes ~1.5 minutes on one GPU)."""
    import torch.distributed as dist
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.training.render import render_frame
    w = dict(syn.WORKLOADS[name])
    mc, sd = syn.workload_state_dict(name, seed=0)
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    model.freeze_geometry()
    model.ray_tracer.trace_tier = bench_tier()
    model.ray_tracer.split_fp8 = bench_fp8()
    H, W = w['image_hw']
    rows = min(H, args.frame_rows) if args.frame_rows > 0 else H
    row0 = (H - rows) // 2              # a band through the middle of the frame (through the object)
    inp = syn.frame_inputs(w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], rows=(row0, rows))
    inp = {k: v.to(dev) for k, v in inp.items()}
    n_pix = rows * W
    warm = {'uv': inp['uv'][:, :1024 * world].contiguous(), 'object_mask': inp['object_mask'][:, :1024 * world].contiguous(),
            'pose': inp['pose'], 'intrinsics': inp['intrinsics']}
    render_frame(model, warm, warm['uv'].shape[1], num_rays=w['num_rays'], memory_capacity_level=w['memory_capacity_level'],
                 rank=rank, world_size=world)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        out = render_frame(model, inp, n_pix, num_rays=w['num_rays'], memory_capacity_level=w['memory_capacity_level'],
                           rank=rank, world_size=world)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    if rank != 0:
        return None
    if dump:
        dump_outputs(dump, {'out': out})
    rays = n_pix * w['num_rays']
    level = w['memory_capacity_level'] - int(math.floor(math.log2(world)))
    return {'metric': 'render rays/sec (full-frame novel-view render, eval mode)', 'value': rays * frames / elapsed,
            'unit': 'rays/s', 'n_gpus': world, 'steps': frames, 'warmup': 0, 'ms_per_step': elapsed / frames * 1e3,
            'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None,
            'dtype': 'f16+fp8x2' if model.ray_tracer.split_fp8 else 'f16x3', 'data': 'synthetic',
            'config': {'workload': '%s: conf.conf model at full width on the non-convex stand-in, %d x %d pixels x %d rays per '
                                   'pixel, chunks of %d pixels dealt round-robin over %d rank(s) and gathered on rank 0'
                                   % (name, rows, W, w['num_rays'], (1 << level) // w['num_rays'], world),
                       'primary_rays_per_frame': rays, 'trace_tier': bool(model.ray_tracer.tier_for()),
                       'bracket_staged_eval': bool(model.ray_tracer.bracket_staged_eval), 'split_fp8': bool(model.ray_tracer.split_fp8),
                       # (a band through the object is dearer per pixel than the frame's average: no extrapolation from it)
                       'seconds_per_800x800_frame': elapsed / frames if rows == H else None,
                       'hit_pixel_fraction': out['network_object_mask'].float().mean().item(),
                       'finite': bool(all(torch.isfinite(v).all() for v in out.values() if v.dtype.is_floating_point)),
                       'parallelism': 'pixel chunks x %d' % world},
            'invalid': False}


class BoardPower:
    """Board power (the amdgpu hwmon sensor power1_input of THIS process's device, found through its PCI address) sampled
    five times a second by a background thread while the timed steps of the headline run, with the cap (power1_cap) beside it:
    the evaluators' bound is the part's power budget, and this puts the sensor's reading into the line the run
    itself prints.  Plain sysfs reads - no child process (a process that has initialised the GPU must not exec, and rocm-smi
    under a profiler's preload does).  Best effort: no sensor, no field."""

    def __init__(self, period=0.2):
        import threading
        self.period, self.samples, self.cap, self.path = period, [], None, None
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _hwmon():
        import glob
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        addr = '%04x:%02x:%02x.0' % (getattr(pr, 'pci_domain_id', 0), pr.pci_bus_id, pr.pci_device_id)
        found = glob.glob('/sys/bus/pci/devices/%s/hwmon/hwmon*/power1_input' % addr)
        return os.path.dirname(found[0]) if found else None

    @staticmethod
    def _read(path):
        with open(path) as f:
            return float(f.read()) * 1e-6      # microwatts

    def _run(self):
        while not self._stop.wait(self.period):
            try:
                self.samples.append(self._read(os.path.join(self.path, 'power1_input')))
            except Exception:
                return

    def __enter__(self):
        try:
            self.path = self._hwmon()
            if self.path:
                self.cap = self._read(os.path.join(self.path, 'power1_cap'))
                self._thread.start()
        except Exception:
            self.path = None
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self._thread.is_alive():
            self._thread.join(timeout=2)

    def summary(self):
        if not self.samples:
            return None
        return {'avg_w': sum(self.samples) / len(self.samples), 'max_w': max(self.samples), 'cap_w': self.cap,
                'samples': len(self.samples), 'source': '%s/power1_input, every %.1f s during the timed steps' % (self.path, self.period)}


def measure_sustained(lib):
    """nefii_mfma_sustained_probe: TFLOP/s of a bare v_mfma_f32_16x16x32_f16 loop on random operands on every CU, for three
    launch lengths - the part is power-limited and what it holds depends on how long the burst lasts: ~0.3 ms (a small
    tracer round), ~3 ms (a big round of config 3) and ~25 ms of uninterrupted MFMAs (`value`: the sustained figure)."""
    import ctypes
    out = {}

    def run(groups):
        ms, fl = ctypes.c_float(), ctypes.c_double()
        rc = lib.nefii_mfma_sustained_probe(groups, ctypes.byref(ms), ctypes.byref(fl), None)
        return (fl.value / (ms.value * 1e-3) / 1e12, ms.value) if rc == 0 and ms.value > 0 else (None, None)

    v, ms = run(250000)             # the long launch first: the bursts below then start from a chip that is warm and clocked up
    if v is None:
        return None
    out['value'], out['ms'] = v, ms
    for tag, groups, reps in (('burst_3ms', 37000, 3), ('burst_0.3ms', 3700, 10)):
        vals = [run(groups)[0] for _ in range(reps)]
        if any(x is None for x in vals):
            return None
        out[tag] = sorted(vals)[len(vals) // 2]
    ms8, fl8 = ctypes.c_float(), ctypes.c_double()
    if lib.nefii_mfma_sustained_probe_chains(125000, 8, ctypes.byref(ms8), ctypes.byref(fl8), None) == 0 and ms8.value > 0:
        out['value_8_chains'] = fl8.value / (ms8.value * 1e-3) / 1e12
    out['unit'] = 'TFLOP/s'
    out['what'] = ('v_mfma_f32_16x16x32_f16 only, random operands, 4 accumulator chains per wave, one wave per SIMD, 256 '
                   'workgroups; value = a 25 ms launch (behind a 6 ms warm-up launch); burst_* = the median of shorter launches right after it, '
                   'each behind a quarter-length warm-up launch.  The 4-chain loop issues 8 MFMAs in 148 cycles, not the 128 of a '
                   'free-running pipe (profiles/r04/slot_probe.txt); value_8_chains is the same 25 ms on 8 independent chains '
                   '(128 cycles per 8): on a power-limited part the denser loop mostly clocks lower - both are in the line')
    return out


DUMP_MAX_BYTES = 60_000_000     # --dump-outputs: the arrays' data in all (64 MB with room for the .npy headers)


def dump_outputs(path, groups):
    """--dump-outputs: every tensor of `groups` ({group: {key: tensor}}: what the last timed step returned - its outputs and
    losses - and the trainable parameters its optimizer step left) as <path>/<group>.<key>.npy, float64 for float64 and integer
    tensors, float32 for the rest.  Past DUMP_MAX_BYTES in all, the arrays are visited smallest first and each keeps at most an
    equal share of what is left of the budget: the small ones whole, a large one as a fixed sample of its elements (sorted flat
    indices drawn with numpy seed 0), flattened."""
    import numpy as np
    arrays = {}
    for g, d in groups.items():
        for k, v in d.items():
            if torch.is_tensor(v):
                wide = v.dtype == torch.float64 or not (v.dtype.is_floating_point or v.dtype == torch.bool)
                arrays['%s.%s' % (g, k)] = v.detach().to('cpu', torch.float64 if wide else torch.float32).numpy()
    total = sum(a.nbytes for a in arrays.values())
    left, kept = DUMP_MAX_BYTES, 0
    os.makedirs(path, exist_ok=True)
    for i, name in enumerate(sorted(arrays, key=lambda k: (arrays[k].nbytes, k))):
        a = arrays[name]
        n = min(a.size, int(left / (len(arrays) - i)) // a.itemsize)
        if n < a.size:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, n, replace=False))]
        np.save(os.path.join(path, name + '.npy'), a)
        left -= a.nbytes
        kept += a.nbytes
    print('dump-outputs: %d arrays, %.1f MB of %.1f MB kept, in %s' % (len(arrays), kept / 1e6, total / 1e6, path),
          file=sys.stderr, flush=True)


def _r(x, nd=4):
    """a float at nd significant digits (the compact line is a result line, not a log)"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        if not math.isfinite(x):
            return None if x != x else (1e308 if x > 0 else -1e308)
        return float('%.*g' % (nd, x))
    return x


def compact_line(full):
    """The LAST line of stdout: a flat JSON object of < 4 KB holding what the driver parses - the contract's keys, `roofline`
    (frac = what the kernels EXECUTED), `cpu_baseline`, `parity` - no prose, no nested configs.  Everything else is in the full
    record (--full-out).  Pure function of the full record: tests/test_bench_line_cpu.py runs it on a canned one."""
    cfg, rf = full.get('config') or {}, full.get('roofline') or {}
    wl = str(cfg.get('workload', ''))
    out = {'metric': full.get('metric'), 'value': _r(full.get('value'), 6), 'unit': full.get('unit'),
           'n_gpus': full.get('n_gpus'), 'steps': full.get('steps'), 'warmup': full.get('warmup'),
           'ms_per_step': _r(full.get('ms_per_step'), 5), 'higher_is_better': full.get('higher_is_better', True),
           'scaling': full.get('scaling'), 'vs_baseline': full.get('vs_baseline'), 'dtype': full.get('dtype'),
           'data': full.get('data', 'synthetic')}
    c = {'workload': wl.split(':')[0] if wl else None}
    for k in ('primary_rays_per_step_per_gpu', 'primary_rays_per_frame', 'parallelism', 'trace_tier', 'bracket_staged_eval', 'split_fp8', 'secondary_miss_search',
              'step_graph', 'cycle_batches', 'trace_prefetch', 'nonfinite_steps', 'num_pixels_override', 'seconds_per_800x800_frame',
              'hit_pixel_fraction'):
        if cfg.get(k) is not None:
            c[k] = _r(cfg[k])
    out['config'] = c
    if rf:
        sus = rf.get('sustained_peak') or {}
        r = {'bound': rf.get('bound'), 'kernel': str(rf.get('kernel', '')).split(' (')[0], 'unit': rf.get('unit'),
             'achieved': _r(rf.get('achieved')), 'peak': rf.get('peak'), 'frac': _r(rf.get('frac')),
             'frac_step': _r(rf.get('frac_step')), 'frac_credited': _r(rf.get('frac_credited', rf.get('frac_kernel'))),
             'issued_tflops': _r(rf.get('issued_tflops')), 'issued_frac_of_sustained': _r(rf.get('issued_frac_of_sustained')),
             'sustained_peak_tflops': _r(sus.get('value')) if isinstance(sus, dict) else None,
             'traffic': _r(rf.get('traffic')), 'traffic_algorithmic': _r(rf.get('traffic_algorithmic')),
             'traffic_measured_by': ('this run' if rf.get('traffic_live') else 'profiles/') if rf.get('traffic') is not None else None,
             'kernel_ms_per_step': _r(rf.get('kernel_ms_per_step')), 'launches_per_step': rf.get('launches_per_step'),
             'sdf_evals_executed_split_precision': rf.get('sdf_evals_executed_split_precision'),
             'sdf_evals_executed_single_pass': rf.get('sdf_evals_executed_single_pass'),
             'sdf_evals_reference': rf.get('sdf_evals_per_step'), 'flops_per_sdf_eval': rf.get('flops_per_sdf_eval'),
             'coarse_tau': _r(rf.get('coarse_tau')), 'coarse_audit_max': _r(rf.get('coarse_audit_max')),
             'minsdf_lipschitz': _r(rf.get('minsdf_lipschitz')),
             'minsdf_lipschitz_violation': _r(rf.get('minsdf_lipschitz_violation')),
             'lipschitz_audited_samples': rf.get('lipschitz_audited_samples'),
             'lipschitz_probe_samples': rf.get('lipschitz_probe_samples'),
             'audit_events': len(rf.get('coarse_audit_events') or []),
             'hit_fraction': _r(rf.get('hit_fraction')), 'secondary_hit_fraction': _r(rf.get('secondary_hit_fraction'))}
        bp = rf.get('board_power')
        if isinstance(bp, dict):
            r['board_power_w'], r['board_power_cap_w'] = _r(bp.get('avg_w')), _r(bp.get('cap_w'))
        out['roofline'] = r
    cb = full.get('cpu_baseline')
    if cb:
        out['cpu_baseline'] = {'value': _r(cb.get('value')), 'unit': cb.get('unit'), 'cores': cb.get('cores'), 'kind': cb.get('kind'),
                               'value_1_thread': _r(cb.get('value_1_thread')), 'host_cpu': cb.get('host_cpu'),
                               'host_cores': cb.get('host_cores'), 'sample': str(cb.get('sample', ''))[:96]}
    pa = full.get('parity_vs_cpu_oracle')
    if pa:
        out['parity'] = {'rgb_rel_l2': _r(pa.get('rgb_rel_l2')), 'albedo_rel_l2': _r(pa.get('albedo_rel_l2')),
                         'rgb_rel_l2_same_samples': _r(pa.get('rgb_rel_l2_same_samples')), 'tolerance_rel_l2': pa.get('tolerance_rel_l2'),
                         'hit_pixels': pa.get('hit_pixels'), 'pixels': pa.get('pixels'), 'flips': pa.get('hit_mask_mismatches'),
                         'rays_with_another_sampled_direction': pa.get('rays_with_another_sampled_direction'),
                         'trace_tier': pa.get('trace_tier')}
    out['ms_per_step_without_dead_min_sdf_search'] = _r(full.get('ms_per_step_without_dead_min_sdf_search'), 5)
    if full.get('untiered'):
        out['ms_per_step_library_defaults'] = _r(full['untiered'].get('ms_per_step'), 5)
    if full.get('split_fp8'):
        out['ms_per_step_split_fp8'] = _r(full['split_fp8'].get('ms_per_step'), 5)
    if full.get('staged_eval_bracket'):
        out['ms_per_step_staged_eval_bracket'] = _r(full['staged_eval_bracket'].get('ms_per_step'), 5)
    others = {}
    for k in ('cfg1', 'cfg2', 'cfg4'):
        if isinstance(full.get(k), dict) and full[k].get('ms_per_step') is not None:
            others[k + '_ms_per_step'] = _r(full[k]['ms_per_step'], 4)
            others[k + '_frac'] = _r((full[k].get('roofline') or {}).get('frac'), 3)
    if isinstance(full.get('cfg5'), dict):
        others['cfg5_band_s'] = _r(full['cfg5'].get('ms_per_step', 0.0) / 1e3, 4)
    if isinstance(full.get('cfg3_replicated_stand_in'), dict):
        others['cfg3_replicated_stand_in_ms_per_step'] = _r(full['cfg3_replicated_stand_in'].get('ms_per_step'), 4)
    if others:
        out['others'] = others
    out['invalid'] = bool(full.get('invalid', False))
    if full.get('invalid_reason'):
        out['invalid_reason'] = str(full['invalid_reason'])[:120]
    out['full_record'] = full.get('full_record')
    line = json.dumps(out, separators=(',', ':'))
    if len(line) >= 4096:       # never again a line the driver cannot hold: shed the optional blocks, keep the contract
        for k in ('others', 'parity', 'full_record'):
            out.pop(k, None)
            line = json.dumps(out, separators=(',', ':'))
            if len(line) < 4096:
                break
    return line


def write_full(full, path):
    """The full record as indented JSON at `path` (best effort: a read-only tree only loses the side file), also copied under
    gpurun_out/ when that scratch directory exists (it is what travels back from a GPU box)."""
    full['full_record'] = os.path.basename(path) if path else None
    for pth in ([path] if path else []) + ([os.path.join(ROOT, 'gpurun_out', os.path.basename(path))]
                                             if path and os.path.isdir(os.path.join(ROOT, 'gpurun_out')) else []):
        try:
            with open(pth, 'w') as f:
                json.dump(full, f, indent=1)
        except OSError:
            full['full_record'] = None


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as CHILD processes (torch.distributed.run on
    127.0.0.1), before this process has touched a GPU, forward their output and exit with their code."""
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    sys.exit(subprocess.run(cmd, env=env).returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=None, help='timed steps (default 20; cfg5: frames, default 1)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workload', default=None, help='measure this workload alone (default: cfg3; with --full the others nested)')
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline: roofline terms (sustained MFMA peak, counters, profiled step, board '
                         'power), the side loop, the nested configs, the CPU baseline and parity, and the full record at --full-out.  '
                         'Without it the run sets up, warms up, times --steps steps once and prints the line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step returned (outputs, losses, trainable parameters after its update) as '
                         'DIR/<name>.npy, float32 / float64, at most 64 MB in all (a fixed seeded sample beyond that)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-nested', action='store_true', help='skip the nested measurements of the other configs')
    ap.add_argument('--no-side-measurement', action='store_true',
                    help='skip the untimed side loop without the min-SDF search (profiling runs: nearly every step of the\n'
                         'process is then the headline step, so rocprofv3 per-kernel averages compare directly)')
    ap.add_argument('--cpu-sample-rays', type=int, default=2048,
                    help='primary rays of the CPU baseline\'s sample (MC workloads: ~4 s per 16-thread step at 2048)')
    ap.add_argument('--repeats', type=int, default=None,
                    help='repetitions of the timed K-step region, median reported (default: 3 with --full, else 1)')
    ap.add_argument('--scaling', choices=['weak', 'strong'], default='weak',
                    help='N > 1: weak = every rank its own num_pixels (default); strong = the workload\'s global batch split '
                         'over the ranks as the dataset does (config 4: 8192 pixels); cfg5 (one frame) is always strong')
    ap.add_argument('--cycle-batches', type=int, default=4,
                    help='distinct pixel batches the steps cycle over (hit counts then differ from step to step, as in training)')
    ap.add_argument('--full-out', default=os.path.join(ROOT, 'bench_full.json'),
                    help='where the FULL record goes (every definition and nested measurement); stdout ends with the compact line')
    ap.add_argument('--frame-rows', type=int, default=0, help='cfg5: render only a band of R rows of the frame (0: all 800)')
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 3 if args.full else 1

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if args.gpus > 1 and world == 1 and 'RANK' not in os.environ:
        spawn_ranks(args.gpus)          # does not return
    import torch.distributed as dist
    # one process per GPU; NEFII_BENCH_BACKEND=gloo lets the multi-process path be smoke-tested on a 1-GPU box
    backend = os.environ.get('NEFII_BENCH_BACKEND', 'nccl')
    dev_index = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    if world > 1:
        if backend == 'nccl':
            dist.init_process_group(backend='nccl', device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    from nefii_amd import _lib
    lib = _lib.lib()
    headline = args.workload or 'cfg3'
    if syn_is_render(headline):
        result = run_render(headline, args, max(1, 1 if args.steps is None else args.steps), rank, world, dev, backend,
                            dump=args.dump_outputs)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            if args.full:
                write_full(result, args.full_out)
            print(compact_line(result), flush=True)
        return
    if args.steps is None:
        args.steps = 20
    sustained = measure_sustained(lib) if args.full else None      # every rank (its own device); rank 0's goes into the line
    result = run_workload(headline, args, args.steps, args.warmup, rank, world, dev, backend, lib,
                          side=not args.no_side_measurement, sustained=sustained, power=args.full, full=args.full,
                          dump=args.dump_outputs)
    nested = {}
    if args.full and args.workload is None and not args.no_nested:
        short = dict(steps=max(1, min(args.steps, 20)), warmup=min(args.warmup, 3))
        # (config 2's traces are enqueued in groups of four, four groups ahead: some twenty steps until the schedule has settled)
        nested['cfg2'] = run_workload('cfg2', args, max(short['steps'], 24), max(short['warmup'], 24), rank, world, dev, backend, lib,
                                      side=True, sustained=sustained)
        nested['cfg2_near'] = run_workload('cfg2_near', args, max(short['steps'], 24), max(short['warmup'], 24), rank, world, dev,
                                           backend, lib, side=False, sustained=sustained)
        # (config 1's traces are enqueued in groups of eight, four groups ahead: some forty steps until the schedule has settled;
        # a step is under a millisecond)
        nested['cfg1'] = run_workload('cfg1', args, max(short['steps'], 96), max(short['warmup'], 48), rank, world, dev, backend,
                                      lib, side=False, sustained=sustained)
        # BASELINE's 8-GPU training config as it is defined: the global 8192-pixel batch split over the ranks
        nested['cfg4'] = run_workload('cfg4', args, max(1, min(args.steps, 10)), min(args.warmup, 2), rank, world, dev, backend,
                                      lib, side=False, scaling='strong' if world > 1 else 'weak', sustained=sustained)
        if world == 1 and headline == 'cfg3' and (bench_tier() or bench_fp8()):
            # the same workload on the LIBRARY's default arithmetic (no tier, fp16 split evaluator: every value the split evaluator's)
            nested['cfg3_untiered'] = run_workload('cfg3', args, max(1, min(args.steps, 10)), min(args.warmup, 3), rank, world,
                                                   dev, backend, lib, side=False, sustained=sustained, tier=False, fp8=False)
        if world == 1 and headline == 'cfg3' and not bench_fp8():
            # ... with the split evaluator's correction products on block-scaled fp8 (RayTracing.split_fp8, opt-in: DESIGN 4g)
            nested['cfg3_split_fp8'] = run_workload('cfg3', args, max(1, min(args.steps, 10)), min(args.warmup, 3), rank, world,
                                                    dev, backend, lib, side=False, sustained=sustained, fp8=True)
        if world == 1 and headline == 'cfg3' and os.environ.get('NEFII_BRACKET_STAGED_EVAL', '0') != '1':
            # ... and with the opt-in staging of the secondary traces' bracket search (NEFII_BRACKET_STAGED_EVAL=1)
            os.environ['NEFII_BRACKET_STAGED_EVAL'] = '1'
            try:
                nested['cfg3_staged_eval'] = run_workload('cfg3', args, max(1, min(args.steps, 10)), min(args.warmup, 3), rank, world,
                                                          dev, backend, lib, side=False, sustained=sustained)
            finally:
                os.environ.pop('NEFII_BRACKET_STAGED_EVAL', None)
        if world == 1 and headline == 'cfg3':
            # the same step on the earlier stand-ins of the same scene: the ZERO-PADDED embedding of an 8 x 64 fit (rounds 2-4:
            # 98 % zero weights - what a power-limited part makes of cheap operands) and its REPLICATED embedding (round 4's
            # headline) - comparable with earlier rounds' lines, not headlines
            from nefii_amd import synthetic as syn
            scene = syn.WORKLOADS['cfg3']['scene']
            # ... and on the conf's own 8 x 512 network TRAINED by the Step-1 runner (tools/train_scene_sdf.py) on the same
            # analytic scene ('bowl_trained': full-rank weights instead of a replicated 8 x 64 fit) and on a thin-feature
            # scene ('frame_trained': the bars of a cube frame, a thin plate, a small ball)
            for key, alt in (('cfg3_zero_padded', 'bowl'), ('cfg3_replicated', 'bowl_dense'), ('cfg3_trained', 'bowl_trained'),
                             ('cfg3_frame_trained', 'frame_trained')):
                if alt == scene:
                    continue
                syn.WORKLOADS['cfg3']['scene'] = alt
                try:
                    nested[key] = run_workload('cfg3', args, max(1, min(args.steps, 10)), min(args.warmup, 3), rank, world,
                                               dev, backend, lib, side=False, sustained=sustained, power=True)
                finally:
                    syn.WORKLOADS['cfg3']['scene'] = scene
        # ... and its render config, bounded: a band of 32 rows through the object (25 600 pixels x 256 rays)
        band = argparse.Namespace(**vars(args))
        band.frame_rows = args.frame_rows or 32
        nested['cfg5'] = run_render('cfg5', band, 1, rank, world, dev, backend)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()        # nothing below communicates (rank 0 alone runs the CPU baseline)
    if rank == 0:
        keep = ('value', 'unit', 'steps', 'warmup', 'ms_per_step', 'ms_per_step_repeats', 'scaling', 'dtype', 'config', 'roofline',
                'ms_per_step_without_dead_min_sdf_search', 'ms_per_step_min_sdf_on_reporting_iterations')
        for k in ('cfg2', 'cfg1', 'cfg4'):
            if nested.get(k) is not None:
                result[k] = {f: nested[k][f] for f in keep if f in nested[k]}
        if nested.get('cfg5') is not None:
            result['cfg5'] = nested['cfg5']
        zp = nested.get('cfg3_zero_padded')
        if zp is not None:
            result['cfg3_zero_padded_stand_in'] = {
                'ms_per_step': zp['ms_per_step'], 'ms_per_step_repeats': zp['ms_per_step_repeats'], 'value': zp['value'],
                'frac': zp['roofline']['frac'], 'board_power': zp['roofline']['board_power'], 'workload': zp['config']['workload'],
                'nonfinite_steps': zp['config']['nonfinite_steps'],
                'note': 'same geometry, same kernels; the SDF net holds 98 % zero weights, the matrix cores draw less power and the '
                        'part clocks higher - the stand-in of rounds 2-4, kept for comparison with their lines'}
        for key, out_key, note in (
                ('cfg3_replicated', 'cfg3_replicated_stand_in',
                 'round 4\'s headline geometry: the 8 x 64 fit of the same scene replicated across the 512 columns without a zero '
                 'weight (rank-64 structure: twice the trained net\'s single-pass error, so a larger coarse_tau and more refined samples)'),
                ('cfg3_trained', 'cfg3_trained_stand_in',
                 'the same analytic scene regressed by the conf\'s own 8 x 512 SDF network with this repo\'s Step-1 runner '
                 '(20 000 iterations, near-surface error 6e-5): full-rank trained weights'),
                ('cfg3_frame_trained', 'cfg3_thin_feature_scene',
                 'a thin-feature scene (cube frame of 0.05-thick bars, a 0.024-thick plate, a small ball) regressed the same way: '
                 'another hit fraction and ray statistics, so ms_per_step is not comparable with the bowl\'s - tau, audit and '
                 'power are')):
            t = nested.get(key)
            if t is not None:
                r = t['roofline']
                result[out_key] = {
                    'ms_per_step': t['ms_per_step'], 'ms_per_step_repeats': t['ms_per_step_repeats'], 'value': t['value'],
                    'frac': r['frac'], 'frac_executed': r['frac_executed'], 'board_power': r['board_power'],
                    'coarse_tau': r['coarse_tau'], 'coarse_audit_max': r['coarse_audit_max'],
                    'coarse_audit_events': r['coarse_audit_events'], 'hit_fraction': r['hit_fraction'],
                    'secondary_hit_fraction': r['secondary_hit_fraction'], 'sdf_evals_per_primary_ray': r['sdf_evals_per_primary_ray'],
                    'kernel_ms_per_step': r['kernel_ms_per_step'], 'nonfinite_steps': t['config']['nonfinite_steps'],
                    'workload': t['config']['workload'], 'note': note}
        near = nested.get('cfg2_near')
        if near is not None:
            # SURVEY.md section 8(d) planned a ~40 % hit fraction for config 2; the geometric-init surface seen from 2.4 gives
            # 18 % (most rays end in the min-SDF search).  The same step with the camera at 1.6 (42 %), for comparison only
            result['cfg2_camera_at_1.6'] = {k: near[k] for k in ('value', 'unit', 'steps', 'warmup', 'ms_per_step',
                                                                 'ms_per_step_repeats')}
            result['cfg2_camera_at_1.6'].update({'workload': near['config']['workload'], 'camera': [0.0, 0.0, 1.6],
                                                 'hit_fraction': near['roofline']['hit_fraction'],
                                                 'nonfinite_steps': near['config']['nonfinite_steps']})
        if args.full and not args.no_cpu_baseline and world == 1:      # the contract: on rank 0 at N = 1 only
            result['cpu_baseline'], result['parity_vs_cpu_oracle'] = cpu_baseline(headline, args.cpu_sample_rays, device=dev)
            if 'cfg2' in result:
                result['cfg2']['cpu_baseline'], result['cfg2']['parity_vs_cpu_oracle'] = cpu_baseline(
                    'cfg2', 512, steps=3, warmup=1, device=dev)
        # a step the NaN guard cancelled costs the same time as a good one but did not train: a throughput of such steps
        # is not a measurement of the metric (round 2's nested config 3 had one in seven)
        cancelled = result['config']['nonfinite_steps'] + sum(
            x['config']['nonfinite_steps'] for k, x in nested.items() if x and k != 'cfg5')
        result['invalid'] = cancelled > 0
        f8 = nested.get('cfg3_split_fp8')
        if f8 is not None:
            result['split_fp8'] = {'ms_per_step': f8['ms_per_step'], 'ms_per_step_repeats': f8['ms_per_step_repeats'],
                                   'value': f8['value'], 'frac': f8['roofline']['frac'],
                                   'kernel_ms_per_step': f8['roofline']['kernel_ms_per_step'],
                                   'nonfinite_steps': f8['config']['nonfinite_steps'],
                                   'note': 'the same workload with RayTracing.split_fp8 on (opt-in: the split evaluator\'s two correction '
                                           'products on v_mfma_scale_f32_16x16x128_f8f6f4; a third arithmetic, |sdf error| ~1e-5)'}
        se = nested.get('cfg3_staged_eval')
        if se is not None:
            result['staged_eval_bracket'] = {'ms_per_step': se['ms_per_step'], 'ms_per_step_repeats': se['ms_per_step_repeats'],
                                             'value': se['value'], 'frac': se['roofline']['frac'],
                                             'minsdf_lipschitz_violation': se['roofline']['minsdf_lipschitz_violation'],
                                             'nonfinite_steps': se['config']['nonfinite_steps'],
                                             'note': 'the same workload with RayTracing.bracket_staged_eval on (opt-in: the secondary '
                                                     'traces\' bracket search staged behind the measured slope bound)'}
        unt = nested.get('cfg3_untiered')
        if unt is not None:
            result['untiered'] = {'ms_per_step': unt['ms_per_step'], 'ms_per_step_repeats': unt['ms_per_step_repeats'],
                                  'value': unt['value'], 'frac': unt['roofline']['frac'],
                                  'kernel_ms_per_step': unt['roofline']['kernel_ms_per_step'],
                                  'nonfinite_steps': unt['config']['nonfinite_steps'],
                                  'note': 'the same workload on the LIBRARY defaults: RayTracing.trace_tier off and split_fp8 off - every '
                                          'sphere-tracing value is the fp16 split evaluator\'s'}
        if cancelled:
            result['invalid_reason'] = '%d training step(s) produced a non-finite loss or gradient and were cancelled' % cancelled
        if args.full:
            write_full(result, args.full_out)
        print(compact_line(result), flush=True)
        if cancelled:
            sys.exit(3)


if __name__ == '__main__':
    main()
