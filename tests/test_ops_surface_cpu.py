"""The surface of nefii_amd.ops, pinned without a GPU: every module-level name callers, tests and tools reach for resolves
on `ops`; every refused call raises the exception type it always raised (CPU tensors or plain values: nothing launches; the
well-formed CPU calls show that an op looks at the device where it always did, first or last); and the launch helper reports
a failed status under the symbol it called.  Needs the library built, as test_lib_abi.py does."""
import ctypes

import pytest
import torch

from nefii_amd import _lib, build, ops

# vars(ops) of the single-file ops.py this package replaced, minus the imported modules, the dunder names and
# _denoise_buffer (a private argument checker nothing outside the file used; check_tensor took its place)
NAMES = """
ACT_ELU ACT_RELU ACT_SOFTPLUS100 AssembleRowsFn COARSE_TAU_SAFETY DENOISE_MAX_SIDE ENVFIT_MAX_LOBES
ENVLIGHT_COORDS EnvRadianceFn FusedMLPFn FusedMLPHiddenFn HEAD_ABS HEAD_NONE HEAD_POW2 HEAD_RELU
HEAD_RELU_INIT HEAD_SIGMOID HEAD_TANH01 HalfStash IdrLossFn LIPSCHITZ_SAFETY LayerSpec MAX_LOBES
MCUBES_MAX_POINTS METRICS_LEVELS METRICS_MAX_BATCH METRICS_MAX_SIDE METRICS_WINDOW MaterialHeadGlobalFn
McShadeFn Mlp PRECISIONS PackedMLP PatchLossFn SGRenderFn TraceRounds TracerParams _SIDE_STREAMS
_SSIM_LOSS_TAPS _TRACE_STREAMS _WORK _audit_of _chunks_with_work _dirs3 _envfit_args
_envlight_bounce _envlight_call _envlight_coord _envlight_map _envlight_mis _envlight_pdf _envlight_radiance
_envlight_rot _envlight_rot_index _envlight_table _f32 _image_to_linear_columns _lib _lip_audit_of
_metrics_window _metrics_workspaces _next_guess _pad_hidden _ptr _raw_stream _rot_given _round32
_stash_tensors _stream _trace_streams algorithmic_evals assemble_rows calibrate_coarse_tau calibrate_lipschitz
camera_rays check_light coarse_supported denoise_atrous encode_inputs envfit_adam envfit_loss_grad
envfit_workspace envlight_bounce_sample envlight_bounce_sample_rot envlight_mis_sample envlight_mis_sample_rot
envlight_pdf envlight_pdf_rot envlight_radiance envlight_radiance_rot envlight_rotations envlight_table
executed_evals fp8corr_supported h16_supported image_metrics make_tracer_params marching_cubes material_specs
mesh_cc_round_cap mesh_cluster_quadrics mesh_components mesh_sdf_query metrics_window mis_sample mlp_backward
mlp_backward_scale mlp_forward mlp_grad_scale mlp_precision param_list patch_loss_params prepare_hits
radiance_specs sdf_eval sdf_specs sdf_value_grad side_stream ssim_loss_window sum_counters trace_iterations
trace_rays
""".split()


def test_every_name_of_the_single_file_module_resolves():
    missing = [n for n in NAMES if not hasattr(ops, n)]
    assert not missing, missing
    assert ops._lib is _lib and ops.Mlp is _lib.Mlp and ops.TracerParams is _lib.TracerParams
    assert ops.ACT_ELU == _lib.ACT_ELU and ops.HEAD_POW2 == _lib.HEAD_POW2


def test_process_wide_state_exists_once():
    """the name on `ops` is the object the code that uses it holds: filling one fills the other"""
    import sys
    for name, user in (('_TRACE_STREAMS', '_trace_streams'), ('_SIDE_STREAMS', 'side_stream'),
                       ('_metrics_workspaces', 'image_metrics'), ('_metrics_window', 'metrics_window')):
        home = sys.modules[getattr(ops, user).__module__]
        assert getattr(home, name) is getattr(ops, name), name
    assert ops.metrics_window() is ops.metrics_window() is ops._metrics_window[0]


def f32(*shape):
    return torch.zeros(*shape)


def denoise(g0=None, g1=None, src=None, dst=None, height=4, width=4, step=1, sigmas=(1., 1., 1.)):
    n = height * width
    g0 = f32(n, 4) if g0 is None else g0
    g1 = f32(n, 4) if g1 is None else g1
    src = f32(1, n, 4) if src is None else src
    return lambda: ops.denoise_atrous(g0, g1, src, f32(*src.shape) if dst is None else dst, height, width, step, *sigmas)


def metrics(x=None, y=None, levels=1, data_range=1.0):
    x = f32(1, 16, 16, 3) if x is None else x
    return lambda: ops.image_metrics(x, x.clone() if y is None else y, levels, data_range)


def sdf_query(node_box=None, points=None, n_leaves=2):
    node_box = torch.zeros(3, 6, dtype=torch.float64) if node_box is None else node_box
    points = torch.zeros(4, 3, dtype=torch.float64) if points is None else points
    return lambda: ops.mesh_sdf_query(node_box, n_leaves, torch.zeros(2, 9, dtype=torch.float64), 1, points)


def cluster(verts):
    i32 = torch.zeros(3, dtype=torch.int32)
    return lambda: ops.mesh_cluster_quadrics(verts, i32.reshape(1, 3), i32, i32, torch.zeros(2, dtype=torch.int64),
                                             torch.zeros(1, 3, dtype=torch.float64), 0.1)


_same = f32(1, 16, 4)
_eye = torch.eye(3).reshape(1, 3, 3)
_idx = torch.zeros(4, dtype=torch.int32)

# (label, call, exception type).  The well-formed CPU calls are the ones that prove where an op looks at the device.
BAD_CALLS = [
    ('denoise: guide shape', denoise(g0=f32(16, 3)), ValueError),
    ('denoise: S = 3', denoise(src=f32(3, 16, 4)), ValueError),
    ('denoise: dst is src', denoise(src=_same, dst=_same), ValueError),
    ('denoise: step = 0', denoise(step=0), ValueError),
    ('denoise: NaN sigma', denoise(sigmas=(1., float('nan'), 1.)), ValueError),
    ('denoise: float64 guide', denoise(g1=f32(16, 4).double()), ValueError),
    ('denoise: bad shape on the CPU', denoise(g1=f32(15, 4)), ValueError),
    ('denoise: well-formed on the CPU', denoise(), RuntimeError),
    ('metrics: shape mismatch', metrics(y=f32(1, 16, 17, 3)), ValueError),
    ('metrics: rank 3', metrics(x=f32(16, 16, 3)), ValueError),
    ('metrics: float64', metrics(x=f32(1, 16, 16, 3).double()), ValueError),
    ('metrics: not contiguous', metrics(x=f32(1, 16, 16, 6)[..., ::2]), ValueError),
    ('metrics: not a tensor', lambda: ops.image_metrics([1.0], [1.0], 1), ValueError),
    ('metrics: levels = 3', metrics(levels=3), ValueError),
    ('metrics: C = 5', metrics(x=f32(1, 16, 16, 5)), ValueError),
    ('metrics: 10-pixel side', metrics(x=f32(1, 10, 16, 3)), ValueError),
    ('metrics: MS-SSIM at 160 pixels', metrics(x=f32(1, 160, 160, 1), levels=5), ValueError),
    ('metrics: data_range = 0', metrics(data_range=0.), ValueError),
    ('metrics: well-formed on the CPU', metrics(), RuntimeError),
    ('sdf query: [*, 5] boxes', sdf_query(node_box=torch.zeros(3, 5, dtype=torch.float64)), ValueError),
    ('sdf query: float32 points', sdf_query(points=f32(4, 3)), ValueError),
    ('sdf query: well-formed on the CPU, wrong box count', sdf_query(n_leaves=3), RuntimeError),
    ('sdf query: well-formed on the CPU', sdf_query(), RuntimeError),
    ('components: CPU faces of a bad shape', lambda: ops.mesh_components(torch.zeros(2, 4), 3), RuntimeError),
    ('components: not a tensor', lambda: ops.mesh_components([[0, 1, 2]], 3), RuntimeError),
    ('cluster: CPU verts of a bad shape', cluster(f32(3, 2).double()), RuntimeError),
    ('cluster: not a tensor', cluster(None), RuntimeError),
    ('envmap: [H, W, 4]', lambda: ops._envlight_map(f32(4, 8, 4)), ValueError),
    ('envmap: no rows', lambda: ops._envlight_map(f32(0, 8, 3)), ValueError),
    ('envmap: float64', lambda: ops._envlight_map(f32(4, 8, 3).double()), ValueError),
    ('envmap: not contiguous', lambda: ops._envlight_map(f32(4, 8, 6)[..., ::2]), ValueError),
    ('envmap: well-formed on the CPU', lambda: ops._envlight_map(f32(4, 8, 3)), RuntimeError),
    ('rotations: [3, 3]', lambda: ops.envlight_rotations(torch.eye(3)), ValueError),
    ('rotations: A = 0', lambda: ops.envlight_rotations(f32(0, 3, 3)), ValueError),
    ('rotations: float64', lambda: ops.envlight_rotations(_eye.double()), ValueError),
    ('rotations: not a tensor', lambda: ops.envlight_rotations(None), ValueError),
    ('rotations: well-formed on the CPU', lambda: ops.envlight_rotations(_eye), RuntimeError),
    ('rot_index: dtype', lambda: ops._envlight_rot_index(_idx.long(), 2, 4, _idx.device), ValueError),
    ('rot_index: length', lambda: ops._envlight_rot_index(_idx, 2, 5, _idx.device), ValueError),
    ('rot_index: out of range', lambda: ops._envlight_rot_index(_idx + 2, 2, 4, _idx.device), ValueError),
    ('coordinate type', lambda: ops._envlight_coord('opengl'), ValueError),
    ('light: no lobes', lambda: ops.check_light(f32(0, 7)), ValueError),
    ('light: too many lobes', lambda: ops.check_light(f32(ops.MAX_LOBES + 1, 7)), ValueError),
    ('light: six columns', lambda: ops.check_light(f32(4, 6)), ValueError),
    ('marching cubes: CPU volume', lambda: ops.marching_cubes(f32(4, 4, 4), 0., (0,) * 3, (1,) * 3), RuntimeError),
    ('marching cubes: one layer', lambda: ops.marching_cubes(f32(4, 4, 1), 0., (0,) * 3, (1,) * 3), ValueError),
    ('envfit: CPU tensors', lambda: ops.envfit_loss_grad(f32(4, 7), f32(8, 3), f32(8, 3)), RuntimeError),
    ('envfit: dirs [n, 2]', lambda: ops.envfit_loss_grad(f32(4, 7), f32(8, 2), f32(8, 2)), ValueError),
    ('_ptr: CPU tensor', lambda: ops._ptr(f32(4)), RuntimeError),
]


@pytest.mark.parametrize('label,bad_call,exc', BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_bad_call_raises_what_it_always_raised(label, bad_call, exc):
    with pytest.raises(Exception) as e:
        bad_call()
    assert type(e.value) is exc, (label, repr(e.value))


def test_messages_name_the_argument_and_what_was_received():
    for bad_call, words in ((denoise(g0=f32(16, 3)), ('guides0', '(16, 3)')),
                            (sdf_query(node_box=torch.zeros(3, 5, dtype=torch.float64)), ('node_box', '(3, 5)')),
                            (sdf_query(points=f32(4, 3)), ('points', 'float64')),
                            (lambda: ops._envlight_map(f32(4, 8, 4)), ('envmap', '(4, 8, 4)')),
                            (lambda: ops.envlight_rotations(_eye.double()), ('rot', 'float64'))):
        with pytest.raises(ValueError) as e:
            bad_call()
        assert all(w in str(e.value) for w in words), str(e.value)


def test_call_reports_a_failed_status_under_the_symbol_it_called(monkeypatch):
    """all-NULL arguments: nefii_trace_rays returns NEFII_E_ARG before it touches the device.  The stream getter needs a GPU,
    so it is replaced by the NULL stream where the helper looks it up."""
    import sys
    build.build(verbose=False)
    home = sys.modules[ops.call.__module__]
    monkeypatch.setattr(home, '_stream', lambda: None)
    params = ops.make_tracer_params({}, training=False)
    with pytest.raises(RuntimeError) as e:
        ops.call('nefii_trace_rays', None, ctypes.byref(params), None, None, None, 0, None, None, None, None, None, None, 0,
                 None)
    assert 'nefii_trace_rays failed' in str(e.value) and 'status -1' in str(e.value)
    with pytest.raises(RuntimeError) as e:
        ops.nbytes('nefii_image_metrics_workspace_bytes', 1, 16, 16, 9, 1)
    assert 'nefii_image_metrics_workspace_bytes' in str(e.value)
