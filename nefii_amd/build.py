"""Build libnefii_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m nefii_amd.build [--force]

The shared library is written next to the sources (nefii_amd/csrc/) so that it travels with the
repo snapshot to the GPU box; it is git-ignored.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
SOURCES = ['nefii_mlp.hip', 'nefii_tracer.hip', 'nefii_sdf.hip', 'nefii_shading.hip', 'nefii_probe.hip', 'nefii_envfit.hip',
           'nefii_mcubes.hip', 'nefii_mcubes_sparse.hip', 'nefii_envlight.hip', 'nefii_denoise.hip', 'nefii_meshsdf.hip', 'nefii_meshcc.hip', 'nefii_metrics.hip',
           'nefii_patchloss.hip', 'nefii_meshsimplify.hip', 'nefii_texbake.hip', 'nefii_adaptive.hip']
HEADERS = ['mlp_tile.h', 'sdf_launch.h', 'mc_tables.h', 'mc_cell.h', 'mc_sampling.h', 'envlight_table.h', 'hip_check.h', os.path.join('..', '..', 'include', 'nefii_amd.h')]
OUT = os.path.join(CSRC, 'libnefii_hip.so')
HOST_SRC = os.path.join(CSRC, 'exr_huf.c')          # host-only helper of utils/exr.py (PIZ Huffman loop)
HOST_OUT = os.path.join(CSRC, 'libnefii_host.so')
FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
         # no packed-fp32 VALU instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32): on gfx950 the form with op_sel on
         # src1 read ZERO for that operand in lanes 48-63 while its wave shared a SIMD with waves of the tracer's
         # single-pass evaluator (csrc/mlp_tile.h, NEFII_CLAIM_SIMD; tools/concurrency_probe.py).  The victim side is
         # pinned to the instruction form; WHAT in the neighbour's instruction stream triggers it is not known (the
         # evaluator with every MFMA compiled out still disturbed 40 of 40 runs: profiles/r03/nan_hunt/18) - so the whole
         # class is compiled out.  The host pass does not know the feature and says so: -Wno-...
         '-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops']


def _stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_host(force=False, verbose=True):
    if not force and os.path.exists(HOST_OUT) and os.path.getmtime(HOST_OUT) >= os.path.getmtime(HOST_SRC):
        return HOST_OUT
    cmd = [os.environ.get('CC', 'gcc'), '-O2', '-shared', '-fPIC', '-o', HOST_OUT, HOST_SRC]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return HOST_OUT


def _run_quietly(cmd):
    """check_call that drops the host pass's note about the device-only target feature"""
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    for ln in r.stderr.splitlines():
        if 'packed-fp32-ops' not in ln:
            print(ln, file=sys.stderr)
    if r.returncode:
        raise subprocess.CalledProcessError(r.returncode, cmd)


def build(force=False, verbose=True):
    build_host(force, verbose)
    if not force and not _stale():
        return OUT
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    extra = os.environ.get('NEFII_EXTRA_HIPCC_FLAGS', '').split()
    objs = []
    for s in SOURCES:
        o = os.path.join(CSRC, s.replace('.hip', '.o'))
        cmd = [hipcc] + FLAGS + extra + ['-c', os.path.join(CSRC, s), '-o', o]
        if verbose:
            print(' '.join(cmd), flush=True)
        _run_quietly(cmd)
        objs.append(o)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', OUT] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT


if __name__ == '__main__':
    build(force='--force' in sys.argv)
