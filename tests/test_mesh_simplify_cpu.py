"""What the simplification needs no GPU for: the build and the host checks of nefii_mesh_cluster_quadrics, the torch
clustering and face bookkeeping of nefii_amd/mesh.py on CPU tensors against tests/meshsimplify_ref.py (exact integer
equality), the properties of that reference on closed meshes, and the refusals of extract_mesh and its command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import meshcc_ref  # noqa: E402
import meshsimplify_ref as ref  # noqa: E402


# ---- kernel and build --------------------------------------------------------------------------------------------------
def test_the_source_is_built_and_the_entry_exported():
    from nefii_amd import _lib, build
    assert 'nefii_meshsimplify.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'nefii_meshsimplify.hip'))
    assert 'nefii_mesh_cluster_quadrics' in _lib.SIGNATURES
    assert _lib.lib().nefii_mesh_cluster_quadrics is not None
    with open(os.path.join(ROOT, 'include', 'nefii_amd.h')) as f:
        assert 'int nefii_mesh_cluster_quadrics(' in f.read()


def test_the_entry_checks_its_arguments_on_the_host():
    from nefii_amd import _lib
    fn = _lib.lib().nefii_mesh_cluster_quadrics
    E_ARG, E_SHAPE = -1, -2
    p = ctypes.c_void_p(256)                                  # never dereferenced: every call below returns before a launch
    inf, nan = float('inf'), float('nan')

    def call(ptrs=None, counts=(4, 2, 2), h=0.1, eps=1e-3, clamp=0.5):
        q = [p] * 8 if ptrs is None else ptrs                 # verts faces cluster corners seg centre pos flags
        V, F, C = counts
        return fn(q[0], V, q[1], F, q[2], q[3], q[4], q[5], C, h, eps, clamp, q[6], q[7], None)

    for i in range(8):
        assert call([None if j == i else p for j in range(8)]) == E_ARG, i
    for h in (0.0, -1.0, inf, nan):
        assert call(h=h) == E_ARG, h
    for eps in (-1e-3, nan, inf):
        assert call(eps=eps) == E_ARG, eps
    for clamp in (0.0, -0.5, inf, nan):
        assert call(clamp=clamp) == E_ARG, clamp
    for bad in (-1, 1 << 31, 1 << 40):
        for which in range(3):
            counts = [4, 2, 2]
            counts[which] = bad
            assert call(counts=counts) == E_SHAPE, (bad, which)
    assert call(counts=(4, 0, 2)) == 0                        # no faces, no clusters: nothing to launch
    assert call(counts=(4, 2, 0)) == 0
    assert call(counts=(0, 0, 0)) == 0


def test_the_gpu_steps_refuse_cpu_tensors_and_bad_cells():
    from nefii_amd import mesh, ops
    v, f = ref.fan(6)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    cluster, centre, C = mesh.cluster_vertices(tv, tf, 0.3)
    corners, seg = mesh.corner_runs(tf, cluster, C)
    with pytest.raises(RuntimeError):
        ops.mesh_cluster_quadrics(tv, tf.int(), cluster.int(), corners, seg, centre, 0.3)
    with pytest.raises(ValueError, match='CUDA'):
        mesh.simplify_mesh(mesh.Mesh(tv, tf), 0.3)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='cell'):
            mesh.simplify_mesh(mesh.Mesh(tv, tf), bad)
        with pytest.raises(ValueError, match='cell'):
            mesh.cluster_vertices(tv, tf, bad)
    empty = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))
    assert mesh.simplify_mesh(empty, 0.3) is empty            # an empty mesh passes through, on any device
    no_faces = mesh.Mesh(tv, torch.zeros(0, 3, dtype=torch.int64))
    assert mesh.simplify_mesh(no_faces, 0.3) is no_faces
    with pytest.raises(ValueError, match='outside'):
        mesh.cluster_vertices(tv, torch.tensor([[0, 1, 7]]), 0.3)
    with pytest.raises(ValueError, match='outside'):
        mesh.cluster_vertices(tv, torch.tensor([[0, -1, 2]]), 0.3)


# ---- cluster_vertices / cluster_faces against the reference -----------------------------------------------------------
def check_host_layer(verts, faces, cell):
    """mesh.cluster_vertices, corner_runs and cluster_faces on CPU tensors against the reference -> the reference's result"""
    from nefii_amd import mesh
    verts, faces = np.array(verts), np.array(faces, dtype=np.int64).reshape(-1, 3)
    tv, tf = torch.from_numpy(verts), torch.from_numpy(faces)
    want = ref.simplify(verts, faces, cell)
    cluster, centre, C = mesh.cluster_vertices(tv, tf, cell)
    assert cluster.dtype == torch.int64 and centre.dtype == torch.float64 and centre.shape == (C, 3)
    assert C == want['clusters'] and np.array_equal(cluster.numpy(), want['cluster'])
    r_centre = ref.cluster_vertices(verts, faces, cell)[1]
    assert np.array_equal(centre.numpy(), r_centre)
    corners, seg = mesh.corner_runs(tf, cluster, C)
    assert corners.dtype == torch.int32 and seg.dtype == torch.int64 and seg.shape == (C + 1,)
    key = want['cluster'][faces.reshape(-1)]
    assert np.array_equal(corners.numpy(), np.argsort(key, kind='stable'))
    assert np.array_equal(seg.numpy(), np.searchsorted(np.sort(key), np.arange(C + 1)))
    nf, kept, cancelled = mesh._cluster_faces(tf, cluster)
    pub = mesh.cluster_faces(tf, cluster)
    assert torch.equal(pub[0], nf) and torch.equal(pub[1], kept)
    assert nf.dtype == torch.int64 and kept.dtype == torch.int64
    r_faces, r_kept, r_cancelled = ref.cluster_faces(faces, want['cluster'])
    assert np.array_equal(nf.numpy().reshape(-1, 3), r_faces) and np.array_equal(kept.numpy(), r_kept)
    assert cancelled == r_cancelled == want['cancelled']
    return want


@pytest.mark.parametrize('name,k', ref.CASES)
def test_clustering_and_faces_match_the_reference_on_grid_meshes(name, k):
    v, f, sp = ref.grid_mesh(name)
    want = check_host_layer(v, f, k * sp)
    print('%s at %g spacings: %d -> %d faces, %d clusters, %d unused, %d sets cancelled' % (
        name, k, len(f), len(want['faces']), want['clusters'], want['unused'], want['cancelled']))
    assert 0 < len(want['faces']) < len(f) / 3
    if name == 'thin':                                       # the case must not go vacuous
        assert want['cancelled'] >= 1 and want['unused'] >= 1


def test_clustering_and_faces_match_the_reference_on_hand_made_cases():
    from nefii_amd import mesh
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [5, 5, 5], [0.1, 0.1, 0.1]],
                  dtype=np.float32)
    # vertices 6 and 7 are used by no face
    w = check_host_layer(sq, [[0, 1, 2], [0, 2, 3], [0, 1, 4]], 0.5)
    assert w['cluster'][6] == -1 and w['cluster'][7] == -1 and w['clusters'] == 5 and len(w['faces']) == 3
    # a face with a repeated index is dropped; what is left keeps its input order
    w = check_host_layer(sq, [[0, 1, 1], [0, 1, 2], [3, 3, 3], [0, 2, 3]], 0.5)
    assert w['kept_face'].tolist() == [1, 3]
    # two identical faces: the first stays
    w = check_host_layer(sq, [[0, 2, 3], [0, 1, 2], [1, 2, 0], [0, 1, 2]], 0.5)
    assert w['kept_face'].tolist() == [0, 1]
    # a face and its mirror cancel; two against one: the first of the majority stays
    w = check_host_layer(sq, [[0, 1, 2], [2, 1, 0], [0, 2, 3]], 0.5)
    assert w['kept_face'].tolist() == [2] and w['cancelled'] == 1 and w['unused'] == 1
    w = check_host_layer(sq, [[0, 1, 2], [2, 1, 0], [0, 2, 3], [1, 0, 2]], 0.5)
    assert w['kept_face'].tolist() == [1, 2] and w['cancelled'] == 0
    # vertices 0 and 7 share a cell: the face over them collapses
    w = check_host_layer(sq, [[0, 7, 1], [7, 1, 2]], 0.5)
    assert w['kept_face'].tolist() == [1]
    # everything in one cell: no face is left
    w = check_host_layer(sq[:6], [[0, 1, 2], [0, 2, 3], [0, 1, 4]], 8.0)
    assert w['clusters'] == 1 and len(w['faces']) == 0 and w['unused'] == 1
    # no faces at all
    w = check_host_layer(sq, np.zeros((0, 3), dtype=np.int64), 0.5)
    assert w['clusters'] == 0 and (w['cluster'] == -1).all()
    nf, kept = mesh.cluster_faces(torch.zeros(0, 3, dtype=torch.int64), torch.full((8,), -1, dtype=torch.int64))
    assert nf.shape == (0, 3) and kept.shape == (0,)
    # disjoint tetrahedra, each vertex alone in its cell: nothing merges, nothing is dropped
    n = 9
    tv = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])[None] + 4.0 * np.arange(n)[:, None, None]).reshape(-1, 3)
    w = check_host_layer(tv.astype(np.float32), meshcc_ref.tetrahedra(n), 0.75)
    assert w['clusters'] == 4 * n and len(w['faces']) == 4 * n and w['unused'] == 0


# ---- properties of the reference on closed meshes ----------------------------------------------------------------------
@pytest.mark.parametrize('name,k', ref.CASES)
def test_the_reference_keeps_closed_meshes_balanced(name, k):
    v, f, sp = ref.grid_mesh(name)
    assert ref.unbalanced_edges(f) == 0
    r = ref.simplify(v, f, k * sp)
    assert ref.unbalanced_edges(r['faces']) == 0             # (not is_closed_oriented: an edge may carry two face pairs)
    assert ref.repeated_index_faces(r['faces']) == 0
    assert ref.shared_vertex_sets(r['faces']) == 0
    assert r['faces'].min() == 0 and r['faces'].max() == len(r['verts']) - 1
    share = r['clamped'].mean()
    print('%s at %g spacings: clamped share %.3f' % (name, k, share))
    assert share < 0.1                                       # the prototype: at most 0.055
    assert ref.unbalanced_edges([[0, 1, 2], [2, 1, 3]]) == 4 and ref.unbalanced_edges(meshcc_ref.TETRA) == 0


def test_quadric_positions_beat_the_cell_means_on_the_box():
    v, f, sp = ref.grid_mesh('box')
    r = ref.simplify(v, f, 3 * sp)
    q = np.abs(meshcc_ref.box_sdf(r['verts'])).mean()
    m = np.abs(meshcc_ref.box_sdf(r['mean'])).mean()
    print('box at 3 spacings: %d -> %d faces; mean |sdf| %.3e (quadrics) against %.3e (cell means): %.2f' % (
        len(f), len(r['faces']), q, m, q / m))
    assert (len(f), len(r['faces'])) == (5448, 506)
    assert q <= 0.5 * m                                      # the prototype: 0.38


def test_projection_runs_on_cpu_tensors_and_respects_max_move():
    from nefii_amd import mesh
    c, radius = np.array(ref.SPHERE[0]), ref.SPHERE[1]

    def vg(x):
        d = x.double() - torch.from_numpy(c)
        n = d.norm(dim=1)
        return n - radius, d / n[:, None]

    start = torch.from_numpy(c + np.array([[0.5, 0, 0], [0, 0.3, 0.3], [0.2, 0.2, 0.2], [0.45, 0.0, 0.0]])).float()
    out = mesh.project_to_level_set(vg, start)
    assert out.dtype == torch.float32 and vg(out)[0].abs().max().item() <= 1e-6
    want = ref.project(lambda x: tuple(t.numpy() for t in vg(torch.from_numpy(x))), start.numpy())
    assert np.abs(out.numpy() - want).max() <= 2.0 ** -23
    held = mesh.project_to_level_set(vg, start, max_move=0.01)
    assert (held - start).abs().max().item() <= 0.01 + 2.0 ** -23 and vg(held)[0].abs().max().item() > 0.01
    assert torch.equal(mesh.project_to_level_set(vg, start, steps=0), start)
    level = mesh.project_to_level_set(vg, start, level=0.05)
    assert (vg(level)[0] - 0.05).abs().max().item() <= 1e-6


# ---- extract_mesh and the command line ---------------------------------------------------------------------------------
def test_extract_mesh_refuses_cells_of_one_spacing_or_less():
    from nefii_amd import mesh, synthetic as syn, conf
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    model = IDRNetwork(conf.from_dict(syn.model_conf('conf')))
    for bad in (0.5, 1.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='simplify'):
            mesh.extract_mesh(model, resolution=8, simplify=bad)


@pytest.mark.parametrize('value', ['-1', '0.5'])
def test_the_command_line_refuses_a_bad_simplify(value, tmp_path):
    r = subprocess.run([sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(tmp_path / 'none.conf'),
                        '--geometry', str(tmp_path / 'none.pth'), '--out', str(tmp_path / 'o.ply'), '--simplify', value],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'extract_mesh: --simplify must be 0 (off) or ' in r.stderr, r.stdout + r.stderr
    assert 'unrecognized' not in r.stderr and 'usage' not in r.stderr       # the script's own refusal, not the parser's
