"""SDFDataset: signed-distance samples of a mesh for the Step-1 geometry fit (reference code/datasets/sdf_dataset.py:
18-103): each item is `sample_num` positions with their signed distance, drawn afresh every time.

The reference delegates to two packages that are not installable here - trimesh 3.12.0 (mesh loading) and mesh-to-sdf
0.0.14 (`get_surface_point_cloud(...).sample_sdf_near_surface`, requirements.sh:11) - so this file restates what that
call does rather than how:
  * query positions, as mesh-to-sdf draws them: 47/50 of the samples lie near the surface - uniformly (by area) sampled
    surface points displaced by isotropic Gaussian noise, half with sigma 0.0025 and half with sigma 0.00025 - and the
    rest are uniform in the unit ball;
  * the signed distance of each query: mesh-to-sdf approximates it from a scanned point cloud (nearest of 10 M scan
    points, sign from the neighbours' normals).  Here it is the exact distance to the triangle mesh, negative inside;
    inside / outside is by default (`sign='parity'`) the parity of ray crossings, which asks for a closed mesh: a hole
    leaves a streak of wrong signs behind it, and an overlap of two closed parts counts as outside.  `sign='winding'`
    takes it from the generalized winding number instead (inside where w > 0.5), much as the scan-based
    sign comes from normals: open meshes and unions of closed parts get the sign a reader of the mesh expects.
  * `scale_to_unit`: the mesh is centred on its bounding-box centre and scaled so that its farthest vertex lies on the
    unit sphere before sampling; positions and distances are mapped back afterwards (sdf_dataset.py:52-55,62-77).
All of it is torch on whatever device the dataset is given: a 16384-sample batch against a 37 k-face mesh is 6e8
point-triangle pairs, 0.28 s on an MI355X, and the cost grows with the face count.

That is `method='brute'`: queries x faces.  On the GPU `method='bvh'` answers the same query through a bounding-volume
hierarchy over the faces (mesh_bvh.py, csrc/nefii_meshsdf.hip), whose cost per query grows with the depth of
the tree instead; `'auto'` (samplers and datasets) picks 'bvh' on a GPU and 'brute' on the CPU."""
import numpy as np
import torch

from ..mesh_bvh import build_bvh, build_moments, morton63

SORT_QUERIES = True                 # MeshSDF(method='bvh'): Morton-sort the queries before the kernel (measured: DESIGN.md 6k)
METHODS = ('brute', 'bvh')
SIGNS = ('parity', 'winding')
WINDING_BETA = 2.0                  # MeshSDF(sign='winding'): the tree's accept ratio (error measured: DESIGN.md 6s)


def resolve_method(method, device):
    """'auto' -> 'bvh' on a CUDA device, 'brute' elsewhere; anything but 'auto', 'brute', 'bvh' is refused"""
    if method == 'auto':
        return 'bvh' if torch.device(device).type == 'cuda' else 'brute'
    if method not in METHODS:
        raise ValueError("method must be 'auto', 'brute' or 'bvh', got %r" % (method,))
    return method


def load_obj(path):
    """Wavefront OBJ -> (vertices [V, 3] float64, triangles [F, 3] int64); polygons are fan-triangulated"""
    verts, faces = [], []
    with open(path) as f:
        for line in f:
            if line.startswith('v '):
                verts.append([float(t) for t in line.split()[1:4]])
            elif line.startswith('f '):
                idx = []
                for t in line.split()[1:]:
                    i = int(t.split('/')[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    if not verts or not faces:
        raise ValueError('no triangles in ' + str(path))
    return np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)


# a fixed rotation applied before the parity test, so that axis-aligned meshes do not put edges exactly under the rays
_SKEW = torch.tensor([[0.8320502943, -0.5547001962, 0.0], [0.4961389384, 0.7442084075, -0.4472135955],
                      [0.2480694692, 0.3721042038, 0.8944271910]], dtype=torch.float64)
_SKEW = torch.linalg.qr(_SKEW)[0]


class MeshSDF:
    """Exact distance to a triangle mesh with an inside / outside sign, and area-uniform surface samples.

    method 'brute': every query against every face in dense fp64 torch ops, on any device.  'bvh': the query kernel over a
    tree built on first use (GPU only: there is no fallback).  sort_queries (bvh): hand the kernel the queries in Morton
    order and un-permute the result - the same bits either way, since a query's result does not depend on its place.

    sign 'parity': inside where a ray crosses an odd number of faces - a closed mesh is asked for.  'winding': inside where
    orientation * w > 0.5, w the generalized winding number (winding()): open meshes and overlapping closed parts are
    welcome.  orientation is the sign of the mesh's signed volume sum a . (b x c) / 6 (+1 when that is 0), so an inside-out
    mesh needs no flag.  winding_beta (bvh): 0 sums every face exactly, b >= 1 takes a node farther than b times its radius
    as one dipole."""

    def __init__(self, vertices, faces, device='cpu', pair_budget=1 << 24, method='brute', sort_queries=SORT_QUERIES,
                 sign='parity', winding_beta=WINDING_BETA):
        if method not in METHODS:
            raise ValueError("method must be 'brute' or 'bvh', got %r" % (method,))
        if sign not in SIGNS:
            raise ValueError("sign must be 'parity' or 'winding', got %r" % (sign,))
        from ..ops.mesh import check_winding_beta
        self.sign, self.winding_beta = sign, check_winding_beta(winding_beta)
        if method == 'bvh' and torch.device(device).type != 'cuda':
            raise ValueError("method='bvh' runs on the HIP kernel and needs a CUDA device, got %r" % (device,))
        self.method, self.sort_queries, self._bvh = method, sort_queries, None
        v = torch.as_tensor(vertices, dtype=torch.float64, device=device)
        f = torch.as_tensor(faces, dtype=torch.long, device=device)
        self.a, self.b, self.c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        n = torch.cross(self.b - self.a, self.c - self.a, dim=1)
        keep = n.norm(dim=1) > 0                                    # zero-area faces carry no surface
        self.a, self.b, self.c, n = self.a[keep], self.b[keep], self.c[keep], n[keep]
        if self.a.shape[0] == 0:
            raise ValueError('the mesh has no face of non-zero area')
        self.n = n
        self.area = 0.5 * n.norm(dim=1)
        self.cdf = torch.cumsum(self.area / self.area.sum(), 0)
        self.pair_budget = pair_budget
        R = _SKEW.to(device)
        self.ra, self.rb, self.rc = self.a @ R.T, self.b @ R.T, self.c @ R.T
        self.R = R
        self.orientation = -1.0 if (self.a * torch.cross(self.b, self.c, dim=1)).sum().item() < 0 else 1.0

    @property
    def device(self):
        return self.a.device

    def sample_surface(self, count, generator=None):
        u = torch.rand(count, 3, dtype=torch.float64, generator=generator).to(self.device)
        tri = torch.searchsorted(self.cdf, u[:, 0].contiguous()).clamp_(max=self.cdf.shape[0] - 1)
        r1 = u[:, 1].sqrt()
        w0, w1, w2 = 1 - r1, r1 * (1 - u[:, 2]), r1 * u[:, 2]
        return w0[:, None] * self.a[tri] + w1[:, None] * self.b[tri] + w2[:, None] * self.c[tri]

    @staticmethod
    def _segment_d2(p, a, ab):
        t = (((p - a) * ab).sum(-1) / (ab * ab).sum(-1).clamp_min(1e-300)).clamp(0, 1)
        d = p - (a + t[..., None] * ab)
        return (d * d).sum(-1)

    @property
    def bvh(self):
        """the tree over the faces in the skewed frame (one tree serves the distance and the parity pass)"""
        if self._bvh is None:
            self._bvh = build_bvh(self.ra, self.rb, self.rc)
        return self._bvh

    def _through_tree(self, points, query):
        """query(q) on the points in the tree's frame, Morton-sorted and un-permuted when sort_queries is set"""
        t = self.bvh
        q = (torch.as_tensor(points, dtype=torch.float64, device=self.device).reshape(-1, 3) @ self.R.T).contiguous()
        if not self.sort_queries or q.shape[0] < 2:
            return query(q)
        order = torch.sort(morton63(q, t.node_box[0, :3], t.node_box[0, 3:])).indices
        return torch.empty(q.shape[0], dtype=torch.float64, device=q.device).index_copy_(0, order, query(q[order]))

    def _call_bvh(self, points, signed):
        from .. import ops
        t = self.bvh
        if not (signed and self.sign == 'winding'):
            return self._through_tree(points,
                                      lambda q: ops.mesh_sdf_query(t.node_box, t.n_leaves, t.tris, t.leaf_size, q, signed))
        moment = build_moments(t)

        def query(q):                                               # the unsigned distance, then the winding number
            d = ops.mesh_sdf_query(t.node_box, t.n_leaves, t.tris, t.leaf_size, q, False)
            w = ops.mesh_winding_query(t.node_box, moment, t.n_leaves, t.tris, t.leaf_size, q, self.winding_beta)
            return torch.where(self.orientation * w > 0.5, -d, d)
        return self._through_tree(points, query)

    def winding(self, points):
        """generalized winding number of points [..., 3] -> [P] fp64, in the orientation the mesh came in: the faces' signed
        solid angles over 4 pi.  'brute': every query against every face (Van Oosterom & Strackee's formula), on any device;
        'bvh': the kernel over the tree and its moments, at winding_beta."""
        if self.method == 'bvh':
            from .. import ops
            t = self.bvh
            moment = build_moments(t)
            return self._through_tree(points, lambda q: ops.mesh_winding_query(t.node_box, moment, t.n_leaves, t.tris,
                                                                                t.leaf_size, q, self.winding_beta))
        p_all = torch.as_tensor(points, dtype=torch.float64, device=self.device).reshape(-1, 3)
        out = torch.empty(p_all.shape[0], dtype=torch.float64, device=self.device)
        step = max(1, self.pair_budget // self.a.shape[0])
        for s in range(0, p_all.shape[0], step):
            p = p_all[s:s + step, None, :]                          # [P, 1, 3] against [1, F, 3]
            A, B, C = self.a[None] - p, self.b[None] - p, self.c[None] - p
            la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
            num = (A * torch.cross(B, C, dim=-1)).sum(-1)
            den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
            out[s:s + step] = (2.0 * torch.atan2(num, den)).sum(1) / (4.0 * np.pi)
        return out

    def __call__(self, points, signed=True):
        """signed distance of points [..., 3] -> [P] fp64; signed=False: the unsigned distance (bvh: no sign pass)"""
        if self.method == 'bvh':
            return self._call_bvh(points, signed)
        if signed and self.sign == 'winding':
            d = self(points, signed=False)
            return torch.where(self.orientation * self.winding(points) > 0.5, -d, d)
        p_all = torch.as_tensor(points, dtype=torch.float64, device=self.device).reshape(-1, 3)
        out = torch.empty(p_all.shape[0], dtype=torch.float64, device=self.device)
        F = self.a.shape[0]
        step = max(1, self.pair_budget // F)
        a, b, c, n = self.a[None], self.b[None], self.c[None], self.n[None]
        nn = (self.n * self.n).sum(-1)[None]
        for s in range(0, p_all.shape[0], step):
            p = p_all[s:s + step, None, :]                          # [P, 1, 3] against [1, F, 3]
            ap, bp, cp = p - a, p - b, p - c
            inside = ((torch.cross(b - a, ap, dim=-1) * n).sum(-1) >= 0) & \
                     ((torch.cross(c - b, bp, dim=-1) * n).sum(-1) >= 0) & \
                     ((torch.cross(a - c, cp, dim=-1) * n).sum(-1) >= 0)
            d_plane = (ap * n).sum(-1) ** 2 / nn
            d_edge = torch.minimum(torch.minimum(self._segment_d2(p, a, b - a), self._segment_d2(p, b, c - b)),
                                   self._segment_d2(p, c, a - c))
            d2 = torch.where(inside, d_plane, d_edge).min(dim=1).values
            # parity of crossings of the ray p + t * z (t > 0), in the skewed frame
            q = (p_all[s:s + step] @ self.R.T)[:, None, :]
            ra, rb, rc = self.ra[None], self.rb[None], self.rc[None]

            def edge(u, v):                                         # 2-D edge function of q against u -> v
                return (v[..., 0] - u[..., 0]) * (q[..., 1] - u[..., 1]) - (v[..., 1] - u[..., 1]) * (q[..., 0] - u[..., 0])
            e0, e1, e2 = edge(ra, rb), edge(rb, rc), edge(rc, ra)
            covers = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
            area2 = e0 + e1 + e2
            z = (e1 * ra[..., 2] + e2 * rb[..., 2] + e0 * rc[..., 2]) / torch.where(area2 == 0, torch.ones_like(area2), area2)
            crossings = (covers & (area2 != 0) & (z > q[..., 2])).sum(dim=1)
            sign = torch.where(crossings % 2 == 1, -1.0, 1.0).to(torch.float64)
            out[s:s + step] = sign * d2.sqrt()
        return out if signed else out.abs()


class SDFSampler(object):                                           # sdf_dataset.py:18-77
    def __init__(self, mesh_path, number_of_points=500000, scale_to_unit=True, device='cpu', mesh=None, method='auto',
                 sign='parity', winding_beta=WINDING_BETA):
        self.method = resolve_method(method, device)
        self.number_of_points = number_of_points
        self.scale_to_unit = scale_to_unit
        vertices, faces = mesh if mesh is not None else load_obj(mesh_path)
        vertices = np.asarray(vertices, dtype=np.float64)
        # centre of the bounding box / farthest vertex (trimesh's bounding_box.centroid, :66-73)
        self.center = (vertices.min(0) + vertices.max(0)) / 2 if scale_to_unit else np.zeros(3)
        self.scale = float(np.linalg.norm(vertices - self.center, axis=1).max()) if scale_to_unit else 1.0
        self.mesh_sdf = MeshSDF((vertices - self.center) / self.scale, faces, device=device, method=self.method, sign=sign,
                                winding_beta=winding_beta)

    def sample(self, generator=None):
        n = self.number_of_points
        near = int(n * 47 / 50) // 2                                # mesh-to-sdf: surface_sample_count
        m = self.mesh_sdf
        surf = m.sample_surface(near, generator)
        noise = torch.randn(2, near, 3, dtype=torch.float64, generator=generator).to(m.device)
        ball = torch.randn(n - 2 * near, 3, dtype=torch.float64, generator=generator).to(m.device)
        radius = torch.rand(n - 2 * near, 1, dtype=torch.float64, generator=generator).to(m.device) ** (1.0 / 3.0)
        ball = ball / ball.norm(dim=1, keepdim=True) * radius
        points = torch.cat([surf + 0.0025 * noise[0], surf + 0.00025 * noise[1], ball], 0)
        sdf = m(points)
        center = torch.as_tensor(self.center, dtype=torch.float64, device=m.device)
        return (points * self.scale + center).reshape(-1, 3), (sdf * self.scale).reshape(-1, 1)


class SDFDataset(torch.utils.data.Dataset):                         # sdf_dataset.py:80-103
    def __init__(self, mesh_path, sample_num, max_iter_num, scale_to_unit=True, device='cpu', mesh=None, method='auto',
                 sign='parity', winding_beta=WINDING_BETA):
        self.sample_num = sample_num
        self.max_iter_num = max_iter_num
        self.sdf_sampler = SDFSampler(mesh_path, sample_num, scale_to_unit=scale_to_unit, device=device, mesh=mesh,
                                      method=method, sign=sign, winding_beta=winding_beta)
        self.generator = None

    def __getitem__(self, idx):
        points, sdf = self.sdf_sampler.sample(self.generator)
        return points.float(), sdf.float()

    def __len__(self):
        return self.max_iter_num

    def collate_fn(self, batch_list):
        return tuple(torch.cat(entry, 0) for entry in zip(*batch_list))
