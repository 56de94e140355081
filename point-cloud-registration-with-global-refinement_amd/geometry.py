"""Stand-ins for the ``o3d.geometry`` objects the reference's hot path touches:
``PointCloud`` with device-resident float32 storage and ``KDTreeSearchParam{KNN,Radius,Hybrid}``.

Reference call sites: ``voxel_down_sample`` ALL_FUNCTIONS.py:293-294, ``remove_statistical_outlier``
:297-298, ``estimate_normals`` :182-183/:214-215/:301-302, ``estimate_covariances`` :216-217,
``get_min_bound/get_max_bound`` :1093-1097, ``transform`` :46, ``copy.deepcopy`` :289-290,
``compute_nearest_neighbor_distance`` :1077-1078, ``get_center`` :1022/:1035, ``compute_mean_and_covariance`` :1043.
Every method that computes dispatches to ``libpcr_hip.so``; the host only builds index lists (``uniform_down_sample``, the ``invert`` form
of ``select_by_index``) and moves rows with torch on the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class KDTreeSearchParamKNN:
    def __init__(self, knn: int = 30):
        self.knn = int(knn)

    def _spec(self):
        return _lib.SEARCH_KNN, self.knn, 0.0


class KDTreeSearchParamRadius:
    def __init__(self, radius: float):
        self.radius = float(radius)

    def _spec(self):
        return _lib.SEARCH_RADIUS, 0, self.radius


class KDTreeSearchParamHybrid:
    def __init__(self, radius: float, max_nn: int):
        self.radius = float(radius)
        self.max_nn = int(max_nn)

    def _spec(self):
        return _lib.SEARCH_HYBRID, self.max_nn, self.radius


def _torch():
    import torch
    return torch


def _dev_f32(a, cols):
    """array-like / torch tensor -> contiguous float32 cuda tensor of shape (N, cols)."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the MI355X registration path cannot run (no CPU fallback)")
    if isinstance(a, torch.Tensor):
        t = a.to(device="cuda", dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()
    return t.reshape(-1, cols).contiguous()


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


class PointCloud:
    """Device-resident point cloud (float32 xyz on the GPU; Open3D keeps float64 on the host)."""

    def __init__(self, points=None):
        self._xyz = None          # torch (N,3) float32 cuda
        self._nrm = None          # torch (N,3) float32 cuda
        self._cov = None          # torch (N,6) float32 cuda  (xx,xy,xz,yy,yz,zz)
        self._col = None          # torch (N,3) float32 cuda  (r,g,b in [0, 1])
        self._tim = None          # torch (N,) float32 cuda   (one time per point: the rule "continuous time" of include/pcr_hip.h)
        if points is not None:
            self.points = points

    # ---- o3d-like attribute surface -------------------------------------------------------------
    @property
    def points(self):
        if self._xyz is None:
            return np.zeros((0, 3), np.float64)
        return self._xyz.detach().cpu().numpy().astype(np.float64)

    @points.setter
    def points(self, value):
        self._xyz = _dev_f32(value, 3)
        self._nrm = None
        self._cov = None
        self._col = None
        self._tim = None

    @property
    def normals(self):
        if self._nrm is None:
            return np.zeros((0, 3), np.float64)
        return self._nrm.detach().cpu().numpy().astype(np.float64)

    @normals.setter
    def normals(self, value):
        self._nrm = _dev_f32(value, 3)

    @property
    def colors(self):
        if self._col is None:
            return np.zeros((0, 3), np.float64)
        return self._col.detach().cpu().numpy().astype(np.float64)

    @colors.setter
    def colors(self, value):
        self._col = _dev_f32(value, 3)

    @property
    def times(self):
        """One time per point, float32 (n,); empty on a cloud without times.  A spinning LiDAR measures every point of a sweep at its own time:
        ``deskew`` and the continuous-time registration (``registration_point_map_continuous``) read them."""
        if self._tim is None:
            return np.zeros((0,), np.float32)
        return self._tim.detach().cpu().numpy()

    @times.setter
    def times(self, value):
        t = _dev_f32(value, 1).reshape(-1)
        if t.shape[0] != len(self):
            raise ValueError(f"times must hold one value per point ({len(self)}), got {t.shape[0]}")
        self._tim = t.contiguous()

    @property
    def covariances(self):
        if self._cov is None:
            return np.zeros((0, 3, 3), np.float64)
        c = self._cov.detach().cpu().numpy().astype(np.float64)
        out = np.empty((c.shape[0], 3, 3))
        out[:, 0, 0] = c[:, 0]; out[:, 0, 1] = out[:, 1, 0] = c[:, 1]; out[:, 0, 2] = out[:, 2, 0] = c[:, 2]
        out[:, 1, 1] = c[:, 3]; out[:, 1, 2] = out[:, 2, 1] = c[:, 4]; out[:, 2, 2] = c[:, 5]
        return out

    @covariances.setter
    def covariances(self, value):
        """(n, 3, 3) matrices (the upper triangle is kept) or (n, 6) rows xx,xy,xz,yy,yz,zz; stored as float32 cov6 on the device."""
        torch = _torch()
        shape = tuple(value.shape) if hasattr(value, "shape") else np.asarray(value).shape
        if len(shape) == 3 and shape[1:] == (3, 3):
            v = value if isinstance(value, torch.Tensor) else np.asarray(value)
            value = v.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]
        elif not (len(shape) == 2 and shape[1] == 6):
            raise ValueError(f"covariances must have shape (n, 3, 3) or (n, 6), got {shape}")
        self._cov = _dev_f32(value, 6)

    def __len__(self):
        return 0 if self._xyz is None else int(self._xyz.shape[0])

    def has_points(self):
        return len(self) > 0

    def has_normals(self):
        return self._nrm is not None and self._nrm.shape[0] == len(self) and len(self) > 0

    def has_covariances(self):
        return self._cov is not None and self._cov.shape[0] == len(self) and len(self) > 0

    def has_colors(self):
        return self._col is not None and self._col.shape[0] == len(self) and len(self) > 0

    def has_times(self):
        return self._tim is not None and self._tim.shape[0] == len(self) and len(self) > 0

    def paint_uniform_color(self, color):
        """``PointCloud.paint_uniform_color`` (ALL_FUNCTIONS.py:23,155-156): every point gets the colour ``color`` = (r, g, b) in [0, 1]; returns self."""
        torch = _torch()
        rgb = torch.as_tensor(np.asarray(color, dtype=np.float32).reshape(3), device="cuda")
        self._col = rgb.repeat(len(self), 1).contiguous()
        return self

    def __deepcopy__(self, memo):
        out = PointCloud()
        out._xyz = None if self._xyz is None else self._xyz.clone()
        out._nrm = None if self._nrm is None else self._nrm.clone()
        out._cov = None if self._cov is None else self._cov.clone()
        out._col = None if self._col is None else self._col.clone()
        out._tim = None if self._tim is None else self._tim.clone()
        return out

    def __repr__(self):
        return f"PointCloud with {len(self)} points."

    # ---- device views used by the registration layer ---------------------------------------------
    def device_xyz(self):
        if self._xyz is None:
            self._xyz = _torch().zeros((0, 3), dtype=_torch().float32, device="cuda")
        return self._xyz

    def device_normals(self):
        return self._nrm

    def device_colors(self):
        return self._col

    def device_times(self):
        return self._tim

    # ---- methods -----------------------------------------------------------------------------
    def get_min_bound(self):
        return self._bounds()[:3]

    def get_max_bound(self):
        return self._bounds()[3:]

    def _bounds(self):
        ctx = _lib.Context.current()
        b = (C.c_double * 6)()
        xyz = self.device_xyz()
        ctx.check(ctx.lib.pcr_bounds(ctx.handle, _ptr(xyz), C.c_int64(len(self)), b), "get_min_bound/get_max_bound")
        return np.array(b, dtype=np.float64)

    def voxel_down_sample(self, voxel_size: float) -> "PointCloud":
        ctx = _lib.Context.current()
        torch = _torch()
        n = len(self)
        xyz = self.device_xyz()
        out_xyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device="cuda")
        has_n = self.has_normals()
        out_nrm = torch.empty((max(n, 1), 3), dtype=torch.float32, device="cuda") if has_n else None
        m = C.c_int64(0)
        out_col = None
        if self.has_colors():          # colours are averaged per voxel too (Open3D); points and normals are those of the call below
            out_col = torch.empty((max(n, 1), 3), dtype=torch.float32, device="cuda")
            ctx.check(ctx.lib.pcr_voxel_down_sample_ex(ctx.handle, _ptr(xyz), _ptr(self._nrm if has_n else None), _ptr(self._col), C.c_int64(n),
                                                       C.c_double(voxel_size), _ptr(out_xyz), _ptr(out_nrm), _ptr(out_col), C.byref(m)),
                      "voxel_down_sample")
        else:
            ctx.check(ctx.lib.pcr_voxel_down_sample(ctx.handle, _ptr(xyz), _ptr(self._nrm if has_n else None), C.c_int64(n),
                                                    C.c_double(voxel_size), _ptr(out_xyz), _ptr(out_nrm), C.byref(m)),
                      "voxel_down_sample")
        out = PointCloud()
        out._xyz = out_xyz[: m.value].contiguous()
        if has_n:
            out._nrm = out_nrm[: m.value].contiguous()
        if out_col is not None:
            out._col = out_col[: m.value].contiguous()
        if self.has_times():           # the per-voxel mean of the times, with the arithmetic of a colour channel: a second call whose colours are (t, t, t)
            ttt = self._tim.reshape(-1, 1).repeat(1, 3).contiguous()
            t_xyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device="cuda")
            t_col = torch.empty((max(n, 1), 3), dtype=torch.float32, device="cuda")
            mt = C.c_int64(0)
            ctx.check(ctx.lib.pcr_voxel_down_sample_ex(ctx.handle, _ptr(xyz), None, _ptr(ttt), C.c_int64(n), C.c_double(voxel_size), _ptr(t_xyz), None, _ptr(t_col),
                                                       C.byref(mt)), "voxel_down_sample")
            if mt.value != m.value:
                raise RuntimeError("voxel_down_sample: the pass over the times gave another number of voxels")
            out._tim = t_col[: m.value, 0].contiguous()
        return out

    def remove_statistical_outlier(self, nb_neighbors: int, std_ratio: float):
        ctx = _lib.Context.current()
        torch = _torch()
        n = len(self)
        xyz = self.device_xyz()
        keep = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        idx = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        m = C.c_int64(0)
        ctx.check(ctx.lib.pcr_remove_statistical_outlier(ctx.handle, _ptr(xyz), C.c_int64(n), C.c_int(nb_neighbors),
                                                         C.c_double(std_ratio), _ptr(keep), None, _ptr(idx), C.byref(m)),
                  "remove_statistical_outlier")
        index = idx[: m.value]
        return self.select_by_index(index), index.cpu().numpy().tolist()

    def remove_radius_outlier(self, nb_points: int, radius: float):
        """``PointCloud.remove_radius_outlier``: keeps the points with MORE than ``nb_points`` points of the cloud (themselves included)
        strictly inside ``radius``; returns ``(PointCloud, list_of_indices)`` like the statistical filter, indices ascending."""
        if nb_points < 1 or not (radius > 0.0):
            raise RuntimeError("Illegal input parameters, number of points and radius must be positive")
        ctx = _lib.Context.current()
        torch = _torch()
        n = len(self)
        keep = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        idx = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        m = C.c_int64(0)
        ctx.check(ctx.lib.pcr_remove_radius_outlier(ctx.handle, _ptr(self.device_xyz()), C.c_int64(n), C.c_int(int(nb_points)), C.c_double(radius),
                                                    _ptr(keep), None, _ptr(idx), C.byref(m)), "remove_radius_outlier")
        index = idx[: m.value]
        return self.select_by_index(index), index.cpu().numpy().tolist()

    def cluster_dbscan(self, eps: float, min_points: int, print_progress: bool = False):
        """``PointCloud.cluster_dbscan``: the DBSCAN label of every point, numpy int32 of length n (Open3D returns an ``IntVector`` that users
        wrap in ``np.asarray``); -1 is noise, clusters are numbered from 0 in the order of their first core point.  The labels are Open3D's,
        row by row (the rules: include/pcr_hip.h).  ``print_progress`` is accepted and ignored."""
        return _cluster_dbscan(self, eps, min_points)[0].cpu().numpy()

    def segment_plane(self, distance_threshold: float, ransac_n: int = 3, num_iterations: int = 100, probability: float = 0.99999999, seed=None):
        """``PointCloud.segment_plane``: the dominant plane of the cloud by RANSAC -> ``(plane_model, inliers)``, the plane ``(a, b, c, d)`` of
        ``a x + b y + c z + d = 0`` as numpy float64 ``(4,)`` (refitted over the inliers, unit normal) and the ascending list of the rows within
        ``distance_threshold`` of the best hypothesis.  The answer is that of one sequential loop, deterministic for a ``seed`` (the rules:
        include/pcr_hip.h); ``seed=None`` draws from a process-local counter, as the registration RANSAC does.  No plane found: the zero plane
        and an empty list."""
        plane, index, _ = _segment_plane(self, distance_threshold, ransac_n, num_iterations, probability, seed)
        return plane, index.cpu().numpy().tolist()

    def farthest_point_down_sample(self, num_samples: int, start_index: int = 0) -> "PointCloud":
        """``PointCloud.farthest_point_down_sample``: ``num_samples`` points that cover the cloud evenly, in selection order -- the first is
        ``start_index``, every further one the point farthest from those chosen so far, the smallest index on a tie (the rules:
        include/pcr_hip.h).  Normals, colours and covariances travel with the points.  ``num_samples == 0`` gives an empty cloud,
        ``num_samples == len(self)`` a copy in the input's order; more samples than points, or a ``start_index`` outside the cloud or on a
        row with a non-finite coordinate, raise ``RuntimeError`` like Open3D."""
        n = len(self)
        num_samples, start_index = int(num_samples), int(start_index)
        if num_samples < 0 or num_samples > n:
            raise RuntimeError(f"farthest_point_down_sample: Illegal number of samples: {num_samples}, must be in 0..{n}")
        if num_samples == 0:
            return PointCloud()
        if start_index < 0 or start_index >= n:
            raise RuntimeError(f"farthest_point_down_sample: Illegal start index: {start_index}, must be in 0..{n - 1}")
        if num_samples == n:
            return self.select_by_index(_torch().arange(n, dtype=_torch().int64, device="cuda"))
        return self.select_by_index(_farthest_point_sample(self, num_samples, start_index)[0])

    def normalize_normals(self) -> "PointCloud":
        """``PointCloud.normalize_normals``: every normal divided by its length (float64 on the float32 components, rounded once); a zero
        normal stays zero.  In place; returns the cloud."""
        if self.has_normals():
            ctx = _lib.Context.current()
            ctx.check(ctx.lib.pcr_normalize_normals(ctx.handle, _ptr(self._nrm), C.c_int64(len(self))), "normalize_normals")
        return self

    def _need_normals(self, what):
        if not self.has_normals():
            raise RuntimeError(f"{what}: No normals in the PointCloud. Call estimate_normals() first.")

    def orient_normals_to_align_with_direction(self, orientation_reference=(0.0, 0.0, 1.0)) -> None:
        """``PointCloud.orient_normals_to_align_with_direction``: a normal is negated iff its dot product with ``orientation_reference`` is
        negative; a zero normal becomes the reference (the rules: include/pcr_hip.h).  In place."""
        self._need_normals("orient_normals_to_align_with_direction")
        self._orient_elementwise(0, orientation_reference, "orient_normals_to_align_with_direction")

    def orient_normals_towards_camera_location(self, camera_location=(0.0, 0.0, 0.0)) -> None:
        """``PointCloud.orient_normals_towards_camera_location``: a normal is negated iff it points away from ``camera_location`` as seen from
        its point; a zero normal becomes the unit vector towards the camera (the rules: include/pcr_hip.h).  In place."""
        self._need_normals("orient_normals_towards_camera_location")
        self._orient_elementwise(1, camera_location, "orient_normals_towards_camera_location")

    def _orient_elementwise(self, mode, ref, what):
        ctx = _lib.Context.current()
        r = (C.c_double * 3)(*np.asarray(ref, dtype=np.float64).reshape(3).tolist())
        ctx.check(ctx.lib.pcr_orient_normals(ctx.handle, _ptr(self.device_xyz()), _ptr(self._nrm), C.c_int64(len(self)), C.c_int(mode), r), what)

    def orient_normals_consistent_tangent_plane(self, k: int, lambda_penalty: float = 0.0, cos_alpha_tol: float = 1.0) -> None:
        """``PointCloud.orient_normals_consistent_tangent_plane``: the signs of the normals made consistent by propagation along the minimum
        spanning tree of the Riemannian graph (Euclidean minimum spanning tree plus ``k``-nearest-neighbour graph, weight 1 - |n_i . n_j|) from
        the highest point, which is turned to +z (the rules: include/pcr_hip.h).  The result does not depend on the signs the normals come
        with.  In place; points, colours and covariances are untouched.  Only the defaults of ``lambda_penalty`` and ``cos_alpha_tol`` are
        supported (Open3D's later penalty form is not built)."""
        if float(lambda_penalty) != 0.0:
            raise ValueError("orient_normals_consistent_tangent_plane: lambda_penalty other than 0.0 is not supported")
        if float(cos_alpha_tol) != 1.0:
            raise ValueError("orient_normals_consistent_tangent_plane: cos_alpha_tol other than 1.0 is not supported")
        _orient_normals_tangent_plane(self, k)

    def compute_boundary_points(self, radius: float, max_nn: int = 30, angle_threshold: float = 90.0):
        """``PointCloud.compute_boundary_points`` (Open3D's tensor ``PointCloud``; the angle criterion of PCL's ``BoundaryEstimation``): the
        points on the rim of the sampled surface -- occlusion shadows, the edge of the field of view, holes -> ``(boundary_cloud, mask)``.
        A point is a boundary point when the directions to its Hybrid(``radius``, ``max_nn``) neighbours, projected into its tangent plane,
        leave an angular gap of more than ``angle_threshold`` degrees (the rules: include/pcr_hip.h).  Needs normals, which are taken as
        unit vectors.  Normals, colours and covariances travel with the points, in the input's order; ``mask`` is a ``torch.bool`` tensor
        of length n on the device.  Bad arguments raise ``ValueError`` before anything touches a device."""
        radius, max_nn, angle_threshold = _boundary_args(radius, max_nn, angle_threshold)
        self._need_normals("compute_boundary_points")
        idx, mask, _, _ = _boundary_call(self, radius, max_nn, angle_threshold)
        return self.select_by_index(idx), mask

    def uniform_down_sample(self, every_k_points: int) -> "PointCloud":
        """``PointCloud.uniform_down_sample``: points 0, k, 2k, ... in their order (host side: an index list for ``select_by_index``)."""
        if every_k_points < 1:
            raise RuntimeError("Illegal sample rate, every_k_points must be a positive integer")
        return self.select_by_index(_torch().arange(0, len(self), int(every_k_points), dtype=_torch().int64, device="cuda"))

    def compute_nearest_neighbor_distance(self):
        """``PointCloud.compute_nearest_neighbor_distance`` (ALL_FUNCTIONS.py:1077-1078): per point the distance to its nearest OTHER
        point -- the second entry of a 2-NN search that finds the point itself first, so a duplicated point gets 0 --, float64, length n;
        all 0 with fewer than two points."""
        ctx = _lib.Context.current()
        torch = _torch()
        n = len(self)
        out = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
        ctx.check(ctx.lib.pcr_nearest_neighbor_distance(ctx.handle, _ptr(self.device_xyz()), C.c_int64(n), _ptr(out)), "compute_nearest_neighbor_distance")
        return out[:n].cpu().numpy()

    def compute_point_cloud_distance(self, target: "PointCloud"):
        """``PointCloud.compute_point_cloud_distance``: per point of this cloud the distance to the nearest point of ``target`` (no
        distance cap, unlike ``evaluate_registration``), float64, length n; all 0 against an empty target."""
        return self._point_cloud_distance(target)[0]

    def _point_cloud_distance(self, target: "PointCloud"):
        """-> (distances float64 (n,), nearest target index int32 (n,), -1 against an empty target)."""
        ctx = _lib.Context.current()
        torch = _torch()
        n = len(self)
        dist = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
        near = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
        ctx.check(ctx.lib.pcr_point_cloud_distance(ctx.handle, _ptr(self.device_xyz()), C.c_int64(n), _ptr(target.device_xyz()), C.c_int64(len(target)),
                                                   _ptr(dist), _ptr(near)), "compute_point_cloud_distance")
        return dist[:n].cpu().numpy(), near[:n].cpu().numpy()

    def compute_mean_and_covariance(self):
        """``PointCloud.compute_mean_and_covariance`` (ALL_FUNCTIONS.py:1043): ``(mean (3,), covariance (3, 3))`` in float64, the
        covariance divided by n; an empty cloud gives a zero mean and the identity."""
        ctx = _lib.Context.current()
        mean, cov = (C.c_double * 3)(), (C.c_double * 9)()
        ctx.check(ctx.lib.pcr_mean_and_covariance(ctx.handle, _ptr(self.device_xyz()), C.c_int64(len(self)), mean, cov), "compute_mean_and_covariance")
        return np.array(mean, dtype=np.float64), np.array(cov, dtype=np.float64).reshape(3, 3)

    def get_center(self):
        """``PointCloud.get_center`` (ALL_FUNCTIONS.py:1022, :1035): the mean of the points, float64 (3,)."""
        ctx = _lib.Context.current()
        mean = (C.c_double * 3)()                 # no covariance asked for: one pass over the points
        ctx.check(ctx.lib.pcr_mean_and_covariance(ctx.handle, _ptr(self.device_xyz()), C.c_int64(len(self)), mean, None), "get_center")
        return np.array(mean, dtype=np.float64)

    def select_by_index(self, indices, invert: bool = False) -> "PointCloud":
        torch = _torch()
        idx = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices, dtype=np.int64), device="cuda")
        idx = idx.to(device="cuda", dtype=torch.int64)
        if invert:
            mask = torch.ones(len(self), dtype=torch.bool, device="cuda")
            mask[idx] = False
            idx = torch.nonzero(mask).reshape(-1)
        out = PointCloud()
        out._xyz = self.device_xyz()[idx].contiguous()
        if self.has_normals():
            out._nrm = self._nrm[idx].contiguous()
        if self.has_covariances():
            out._cov = self._cov[idx].contiguous()
        if self.has_colors():
            out._col = self._col[idx].contiguous()
        if self.has_times():
            out._tim = self._tim[idx].contiguous()
        return out

    def random_down_sample(self, sampling_ratio: float, seed=None) -> "PointCloud":
        """``PointCloud.random_down_sample`` (ALL_FUNCTIONS.py:248): a uniformly random subset of ``int(n * sampling_ratio)`` points
        in shuffled order (Open3D shuffles the index list with a ``random_device``-seeded engine and keeps its head; ``seed`` makes
        the draw repeatable here).  Raises like Open3D for a ratio outside (0, 1]."""
        if not (0.0 < sampling_ratio <= 1.0):
            raise RuntimeError("Illegal sampling_ratio, sampling_ratio must be between 0 and 1.")
        torch = _torch()
        n = len(self)
        m = int(n * sampling_ratio)
        g = torch.Generator(device="cuda")
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        return self.select_by_index(torch.randperm(n, device="cuda", generator=g)[:m])

    def estimate_normals(self, search_param=None, fast_normal_computation: bool = True):
        ctx = _lib.Context.current()
        torch = _torch()
        kind, knn, radius = (search_param or KDTreeSearchParamKNN(30))._spec()
        n = len(self)
        out = torch.empty((max(n, 1), 3), dtype=torch.float32, device="cuda")
        prior = self._nrm if self.has_normals() else None
        ctx.check(ctx.lib.pcr_estimate_normals(ctx.handle, _ptr(self.device_xyz()), C.c_int64(n), C.c_int(kind), C.c_int(knn),
                                               C.c_double(radius), _ptr(prior), _ptr(out)), "estimate_normals")
        self._nrm = out[:n].contiguous()

    def estimate_covariances(self, search_param=None):
        ctx = _lib.Context.current()
        torch = _torch()
        kind, knn, radius = (search_param or KDTreeSearchParamKNN(30))._spec()
        n = len(self)
        out = torch.empty((max(n, 1), 6), dtype=torch.float32, device="cuda")
        ctx.check(ctx.lib.pcr_estimate_covariances(ctx.handle, _ptr(self.device_xyz()), C.c_int64(n), C.c_int(kind), C.c_int(knn),
                                                   C.c_double(radius), _ptr(out)), "estimate_covariances")
        self._cov = out[:n].contiguous()

    def deskew(self, motion, reference: float = 1.0, t_begin=None, t_end=None) -> "PointCloud":
        """The cloud with the motion of the sensor during the sweep taken out (``pcr_deskew``; DESKEW of include/pcr_hip.h, KISS-ICP's step):
        ``motion`` is the relative motion ``inv(T_begin) @ T_end`` over the sweep (4x4), a point measured at the fraction
        ``alpha = (time - t_begin) / (t_end - t_begin)`` of it is moved into the sensor frame at the fraction ``reference`` (1.0: the end of
        the sweep, so that the pose a rigid registration then finds is the END pose; 0.5: the middle, as KISS-ICP's earlier releases).
        ``t_begin`` / ``t_end`` default to the cloud's minimum / maximum time; ``alpha`` is not clamped.  Normals are rotated the same way
        (not normalised), times and colours are carried unchanged; covariances are NOT carried (the result has none).  Needs times."""
        fn = "PointCloud.deskew"
        if not self.has_times():
            raise RuntimeError(f"{fn}: the cloud has no times (PointCloud.times)")
        D = np.ascontiguousarray(np.asarray(motion, dtype=np.float64))
        if D.shape != (4, 4):
            raise ValueError(f"{fn}: motion must have shape (4, 4), got {D.shape}")
        t0, t1 = self._time_span(fn, t_begin, t_end)
        ctx = _lib.Context.current()
        torch = _torch()
        n = len(self)
        out = PointCloud()
        out._xyz = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        has_n = self.has_normals()
        if has_n:
            out._nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        ctx.check(ctx.lib.pcr_deskew(ctx.handle, _ptr(self._xyz), _ptr(self._nrm if has_n else None), _ptr(self._tim), C.c_int64(n),
                                     D.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(t0), C.c_double(t1), C.c_double(float(reference)), _ptr(out._xyz),
                                     _ptr(out._nrm if has_n else None)), fn)
        out._tim = self._tim.clone()
        if self.has_colors():
            out._col = self._col.clone()
        return out

    def _time_span(self, fn, t_begin=None, t_end=None):
        """(t0, t1) of the TIMES rule as Python floats: the arguments, or the cloud's minimum / maximum time; ``ValueError`` unless t0 < t1"""
        t0 = float(self._tim.min().item()) if t_begin is None else float(t_begin)
        t1 = float(self._tim.max().item()) if t_end is None else float(t_end)
        if not (np.isfinite(t0) and np.isfinite(t1) and t1 > t0):
            raise ValueError(f"{fn}: t_end must be greater than t_begin and both finite, got {t0!r}, {t1!r}")
        return t0, t1

    def transform(self, T):
        """In place, like Open3D (points, normals; covariances rotated; colours and times untouched)."""
        torch = _torch()
        T = np.asarray(T, dtype=np.float64).reshape(4, 4)
        R = torch.as_tensor(T[:3, :3], dtype=torch.float64, device="cuda")
        t = torch.as_tensor(T[:3, 3], dtype=torch.float64, device="cuda")
        if len(self):
            self._xyz = (self._xyz.double() @ R.T + t).float().contiguous()
            if self.has_normals():
                self._nrm = (self._nrm.double() @ R.T).float().contiguous()
            if self.has_covariances():
                C3 = torch.as_tensor(self.covariances, dtype=torch.float64, device="cuda")
                C3 = R @ C3 @ R.T
                self._cov = torch.stack([C3[:, 0, 0], C3[:, 0, 1], C3[:, 0, 2], C3[:, 1, 1], C3[:, 1, 2], C3[:, 2, 2]], 1).float().contiguous()
        return self


def _cluster_dbscan(cloud: PointCloud, eps: float, min_points: int):
    """``pcr_cluster_dbscan`` -> ``(labels (n,) torch int32 on the device, core mask (n,) torch bool on the device, number of clusters)``:
    the form a pipeline that stays on the device builds on (``functions.remove_small_clusters``)."""
    ctx = _lib.Context.current()
    torch = _torch()
    n = len(cloud)
    labels = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    core = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    m = C.c_int64(0)
    ctx.check(ctx.lib.pcr_cluster_dbscan(ctx.handle, _ptr(cloud.device_xyz()), C.c_int64(n), C.c_double(eps), C.c_int(int(min_points)), _ptr(labels),
                                         _ptr(core), C.byref(m)), "cluster_dbscan")
    return labels[:n], core[:n].bool(), int(m.value)


_plane_seed_counter = [0xD1B54A32D192ED03]


def _segment_plane(cloud: PointCloud, distance_threshold: float, ransac_n: int = 3, num_iterations: int = 100, probability: float = 0.99999999, seed=None):
    """``pcr_segment_plane`` -> ``(plane (4,) numpy float64, inlier rows as a torch int64 tensor on the device (ascending), info)``; ``info`` is a
    dict with ``iterations_run``, ``best_iteration`` (-1: none), ``n_valid``, ``n_inliers``, ``fitness``, ``inlier_rmse`` (the best hypothesis's) and
    ``mask`` (the inlier mask, ``(n,)`` torch bool on the device): the form a pipeline that stays on the device builds on
    (``functions.remove_plane``)."""
    ctx = _lib.Context.current()
    torch = _torch()
    n = len(cloud)
    if seed is None:                       # Open3D draws from std::random_device; here a process-local counter
        _plane_seed_counter[0] = (_plane_seed_counter[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        seed = _plane_seed_counter[0]
    params = _lib.PcrPlaneParams(int(ransac_n), int(num_iterations), float(probability), int(seed) & (2 ** 64 - 1))
    plane = (C.c_double * 4)()
    mask = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    idx = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    m = C.c_int64(0)
    info = _lib.PcrPlaneInfo()
    ctx.check(ctx.lib.pcr_segment_plane(ctx.handle, _ptr(cloud.device_xyz()), C.c_int64(n), C.c_double(distance_threshold), C.byref(params), plane,
                                        _ptr(mask), _ptr(idx), C.byref(m), C.byref(info)), "segment_plane")
    out = {k: getattr(info, k) for k, _ in _lib.PcrPlaneInfo._fields_}
    out["mask"] = mask[:n].bool()
    return np.array(plane, dtype=np.float64), idx[: m.value], out


def _farthest_point_sample(cloud: PointCloud, num_samples: int, start_index: int = 0):
    """``pcr_farthest_point_sample`` -> ``(indices as a torch int64 tensor on the device, in selection order, info)``; ``info`` is a dict with
    ``form`` (0: one launch per step, 1: the persistent launch), ``workgroups``, ``fell_back``, ``cover_dist2``, ``cover_radius`` (its square
    root: the largest distance of any point to the subset) and ``dist2`` (the final squared distance of every row to the subset, ``(n,)``
    torch float64 on the device, -1 on rows with a non-finite coordinate): the form a pipeline that stays on the device builds on."""
    ctx = _lib.Context.current()
    torch = _torch()
    n, k = len(cloud), int(num_samples)
    idx = torch.empty(max(min(k, n), 1), dtype=torch.int64, device="cuda")
    dist2 = torch.full((max(n, 1),), -1.0, dtype=torch.float64, device="cuda")
    info = _lib.PcrFpsInfo()
    ctx.check(ctx.lib.pcr_farthest_point_sample(ctx.handle, _ptr(cloud.device_xyz()), C.c_int64(n), C.c_int64(k), C.c_int64(int(start_index)), _ptr(idx),
                                                _ptr(dist2), C.byref(info)), "farthest_point_down_sample")
    out = {f: getattr(info, f) for f, _ in _lib.PcrFpsInfo._fields_}
    out["cover_radius"] = float(np.sqrt(info.cover_dist2))
    out["dist2"] = dist2[:n]
    return idx[:k], out


def farthest_point_indices(cloud: PointCloud, num_samples: int, start_index: int = 0) -> np.ndarray:
    """The rows ``PointCloud.farthest_point_down_sample`` selects, int64, in selection order: what picks the feature rows of the samples
    (``Feature.select_by_index``) next to ``cloud.select_by_index``."""
    return _farthest_point_sample(cloud, num_samples, start_index)[0].cpu().numpy()


def _orient_normals_tangent_plane(cloud: PointCloud, k: int):
    """``pcr_orient_normals_tangent_plane`` on the cloud's normals, in place -> ``(flipped mask (n,) torch bool on the device, info)``; ``info`` is a
    dict with ``tree_edges`` (the propagation tree, ``(n - 1, 2)`` torch int64 on the device, rows (lo, hi) ascending) and the fields of
    ``pcr_orient_info``: ``emst_rounds``, ``tree_rounds``, ``walked_rows``, ``n_flipped``, ``root``."""
    if not cloud.has_normals():
        raise RuntimeError("orient_normals_consistent_tangent_plane: No normals in the PointCloud. Call estimate_normals() first.")
    ctx = _lib.Context.current()
    torch = _torch()
    n = len(cloud)
    flipped = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    edges = torch.zeros((max(n - 1, 1), 2), dtype=torch.int32, device="cuda")
    info = _lib.PcrOrientInfo()
    ctx.check(ctx.lib.pcr_orient_normals_tangent_plane(ctx.handle, _ptr(cloud.device_xyz()), _ptr(cloud._nrm), C.c_int64(n), C.c_int(int(k)), _ptr(flipped),
                                                       _ptr(edges), C.byref(info)), "orient_normals_consistent_tangent_plane")
    out = {f: getattr(info, f) for f, _ in _lib.PcrOrientInfo._fields_}
    out["tree_edges"] = edges[: max(n - 1, 0)].to(torch.int64)
    return flipped[:n].bool(), out


def euclidean_minimum_spanning_tree(cloud: PointCloud):
    """The Euclidean minimum spanning tree of the cloud (``pcr_euclidean_mst``) -> ``(edges (n - 1, 2) torch int64 on the device, rows (lo, hi)
    ascending by (lo, hi), d2 (n - 1,) torch float64 on the device)``: unique under the order (d^2, lo, hi) of include/pcr_hip.h; what
    single-linkage clustering reads."""
    ctx = _lib.Context.current()
    torch = _torch()
    n = len(cloud)
    edges = torch.zeros((max(n - 1, 1), 2), dtype=torch.int32, device="cuda")
    d2 = torch.zeros(max(n - 1, 1), dtype=torch.float64, device="cuda")
    ctx.check(ctx.lib.pcr_euclidean_mst(ctx.handle, _ptr(cloud.device_xyz()), C.c_int64(n), _ptr(edges), _ptr(d2), None), "euclidean_minimum_spanning_tree")
    return edges[: max(n - 1, 0)].to(torch.int64), d2[: max(n - 1, 0)]


# ---- boundary points --------------------------------------------------------------------------------------------
def _boundary_args(radius, max_nn, angle_threshold):
    """The arguments of the boundary detector as (float, int, float), or ``ValueError``: checked on the host, before a device is touched."""
    radius, max_nn, angle_threshold = float(radius), int(max_nn), float(angle_threshold)
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError(f"compute_boundary_points: radius must be finite and > 0, got {radius}")
    if not 1 <= max_nn <= 200:
        raise ValueError(f"compute_boundary_points: max_nn must be in 1..200, got {max_nn}")
    if not (np.isfinite(angle_threshold) and 0.0 <= angle_threshold <= 360.0):
        raise ValueError(f"compute_boundary_points: angle_threshold must be finite and in [0, 360] degrees, got {angle_threshold}")
    return radius, max_nn, angle_threshold


def _boundary_call(cloud: PointCloud, radius, max_nn, angle_threshold):
    """``pcr_boundary_points`` with every output, all on the device -> ``(indices int64 ascending, mask (n,) bool, max_gap (n,) float64 in
    radians, counts (n,) int32)``."""
    n = len(cloud)
    if n > 0:
        cloud._need_normals("compute_boundary_points")
    ctx = _lib.Context.current()
    torch = _torch()
    mask = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    idx = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    gap = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
    counts = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    m = C.c_int64(0)
    ctx.check(ctx.lib.pcr_boundary_points(ctx.handle, _ptr(cloud.device_xyz()), _ptr(cloud._nrm if n > 0 else None), C.c_int64(n), C.c_double(radius),
                                          C.c_int(max_nn), C.c_double(angle_threshold), _ptr(mask), None, _ptr(idx), C.byref(m), _ptr(gap), _ptr(counts)),
              "compute_boundary_points")
    return idx[: m.value], mask[:n].bool(), gap[:n], counts[:n]


def _boundary_points(cloud: PointCloud, radius, max_nn=30, angle_threshold=90.0):
    """``pcr_boundary_points`` with every output -> ``(indices (torch int64, device, ascending), mask (n,) bool, max_gap (n,) float64 in radians,
    counts (n,) int32: the neighbours each row had)``; the arrays on the host."""
    idx, mask, gap, counts = _boundary_call(cloud, *_boundary_args(radius, max_nn, angle_threshold))
    return idx, mask.cpu().numpy(), gap.cpu().numpy(), counts.cpu().numpy()


def boundary_point_indices(cloud: PointCloud, radius: float, max_nn: int = 30, angle_threshold: float = 90.0) -> np.ndarray:
    """The rows ``PointCloud.compute_boundary_points`` selects, int64, ascending: what takes rim points out of a keypoint list
    (``np.setdiff1d(iss_keypoint_indices(cloud), boundary_point_indices(cloud, radius))``) or marks the rows of a correspondence set whose
    target is a rim point (``np.isin(corres[:, 1], boundary_point_indices(target, radius))``)."""
    return _boundary_call(cloud, *_boundary_args(radius, max_nn, angle_threshold))[0].cpu().numpy()


# ---- o3d.geometry.keypoint ------------------------------------------------------------------------------------
def _iss_keypoints(input: PointCloud, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """``pcr_iss_keypoints`` with every output -> ``(indices (torch int64, device, ascending), mask (n,) bool, saliency (n,) float64,
    eigenvalues (n, 3) float64 descending, (salient radius, non-max radius) used)``; the arrays on the host."""
    ctx = _lib.Context.current()
    torch = _torch()
    n = len(input)
    keep = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    idx = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    sal = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
    eig = torch.zeros((max(n, 1), 3), dtype=torch.float64, device="cuda")
    m = C.c_int64(0)
    radii = (C.c_double * 2)()
    ctx.check(ctx.lib.pcr_iss_keypoints(ctx.handle, _ptr(input.device_xyz()), C.c_int64(n), C.c_double(salient_radius), C.c_double(non_max_radius),
                                        C.c_double(gamma_21), C.c_double(gamma_32), C.c_int(int(min_neighbors)), _ptr(keep), None, _ptr(idx),
                                        C.byref(m), _ptr(sal), _ptr(eig), radii), "compute_iss_keypoints")
    return idx[: m.value], keep[:n].cpu().numpy().astype(bool), sal[:n].cpu().numpy(), eig[:n].cpu().numpy(), (float(radii[0]), float(radii[1]))


def iss_keypoint_indices(input: PointCloud, salient_radius: float = 0.0, non_max_radius: float = 0.0, gamma_21: float = 0.975,
                         gamma_32: float = 0.975, min_neighbors: int = 5) -> np.ndarray:
    """The rows ``compute_iss_keypoints`` selects, int64, ascending: what picks the feature rows of the keypoints
    (``Feature.select_by_index``) next to ``input.select_by_index``."""
    return _iss_keypoints(input, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)[0].cpu().numpy()


def compute_iss_keypoints(input: PointCloud, salient_radius: float = 0.0, non_max_radius: float = 0.0, gamma_21: float = 0.975,
                          gamma_32: float = 0.975, min_neighbors: int = 5) -> PointCloud:
    """``o3d.geometry.keypoint.compute_iss_keypoints``: the ISS keypoints of ``input`` as a cloud (normals, colours and covariances
    travel with the points, in the input's order).  With either radius 0 both come from the cloud's resolution (6 x and 4 x the mean
    nearest-neighbour distance).  A neighbour suppresses a point only when its saliency is larger by more than
    ``1e-11 salient_radius**2`` (include/pcr_hip.h): points that share one neighbourhood are all kept, as Open3D keeps them on an exact tie."""
    return input.select_by_index(_iss_keypoints(input, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)[0])
