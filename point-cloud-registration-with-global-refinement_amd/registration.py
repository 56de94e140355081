"""Stand-ins for ``o3d.pipelines.registration`` as used on the reference's hot path.

``registration_generalized_icp`` ALL_FUNCTIONS.py:304-311 / 2_MGICP...py:155-162; ``registration_icp`` with
``TransformationEstimationForGeneralizedICP`` :220-226; ``L1Loss`` :284, ``GMLoss`` :219;
``ICPConvergenceCriteria`` :309-311; ``evaluate_registration`` :809-820;
``get_information_matrix_from_point_clouds`` :327-331; ``compute_fpfh_feature`` :186-187;
``FastGlobalRegistrationOption`` :189-196; ``registration_fgr_based_on_feature_matching`` :198-202.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .geometry import PointCloud, _ptr, _torch


class RobustKernel:
    kind = _lib.LOSS_L2
    k = 1.0


class L2Loss(RobustKernel):
    pass


class L1Loss(RobustKernel):
    kind = _lib.LOSS_L1


class GMLoss(RobustKernel):
    kind = _lib.LOSS_GM

    def __init__(self, k: float = 1.0):
        self.k = float(k)


class TransformationEstimation:
    """Open3D's ``TransformationEstimation`` methods on a correspondence list the caller holds (``pcr_estimation_compute_transformation`` /
    ``pcr_estimation_compute_rmse``, include/pcr_hip.h): ``corres`` is (C, 2) rows of (source index, target index), a device tensor or
    anything ``np.asarray`` turns into integers.  Every row counts (no distance test); an empty list gives the identity and 0."""

    def _estimation(self) -> _lib.PcrEstimation:
        raise RuntimeError(f"{type(self).__name__} is not implemented on the MI355X path")

    def compute_transformation(self, source, target, corres) -> np.ndarray:
        """The estimator's one update from the identity over the rows of ``corres``: a 4x4 float64 array (ALL_FUNCTIONS.py:438-439)."""
        T = np.zeros(16, dtype=np.float64)
        _estimation_call(self, "compute_transformation", source, target, corres, T)
        return T.reshape(4, 4)

    def compute_rmse(self, source, target, corres) -> float:
        """The estimator's error over the rows of ``corres``: Euclidean for point-to-point and GICP, along the target normal for point-to-plane."""
        out = np.zeros(1, dtype=np.float64)
        _estimation_call(self, "compute_rmse", source, target, corres, out)
        return float(out[0])


class TransformationEstimationForGeneralizedICP(TransformationEstimation):
    def __init__(self, kernel: RobustKernel | None = None, epsilon: float = 1e-3):
        self.kernel = kernel if kernel is not None else L2Loss()
        self.epsilon = float(epsilon)

    def _estimation(self):
        return _lib.PcrEstimation(_lib.EST_GENERALIZED_ICP, 0, int(self.kernel.kind), float(self.kernel.k), float(self.epsilon))


class TransformationEstimationPointToPoint(TransformationEstimation):
    """Open3D's default ``registration_icp`` estimator: the Umeyama fit of the correspondences (with a uniform scale when
    ``with_scaling``).  ``kernel`` is read by ``registration_point_map`` alone, whose point-to-point update is the weighted Gauss-Newton
    form; the Umeyama fit of ``registration_icp`` has no weights and ignores it."""

    def __init__(self, with_scaling: bool = False, kernel: RobustKernel | None = None):
        self.with_scaling = bool(with_scaling)
        self.kernel = kernel if kernel is not None else L2Loss()

    def _estimation(self):
        return _lib.PcrEstimation(_lib.EST_POINT_TO_POINT, int(self.with_scaling), _lib.LOSS_L2, 1.0, 1e-3)


class TransformationEstimationPointToPlane(TransformationEstimation):
    """Point-to-plane ICP over the target's normals, robustly weighted by ``kernel`` (L2, L1 or GM)."""

    def __init__(self, kernel: RobustKernel | None = None):
        self.kernel = kernel if kernel is not None else L2Loss()

    def _estimation(self):
        return _lib.PcrEstimation(_lib.EST_POINT_TO_PLANE, 0, int(self.kernel.kind), float(self.kernel.k), 1e-3)


class TransformationEstimationForColoredICP(TransformationEstimation):
    """Colored ICP (Park, Zhou, Koltun, ICCV 2017): a point-to-plane term weighted ``lambda_geometric`` and a photometric term over the
    target's colour gradients weighted ``1 - lambda_geometric``, both robustly weighted by ``kernel``.  As in Open3D a ``lambda_geometric``
    outside [0, 1] is reset to 0.968."""

    def __init__(self, lambda_geometric: float = 0.968, kernel: RobustKernel | None = None):
        lam = float(lambda_geometric)
        self.lambda_geometric = lam if 0.0 <= lam <= 1.0 else 0.968
        self.kernel = kernel if kernel is not None else L2Loss()

    # Open3D's own methods need the gradient-carrying target that only registration_colored_icp builds
    def compute_transformation(self, source, target, corres):
        raise RuntimeError("TransformationEstimationForColoredICP.compute_transformation is not implemented on the MI355X path")

    def compute_rmse(self, source, target, corres):
        raise RuntimeError("TransformationEstimationForColoredICP.compute_rmse is not implemented on the MI355X path")


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, max_iteration: int = 30):
        self.relative_fitness = float(relative_fitness)
        self.relative_rmse = float(relative_rmse)
        self.max_iteration = int(max_iteration)


class FastGlobalRegistrationOption:
    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=False,
                 maximum_correspondence_distance=0.025, iteration_number=64, tuple_scale=0.95,
                 maximum_tuple_count=1000, tuple_test=True, seed=None):
        self.division_factor = float(division_factor)
        self.use_absolute_scale = bool(use_absolute_scale)
        self.decrease_mu = bool(decrease_mu)
        self.maximum_correspondence_distance = float(maximum_correspondence_distance)
        self.iteration_number = int(iteration_number)
        self.tuple_scale = float(tuple_scale)
        self.maximum_tuple_count = int(maximum_tuple_count)
        self.tuple_test = bool(tuple_test)
        self.seed = seed


class RegistrationResult:
    """``transformation`` (4x4 float64, source->target), ``fitness``, ``inlier_rmse``, ``correspondence_set``."""

    def __init__(self, transformation=None, fitness=0.0, inlier_rmse=0.0, correspondence_set=None, iterations=0,
                 converged=False, scales=None):
        self.transformation = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64).reshape(4, 4)
        self.fitness = float(fitness)
        self.inlier_rmse = float(inlier_rmse)
        self._corr = correspondence_set           # torch int32 (K,2) on device, materialised lazily
        self.iterations = int(iterations)
        self.converged = bool(converged)
        self.scales = scales or []

    @property
    def correspondence_set(self):
        if self._corr is None:
            return np.zeros((0, 2), np.int32)
        if not isinstance(self._corr, np.ndarray):
            self._corr = self._corr.cpu().numpy()
        return self._corr

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, "
                f"and correspondence_set size of {len(self.correspondence_set)}")


class Feature:
    """``o3d.pipelines.registration.Feature``: ``data`` is (dimension, N) float64 like Open3D's."""

    def __init__(self, dev):
        self._dev = dev            # torch (N,33) float32 cuda

    @property
    def data(self):
        return self._dev.detach().cpu().numpy().astype(np.float64).T

    def dimension(self):
        return int(self._dev.shape[1])

    def num(self):
        return int(self._dev.shape[0])

    def select_by_index(self, indices, invert: bool = False) -> "Feature":
        """``Feature.select_by_index`` (Open3D >= 0.18): the feature rows of the points ``indices``, in that order -- a gather on the
        device, like ``PointCloud.select_by_index``; ``invert`` keeps the other rows in their order."""
        torch = _torch()
        idx = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices, dtype=np.int64), device="cuda")
        idx = idx.to(device="cuda", dtype=torch.int64).reshape(-1)
        if invert:
            mask = torch.ones(self.num(), dtype=torch.bool, device="cuda")
            mask[idx] = False
            idx = torch.nonzero(mask).reshape(-1)
        return Feature(self._dev[idx].contiguous())


def _params(estimation, criteria) -> _lib.PcrGicpParams:
    return _lib.PcrGicpParams(int(estimation.kernel.kind), float(estimation.kernel.k), float(estimation.epsilon),
                              float(criteria.relative_fitness), float(criteria.relative_rmse), int(criteria.max_iteration))


def _result(r: _lib.PcrResult, corr=None, scales=None) -> RegistrationResult:
    if corr is not None:
        corr = corr[: r.n_correspondences]
    return RegistrationResult(np.array(r.transformation, dtype=np.float64).reshape(4, 4), r.fitness, r.inlier_rmse, corr,
                              r.iterations, bool(r.converged), scales)


def _T(init):
    T = np.ascontiguousarray(np.asarray(init, dtype=np.float64).reshape(4, 4))
    return T, T.ctypes.data_as(C.POINTER(C.c_double))


def _corres_device(fn: str, corres, ns: int, nt: int):
    """A caller's correspondence list as a contiguous device int32 tensor (C, 2): a torch tensor, or anything ``np.asarray`` turns into
    integers (the reference passes a float array of integral values, ALL_FUNCTIONS.py:433-435).  A wrong shape or a row outside the two
    clouds raises ``RuntimeError`` before the library is called; a host list is checked on the host, before anything touches a device."""
    torch = _torch()
    if isinstance(corres, torch.Tensor):
        if corres.dim() == 2 and corres.shape[1] != 2:
            raise RuntimeError(f"{fn}: corres must have shape (C, 2), got {tuple(corres.shape)}")
        cd = corres.to(device="cuda", dtype=torch.int32).reshape(-1, 2).contiguous()
        lo, hi = (cd.min(0).values.tolist(), cd.max(0).values.tolist()) if cd.shape[0] else ((0, 0), (-1, -1))
    else:
        a = np.asarray(corres, dtype=np.int64)
        if a.ndim == 2 and a.shape[1] != 2:
            raise RuntimeError(f"{fn}: corres must have shape (C, 2), got {a.shape}")
        a = np.ascontiguousarray(a.reshape(-1, 2))
        lo, hi = (a.min(0).tolist(), a.max(0).tolist()) if a.shape[0] else ((0, 0), (-1, -1))
        cd = None
    if hi[0] >= lo[0] and (ns == 0 or nt == 0 or lo[0] < 0 or lo[1] < 0 or hi[0] >= ns or hi[1] >= nt):
        raise RuntimeError(f"{fn}: correspondence index out of range")
    return cd if cd is not None else torch.from_numpy(a.astype(np.int32)).cuda()


def _estimation_call(estimation, what: str, source: PointCloud, target: PointCloud, corres, out: np.ndarray) -> None:
    fn = f"{type(estimation).__name__}.{what}"
    e = estimation._estimation()
    ns, nt = len(source), len(target)
    cd = _corres_device(fn, corres, ns, nt)
    ctx = _lib.Context.current()
    call = getattr(ctx.lib, "pcr_estimation_" + what)
    ctx.check(call(ctx.handle, C.byref(e), _ptr(source.device_xyz()), _ptr(source.device_normals() if source.has_normals() else None),
                   _ptr(source._cov if source.has_covariances() else None), C.c_int64(ns), _ptr(target.device_xyz()),
                   _ptr(target.device_normals() if target.has_normals() else None), _ptr(target._cov if target.has_covariances() else None),
                   C.c_int64(nt), _ptr(cd), C.c_int64(int(cd.shape[0])), out.ctypes.data_as(C.POINTER(C.c_double))), fn)


def _ensure_gicp_normals(pc: PointCloud):
    """Open3D InitializePointCloudForGeneralizedICP: clouds without covariances and without normals get
    ``estimate_normals()`` with the default search (KNN 30) first."""
    if not pc.has_normals():
        pc = pc.__deepcopy__({})
        pc.estimate_normals()
    return pc


def registration_generalized_icp(source: PointCloud, target: PointCloud, max_correspondence_distance: float,
                                 init=np.eye(4), estimation_method=None, criteria=None) -> RegistrationResult:
    estimation = estimation_method or TransformationEstimationForGeneralizedICP()
    criteria = criteria or ICPConvergenceCriteria()
    ctx = _lib.Context.current()
    torch = _torch()
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    ns, nt = len(source), len(target)
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res = _lib.PcrResult()
    T, Tp = _T(init)
    p = _params(estimation, criteria)
    if source.has_covariances() and target.has_covariances():
        # Open3D InitializePointCloudForGeneralizedICP: clouds that already carry covariances keep them untouched
        ctx.check(ctx.lib.pcr_registration_generalized_icp_cov(
            ctx.handle, _ptr(source.device_xyz()), _ptr(source._cov), C.c_int64(ns), _ptr(target.device_xyz()), _ptr(target._cov),
            C.c_int64(nt), C.c_double(max_correspondence_distance), Tp, C.byref(p), C.byref(res), _ptr(corr)),
            "registration_generalized_icp")
        return _result(res, corr)
    if source.has_covariances() != target.has_covariances():
        raise RuntimeError("registration_generalized_icp: either both clouds carry covariances or neither (mixed case not on the MI355X path)")
    source = _ensure_gicp_normals(source); target = _ensure_gicp_normals(target)
    ctx.check(ctx.lib.pcr_registration_generalized_icp(
        ctx.handle, _ptr(source.device_xyz()), _ptr(source.device_normals()), C.c_int64(ns), _ptr(target.device_xyz()),
        _ptr(target.device_normals()), C.c_int64(nt), C.c_double(max_correspondence_distance), Tp, C.byref(p), C.byref(res),
        _ptr(corr)), "registration_generalized_icp")
    return _result(res, corr)


def registration_icp(source, target, max_correspondence_distance, init=np.eye(4), estimation_method=None, criteria=None):
    """Open3D ``registration_icp``: ``estimation_method`` None is ``TransformationEstimationPointToPoint(False)``, Open3D's default;
    the GICP estimator (ALL_FUNCTIONS.py:220-226) runs ``registration_generalized_icp``; point-to-point and point-to-plane run
    ``pcr_registration_icp``, the same device loop with their own update."""
    if isinstance(estimation_method, TransformationEstimationForGeneralizedICP):
        return registration_generalized_icp(source, target, max_correspondence_distance, init, estimation_method, criteria)
    if isinstance(estimation_method, TransformationEstimationForColoredICP):
        return registration_colored_icp(source, target, max_correspondence_distance, init, estimation_method, criteria)
    estimation = TransformationEstimationPointToPoint() if estimation_method is None else estimation_method
    if isinstance(estimation, TransformationEstimationPointToPoint):
        p = _lib.PcrIcpParams(_lib.ICP_POINT_TO_POINT, int(estimation.with_scaling), _lib.LOSS_L2, 1.0, 0.0, 0.0, 0)
    elif isinstance(estimation, TransformationEstimationPointToPlane):
        p = _lib.PcrIcpParams(_lib.ICP_POINT_TO_PLANE, 0, int(estimation.kernel.kind), float(estimation.kernel.k), 0.0, 0.0, 0)
    else:
        raise RuntimeError(f"registration_icp: {type(estimation).__name__} is not implemented on the MI355X path")
    criteria = criteria or ICPConvergenceCriteria()
    p.relative_fitness, p.relative_rmse, p.max_iteration = float(criteria.relative_fitness), float(criteria.relative_rmse), int(criteria.max_iteration)
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    p2pl = p.estimation == _lib.ICP_POINT_TO_PLANE
    if p2pl and not target.has_normals():
        raise RuntimeError("TransformationEstimationPointToPlane and TransformationEstimationColoredICP require pre-computed normal vectors for target PointCloud.")
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res = _lib.PcrResult()
    T, Tp = _T(init)
    ctx.check(ctx.lib.pcr_registration_icp(
        ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), _ptr(target.device_xyz()), _ptr(target.device_normals() if target.has_normals() else None),
        C.c_int64(nt), C.c_double(max_correspondence_distance), Tp, C.byref(p), C.byref(res), _ptr(corr)), "registration_icp")
    return _result(res, corr)


def registration_colored_icp(source, target, max_correspondence_distance, init=np.eye(4), estimation_method=None, criteria=None):
    """Open3D ``registration_colored_icp`` (``pcr_registration_colored_icp``, include/pcr_hip.h): the target's colour gradients over
    ``KDTreeSearchParamHybrid(2 * max_correspondence_distance, 30)``, then the loop of ``registration_icp`` with the two-row update of
    ``TransformationEstimationForColoredICP``.  ``fitness`` and ``inlier_rmse`` are the geometric ones of the correspondence search."""
    estimation = TransformationEstimationForColoredICP() if estimation_method is None else estimation_method
    if not isinstance(estimation, TransformationEstimationForColoredICP):
        raise RuntimeError(f"registration_colored_icp: {type(estimation).__name__} is not TransformationEstimationForColoredICP")
    criteria = criteria or ICPConvergenceCriteria()
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    ns, nt = len(source), len(target)
    if nt and not target.has_normals():
        raise RuntimeError("ColoredICP requires pre-computed normal vectors for target PointCloud.")
    if ns and not source.has_colors():
        raise RuntimeError("ColoredICP requires pre-computed colors for source PointCloud.")
    if nt and not target.has_colors():
        raise RuntimeError("ColoredICP requires pre-computed colors for target PointCloud.")
    p = _lib.PcrColoredIcpParams(float(estimation.lambda_geometric), int(estimation.kernel.kind), float(estimation.kernel.k),
                                 float(criteria.relative_fitness), float(criteria.relative_rmse), int(criteria.max_iteration))
    ctx = _lib.Context.current()
    torch = _torch()
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res = _lib.PcrResult()
    T, Tp = _T(init)
    ctx.check(ctx.lib.pcr_registration_colored_icp(
        ctx.handle, _ptr(source.device_xyz()), _ptr(source.device_colors() if ns else None), C.c_int64(ns), _ptr(target.device_xyz()),
        _ptr(target.device_normals() if nt else None), _ptr(target.device_colors() if nt else None), C.c_int64(nt),
        C.c_double(max_correspondence_distance), Tp, C.byref(p), C.byref(res), _ptr(corr)), "registration_colored_icp")
    return _result(res, corr)


def color_gradient(cloud: PointCloud, search_param) -> np.ndarray:
    """The colour gradients colored ICP takes of a target cloud (``pcr_color_gradient``): (N, 3) float32, one row per point, over the
    neighbours of ``search_param`` (KNN or Hybrid, at most 32 neighbours).  The cloud needs normals and colours."""
    if not cloud.has_normals() or not cloud.has_colors():
        raise RuntimeError("color_gradient: the cloud needs normals and colors")
    ctx = _lib.Context.current()
    torch = _torch()
    kind, knn, radius = search_param._spec()
    n = len(cloud)
    out = torch.zeros((max(n, 1), 3), dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.pcr_color_gradient(ctx.handle, _ptr(cloud.device_xyz()), _ptr(cloud.device_normals()), _ptr(cloud.device_colors()), C.c_int64(n),
                                         C.c_int(kind), C.c_int(knn), C.c_double(radius), _ptr(out)), "color_gradient")
    return out[:n].cpu().numpy()


# ---- voxelized GICP on a reusable voxel covariance map (pcr_voxel_map_*, pcr_registration_voxelized_gicp; the rule: include/pcr_hip.h)
def _check_vgicp_rule(fn: str, neighborhood, min_points_per_voxel):
    if neighborhood not in (1, 7, 27):
        raise ValueError(f"{fn}: neighborhood must be 1, 7 or 27, got {neighborhood!r}")
    if not isinstance(min_points_per_voxel, (int, np.integer)) or min_points_per_voxel < 1:
        raise ValueError(f"{fn}: min_points_per_voxel must be an integer >= 1, got {min_points_per_voxel!r}")


def _check_voxel_size(fn: str, voxel_size):
    try:
        v = float(voxel_size)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: voxel_size must be a number greater than 0, got {voxel_size!r}") from None
    if not (v > 0.0) or not np.isfinite(v):
        raise ValueError(f"{fn}: voxel_size must be a finite number greater than 0, got {voxel_size!r}")
    return v


class _GrowingVoxelMap:
    """What ``VoxelCovarianceMap`` and ``NormalDistributionsMap`` are alike: a handle to a map on the device with one row per occupied cell of
    a fixed grid, which ``insert``, ``merge`` and ``remove_far`` replace as a whole.  A subclass names its entry points (``_C``, the prefix of
    ``<_C>_create`` ... ``<_C>_read``), the name its error texts carry (``_NAME``) and its columns in the argument order of ``<_C>_read``
    (``_COLUMNS``: name -> (width or None, dtype)); it keeps its constructor, ``on_grid``, ``insert``, ``grid_min``, ``origin`` and what only
    it can do."""

    _handle = None
    _C = _NAME = None
    _COLUMNS = {}

    @staticmethod
    def centered_grid_min(point, voxel_size) -> np.ndarray:
        """``floor(point / voxel_size) * voxel_size - 2^20 * voxel_size`` per axis (float64): the ``grid_min`` of a grid with ``point`` in the
        middle of its 2^21 cells per axis, so the map can grow by 2^20 cells in every direction."""
        v = _check_voxel_size("VoxelCovarianceMap.centered_grid_min", voxel_size)
        p = np.asarray(point, np.float64).reshape(-1)
        if p.shape != (3,) or not np.isfinite(p).all():
            raise ValueError(f"VoxelCovarianceMap.centered_grid_min: point must be three finite numbers, got {point!r}")
        return np.floor(p / v) * v - float(1 << 20) * v

    @staticmethod
    def _pose(fn: str, transformation):
        """(array kept alive, pointer) of an optional 4x4 pose; ``None`` is the NULL pointer (the identity)"""
        if transformation is None:
            return None, None
        T = np.asarray(transformation, dtype=np.float64)
        if T.shape != (4, 4):
            raise ValueError(f"{fn}: transformation must have shape (4, 4), got {T.shape}")
        return _T(T)

    @classmethod
    def _placement(cls, grid_min, transformation):
        """(grid_min as three float64 or None, pose kept alive, pose pointer) of ``on_grid``: a pose needs a ``grid_min``"""
        fn = cls._NAME
        T, Tp = cls._pose(fn, transformation)
        g = None
        if grid_min is not None:
            g = np.ascontiguousarray(np.asarray(grid_min, np.float64).reshape(-1))
            if g.shape != (3,):
                raise ValueError(f"{fn}: grid_min must hold three numbers, got {grid_min!r}")
        if g is None and T is not None:
            raise ValueError(f"{fn}: a transformation needs a grid_min (the placed target's minimum is not known before the call)")
        return g, T, Tp

    def _call(self, ctx, name):
        return getattr(ctx.lib, f"{self._C}_{name}")

    def _adopt(self, ctx, handle):
        self._handle = handle
        self._lib = ctx.lib
        self._refresh()

    def _refresh(self):
        m = C.c_int64(0)
        getattr(self._lib, self._C + "_size")(self._handle, C.byref(m))
        self._cells = int(m.value)

    def _open(self):
        if self._handle is None:
            raise RuntimeError(f"{self._NAME}: the map is closed")
        return self._handle

    def close(self):
        """Destroy the map (waits for the device)."""
        h, self._handle = self._handle, None
        if h is not None and h.value:
            getattr(self._lib, self._C + "_destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __len__(self):
        self._open()
        return self._cells

    @property
    def voxel_size(self) -> float:
        self._open()
        return self._voxel_size

    def merge(self, other):
        """Add the cells of ``other``, a map of the same class on the same grid -- and, for a ``NormalDistributionsMap``, with the same
        ``min_points_per_voxel`` and ``eigenvalue_ratio`` -- (``pcr_voxel_map_merge`` / ``pcr_ndt_map_merge``); ``other`` is unchanged.  A cell
        in both gets the sum of the counts and the count-weighted means: of the nine channels in a ``VoxelCovarianceMap``; of the mean, with
        the covariance about that mean and a recomputed ``A_v``, in a ``NormalDistributionsMap``."""
        fn = self._NAME + ".merge"
        h = self._open()
        if not isinstance(other, _GrowingVoxelMap) or other._C != self._C:
            raise TypeError(f"{fn}: other must be a {self._NAME}, got {type(other).__name__}")
        ho = other._open()
        ctx = _lib.Context.current()
        ctx.check(self._call(ctx, "merge")(ctx.handle, h, ho), fn)
        self._refresh()

    def remove_far(self, center, max_distance) -> int:
        """Drop every cell whose mean is not closer to ``center`` than ``max_distance`` (``pcr_voxel_map_remove_far`` /
        ``pcr_ndt_map_remove_far``; d^2 < r^2 keeps) and return the number of rows removed.  A call that would keep nothing raises the
        library's error and leaves the map as it was."""
        fn = self._NAME + ".remove_far"
        h = self._open()
        c = np.ascontiguousarray(np.asarray(center, np.float64).reshape(-1))
        if c.shape != (3,):
            raise ValueError(f"{fn}: center must hold three numbers, got {center!r}")
        try:
            r = float(max_distance)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: max_distance must be a number greater than 0, got {max_distance!r}") from None
        if not np.isfinite(r) or not (r > 0.0):
            raise ValueError(f"{fn}: max_distance must be a finite number greater than 0, got {max_distance!r}")
        ctx = _lib.Context.current()
        removed = C.c_int64(0)
        ctx.check(self._call(ctx, "remove_far")(ctx.handle, h, c.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(r), C.byref(removed)), fn)
        self._refresh()
        return int(removed.value)

    def _read(self, what: str):
        """one column as a device tensor"""
        h = self._open()
        ctx = _lib.Context.current()
        torch = _torch()
        cols, dtype = self._COLUMNS[what]
        t = torch.empty((self._cells,) if cols is None else (self._cells, cols), dtype=getattr(torch, dtype), device="cuda")
        args = [_ptr(t if k == what else None) for k in self._COLUMNS]
        ctx.check(self._call(ctx, "read")(ctx.handle, h, *args), f"{self._NAME}.{what}")
        return t

    @property
    def cells(self) -> np.ndarray:
        """(cells, 3) int32: the cell index (ix, iy, iz) of every row"""
        return self._read("cells").cpu().numpy()

    @property
    def counts(self) -> np.ndarray:
        """(cells,) int32: the member count N_v"""
        return self._read("counts").cpu().numpy()

    @property
    def points(self) -> np.ndarray:
        """(cells, 3) float32: the mean point of every cell"""
        return self._read("points").cpu().numpy()

    @property
    def covariances(self) -> np.ndarray:
        """(cells, 6) float32, xx,xy,xz,yy,yz,zz: in a ``VoxelCovarianceMap`` the mean covariance of every cell, in a
        ``NormalDistributionsMap`` C_v, the mean of the members' products about the cell mean"""
        return self._read("covariances").cpu().numpy()

    def to_point_cloud(self) -> PointCloud:
        """The cells' means as a cloud that carries the cells' covariances."""
        pc = PointCloud()
        pc._xyz = self._read("points")
        pc._cov = self._read("covariances")
        return pc


class VoxelCovarianceMap(_GrowingVoxelMap):
    """The target of voxelized GICP (Koide et al., ICRA 2021): per occupied cell of ``voxel_down_sample``'s grid the member count, the mean
    point and the mean covariance, behind a cell hash on the device.  Built once from ``target.covariances`` (or, without them, from its
    normals with ``epsilon`` as the GICP estimator forms them) and good for any number of registrations until ``close()``.  Rows are in
    Morton order of the cell index, the order in which ``voxel_down_sample`` lists its points.

    ``VoxelCovarianceMap(target, voxel_size)`` takes the grid from the target's own minimum, so nothing below that minimum can ever be added.
    A map that will grow is made by ``VoxelCovarianceMap.on_grid(target, voxel_size, grid_min=centered_grid_min(point, voxel_size))``, whose
    grid has ``point`` in its middle; then ``insert`` adds a scan at a pose, ``merge`` adds another map of the same grid and ``remove_far``
    drops the cells far from a point (the GRID / MERGE / INSERT / REMOVE_FAR rules of include/pcr_hip.h).  Each of them replaces the rows as a
    whole: row indices of an earlier ``correspondence_set`` are stale afterwards, and no other call may use the map while one runs."""

    _C, _NAME = "pcr_voxel_map", "VoxelCovarianceMap"
    _COLUMNS = {"cells": (3, "int32"), "counts": (None, "int32"), "points": (3, "float32"), "covariances": (6, "float32")}

    def __init__(self, target: PointCloud, voxel_size: float, epsilon: float = 1e-3):
        self._create(target, voxel_size, epsilon, None, None)

    @classmethod
    def on_grid(cls, target: PointCloud, voxel_size: float, epsilon: float = 1e-3, grid_min=None, transformation=None):
        """The map of ``target`` placed at ``transformation`` (4x4; ``None``: as it lies) on the grid whose origin is
        ``grid_min - voxel_size / 2`` (``pcr_voxel_map_create_on_grid``).  With both ``None`` this is
        ``VoxelCovarianceMap(target, voxel_size, epsilon)``, through the same call and with the same bits; a pose needs a ``grid_min``.  A point outside
        the grid's 2^21 cells per axis -- below ``grid_min - voxel_size / 2`` too -- raises the library's error."""
        m = cls.__new__(cls)
        m._create(target, voxel_size, epsilon, grid_min, transformation)
        return m

    @staticmethod
    def _cloud_arrays(fn: str, cloud, what: str = "cloud"):
        """(covariances or None, normals or None) of a cloud that goes into a map: exactly one is given"""
        if not isinstance(cloud, PointCloud) or len(cloud) == 0:
            raise RuntimeError(f"{fn}: the {what} must be a PointCloud with at least one point")
        cov = cloud._cov if cloud.has_covariances() else None
        nrm = cloud._nrm if cov is None and cloud.has_normals() else None
        if cov is None and nrm is None:
            raise RuntimeError(f"{fn}: the {what} has neither covariances nor normals")
        return cov, nrm

    def _create(self, target, voxel_size, epsilon, grid_min, transformation):
        fn = "VoxelCovarianceMap"
        self._voxel_size = _check_voxel_size(fn, voxel_size)
        self.epsilon = float(epsilon)
        if not np.isfinite(self.epsilon):
            raise ValueError(f"VoxelCovarianceMap: epsilon must be finite, got {epsilon!r}")
        cov, nrm = self._cloud_arrays(fn, target, "target")
        g, T, Tp = self._placement(grid_min, transformation)
        ctx = _lib.Context.current()
        h = C.c_void_p()
        if g is None:
            ctx.check(ctx.lib.pcr_voxel_map_create(ctx.handle, _ptr(target.device_xyz()), _ptr(cov), _ptr(nrm), C.c_int64(len(target)),
                                                   C.c_double(self._voxel_size), C.c_double(self.epsilon), C.byref(h)), fn)
        else:
            ctx.check(ctx.lib.pcr_voxel_map_create_on_grid(ctx.handle, _ptr(target.device_xyz()), _ptr(cov), _ptr(nrm), C.c_int64(len(target)),
                                                           C.c_double(self._voxel_size), C.c_double(self.epsilon), g.ctypes.data_as(C.POINTER(C.c_double)),
                                                           Tp, C.byref(h)), fn)
        self._adopt(ctx, h)

    def _grid(self):
        h = self._open()
        g, o, v = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(0)
        self._lib.pcr_voxel_map_grid(h, g, o, C.byref(v))
        return np.array(g, np.float64), np.array(o, np.float64), float(v.value)

    @property
    def grid_min(self) -> np.ndarray:
        """(3,) float64: g of the GRID rule; for a map made without ``grid_min`` the target's minimum"""
        return self._grid()[0]

    @property
    def origin(self) -> np.ndarray:
        """(3,) float64: ``grid_min - voxel_size / 2``, the corner of cell (0, 0, 0)"""
        return self._grid()[1]

    def insert(self, cloud: PointCloud, transformation=np.eye(4)):
        """Add ``cloud`` placed at ``transformation`` (``pcr_voxel_map_insert``): the map becomes MERGE(map, the map of the placed cloud on this
        grid).  The cloud carries covariances or normals, as the target of the constructor.  A point outside the grid raises the library's
        error and leaves the map as it was."""
        fn = "VoxelCovarianceMap.insert"
        h = self._open()
        cov, nrm = self._cloud_arrays(fn, cloud)
        T, Tp = self._pose(fn, np.eye(4) if transformation is None else transformation)
        ctx = _lib.Context.current()
        ctx.check(ctx.lib.pcr_voxel_map_insert(ctx.handle, h, _ptr(cloud.device_xyz()), _ptr(cov), _ptr(nrm), C.c_int64(len(cloud)), C.c_double(self.epsilon), Tp), fn)
        self._refresh()

    def correspondences(self, source: PointCloud, T=np.eye(4), neighborhood: int = 1, min_points_per_voxel: int = 1):
        """The rows (source index, map row) of the rule at the pose ``T``, ordered by source index and then by the neighbourhood's offset
        order: a device tensor (rows, 2) int32."""
        _check_vgicp_rule("VoxelCovarianceMap.correspondences", neighborhood, min_points_per_voxel)
        h = self._open()
        ctx = _lib.Context.current()
        torch = _torch()
        ns = len(source)
        rows = torch.empty((max(ns, 1) * int(neighborhood), 2), dtype=torch.int32, device="cuda")
        n = C.c_int64(0)
        _, Tp = _T(T)
        ctx.check(ctx.lib.pcr_voxel_map_correspondences(ctx.handle, h, _ptr(source.device_xyz()), C.c_int64(ns), Tp, C.c_int(int(neighborhood)),
                                                        C.c_int(int(min_points_per_voxel)), _ptr(rows), C.byref(n)), "VoxelCovarianceMap.correspondences")
        return rows[: n.value]


def registration_voxelized_gicp(source: PointCloud, target_or_map, voxel_size=None, init=np.eye(4), estimation_method=None, criteria=None,
                                neighborhood: int = 1, min_points_per_voxel: int = 1) -> RegistrationResult:
    """Voxelized GICP (``pcr_registration_voxelized_gicp``, include/pcr_hip.h): the loop of ``registration_generalized_icp`` without its
    nearest-neighbour search -- a source point is matched to the cell of the target's voxel covariance map it falls into (``neighborhood``
    1), or to that cell and its 6 / 26 neighbours (7 / 27), and every such row weighs in with the cell's member count.  ``target_or_map`` is
    a ``VoxelCovarianceMap`` (``voxel_size`` is then ignored; the map serves any number of calls) or a ``PointCloud``, for which a map of
    ``voxel_size`` is built and closed inside the call.  ``correspondence_set`` holds (source index, map row)."""
    fn = "registration_voxelized_gicp"
    estimation = TransformationEstimationForGeneralizedICP() if estimation_method is None else estimation_method
    if not isinstance(estimation, TransformationEstimationForGeneralizedICP):
        raise RuntimeError(f"{fn}: {type(estimation).__name__} is not TransformationEstimationForGeneralizedICP")
    _check_vgicp_rule(fn, neighborhood, min_points_per_voxel)
    criteria = criteria or ICPConvergenceCriteria()
    own = None
    if isinstance(target_or_map, VoxelCovarianceMap):
        vmap = target_or_map
        vmap._open()
    elif isinstance(target_or_map, PointCloud):
        if voxel_size is None:
            raise ValueError(f"{fn}: voxel_size is required when the target is a PointCloud")
        _check_voxel_size(fn, voxel_size)
        target = target_or_map
        if len(target) and not target.has_covariances():
            target = _ensure_gicp_normals(target)
        own = vmap = VoxelCovarianceMap(target, voxel_size, estimation.epsilon)
    else:
        raise TypeError(f"{fn}: the target must be a PointCloud or a VoxelCovarianceMap, got {type(target_or_map).__name__}")
    try:
        if len(source) and not source.has_covariances():
            source = _ensure_gicp_normals(source)
        ctx = _lib.Context.current()
        torch = _torch()
        ns = len(source)
        corr = torch.empty((max(ns, 1) * int(neighborhood), 2), dtype=torch.int32, device="cuda")
        res = _lib.PcrResult()
        _, Tp = _T(init)
        p = _lib.PcrVgicpParams(int(estimation.kernel.kind), float(estimation.kernel.k), float(estimation.epsilon), float(criteria.relative_fitness),
                                float(criteria.relative_rmse), int(criteria.max_iteration), int(neighborhood), int(min_points_per_voxel))
        cov = source._cov if source.has_covariances() else None
        ctx.check(ctx.lib.pcr_registration_voxelized_gicp(ctx.handle, _ptr(source.device_xyz()), _ptr(cov), _ptr(source.device_normals() if cov is None else None),
                                                          C.c_int64(ns), vmap._open(), Tp, C.byref(p), C.byref(res), _ptr(corr)), fn)
        return _result(res, corr)
    finally:
        if own is not None:
            own.close()


def _scan_to_map(fn, scans, voxel_size, init, motion_model, max_range, grid_min, check_rule, check_scan, make_map, register, prepare=None):
    """The recipe of ``scan_to_map_odometry`` and ``scan_to_map_odometry_ndt`` -> ``(poses, results, map)``: the argument checks
    (``check_rule()`` for the caller's own, ``check_scan(k, scan)`` per scan), ``map = make_map(scans[0], grid_min, init)`` with
    ``centered_grid_min`` of scan 0's centre placed at ``init`` for a ``grid_min`` of ``None``, then per further scan
    ``register(scan, map, start)`` from the motion model's start, ``map.insert`` and, with a ``max_range``, ``map.remove_far``.  With a
    ``prepare(k, scan, poses)`` the scan it returns is what is registered and inserted.  An error closes the map."""
    if motion_model not in ("constant_velocity", "static"):
        raise ValueError(f"{fn}: motion_model must be 'constant_velocity' or 'static', got {motion_model!r}")
    _check_voxel_size(fn, voxel_size)
    check_rule()
    if max_range is not None and (not np.isfinite(float(max_range)) or not float(max_range) > 0.0):
        raise ValueError(f"{fn}: max_range must be a finite number greater than 0, got {max_range!r}")
    scans = list(scans)
    if not scans:
        raise ValueError(f"{fn}: at least one scan is needed")
    for k, s in enumerate(scans):
        check_scan(k, s)
    P0 = np.array(np.asarray(init, np.float64), np.float64)
    if P0.shape != (4, 4):
        raise ValueError(f"{fn}: init must have shape (4, 4), got {P0.shape}")
    if grid_min is None:
        c = np.asarray(scans[0].get_center(), np.float64).reshape(3)
        grid_min = _GrowingVoxelMap.centered_grid_min(P0[:3, :3] @ c + P0[:3, 3], voxel_size)
    gmap = make_map(scans[0], grid_min, P0)
    poses, results = [P0], [None]
    try:
        for k in range(1, len(scans)):
            start = poses[-1]
            if motion_model == "constant_velocity" and k >= 2:
                start = poses[-1] @ np.linalg.inv(poses[-2]) @ poses[-1]
            scan = scans[k] if prepare is None else prepare(k, scans[k], poses)
            res = register(scan, gmap, start)
            poses.append(np.array(res.transformation, np.float64))
            results.append(res)
            gmap.insert(scan, poses[-1])
            if max_range is not None:
                gmap.remove_far(poses[-1][:3, 3], max_range)
    except BaseException:
        gmap.close()
        raise
    return poses, results, gmap


def scan_to_map_odometry(scans, voxel_size, init=np.eye(4), estimation_method=None, criteria=None, neighborhood: int = 1, min_points_per_voxel: int = 1,
                         motion_model: str = "constant_velocity", max_range=None, grid_min=None):
    """LiDAR odometry by scan-to-map voxelized GICP -> ``(poses, results, map)``.  Exactly these public calls, in this order (calling them by
    hand with the same arguments gives the same poses bit for bit):

    * ``map = VoxelCovarianceMap.on_grid(scans[0], voxel_size, estimation.epsilon, grid_min, init)``; ``grid_min=None`` is
      ``centered_grid_min`` of scan 0's centre (``get_center()``) placed at ``init``; ``poses[0] = init``, ``results[0] = None``;
    * for every further scan k: ``results[k] = registration_voxelized_gicp(scans[k], map, None, start, estimation_method, criteria, neighborhood,
      min_points_per_voxel)`` with ``start = P[k-1] @ inv(P[k-2]) @ P[k-1]`` under ``"constant_velocity"`` and ``P[k-1]`` under ``"static"`` (and
      for scan 1 in either model); ``poses[k]`` is its transformation;
    * ``map.insert(scans[k], poses[k])``, and with a ``max_range``, ``map.remove_far(poses[k][:3, 3], max_range)``.

    Every scan carries covariances or normals.  A scan that would leave the grid raises the library's error (the map is closed then).  The caller
    owns the returned map and closes it."""
    fn = "scan_to_map_odometry"
    estimation = TransformationEstimationForGeneralizedICP() if estimation_method is None else estimation_method

    def check_rule():
        _check_vgicp_rule(fn, neighborhood, min_points_per_voxel)
        if not isinstance(estimation, TransformationEstimationForGeneralizedICP):
            raise RuntimeError(f"{fn}: {type(estimation).__name__} is not TransformationEstimationForGeneralizedICP")

    return _scan_to_map(fn, scans, voxel_size, init, motion_model, max_range, grid_min, check_rule,
                        lambda k, s: VoxelCovarianceMap._cloud_arrays(fn, s, f"scan {k}"),
                        lambda s, g, P0: VoxelCovarianceMap.on_grid(s, voxel_size, estimation.epsilon, g, P0),
                        lambda s, m, start: registration_voxelized_gicp(s, m, None, start, estimation_method, criteria, neighborhood, min_points_per_voxel))


# ---- NDT on a normal-distributions voxel map (pcr_ndt_map_*, pcr_ndt_linearize, pcr_registration_ndt; the rule: include/pcr_hip.h)
def _check_ndt_rule(fn: str, neighborhood=7, outlier_ratio=0.55, min_points_per_voxel=6, eigenvalue_ratio=0.01):
    if neighborhood not in (1, 7, 27):
        raise ValueError(f"{fn}: neighborhood must be 1, 7 or 27, got {neighborhood!r}")
    if not isinstance(min_points_per_voxel, (int, np.integer)) or min_points_per_voxel < 2:
        raise ValueError(f"{fn}: min_points_per_voxel must be an integer >= 2, got {min_points_per_voxel!r}")
    for name, v, closed in (("outlier_ratio", outlier_ratio, False), ("eigenvalue_ratio", eigenvalue_ratio, True)):
        try:
            x = float(v)
        except (TypeError, ValueError):
            x = float("nan")
        if not (0.0 < x < 1.0 or (closed and x == 1.0)):
            raise ValueError(f"{fn}: {name} must lie in (0, 1{']' if closed else ')'}, got {v!r}")


class NdtLinearization:
    """What ``NormalDistributionsMap.linearize`` returns: ``JTJ`` (6, 6), ``JTr`` (6,), ``score``, ``rows``, ``points_with_rows``, ``sum_d2``."""

    def __init__(self, JTJ, JTr, score, rows, points_with_rows, sum_d2):
        self.JTJ, self.JTr, self.score, self.rows, self.points_with_rows, self.sum_d2 = JTJ, JTr, score, rows, points_with_rows, sum_d2

    def __repr__(self):
        return f"NdtLinearization(score={self.score!r}, rows={self.rows}, points_with_rows={self.points_with_rows}, sum_d2={self.sum_d2!r})"


class NormalDistributionsMap(_GrowingVoxelMap):
    """The target of NDT registration (Biber & Strasser 2003; Magnusson 2009; PCL's ``NormalDistributionsTransform``): per occupied cell of
    ``voxel_down_sample``'s grid the member count, the mean, the covariance ``C_v`` of the member positions about it and -- for a cell with at
    least ``min_points_per_voxel`` members that do not coincide -- the float64 information matrix ``A_v``, the inverse of the sample covariance
    with its eigenvalues raised to ``eigenvalue_ratio`` times the largest.  Built once from the target's positions alone (no normals, no
    covariances) and good for any number of registrations until ``close()``.  Rows are in Morton order of the cell index.

    ``NormalDistributionsMap(target, voxel_size)`` takes the grid from the target's own minimum, so nothing below that minimum can ever be
    added.  A map that will grow is made by ``NormalDistributionsMap.on_grid(target, voxel_size, grid_min=centered_grid_min(point,
    voxel_size))``, whose grid has ``point`` in its middle; then ``insert`` adds a scan at a pose, ``merge`` adds another map of the same grid
    and rule, and ``remove_far`` drops the cells far from a point (RULE OF A MAP / MERGE / INSERT / REMOVE_FAR of include/pcr_hip.h).  A cell
    held by both sides of a merge gets the summed count, the count-weighted mean, the covariances moved to that mean by the parallel-axis term,
    and its validity and ``A_v`` computed anew -- so cells too thin after one scan become valid as scans accumulate.  Each of these calls
    replaces the rows as a whole: row indices of an earlier ``correspondence_set`` are stale afterwards, and no other call may use the map while
    one runs.  ``len(map)`` and every property read the map as it is after the call."""

    _C, _NAME = "pcr_ndt_map", "NormalDistributionsMap"
    _COLUMNS = {"cells": (3, "int32"), "counts": (None, "int32"), "points": (3, "float32"), "covariances": (6, "float32"), "information": (6, "float64"),
                "valid": (None, "uint8")}

    def __init__(self, target: PointCloud, voxel_size: float, min_points_per_voxel: int = 6, eigenvalue_ratio: float = 0.01):
        self._create(target, voxel_size, min_points_per_voxel, eigenvalue_ratio, None, None)

    @classmethod
    def on_grid(cls, target: PointCloud, voxel_size: float, min_points_per_voxel: int = 6, eigenvalue_ratio: float = 0.01, grid_min=None, transformation=None):
        """The map of ``target`` placed at ``transformation`` (4x4; ``None``: as it lies) on the grid whose origin is
        ``grid_min - voxel_size / 2`` (``pcr_ndt_map_create_on_grid``).  With both ``None`` this is
        ``NormalDistributionsMap(target, voxel_size, min_points_per_voxel, eigenvalue_ratio)``, through the same call and with the same bits; a
        pose needs a ``grid_min``.  A point outside the grid's 2^21 cells per axis -- below ``grid_min - voxel_size / 2`` too -- raises the
        library's error."""
        m = cls.__new__(cls)
        m._create(target, voxel_size, min_points_per_voxel, eigenvalue_ratio, grid_min, transformation)
        return m

    def _create(self, target, voxel_size, min_points_per_voxel, eigenvalue_ratio, grid_min, transformation):
        fn = "NormalDistributionsMap"
        self._voxel_size = _check_voxel_size(fn, voxel_size)
        _check_ndt_rule(fn, min_points_per_voxel=min_points_per_voxel, eigenvalue_ratio=eigenvalue_ratio)
        self.min_points_per_voxel, self.eigenvalue_ratio = int(min_points_per_voxel), float(eigenvalue_ratio)
        if not isinstance(target, PointCloud) or len(target) == 0:
            raise RuntimeError(f"{fn}: the target must be a PointCloud with at least one point")
        g, T, Tp = self._placement(grid_min, transformation)
        ctx = _lib.Context.current()
        h = C.c_void_p()
        if g is None:
            ctx.check(ctx.lib.pcr_ndt_map_create(ctx.handle, _ptr(target.device_xyz()), C.c_int64(len(target)), C.c_double(self._voxel_size),
                                                 C.c_int(self.min_points_per_voxel), C.c_double(self.eigenvalue_ratio), C.byref(h)), fn)
        else:
            ctx.check(ctx.lib.pcr_ndt_map_create_on_grid(ctx.handle, _ptr(target.device_xyz()), C.c_int64(len(target)), C.c_double(self._voxel_size),
                                                         C.c_int(self.min_points_per_voxel), C.c_double(self.eigenvalue_ratio),
                                                         g.ctypes.data_as(C.POINTER(C.c_double)), Tp, C.byref(h)), fn)
        self._adopt(ctx, h)

    @property
    def grid_min(self) -> np.ndarray:
        """(3,) float64: g of the RULE OF A MAP; for a map made without ``grid_min`` the target's minimum"""
        h = self._open()
        g = (C.c_double * 3)()
        self._lib.pcr_ndt_map_rule(h, g, None, None)
        return np.array(g, np.float64)

    @property
    def origin(self) -> np.ndarray:
        """(3,) float64: the target's minimum - ``voxel_size / 2``, the corner of cell (0, 0, 0)"""
        h = self._open()
        o = (C.c_double * 3)()
        self._lib.pcr_ndt_map_grid(h, o, None)
        return np.array(o, np.float64)

    def insert(self, cloud: PointCloud, transformation=None):
        """Add ``cloud`` placed at ``transformation`` (``pcr_ndt_map_insert``; ``None`` is the identity): the map becomes MERGE(map, the map of
        the placed cloud on this grid with this map's rule).  A point outside the grid raises the library's error and leaves the map as it
        was."""
        fn = "NormalDistributionsMap.insert"
        h = self._open()
        if not isinstance(cloud, PointCloud) or len(cloud) == 0:
            raise RuntimeError(f"{fn}: the cloud must be a PointCloud with at least one point")
        T, Tp = self._pose(fn, np.eye(4) if transformation is None else transformation)
        ctx = _lib.Context.current()
        ctx.check(ctx.lib.pcr_ndt_map_insert(ctx.handle, h, _ptr(cloud.device_xyz()), C.c_int64(len(cloud)), Tp), fn)
        self._refresh()

    @property
    def information(self) -> np.ndarray:
        """(cells, 6) float64: A_v, xx,xy,xz,yy,yz,zz; zero for an invalid cell"""
        return self._read("information").cpu().numpy()

    @property
    def valid(self) -> np.ndarray:
        """(cells,) bool: the cells that give rows"""
        return self._read("valid").cpu().numpy().astype(bool)

    def correspondences(self, source: PointCloud, T=np.eye(4), neighborhood: int = 7):
        """The rows (source index, map row) of the rule at the pose ``T``, ordered by source index and then by the neighbourhood's offset
        order: a device tensor (rows, 2) int32."""
        fn = "NormalDistributionsMap.correspondences"
        _check_ndt_rule(fn, neighborhood)
        h = self._open()
        ctx = _lib.Context.current()
        torch = _torch()
        ns = len(source)
        rows = torch.empty((max(ns, 1) * int(neighborhood), 2), dtype=torch.int32, device="cuda")
        n = C.c_int64(0)
        _, Tp = _T(T)
        ctx.check(ctx.lib.pcr_ndt_map_correspondences(ctx.handle, h, _ptr(source.device_xyz()), C.c_int64(ns), Tp, C.c_int(int(neighborhood)), _ptr(rows), C.byref(n)), fn)
        return rows[: n.value]

    def linearize(self, source: PointCloud, T=np.eye(4), neighborhood: int = 7, outlier_ratio: float = 0.55) -> NdtLinearization:
        """The sums of one update at the pose ``T`` (``pcr_ndt_linearize``, one kernel launch, the same bits on every run): the 6x6 matrix, the
        right-hand side, the NDT score, the number of rows, of source points with a row, and the rows' summed squared distances."""
        fn = "NormalDistributionsMap.linearize"
        _check_ndt_rule(fn, neighborhood, outlier_ratio)
        h = self._open()
        ctx = _lib.Context.current()
        JTJ, JTr = np.zeros((6, 6), np.float64), np.zeros(6, np.float64)
        score, sum_d2, rows, hits = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int64(0)
        _, Tp = _T(T)
        dp = C.POINTER(C.c_double)
        ctx.check(ctx.lib.pcr_ndt_linearize(ctx.handle, h, _ptr(source.device_xyz()), C.c_int64(len(source)), Tp, C.c_int(int(neighborhood)), C.c_double(float(outlier_ratio)),
                                            JTJ.ctypes.data_as(dp), JTr.ctypes.data_as(dp), C.byref(score), C.byref(rows), C.byref(hits), C.byref(sum_d2)), fn)
        return NdtLinearization(JTJ, JTr, float(score.value), int(rows.value), int(hits.value), float(sum_d2.value))


def registration_ndt(source: PointCloud, target_or_map, voxel_size=None, init=np.eye(4), criteria=None, neighborhood: int = 7, outlier_ratio: float = 0.55,
                     min_points_per_voxel: int = 6) -> RegistrationResult:
    """NDT registration (``pcr_registration_ndt``, include/pcr_hip.h): RegistrationICP's loop in which a source point is scored against the
    normal distribution of the cell of the target's ``NormalDistributionsMap`` it falls into (``neighborhood`` 1), or of that cell and its
    6 / 26 neighbours (7 / 27).  Neither cloud needs normals or covariances.  The update is the Gauss-Newton (IRLS) step of Magnusson's
    score with ``outlier_ratio``, not PCL's Newton step with a line search.  ``target_or_map`` is a ``NormalDistributionsMap``
    (``voxel_size`` and ``min_points_per_voxel`` are then the map's own) or a ``PointCloud``, for which a map of ``voxel_size`` is built and
    closed inside the call.  ``correspondence_set`` holds (source index, map row)."""
    fn = "registration_ndt"
    _check_ndt_rule(fn, neighborhood, outlier_ratio, min_points_per_voxel)
    criteria = criteria or ICPConvergenceCriteria()
    own = None
    if isinstance(target_or_map, NormalDistributionsMap):
        nmap = target_or_map
        nmap._open()
    elif isinstance(target_or_map, PointCloud):
        if voxel_size is None:
            raise ValueError(f"{fn}: voxel_size is required when the target is a PointCloud")
        _check_voxel_size(fn, voxel_size)
        own = nmap = NormalDistributionsMap(target_or_map, voxel_size, min_points_per_voxel)
    else:
        raise TypeError(f"{fn}: the target must be a PointCloud or a NormalDistributionsMap, got {type(target_or_map).__name__}")
    try:
        ctx = _lib.Context.current()
        torch = _torch()
        ns = len(source)
        corr = torch.empty((max(ns, 1) * int(neighborhood), 2), dtype=torch.int32, device="cuda")
        res = _lib.PcrResult()
        _, Tp = _T(init)
        p = _lib.PcrNdtParams(float(criteria.relative_fitness), float(criteria.relative_rmse), int(criteria.max_iteration), int(neighborhood), float(outlier_ratio))
        ctx.check(ctx.lib.pcr_registration_ndt(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), nmap._open(), Tp, C.byref(p), C.byref(res), _ptr(corr)), fn)
        return _result(res, corr)
    finally:
        if own is not None:
            own.close()


def scan_to_map_odometry_ndt(scans, voxel_size, init=np.eye(4), criteria=None, neighborhood: int = 7, outlier_ratio: float = 0.55, min_points_per_voxel: int = 6,
                             eigenvalue_ratio: float = 0.01, motion_model: str = "constant_velocity", max_range=None, grid_min=None):
    """LiDAR odometry by scan-to-map NDT -> ``(poses, results, map)``: ``scan_to_map_odometry`` with a ``NormalDistributionsMap``, so the scans
    need neither normals nor covariances.  Exactly these public calls, in this order (calling them by hand with the same arguments gives the
    same poses bit for bit):

    * ``map = NormalDistributionsMap.on_grid(scans[0], voxel_size, min_points_per_voxel, eigenvalue_ratio, grid_min, init)``; ``grid_min=None``
      is ``centered_grid_min`` of scan 0's centre (``get_center()``) placed at ``init``; ``poses[0] = init``, ``results[0] = None``;
    * for every further scan k: ``results[k] = registration_ndt(scans[k], map, None, start, criteria, neighborhood, outlier_ratio,
      min_points_per_voxel)`` with ``start = P[k-1] @ inv(P[k-2]) @ P[k-1]`` under ``"constant_velocity"`` and ``P[k-1]`` under ``"static"``
      (and for scan 1 in either model); ``poses[k]`` is its transformation;
    * ``map.insert(scans[k], poses[k])``, and with a ``max_range``, ``map.remove_far(poses[k][:3, 3], max_range)``.

    A scan that would leave the grid raises the library's error (the map is closed then).  The caller owns the returned map and closes it."""
    fn = "scan_to_map_odometry_ndt"

    def check_scan(k, s):
        if not isinstance(s, PointCloud) or len(s) == 0:
            raise RuntimeError(f"{fn}: scan {k} must be a PointCloud with at least one point")

    return _scan_to_map(fn, scans, voxel_size, init, motion_model, max_range, grid_min,
                        lambda: _check_ndt_rule(fn, neighborhood, outlier_ratio, min_points_per_voxel, eigenvalue_ratio), check_scan,
                        lambda s, g, P0: NormalDistributionsMap.on_grid(s, voxel_size, min_points_per_voxel, eigenvalue_ratio, g, P0),
                        lambda s, m, start: registration_ndt(s, m, None, start, criteria, neighborhood, outlier_ratio, min_points_per_voxel))


# ---- scan-to-map ICP on a voxel point map (pcr_point_map_*, pcr_registration_point_map; the rule: include/pcr_hip.h)
def _check_point_map_rule(fn: str, neighborhood=27, max_points_per_voxel=20):
    if neighborhood not in (1, 7, 27):
        raise ValueError(f"{fn}: neighborhood must be 1, 7 or 27, got {neighborhood!r}")
    if not isinstance(max_points_per_voxel, (int, np.integer)) or not 1 <= max_points_per_voxel <= 64:
        raise ValueError(f"{fn}: max_points_per_voxel must be an integer in 1 .. 64, got {max_points_per_voxel!r}")


def _check_distance(fn: str, max_correspondence_distance) -> float:
    try:
        d = float(max_correspondence_distance)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: max_correspondence_distance must be a number greater than 0, got {max_correspondence_distance!r}") from None
    if not np.isfinite(d) or not (d > 0.0):
        raise ValueError(f"{fn}: max_correspondence_distance must be a finite number greater than 0, got {max_correspondence_distance!r}")
    return d


def _point_map_estimation(fn: str, estimation_method) -> _lib.PcrEstimation:
    """the estimator of the point map as the C struct: point to point (the default; its ``kernel`` is read here) or point to plane"""
    est = TransformationEstimationPointToPoint() if estimation_method is None else estimation_method
    if isinstance(est, TransformationEstimationPointToPoint):
        if est.with_scaling:
            raise ValueError(f"{fn}: with_scaling is not supported (the point-to-point update is the Gauss-Newton form, not the Umeyama fit)")
        return _lib.PcrEstimation(_lib.EST_POINT_TO_POINT, 0, int(est.kernel.kind), float(est.kernel.k), 1e-3)
    if isinstance(est, TransformationEstimationPointToPlane):
        return _lib.PcrEstimation(_lib.EST_POINT_TO_PLANE, 0, int(est.kernel.kind), float(est.kernel.k), 1e-3)
    raise RuntimeError(f"{fn}: {type(est).__name__} is neither TransformationEstimationPointToPoint nor TransformationEstimationPointToPlane")


class PointMapLinearization:
    """What ``VoxelPointMap.linearize`` returns: ``JTJ`` (6, 6), ``JTr`` (6,), ``rows``, ``sum_d2``, ``sum_r2``."""

    def __init__(self, JTJ, JTr, rows, sum_d2, sum_r2):
        self.JTJ, self.JTr, self.rows, self.sum_d2, self.sum_r2 = JTJ, JTr, rows, sum_d2, sum_r2

    def __repr__(self):
        return f"PointMapLinearization(rows={self.rows}, sum_d2={self.sum_d2!r}, sum_r2={self.sum_r2!r})"


class VoxelPointMap(_GrowingVoxelMap):
    """A local map of raw points (KISS-ICP's: a voxel hash with at most ``max_points_per_voxel`` points per cell) behind a cell hash on the
    device, the target of ``registration_point_map``.  The rows are the kept points -- with their normals when the target carries normals --
    ordered by (Morton key of the cell, arrival); ``len(map)`` is the number of rows.  A cell keeps the first ``max_points_per_voxel`` points
    that arrive in it and drops the others, whether they arrive in one cloud or in many (MAP / MERGE / INSERT of include/pcr_hip.h).

    ``VoxelPointMap(target, voxel_size)`` takes the grid from the target's own minimum; a map that will grow is made by
    ``VoxelPointMap.on_grid(target, voxel_size, grid_min=centered_grid_min(point, voxel_size))``.  ``insert`` adds a scan at a pose, ``merge``
    another map of the same grid and rule (NOT commutative: in a full cell the map's own points stay), ``remove_far`` drops the ROWS far from a
    point.  Each of them replaces the rows as a whole: row indices of an earlier ``correspondence_set`` are stale afterwards, and no other call
    may use the map while one runs.

    A map made from a target without normals can compute them from its own rows: ``estimate_normals(radius, min_neighbors)`` (ESTIMATE of
    include/pcr_hip.h).  From then on the map keeps them current through ``insert``, ``merge`` and ``remove_far``, and point-to-plane ICP runs on
    it with scans that carry no normals; a row with fewer than ``min_neighbors`` neighbours is not valid and gives the estimator no row."""

    _C, _NAME = "pcr_point_map", "VoxelPointMap"
    _COLUMNS = {"cells": (3, "int32"), "starts": (None, "int32"), "counts": (None, "int32"), "points": (3, "float32"), "normals": (3, "float32")}
    _PER_ROW = ("points", "normals")

    def __init__(self, target: PointCloud, voxel_size: float, max_points_per_voxel: int = 20):
        self._create(target, voxel_size, max_points_per_voxel, None, None)

    @classmethod
    def on_grid(cls, target: PointCloud, voxel_size: float, max_points_per_voxel: int = 20, grid_min=None, transformation=None):
        """The map of ``target`` placed at ``transformation`` (4x4; ``None``: as it lies, bit for bit) on the grid whose origin is
        ``grid_min - voxel_size / 2`` (``pcr_point_map_create_on_grid``); a pose needs a ``grid_min``.  A point outside the grid's 2^21 cells
        per axis raises the library's error."""
        m = cls.__new__(cls)
        m._create(target, voxel_size, max_points_per_voxel, grid_min, transformation)
        return m

    def _create(self, target, voxel_size, max_points_per_voxel, grid_min, transformation):
        fn = "VoxelPointMap"
        self._voxel_size = _check_voxel_size(fn, voxel_size)
        _check_point_map_rule(fn, max_points_per_voxel=max_points_per_voxel)
        self.max_points_per_voxel = int(max_points_per_voxel)
        if not isinstance(target, PointCloud) or len(target) == 0:
            raise RuntimeError(f"{fn}: the target must be a PointCloud with at least one point")
        g, T, Tp = self._placement(grid_min, transformation)
        self.has_normals = bool(target.has_normals())
        nrm = target.device_normals() if self.has_normals else None
        ctx = _lib.Context.current()
        h = C.c_void_p()
        if g is None:
            ctx.check(ctx.lib.pcr_point_map_create(ctx.handle, _ptr(target.device_xyz()), _ptr(nrm), C.c_int64(len(target)), C.c_double(self._voxel_size),
                                                   C.c_int(self.max_points_per_voxel), C.byref(h)), fn)
        else:
            ctx.check(ctx.lib.pcr_point_map_create_on_grid(ctx.handle, _ptr(target.device_xyz()), _ptr(nrm), C.c_int64(len(target)), C.c_double(self._voxel_size),
                                                           C.c_int(self.max_points_per_voxel), g.ctypes.data_as(C.POINTER(C.c_double)), Tp, C.byref(h)), fn)
        self._adopt(ctx, h)

    def _refresh(self):
        rows, cells = C.c_int64(0), C.c_int64(0)
        self._lib.pcr_point_map_size(self._handle, C.byref(rows), C.byref(cells))
        self._cells, self._n_cells = int(rows.value), int(cells.value)      # (the base's _cells is what len() returns: the rows)
        nrm = C.c_int(0)
        self._lib.pcr_point_map_grid(self._handle, None, None, None, None, C.byref(nrm))
        self.has_normals = bool(nrm.value)                                  # (a merge with an estimated map, or estimate_normals, may change it)

    def _normal_rule(self):
        est, radius, kmin = C.c_int(0), C.c_double(0), C.c_int(0)
        self._lib.pcr_point_map_normal_rule(self._open(), C.byref(est), C.byref(radius), C.byref(kmin))
        return bool(est.value), float(radius.value), int(kmin.value)

    @property
    def normals_estimated(self) -> bool:
        """whether the normals are the map's own (``estimate_normals``), kept current by the map itself"""
        return self._normal_rule()[0]

    @property
    def normal_radius(self):
        """the radius of ``estimate_normals``, or ``None`` on a map that does not estimate its normals"""
        est, radius, _ = self._normal_rule()
        return radius if est else None

    @property
    def normal_min_neighbors(self):
        """``min_neighbors`` of ``estimate_normals``, or ``None`` on a map that does not estimate its normals"""
        est, _, kmin = self._normal_rule()
        return kmin if est else None

    @property
    def normal_counts(self) -> np.ndarray:
        """(rows,) int32: the map rows within ``normal_radius`` of every row, itself included (an estimated map only)"""
        h = self._open()
        if not self.normals_estimated:
            raise RuntimeError("VoxelPointMap.normal_counts: the map does not estimate its normals (estimate_normals)")
        ctx = _lib.Context.current()
        t = _torch().empty((self._cells,), dtype=_torch().int32, device="cuda")
        ctx.check(ctx.lib.pcr_point_map_read_normal_counts(ctx.handle, h, _ptr(t)), "VoxelPointMap.normal_counts")
        return t.cpu().numpy()

    @property
    def normal_valid(self) -> np.ndarray:
        """(rows,) bool: ``normal_counts >= normal_min_neighbors``, the rows point-to-plane ICP takes"""
        return self.normal_counts >= self.normal_min_neighbors

    def estimate_normals(self, radius=None, min_neighbors: int = 5) -> int:
        """Compute the normal of every row from the map rows within ``radius`` of it (``pcr_point_map_estimate_normals``; ``None``: the voxel
        size, the largest radius for which the 27 cells around a row hold every such row) and return the number of valid rows, those with at
        least ``min_neighbors`` neighbours (the row itself counts).  The map keeps the rule: ``insert``, ``merge`` and ``remove_far`` estimate
        the whole new map again.  Refused on a map with normals of the caller's; on an estimated map it estimates again with the new arguments.
        The normals carry no orientation (the point-to-plane row does not read the sign)."""
        fn = "VoxelPointMap.estimate_normals"
        h = self._open()
        r = self._voxel_size if radius is None else radius
        try:
            r = float(r)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: radius must be a number in (0, voxel_size], got {radius!r}") from None
        if not np.isfinite(r) or not (0.0 < r <= self._voxel_size):
            raise ValueError(f"{fn}: radius must be a finite number in (0, voxel_size = {self._voxel_size!r}], got {radius!r}")
        if not isinstance(min_neighbors, (int, np.integer)) or isinstance(min_neighbors, bool) or min_neighbors < 3:
            raise ValueError(f"{fn}: min_neighbors must be an integer of at least 3, got {min_neighbors!r}")
        if self.has_normals and not self.normals_estimated:
            raise RuntimeError(f"{fn}: the map has normals of the caller's; normals are estimated on a map made without")
        ctx = _lib.Context.current()
        valid = C.c_int64(0)
        ctx.check(ctx.lib.pcr_point_map_estimate_normals(ctx.handle, h, C.c_double(r), C.c_int(int(min_neighbors)), C.byref(valid)), fn)
        self._refresh()
        return int(valid.value)

    def _read(self, what: str):
        """one column as a device tensor: per row for the points and normals, per cell for the cell table"""
        h = self._open()
        if what == "normals" and not self.has_normals:
            raise RuntimeError("VoxelPointMap.normals: the map has no normals")
        ctx = _lib.Context.current()
        torch = _torch()
        cols, dtype = self._COLUMNS[what]
        n = self._cells if what in self._PER_ROW else self._n_cells
        t = torch.empty((n,) if cols is None else (n, cols), dtype=getattr(torch, dtype), device="cuda")
        args = [_ptr(t if k == what else None) for k in self._COLUMNS]
        ctx.check(ctx.lib.pcr_point_map_read(ctx.handle, h, *args), f"VoxelPointMap.{what}")
        return t

    @property
    def covariances(self):
        raise AttributeError("VoxelPointMap keeps points, not statistics: it has no covariances")

    @property
    def starts(self) -> np.ndarray:
        """(cells,) int32: the first row of every cell; its rows are ``starts[c] .. starts[c] + counts[c] - 1``"""
        return self._read("starts").cpu().numpy()

    @property
    def normals(self) -> np.ndarray:
        """(rows, 3) float32: the normal of every row, as inserted (rotated by the pose, not normalised), or as estimated by the map"""
        return self._read("normals").cpu().numpy()

    def _grid(self):
        h = self._open()
        g, o = (C.c_double * 3)(), (C.c_double * 3)()
        self._lib.pcr_point_map_grid(h, g, o, None, None, None)
        return np.array(g, np.float64), np.array(o, np.float64)

    @property
    def grid_min(self) -> np.ndarray:
        """(3,) float64: g of the GRID rule; for a map made without ``grid_min`` the target's minimum"""
        return self._grid()[0]

    @property
    def origin(self) -> np.ndarray:
        """(3,) float64: ``grid_min - voxel_size / 2``, the corner of cell (0, 0, 0)"""
        return self._grid()[1]

    def to_point_cloud(self) -> PointCloud:
        """The rows as a cloud, with their normals if the map has normals."""
        pc = PointCloud()
        pc._xyz = self._read("points")
        if self.has_normals:
            pc._nrm = self._read("normals")
        return pc

    def insert(self, cloud: PointCloud, transformation=None):
        """Add ``cloud`` placed at ``transformation`` (``pcr_point_map_insert``; ``None``: as it lies): every point, in the cloud's order, joins
        its cell's list while that list has fewer than ``max_points_per_voxel`` entries.  A map with normals of the caller's needs a cloud with
        normals; a map that estimates its normals takes the points alone (normals the cloud carries are not read) and estimates again.  A point
        outside the grid raises the library's error and leaves the map as it was."""
        fn = "VoxelPointMap.insert"
        h = self._open()
        if not isinstance(cloud, PointCloud) or len(cloud) == 0:
            raise RuntimeError(f"{fn}: the cloud must be a PointCloud with at least one point")
        own = self.has_normals and not self.normals_estimated
        if own and not cloud.has_normals():
            raise RuntimeError(f"{fn}: the map has normals and the cloud has none")
        T, Tp = self._pose(fn, transformation)
        ctx = _lib.Context.current()
        ctx.check(ctx.lib.pcr_point_map_insert(ctx.handle, h, _ptr(cloud.device_xyz()), _ptr(cloud.device_normals() if own else None),
                                               C.c_int64(len(cloud)), Tp), fn)
        self._refresh()

    def correspondences(self, source: PointCloud, T=np.eye(4), max_correspondence_distance=None, neighborhood: int = 27):
        """The rows (source index, map row) of the rule at the pose ``T``, at most one per source point, ordered by source index: a device
        tensor (rows, 2) int32."""
        fn = "VoxelPointMap.correspondences"
        _check_point_map_rule(fn, neighborhood)
        d = _check_distance(fn, max_correspondence_distance)
        h = self._open()
        ctx = _lib.Context.current()
        torch = _torch()
        ns = len(source)
        rows = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
        n = C.c_int64(0)
        _, Tp = _T(T)
        ctx.check(ctx.lib.pcr_point_map_correspondences(ctx.handle, h, _ptr(source.device_xyz()), C.c_int64(ns), Tp, C.c_double(d), C.c_int(int(neighborhood)), _ptr(rows),
                                                        C.byref(n)), fn)
        return rows[: n.value]

    def linearize(self, source: PointCloud, T=np.eye(4), max_correspondence_distance=None, estimation_method=None, neighborhood: int = 27) -> PointMapLinearization:
        """The sums of one update at the pose ``T`` (``pcr_point_map_linearize``, one launch of the iteration kernel, the same bits on every
        run): the 6x6 matrix, the right-hand side, the number of rows, their summed squared distances and squared residuals.  Point to plane on
        a map that estimates its normals counts the rows whose map row is valid, and no others."""
        fn = "VoxelPointMap.linearize"
        _check_point_map_rule(fn, neighborhood)
        d = _check_distance(fn, max_correspondence_distance)
        est = _point_map_estimation(fn, estimation_method)
        h = self._open()
        if est.kind == _lib.EST_POINT_TO_PLANE and not self.has_normals:
            raise RuntimeError(f"{fn}: TransformationEstimationPointToPlane needs a map with normals")
        ctx = _lib.Context.current()
        JTJ, JTr = np.zeros((6, 6), np.float64), np.zeros(6, np.float64)
        sum_d2, sum_r2, rows = C.c_double(0), C.c_double(0), C.c_int64(0)
        _, Tp = _T(T)
        dp = C.POINTER(C.c_double)
        ctx.check(ctx.lib.pcr_point_map_linearize(ctx.handle, h, _ptr(source.device_xyz()), C.c_int64(len(source)), Tp, C.c_double(d), C.c_int(int(neighborhood)), C.byref(est),
                                                  JTJ.ctypes.data_as(dp), JTr.ctypes.data_as(dp), C.byref(rows), C.byref(sum_d2), C.byref(sum_r2)), fn)
        return PointMapLinearization(JTJ, JTr, int(rows.value), float(sum_d2.value), float(sum_r2.value))

    def linearize_continuous(self, source: PointCloud, T_begin, T_end, max_correspondence_distance, estimation_method=None, neighborhood: int = 27, t_begin=None, t_end=None,
                             return_matches: bool = False) -> "ContinuousTimeLinearization":
        """The sums of one continuous-time update at the pose pair (``T_begin``, ``T_end``) of the sweep
        (``pcr_point_map_linearize_continuous``, one launch, the same bits on every run): every source point is placed at the pose
        interpolated at its own time (``source.times``; ``t_begin`` / ``t_end`` default to their minimum / maximum), matched by the map's own
        rule, and gives the 12-column rows ``[(1 - alpha) J6, alpha J6]`` of include/pcr_hip.h (continuous time): ``H`` (12, 12), ``g`` (12,),
        ``rows``, ``sum_d2``, ``sum_r2`` and, with ``return_matches``, ``matches`` -- a device int32 tensor with the map row of every source
        point, or -1."""
        fn = "VoxelPointMap.linearize_continuous"
        _check_point_map_rule(fn, neighborhood)
        d = _check_distance(fn, max_correspondence_distance)
        est = _point_map_estimation(fn, estimation_method)
        if not isinstance(source, PointCloud) or not source.has_times():
            raise RuntimeError(f"{fn}: the source must be a PointCloud with times (PointCloud.times)")
        t0, t1 = source._time_span(fn, t_begin, t_end)
        h = self._open()
        if est.kind == _lib.EST_POINT_TO_PLANE and not self.has_normals:
            raise RuntimeError(f"{fn}: TransformationEstimationPointToPlane needs a map with normals")
        ctx = _lib.Context.current()
        ns = len(source)
        H, g = np.zeros((12, 12), np.float64), np.zeros(12, np.float64)
        sum_d2, sum_r2, rows = C.c_double(0), C.c_double(0), C.c_int64(0)
        matches = _torch().empty((ns,), dtype=_torch().int32, device="cuda") if return_matches else None
        _, Tb = _T(T_begin)
        _, Te = _T(T_end)
        dp = C.POINTER(C.c_double)
        ctx.check(ctx.lib.pcr_point_map_linearize_continuous(ctx.handle, h, _ptr(source.device_xyz()), _ptr(source.device_times()), C.c_int64(ns), Tb, Te, C.c_double(t0),
                                                             C.c_double(t1), C.c_double(d), C.c_int(int(neighborhood)), C.byref(est), H.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                                             C.byref(rows), C.byref(sum_d2), C.byref(sum_r2), _ptr(matches)), fn)
        return ContinuousTimeLinearization(H, g, int(rows.value), float(sum_d2.value), float(sum_r2.value), matches)


def registration_point_map(source: PointCloud, target_or_map, max_correspondence_distance, voxel_size=None, init=np.eye(4), estimation_method=None, criteria=None,
                           neighborhood: int = 27, max_points_per_voxel: int = 20) -> RegistrationResult:
    """Scan-to-map ICP (``pcr_registration_point_map``, include/pcr_hip.h): RegistrationICP's loop in which a source point is matched to the
    nearest point among the members of the cell of a ``VoxelPointMap`` it falls into (``neighborhood`` 1) or of that cell and its 6 / 26
    neighbours (7 / 27) -- with 27 and ``max_correspondence_distance <= voxel_size`` the exact nearest map point within that distance.  The
    cost follows the scan, not the map.  ``estimation_method``: ``TransformationEstimationPointToPoint()`` (the default; its update here is
    the Gauss-Newton step weighted by its ``kernel``, what KISS-ICP runs, NOT the Umeyama fit of ``registration_icp``; ``with_scaling`` is
    refused) or ``TransformationEstimationPointToPlane(kernel)``, which needs a map with normals -- the caller's, or the map's own
    (``VoxelPointMap.estimate_normals``), with which a match to a row that is not valid is no row: ``fitness``, ``inlier_rmse`` and
    ``correspondence_set`` are those of the counted rows.  ``target_or_map`` is a ``VoxelPointMap``
    (``voxel_size`` and ``max_points_per_voxel`` are then the map's own) or a ``PointCloud``, for which a map of ``voxel_size`` is built and
    closed inside the call.  ``correspondence_set`` holds (source index, map row)."""
    fn = "registration_point_map"
    _check_point_map_rule(fn, neighborhood, max_points_per_voxel)
    d = _check_distance(fn, max_correspondence_distance)
    est = _point_map_estimation(fn, estimation_method)
    criteria = criteria or ICPConvergenceCriteria()
    own = None
    if isinstance(target_or_map, VoxelPointMap):
        pmap = target_or_map
        pmap._open()
    elif isinstance(target_or_map, PointCloud):
        if voxel_size is None:
            raise ValueError(f"{fn}: voxel_size is required when the target is a PointCloud")
        _check_voxel_size(fn, voxel_size)
        own = pmap = VoxelPointMap(target_or_map, voxel_size, max_points_per_voxel)
    else:
        raise TypeError(f"{fn}: the target must be a PointCloud or a VoxelPointMap, got {type(target_or_map).__name__}")
    try:
        if est.kind == _lib.EST_POINT_TO_PLANE and not pmap.has_normals:
            raise RuntimeError(f"{fn}: TransformationEstimationPointToPlane needs a map with normals")
        ctx = _lib.Context.current()
        torch = _torch()
        ns = len(source)
        corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
        res = _lib.PcrResult()
        _, Tp = _T(init)
        p = _lib.PcrPointMapParams(est, float(criteria.relative_fitness), float(criteria.relative_rmse), int(criteria.max_iteration), int(neighborhood))
        ctx.check(ctx.lib.pcr_registration_point_map(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), pmap._open(), C.c_double(d), Tp, C.byref(p), C.byref(res),
                                                     _ptr(corr)), fn)
        return _result(res, corr)
    finally:
        if own is not None:
            own.close()


class ContinuousTimeLinearization:
    """What ``VoxelPointMap.linearize_continuous`` returns: ``H`` (12, 12), ``g`` (12,), ``rows``, ``sum_d2``, ``sum_r2``, ``matches`` (or None)."""

    def __init__(self, H, g, rows, sum_d2, sum_r2, matches=None):
        self.H, self.g, self.rows, self.sum_d2, self.sum_r2, self.matches = H, g, rows, sum_d2, sum_r2, matches

    def __repr__(self):
        return f"ContinuousTimeLinearization(rows={self.rows}, sum_d2={self.sum_d2!r}, sum_r2={self.sum_r2!r})"


class ContinuousTimeResult:
    """What ``registration_point_map_continuous`` returns: ``begin_pose`` and ``end_pose`` of the sweep (4x4 float64), ``transformation`` (the
    end pose), ``fitness``, ``inlier_rmse``, ``iterations``, ``converged`` and ``correspondence_set`` ((source index, map row) at the
    returned poses, int32)."""

    def __init__(self, begin_pose, end_pose, fitness, inlier_rmse, iterations, converged, matches=None):
        self.begin_pose = np.array(begin_pose, np.float64).reshape(4, 4)
        self.end_pose = np.array(end_pose, np.float64).reshape(4, 4)
        self.transformation = self.end_pose
        self.fitness, self.inlier_rmse, self.iterations, self.converged = float(fitness), float(inlier_rmse), int(iterations), bool(converged)
        self._matches = matches

    @property
    def correspondence_set(self):
        if self._matches is None:
            return np.zeros((0, 2), np.int32)
        m = self._matches if isinstance(self._matches, np.ndarray) else self._matches.cpu().numpy()
        self._matches = m
        i = np.nonzero(m >= 0)[0]
        return np.stack([i, m[i]], 1).astype(np.int32)

    def __repr__(self):
        return f"ContinuousTimeResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, iterations={self.iterations}"


def _ct_exp3(v) -> np.ndarray:
    """E(v) = I + A [v]x + B [v]x^2 of the rule (include/pcr_hip.h, continuous time), float64"""
    x, y, z = (float(c) for c in np.asarray(v, np.float64).reshape(3))
    xx, yy, zz = x * x, y * y, z * z
    t2 = (xx + yy) + zz
    th = np.sqrt(t2)
    if th >= 1e-4:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / t2
    else:
        A, B = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    xy, xz, yz = x * y, x * z, y * z
    return np.array([[1.0 - B * (yy + zz), B * xy - A * z, B * xz + A * y],
                     [B * xy + A * z, 1.0 - B * (xx + zz), B * yz - A * x],
                     [B * xz - A * y, B * yz + A * x, 1.0 - B * (xx + yy)]], np.float64)


def _ct_log3(R) -> np.ndarray:
    """Log(R): the rotation vector with its angle in [0, pi] (the host expression of pcr_ctime.hip)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    s = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    c = ((R[0, 0] + R[1, 1]) + R[2, 2] - 1.0) * 0.5
    theta = np.arctan2(s, c)
    if s < 1e-8 and c > 0.0:
        return w
    if c > -0.99:
        return w * (theta / s)
    d = np.diag(R)
    k = int(np.argmax(d))
    a = np.zeros(3)
    a[k] = np.sqrt(max((d[k] - c) / (1.0 - c), 0.0))
    for j in range(3):
        if j != k:
            a[j] = (R[k, j] + R[j, k]) * 0.5 / ((1.0 - c) * a[k]) if a[k] > 0.0 else 0.0
    n = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    sign = -1.0 if (a[0] * w[0] + a[1] * w[1]) + a[2] * w[2] < 0.0 else 1.0
    return sign * theta * a / n if n > 0.0 else np.zeros(3)


def _ct_step(H, g, rows, T_b, T_e, begin, prior, prior_weight):
    """STEP of the rule -> (T_b, T_e, applied): the Cholesky solve of the free block and the update of the poses; a failed factorisation or a
    non-finite solution applies nothing"""
    T_b, T_e = np.array(T_b, np.float64), np.array(T_e, np.float64)
    H, g = np.array(H, np.float64), np.array(g, np.float64)
    if begin == "free" and prior_weight is not None:
        w_rot, w_trans = float(prior_weight[0]), float(prior_weight[1])
        H[0:3, 0:3] += rows * w_rot * np.eye(3)
        H[3:6, 3:6] += rows * w_trans * np.eye(3)
        g[0:3] += rows * w_rot * _ct_log3(T_b[:3, :3] @ prior[:3, :3].T)
        g[3:6] += rows * w_trans * (T_b[:3, 3] - prior[:3, 3])
    lo = 6 if begin == "fixed" else 0
    delta = np.zeros(12)
    try:
        L = np.linalg.cholesky(H[lo:, lo:])
        delta[lo:] = -np.linalg.solve(L.T, np.linalg.solve(L, g[lo:]))
    except np.linalg.LinAlgError:
        return T_b, T_e, False
    if not np.isfinite(delta).all():
        return T_b, T_e, False
    if begin != "fixed":
        T_b[:3, :3] = _ct_exp3(delta[0:3]) @ T_b[:3, :3]
        T_b[:3, 3] = T_b[:3, 3] + delta[3:6]
    T_e[:3, :3] = _ct_exp3(delta[6:9]) @ T_e[:3, :3]
    T_e[:3, 3] = T_e[:3, 3] + delta[9:12]
    return T_b, T_e, True


def _check_ct_begin(fn, begin, begin_prior_weight):
    if begin not in ("fixed", "free"):
        raise ValueError(f"{fn}: begin must be 'fixed' or 'free', got {begin!r}")
    if begin_prior_weight is None:
        return None
    if begin != "free":
        raise ValueError(f"{fn}: begin_prior_weight needs begin='free'")
    try:
        w = (float(begin_prior_weight[0]), float(begin_prior_weight[1]))
        ok = len(begin_prior_weight) == 2
    except (TypeError, ValueError, IndexError):
        ok, w = False, None
    if not ok or not all(np.isfinite(v) and v >= 0.0 for v in w):
        raise ValueError(f"{fn}: begin_prior_weight must be two finite numbers (w_rot, w_trans) >= 0, got {begin_prior_weight!r}")
    return w


def _ct_pose(fn, name, T):
    T = np.array(np.asarray(T, np.float64), np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{fn}: {name} must have shape (4, 4), got {T.shape}")
    return T


def registration_point_map_continuous(source: PointCloud, target_or_map, max_correspondence_distance, T_begin, T_end=None, voxel_size=None, estimation_method=None,
                                      criteria=None, neighborhood: int = 27, max_points_per_voxel: int = 20, begin: str = "fixed", begin_prior_weight=None, t_begin=None,
                                      t_end=None) -> ContinuousTimeResult:
    """Continuous-time scan-to-map ICP (CT-ICP's elastic formulation as include/pcr_hip.h, continuous time, specifies it; not compared with
    CT-ICP's code): the registration estimates the pose of the sensor at the begin and at the end of the sweep, and every source point is
    placed at the pose interpolated at its own time (``source.times``; ``t_begin`` / ``t_end`` default to their minimum / maximum).  The loop
    is RegistrationICP's, on the host: ``VoxelPointMap.linearize_continuous`` at the start poses (``T_end=None``: ``T_begin``), then a
    Cholesky step on the 12x12 system and the sums again, until the criteria hold or ``max_iteration`` -- one launch and one read-back of 160
    doubles per iteration.  ``begin="fixed"`` (the default) keeps ``T_begin`` bit for bit -- it is the end pose of the sweep before -- and
    estimates the end pose alone; ``begin="free"`` estimates both, optionally held to the given ``T_begin`` by ``begin_prior_weight=(w_rot,
    w_trans)`` per row.  The estimators, the neighbourhoods and the map are those of ``registration_point_map``.  The rotation columns are
    first order in the rotation between the two poses (exact when there is none)."""
    fn = "registration_point_map_continuous"
    _check_point_map_rule(fn, neighborhood, max_points_per_voxel)
    d = _check_distance(fn, max_correspondence_distance)
    _point_map_estimation(fn, estimation_method)
    prior_weight = _check_ct_begin(fn, begin, begin_prior_weight)
    criteria = criteria or ICPConvergenceCriteria()
    T_b = _ct_pose(fn, "T_begin", T_begin)
    T_e = T_b.copy() if T_end is None else _ct_pose(fn, "T_end", T_end)
    if not isinstance(source, PointCloud) or not source.has_times():
        raise RuntimeError(f"{fn}: the source must be a PointCloud with times (PointCloud.times)")
    t0, t1 = source._time_span(fn, t_begin, t_end)
    own = None
    if isinstance(target_or_map, VoxelPointMap):
        pmap = target_or_map
        pmap._open()
    elif isinstance(target_or_map, PointCloud):
        if voxel_size is None:
            raise ValueError(f"{fn}: voxel_size is required when the target is a PointCloud")
        _check_voxel_size(fn, voxel_size)
        own = pmap = VoxelPointMap(target_or_map, voxel_size, max_points_per_voxel)
    else:
        raise TypeError(f"{fn}: the target must be a PointCloud or a VoxelPointMap, got {type(target_or_map).__name__}")
    try:
        n = len(source)
        prior = T_b.copy()

        def sums(T_b, T_e):
            s = pmap.linearize_continuous(source, T_b, T_e, d, estimation_method, neighborhood, t0, t1, True)
            return s, (s.rows / n if n else 0.0), (float(np.sqrt(s.sum_d2 / s.rows)) if s.rows else 0.0)

        s, fit, rmse = sums(T_b, T_e)
        it, converged = 0, False
        while it < int(criteria.max_iteration):
            applied = False
            if s.rows:
                T_b, T_e, applied = _ct_step(s.H, s.g, s.rows, T_b, T_e, begin, prior, prior_weight)
            if not applied:
                break
            before = (fit, rmse)
            s, fit, rmse = sums(T_b, T_e)
            it += 1
            if abs(before[0] - fit) < float(criteria.relative_fitness) and abs(before[1] - rmse) < float(criteria.relative_rmse):
                converged = True
                break
        return ContinuousTimeResult(T_b, T_e, fit, rmse, it, converged, s.matches)
    finally:
        if own is not None:
            own.close()


class AdaptiveThreshold:
    """The correspondence threshold of KISS-ICP, as this statement specifies it (it has not been compared with KISS-ICP's code): the model
    error ``sigma = sqrt(sse / samples)`` starts from ``initial_threshold`` (``sse = initial_threshold^2``, one sample); ``update(predicted,
    estimated)`` forms ``D = inv(predicted) @ estimated``, the deviation of the registration from the motion model's prediction, and
    ``e = |t_D| + 2 max_range sin(theta_D / 2)`` -- how far a point at ``max_range`` moves under it -- and adds ``e^2`` as one more sample
    when ``e > min_motion``.  ``scan_to_map_odometry_icp`` registers with ``max_correspondence_distance = 3 sigma`` and ``GMLoss(sigma / 3)``.
    Plain host Python."""

    def __init__(self, initial_threshold: float, min_motion: float, max_range: float):
        for name, v in (("initial_threshold", initial_threshold), ("min_motion", min_motion), ("max_range", max_range)):
            try:
                x = float(v)
            except (TypeError, ValueError):
                x = float("nan")
            if not np.isfinite(x) or (x < 0.0 if name == "min_motion" else not x > 0.0):
                raise ValueError(f"AdaptiveThreshold: {name} must be a finite number {'>= 0' if name == 'min_motion' else 'greater than 0'}, got {v!r}")
        self.initial_threshold, self.min_motion, self.max_range = float(initial_threshold), float(min_motion), float(max_range)
        self.sse = self.initial_threshold * self.initial_threshold
        self.samples = 1

    @property
    def sigma(self) -> float:
        return float(np.sqrt(self.sse / self.samples))

    @staticmethod
    def model_error(predicted, estimated, max_range: float) -> float:
        D = np.linalg.inv(np.asarray(predicted, np.float64)) @ np.asarray(estimated, np.float64)
        theta = np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
        return float(np.linalg.norm(D[:3, 3]) + 2.0 * max_range * np.sin(theta / 2.0))

    def update(self, predicted, estimated) -> float:
        """Take in one registration; returns its model error ``e``."""
        e = self.model_error(predicted, estimated, self.max_range)
        if e > self.min_motion:
            self.sse += e * e
            self.samples += 1
        return e


def scan_to_map_odometry_icp(scans, voxel_size, max_correspondence_distance=None, init=np.eye(4), estimation_method=None, criteria=None, neighborhood: int = 27,
                             max_points_per_voxel: int = 20, motion_model: str = "constant_velocity", max_range=None, grid_min=None, adaptive_threshold=None):
    """LiDAR odometry by scan-to-map ICP on a ``VoxelPointMap`` (KISS-ICP's recipe without deskewing) -> ``(poses, results, map)``.  Exactly
    these public calls, in this order:

    * ``map = VoxelPointMap.on_grid(scans[0], voxel_size, max_points_per_voxel, grid_min, init)``; ``grid_min=None`` is ``centered_grid_min`` of
      scan 0's centre placed at ``init``; ``poses[0] = init``, ``results[0] = None``;
    * for every further scan k: ``results[k] = registration_point_map(scans[k], map, d, None, start, est, criteria, neighborhood,
      max_points_per_voxel)`` from the motion model's ``start`` (as in ``scan_to_map_odometry``).  With a fixed distance ``d`` is
      ``max_correspondence_distance`` and ``est`` is ``estimation_method``; with an ``AdaptiveThreshold`` ``d = 3 sigma`` and ``est`` is the
      estimator with ``GMLoss(sigma / 3)``, and after the call ``adaptive_threshold.update(start, results[k].transformation)``;
    * ``map.insert(scans[k], poses[k])``, and with a ``max_range``, ``map.remove_far(poses[k][:3, 3], max_range)``.

    Exactly one of ``max_correspondence_distance`` and ``adaptive_threshold`` is given.  Point to plane needs normals on every scan
    (``scan_to_map_odometry_icp_map_normals`` runs it on scans without, on normals the map estimates from its own rows).  The
    caller owns the returned map and closes it."""
    return _scan_to_map_odometry_icp("scan_to_map_odometry_icp", scans, voxel_size, max_correspondence_distance, init, estimation_method, criteria, neighborhood,
                                     max_points_per_voxel, motion_model, max_range, grid_min, adaptive_threshold, False, None, 5)


def scan_to_map_odometry_icp_map_normals(scans, voxel_size, max_correspondence_distance=None, init=np.eye(4), estimation_method=None, criteria=None,
                                         neighborhood: int = 27, max_points_per_voxel: int = 20, motion_model: str = "constant_velocity", max_range=None, grid_min=None,
                                         adaptive_threshold=None, map_normal_radius=None, map_normal_min_neighbors: int = 5):
    """Point-to-plane ``scan_to_map_odometry_icp`` on a map that estimates its normals from its own rows, where the scans of a drive have
    filled in the surface -> ``(poses, results, map)``.  The scans need no normals, and those they carry are not read.  The recipe is that
    of ``scan_to_map_odometry_icp`` with ``estimate_normals`` once after ``on_grid``; exactly these public calls, in this order:

    * ``map = VoxelPointMap.on_grid(PointCloud(scans[0].points), voxel_size, max_points_per_voxel, grid_min, init)`` (the points alone, so
      the map has no normals of the caller's), then once ``map.estimate_normals(map_normal_radius, map_normal_min_neighbors)``
      (``map_normal_radius=None``: the voxel size); ``poses[0] = init``, ``results[0] = None``;
    * for every further scan k the ``registration_point_map`` call of ``scan_to_map_odometry_icp``, whose estimator is
      ``TransformationEstimationPointToPlane`` (``estimation_method=None``: with ``L2Loss``; any other estimator is refused);
    * ``map.insert(scans[k], poses[k])``, and with a ``max_range``, ``map.remove_far(poses[k][:3, 3], max_range)``, each of which estimates
      the whole new map again.

    It is a function of its own so that ``scan_to_map_odometry_icp`` keeps its signature.  The caller owns the returned map and closes it."""
    return _scan_to_map_odometry_icp("scan_to_map_odometry_icp_map_normals", scans, voxel_size, max_correspondence_distance, init,
                                     TransformationEstimationPointToPlane() if estimation_method is None else estimation_method, criteria, neighborhood, max_points_per_voxel,
                                     motion_model, max_range, grid_min, adaptive_threshold, True, map_normal_radius, map_normal_min_neighbors)


def _scan_to_map_odometry_icp(fn, scans, voxel_size, max_correspondence_distance, init, estimation_method, criteria, neighborhood, max_points_per_voxel, motion_model,
                              max_range, grid_min, adaptive_threshold, map_normals, map_normal_radius, map_normal_min_neighbors, deskew=False):
    """the body of ``scan_to_map_odometry_icp`` (``map_normals`` False) and of ``scan_to_map_odometry_icp_map_normals`` (True); ``deskew``: that of
    ``scan_to_map_odometry_icp_deskew``"""
    estimation = TransformationEstimationPointToPoint() if estimation_method is None else estimation_method
    plane = isinstance(estimation, TransformationEstimationPointToPlane)

    def check_rule():
        _check_point_map_rule(fn, neighborhood, max_points_per_voxel)
        _point_map_estimation(fn, estimation)
        if (max_correspondence_distance is None) == (adaptive_threshold is None):
            raise ValueError(f"{fn}: exactly one of max_correspondence_distance and adaptive_threshold must be given")
        if adaptive_threshold is None:
            _check_distance(fn, max_correspondence_distance)
        elif not isinstance(adaptive_threshold, AdaptiveThreshold):
            raise TypeError(f"{fn}: adaptive_threshold must be an AdaptiveThreshold, got {type(adaptive_threshold).__name__}")
        if map_normals:
            if not plane:
                raise ValueError(f"{fn}: estimation_method must be a TransformationEstimationPointToPlane (point to point reads no normals)")
            v = _check_voxel_size(fn, voxel_size)
            try:
                r = v if map_normal_radius is None else float(map_normal_radius)
            except (TypeError, ValueError):
                r = float("nan")
            if not np.isfinite(r) or not (0.0 < r <= v):
                raise ValueError(f"{fn}: map_normal_radius must be a finite number in (0, voxel_size], got {map_normal_radius!r}")
            if not isinstance(map_normal_min_neighbors, (int, np.integer)) or isinstance(map_normal_min_neighbors, bool) or map_normal_min_neighbors < 3:
                raise ValueError(f"{fn}: map_normal_min_neighbors must be an integer of at least 3, got {map_normal_min_neighbors!r}")

    def check_scan(k, s):
        if not isinstance(s, PointCloud) or len(s) == 0:
            raise RuntimeError(f"{fn}: scan {k} must be a PointCloud with at least one point")
        if plane and not map_normals and not s.has_normals():
            raise RuntimeError(f"{fn}: scan {k} has no normals (TransformationEstimationPointToPlane needs a map with normals; see scan_to_map_odometry_icp_map_normals)")
        if deskew and not s.has_times():
            raise RuntimeError(f"{fn}: scan {k} has no times (deskewing needs PointCloud.times on every scan)")

    prepare = None
    if deskew and motion_model == "constant_velocity":
        def prepare(k, s, poses):
            return s.deskew(np.linalg.inv(poses[-2]) @ poses[-1]) if k >= 2 else s

    def register(s, m, start):
        if adaptive_threshold is None:
            return registration_point_map(s, m, max_correspondence_distance, None, start, estimation_method, criteria, neighborhood, max_points_per_voxel)
        sigma = adaptive_threshold.sigma
        est = TransformationEstimationPointToPlane(GMLoss(sigma / 3.0)) if plane else TransformationEstimationPointToPoint(False, GMLoss(sigma / 3.0))
        res = registration_point_map(s, m, 3.0 * sigma, None, start, est, criteria, neighborhood, max_points_per_voxel)
        adaptive_threshold.update(start, res.transformation)
        return res

    def make_map(s, g, P0):
        if not map_normals:
            return VoxelPointMap.on_grid(s, voxel_size, max_points_per_voxel, g, P0)
        bare = PointCloud()
        bare._xyz = s.device_xyz()
        m = VoxelPointMap.on_grid(bare, voxel_size, max_points_per_voxel, g, P0)
        try:
            m.estimate_normals(map_normal_radius, map_normal_min_neighbors)
        except BaseException:
            m.close()
            raise
        return m

    return _scan_to_map(fn, scans, voxel_size, init, motion_model, max_range, grid_min, check_rule, check_scan, make_map, register, prepare)


def scan_to_map_odometry_icp_deskew(scans, voxel_size, max_correspondence_distance=None, init=np.eye(4), estimation_method=None, criteria=None, neighborhood: int = 27,
                                    max_points_per_voxel: int = 20, motion_model: str = "constant_velocity", max_range=None, grid_min=None, adaptive_threshold=None,
                                    map_normals: bool = False, map_normal_radius=None, map_normal_min_neighbors: int = 5):
    """``scan_to_map_odometry_icp`` (``map_normals=False``) or ``scan_to_map_odometry_icp_map_normals`` (``True``) WITH deskewing -- KISS-ICP's
    whole recipe -> ``(poses, results, map)``.  Every scan must carry times.  Under ``"constant_velocity"`` scan k >= 2 is replaced by
    ``scans[k].deskew(inv(poses[k - 2]) @ poses[k - 1])`` -- the motion of the sweep before, taken as the motion of this one, with the end of
    the sweep as the reference -- before it is registered and inserted; scans 0 and 1, and every scan under ``"static"``, are taken as they
    are.  Everything else is the recipe of the function it extends, call by call.  It is a function of its own so that the two others keep
    their signatures."""
    fn = "scan_to_map_odometry_icp_deskew"
    est = estimation_method
    if map_normals and est is None:
        est = TransformationEstimationPointToPlane()
    return _scan_to_map_odometry_icp(fn, scans, voxel_size, max_correspondence_distance, init, est, criteria, neighborhood, max_points_per_voxel, motion_model, max_range,
                                     grid_min, adaptive_threshold, bool(map_normals), map_normal_radius, map_normal_min_neighbors, deskew=True)


def scan_to_map_odometry_ct(scans, voxel_size, max_correspondence_distance, init=np.eye(4), estimation_method=None, criteria=None, neighborhood: int = 27,
                            max_points_per_voxel: int = 20, max_range=None, grid_min=None, begin: str = "fixed", begin_prior_weight=None):
    """LiDAR odometry by continuous-time scan-to-map ICP on a ``VoxelPointMap`` -> ``(begin_poses, end_poses, results, map)``.  Every scan
    from the second on must carry times.  Exactly these public calls, in this order:

    * ``map = VoxelPointMap.on_grid(scans[0], voxel_size, max_points_per_voxel, grid_min, init)`` -- scan 0 as it is; ``grid_min=None`` is
      ``centered_grid_min`` of scan 0's centre placed at ``init``; ``begin_poses[0] = end_poses[0] = init``, ``results[0] = None``;
    * for every further scan k: ``T_b = end_poses[k - 1]`` and ``T_e = end_poses[k - 1] @ inv(begin_poses[k - 1]) @ end_poses[k - 1]`` (for
      k = 1 that is ``T_b``), then ``results[k] = registration_point_map_continuous(scans[k], map, max_correspondence_distance, T_b, T_e,
      None, estimation_method, criteria, neighborhood, max_points_per_voxel, begin, begin_prior_weight)``; ``begin_poses[k]`` and
      ``end_poses[k]`` are its poses (with ``begin="fixed"``, ``begin_poses[k]`` is ``end_poses[k - 1]`` bit for bit);
    * ``map.insert(scans[k].deskew(inv(begin_poses[k]) @ end_poses[k], reference=1.0), end_poses[k])``, and with a ``max_range``,
      ``map.remove_far(end_poses[k][:3, 3], max_range)``.

    Point to plane needs normals on every scan.  The caller owns the returned map and closes it."""
    fn = "scan_to_map_odometry_ct"
    _check_voxel_size(fn, voxel_size)
    _check_point_map_rule(fn, neighborhood, max_points_per_voxel)
    _check_distance(fn, max_correspondence_distance)
    est = _point_map_estimation(fn, estimation_method)
    _check_ct_begin(fn, begin, begin_prior_weight)
    if max_range is not None and (not np.isfinite(float(max_range)) or not float(max_range) > 0.0):
        raise ValueError(f"{fn}: max_range must be a finite number greater than 0, got {max_range!r}")
    scans = list(scans)
    if not scans:
        raise ValueError(f"{fn}: at least one scan is needed")
    for k, s in enumerate(scans):
        if not isinstance(s, PointCloud) or len(s) == 0:
            raise RuntimeError(f"{fn}: scan {k} must be a PointCloud with at least one point")
        if k and not s.has_times():
            raise RuntimeError(f"{fn}: scan {k} has no times (PointCloud.times)")
        if est.kind == _lib.EST_POINT_TO_PLANE and not s.has_normals():
            raise RuntimeError(f"{fn}: scan {k} has no normals (TransformationEstimationPointToPlane needs a map with normals)")
    P0 = _ct_pose(fn, "init", init)
    if grid_min is None:
        c = np.asarray(scans[0].get_center(), np.float64).reshape(3)
        grid_min = _GrowingVoxelMap.centered_grid_min(P0[:3, :3] @ c + P0[:3, 3], voxel_size)
    gmap = VoxelPointMap.on_grid(scans[0], voxel_size, max_points_per_voxel, grid_min, P0)
    begins, ends, results = [P0], [P0], [None]
    try:
        for k in range(1, len(scans)):
            T_b = ends[-1]
            T_e = ends[-1] @ np.linalg.inv(begins[-1]) @ ends[-1] if k > 1 else T_b
            res = registration_point_map_continuous(scans[k], gmap, max_correspondence_distance, T_b, T_e, None, estimation_method, criteria, neighborhood,
                                                    max_points_per_voxel, begin, begin_prior_weight)
            begins.append(res.begin_pose); ends.append(res.end_pose); results.append(res)
            gmap.insert(scans[k].deskew(np.linalg.inv(res.begin_pose) @ res.end_pose, reference=1.0), res.end_pose)
            if max_range is not None:
                gmap.remove_far(res.end_pose[:3, 3], max_range)
    except BaseException:
        gmap.close()
        raise
    return begins, ends, results, gmap


def multiscale_gicp(source: PointCloud, target: PointCloud, voxel_sizes, max_correspondence_distances, init=np.eye(4),
                    estimation_method=None, criteria=None, nb_neighbors: int = 30, std_ratio: float = 1.0,
                    normal_knn: int = 20) -> RegistrationResult:
    """Device-resident body of the reference's ``Multiscale_GICP`` loops (one C-ABI call for all scales)."""
    estimation = estimation_method or TransformationEstimationForGeneralizedICP()
    criteria = criteria or ICPConvergenceCriteria()
    ctx = _lib.Context.current()
    torch = _torch()
    vox = np.ascontiguousarray(np.asarray(voxel_sizes, dtype=np.float64).reshape(-1))
    dst = np.ascontiguousarray(np.asarray(max_correspondence_distances, dtype=np.float64).reshape(-1))
    if vox.size != dst.size or vox.size < 1:
        raise RuntimeError("multiscale_gicp: voxel_sizes and max_correspondence_distances must have the same length >= 1")
    ns, nt = len(source), len(target)
    recs = (_lib.PcrScaleRecord * vox.size)()
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    T, Tp = _T(init)
    p = _params(estimation, criteria)
    sn = source.device_normals() if source.has_normals() else None
    tn = target.device_normals() if target.has_normals() else None
    ctx.check(ctx.lib.pcr_multiscale_gicp(
        ctx.handle, _ptr(source.device_xyz()), _ptr(sn), C.c_int64(ns), _ptr(target.device_xyz()), _ptr(tn), C.c_int64(nt),
        vox.ctypes.data_as(C.POINTER(C.c_double)), dst.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(vox.size),
        C.c_int(nb_neighbors), C.c_double(std_ratio), C.c_int(normal_knn), Tp, C.byref(p), recs, _ptr(corr)),
        "multiscale_gicp")
    scales = _scale_dicts(recs, vox, dst)
    return _result(recs[vox.size - 1].icp, corr, scales)


_fgr_seed_counter = [0x9E3779B97F4A7C15]


def _scale_dicts(recs, vox, dst):
    return [dict(voxel=float(vox[i]), max_dist=float(dst[i]), n_voxel=tuple(recs[i].n_voxel), n_clean=tuple(recs[i].n_clean),
                 iterations=int(recs[i].icp.iterations), fitness=recs[i].icp.fitness, inlier_rmse=recs[i].icp.inlier_rmse,
                 converged=bool(recs[i].icp.converged), n_corr=int(recs[i].icp.n_correspondences),
                 T=np.array(recs[i].icp.transformation).reshape(4, 4)) for i in range(len(vox))]


def _fgr_params(voxel_size: float, use_absolute_scale: bool, n_pontos: int, seed) -> _lib.PcrFgrParams:
    """The constants of ``registro_FGR`` (ALL_FUNCTIONS.py:181-196 / 1_FGR...py:44-59) for one voxel size."""
    if seed is None:                       # Open3D draws from std::random_device; here a process-local counter
        _fgr_seed_counter[0] = (_fgr_seed_counter[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        seed = _fgr_seed_counter[0]
    opt = _lib.PcrFgrOption(1.4, int(bool(use_absolute_scale)), 1, 2 * voxel_size, 300, 0.95, -1 if n_pontos is None else int(n_pontos * 0.2), 1, int(seed) & (2 ** 64 - 1))
    return _lib.PcrFgrParams(2 * voxel_size, 20, 10 * voxel_size, 200, opt)


def registro_fgr(source: PointCloud, target: PointCloud, voxel_size: float, use_absolute_scale: bool = True, seed=None) -> RegistrationResult:
    """``registro_FGR`` (ALL_FUNCTIONS.py:178-203; script 1:41-66 with ``use_absolute_scale=False``) as ONE library call:
    hybrid normals, FPFH, feature matching, tuple test, GNC optimisation and the final evaluation, every cloud sorted and
    indexed once.  Like the reference it leaves normals on ``source`` and ``target``."""
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    fp = _fgr_params(voxel_size, use_absolute_scale, int((ns + nt) / 2), seed)
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    sno = torch.empty((max(ns, 1), 3), dtype=torch.float32, device="cuda")
    tno = torch.empty((max(nt, 1), 3), dtype=torch.float32, device="cuda")
    res = _lib.PcrResult()
    ctx.check(ctx.lib.pcr_registro_fgr(ctx.handle, _ptr(source.device_xyz()), _ptr(source.device_normals() if source.has_normals() else None), C.c_int64(ns),
                                       _ptr(target.device_xyz()), _ptr(target.device_normals() if target.has_normals() else None), C.c_int64(nt),
                                       C.byref(fp), _ptr(sno), _ptr(tno), C.byref(res), _ptr(corr)), "registro_FGR")
    if ns:
        source._nrm = sno[:ns]
    if nt:
        target._nrm = tno[:nt]
    return _result(res, corr)


def default_group(points_per_cloud: float) -> int:
    """Pairs per lockstep GICP group for clouds of this size: about 1.2M points per group, at most 8 (the by-value argument batch
    of ``k_icp_fused_b``; larger groups take the by-pointer kernel) -- 24 up to 40k points per cloud (round 5, below).  Measured on one
    MI355X, 4 groups in flight, 3-scale GICP stage, pair by pair -> groups: 200k-point pairs 340 -> 530 pairs/s (groups of 6), 100k
    440 -> 850 (8), 50k 540 -> 1360 (8) (round 3/4 numbers; HISTORY.md)."""
    if points_per_cloud >= 400_000:           # PCR_GROUP_FORMS_MAX_POINTS: such pairs run one by one with the single-pair kernel forms
        return 1
    g = int(round(1_200_000 / max(float(points_per_cloud), 1.0)))
    # Round 5: up to 24 pairs (the library's limit) for clouds up to 40k points -- the reference's NCLT scans.  The by-pointer kernel of groups beyond 8
    # holds 117 VGPRs now (146 before: one workgroup per CU, which is why 8 was the rule) and such pairs take 512-point tiles: script-2 stage on the
    # shipped-size scans, tiled and in three random orders, 8 / 12 / 16 / 24 pairs x 4 groups in flight = 1970 / 2530 / 2390 / 2920 pairs/s
    # (tools/gicp_nclt_sweep.py).  From 50k points the group size makes no difference (8 / 12 / 24: 1892 / 1874 / 1918 pairs/s at 50k, 1197 / 1199 / 1196 at 100k).
    return max(1, min(24 if points_per_cloud <= 40_000 else 8, g))


def default_fgr_group(points_per_cloud: float) -> int:
    """Pairs per lockstep ``registro_FGR`` group (``pcr_pairs_plan.fgr_group``): NCLT-size pairs are ~125 small dependent launches and 8
    host waits each, which a group shares (24 pairs up to 30k points per cloud -- measured on the shipped-size NCLT scans with the K = 64
    feature screen: 8 / 12 / 16 / 24 pairs x 4 groups in flight = 1762 / 1775 / 1841 / 1885 pairs/s; 16 at 20k-40k by the older rule); from ~70k
    points the tile-pruned feature search takes over and pairs run one by one."""
    if points_per_cloud >= 70_000:
        return 1
    if points_per_cloud <= 30_000:
        return 24
    return max(1, min(16, int(round(320_000 / max(float(points_per_cloud), 1.0)))))


def balanced_group(group: int, n_pairs: int, inflight: int) -> int:
    """Group size near ``group`` for which the groups of a batch of ``n_pairs`` fill whole rounds of ``inflight`` workers: 96 pairs in
    groups of 16 are 6 groups -- a round of 4 and a round of 2 -- in groups of 12 they are two full rounds (NCLT-size pairs, 5-scale
    GICP stage: 1930 -> 2138 pairs/s)."""
    if group <= 1 or inflight <= 1 or n_pairs <= group * inflight:
        return max(1, group)
    n_groups = -(-n_pairs // group)
    n_groups = -(-n_groups // inflight) * inflight
    return max(1, -(-n_pairs // n_groups))


def register_pairs_plan(pairs, stage: str = "gicp", voxel_sizes=None, max_correspondence_distances=None, estimation_method=None, criteria=None,
                        nb_neighbors: int = 30, std_ratio: float = 1.0, normal_knn: int = 20, inflight: int = 3, with_correspondences: bool = True,
                        fgr_voxel_size: float = 0.1, fgr_use_absolute_scale: bool = True, fgr_seed=None, radius_rule: str = "given",
                        prior_from_fgr: bool = False, info_max_dist: float = 0.0, keep_fgr_normals: bool = False, group=1, pair_forms=None, fgr_group=None) -> list:
    """The per-pair loops of the reference as ONE library call (``pcr_register_pairs_plan``): `pairs` = [(source PointCloud,
    target PointCloud, initial 4x4 or None), ...].

    stage "fgr"       = script 1 (1_FGR...py:134-147): ``registro_FGR`` per pair;
    stage "gicp"      = script 2 (2_MGICP...py:187-214): ``Multiscale_GICP`` from the given initial pose;
    stage "fgr+gicp"  = ``Coarse_to_fine_FGR_M_GICP`` / ``full_registration`` (ALL_FUNCTIONS.py:317-332, 349-392).
    radius_rule "af"  = search radii ``radius_from_cloud_pair * 2**-i`` per pair (ALL_FUNCTIONS.py:277-278) instead of the given list.
    ``group`` > 1 (stages "gicp" and "fgr+gicp"): that many consecutive pairs run in LOCKSTEP through the same GICP launches (preprocessing
    batched over clouds and scales, one GICP loop per scale for the whole group; same per-pair arithmetic; with "fgr+gicp" the worker runs
    registro_FGR pair by pair first); ``inflight`` counts groups.
    ``group=None`` picks by cloud size (``default_group``).
    ``fgr_group`` (stages with FGR; None = ``default_fgr_group`` of the mean cloud size, 1 = pair by pair): that many consecutive pairs go
    through ``registro_FGR`` in lockstep (``pcr_pairs_plan.fgr_group``); the same bits per pair either way.
    ``pair_forms`` (default: on exactly when ``group`` is None): the kernel forms of the GICP stage go by the PAIR alone
    (``pcr_pairs_plan.pair_forms``), so a pair's pose bits are the same in every batch, group size and shard of a multi-GPU run.
    The library keeps ``inflight`` pairs in flight on the current device.  Returns RegistrationResults in input order (for
    stages with FGR the FGR result is attached as ``.fgr``; ``.information`` when ``info_max_dist > 0``)."""
    estimation = estimation_method or TransformationEstimationForGeneralizedICP()
    criteria = criteria or ICPConvergenceCriteria()
    torch = _torch()
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible to torch: the MI355X registration path cannot run (no CPU fallback)")
    stage_id = {"gicp": _lib.STAGE_GICP, "fgr": _lib.STAGE_FGR, "fgr+gicp": _lib.STAGE_FGR_GICP}[stage]
    do_fgr, do_gicp = stage_id != _lib.STAGE_GICP, stage_id != _lib.STAGE_FGR
    vox = np.ascontiguousarray(np.asarray(voxel_sizes if voxel_sizes is not None else [], dtype=np.float64).reshape(-1))
    rule = {"given": 0, "af": 1}[radius_rule]
    dst = np.ascontiguousarray(np.asarray(max_correspondence_distances if max_correspondence_distances is not None else np.zeros(vox.size), dtype=np.float64).reshape(-1))
    if do_gicp and (vox.size < 1 or vox.size > 8 or dst.size != vox.size):
        raise RuntimeError("register_pairs: voxel_sizes and max_correspondence_distances must have the same length (1..8)")
    n = len(pairs)
    if n == 0:
        return []
    if pair_forms is None:
        pair_forms = group is None
    if fgr_group is None:
        fgr_group = default_fgr_group(float(np.mean([len(s_) + len(t_) for s_, t_, _ in pairs])) / 2) if do_fgr else 1
        if stage == "fgr":
            fgr_group = balanced_group(fgr_group, n, int(inflight))
    if group is None:
        mean_pts = float(np.mean([len(s_) + len(t_) for s_, t_, _ in pairs])) / 2
        group = balanced_group(default_group(mean_pts), n, int(inflight))
    # FGR groups and GICP groups of the same size (NCLT-size clouds: 24 and 24): ONE library call, every worker runs registro_FGR and the GICP of
    # its group back to back -- the same poses, 1170 -> 1220 pairs/s on the shipped scans (PCR_PLAN_ONE_CALL=0: two passes as below)
    import os as _os
    one_call = (fgr_group == group and _os.environ.get("PCR_PLAN_ONE_CALL", "1") != "0") or _os.environ.get("PCR_PLAN_ONE_CALL") == "2"
    if stage == "fgr+gicp" and group > 1 and n > 1 and not one_call:
        # Two passes over the batch instead of FGR -> GICP pair by pair: registro_FGR is a chain of ~150 small launches with a few host
        # waits and wants MANY pairs in flight (20k-point pairs: 230 / 590 / 700 pairs/s with 1 / 4 / 8), the GICP wants lockstep groups.
        # Same arithmetic as the single call (same seeds per pair, the FGR normals as the orientation prior, the same radius rule).
        def view(pc):                         # a cloud object of our own on the caller's tensors: the FGR normals land here, not on the caller's cloud
            v = PointCloud(); v._xyz = pc.device_xyz(); v._nrm = pc.device_normals() if pc.has_normals() else None
            return v
        views = [(view(s_), view(t_), None) for s_, t_, _ in pairs]
        fg = register_pairs_plan(views, "fgr", None, None, estimation, criteria, nb_neighbors, std_ratio, normal_knn, max(int(inflight), 8) if fgr_group <= 1 else max(int(inflight), 4), False,
                                 fgr_voxel_size, fgr_use_absolute_scale, fgr_seed, "given", False, 0.0, True, 1, fgr_group=fgr_group)
        second = [((vs if prior_from_fgr else s_), (vt if prior_from_fgr else t_), f.transformation) for (vs, vt, _), (s_, t_, _), f in zip(views, pairs, fg)]
        out = register_pairs_plan(second, "gicp", voxel_sizes, max_correspondence_distances, estimation, criteria, nb_neighbors, std_ratio, normal_knn, inflight,
                                  with_correspondences, radius_rule=radius_rule, info_max_dist=info_max_dist, group=group, pair_forms=pair_forms)
        for r, f, (vs, vt, _), (s_, t_, _) in zip(out, fg, views, pairs):
            r.fgr = f
            if keep_fgr_normals:              # the reference's side effect: both inputs gain normals
                if len(s_):
                    s_._nrm = vs._nrm
                if len(t_):
                    t_._nrm = vt._nrm
        return out
    arr = (_lib.PcrPairEx * n)()
    keep = []                                   # device tensors and record arrays must outlive the call
    # the correspondence sets of the batch in ONE allocation (a view per pair): 48 allocator calls per bench step were a third of the ~1 ms a step
    # spent outside the library call
    corr_rows = [max(len(src), 1) for src, _, _ in pairs]
    corr_all = torch.empty((sum(corr_rows), 2), dtype=torch.int32, device="cuda") if with_correspondences else None
    corr_off = 0
    for k, (src, tgt, init) in enumerate(pairs):
        recs = (_lib.PcrScaleRecord * max(vox.size, 1))()
        corr = corr_all[corr_off: corr_off + corr_rows[k]] if with_correspondences else None
        corr_off += corr_rows[k]
        sx, tx = src.device_xyz(), tgt.device_xyz()
        sn = src.device_normals() if src.has_normals() else None
        tn = tgt.device_normals() if tgt.has_normals() else None
        sno = torch.empty((max(len(src), 1), 3), dtype=torch.float32, device="cuda") if (do_fgr and keep_fgr_normals) else None
        tno = torch.empty((max(len(tgt), 1), 3), dtype=torch.float32, device="cuda") if (do_fgr and keep_fgr_normals) else None
        keep.append((recs, corr, sx, tx, sn, tn, sno, tno))
        a = arr[k].base
        a.src_xyz = sx.data_ptr(); a.src_normals = sn.data_ptr() if sn is not None else None; a.n_src = len(src)
        a.tgt_xyz = tx.data_ptr(); a.tgt_normals = tn.data_ptr() if tn is not None else None; a.n_tgt = len(tgt)
        a.init_T[:] = list(np.asarray(np.eye(4) if init is None else init, dtype=np.float64).reshape(16))
        a.records = C.cast(recs, C.POINTER(_lib.PcrScaleRecord)); a.correspondences = corr.data_ptr() if corr is not None else None
        arr[k].src_normals_out = sno.data_ptr() if sno is not None else None
        arr[k].tgt_normals_out = tno.data_ptr() if tno is not None else None
    p = _params(estimation, criteria)
    plan = _lib.PcrPairsPlan()
    plan.stage = stage_id
    fp = None
    if do_fgr:
        # maximum_tuple_count = int(0.2 * n_pontos) depends on the pair's sizes (ALL_FUNCTIONS.py:179,196): the library applies the rule per pair
        n_pontos = None
        fp = _fgr_params(fgr_voxel_size, fgr_use_absolute_scale, n_pontos, fgr_seed)
        plan.fgr = C.pointer(fp)
    plan.voxel_sizes = vox.ctypes.data_as(C.POINTER(C.c_double)); plan.max_distances = dst.ctypes.data_as(C.POINTER(C.c_double))
    plan.n_scales = int(vox.size); plan.radius_rule = rule
    plan.sor_k = int(nb_neighbors); plan.sor_std = float(std_ratio); plan.normal_k = int(normal_knn)
    plan.gicp = C.pointer(p); plan.gicp_prior_from_fgr = int(bool(prior_from_fgr)); plan.info_max_dist = float(info_max_dist); plan.inflight = int(inflight); plan.group = int(group); plan.pair_forms = int(pair_forms); plan.fgr_group = int(fgr_group)
    dev = torch.cuda.current_device()
    rc = lib.pcr_register_pairs_plan(C.c_int(dev), arr, C.c_int(n), C.byref(plan), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    out = []
    empty = torch.empty((0, 2), dtype=torch.int32, device="cuda")
    for k in range(n):
        b = arr[k].base
        if b.status != 0:
            raise RuntimeError(f"register_pairs: pair {k} failed with code {b.status}: {b.error.decode(errors='replace')}")
        recs, corr, sno, tno = keep[k][0], keep[k][1], keep[k][6], keep[k][7]
        if do_gicp:
            used = np.array(arr[k].max_distances[: vox.size]) if rule == 1 else dst
            r = _result(recs[vox.size - 1].icp, corr if corr is not None else empty, _scale_dicts(recs, vox, used))
        else:
            r = _result(arr[k].fgr, corr if corr is not None else empty)
        if do_fgr:
            r.fgr = _result(arr[k].fgr, None)
            if keep_fgr_normals:              # the reference's side effect: both inputs gain normals
                src, tgt, _ = pairs[k]
                if len(src):
                    src._nrm = sno[: len(src)]
                if len(tgt):
                    tgt._nrm = tno[: len(tgt)]
        if info_max_dist > 0:
            r.information = np.array(arr[k].info36, dtype=np.float64).reshape(6, 6)
        out.append(r)
    if rc != 0:
        raise RuntimeError(f"register_pairs failed with code {rc}")
    return out


def register_pairs(pairs, voxel_sizes, max_correspondence_distances, estimation_method=None, criteria=None, nb_neighbors: int = 30,
                   std_ratio: float = 1.0, normal_knn: int = 20, inflight: int = 3, with_correspondences: bool = True, group=1) -> list:
    """The per-pair loop of script 2 (2_MGICP...py:187-214) as ONE library call: every pair gets the body of ``multiscale_gicp``
    from its initial pose; see ``register_pairs_plan``."""
    return register_pairs_plan(pairs, "gicp", voxel_sizes, max_correspondence_distances, estimation_method, criteria, nb_neighbors, std_ratio,
                               normal_knn, inflight, with_correspondences, group=group)


def evaluate_registration(source: PointCloud, target: PointCloud, max_correspondence_distance: float,
                          transformation=np.eye(4)) -> RegistrationResult:
    ctx = _lib.Context.current()
    torch = _torch()
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    ns, nt = len(source), len(target)
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res = _lib.PcrResult()
    T, Tp = _T(transformation)
    ctx.check(ctx.lib.pcr_evaluate_registration(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), _ptr(target.device_xyz()),
                                                C.c_int64(nt), C.c_double(max_correspondence_distance), Tp, C.byref(res),
                                                _ptr(corr)), "evaluate_registration")
    return _result(res, corr)


def get_information_matrix_from_point_clouds(source: PointCloud, target: PointCloud, max_correspondence_distance: float,
                                             transformation) -> np.ndarray:
    ctx = _lib.Context.current()
    info = np.zeros(36, dtype=np.float64)
    T, Tp = _T(transformation)
    ctx.check(ctx.lib.pcr_information_matrix(ctx.handle, _ptr(source.device_xyz()), C.c_int64(len(source)),
                                             _ptr(target.device_xyz()), C.c_int64(len(target)),
                                             C.c_double(max_correspondence_distance), Tp,
                                             info.ctypes.data_as(C.POINTER(C.c_double))), "get_information_matrix_from_point_clouds")
    return info.reshape(6, 6)


def compute_fpfh_feature(cloud: PointCloud, search_param) -> Feature:
    ctx = _lib.Context.current()
    torch = _torch()
    if not cloud.has_normals():
        raise RuntimeError("Failed because input point cloud has no normal.")
    kind, knn, radius = search_param._spec()
    n = len(cloud)
    feat = torch.zeros((max(n, 1), 33), dtype=torch.float32, device="cuda")
    ctx.check(ctx.lib.pcr_compute_fpfh_feature(ctx.handle, _ptr(cloud.device_xyz()), _ptr(cloud.device_normals()), C.c_int64(n),
                                               C.c_int(kind), C.c_int(knn), C.c_double(radius), _ptr(feat)), "compute_fpfh_feature")
    return Feature(feat[:n].contiguous())


def _fgr_option(option) -> _lib.PcrFgrOption:
    option = option or FastGlobalRegistrationOption()
    seed = option.seed
    if seed is None:                       # Open3D draws from std::random_device; here a process-local counter
        _fgr_seed_counter[0] = (_fgr_seed_counter[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        seed = _fgr_seed_counter[0]
    return _lib.PcrFgrOption(option.division_factor, int(option.use_absolute_scale), int(option.decrease_mu),
                             option.maximum_correspondence_distance, option.iteration_number, option.tuple_scale,
                             option.maximum_tuple_count, int(option.tuple_test), int(seed))


def registration_fgr_based_on_feature_matching(source: PointCloud, target: PointCloud, source_feature: Feature,
                                               target_feature: Feature, option: FastGlobalRegistrationOption | None = None):
    ctx = _lib.Context.current()
    torch = _torch()
    o = _fgr_option(option)
    ns, nt = len(source), len(target)
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res = _lib.PcrResult()
    ctx.check(ctx.lib.pcr_registration_fgr(ctx.handle, _ptr(source.device_xyz()), _ptr(source_feature._dev), C.c_int64(ns),
                                           _ptr(target.device_xyz()), _ptr(target_feature._dev), C.c_int64(nt), C.byref(o),
                                           C.byref(res), _ptr(corr)), "registration_fgr_based_on_feature_matching")
    return _result(res, corr)


def registration_fgr_based_on_correspondence(source: PointCloud, target: PointCloud, corres, option: FastGlobalRegistrationOption | None = None):
    """Open3D ``registration_fgr_based_on_correspondence``: fast global registration on a list of (source index, target index) rows the
    caller holds -- ``correspondences_from_features`` gives the one the feature form builds -- instead of on features
    (``pcr_registration_fgr_correspondence``, include/pcr_hip.h).  With ``option.tuple_test`` the tuple test draws from the list in its
    given order; without it every row goes to the optimiser.  The result is ``evaluate_registration`` under the pose found."""
    o = _fgr_option(option)
    ns, nt = len(source), len(target)
    cd = _corres_device("registration_fgr_based_on_correspondence", corres, ns, nt)
    ctx = _lib.Context.current()
    torch = _torch()
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res = _lib.PcrResult()
    ctx.check(ctx.lib.pcr_registration_fgr_correspondence(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), _ptr(target.device_xyz()), C.c_int64(nt),
                                                          _ptr(cd), C.c_int64(int(cd.shape[0])), C.byref(o), C.byref(res), _ptr(corr)),
              "registration_fgr_based_on_correspondence")
    return _result(res, corr)


def correspondences_from_features(source_features: Feature, target_features: Feature, mutual_filter: bool = False, mutual_consistency_ratio: float = 0.1):
    """Open3D ``correspondences_from_features`` (0.17 and later): every source feature row paired with its nearest target row -- float64
    distance, ties to the smaller index --, in source order; with ``mutual_filter`` only the rows whose target row points back, unless fewer
    than ``int(mutual_consistency_ratio * n_source)`` remain (then all rows).  Returns a device int32 tensor (M, 2) that
    ``registration_ransac_based_on_correspondence``, ``registration_fgr_based_on_correspondence`` and the estimators' methods take as it
    is; ``.cpu().numpy()`` gives Open3D's array."""
    if source_features.dimension() != target_features.dimension():
        raise RuntimeError("correspondences_from_features: the two feature sets have different dimensions")
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = source_features.num(), target_features.num()
    out = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    n = C.c_int64(0)
    ctx.check(ctx.lib.pcr_correspondences_from_features(ctx.handle, _ptr(source_features._dev.contiguous()), C.c_int64(ns), _ptr(target_features._dev.contiguous()),
                                                        C.c_int64(nt), C.c_int(source_features.dimension()), C.c_int(int(bool(mutual_filter))),
                                                        C.c_double(float(mutual_consistency_ratio)), _ptr(out), C.byref(n)), "correspondences_from_features")
    return out[: n.value]


class RANSACConvergenceCriteria:
    def __init__(self, max_iteration: int = 100000, confidence: float = 0.999):
        self.max_iteration = int(max_iteration)
        self.confidence = float(confidence)


class CorrespondenceChecker:
    """Base of the RANSAC pruning checks; ``require_pointcloud_alignment_`` as in Open3D (False: checked on the sample before the fit)."""
    require_pointcloud_alignment_ = True


class CorrespondenceCheckerBasedOnEdgeLength(CorrespondenceChecker):
    require_pointcloud_alignment_ = False

    def __init__(self, similarity_threshold: float = 0.9):
        self.similarity_threshold = float(similarity_threshold)


class CorrespondenceCheckerBasedOnDistance(CorrespondenceChecker):
    def __init__(self, distance_threshold: float):
        self.distance_threshold = float(distance_threshold)


class CorrespondenceCheckerBasedOnNormal(CorrespondenceChecker):
    def __init__(self, normal_angle_threshold: float):
        self.normal_angle_threshold = float(normal_angle_threshold)


def _ransac_params(fn, max_correspondence_distance, estimation_method, ransac_n, checkers, criteria, seed) -> _lib.PcrRansacParams:
    """Arguments of the two RANSAC entry points -> ``pcr_ransac_params``.  Several checkers of one kind act as their strictest member (a
    hypothesis has to pass all of them); a negative threshold tells the library that the checker is absent."""
    estimation = TransformationEstimationPointToPoint() if estimation_method is None else estimation_method
    if not isinstance(estimation, TransformationEstimationPointToPoint):
        raise RuntimeError(f"{fn}: {type(estimation).__name__} is not implemented on the MI355X path")
    if max_correspondence_distance <= 0:
        raise RuntimeError("Invalid max_correspondence_distance.")
    if not 3 <= int(ransac_n) <= 8:
        raise RuntimeError(f"{fn}: ransac_n must be in 3..8 (got {ransac_n})")
    criteria = criteria or RANSACConvergenceCriteria()
    if criteria.max_iteration < 0 or not 0.0 < criteria.confidence <= 1.0:
        raise RuntimeError(f"{fn}: RANSACConvergenceCriteria needs max_iteration >= 0 and 0 < confidence <= 1")
    edge, dist, ang = -1.0, -1.0, -1.0
    for c in checkers or ():
        if isinstance(c, CorrespondenceCheckerBasedOnEdgeLength):
            thr = c.similarity_threshold
            edge = max(edge, thr)
        elif isinstance(c, CorrespondenceCheckerBasedOnDistance):
            thr = c.distance_threshold
            dist = thr if dist < 0 else min(dist, thr)
        elif isinstance(c, CorrespondenceCheckerBasedOnNormal):
            thr = c.normal_angle_threshold
            ang = thr if ang < 0 else min(ang, thr)
        else:
            raise RuntimeError(f"{fn}: {type(c).__name__} is not implemented on the MI355X path")
        if not thr >= 0:
            raise RuntimeError(f"{fn}: negative threshold in {type(c).__name__}")
    if seed is None:                       # Open3D draws from std::random_device; here a process-local counter
        _fgr_seed_counter[0] = (_fgr_seed_counter[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        seed = _fgr_seed_counter[0]
    return _lib.PcrRansacParams(int(ransac_n), int(estimation.with_scaling), int(criteria.max_iteration), float(criteria.confidence),
                                int(seed) & (2 ** 64 - 1), edge, dist, ang)


def _ransac_result(res: _lib.PcrResult, info: _lib.PcrRansacInfo, corr) -> RegistrationResult:
    out = _result(res, corr)
    out.iterations = int(info.iterations_run)
    out.best_iteration = int(info.best_iteration)
    out.n_valid = int(info.n_valid)
    out.n_corres = int(info.n_corres)
    return out


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, estimation_method=None, ransac_n=3,
                                                checkers=[], criteria=None, seed=None):
    """Open3D ``registration_ransac_based_on_correspondence`` (0.13 and later): ``corres`` is (C, 2) rows of (source index, target index);
    fitness and RMSE of the result are taken over that list, ``correspondence_set`` holds its inlier rows.  The loop is the sequential one
    of include/pcr_hip.h (deterministic for a ``seed``; ``seed=None`` draws from a process-local counter).  The result also carries
    ``iterations`` (iterations run), ``best_iteration`` (-1: none), ``n_valid`` (hypotheses among those run that passed every checker) and
    ``n_corres`` (rows of the list), the fields of ``pcr_ransac_info``."""
    p = _ransac_params("registration_ransac_based_on_correspondence", max_correspondence_distance, estimation_method, ransac_n, checkers, criteria, seed)
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    cd = _corres_device("registration_ransac_based_on_correspondence", corres, ns, nt)
    nc = int(cd.shape[0])
    out = torch.empty((max(nc, 1), 2), dtype=torch.int32, device="cuda")
    res, info = _lib.PcrResult(), _lib.PcrRansacInfo()
    ctx.check(ctx.lib.pcr_registration_ransac_correspondence(
        ctx.handle, _ptr(source.device_xyz()), _ptr(source.device_normals() if source.has_normals() else None), C.c_int64(ns),
        _ptr(target.device_xyz()), _ptr(target.device_normals() if target.has_normals() else None), C.c_int64(nt), _ptr(cd), C.c_int64(nc),
        C.c_double(max_correspondence_distance), C.byref(p), C.byref(res), _ptr(out), C.byref(info)), "registration_ransac_based_on_correspondence")
    return _ransac_result(res, info, out)


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter, max_correspondence_distance,
                                                  estimation_method=None, ransac_n=3, checkers=[], criteria=None, seed=None):
    """Open3D ``registration_ransac_based_on_feature_matching`` (0.13 and later): every source point is paired with its nearest target point
    in feature space (with ``mutual_filter`` only the pairs whose target point points back, unless fewer than ``ransac_n`` remain), then
    ``registration_ransac_based_on_correspondence`` runs on that list (same extra result fields; ``n_corres`` is the length of the list built)."""
    p = _ransac_params("registration_ransac_based_on_feature_matching", max_correspondence_distance, estimation_method, ransac_n, checkers, criteria, seed)
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    if source_feature.num() != ns or target_feature.num() != nt:
        raise RuntimeError("registration_ransac_based_on_feature_matching: one feature row per point is required")
    out = torch.empty((max(ns, 1), 2), dtype=torch.int32, device="cuda")
    res, info = _lib.PcrResult(), _lib.PcrRansacInfo()
    ctx.check(ctx.lib.pcr_registration_ransac_feature_matching(
        ctx.handle, _ptr(source.device_xyz()), _ptr(source.device_normals() if source.has_normals() else None), C.c_int64(ns),
        _ptr(source_feature._dev), _ptr(target.device_xyz()), _ptr(target.device_normals() if target.has_normals() else None), C.c_int64(nt),
        _ptr(target_feature._dev), C.c_int(int(bool(mutual_filter))), C.c_double(max_correspondence_distance), C.byref(p), C.byref(res), _ptr(out),
        C.byref(info)), "registration_ransac_based_on_feature_matching")
    return _ransac_result(res, info, out)


SC2_MAX_CORRESPONDENCES = 65536


class SpatialCompatibilityOption:
    """Options of ``registration_sc2_based_on_correspondence`` (``pcr_sc2_option``, include/pcr_hip.h states the rule): ``inlier_threshold``
    is the compatibility tolerance and the inlier distance (no default), ``nms_radius`` the source-space radius inside which a better row
    suppresses a seed (``None``: ``inlier_threshold``), ``k1`` / ``k2`` the sizes of the two consensus stages of a seed, ``seed_ratio`` and
    ``max_seeds`` bound the seeds, ``refine_iterations`` the refits over the inlier rows."""

    def __init__(self, inlier_threshold, nms_radius=None, k1=30, k2=20, seed_ratio=0.2, max_seeds=2048, refine_iterations=20):
        self.inlier_threshold = float(inlier_threshold)
        self.nms_radius = None if nms_radius is None else float(nms_radius)
        self.k1 = int(k1)
        self.k2 = int(k2)
        self.seed_ratio = float(seed_ratio)
        self.max_seeds = int(max_seeds)
        self.refine_iterations = int(refine_iterations)


def _sc2_threshold(fn, tau):
    tau = float(tau)
    if not (tau > 0.0 and np.isfinite(tau)):
        raise RuntimeError(f"{fn}: inlier_threshold must be positive and finite (got {tau})")
    return tau


def _sc2_rows(fn, corres) -> int:
    """Rows of a caller's list, read from its shape alone; more than the limit is refused before anything touches a device."""
    shape = tuple(corres.shape) if hasattr(corres, "shape") else np.shape(corres)
    n = int(shape[0]) if len(shape) == 2 else int(np.prod(shape, dtype=np.int64)) // 2
    if n > SC2_MAX_CORRESPONDENCES:
        raise RuntimeError(f"{fn}: {n} correspondences, the limit is {SC2_MAX_CORRESPONDENCES} (the bit matrix would exceed 512 MB): use the mutual "
                           "filter of correspondences_from_features or a keypoint subset")
    return n


def _sc2_option(fn, option) -> _lib.PcrSc2Option:
    """``SpatialCompatibilityOption`` -> ``pcr_sc2_option``; every limit of the header raises here, from the arguments alone."""
    if not isinstance(option, SpatialCompatibilityOption):
        raise RuntimeError(f"{fn}: option must be a SpatialCompatibilityOption")
    tau = _sc2_threshold(fn, option.inlier_threshold)
    nms = tau if option.nms_radius is None else float(option.nms_radius)
    if not nms >= 0.0:
        raise RuntimeError(f"{fn}: nms_radius must be >= 0 (got {nms})")
    if not 2 <= option.k1 <= 63:
        raise RuntimeError(f"{fn}: k1 must be in 2..63 (got {option.k1})")
    if not 1 <= option.k2 <= option.k1:
        raise RuntimeError(f"{fn}: k2 must be in 1..k1 (got {option.k2})")
    if not 0.0 < option.seed_ratio <= 1.0:
        raise RuntimeError(f"{fn}: seed_ratio must be in (0, 1] (got {option.seed_ratio})")
    if not 1 <= option.max_seeds <= 65536:
        raise RuntimeError(f"{fn}: max_seeds must be in 1..65536 (got {option.max_seeds})")
    if option.refine_iterations < 0:
        raise RuntimeError(f"{fn}: refine_iterations must be >= 0 (got {option.refine_iterations})")
    return _lib.PcrSc2Option(tau, nms, option.k1, option.k2, option.seed_ratio, option.max_seeds, option.refine_iterations)


def registration_sc2_based_on_correspondence(source, target, corres, option):
    """Global registration on a correspondence list by second-order spatial compatibility (after SC2-PCR; include/pcr_hip.h states the
    rule): true matches preserve the distance between them AND share many other matches that do, so the second-order count separates
    inliers from outliers at inlier rates where sampling gives up.  Deterministic: no random numbers.  ``corres`` is (C, 2) rows of (source
    index, target index), at most 65536 of them; fitness and RMSE are taken over that list, ``correspondence_set`` holds its inlier rows in
    input order.  The result also carries ``info``: ``n_corres``, ``n_seeds``, ``n_valid``, ``best_seed``, ``best_seed_count``,
    ``refine_iterations_run`` (``pcr_sc2_info``).  Fewer than 3 rows or no valid seed: the empty result."""
    fn = "registration_sc2_based_on_correspondence"
    o = _sc2_option(fn, option)
    _sc2_rows(fn, corres)
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    cd = _corres_device(fn, corres, ns, nt)
    nc = int(cd.shape[0])
    out = torch.empty((max(nc, 1), 2), dtype=torch.int32, device="cuda")
    res, info = _lib.PcrResult(), _lib.PcrSc2Info()
    ctx.check(ctx.lib.pcr_registration_sc2_correspondence(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), _ptr(target.device_xyz()), C.c_int64(nt),
                                                          _ptr(cd), C.c_int64(nc), C.byref(o), C.byref(res), _ptr(out), C.byref(info)), fn)
    r = _result(res, out)
    r.info = {name: int(getattr(info, name)) for name, _ in _lib.PcrSc2Info._fields_}
    return r


def registration_sc2_based_on_feature_matching(source, target, source_feature, target_feature, option, mutual_filter=True, mutual_consistency_ratio=0.1):
    """``correspondences_from_features(source_feature, target_feature, mutual_filter, mutual_consistency_ratio)`` followed by
    ``registration_sc2_based_on_correspondence`` on that list."""
    fn = "registration_sc2_based_on_feature_matching"
    _sc2_option(fn, option)
    if source_feature.num() != len(source) or target_feature.num() != len(target):
        raise RuntimeError(f"{fn}: one feature row per point is required")
    corres = correspondences_from_features(source_feature, target_feature, mutual_filter, mutual_consistency_ratio)
    return registration_sc2_based_on_correspondence(source, target, corres, option)


class SpatialCompatibility:
    """The compatibility graph of a correspondence list (device tensors): ``bits`` (N, ceil(N / 64)) int64 -- bit b of word w of row i says
    that rows i and 64 w + b preserve their distance within the threshold --, ``degrees`` int32 (compatible rows per row) and ``scores`` int64
    (the second-order count: twice the triangles through the row)."""

    def __init__(self, bits, degrees, scores):
        self.bits, self.degrees, self.scores = bits, degrees, scores


def spatial_compatibility(source, target, corres, inlier_threshold) -> SpatialCompatibility:
    """First- and second-order spatial compatibility of a correspondence list (``pcr_spatial_compatibility``, include/pcr_hip.h): a row's
    degree or score is a filter on its own, e.g. before ``registration_fgr_based_on_correspondence``.  At most 65536 rows."""
    fn = "spatial_compatibility"
    tau = _sc2_threshold(fn, inlier_threshold)
    _sc2_rows(fn, corres)
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    cd = _corres_device(fn, corres, ns, nt)
    nc = int(cd.shape[0])
    bits = torch.zeros((nc, (nc + 63) // 64), dtype=torch.int64, device="cuda")
    deg = torch.zeros((nc,), dtype=torch.int32, device="cuda")
    score = torch.zeros((nc,), dtype=torch.int64, device="cuda")
    ctx.check(ctx.lib.pcr_spatial_compatibility(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), _ptr(target.device_xyz()), C.c_int64(nt), _ptr(cd),
                                                C.c_int64(nc), C.c_double(tau), _ptr(bits), _ptr(deg), _ptr(score)), fn)
    return SpatialCompatibility(bits, deg, score)


def debug_sc2_seeds(source, target, corres, option):
    """Test hook ``pcr_debug_sc2_seeds``: per seed, in order, its row, the rows of K1 and K2 (-1 padded to 64), the 4 x 4 hypothesis, validity,
    count and err2, as numpy arrays in a dict."""
    fn = "debug_sc2_seeds"
    o = _sc2_option(fn, option)
    n = _sc2_rows(fn, corres)
    ctx = _lib.Context.current()
    torch = _torch()
    ns, nt = len(source), len(target)
    cd = _corres_device(fn, corres, ns, nt)
    cap = max(1, min(max(1, int(o.seed_ratio * n)), o.max_seeds))
    dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    seed, k1, k2 = dev((cap,), torch.int32), dev((cap, 64), torch.int32), dev((cap, 64), torch.int32)
    T, valid, cnt, err2 = dev((cap, 4, 4), torch.float64), dev((cap,), torch.uint8), dev((cap,), torch.int32), dev((cap,), torch.float64)
    m = C.c_int64(0)
    ctx.check(ctx.lib.pcr_debug_sc2_seeds(ctx.handle, _ptr(source.device_xyz()), C.c_int64(ns), _ptr(target.device_xyz()), C.c_int64(nt), _ptr(cd),
                                          C.c_int64(int(cd.shape[0])), C.byref(o), C.byref(m), _ptr(seed), _ptr(k1), _ptr(k2), _ptr(T), _ptr(valid), _ptr(cnt),
                                          _ptr(err2)), fn)
    k = m.value
    return {"seeds": seed[:k].cpu().numpy(), "k1": k1[:k].cpu().numpy(), "k2": k2[:k].cpu().numpy(), "T": T[:k].cpu().numpy(),
            "valid": valid[:k].cpu().numpy().astype(bool), "count": cnt[:k].cpu().numpy(), "err2": err2[:k].cpu().numpy()}


# pose-graph slice of o3d.pipelines.registration (3_Global_Optimizations...py:292-358; host side, posegraph.py)
from .posegraph import (GlobalOptimizationConvergenceCriteria, GlobalOptimizationLevenbergMarquardt,  # noqa: E402,F401
                        GlobalOptimizationOption, PoseGraph, PoseGraphEdge, PoseGraphNode, global_optimization)
