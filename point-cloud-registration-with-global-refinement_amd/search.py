"""Nearest-neighbour search over a cloud with arbitrary query points: ``NearestNeighborSearch`` (``o3d.core.nns.NearestNeighborSearch``)
and ``KDTreeFlann`` (``o3d.geometry.KDTreeFlann``), on the persistent index of ``libpcr_hip.so`` (``pcr_index_*``, include/pcr_hip.h).

One result rule for every search: d² of a query and a dataset point is taken in float64 on the float32 coordinates (differences, squares
and sums in the order x, y, z, each rounded once), and the dataset is ordered for a query by (d², index), ascending.  ``knn`` gives the first
k of that order, ``radius`` every point with d² < radius², ``hybrid`` the first ``max_nn`` of the radius set.  A brute-force numpy
recomputation gives the same rows bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from . import geometry as _g

MAX_NN = 200          # bound of knn / max_knn / max_nn (the k-best structures of the library)


# ---- argument validation: before a context is created or the library is touched, so it runs on a machine without a GPU
def _check_count(name, value):
    try:
        k = int(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integer in 1..{MAX_NN}, got {value!r}") from None
    if k != value or k < 1 or k > MAX_NN:
        raise ValueError(f"{name} must be an integer in 1..{MAX_NN}, got {value!r}")
    return k


def _check_radius(value):
    try:
        r = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"radius must be a number greater than 0, got {value!r}") from None
    if not (r > 0.0) or math.isinf(r):
        raise ValueError(f"radius must be a finite number greater than 0, got {value!r}")
    return r


def _check_rows(name, a):
    """(m, 3) rows, or one point of 3 coordinates; returns the shape checked (no copy, no device)."""
    shape = tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape
    if len(shape) == 1 and shape[0] == 3:
        return (1, 3)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{name} must have shape (m, 3) (or (3,) for one point), got {shape}")
    return shape


def _rows_of(name, a):
    if isinstance(a, _g.PointCloud):
        return a.device_xyz()
    if _is_feature(a):
        raise TypeError(f"{name}: only 3-D point indices exist; the 33-D feature search stays inside registration_fgr_based_on_feature_matching and "
                        "registration_ransac_based_on_feature_matching")
    _check_rows(name, a)
    return a


def _is_feature(x):
    from .registration import Feature
    return isinstance(x, Feature)


class NearestNeighborSearch:
    """``o3d.core.nns.NearestNeighborSearch``: the index is built by the constructor and lives until ``close()``.

    ``dataset`` is a ``PointCloud``, an (n, 3) array or a device tensor; the index keeps its own copy, so the dataset may be changed
    afterwards.  Results are torch tensors on the device; the int64 indices feed ``PointCloud.select_by_index`` directly."""

    _handle = None

    def __init__(self, dataset):
        if _is_feature(dataset):
            raise TypeError("NearestNeighborSearch: only 3-D point indices exist; the 33-D feature search stays inside the FGR and RANSAC calls")
        rows = _rows_of("dataset", dataset)
        xyz = _g._dev_f32(rows, 3)
        ctx = _lib.Context.current()
        h = C.c_void_p()
        ctx.check(ctx.lib.pcr_index_create(ctx.handle, _g._ptr(xyz), C.c_int64(xyz.shape[0]), C.byref(h)), "NearestNeighborSearch")
        self._handle = h
        self._lib = ctx.lib
        self._device = ctx.device
        self.n = int(xyz.shape[0])

    # Open3D builds one index per search kind on request; here the one index serves all three and exists already
    def knn_index(self):
        return True

    def fixed_radius_index(self, radius=None):
        return True

    def hybrid_index(self, radius=None):
        return True

    def close(self):
        """Destroy the index (waits for the device)."""
        h, self._handle = self._handle, None
        if h is not None and h.value:
            self._lib.pcr_index_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n

    def _queries(self, queries):
        """-> (context, (m, 3) float32 device rows); raises after close()."""
        rows = _rows_of("queries", queries)
        if self._handle is None:
            raise RuntimeError("NearestNeighborSearch: the index is closed")
        q = _g._dev_f32(rows, 3)
        return _lib.Context.current(), q

    def knn_search(self, queries, knn):
        """-> (indices (m, min(knn, n)) int64, d² (m, min(knn, n)) float64), rows ordered by (d², index)."""
        k = _check_count("knn", knn)
        ctx, q = self._queries(queries)
        torch = _g._torch()
        m = q.shape[0]
        idx = torch.empty((m, k), dtype=torch.int32, device="cuda")
        d2 = torch.empty((m, k), dtype=torch.float64, device="cuda")
        ctx.check(ctx.lib.pcr_index_knn(ctx.handle, self._handle, _g._ptr(q), C.c_int64(m), C.c_int(k), _g._ptr(idx), _g._ptr(d2)), "knn_search")
        cols = min(k, self.n)
        return idx[:, :cols].to(torch.int64).contiguous(), d2[:, :cols].contiguous()

    def hybrid_search(self, queries, radius, max_knn):
        """-> (indices (m, max_knn) int64, d² (m, max_knn) float64, counts (m,) int32); places beyond the count hold -1 and 0."""
        r = _check_radius(radius)
        k = _check_count("max_knn", max_knn)
        ctx, q = self._queries(queries)
        torch = _g._torch()
        m = q.shape[0]
        idx = torch.empty((m, k), dtype=torch.int32, device="cuda")
        d2 = torch.empty((m, k), dtype=torch.float64, device="cuda")
        cnt = torch.empty((m,), dtype=torch.int32, device="cuda")
        ctx.check(ctx.lib.pcr_index_hybrid(ctx.handle, self._handle, _g._ptr(q), C.c_int64(m), C.c_double(r), C.c_int(k), _g._ptr(idx), _g._ptr(d2),
                                           _g._ptr(cnt)), "hybrid_search")
        return idx.to(torch.int64), d2, cnt

    def fixed_radius_search(self, queries, radius, sort=True):
        """-> (indices (T,) int64, d² (T,) float64, row_splits (m + 1,) int64): row i is [row_splits[i], row_splits[i + 1])."""
        r = _check_radius(radius)
        ctx, q = self._queries(queries)
        torch = _g._torch()
        m = q.shape[0]
        cnt = torch.empty((m,), dtype=torch.int32, device="cuda")
        ctx.check(ctx.lib.pcr_index_radius_count(ctx.handle, self._handle, _g._ptr(q), C.c_int64(m), C.c_double(r), _g._ptr(cnt)), "fixed_radius_search")
        splits = torch.zeros((m + 1,), dtype=torch.int64, device="cuda")
        if m > 0:
            splits[1:] = torch.cumsum(cnt.to(torch.int64), 0)
        total = int(splits[-1].item())
        idx = torch.empty((total,), dtype=torch.int32, device="cuda")
        d2 = torch.empty((total,), dtype=torch.float64, device="cuda")
        if total > 0:
            ctx.check(ctx.lib.pcr_index_radius_fill(ctx.handle, self._handle, _g._ptr(q), C.c_int64(m), C.c_double(r), _g._ptr(splits), _g._ptr(idx),
                                                    _g._ptr(d2), C.c_int(1 if sort else 0)), "fixed_radius_search")
        return idx.to(torch.int64), d2, splits


class KDTreeFlann:
    """``o3d.geometry.KDTreeFlann``: one-query calls of the batch searches on an index built once by ``set_geometry``.  Every search
    returns ``(count, indices numpy int32, d² numpy float64)`` like Open3D."""

    def __init__(self, geometry=None):
        self._nns = None
        if geometry is not None:
            self.set_geometry(geometry)

    def set_geometry(self, geometry):
        if _is_feature(geometry):
            raise TypeError("KDTreeFlann: only 3-D point indices exist; the 33-D feature search stays inside the FGR and RANSAC calls")
        old, self._nns = self._nns, NearestNeighborSearch(geometry)
        if old is not None:
            old.close()
        return True

    def set_feature(self, feature):
        raise TypeError("KDTreeFlann: only 3-D point indices exist; the 33-D feature search stays inside the FGR and RANSAC calls")

    def close(self):
        nns, self._nns = self._nns, None
        if nns is not None:
            nns.close()

    def _index(self):
        if self._nns is None:
            raise RuntimeError("KDTreeFlann: no geometry set")
        return self._nns

    @staticmethod
    def _one(query):
        if _is_feature(query):
            raise TypeError("KDTreeFlann: only 3-D point indices exist; the 33-D feature search stays inside the FGR and RANSAC calls")
        q = np.asarray(query, dtype=np.float64).reshape(-1)
        if q.shape != (3,):
            raise ValueError(f"query must be one point of 3 coordinates, got shape {np.asarray(query).shape}")
        return q.astype(np.float32).reshape(1, 3)

    def search_knn_vector_3d(self, query, knn):
        k = _check_count("knn", knn)
        q = self._one(query)
        idx, d2 = self._index().knn_search(q, k)
        idx = idx[0].cpu().numpy().astype(np.int32); d2 = d2[0].cpu().numpy()
        return int(idx.shape[0]), idx, d2

    def search_radius_vector_3d(self, query, radius):
        r = _check_radius(radius)
        q = self._one(query)
        idx, d2, _ = self._index().fixed_radius_search(q, r, sort=True)
        idx = idx.cpu().numpy().astype(np.int32); d2 = d2.cpu().numpy()
        return int(idx.shape[0]), idx, d2

    def search_hybrid_vector_3d(self, query, radius, max_nn):
        r = _check_radius(radius)
        k = _check_count("max_nn", max_nn)
        q = self._one(query)
        idx, d2, cnt = self._index().hybrid_search(q, r, k)
        c = int(cnt[0].item())
        return c, idx[0, :c].cpu().numpy().astype(np.int32), d2[0, :c].cpu().numpy()

    def search_vector_3d(self, query, search_param):
        if isinstance(search_param, _g.KDTreeSearchParamKNN):
            return self.search_knn_vector_3d(query, search_param.knn)
        if isinstance(search_param, _g.KDTreeSearchParamRadius):
            return self.search_radius_vector_3d(query, search_param.radius)
        if isinstance(search_param, _g.KDTreeSearchParamHybrid):
            return self.search_hybrid_vector_3d(query, search_param.radius, search_param.max_nn)
        raise ValueError(f"search_param must be a KDTreeSearchParamKNN, KDTreeSearchParamRadius or KDTreeSearchParamHybrid, got {type(search_param).__name__}")
