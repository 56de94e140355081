"""Place recognition with Scan Context (Kim and Kim, IROS 2018) on the device: the polar height image of a ring-LiDAR scan
(``scan_context``), a growing database of such images with the exact all-pairs search (``ScanContextDatabase``), and the loop closures it
finds in a trajectory (``detect_loop_closures``), ready for ``posegraph.loop_closure_edges``.  The rule -- bins, maxima, the column cosine
distance minimised over the circular shifts, the tie orders -- is stated in include/pcr_hip.h next to ``pcr_scan_context``; the kernels
(csrc/pcr_place.hip) give the bits of its numpy restatement.  The reference has no counterpart: its loop closures are known beforehand.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .geometry import PointCloud, _dev_f32, _ptr, _torch

MAX_RINGS, MAX_SECTORS = 64, 128


def _check_shape(fn: str, num_rings, num_sectors):
    R, S = int(num_rings), int(num_sectors)
    if R != num_rings or S != num_sectors:
        raise ValueError(f"{fn}: num_rings and num_sectors must be integers, got {num_rings!r}, {num_sectors!r}")
    if not 1 <= R <= MAX_RINGS:
        raise ValueError(f"{fn}: num_rings must be in 1..{MAX_RINGS}, got {R}")
    if not 4 <= S <= MAX_SECTORS or S % 4:
        raise ValueError(f"{fn}: num_sectors must be a multiple of 4 in 4..{MAX_SECTORS}, got {S}")
    return R, S


def _check_params(fn: str, num_rings, num_sectors, max_range, height_offset):
    R, S = _check_shape(fn, num_rings, num_sectors)
    L, h = float(max_range), float(height_offset)
    if not (math.isfinite(L) and L > 0.0):
        raise ValueError(f"{fn}: max_range must be finite and > 0, got {max_range!r}")
    if not (math.isfinite(h) and np.isfinite(np.float32(h))):
        raise ValueError(f"{fn}: height_offset must be finite, got {height_offset!r}")
    return R, S, L, h


def scan_context_tables(num_rings: int, num_sectors: int, max_range: float):
    """The float64 tables ``pcr_scan_context`` takes (include/pcr_hip.h, TABLES): ``(ring_bound2, cos_k, sin_k, range2)``."""
    R, S = _check_shape("scan_context_tables", num_rings, num_sectors)
    L = float(max_range)
    bounds = [float(k) * L / R for k in range(1, R)]
    ring_bound2 = np.array([b * b for b in bounds], dtype=np.float64)
    cos_k = np.array([math.cos(2.0 * math.pi * k / S) for k in range(1, S // 4)], dtype=np.float64)
    sin_k = np.array([math.sin(2.0 * math.pi * k / S) for k in range(1, S // 4)], dtype=np.float64)
    return ring_bound2, cos_k, sin_k, L * L


def _cloud_xyz(fn: str, cloud):
    """the (n, 3) float32 device tensor of a PointCloud or an (n, 3) array (a device tensor of that form passes through)"""
    if isinstance(cloud, PointCloud):
        return cloud.device_xyz()
    torch = _torch()
    shape = tuple(cloud.shape) if isinstance(cloud, torch.Tensor) else np.asarray(cloud).shape
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{fn}: a cloud must be a PointCloud or an (n, 3) array, got shape {shape}")
    return _dev_f32(cloud, 3)


def _descriptor_into(fn: str, cloud, R, S, L, h, out, want_info=False):
    """run pcr_scan_context on one cloud into the (R, S) float32 device tensor ``out``"""
    xyz = _cloud_xyz(fn, cloud)
    ring_bound2, cos_k, sin_k, range2 = scan_context_tables(R, S, L)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if len(a) else None
    params = _lib.PcrScanContextParams(R, S, L, h)
    tables = _lib.PcrScanContextTables(dp(ring_bound2), dp(cos_k), dp(sin_k), range2)
    info = _lib.PcrScanContextInfo() if want_info else None
    ctx = _lib.Context.current()
    ctx.check(ctx.lib.pcr_scan_context(ctx.handle, _ptr(xyz), C.c_int64(int(xyz.shape[0])), C.byref(params), C.byref(tables), _ptr(out),
                                       C.byref(info) if want_info else None), fn)
    if want_info:
        return dict(used=int(info.used), dropped_nonfinite=int(info.dropped_nonfinite), dropped_range=int(info.dropped_range))
    return None


def scan_context(cloud, num_rings: int = 20, num_sectors: int = 60, max_range: float = 80.0, height_offset: float = 2.0, return_info: bool = False):
    """The Scan Context descriptor of a scan in the sensor's frame (z up): an ``(num_rings, num_sectors)`` float32 device tensor whose cell
    (ring, sector) holds the largest ``z + height_offset`` of the points in that polar bin out to ``max_range``, 0 where there is none.
    ``cloud`` is a ``PointCloud`` or an (n, 3) array.  With ``return_info`` the result is ``(descriptor, dict(used, dropped_nonfinite,
    dropped_range))``, the row counts of the rule."""
    fn = "scan_context"
    R, S, L, h = _check_params(fn, num_rings, num_sectors, max_range, height_offset)
    xyz = _cloud_xyz(fn, cloud)
    out = _torch().empty((R, S), dtype=_torch().float32, device="cuda")
    info = _descriptor_into(fn, xyz, R, S, L, h, out, want_info=return_info)
    return (out, info) if return_info else out


def shift_to_transformation(shift: int, num_sectors: int) -> np.ndarray:
    """``Rz(2 pi shift / num_sectors)`` as a 4x4 float64 matrix: the initial pose of a registration of the candidate's cloud (source) onto
    the query's cloud (target) when the distance of (query, candidate) came with this shift."""
    S = int(num_sectors)
    if S < 1:
        raise ValueError(f"shift_to_transformation: num_sectors must be positive, got {num_sectors!r}")
    a = 2.0 * math.pi * (int(shift) % S) / S
    c, s = math.cos(a), math.sin(a)
    T = np.identity(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    return T


def scan_context_distance(desc_a, desc_b):
    """All pairs of two stacks of descriptors, ``(nA, R, S)`` queries and ``(nB, R, S)`` candidates (float32; a single (R, S) image counts as a
    stack of one): ``(dist, shift)`` as ``(nA, nB)`` float64 and int32 device tensors."""
    fn = "scan_context_distance"
    torch = _torch()
    sa, sb = tuple(desc_a.shape), tuple(desc_b.shape)
    sa, sb = ((1,) + sa if len(sa) == 2 else sa), ((1,) + sb if len(sb) == 2 else sb)
    if len(sa) != 3 or len(sb) != 3 or sa[1:] != sb[1:]:
        raise ValueError(f"{fn}: descriptor stacks must be (n, R, S) with the same (R, S), got {tuple(desc_a.shape)} and {tuple(desc_b.shape)}")
    R, S = _check_shape(fn, sa[1], sa[2])
    to_dev = lambda d, s: (d if isinstance(d, torch.Tensor) else torch.from_numpy(np.array(d, dtype=np.float32))).to(device="cuda", dtype=torch.float32).reshape(s).contiguous()
    A, B = to_dev(desc_a, sa), to_dev(desc_b, sb)
    dist = torch.empty((sa[0], sb[0]), dtype=torch.float64, device="cuda")
    shift = torch.empty((sa[0], sb[0]), dtype=torch.int32, device="cuda")
    ctx = _lib.Context.current()
    ctx.check(ctx.lib.pcr_scan_context_distance(ctx.handle, _ptr(A), C.c_int64(sa[0]), _ptr(B), C.c_int64(sb[0]), C.c_int(R), C.c_int(S), _ptr(dist), _ptr(shift)), fn)
    return dist, shift


class ScanContextDatabase:
    """The Scan Context descriptors of a trajectory on the device, one row per scan in the order they were added, with the exact all-pairs
    search over them (no ring-key pre-selection: every candidate is compared at every shift).  A context manager like ``VoxelCovarianceMap``:
    ``close()`` drops the device storage.

        with ScanContextDatabase() as db:
            db.extend(scans)
            closures, dist = db.detect_loop_closures(max_distance=0.4, exclude_recent=50)
    """

    BLOCK_ROWS = 256          # query rows per launch of detect_loop_closures: the largest matrix it holds is BLOCK_ROWS x len(db)

    def __init__(self, num_rings: int = 20, num_sectors: int = 60, max_range: float = 80.0, height_offset: float = 2.0):
        self.num_rings, self.num_sectors, self.max_range, self.height_offset = _check_params("ScanContextDatabase", num_rings, num_sectors, max_range, height_offset)
        self._store = None        # (capacity, R, S) float32 device tensor
        self._n = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        self._store, self._n = None, 0

    def __len__(self):
        return self._n

    @property
    def descriptors(self):
        """the ``(len(db), R, S)`` float32 device tensor of the rows (a view of the storage: valid until the next ``add``)"""
        if self._store is None:
            return _torch().zeros((0, self.num_rings, self.num_sectors), dtype=_torch().float32, device="cuda")
        return self._store[:self._n]

    def _reserve(self, rows):
        torch = _torch()
        cap = 0 if self._store is None else int(self._store.shape[0])
        if rows <= cap:
            return
        new = torch.zeros((max(rows, 2 * cap, 64), self.num_rings, self.num_sectors), dtype=torch.float32, device="cuda")
        if self._n:
            new[:self._n] = self._store[:self._n]
        self._store = new

    def add(self, cloud) -> int:
        """Append the descriptor of a scan (a ``PointCloud`` or an (n, 3) array); returns its row index."""
        self._reserve(self._n + 1)
        _descriptor_into("ScanContextDatabase.add", cloud, self.num_rings, self.num_sectors, self.max_range, self.height_offset, self._store[self._n])
        self._n += 1
        return self._n - 1

    def extend(self, clouds):
        """``add`` every scan of a sequence; returns the list of row indices."""
        clouds = list(clouds)
        self._reserve(self._n + len(clouds))
        return [self.add(c) for c in clouds]

    def _rows(self, fn, rows):
        """None (all rows), a slice or a list of row indices -> (int64 numpy indices, (k, R, S) contiguous device tensor)"""
        if rows is None:
            idx = np.arange(self._n, dtype=np.int64)
        elif isinstance(rows, slice):
            idx = np.arange(self._n, dtype=np.int64)[rows]
        else:
            idx = np.asarray(rows, dtype=np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= self._n):
                raise ValueError(f"{fn}: a row index is outside 0..{self._n - 1}")
        if len(idx) == 0:
            return idx, None
        if len(idx) == idx[-1] - idx[0] + 1 and (np.diff(idx) == 1).all():
            return idx, self._store[int(idx[0]):int(idx[-1]) + 1]
        return idx, self._store[_torch().from_numpy(idx).cuda()].contiguous()

    def distances(self, rows_a=None, rows_b=None):
        """``(dist, shift)`` of the query rows ``rows_a`` against the candidate rows ``rows_b`` (None: all rows; a slice or a list of row
        indices otherwise): ``(len(rows_a), len(rows_b))`` float64 and int32 device tensors."""
        fn = "ScanContextDatabase.distances"
        ia, A = self._rows(fn, rows_a)
        ib, B = self._rows(fn, rows_b)
        torch = _torch()
        if A is None or B is None:
            return (torch.zeros((len(ia), len(ib)), dtype=torch.float64, device="cuda"), torch.zeros((len(ia), len(ib)), dtype=torch.int32, device="cuda"))
        return scan_context_distance(A, B)

    def query(self, cloud_or_descriptor, top_k: int = 1, rows=None):
        """The ``top_k`` rows nearest to a scan (a ``PointCloud`` or an (n, 3) array) or to its ``(R, S)`` descriptor, among ``rows`` (None:
        all): ``(index, dist, shift)`` as int64, float64 and int64 numpy arrays ordered by ``(dist, index)``.  ``shift`` turns the ROW's cloud
        onto the query's (``shift_to_transformation``)."""
        fn = "ScanContextDatabase.query"
        top_k = self._check_top_k(fn, top_k)
        torch = _torch()
        q = cloud_or_descriptor
        if not isinstance(q, (PointCloud, torch.Tensor)):
            q = np.asarray(q)
        shape = None if isinstance(q, PointCloud) else tuple(q.shape)
        if shape is not None and not (len(shape) == 2 and shape[1] == 3):          # (S is a multiple of 4: a descriptor never looks like a cloud)
            if shape != (self.num_rings, self.num_sectors):
                raise ValueError(f"{fn}: a descriptor must have shape ({self.num_rings}, {self.num_sectors}) and a cloud (n, 3), got {shape}")
            qd = (q if isinstance(q, torch.Tensor) else torch.from_numpy(np.array(q, dtype=np.float32))).to(device="cuda", dtype=torch.float32).contiguous()
        else:
            qd = torch.empty((self.num_rings, self.num_sectors), dtype=torch.float32, device="cuda")
            _descriptor_into(fn, q, self.num_rings, self.num_sectors, self.max_range, self.height_offset, qd)
        idx, B = self._rows(fn, rows)
        idx = np.sort(idx)
        if len(idx) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64)
        _, B = self._rows(fn, idx)
        dist, shift = scan_context_distance(qd, B)
        d, order = torch.sort(dist[0], stable=True)          # candidates ascend in row index: a stable sort orders by (dist, index)
        order = order[:top_k]
        return idx[order.cpu().numpy()], d[:top_k].cpu().numpy(), shift[0][order].cpu().numpy().astype(np.int64)

    @staticmethod
    def _check_top_k(fn, top_k):
        if int(top_k) != top_k or int(top_k) < 1:
            raise ValueError(f"{fn}: top_k must be an integer >= 1, got {top_k!r}")
        return int(top_k)

    def detect_loop_closures(self, max_distance: float, exclude_recent: int = 50, top_k: int = 1):
        """For every row i, the candidates are the rows j with ``i - j > exclude_recent`` (the scans just before i are the same place by
        construction); at most ``top_k`` of them with ``dist <= max_distance`` are kept, ordered by ``(dist, j)``.  Returns
        ``(closures, dist)``: an int64 array of rows ``(i, j, shift)`` ascending in i and the float64 array of their distances.  ``shift`` turns
        scan j onto scan i, which is what ``posegraph.loop_closure_edges`` starts its registration from.

        ``max_distance`` has no default, on purpose.  The authors of the method recommend 0.1 to 0.15 when nothing downstream can reject a
        false closure, and 0.4 to 0.6 in front of a robust back end (``global_optimization`` with its line process on ``uncertain`` edges is
        one).  On this repository's NCLT fixtures two adjacent scans sit at 0.10 to 0.30 and scans of different places at 0.51 and above.

        The search runs in blocks of ``BLOCK_ROWS`` query rows, so no ``N x N`` matrix is ever held; the selection after the kernel is torch
        on the device (a stable sort gives the tie order)."""
        fn = "ScanContextDatabase.detect_loop_closures"
        top_k = self._check_top_k(fn, top_k)
        max_distance = float(max_distance)
        if math.isnan(max_distance):
            raise ValueError(f"{fn}: max_distance is NaN")
        if int(exclude_recent) != exclude_recent or int(exclude_recent) < 0:
            raise ValueError(f"{fn}: exclude_recent must be an integer >= 0, got {exclude_recent!r}")
        exclude_recent = int(exclude_recent)
        torch = _torch()
        rows, dists = [], []
        for i0 in range(0, self._n, self.BLOCK_ROWS):
            i1 = min(self._n, i0 + self.BLOCK_ROWS)
            ncand = i1 - 1 - exclude_recent                # the candidates of the block's last row: 0 .. ncand - 1
            if ncand <= 0:
                continue
            dist, shift = scan_context_distance(self._store[i0:i1], self._store[:ncand])
            i = torch.arange(i0, i1, device="cuda").reshape(-1, 1)
            j = torch.arange(ncand, device="cuda").reshape(1, -1)
            keep = (i - j > exclude_recent) & (dist <= max_distance)
            d, order = torch.sort(torch.where(keep, dist, torch.full_like(dist, float("inf"))), dim=1, stable=True)
            k = min(top_k, ncand)
            d, order = d[:, :k], order[:, :k]
            taken = torch.gather(keep, 1, order)           # (an infinite distance that max_distance = inf admits is still a row that was kept)
            sh = torch.gather(shift, 1, order).to(torch.int64)
            ii = i.expand(-1, k)
            rows.append(torch.stack([ii[taken], order[taken], sh[taken]], dim=1).cpu().numpy())
            dists.append(d[taken].cpu().numpy())
        if not rows:
            return np.zeros((0, 3), np.int64), np.zeros(0, np.float64)
        return np.concatenate(rows).astype(np.int64), np.concatenate(dists).astype(np.float64)
