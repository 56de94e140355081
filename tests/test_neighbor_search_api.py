"""CPU-side checks of the nearest-neighbour search index: the six ``pcr_index_*`` entry points are declared in the header, exported by the
built library and carry ctypes prototypes that match the declarations; the two classes exist on the package and in the Open3D-shaped
namespace; argument validation raises before the library or a device is touched; and the numpy reference of the result rule
(``neighbor_reference``) agrees with the oracle's k-d tree row by row and bit by bit.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import neighbor_reference as ref
from conftest import ROOT, pkg

SYMBOLS = ["pcr_index_create", "pcr_index_destroy", "pcr_index_knn", "pcr_index_hybrid", "pcr_index_radius_count", "pcr_index_radius_fill"]
_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/pcr_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entry_points_are_declared_exported_and_prototyped():
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    assert re.search(r"typedef\s+struct\s+pcr_index\s+pcr_index\s*;", hdr)
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    for name in SYMBOLS:
        params = _declaration(hdr, name)
        assert name in P._lib.EXPORTS and name in P._lib.QUERY_PROTOTYPES
        assert hasattr(lib, name), f"{name} is not exported by libpcr_hip.so"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None, f"{name} has no prototype in _lib"
        assert len(fn.argtypes) == len(params), (name, params)
        for at, p in zip(fn.argtypes, params):
            if "*" in p:
                assert at is C.c_void_p or issubclass(at, C._Pointer), (name, p, at)
            else:
                assert at is _CTYPE[p.split()[-2]], (name, p, at)
    # the dataset and the query pointers are inputs
    for name in SYMBOLS[2:]:
        params = _declaration(hdr, name)
        assert params[1] == "const pcr_index *index" and params[2] == "const float *query_xyz", (name, params)
    assert _declaration(hdr, "pcr_index_create")[1] == "const float *xyz"
    assert "const int64_t *row_splits" in _declaration(hdr, "pcr_index_radius_fill")


def test_classes_exist_on_the_package_and_under_o3d():
    P = pkg()
    assert P.NearestNeighborSearch is P.search.NearestNeighborSearch and P.KDTreeFlann is P.search.KDTreeFlann
    assert P.o3d.geometry.KDTreeFlann is P.KDTreeFlann
    assert P.o3d.core.nns.NearestNeighborSearch is P.NearestNeighborSearch
    for m in ("knn_search", "fixed_radius_search", "hybrid_search", "knn_index", "fixed_radius_index", "hybrid_index", "close", "__del__"):
        assert callable(getattr(P.NearestNeighborSearch, m, None)), m
    for m in ("set_geometry", "search_knn_vector_3d", "search_radius_vector_3d", "search_hybrid_vector_3d", "search_vector_3d"):
        assert callable(getattr(P.KDTreeFlann, m, None)), m


def _unbuilt(P):
    """A NearestNeighborSearch without an index (no device touched): what a closed one looks like."""
    return object.__new__(P.NearestNeighborSearch)


def test_validation_raises_before_any_device_work():
    P = pkg()
    q = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="dataset"):
        P.NearestNeighborSearch(np.zeros((5, 2), np.float32))
    with pytest.raises(ValueError, match="dataset"):
        P.NearestNeighborSearch(np.zeros((5, 3, 1), np.float32))
    nns = _unbuilt(P)
    assert nns.knn_index() is True and nns.fixed_radius_index() is True and nns.hybrid_index() is True
    for bad in (0, -1, 201, 2.5, None):
        with pytest.raises(ValueError, match="knn.*1\\.\\.200"):
            nns.knn_search(q, bad)
        with pytest.raises(ValueError, match="max_knn.*1\\.\\.200"):
            nns.hybrid_search(q, 0.5, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="radius.*greater than 0"):
            nns.fixed_radius_search(q, bad)
        with pytest.raises(ValueError, match="radius.*greater than 0"):
            nns.hybrid_search(q, bad, 5)
    for bad in (np.zeros((4, 2)), np.zeros((2, 3, 3)), np.zeros(4)):
        with pytest.raises(ValueError, match="queries.*\\(m, 3\\)"):
            nns.knn_search(bad, 3)
        with pytest.raises(ValueError, match="queries.*\\(m, 3\\)"):
            nns.fixed_radius_search(bad, 1.0)
        with pytest.raises(ValueError, match="queries.*\\(m, 3\\)"):
            nns.hybrid_search(bad, 1.0, 3)
    with pytest.raises(RuntimeError, match="closed"):          # valid arguments, no index
        nns.knn_search(q, 3)

    tree = P.KDTreeFlann()
    with pytest.raises(ValueError, match="knn.*1\\.\\.200"):
        tree.search_knn_vector_3d([0, 0, 0], 0)
    with pytest.raises(ValueError, match="max_nn.*1\\.\\.200"):
        tree.search_hybrid_vector_3d([0, 0, 0], 1.0, 201)
    with pytest.raises(ValueError, match="radius.*greater than 0"):
        tree.search_radius_vector_3d([0, 0, 0], 0.0)
    with pytest.raises(ValueError, match="query.*3 coordinates"):
        tree.search_knn_vector_3d([0, 0, 0, 0], 3)
    with pytest.raises(ValueError, match="search_param"):
        tree.search_vector_3d([0, 0, 0], 30)
    with pytest.raises(ValueError, match="knn.*1\\.\\.200"):
        tree.search_vector_3d([0, 0, 0], P.KDTreeSearchParamKNN(0))
    with pytest.raises(RuntimeError, match="no geometry"):
        tree.search_knn_vector_3d([0, 0, 0], 3)


def test_a_feature_is_refused_with_a_type_error():
    P = pkg()
    feat = P.registration.Feature(None)
    for call in (lambda: P.KDTreeFlann(feat), lambda: P.KDTreeFlann().set_geometry(feat), lambda: P.KDTreeFlann().set_feature(feat),
                 lambda: P.NearestNeighborSearch(feat), lambda: _unbuilt(P).knn_search(feat, 3), lambda: P.KDTreeFlann().search_knn_vector_3d(feat, 3)):
        with pytest.raises(TypeError, match="only 3-D point indices exist"):
            call()


def test_reference_agrees_with_the_oracles_kdtree(oracle, small_pair):
    """Dataset: the source of golden pair 899 after the oracle's voxel_down_sample(0.2), cast to float32; queries: the target prepared the
    same way.  oracle.knn(.., 30) and the numpy reference agree on every index of every row and on d^2 bit for bit (no row of this input
    has an exact float64 tie among its first neighbours, so the k-d tree's own tie order does not show)."""
    src = oracle.voxel_down_sample(small_pair["source"], 0.2).astype(np.float32)
    tgt = oracle.voxel_down_sample(small_pair["target"], 0.2).astype(np.float32)
    assert (len(src), len(tgt)) == (9517, 9716)
    oi, od2, _ = oracle.knn(src, tgt, 30)
    ri, rd2 = ref.knn(src, tgt, 30)
    same = (oi == ri).all(1)
    print(f"rows identical: {same.mean() * 100:.4f} %, largest d2 difference {np.abs(od2 - rd2).max():.3e}")
    assert same.all()
    assert (od2.view(np.int64) == rd2.view(np.int64)).all()
