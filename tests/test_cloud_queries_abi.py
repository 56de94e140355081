"""CPU-side checks of the cloud queries (nearest-neighbour distances, cloud-to-cloud distances, the radius outlier filter, mean and
covariance): the four entry points are declared in the header, exported by the built library and carry ctypes prototypes that match the
declarations; the PointCloud stand-in and the function module have the calls built on them.  Needs no GPU."""
import ctypes as C
import os
import re

from conftest import ROOT, pkg

SYMBOLS = ["pcr_nearest_neighbor_distance", "pcr_point_cloud_distance", "pcr_remove_radius_outlier", "pcr_mean_and_covariance"]

# C parameter type -> what the prototype in _lib must say (every pointer but the two host outputs is passed as an address)
_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/pcr_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entry_points_are_declared_exported_and_prototyped():
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    for name in SYMBOLS:
        params = _declaration(hdr, name)
        assert name in P._lib.EXPORTS
        assert hasattr(lib, name), f"{name} is not exported by libpcr_hip.so"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None, f"{name} has no prototype in _lib"
        assert len(fn.argtypes) == len(params), (name, params)
        for at, p in zip(fn.argtypes, params):
            if "*" in p:
                assert at is C.c_void_p or issubclass(at, C._Pointer), (name, p, at)
                if issubclass(at, C._Pointer):               # a typed host output: the pointee must be the declared one
                    base = p.replace("const", "").split("*")[0].split()[-1]
                    assert at._type_ is _CTYPE[base], (name, p, at)
            else:
                assert at is _CTYPE[p.split()[-2]], (name, p, at)


def test_point_cloud_and_functions_have_the_new_calls():
    P = pkg()
    for method in ("compute_nearest_neighbor_distance", "compute_point_cloud_distance", "remove_radius_outlier", "get_center",
                   "compute_mean_and_covariance", "uniform_down_sample"):
        assert callable(getattr(P.PointCloud, method, None)), method
    for fn in ("extract_eigen_features", "knn_distance_table"):
        assert callable(getattr(P.functions, fn, None)), fn
        assert getattr(P, fn) is getattr(P.functions, fn)
