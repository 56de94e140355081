"""CPU-side checks of the DBSCAN clustering: ``pcr_cluster_dbscan`` is declared in the header with its six rules, exported by the built library
and carries a ctypes prototype that matches the declaration; ``PointCloud.cluster_dbscan``, ``functions.remove_small_clusters`` and the
package-level alias exist; the unit is in the build; and the float64 restatement the GPU tests compare against (dbscan_reference.py) gives
scikit-learn's labels.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pkg
from dbscan_reference import dbscan_reference

NAME = "pcr_cluster_dbscan"
_CTYPE = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
HOST_OUTPUTS = {"out_n_clusters": C.c_int64}          # typed pointers; every other pointer is passed as an address


def _declaration(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/pcr_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entry_point_is_declared_exported_and_prototyped():
    P = pkg()
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    params = _declaration(hdr, NAME)
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "xyz", "n", "eps", "min_points", "labels", "core_mask", "out_n_clusters"]
    if not os.path.exists(P._lib.SO_PATH):
        P._lib.build()
    lib = P._lib.load()
    assert NAME in P._lib.EXPORTS
    assert hasattr(lib, NAME), f"{NAME} is not exported by libpcr_hip.so"
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and fn.argtypes is not None, f"{NAME} has no prototype in _lib"
    assert len(fn.argtypes) == len(params), params
    for at, p in zip(fn.argtypes, params):
        arg = p.split()[-1].lstrip("*")
        if "*" in p:
            if arg in HOST_OUTPUTS:
                assert issubclass(at, C._Pointer) and at._type_ is HOST_OUTPUTS[arg], (p, at)
                assert _CTYPE[p.replace("const", "").split("*")[0].split()[-1]] is at._type_, (p, at)      # ... and the declared pointee
            else:
                assert at is C.c_void_p, (p, at)
        else:
            assert at is _CTYPE[p.split()[-2]], (p, at)
    # the six rules are stated next to the entry point
    doc = hdr[:hdr.index("int " + NAME)].rsplit("/*", 1)[1]
    for word in ("ClusterDBSCAN", "NEIGHBOURHOOD", "CORE", "CLUSTERS", "NUMBERING", "BORDER", "NOISE", "d^2(i, j) < eps^2", "SMALLEST"):
        assert word in doc, word


def test_python_surface_has_the_clustering_calls():
    P = pkg()
    sig = inspect.signature(P.PointCloud.cluster_dbscan).parameters
    assert list(sig) == ["self", "eps", "min_points", "print_progress"] and sig["print_progress"].default is False
    assert list(inspect.signature(P.geometry._cluster_dbscan).parameters) == ["cloud", "eps", "min_points"]
    assert list(inspect.signature(P.functions.remove_small_clusters).parameters) == ["cloud", "eps", "min_points", "min_cluster_size"]
    assert P.remove_small_clusters is P.functions.remove_small_clusters
    assert P.o3d.geometry.PointCloud.cluster_dbscan is P.PointCloud.cluster_dbscan


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_cluster.hip"))
    assert re.search(r"^for f in .*\bpcr_cluster\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_cluster"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()


def test_restatement_gives_the_labels_of_scikit_learn():
    """scikit-learn follows the rules 2-6 with d <= eps instead of d^2 < eps^2 and its own distance arithmetic: equal labels wherever no pair
    sits within 1e-9 relative of eps^2, which this input at (0.5, 10) has none of."""
    cluster = pytest.importorskip("sklearn.cluster")
    pts = np.load(os.path.join(GOLDEN, "nclt_pair_899.npz"))["source"][::2]
    assert pts.shape == (8263, 3)
    ref = dbscan_reference(pts, 0.5, 10)
    assert ref["rim_pairs"] == 0
    p = pts.astype(np.float64)
    e2 = 0.5 * 0.5
    for i0 in range(0, len(p), 1000):                        # ... and no exact tie either (the two rules differ there)
        d2 = ((p[i0:i0 + 1000, None, :] - p[None, :, :]) ** 2).sum(2)
        assert not (np.abs(d2 - e2) <= 1e-9 * e2).any()
    sk = cluster.DBSCAN(eps=0.5, min_samples=10, algorithm="brute").fit(p).labels_
    print(f"restatement: {ref['n_clusters']} clusters, {int(ref['core'].sum())} core, {int((ref['labels'] < 0).sum())} noise; scikit-learn: {sk.max() + 1} clusters")
    assert ref["n_clusters"] == 35 and ref["n_clusters"] == sk.max() + 1
    assert np.array_equal(sk, ref["labels"])
