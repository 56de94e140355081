"""CPU-side checks of the spatial-compatibility (SC2) global registration: the exports and signatures, the ctypes images of ``pcr_sc2_option``
/ ``pcr_sc2_info`` against include/pcr_hip.h, every limit of the rule raised from the arguments alone, and the numpy restatement
(tests/sc2_reference.py) recovering the planted pose of its own planted lists."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import sc2_reference as ref
from conftest import ROOT, pkg

NAMES = ("pcr_registration_sc2_correspondence", "pcr_spatial_compatibility", "pcr_debug_sc2_seeds")


def test_exports_and_signatures():
    P, R, L = pkg(), pkg("registration"), pkg("_lib")
    for name in ("SpatialCompatibilityOption", "registration_sc2_based_on_correspondence", "registration_sc2_based_on_feature_matching", "spatial_compatibility"):
        assert getattr(P, name) is getattr(R, name)
        assert getattr(pkg("o3d").pipelines.registration, name) is getattr(R, name)
    sig = inspect.signature(R.SpatialCompatibilityOption.__init__)
    assert list(sig.parameters)[1:] == ["inlier_threshold", "nms_radius", "k1", "k2", "seed_ratio", "max_seeds", "refine_iterations"]
    assert sig.parameters["inlier_threshold"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, 30, 20, 0.2, 2048, 20]
    assert list(inspect.signature(R.registration_sc2_based_on_correspondence).parameters) == ["source", "target", "corres", "option"]
    sig = inspect.signature(R.registration_sc2_based_on_feature_matching)
    assert list(sig.parameters) == ["source", "target", "source_feature", "target_feature", "option", "mutual_filter", "mutual_consistency_ratio"]
    assert sig.parameters["mutual_filter"].default is True and sig.parameters["mutual_consistency_ratio"].default == 0.1
    assert list(inspect.signature(R.spatial_compatibility).parameters) == ["source", "target", "corres", "inlier_threshold"]
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    for name in NAMES:
        assert name in L.EXPORTS and name in L.QUERY_PROTOTYPES
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name)


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_structs_match_the_header():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    ctmap = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    opt = _struct_fields(hdr, "pcr_sc2_option")
    assert [n for n, _ in opt] == ["inlier_threshold", "nms_radius", "k1", "k2", "seed_ratio", "max_seeds", "refine_iterations"]
    assert [(n, ctmap[t]) for n, t in opt] == list(L.PcrSc2Option._fields_)
    info = _struct_fields(hdr, "pcr_sc2_info")
    assert [n for n, _ in info] == ["n_corres", "n_seeds", "n_valid", "best_seed", "best_seed_count", "refine_iterations_run"]
    assert [(n, ctmap[t]) for n, t in info] == list(L.PcrSc2Info._fields_)


def test_option_mapping():
    R = pkg("registration")
    o = R._sc2_option("f", R.SpatialCompatibilityOption(0.5))
    assert (o.inlier_threshold, o.nms_radius, o.k1, o.k2, o.seed_ratio, o.max_seeds, o.refine_iterations) == (0.5, 0.5, 30, 20, 0.2, 2048, 20)
    o = R._sc2_option("f", R.SpatialCompatibilityOption(0.1, nms_radius=0.0, k1=63, k2=63, seed_ratio=1.0, max_seeds=65536, refine_iterations=0))
    assert (o.inlier_threshold, o.nms_radius, o.k1, o.k2, o.seed_ratio, o.max_seeds, o.refine_iterations) == (0.1, 0.0, 63, 63, 1.0, 65536, 0)
    o = R._sc2_option("f", R.SpatialCompatibilityOption(0.1, k1=2, k2=1, max_seeds=1))
    assert (o.k1, o.k2, o.max_seeds) == (2, 1, 1)


BAD = [dict(inlier_threshold=0.0), dict(inlier_threshold=-1.0), dict(inlier_threshold=float("inf")), dict(inlier_threshold=float("nan")),
       dict(nms_radius=-0.1), dict(nms_radius=float("nan")), dict(k1=1), dict(k1=64), dict(k2=0), dict(k1=10, k2=11), dict(seed_ratio=0.0),
       dict(seed_ratio=1.5), dict(seed_ratio=float("nan")), dict(max_seeds=0), dict(max_seeds=65537), dict(refine_iterations=-1)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_every_limit_raises_before_the_device(bad):
    R, P = pkg("registration"), pkg()
    src, tgt = P.PointCloud(), P.PointCloud()
    corres = [[0, 0], [1, 1], [2, 2]]
    key = next(iter(bad))
    opt = R.SpatialCompatibilityOption(**{"inlier_threshold": 0.5, **bad})
    with pytest.raises(RuntimeError, match=key):
        R.registration_sc2_based_on_correspondence(src, tgt, corres, opt)
    with pytest.raises(RuntimeError, match=key):
        R.registration_sc2_based_on_feature_matching(src, tgt, None, None, opt)
    if key == "inlier_threshold":
        with pytest.raises(RuntimeError, match=key):
            R.spatial_compatibility(src, tgt, corres, bad[key])


def test_list_limit_raises_before_the_device():
    R, P = pkg("registration"), pkg()
    src, tgt = P.PointCloud(), P.PointCloud()
    big = np.zeros((65537, 2), dtype=np.int32)
    with pytest.raises(RuntimeError, match="65537 correspondences, the limit is 65536.*mutual filter.*keypoint subset"):
        R.registration_sc2_based_on_correspondence(src, tgt, big, R.SpatialCompatibilityOption(0.5))
    with pytest.raises(RuntimeError, match="the limit is 65536"):
        R.spatial_compatibility(src, tgt, big, 0.5)
    with pytest.raises(RuntimeError, match="SpatialCompatibilityOption"):
        R.registration_sc2_based_on_correspondence(src, tgt, big[:3], None)


def test_restatement_packs_bits_as_the_header_says():
    C = np.zeros((70, 70), dtype=bool)
    C[0, 1] = C[0, 63] = C[0, 64] = C[0, 69] = C[5, 7] = True
    b = ref.pack_bits(C).view(np.uint64)
    assert b.shape == (70, 2)
    assert int(b[0, 0]) == (1 << 1) | (1 << 63) and int(b[0, 1]) == (1 << 0) | (1 << 5) and int(b[5, 0]) == 1 << 7 and int(b[1:5].sum()) == 0


@pytest.mark.parametrize("n,f,sigma,tau", [(1000, 0.05, 0.02, 0.1), (1000, 0.02, 0.02, 0.1), (2000, 0.01, 0.02, 0.1)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_recovers_the_planted_pose(n, f, sigma, tau, seed):
    """Bound: 1e-3 rad and 5e-2 m from the planted pose -- about three times the worst of the prototype (3.3e-4 rad, 1.5e-2 m) over these nine
    lists, whose poses rest on as few as 20 rows with 2 cm of noise each."""
    src, tgt, corres, T_true = ref.planted_list(n, f, sigma, seed)
    r = ref.register(src, tgt, corres, tau)
    ang, dt = ref.pose_error(r["T"], T_true)
    k = max(3, int(np.floor(f * n)))
    s, t = ref.list_points(src, tgt, corres)
    planted = ref.residual2(T_true, s, t) < (6 * sigma) ** 2
    print(f"planted n={n} f={f} seed={seed}: {ang:.2e} rad {dt:.2e} m; {r['n_inliers']} inliers, {int((r['inliers'] & planted).sum())} of {k} planted rows, "
          f"{len(r['seeds'])} seeds, best {r['best']}")
    assert r["best"] >= 0
    assert ang < 1e-3 and dt < 5e-2, (ang, dt)
    assert int((r["inliers"] & planted).sum()) >= int(planted.sum()) - 1
