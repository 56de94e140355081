"""CPU-side checks of the RANSAC global-registration surface: the criteria and checker classes, the two signatures, where they are
reachable, the argument errors raised before the device is touched, and the ctypes images of ``pcr_ransac_params`` /
``pcr_ransac_info`` against include/pcr_hip.h."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT, pkg


def test_criteria_and_checker_classes_and_defaults():
    R = pkg("registration")
    c = R.RANSACConvergenceCriteria()
    assert c.max_iteration == 100000 and c.confidence == 0.999
    c = R.RANSACConvergenceCriteria(4000, 0.5)
    assert c.max_iteration == 4000 and c.confidence == 0.5
    c = R.RANSACConvergenceCriteria(max_iteration=7, confidence=1.0)
    assert c.max_iteration == 7 and c.confidence == 1.0
    assert R.CorrespondenceCheckerBasedOnEdgeLength().similarity_threshold == 0.9
    assert R.CorrespondenceCheckerBasedOnEdgeLength(0.8).similarity_threshold == 0.8
    assert R.CorrespondenceCheckerBasedOnEdgeLength(similarity_threshold=0.7).similarity_threshold == 0.7
    assert R.CorrespondenceCheckerBasedOnDistance(0.2).distance_threshold == 0.2
    assert R.CorrespondenceCheckerBasedOnDistance(distance_threshold=0.3).distance_threshold == 0.3
    assert R.CorrespondenceCheckerBasedOnNormal(0.5).normal_angle_threshold == 0.5
    assert R.CorrespondenceCheckerBasedOnNormal(normal_angle_threshold=0.25).normal_angle_threshold == 0.25
    # Open3D: the edge-length check runs on the sample before the fit, the other two after it
    assert R.CorrespondenceCheckerBasedOnEdgeLength().require_pointcloud_alignment_ is False
    assert R.CorrespondenceCheckerBasedOnDistance(1.0).require_pointcloud_alignment_ is True
    assert R.CorrespondenceCheckerBasedOnNormal(1.0).require_pointcloud_alignment_ is True


def test_ransac_signatures():
    R = pkg("registration")
    sig = inspect.signature(R.registration_ransac_based_on_correspondence)
    assert list(sig.parameters) == ["source", "target", "corres", "max_correspondence_distance", "estimation_method", "ransac_n", "checkers",
                                    "criteria", "seed"]
    sigf = inspect.signature(R.registration_ransac_based_on_feature_matching)
    assert list(sigf.parameters) == ["source", "target", "source_feature", "target_feature", "mutual_filter", "max_correspondence_distance",
                                     "estimation_method", "ransac_n", "checkers", "criteria", "seed"]
    for s in (sig, sigf):
        assert s.parameters["estimation_method"].default is None
        assert s.parameters["ransac_n"].default == 3
        assert s.parameters["checkers"].default == []
        assert s.parameters["criteria"].default is None
        assert s.parameters["seed"].default is None
        assert s.parameters["max_correspondence_distance"].default is inspect.Parameter.empty
    assert sigf.parameters["mutual_filter"].default is inspect.Parameter.empty


def test_ransac_reachable_through_the_o3d_facade():
    o3d = pkg("o3d")
    R = pkg("registration")
    reg = o3d.pipelines.registration
    for name in ("RANSACConvergenceCriteria", "CorrespondenceCheckerBasedOnEdgeLength", "CorrespondenceCheckerBasedOnDistance",
                 "CorrespondenceCheckerBasedOnNormal", "registration_ransac_based_on_correspondence",
                 "registration_ransac_based_on_feature_matching"):
        assert getattr(reg, name) is getattr(R, name)


def test_argument_errors_come_before_the_device():
    """Open3D's messages; all of them are raised from the arguments alone (no GPU here)."""
    R = pkg("registration")
    P = pkg()
    src, tgt = P.PointCloud(), P.PointCloud()
    corres = [[0, 0], [1, 1], [2, 2]]
    for d in (0.0, -1.0):
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance."):
            R.registration_ransac_based_on_correspondence(src, tgt, corres, d)
        with pytest.raises(RuntimeError, match="Invalid max_correspondence_distance."):
            R.registration_ransac_based_on_feature_matching(src, tgt, None, None, True, d)
    for n in (2, 9, 0):
        with pytest.raises(RuntimeError, match="ransac_n"):
            R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, ransac_n=n)
        with pytest.raises(RuntimeError, match="ransac_n"):
            R.registration_ransac_based_on_feature_matching(src, tgt, None, None, False, 0.5, ransac_n=n)
    for est in (R.TransformationEstimationPointToPlane(), R.TransformationEstimationForGeneralizedICP()):
        with pytest.raises(RuntimeError, match="is not implemented on the MI355X path"):
            R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, est)
        with pytest.raises(RuntimeError, match="is not implemented on the MI355X path"):
            R.registration_ransac_based_on_feature_matching(src, tgt, None, None, True, 0.5, est)
    with pytest.raises(RuntimeError, match="is not implemented on the MI355X path"):
        R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, checkers=[object()])
    with pytest.raises(RuntimeError, match="confidence"):
        R.registration_ransac_based_on_correspondence(src, tgt, corres, 0.5, criteria=R.RANSACConvergenceCriteria(10, 1.5))


def test_ransac_params_mapping():
    """What the Python arguments become in ``pcr_ransac_params``: an absent checker is a negative threshold, several checkers of one kind act
    as the strictest, ``seed=None`` draws a fresh seed per call."""
    R = pkg("registration")
    p = R._ransac_params("f", 0.5, None, 3, [], None, 7)
    assert (p.ransac_n, p.with_scaling, p.max_iteration, p.confidence, p.seed) == (3, 0, 100000, 0.999, 7)
    assert p.edge_length_threshold < 0 and p.distance_threshold < 0 and p.normal_angle_threshold < 0
    p = R._ransac_params("f", 0.5, R.TransformationEstimationPointToPoint(True), 4,
                         [R.CorrespondenceCheckerBasedOnEdgeLength(0.9), R.CorrespondenceCheckerBasedOnEdgeLength(0.8),
                          R.CorrespondenceCheckerBasedOnDistance(0.2), R.CorrespondenceCheckerBasedOnDistance(0.3),
                          R.CorrespondenceCheckerBasedOnNormal(0.5), R.CorrespondenceCheckerBasedOnNormal(0.4)],
                         R.RANSACConvergenceCriteria(50, 1.0), 2 ** 64 - 1)
    assert (p.ransac_n, p.with_scaling, p.max_iteration, p.confidence, p.seed) == (4, 1, 50, 1.0, 2 ** 64 - 1)
    assert (p.edge_length_threshold, p.distance_threshold, p.normal_angle_threshold) == (0.9, 0.2, 0.4)
    a = R._ransac_params("f", 0.5, None, 3, [], None, None).seed
    b = R._ransac_params("f", 0.5, None, 3, [], None, None).seed
    assert a != b


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_ransac_structs_match_the_header():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    ctmap = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    params = _struct_fields(hdr, "pcr_ransac_params")
    assert [n for n, _ in params] == ["ransac_n", "with_scaling", "max_iteration", "confidence", "seed", "edge_length_threshold",
                                      "distance_threshold", "normal_angle_threshold"]
    assert [(n, ctmap[t]) for n, t in params] == list(L.PcrRansacParams._fields_)
    info = _struct_fields(hdr, "pcr_ransac_info")
    assert [n for n, _ in info] == ["iterations_run", "best_iteration", "n_valid", "n_corres"]
    assert [(n, ctmap[t]) for n, t in info] == list(L.PcrRansacInfo._fields_)
    for name in ("pcr_registration_ransac_correspondence", "pcr_registration_ransac_feature_matching", "pcr_debug_ransac_hypotheses"):
        assert name in L.EXPORTS
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
