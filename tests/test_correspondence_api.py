"""CPU-side checks of the calls on a correspondence list: the estimators' ``compute_transformation`` / ``compute_rmse``,
``correspondences_from_features``, ``registration_fgr_based_on_correspondence``, ``utility.Vector2iVector`` and ``registro_manual`` --
signatures, where they are reachable, the ctypes image of ``pcr_estimation`` against include/pcr_hip.h, and the argument errors that are
raised before a device context is asked for (there is no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

import correspondence_reference as ref


def test_estimator_methods_and_functions_exist_with_their_signatures():
    R = pkg("registration")
    for cls in (R.TransformationEstimationPointToPoint, R.TransformationEstimationPointToPlane, R.TransformationEstimationForGeneralizedICP,
                R.TransformationEstimationForColoredICP):
        for name in ("compute_transformation", "compute_rmse"):
            assert list(inspect.signature(getattr(cls, name)).parameters) == ["self", "source", "target", "corres"], (cls, name)
    sig = inspect.signature(R.correspondences_from_features).parameters
    assert list(sig) == ["source_features", "target_features", "mutual_filter", "mutual_consistency_ratio"]
    assert sig["mutual_filter"].default is False and sig["mutual_consistency_ratio"].default == 0.1
    sig = inspect.signature(R.registration_fgr_based_on_correspondence).parameters
    assert list(sig) == ["source", "target", "corres", "option"] and sig["option"].default is None
    F = pkg("functions")
    assert list(inspect.signature(F.registro_manual).parameters) == ["source", "target", "picked_id_source", "picked_id_target"]
    assert pkg().registro_manual is F.registro_manual


def test_reachable_through_the_o3d_facade():
    o3d = pkg("o3d")
    R = pkg("registration")
    reg = o3d.pipelines.registration
    for name in ("correspondences_from_features", "registration_fgr_based_on_correspondence", "registration_ransac_based_on_correspondence"):
        assert getattr(reg, name) is getattr(R, name)
    assert reg.TransformationEstimationPointToPoint.compute_transformation is R.TransformationEstimationPointToPoint.compute_transformation
    v = o3d.utility.Vector2iVector(np.array([[0.0, 3.0], [2.0, 1.0]]))          # the reference passes a float array of integral values
    assert v.dtype == np.int32 and v.shape == (2, 2) and v.tolist() == [[0, 3], [2, 1]]
    assert o3d.utility.Vector2iVector([]).shape == (0, 2)


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


def test_estimation_struct_matches_the_header():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    ctmap = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    fields = _struct_fields(hdr, "pcr_estimation")
    assert [n for n, _ in fields] == ["kind", "with_scaling", "loss", "loss_k", "epsilon"]
    assert [(n, ctmap[t]) for n, t in fields] == list(L.PcrEstimation._fields_)
    enum = re.search(r"typedef enum \{([^}]*)\} pcr_estimation_kind;", hdr).group(1)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in enum.split(",")))
    assert vals == {"PCR_EST_POINT_TO_POINT": L.EST_POINT_TO_POINT, "PCR_EST_POINT_TO_PLANE": L.EST_POINT_TO_PLANE,
                    "PCR_EST_GENERALIZED_ICP": L.EST_GENERALIZED_ICP}
    for name in ("pcr_estimation_compute_transformation", "pcr_estimation_compute_rmse", "pcr_correspondences_from_features",
                 "pcr_registration_fgr_correspondence"):
        assert name in L.EXPORTS and name in L.QUERY_PROTOTYPES
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
    R = pkg("registration")
    e = R.TransformationEstimationPointToPoint(True)._estimation()
    assert (e.kind, e.with_scaling) == (L.EST_POINT_TO_POINT, 1)
    e = R.TransformationEstimationPointToPlane(R.GMLoss(0.5))._estimation()
    assert (e.kind, e.loss, e.loss_k) == (L.EST_POINT_TO_PLANE, L.LOSS_GM, 0.5)
    e = R.TransformationEstimationForGeneralizedICP(R.L1Loss(), 2e-3)._estimation()
    assert (e.kind, e.loss, e.epsilon) == (L.EST_GENERALIZED_ICP, L.LOSS_L1, 2e-3)


def test_argument_errors_come_before_the_device():
    R = pkg("registration")
    P = pkg()
    src, tgt = P.PointCloud(), P.PointCloud()
    ests = (R.TransformationEstimationPointToPoint(), R.TransformationEstimationPointToPlane(), R.TransformationEstimationForGeneralizedICP())
    for est in ests:
        for call in (est.compute_transformation, est.compute_rmse):
            with pytest.raises(RuntimeError, match=r"corres must have shape \(C, 2\)"):
                call(src, tgt, np.zeros((5, 3)))
            with pytest.raises(RuntimeError, match="correspondence index out of range"):
                call(src, tgt, [[0, 0], [-1, 2]])
    with pytest.raises(RuntimeError, match=r"corres must have shape \(C, 2\)"):
        R.registration_fgr_based_on_correspondence(src, tgt, np.zeros((5, 3)))
    with pytest.raises(RuntimeError, match="registration_fgr_based_on_correspondence: correspondence index out of range"):
        R.registration_fgr_based_on_correspondence(src, tgt, [[0, 0], [-1, 2]])
    col = R.TransformationEstimationForColoredICP()
    with pytest.raises(RuntimeError, match=r"TransformationEstimationForColoredICP\.compute_transformation is not implemented on the MI355X path"):
        col.compute_transformation(src, tgt, [[0, 0]])
    with pytest.raises(RuntimeError, match=r"TransformationEstimationForColoredICP\.compute_rmse is not implemented on the MI355X path"):
        col.compute_rmse(src, tgt, [[0, 0]])


def test_registro_manual_refuses_too_few_or_unequal_picks():
    F = pkg("functions")
    P = pkg()
    src, tgt = P.PointCloud(), P.PointCloud()
    with pytest.raises(AssertionError):
        F.registro_manual(src, tgt, [0, 1], [0, 1])
    with pytest.raises(AssertionError):
        F.registro_manual(src, tgt, [0, 1, 2, 3], [0, 1, 2])


def test_unit_is_in_the_build_and_in_the_packed_fp32_scan():
    csrc = os.path.join(ROOT, "point-cloud-registration-with-global-refinement_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "pcr_corres.hip")) and os.path.exists(os.path.join(csrc, "pcr_solve6.h"))
    assert re.search(r"^for f in .*\bpcr_corres\b", open(os.path.join(csrc, "build.sh")).read(), re.M)
    assert '"pcr_corres"' in open(os.path.join(ROOT, "tools", "pk_trans_scan.py")).read()
    unit = open(os.path.join(csrc, "pcr_corres.hip")).read()
    for kernel in ("k_corr_check", "k_corr_rows", "k_corr_fit"):
        assert kernel in unit
    # the 6x6 solve exists once, in the header both units include
    assert "icp_ldlt6_fast(const double" not in unit and "icp_ldlt6_fast(const double" not in open(os.path.join(csrc, "pcr_gicp.hip")).read()
    assert open(os.path.join(csrc, "pcr_solve6.h")).read().count("icp_ldlt6_fast(const double") == 1


def test_reference_matcher_rules():
    """the numpy matcher itself: ties go to the smaller index, the ratio decides between the mutual rows and all rows"""
    src = np.array([[0.0] * 33, [1.0] * 33, [1.0] * 33, [5.0] * 33], np.float32)
    tgt = np.array([[1.0] * 33, [1.0] * 33, [0.0] * 33], np.float32)
    rows, n_mutual = ref.match_features(src, tgt, False)
    assert rows.tolist() == [[0, 2], [1, 0], [2, 0], [3, 0]] and n_mutual == 2
    assert ref.match_features(src, tgt, True, 0.0)[0].tolist() == [[0, 2], [1, 0]]
    assert ref.match_features(src, tgt, True, 0.5)[0].tolist() == [[0, 2], [1, 0]]          # 2 >= int(0.5 * 4)
    assert ref.match_features(src, tgt, True, 0.9)[0].tolist() == rows.tolist()             # 2 < int(0.9 * 4) = 3: all rows
    idx, best, second = ref.nearest_rows(src, tgt)
    assert idx.tolist() == [2, 0, 0, 0] and best.tolist() == [0.0, 0.0, 0.0, 16.0 * 33] and second.tolist() == [33.0, 0.0, 0.0, 16.0 * 33]


def test_reference_fits_recover_a_planted_motion():
    rng = np.random.default_rng(5)
    src = rng.uniform(-2, 2, (200, 3))
    a = np.deg2rad(3.0)
    Rm = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    T_true = np.eye(4); T_true[:3, :3] = 1.05 * Rm; T_true[:3, 3] = [0.3, -0.2, 0.1]
    tgt = src @ T_true[:3, :3].T + T_true[:3, 3]
    corres = np.stack([np.arange(200), np.arange(200)], axis=1)
    assert np.abs(ref.point_to_point(src, tgt, corres, True) - T_true).max() < 1e-12
    assert ref.rmse_euclidean(tgt, tgt, corres) == 0.0 and abs(ref.rmse_euclidean(src, src + [0, 0, 2.0], corres) - 2.0) < 1e-15
    n = np.tile([0.0, 0.0, 2.0], (200, 1))
    assert abs(ref.rmse_plane(src, src + [1.0, 0, 0.5], n, corres) - 1.0) < 1e-15 and ref.rmse_plane(src, tgt, None, corres) == 0.0
