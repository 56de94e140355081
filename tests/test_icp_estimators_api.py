"""CPU-side checks of the point-to-point / point-to-plane surface of ``registration_icp``: the estimator classes, where they are
reachable, the signature, and the ctypes image of ``pcr_icp_params`` against include/pcr_hip.h."""
import ctypes
import inspect
import os
import re

import numpy as np

from conftest import ROOT, pkg


def test_estimator_classes_and_defaults():
    R = pkg("registration")
    p2p = R.TransformationEstimationPointToPoint()
    assert p2p.with_scaling is False
    assert R.TransformationEstimationPointToPoint(True).with_scaling is True
    assert R.TransformationEstimationPointToPoint(with_scaling=True).with_scaling is True
    p2pl = R.TransformationEstimationPointToPlane()
    assert isinstance(p2pl.kernel, R.L2Loss)
    gm = R.GMLoss(0.3)
    assert R.TransformationEstimationPointToPlane(gm).kernel is gm
    assert isinstance(R.TransformationEstimationPointToPlane(kernel=R.L1Loss()).kernel, R.L1Loss)


def test_estimators_reachable_through_the_o3d_facade():
    o3d = pkg("o3d")
    R = pkg("registration")
    reg = o3d.pipelines.registration
    assert reg.TransformationEstimationPointToPoint is R.TransformationEstimationPointToPoint
    assert reg.TransformationEstimationPointToPlane is R.TransformationEstimationPointToPlane
    assert reg.registration_icp is R.registration_icp


def test_registration_icp_signature():
    R = pkg("registration")
    sig = inspect.signature(R.registration_icp)
    assert list(sig.parameters) == ["source", "target", "max_correspondence_distance", "init", "estimation_method", "criteria"]
    assert np.array_equal(sig.parameters["init"].default, np.eye(4))
    assert sig.parameters["estimation_method"].default is None
    assert sig.parameters["criteria"].default is None


def test_icp_params_match_the_header():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pcr_icp_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    ctmap = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctmap[t]) for n, t in fields] == list(L.PcrIcpParams._fields_)
    enum = re.search(r"typedef enum \{([^}]*)\} pcr_icp_estimation;", hdr).group(1)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in enum.split(",")))
    assert vals == {"PCR_ICP_POINT_TO_POINT": L.ICP_POINT_TO_POINT, "PCR_ICP_POINT_TO_PLANE": L.ICP_POINT_TO_PLANE}
    assert "pcr_registration_icp" in L.EXPORTS
