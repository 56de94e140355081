"""CPU-side checks of the colored-ICP surface: the estimator class, where it is reachable, the ctypes image of ``pcr_colored_icp_params``
against include/pcr_hip.h, the new exports, and colours through the PCD reader and writer."""
import ctypes
import inspect
import os
import re

import numpy as np

from conftest import GOLDEN, ROOT, pkg


def test_estimator_defaults_and_lambda_reset():
    R = pkg("registration")
    e = R.TransformationEstimationForColoredICP()
    assert e.lambda_geometric == 0.968 and isinstance(e.kernel, R.L2Loss)
    assert R.TransformationEstimationForColoredICP(0.5).lambda_geometric == 0.5
    assert R.TransformationEstimationForColoredICP(lambda_geometric=0.0).lambda_geometric == 0.0
    assert R.TransformationEstimationForColoredICP(1.0).lambda_geometric == 1.0
    for bad in (-0.1, 1.5, float("nan")):
        assert R.TransformationEstimationForColoredICP(bad).lambda_geometric == 0.968
    gm = R.GMLoss(0.3)
    assert R.TransformationEstimationForColoredICP(0.9, gm).kernel is gm
    assert isinstance(R.TransformationEstimationForColoredICP(kernel=R.L1Loss()).kernel, R.L1Loss)


def test_reachable_through_the_o3d_facade_and_signature():
    o3d = pkg("o3d")
    R = pkg("registration")
    reg = o3d.pipelines.registration
    assert reg.TransformationEstimationForColoredICP is R.TransformationEstimationForColoredICP
    assert reg.registration_colored_icp is R.registration_colored_icp
    sig = inspect.signature(R.registration_colored_icp)
    assert list(sig.parameters) == ["source", "target", "max_correspondence_distance", "init", "estimation_method", "criteria"]
    assert np.array_equal(sig.parameters["init"].default, np.eye(4))
    pc = o3d.geometry.PointCloud
    for name in ("colors", "has_colors", "paint_uniform_color"):
        assert hasattr(pc, name), name


def test_colored_icp_params_match_the_header():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pcr_colored_icp_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    ctmap = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctmap[t]) for n, t in fields] == list(L.PcrColoredIcpParams._fields_)
    assert [n for n, _ in fields] == ["lambda_geometric", "loss", "loss_k", "relative_fitness", "relative_rmse", "max_iteration"]
    for sym in ("pcr_registration_colored_icp", "pcr_color_gradient", "pcr_voxel_down_sample_ex"):
        assert sym in L.EXPORTS, sym
        assert re.search(r"\bint " + sym + r"\(pcr_context \*ctx,", hdr), sym
    # the existing entry points keep their declarations
    assert "int pcr_voxel_down_sample(pcr_context *ctx, const float *xyz, const float *normals_in, int64_t n, double voxel_size," in hdr


def _packed(rgb8):
    rgb8 = np.asarray(rgb8, np.uint32)
    return (rgb8[:, 0] << 16) | (rgb8[:, 1] << 8) | rgb8[:, 2]


def _write(path, xyz, word, typ, data):
    n = len(xyz)
    hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\n"
           f"TYPE F F F {typ}\nCOUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {data}\n")
    with open(path, "wb") as f:
        f.write(hdr.encode("ascii"))
        if data == "binary":
            rec = np.empty(n, dtype=[("xyz", "<f4", (3,)), ("rgb", "<u4")])
            rec["xyz"] = xyz; rec["rgb"] = word
            f.write(rec.tobytes())
        else:
            for p, w in zip(xyz, word):
                last = repr(float(np.uint32(w).view(np.float32))) if typ == "F" else str(int(w))
                f.write((" ".join(repr(float(v)) for v in p) + " " + last + "\n").encode("ascii"))


def test_pcd_color_roundtrip(tmp_path):
    pio = pkg("io")
    rng = np.random.default_rng(5)
    xyz = rng.standard_normal((64, 3)).astype(np.float32)
    rgb8 = rng.integers(0, 256, (64, 3))
    rgb8[0] = [0, 0, 1]; rgb8[1] = [255, 255, 255]; rgb8[2] = [1, 0, 0]          # denormal, large and small words under a float's name
    want = rgb8.astype(np.float32) / np.float32(255.0)
    for typ in ("F", "U"):
        for data in ("binary", "ascii"):
            p = str(tmp_path / f"c_{typ}_{data}.pcd")
            _write(p, xyz, _packed(rgb8), typ, data)
            got_xyz, got = pio.read_pcd(p)
            assert np.array_equal(got_xyz, xyz) and got.dtype == np.float32, (typ, data)
            assert np.array_equal(got, want), (typ, data)
            assert np.array_equal(pio.read_pcd_xyz(p), xyz)
    # the writer's own layout: x y z rgb with rgb typed F 4, as the reference ships
    p = str(tmp_path / "w.pcd")
    pio.write_pcd(p, xyz, want)
    head = open(p, "rb").read(200).decode("ascii", "replace")
    assert "FIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\n" in head
    got_xyz, got = pio.read_pcd(p)
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got, want)
    # a non-finite point is dropped from both arrays
    bad = xyz.copy(); bad[7, 1] = np.nan
    pio.write_pcd(p, bad, want)
    got_xyz, got = pio.read_pcd(p)
    keep = np.arange(64) != 7
    assert np.array_equal(got_xyz, xyz[keep]) and np.array_equal(got, want[keep])
    # no colours: write_pcd_xyz's bytes, and read_pcd says so
    q = str(tmp_path / "plain.pcd"); q2 = str(tmp_path / "plain2.pcd")
    pio.write_pcd(q, xyz); pio.write_pcd_xyz(q2, xyz)
    assert open(q, "rb").read() == open(q2, "rb").read()
    got_xyz, got = pio.read_pcd(q)
    assert got is None and np.array_equal(got_xyz, xyz)


def test_facade_golden_head_decodes_to_the_shipped_colour():
    """tests/golden/facade_s0_head.pcd: the header of the reference's Facade s0.pcd with WIDTH / POINTS 256 and its first 256 records."""
    pio = pkg("io")
    path = os.path.join(GOLDEN, "facade_s0_head.pcd")
    assert os.path.getsize(path) < 8192
    xyz, colors = pio.read_pcd(path)
    assert xyz.shape == (256, 3) and colors.shape == (256, 3) and np.isfinite(xyz).all()
    assert np.array_equal(colors, np.tile((np.float32([0, 215, 79]) / np.float32(255.0)), (256, 1)))
    assert np.array_equal(pio.read_pcd_xyz(path), xyz)
    assert pio.pcd_point_count(path) == 256
