"""Generate tests/golden/focal_image.npz with the REFERENCE's own Calibration (detector3d/pcdet/utils/calibration_kitti.py, numpy only, loaded by its
path): lidar_to_img on every case's voxel centres with the world transforms taken back (tests/focal_image_reference.py: centres32), and
lidar_to_rect / rect_to_lidar / img_to_rect / rect_to_img / corners3d_to_img_boxes on seeded points for the restated class.

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_focal_image_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport as R  # noqa: E402
import focal_image_reference as FI  # noqa: E402

path = os.path.join(R.REF, "detector3d", "pcdet", "utils", "calibration_kitti.py")
spec = importlib.util.spec_from_file_location("ref_calibration_kitti", path)
ck = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ck)


def ref_calib(c):
    return ck.Calibration({"P2": c.P2, "R0": c.R0, "Tr_velo2cam": c.V2C})


out = {}
for name in FI.CASE_NAMES:
    case = FI.make_case(name)
    coords = case["coords"]
    centres = FI.centres32(case, coords)
    img = np.zeros((len(coords), 2), np.float32)
    depth = np.zeros(len(coords), np.float32)
    for b, c in enumerate(case["calibs"]):
        m = coords[:, 0] == b
        if m.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                img[m], depth[m] = ref_calib(c).lidar_to_img(centres[m])
    assert img.dtype == np.float32
    out[name + "_coords"], out[name + "_centres"], out[name + "_img"], out[name + "_depth"] = coords, centres, img, depth
    print(name, "rows", len(coords), "inside", int((FI.pixels(img[:, 0], img[:, 1], case["image"]) >= 0).sum()))

rng = np.random.RandomState(77)
calib = FI.make_calib(FI.KITTI_IMAGE, 0)
ref = ref_calib(calib)
lidar = (rng.rand(200, 3) * [70, 80, 4] + [0.5, -40, -3]).astype(np.float32)
rect = ref.lidar_to_rect(lidar)
img, depth = ref.rect_to_img(rect)
corners = (rng.rand(12, 8, 3) * [20, 3, 40] + [-10, -1, 5]).astype(np.float32)
boxes, boxes_corner = ref.corners3d_to_img_boxes(corners)
out.update(cal_lidar=lidar, cal_rect=rect, cal_img=img, cal_depth=depth, cal_back=ref.rect_to_lidar(rect),
           cal_unproject=ref.img_to_rect(img[:, 0], img[:, 1], depth), cal_corners=corners, cal_boxes=boxes, cal_boxes_corner=boxes_corner,
           cal_scalars=np.array([ref.cu, ref.cv, ref.fu, ref.fv, ref.tx, ref.ty], np.float32))
path = os.path.join(HERE, "focal_image.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
