"""KITTI calibration (reference pcdet/utils/calibration_kitti.py:4-125), restated: the same attributes and numpy arithmetic, so a projection here
rounds as the reference's does, and the packer that puts a batch's calibrations on the device for the focal image branch."""
import numpy as np
import torch


def get_calib_from_file(calib_file):
    """P2, P3 (3 x 4), R0 (3 x 3), Tr_velo2cam (3 x 4) as float32 from lines 2-5 of a KITTI calib file (:4-20)."""
    with open(calib_file) as f:
        lines = f.readlines()
    rows = [np.array(lines[i].strip().split(' ')[1:], dtype=np.float32) for i in (2, 3, 4, 5)]
    return {'P2': rows[0].reshape(3, 4), 'P3': rows[1].reshape(3, 4), 'R0': rows[2].reshape(3, 3), 'Tr_velo2cam': rows[3].reshape(3, 4)}


class Calibration(object):
    def __init__(self, calib_file):
        calib = calib_file if isinstance(calib_file, dict) else get_calib_from_file(calib_file)
        self.P2 = calib['P2']                # 3 x 4
        self.R0 = calib['R0']                # 3 x 3
        self.V2C = calib['Tr_velo2cam']      # 3 x 4
        self.cu = self.P2[0, 2]
        self.cv = self.P2[1, 2]
        self.fu = self.P2[0, 0]
        self.fv = self.P2[1, 1]
        self.tx = self.P2[0, 3] / (-self.fu)
        self.ty = self.P2[1, 3] / (-self.fv)

    def cart_to_hom(self, pts):
        """(N, 3 or 2) -> (N, 4 or 3): a column of float32 ones appended"""
        return np.hstack((pts, np.ones((pts.shape[0], 1), dtype=np.float32)))

    def rect_to_lidar(self, pts_rect):
        """(N, 3) rect -> (N, 3) lidar, through the inverse of the 4 x 4 extensions of R0 and V2C (:50-63)"""
        pts_rect_hom = self.cart_to_hom(pts_rect)
        R0_ext = np.zeros((4, 4), dtype=np.float32)
        R0_ext[:3, :3] = self.R0
        R0_ext[3, 3] = 1
        V2C_ext = np.zeros((4, 4), dtype=np.float32)
        V2C_ext[:3, :4] = self.V2C
        V2C_ext[3, 3] = 1
        pts_lidar = np.dot(pts_rect_hom, np.linalg.inv(np.dot(R0_ext, V2C_ext).T))
        return pts_lidar[:, 0:3]

    def lidar_to_rect(self, pts_lidar):
        """(N, 3) lidar -> (N, 3) rect"""
        return np.dot(self.cart_to_hom(pts_lidar), np.dot(self.V2C.T, self.R0.T))

    def rect_to_img(self, pts_rect):
        """(N, 3) rect -> (N, 2) pixels [u, v] and the depth in the rect camera frame.  The divisor is the rect z, not the third homogeneous
        image coordinate (:82)."""
        pts_rect_hom = self.cart_to_hom(pts_rect)
        pts_2d_hom = np.dot(pts_rect_hom, self.P2.T)
        pts_img = (pts_2d_hom[:, 0:2].T / pts_rect_hom[:, 2]).T
        pts_rect_depth = pts_2d_hom[:, 2] - self.P2.T[3, 2]
        return pts_img, pts_rect_depth

    def lidar_to_img(self, pts_lidar):
        return self.rect_to_img(self.lidar_to_rect(pts_lidar))

    def img_to_rect(self, u, v, depth_rect):
        x = ((u - self.cu) * depth_rect) / self.fu + self.tx
        y = ((v - self.cv) * depth_rect) / self.fv + self.ty
        return np.concatenate((x.reshape(-1, 1), y.reshape(-1, 1), depth_rect.reshape(-1, 1)), axis=1)

    def corners3d_to_img_boxes(self, corners3d):
        """(N, 8, 3) rect corners -> boxes (N, 4) [x1, y1, x2, y2] and boxes_corner (N, 8, 2) in the image"""
        sample_num = corners3d.shape[0]
        corners3d_hom = np.concatenate((corners3d, np.ones((sample_num, 8, 1))), axis=2)
        img_pts = np.matmul(corners3d_hom, self.P2.T)
        x, y = img_pts[:, :, 0] / img_pts[:, :, 2], img_pts[:, :, 1] / img_pts[:, :, 2]
        x1, y1 = np.min(x, axis=1), np.min(y, axis=1)
        x2, y2 = np.max(x, axis=1), np.max(y, axis=1)
        boxes = np.concatenate((x1.reshape(-1, 1), y1.reshape(-1, 1), x2.reshape(-1, 1), y2.reshape(-1, 1)), axis=1)
        boxes_corner = np.concatenate((x.reshape(-1, 8, 1), y.reshape(-1, 8, 1)), axis=2)
        return boxes, boxes_corner


def pack_calib_host(calibs):
    """(B, 24) float32 on the host: per scene M = np.dot(V2C.T, R0.T) (4 x 3; formed in float32 exactly as lidar_to_rect forms it) then P2 (3 x 4),
    both row-major.  `calibs`: any objects with P2, R0 and V2C."""
    table = np.empty((len(calibs), 24), dtype=np.float32)
    for b, c in enumerate(calibs):
        V2C, R0, P2 = (np.asarray(m, dtype=np.float32) for m in (c.V2C, c.R0, c.P2))
        table[b, :12] = np.dot(V2C.T, R0.T).reshape(12)
        table[b, 12:] = P2.reshape(12)
    return table


def pack_calib(calibs, device):
    """The table of pack_calib_host on `device`: one upload, no read."""
    return torch.from_numpy(pack_calib_host(calibs)).to(device, non_blocking=True)
