"""GT sampling with the database on the device (reference: datasets/augmentor/database_sampler.py).

`GtDatabase` is one flat (T, C) point tensor, (K + 1) offsets, (K, W) boxes and (K,) class ids on the device.  `DataBaseSampler` keeps the
reference's host logic -- the PREPARE filters, LIMIT_WHOLE_SCENE and the pointer / np.random.permutation walk of sample_with_fixed_number -- and
hands the drawn candidates to csrc/augment.hip: sv_gt_sample_select decides which go in, sv_gt_sample_paste writes their points and removes the
scene points they cover.
"""
import os

import numpy as np
import torch

from .... import _lib as L
from ...utils.common_utils import cfg_get
from . import augmentor_utils as A


class GtDatabase:
    def __init__(self, points, offsets, boxes, class_ids):
        L.require_cuda(points, offsets, boxes, class_ids)
        assert points.dtype == boxes.dtype == torch.float32 and offsets.dtype == torch.int64 and class_ids.dtype == torch.int32
        assert offsets.numel() == boxes.shape[0] + 1 == class_ids.numel() + 1 and boxes.shape[1] >= 7
        self.points, self.offsets, self.boxes, self.class_ids = points.contiguous(), offsets.contiguous(), boxes.contiguous(), class_ids.contiguous()
        self.counts = np.diff(offsets.cpu().numpy())             # points per object, for the host's sizing (read once, when the database is built)

    @classmethod
    def from_arrays(cls, points_list, boxes, class_ids, device):
        """points_list[k] (n_k, C) fp32 in the object's own frame (as the .bin files hold them), boxes (K, W), class_ids (K,): host arrays."""
        counts = np.array([len(p) for p in points_list], np.int64)
        C = points_list[0].shape[1] if len(points_list) else 4
        flat = np.concatenate(points_list).astype(np.float32) if counts.sum() else np.zeros((1, C), np.float32)
        inst = cls(torch.from_numpy(flat).to(device), torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(device),
                   torch.from_numpy(np.ascontiguousarray(boxes, np.float32).reshape(len(counts), -1)).to(device),
                   torch.from_numpy(np.ascontiguousarray(class_ids, np.int32)).to(device))
        return inst

    @classmethod
    def from_infos(cls, infos, root_path, num_point_features, class_names, device):
        """infos: the reference's db_infos dict {class name: [info, ...]} (create_groundtruth_database); every info's 'path' is read with
        np.fromfile(float32).reshape(-1, num_point_features) (database_sampler.py:386-388).  Sets info['db_index'], the object's row here."""
        pts, boxes, ids = [], [], []
        for name in class_names:
            for info in infos.get(name, []):
                info["db_index"] = len(pts)
                pts.append(np.fromfile(os.path.join(str(root_path), info["path"]), dtype=np.float32).reshape([-1, num_point_features]))
                boxes.append(np.asarray(info["box3d_lidar"], np.float32))
                ids.append(class_names.index(name))
        return cls.from_arrays(pts, np.stack(boxes) if boxes else np.zeros((0, 7), np.float32), ids, device)


class DataBaseSampler:
    """sampler_cfg as in the reference (PREPARE, SAMPLE_GROUPS, REMOVE_EXTRA_WIDTH, LIMIT_WHOLE_SCENE, NUM_POINT_FEATURES); db_infos: the dict the
    reference unpickles from DB_INFO_PATH, given directly, every info carrying 'db_index' (GtDatabase.from_infos sets it)."""

    def __init__(self, root_path, sampler_cfg, class_names, db_infos, database, logger=None):
        if cfg_get(sampler_cfg, "USE_ROAD_PLANE", False):
            raise NotImplementedError("USE_ROAD_PLANE")
        if cfg_get(sampler_cfg, "IMG_AUG_TYPE", None) is not None:
            raise NotImplementedError("IMG_AUG_TYPE")
        self.root_path, self.class_names, self.sampler_cfg, self.logger, self.database = root_path, list(class_names), sampler_cfg, logger, database
        self.db_infos = {name: list(db_infos.get(name, [])) for name in class_names}
        for func_name, val in (cfg_get(sampler_cfg, "PREPARE") or {}).items():
            self.db_infos = getattr(self, func_name)(self.db_infos, val)
        self.sample_groups, self.sample_class_num = {}, {}
        self.limit_whole_scene = cfg_get(sampler_cfg, "LIMIT_WHOLE_SCENE", False)
        self.extra_width = [float(v) for v in cfg_get(sampler_cfg, "REMOVE_EXTRA_WIDTH", [0.0, 0.0, 0.0])]
        for x in cfg_get(sampler_cfg, "SAMPLE_GROUPS"):
            class_name, sample_num = x.split(":")
            if class_name not in class_names:
                continue
            self.sample_class_num[class_name] = sample_num
            self.sample_groups[class_name] = {"sample_num": sample_num, "pointer": len(self.db_infos[class_name]),
                                              "indices": np.arange(len(self.db_infos[class_name]))}

    def filter_by_difficulty(self, db_infos, removed_difficulty):
        """database_sampler.py:94-104"""
        return {key: [info for info in dinfos if info["difficulty"] not in removed_difficulty] for key, dinfos in db_infos.items()}

    def filter_by_min_points(self, db_infos, min_gt_points_list):
        """database_sampler.py:106-121"""
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(":")
            min_num = int(min_num)
            if min_num > 0 and name in db_infos.keys():
                db_infos[name] = [info for info in db_infos[name] if info["num_points_in_gt"] >= min_num]
        return db_infos

    def sample_with_fixed_number(self, class_name, sample_group, rng=np.random):
        """database_sampler.py:123-140: the pointer walk; a new permutation is drawn when the pointer has run past the class's infos."""
        sample_num, pointer, indices = int(sample_group["sample_num"]), sample_group["pointer"], sample_group["indices"]
        if pointer >= len(self.db_infos[class_name]):
            indices = rng.permutation(len(self.db_infos[class_name]))
            pointer = 0
        sampled_dict = [self.db_infos[class_name][idx] for idx in indices[pointer: pointer + sample_num]]
        pointer += sample_num
        sample_group["pointer"] = pointer
        sample_group["indices"] = indices
        return sampled_dict

    def draw(self, gt_names, rng=np.random):
        """The host half of __call__ (:438-445) for one scene: [(group number, info), ...] in group and draw order.  gt_names: the names of the
        scene's boxes after MIN_POINTS_OF_GT."""
        gt_names = np.asarray(gt_names).astype(str)
        out = []
        for g, (class_name, sample_group) in enumerate(self.sample_groups.items()):
            if self.limit_whole_scene:
                num_gt = np.sum(class_name == gt_names)
                sample_group["sample_num"] = str(int(self.sample_class_num[class_name]) - num_gt)
            if int(sample_group["sample_num"]) > 0:
                out.extend((g, info) for info in self.sample_with_fixed_number(class_name, sample_group, rng))
        return out

    def __call__(self, batch, candidates):
        """candidates[b]: scene b's list from draw().  The batch was built with the candidates' rows in place (DeviceBatch.from_scenes with
        point_slots / box_slots).  Two library calls whatever the batch; returns the accept flags (device int32, one per candidate)."""
        db, dev, B = self.database, batch.points.device, batch.batch_size
        assert db.boxes.shape[1] == batch.box_width and db.points.shape[1] == batch.num_point_features
        idx = [info["db_index"] for c in candidates for _, info in c]
        total = len(idx)
        if total == 0:
            return torch.zeros(0, dtype=torch.int32, device=dev)
        npts = db.counts[idx]
        sizes = np.array([len(c) for c in candidates], np.int64)
        cand_start = np.concatenate([[0], np.cumsum(sizes)])
        ptoff = np.concatenate([[0], np.cumsum(npts)])
        # candidate i's rows: behind the rows of the scene's earlier candidates, at the head of the scene
        dest = np.concatenate([batch.pt_offsets[b] + ptoff[cand_start[b]:cand_start[b + 1]] - ptoff[cand_start[b]] for b in range(B)])
        head = np.array([ptoff[cand_start[b + 1]] - ptoff[cand_start[b]] for b in range(B)])
        assert all(head[b] == batch.point_slots[b] for b in range(B)), "the batch was not built for these candidates"
        host = np.concatenate([idx, [g for c in candidates for g, _ in c], cand_start, ptoff, dest, head]).astype(np.int32)
        up = torch.from_numpy(host).to(dev)                      # one upload
        o = np.cumsum([0, total, total, B + 1, total + 1, total])
        cand_idx, cand_group, cand_start_d, ptoff_d, dest_d, head_d = [up[o[i]:o[i + 1]] if i < 5 else up[o[5]:] for i in range(6)]
        accept = torch.empty(total, dtype=torch.int32, device=dev)
        A.call("sv_gt_sample_select", L.ptr(batch.boxes), batch.box_width, L.ptr(batch.box_start), L.ptr(batch.box_cnt), L.ptr(batch.box_cap),
               L.ptr(batch.box_cls), B, L.ptr(db.boxes), L.ptr(db.class_ids), L.ptr(cand_idx), L.ptr(cand_group), L.ptr(cand_start_d), total, L.ptr(accept))
        A.call("sv_gt_sample_paste", *batch._pt_args(), L.ptr(head_d), L.ptr(batch.keep), B, batch.max_scene_points, L.ptr(db.points), L.ptr(db.offsets),
               L.ptr(db.boxes), batch.box_width, L.ptr(cand_idx), L.ptr(cand_start_d), L.ptr(ptoff_d), L.ptr(dest_d), L.ptr(accept), total, int(ptoff[-1]),
               *self.extra_width)
        return accept
