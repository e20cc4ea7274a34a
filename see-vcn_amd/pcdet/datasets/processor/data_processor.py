"""The steps of the reference's DataProcessor (datasets/processor/data_processor.py) that touch points and boxes, as arguments of the batch
augmentor's final compaction: mask_points_and_boxes_outside_range (:78-91) and shuffle_points (:93-103).  The voxel steps are the voxelisers'
(pcdet.ops.voxel_ops take the stacked points and per-scene starts this returns); transform_points_to_voxels(_placeholder) only records the grid.
"""
import numpy as np

from ...utils.common_utils import cfg_get

STEPS = ("mask_points_and_boxes_outside_range", "shuffle_points", "transform_points_to_voxels", "transform_points_to_voxels_placeholder")


class DataProcessor:
    def __init__(self, processor_configs, point_cloud_range, training, num_point_features=None):
        self.point_cloud_range = np.asarray(point_cloud_range)
        self.training = training
        self.mode = "train" if training else "test"
        self.num_point_features = num_point_features
        self.grid_size = self.voxel_size = None
        self.mask_range = False
        self.min_num_corners = 0
        self.shuffle = False
        for cur in processor_configs:
            name = cfg_get(cur, "NAME")
            if name not in STEPS:
                raise NotImplementedError(name)
            if name == "mask_points_and_boxes_outside_range":
                self.mask_range = True
                if cfg_get(cur, "REMOVE_OUTSIDE_BOXES") and training:
                    self.min_num_corners = int(cfg_get(cur, "min_num_corners", 1))
            elif name == "shuffle_points":
                self.shuffle = bool(cfg_get(cur, "SHUFFLE_ENABLED")[self.mode])
            else:
                self.voxel_size = cfg_get(cur, "VOXEL_SIZE")
                grid = (self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(self.voxel_size)
                self.grid_size = np.round(grid).astype(np.int64)

    def tail_args(self, shuffle=None):
        """Keyword arguments of augmentor_utils.compact.  shuffle: explicit permutations per scene; by default device-generated ones when
        SHUFFLE_ENABLED holds for the mode."""
        return {"point_range": self.point_cloud_range if self.mask_range else None,
                "box_range": self.point_cloud_range if self.min_num_corners else None, "min_num_corners": self.min_num_corners,
                "shuffle": shuffle if shuffle is not None else (True if self.shuffle else None)}
