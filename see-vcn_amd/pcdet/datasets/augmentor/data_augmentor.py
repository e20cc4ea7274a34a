"""Config-driven batch augmentor (reference: datasets/augmentor/data_augmentor.py and the training half of DatasetTemplate.prepare_data,
datasets/dataset.py:126-172) for scenes that are already on the device.

`draw_params` makes every random draw on the host, scene by scene and in the reference's call order, from a numpy RandomState;
`BatchDataAugmentor.forward` uploads them once and runs MIN_POINTS_OF_GT, the augmentors of AUG_CONFIG_LIST, the class filter and the point
half of DataProcessor as a fixed number of library calls with one host read, and returns the batch_dict the detectors consume.
"""
import numpy as np
import torch

from ...utils.common_utils import cfg_get
from . import augmentor_utils as A
from . import database_sampler

NUM_TRY = 50                                                     # scale_pre_object's default (augmentor_utils.py:10)

BUILT = ("gt_sampling", "random_object_scaling", "random_world_flip", "random_world_rotation", "random_world_scaling", "random_world_translation")


def _queue(augmentor_configs):
    """The enabled entries of AUG_CONFIG_LIST (data_augmentor.py:15-24); a name that is not built here raises with the name."""
    is_list = isinstance(augmentor_configs, (list, tuple))
    cfgs = augmentor_configs if is_list else cfg_get(augmentor_configs, "AUG_CONFIG_LIST")
    disabled = [] if is_list else (cfg_get(augmentor_configs, "DISABLE_AUG_LIST") or [])
    queue = []
    for cur in cfgs:
        name = cfg_get(cur, "NAME")
        if name in disabled:
            continue
        if name not in BUILT:
            raise NotImplementedError(name)
        if name == "random_object_scaling" and any(cfg_get(q, "NAME") == "gt_sampling" for q in queue):
            # the reference's gt_sampling pops gt_boxes_mask, which its random_object_scaling then looks up (data_augmentor.py:48)
            raise NotImplementedError("random_object_scaling after gt_sampling")
        queue.append(cur)
    return queue


def draw_params(rng, augmentor_configs, num_boxes, sampler=None, gt_names=None):
    """Every draw of one batch: rng is a numpy.random.RandomState, num_boxes[b] the boxes that enter scene b's augmentation (after
    MIN_POINTS_OF_GT) and, for gt_sampling, gt_names[b] their names and sampler the DataBaseSampler.  Scene by scene, per scene in queue order, with
    the reference's calls:
      gt_sampling               permutation(len(db_infos[class])) whenever a group's pointer has wrapped    database_sampler.py:132-134
      random_object_scaling     uniform(lo, hi, size=[N, 50])                                    augmentor_utils.py:26
      random_world_flip         choice([False, True], replace=False, p=[.5, .5]) per axis         :89, :109
      random_world_rotation     uniform(lo, hi)                                                   :130
      random_world_scaling      uniform(lo, hi), nothing when hi - lo < 1e-3                      :153-155
      random_world_translation  normal(0, std, 1) per axis, nothing at all when std == 0          data_augmentor.py:120-122, :211
    Returns one list per scene of (name, value) in draw order; ops without a draw are left out."""
    queue = _queue(augmentor_configs)
    out = []
    for n in num_boxes:
        draws = []
        for cur in queue:
            name = cfg_get(cur, "NAME")
            if name == "gt_sampling":
                draws.append(("gt_sampling", sampler.draw(gt_names[len(out)], rng)))
            elif name == "random_object_scaling":
                s = cfg_get(cur, "SCALE_UNIFORM_NOISE")
                s = list(s) if isinstance(s, (list, tuple, np.ndarray)) else [-s, s]
                draws.append(("object_scaling", rng.uniform(s[0], s[1], size=[int(n), NUM_TRY])))
            elif name == "random_world_flip":
                for axis in cfg_get(cur, "ALONG_AXIS_LIST"):
                    assert axis in ("x", "y")
                    draws.append(("flip_" + axis, bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))))
            elif name == "random_world_rotation":
                r = cfg_get(cur, "WORLD_ROT_ANGLE")
                r = list(r) if isinstance(r, (list, tuple)) else [-r, r]
                draws.append(("rotation", rng.uniform(r[0], r[1])))
            elif name == "random_world_scaling":
                r = cfg_get(cur, "WORLD_SCALE_RANGE")
                if not r[1] - r[0] < 1e-3:
                    draws.append(("scaling", rng.uniform(r[0], r[1])))
            elif name == "random_world_translation":
                std = cfg_get(cur, "NOISE_TRANSLATE_STD")
                if std == 0:
                    continue
                for axis in cfg_get(cur, "ALONG_AXIS_LIST"):
                    assert axis in ("x", "y", "z")
                    draws.append(("translation_" + axis, float(rng.normal(0, std, 1)[0])))
        out.append(draws)
    return out


class BatchDataAugmentor:
    """DataAugmentor + the training half of prepare_data for a whole batch on the device.

    scenes: a list of dicts with points (n, C) and gt_boxes (m, W >= 7) fp32 device tensors, gt_names (m,) host strings and optionally
    num_points_in_gt (m,) host integers (as the reference's infos carry them).  Without num_points_in_gt the per-box counts are made on the device
    and read back once more: the reference sizes its uniform(size=[N, 50]) draw by the number of boxes that pass MIN_POINTS_OF_GT."""

    def __init__(self, root_path, augmentor_configs, class_names, logger=None, min_points_of_gt=1, data_processor=None, db_infos=None,
                 database=None):
        self.root_path, self.class_names, self.logger = root_path, list(class_names), logger
        self.augmentor_configs = augmentor_configs
        self.data_augmentor_queue = _queue(augmentor_configs)
        self.min_points_of_gt = int(min_points_of_gt)
        self.data_processor = data_processor
        self.db_sampler = None
        for cur in self.data_augmentor_queue:
            if cfg_get(cur, "NAME") == "gt_sampling":
                self.db_sampler = database_sampler.DataBaseSampler(root_path, cur, self.class_names, db_infos, database, logger)

    def _class_index(self, names):
        return np.array([self.class_names.index(n) if n in self.class_names else -1 for n in names], np.int32)

    def forward(self, scenes, rng=None, draws=None):
        cls = [self._class_index(s["gt_names"]) for s in scenes]
        pts, boxes = [s["points"] for s in scenes], [s["gt_boxes"] for s in scenes]
        batch = None
        # MIN_POINTS_OF_GT before anything else (dataset.py:129-137)
        if all(s.get("num_points_in_gt") is not None for s in scenes):
            counts = np.concatenate([np.asarray(s["num_points_in_gt"]).reshape(-1) for s in scenes])
        else:
            batch = A.DeviceBatch.from_scenes(pts, boxes, cls)
            counts = A.read(A.points_in_boxes_count(batch))
        present = counts >= self.min_points_of_gt
        sizes = np.array([len(c) for c in cls], np.int64)
        ends = np.cumsum(sizes)
        present = [present[e - n:e] for e, n in zip(ends, sizes)]
        if draws is None:
            names = [np.asarray(s["gt_names"])[p] for s, p in zip(scenes, present)]
            draws = draw_params(rng if rng is not None else np.random, self.augmentor_configs, [int(p.sum()) for p in present], self.db_sampler, names)
        B = len(scenes)
        candidates = [next((v for n, v in d if n == "gt_sampling"), []) for d in draws]
        if any(candidates):
            npts = self.db_sampler.database.counts
            batch = A.DeviceBatch.from_scenes(pts, boxes, cls, [int(sum(npts[i["db_index"]] for _, i in c)) for c in candidates],
                                              [len(c) for c in candidates])
        elif batch is None:
            batch = A.DeviceBatch.from_scenes(pts, boxes, cls)
        # one upload: the class codes after the filter, then every draw of the batch
        N = batch.total_boxes
        names = [name for name, _ in draws[0]]
        assert all([name for name, _ in d] == names for d in draws), "every scene makes the same draws"
        codes = np.full(N, -2, np.int32)
        noises = np.zeros((max(N, 1), NUM_TRY))
        world = [name for name in names if name not in ("object_scaling", "gt_sampling")]
        params = np.zeros((B, max(len(world), 1)))
        for b, d in enumerate(draws):
            first = batch.box_offsets[b]
            codes[first:first + sizes[b]] = np.where(present[b], cls[b], -2)
            rows = first + np.nonzero(present[b])[0]
            col = 0
            for name, value in d:
                if name == "object_scaling":
                    assert value.shape == (len(rows), NUM_TRY)
                    noises[rows] = value                         # row i of the draw belongs to the i-th box that passed the filter
                elif name != "gt_sampling":
                    params[b, col] = float(value)
                    col += 1
        dev = batch.points.device
        up = torch.from_numpy(np.concatenate([codes.astype(np.float64), noises.reshape(-1), params.reshape(-1)])).to(dev)
        batch.box_cls[:N].copy_(up[:N].to(torch.int32))
        noises_d = up[N:N + noises.size].view(-1, NUM_TRY)[:N]
        params_d = up[N + noises.size:].view(B, -1)
        # the queue in order; consecutive world transforms share one pair of launches
        pending, done = [], 0
        for name in names + [None]:
            if name is not None and name not in ("object_scaling", "gt_sampling"):
                pending.append(name)
                continue
            last = name is None
            if pending or last:
                A.world_transform(batch, pending, params_d[:, done:done + len(pending)].contiguous() if pending else None, limit_heading=last)
                done += len(pending)
                pending = []
            if name == "object_scaling":
                A.scale_pre_object(batch, noises_d)
            elif name == "gt_sampling":
                self.db_sampler(batch, candidates)
        dp = self.data_processor
        out = A.compact(batch, **(dp.tail_args() if dp is not None else {}))
        out["draws"] = draws
        return out
