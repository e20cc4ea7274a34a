"""Config-driven batch augmentor (reference: datasets/augmentor/data_augmentor.py and the training half of DatasetTemplate.prepare_data,
datasets/dataset.py:126-172) for scenes that are already on the device.

`draw_params` makes every random draw on the host, scene by scene and in the reference's call order, from a numpy RandomState;
`BatchDataAugmentor.forward` uploads them once and runs MIN_POINTS_OF_GT, the augmentors of AUG_CONFIG_LIST, the class filter and the point
half of DataProcessor as a fixed number of library calls with one host read, and returns the batch_dict the detectors consume.

Staged draws.  The local augmentors draw once per box, counted by the boxes that exist at that point of the queue, and two ops change that count
on the device: gt_sampling (by its acceptances) and random_world_frustum_dropout (by the boxes it drops).  A queue in which a per-box draw
follows one of the two is cut behind it into stages: `forward` then takes one RandomState per scene, draws every scene's stream up to the
boundary, runs the device work, reads the class codes back (one host read per boundary, a number fixed by the queue) and continues every stream.

random_local_pyramid_aug sizes draws by point counts that only the device knows, so a queue that holds it is always staged, and the entry cuts
itself twice: dropout and sparsify box draws -> device -> read of the selected pyramids' counts; choice draws and swap box draws -> device ->
read of the swap's counts; the swap's choices and the rest of the queue.  A read is skipped when no scene selected a box for that step.
"""
import numpy as np
import torch

from .... import data_pipeline as P
from ...utils.common_utils import cfg_get
from . import augmentor_utils as A
from . import database_sampler

NUM_TRY = 50                                                     # scale_pre_object's default (augmentor_utils.py:10)
DIRECTIONS = ("top", "bottom", "left", "right")


# ---------------------------------------------------------------------------------------------------------- the augmentor table
# One generator per config NAME: given the entry it yields the entry's draws in order as (draw name, per box, draw(rng, n, sampler, gt_names)), n
# being the boxes the scene holds at that point (only gt_sampling looks at the sampler and the names).  The config is read once, when the
# generator runs; the draw functions are then called scene after scene.  The calls are the reference's, per scene in queue order:
#   gt_sampling               permutation(len(db_infos[class])) whenever a group's pointer has wrapped    database_sampler.py:132-134
#   random_object_scaling     uniform(lo, hi, size=[N, 50])                                    augmentor_utils.py:26
#   random_world_flip         choice([False, True], replace=False, p=[.5, .5]) per axis         :89, :109
#   random_world_rotation     uniform(lo, hi)                                                   :130
#   random_world_scaling      uniform(lo, hi), nothing when hi - lo < 1e-3                      :153-155
#   random_world_translation  normal(0, std, 1) per axis, nothing at all when std == 0          data_augmentor.py:120-122, :211
#   random_local_translation  uniform(lo, hi) per axis, per box                                 augmentor_utils.py:267, :290, :313
#   random_local_rotation     uniform(lo, hi) per box                                           :435
#   random_local_scaling      uniform(lo, hi) per box, nothing at all when hi - lo < 1e-3       :399-404
#   random_world_frustum_dropout   uniform(lo, hi) per direction                                :331, :348, :365, :382
#   random_local_frustum_dropout   uniform(lo, hi) per direction, per box                       :484, :504, :524, :544
#   random_local_pyramid_aug  randint(0, 6, n), uniform(0, 1, n); randint(0, 6, m), uniform(0, 1, m), choice(count, MAX, replace=False) per
#                             sparsified pyramid; uniform(0, 1, k), choice(valid faces) per selected box, choice(valid boxes) per pair
#                             (made by BatchDataAugmentor._run_pyramid between its device steps)                  :617-619, :635-656, :687-710
def _per_box(lo, hi):
    """One Python-float draw per box, as the reference's loop over the boxes makes them."""
    return lambda rng, n, *scene: np.array([rng.uniform(lo, hi) for _ in range(int(n))], np.float64)


def _symmetric(r):
    return list(r) if isinstance(r, (list, tuple)) else [-r, r]


def _gt_sampling(cur):
    yield "gt_sampling", False, lambda rng, n, sampler, gt_names: sampler.draw(gt_names, rng)


def _object_scaling(cur):
    s = cfg_get(cur, "SCALE_UNIFORM_NOISE")
    s = list(s) if isinstance(s, (list, tuple, np.ndarray)) else [-s, s]
    yield "object_scaling", True, lambda rng, n, *scene: rng.uniform(s[0], s[1], size=[int(n), NUM_TRY])


def _world_flip(cur):
    for axis in cfg_get(cur, "ALONG_AXIS_LIST"):
        assert axis in ("x", "y")
        yield "flip_" + axis, False, lambda rng, n, *scene: bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))


def _world_rotation(cur):
    r = _symmetric(cfg_get(cur, "WORLD_ROT_ANGLE"))
    yield "rotation", False, lambda rng, n, *scene: rng.uniform(r[0], r[1])


def _world_scaling(cur):
    r = cfg_get(cur, "WORLD_SCALE_RANGE")
    if not r[1] - r[0] < 1e-3:
        yield "scaling", False, lambda rng, n, *scene: rng.uniform(r[0], r[1])


def _world_translation(cur):
    std = cfg_get(cur, "NOISE_TRANSLATE_STD")
    if std == 0:
        return
    for axis in cfg_get(cur, "ALONG_AXIS_LIST"):
        assert axis in ("x", "y", "z")
        yield "translation_" + axis, False, lambda rng, n, *scene: float(rng.normal(0, std, 1)[0])


def _local_translation(cur):
    r = cfg_get(cur, "LOCAL_TRANSLATION_RANGE")
    for axis in cfg_get(cur, "ALONG_AXIS_LIST"):                 # every axis is a whole pass over the boxes
        assert axis in ("x", "y", "z")
        yield "local_translation_" + axis, True, _per_box(r[0], r[1])


def _local_rotation(cur):
    r = _symmetric(cfg_get(cur, "LOCAL_ROT_ANGLE"))
    yield "local_rotation", True, _per_box(r[0], r[1])


def _local_scaling(cur):
    r = cfg_get(cur, "LOCAL_SCALE_RANGE")
    if not r[1] - r[0] < 1e-3:
        yield "local_scaling", True, _per_box(r[0], r[1])


def _frustum_dropout(prefix, per_box):
    def draws(cur):
        r = cfg_get(cur, "INTENSITY_RANGE")
        for d in cfg_get(cur, "DIRECTION"):
            assert d in DIRECTIONS
            yield prefix + d, per_box, _per_box(r[0], r[1]) if per_box else (lambda rng, n, *scene: rng.uniform(r[0], r[1]))
    return draws


PYRAMID = "random_local_pyramid_aug"
PYRAMID_KEYS = ("DROP_PROB", "SPARSIFY_PROB", "SPARSIFY_MAX_NUM", "SWAP_PROB", "SWAP_MAX_NUM")


def _pyramid(cur):
    for name in A.PYRAMID_DRAWS:                                 # sized by what the device decides: no draw function, the entry is a stage of its own
        yield name, True, None


# NAME -> (the keys the entry is read by and the reference has no default for (data_augmentor.py:134-219), whether it changes the number of boxes
# on the device, its draws)
AUGMENTORS = {
    "gt_sampling": ((), True, _gt_sampling),
    "random_object_scaling": ((), False, _object_scaling),
    "random_world_flip": ((), False, _world_flip),
    "random_world_rotation": ((), False, _world_rotation),
    "random_world_scaling": ((), False, _world_scaling),
    "random_world_translation": ((), False, _world_translation),
    "random_local_rotation": (("LOCAL_ROT_ANGLE",), False, _local_rotation),
    "random_local_scaling": (("LOCAL_SCALE_RANGE",), False, _local_scaling),
    "random_local_translation": (("LOCAL_TRANSLATION_RANGE", "ALONG_AXIS_LIST"), False, _local_translation),
    "random_world_frustum_dropout": (("INTENSITY_RANGE", "DIRECTION"), True, _frustum_dropout("world_dropout_", False)),
    "random_local_frustum_dropout": (("INTENSITY_RANGE", "DIRECTION"), False, _frustum_dropout("local_dropout_", True)),
}
# the same three per NAME for the entries whose draws are sized by numbers the device decides: a stage of their own, never drawn ahead
DEVICE_SIZED = {PYRAMID: (PYRAMID_KEYS, False, _pyramid)}


def _entry(name):
    """The table row of a config NAME, None for a name that is not built."""
    return AUGMENTORS.get(name) or DEVICE_SIZED.get(name)


def _draws(cur):
    """The draws of one queue entry: (draw name, per box, draw) in order."""
    return _entry(cfg_get(cur, "NAME"))[2](cur)


def _plan(entries):
    """The draws of a run of queue entries, read from the config once for all scenes: [(draw name, draw), ...] in order."""
    return [(name, draw) for cur in entries for name, _, draw in _draws(cur)]


def _draw(plan, rng, n, sampler=None, gt_names=None):
    """One scene's draws: [(name, value), ...] in draw order; n: the boxes the scene holds at that point."""
    return [(name, draw(rng, n, sampler, gt_names)) for name, draw in plan]


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
        if _entry(name) is None:
            raise NotImplementedError(name)
        for key in _entry(name)[0]:
            if cfg_get(cur, key) is None:                        # refused when the queue is built, not at the first draw
                raise NotImplementedError(f"{name} without {key}")
        if name == "random_object_scaling" and any(cfg_get(q, "NAME") == "gt_sampling" for q in queue):
            # the reference's gt_sampling pops gt_boxes_mask, which its random_object_scaling then looks up (data_augmentor.py:48)
            raise NotImplementedError("random_object_scaling after gt_sampling")
        if name == "random_object_scaling" and any(cfg_get(q, "NAME") == "random_world_frustum_dropout" for q in queue):
            # the reference's dropout shortens gt_boxes but not the gt_boxes_mask that random_object_scaling indexes with
            raise NotImplementedError("random_object_scaling after random_world_frustum_dropout")
        queue.append(cur)
    return queue


def _draws_per_box(cur):
    """Whether the entry makes a draw per box of the scene."""
    return any(per_box for _, per_box, _ in _draws(cur))


def _is_pyramid(stage):
    return len(stage) == 1 and cfg_get(stage[0], "NAME") == PYRAMID


def _stages(queue):
    """The queue cut behind every gt_sampling / random_world_frustum_dropout that a per-box draw follows; one stage for every queue without.  A
    random_local_pyramid_aug is a stage of its own (it cuts itself further: _run_pyramid), between stages of the other entries; the first and the
    last stage are always of the other kind (empty where the queue begins or ends with the pyramid entry): they carry the class codes' upload and the
    heading's limit_period."""
    stages, cur = [], []
    for i, q in enumerate(queue):
        if cfg_get(q, "NAME") == "gt_sampling" and stages:
            # its draw needs the names of the boxes that are left, which only the device knows by then
            raise NotImplementedError("gt_sampling behind a per-box draw that follows random_world_frustum_dropout")
        if cfg_get(q, "NAME") == PYRAMID:
            stages += ([cur] if cur or not stages else []) + [[q]]
            cur = []
            continue
        cur.append(q)
        if _entry(cfg_get(q, "NAME"))[1] and any(_draws_per_box(r) for r in queue[i + 1:]):
            stages.append(cur)
            cur = []
    return stages + [cur]


def _entry_names(cur):
    """The names of the draws one queue entry makes, in order (fixed by the config)."""
    return [name for name, _, _ in _draws(cur)]


def _draw_scene(rng, entries, n, sampler=None, gt_names=None):
    """One scene's draws for a run of queue entries: [(name, value), ...] in draw order; n: the boxes the scene holds at that point."""
    return _draw(_plan(entries), rng, n, sampler, gt_names)


def draw_params(rng, augmentor_configs, num_boxes, sampler=None, gt_names=None):
    """Every draw of one batch: rng is a numpy.random.RandomState, num_boxes[b] the boxes that enter scene b's augmentation (after
    MIN_POINTS_OF_GT) and, for gt_sampling, gt_names[b] their names and sampler the DataBaseSampler.  Scene by scene, per scene in queue order, with
    the reference's calls (the table above AUGMENTORS lists them with their lines).
    Returns one list per scene of (name, value) in draw order; ops without a draw are left out; a per-box draw is an (n,) float64 array.
    A queue in which a per-box draw follows gt_sampling or random_world_frustum_dropout cannot be drawn ahead: ValueError (see forward)."""
    queue = _queue(augmentor_configs)
    if len(_stages(queue)) > 1:
        raise ValueError("a per-box draw follows gt_sampling or random_world_frustum_dropout, or the queue holds random_local_pyramid_aug: the "
                         "number of boxes or points it is sized by is decided on the device, so one shared stream cannot be replayed; give "
                         "forward() one RandomState per scene")
    plan = _plan(queue)
    return [_draw(plan, rng, n, sampler, None if gt_names is None else gt_names[b]) for b, n in enumerate(num_boxes)]


class BatchDataAugmentor:
    """DataAugmentor + the training half of prepare_data for a whole batch on the device.

    scenes: a list of dicts with points (n, C) and gt_boxes (m, W >= 7) fp32 device tensors, gt_names (m,) host strings and optionally
    num_points_in_gt (m,) host integers (as the reference's infos carry them).  Without num_points_in_gt the per-box counts are made on the device
    and read back once more: the reference sizes its uniform(size=[N, 50]) draw by the number of boxes that pass MIN_POINTS_OF_GT.

    forward(scenes, rng): rng is one RandomState for the batch (scene by scene from one stream) or a list of one per scene; per scene the result
    then equals the reference run on that sample alone from that state.  A staged queue (module docstring) needs the list, and costs one more
    host read per boundary.  The local augmentors move every box that exists (box_cls != -2), those of other classes too, as the reference's
    loops over gt_boxes do; behind a gt_sampling that accepted something, the scene's boxes of other classes are gone, as they are there
    (database_sampler.py: gt_boxes[gt_boxes_mask]).

    random_local_pyramid_aug (SE-SSD's face dropout, sparsify and swap; csrc/augment_pyramid.hip) is always staged: it needs the list of random
    states and adds at most two host reads, whatever the batch.  Every box row that exists takes part, other classes included.  Its rows come out
    in the reference's order: the scene's remaining points, then each sparsified pyramid's chosen points, then per swapped pair the two mapped
    blocks (a self-swap and a shared partner repeat points, as they do there).  SWAP_PROB > 0 needs points of exactly 4 columns and raises
    otherwise when the batch is formed (the reference raises at the first swap); dropout and sparsify work for any C >= 3."""

    def __init__(self, root_path, augmentor_configs, class_names, logger=None, min_points_of_gt=1, data_processor=None, db_infos=None,
                 database=None):
        self.root_path, self.class_names, self.logger = root_path, list(class_names), logger
        self.augmentor_configs = augmentor_configs
        self.data_augmentor_queue = _queue(augmentor_configs)
        self.stages = _stages(self.data_augmentor_queue)
        self.min_points_of_gt = int(min_points_of_gt)
        self.data_processor = data_processor
        self.db_sampler = None
        for cur in self.data_augmentor_queue:
            if cfg_get(cur, "NAME") == "gt_sampling":
                self.db_sampler = database_sampler.DataBaseSampler(root_path, cur, self.class_names, db_infos, database, logger)

    def _class_index(self, names):
        return np.array([self.class_names.index(n) if n in self.class_names else -1 for n in names], np.int32)

    def _run_stage(self, batch, draws, rows, codes, candidates, last):
        """One stage on the device: one upload (the class codes with the first stage, then every draw of the stage), then the queue in order;
        consecutive world transforms, consecutive local steps and consecutive world dropouts share their launches."""
        B, N, dev = batch.batch_size, batch.total_boxes, batch.points.device
        names = [name for name, _ in draws[0]]
        assert all([name for name, _ in d] == names for d in draws), "every scene makes the same draws"
        count = {k: sum(P.op_kind(n) == k for n in names) for k in ("world", "local", "drop")}
        noises = np.zeros((max(N, 1) if "object_scaling" in names else 0, NUM_TRY))
        world, local, drop = np.zeros((B, count["world"])), np.zeros((N, count["local"])), np.zeros((B, count["drop"]))
        for b, d in enumerate(draws):
            col = {"world": 0, "local": 0, "drop": 0}
            for name, value in d:
                k = P.op_kind(name)
                if name == "object_scaling":
                    assert np.shape(value) == (len(rows[b]), NUM_TRY)
                    noises[rows[b]] = value                      # row i of the draw belongs to the i-th box that exists
                elif k == "local":
                    value = np.asarray(value, np.float64).reshape(-1)
                    if len(value) != len(rows[b]):
                        raise ValueError(f"scene {b}: {name} holds {len(value)} draws, the scene has {len(rows[b])} boxes at that point")
                    local[rows[b], col[k]] = value
                    col[k] += 1
                elif k in col:
                    (world if k == "world" else drop)[b, col[k]] = float(value)
                    col[k] += 1
        parts = ([] if codes is None else [codes.astype(np.float64)]) + [noises.reshape(-1), world.reshape(-1), local.reshape(-1), drop.reshape(-1)]
        up = torch.from_numpy(np.concatenate(parts)).to(dev)
        at = 0
        if codes is not None:
            batch.box_cls[:N].copy_(up[:N].to(torch.int32))
            at = N
        noises_d = up[at:at + noises.size].view(noises.shape)[:N]
        at += noises.size
        params = {}
        for k, host in (("world", world), ("local", local), ("drop", drop)):
            params[k] = up[at:at + host.size].view(host.shape)
            at += host.size
        done = {"world": 0, "local": 0, "drop": 0}
        pending, kind = [], None
        for name in names + [None]:
            k = None if name is None else P.op_kind(name)
            if k in done and (k == kind or not pending):
                pending.append(name)
                kind = k
                continue
            final = name is None and last
            if pending:
                p = params[kind][:, done[kind]:done[kind] + len(pending)].contiguous()
                done[kind] += len(pending)
                if kind == "local":
                    A.local_transform(batch, pending, p)
                elif kind == "drop":
                    A.world_frustum_dropout(batch, pending, p)
                else:
                    A.world_transform(batch, pending, p, limit_heading=final)
            if final and kind != "world":
                A.world_transform(batch, [], None, limit_heading=True)
            pending, kind = ([name], k) if k in done else ([], None)
            if name == "object_scaling":
                A.scale_pre_object(batch, noises_d)
            elif name == "gt_sampling":
                before = batch.box_cnt.clone()
                self.db_sampler(batch, candidates)
                if not last:
                    # the reference keeps gt_boxes[gt_boxes_mask] + the sampled boxes wherever something was accepted (database_sampler.py:
                    # add_sampled_boxes_to_scene): for the per-box ops that follow, that scene's boxes of other classes do not exist
                    sizes = np.diff(np.append(batch.box_offsets, N))
                    scene = torch.from_numpy(np.repeat(np.arange(B), sizes)).to(dev)
                    cls = batch.box_cls[:N]
                    cls.copy_(torch.where((cls == -1) & (batch.box_cnt > before)[scene], torch.full_like(cls, -2), cls))

    def _run_pyramid(self, batch, cur, rows, rng, given):
        """random_local_pyramid_aug on the device (data_augmentor.py:221-242).  rows[b]: the box rows of scene b that exist; rng: one RandomState
        per scene, or given[b]: the scene's eight replayed draws.  A fixed number of library calls and at most two host reads; returns the draws."""
        B, N = batch.batch_size, batch.total_boxes
        drop_p, sp_p, sp_max, sw_p, sw_max = (cfg_get(cur, k) for k in PYRAMID_KEYS)
        replay = None if given is None else [dict(d) for d in given]
        if replay is not None and any(tuple(n for n, _ in d) != A.PYRAMID_DRAWS for d in given):
            raise ValueError(f"random_local_pyramid_aug replays the draws {A.PYRAMID_DRAWS} in that order")

        def draw(b, name, n, make):
            if replay is None:
                return make(rng[b])
            value = np.asarray(replay[b][name]).reshape(-1)
            if len(value) != n:
                raise ValueError(f"scene {b}: {name} holds {len(value)} draws, the scene has {n} boxes at that point")
            return value

        out = [{} for _ in range(B)]
        # dropout's and sparsify's box draws; the device drops the faces and counts the selected pyramids
        faces, u = np.full(N, np.nan), np.full(N, np.nan)
        for b in range(B):
            n = len(rows[b])
            out[b]["pyramid_drop_face"] = faces[rows[b]] = draw(b, "pyramid_drop_face", n, lambda r: r.randint(0, 6, n))
            out[b]["pyramid_drop_u"] = u[rows[b]] = draw(b, "pyramid_drop_u", n, lambda r: r.uniform(0, 1, n))
        dropped = A.local_pyramid_dropout(batch, faces, u, drop_p)
        selected, left = [], []
        mask = np.zeros(N, np.int64)
        for b in range(B):
            mine = rows[b][~dropped[rows[b]]]
            m = len(mine)
            f = out[b]["pyramid_sparsify_face"] = draw(b, "pyramid_sparsify_face", m, lambda r: r.randint(0, 6, m))
            v = out[b]["pyramid_sparsify_u"] = draw(b, "pyramid_sparsify_u", m, lambda r: r.uniform(0, 1, m))
            sel = v <= sp_p
            selected.append((mine[sel], np.asarray(f)[sel].astype(np.int64)))
            left.append(mine[~sel])
            mask[selected[b][0]] = 1 << selected[b][1]
        counts = A.read_checked(batch, A.points_in_pyramids_mask(batch, mask)) if mask.any() else np.zeros((N, 6), np.int32)
        # the choices the counts size; sparsify; the swap's box draws; the device counts the pyramids of the boxes that are left
        plan = A.plan_pyramid_sparsify(counts, selected, sp_max, rng, None if replay is None else [d["pyramid_sparsify_choice"] for d in replay])
        A.local_pyramid_sparsify(batch, plan)
        chosen = []
        mask = np.zeros(N, np.int64)
        for b in range(B):
            out[b]["pyramid_sparsify_choice"] = plan["choices"][b]
            k = len(left[b])
            v = out[b]["pyramid_swap_u"] = draw(b, "pyramid_swap_u", k, lambda r: r.uniform(0, 1, k))
            chosen.append(v <= sw_p)
            if chosen[b].any():
                mask[left[b]] = 63
        counts = A.read_checked(batch, A.points_in_pyramids_mask(batch, mask)) if mask.any() else np.zeros((N, 6), np.int32)
        # the swap's choices; the swap
        plan = A.plan_pyramid_swap(counts, left, chosen, sw_max, rng, None if replay is None else [d["pyramid_swap_face"] for d in replay],
                                   None if replay is None else [d["pyramid_swap_partner"] for d in replay])
        A.local_pyramid_swap(batch, plan)
        for b in range(B):
            out[b]["pyramid_swap_face"], out[b]["pyramid_swap_partner"] = plan["faces"][b], plan["partners"][b]
        return [[(name, d[name]) for name in A.PYRAMID_DRAWS] for d in out]

    def forward(self, scenes, rng=None, draws=None):
        cls = [self._class_index(s["gt_names"]) for s in scenes]
        pts, boxes = [s["points"] for s in scenes], [s["gt_boxes"] for s in scenes]
        for cur in self.data_augmentor_queue:
            if cfg_get(cur, "NAME") == PYRAMID and cfg_get(cur, "SWAP_PROB") > 0 and any(p.shape[1] != 4 for p in pts):
                raise ValueError("random_local_pyramid_aug with SWAP_PROB > 0 needs points of exactly 4 columns: the swap re-assembles x y z and "
                                 f"the last column (the reference raises at the first swap); got {sorted({int(p.shape[1]) for p in pts})}")
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
        B, stages = len(scenes), self.stages
        per_scene = isinstance(rng, (list, tuple))
        if per_scene and len(rng) != B:
            raise ValueError(f"{len(rng)} random states for {B} scenes")
        if draws is None and len(stages) > 1 and not per_scene:
            raise ValueError("this queue makes a per-box draw behind gt_sampling or random_world_frustum_dropout, whose number of boxes is decided "
                             "on the device (or holds random_local_pyramid_aug, whose draws are sized by point counts decided there): scene 1's "
                             "draws would have to come before it is known how many scene 0 makes, so one shared "
                             "stream cannot follow the reference; pass rng as a list of one numpy RandomState per scene")
        given, taken = draws, [0] * B
        names = [np.asarray(s["gt_names"])[p] for s, p in zip(scenes, present)]
        num_boxes = [int(p.sum()) for p in present]

        def stage_draws(entries):
            if given is not None:
                n = sum(len(_entry_names(cur)) for cur in entries)
                out = [list(given[b][taken[b]:taken[b] + n]) for b in range(B)]
                for b in range(B):
                    taken[b] += n
                return out
            if per_scene:
                plan = _plan(entries)
                return [_draw(plan, rng[b], num_boxes[b], self.db_sampler, names[b]) for b in range(B)]
            return draw_params(rng if rng is not None else np.random, self.augmentor_configs, num_boxes, self.db_sampler, names)

        first = stage_draws(stages[0]) if len(stages) > 1 or given is None else [list(d) for d in given]
        candidates = [next((v for n, v in d if n == "gt_sampling"), []) for d in first]
        if any(candidates):
            npts = self.db_sampler.database.counts
            batch = A.DeviceBatch.from_scenes(pts, boxes, cls, [int(sum(npts[i["db_index"]] for _, i in c)) for c in candidates],
                                              [len(c) for c in candidates])
        elif batch is None:
            batch = A.DeviceBatch.from_scenes(pts, boxes, cls)
        N = batch.total_boxes
        codes = np.full(N, -2, np.int32)                          # the class codes after the filter
        rows = []
        for b in range(B):
            start = batch.box_offsets[b]
            codes[start:start + sizes[b]] = np.where(present[b], cls[b], -2)
            rows.append(start + np.nonzero(present[b])[0])
        all_draws = [list(d) for d in first]
        self._run_stage(batch, first, rows, codes, candidates, len(stages) == 1)
        bounds = np.append(batch.box_offsets, N)
        changes_boxes = lambda entries: any(_entry(cfg_get(q, "NAME"))[1] for q in entries)
        stale = changes_boxes(stages[0])                         # whether the device has changed which box rows exist since the host last knew
        for s in range(1, len(stages)):
            if stale:
                now = A.read_checked(batch, batch.box_cls[:N])   # the boundary: which box rows exist now
                rows = [bounds[b] + np.nonzero(now[bounds[b]:bounds[b + 1]] != -2)[0] for b in range(B)]
                num_boxes = [len(r) for r in rows]
                stale = False
            if _is_pyramid(stages[s]):
                mine = None
                if given is not None:
                    mine = [list(given[b][taken[b]:taken[b] + len(A.PYRAMID_DRAWS)]) for b in range(B)]
                    for b in range(B):
                        taken[b] += len(A.PYRAMID_DRAWS)
                cur = self._run_pyramid(batch, stages[s][0], rows, rng, mine)
            else:
                cur = stage_draws(stages[s])
                self._run_stage(batch, cur, rows, None, candidates, s == len(stages) - 1)
                stale = changes_boxes(stages[s])
            for b in range(B):
                all_draws[b] += cur[b]
        dp = self.data_processor
        out = A.compact(batch, **(dp.tail_args() if dp is not None else {}))
        out["draws"] = all_draws
        return out


def world_draws_to_batch(draws, device=None):
    """The per-scene tensors the focal image branch reads from batch_dict to take the world transforms back (reference data_augmentor.py sets
    'flip_x' / 'flip_y', 'noise_rot', 'noise_scale' beside the points): {'noise_scale', 'noise_rot' (B,) fp32, 'flip_x', 'flip_y' (B,) bool} from
    out["draws"] of BatchDataAugmentor.forward.  A draw the queue does not make is the identity (1, 0, False); one upload per tensor, no read."""
    def column(name, identity):
        return [next((value for key, value in scene if key == name), identity) for scene in draws]
    return {"noise_scale": torch.tensor(column("scaling", 1.0), dtype=torch.float32, device=device),
            "noise_rot": torch.tensor(column("rotation", 0.0), dtype=torch.float32, device=device),
            "flip_x": torch.tensor(column("flip_x", False), dtype=torch.bool, device=device),
            "flip_y": torch.tensor(column("flip_y", False), dtype=torch.bool, device=device)}
