"""Inputs shared by make_multihead_golden.py and the multi-head tests: a 4 x 6 feature map (non-square: a y/x swap in the head-major anchor
order would pass on a square one), three classes in two heads ([A], [B, C]), two rotations."""
import numpy as np

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
GRID = np.array([48, 32, 40])                       # / feature_map_stride 8 -> 6 (x) by 4 (y)
PC_RANGE = [0, -8, -3, 24, 8, 1]
IN_CHANNELS = 8
BATCH = 2


def _anchor(name, size, bottom, matched, unmatched):
    return dict(class_name=name, anchor_sizes=[size], anchor_rotations=[0, 1.57], anchor_bottom_heights=[bottom], align_center=False,
                feature_map_stride=8, matched_threshold=matched, unmatched_threshold=unmatched)


ANCHORS = [_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), _anchor('Pedestrian', [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
           _anchor('Cyclist', [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)]
_ASSIGNER = dict(NAME='AxisAlignedTargetAssigner', POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False,
                 BOX_CODER='ResidualCoder')
_HEADS = [dict(HEAD_CLS_NAME=['Car']), dict(HEAD_CLS_NAME=['Pedestrian', 'Cyclist'])]

# case "coded": 9-d boxes, heading as cos/sin differences, no direction classifier, every head with its own classes, shared conv and
# separate regression towers, L1 loss with class-balance weights (the nuScenes multihead yamls in small)
HEAD_CODED = dict(
    NAME='AnchorHeadMulti', CLASS_AGNOSTIC=False, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2, USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True,
    ANCHOR_GENERATOR_CONFIG=ANCHORS, SHARED_CONV_NUM_FILTER=16, RPN_HEAD_CFGS=_HEADS,
    SEPARATE_REG_CONFIG=dict(NUM_MIDDLE_CONV=1, NUM_MIDDLE_FILTER=16, REG_LIST=['reg:2', 'height:1', 'size:3', 'angle:2', 'velo:2']),
    TARGET_ASSIGNER_CONFIG=dict(_ASSIGNER, BOX_CODER_CONFIG=dict(code_size=9, encode_angle_by_sincos=True)),
    LOSS_CONFIG=dict(REG_LOSS_TYPE='WeightedL1Loss',
                     LOSS_WEIGHTS=dict(pos_cls_weight=1.0, neg_cls_weight=2.0, cls_weight=1.0, loc_weight=0.25, dir_weight=0.2,
                                       code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2])))
# case "plain": 7-d boxes, direction classifier, the heads' predictions concatenated (SEPARATE_MULTIHEAD False), 1 x 1 convolutions
HEAD_PLAIN = dict(
    NAME='AnchorHeadMulti', CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
    USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=False, ANCHOR_GENERATOR_CONFIG=ANCHORS, RPN_HEAD_CFGS=_HEADS, TARGET_ASSIGNER_CONFIG=dict(_ASSIGNER),
    LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])))

POST = dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.3, OUTPUT_RAW_SCORE=False, EVAL_METRIC='kitti',
            NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=0.2, NMS_PRE_MAXSIZE=30, NMS_POST_MAXSIZE=16))


def features(seed=77):
    return (np.random.default_rng(seed).normal(size=(BATCH, IN_CHANNELS, 4, 6)) * 0.5).astype(np.float32)


def gt_boxes(car_anchor):
    """(2, 6, 10) [x, y, z, dx, dy, dz, heading, vx, vy, class]: scene 0 has no Cyclist and a zero-padded tail, scene 1 no box at all.
    car_anchor: one Car anchor (7,) -- row 0 lies exactly on it (IoU 1, a forced match that is also a positive)."""
    gt = np.zeros((BATCH, 6, 10), np.float32)
    gt[0, 0, :7] = car_anchor
    gt[0, 0, 7:] = [1.5, -0.5, 1]
    gt[0, 1] = [12.0, 3.5, -0.9, 4.2, 1.7, 1.5, 0.3, -2.0, 0.25, 1]       # Car between anchors: best IoU below unmatched_threshold -> forced match only
    gt[0, 2] = [4.9, -2.6, 0.2, 0.75, 0.65, 1.7, -0.4, 0.3, 0.1, 2]       # Pedestrian on an anchor: a positive
    gt[0, 3] = [7.2, 0.0, 0.2, 0.7, 0.6, 1.8, 2.0, 0.0, 0.0, 2]           # Pedestrian touching no anchor: IoU 0 everywhere, matches nothing
    return gt


def seeded_head_state(head, seed):
    """seeded_state_dict for every float tensor; the integer buffers `head_label_indices` (class ids, not weights) keep the module's values"""
    from seeding import seeded_state_dict
    sd = seeded_state_dict(head, seed=seed)
    sd.update({k: v for k, v in head.state_dict().items() if k.endswith('head_label_indices')})
    return sd


CASES = {"coded": (HEAD_CODED, 11, 2, 1), "plain": (HEAD_PLAIN, 12, 0, 0)}        # config, seed, extra box columns, sin/cos heading code


def build_head(case, **kw):
    """the package's AnchorHeadMulti of a case with the generator's weights"""
    from seevcn_amd.pcdet.models import dense_heads
    cfg, seed, _, _ = CASES[case]
    head = dense_heads.__all__["AnchorHeadMulti"](model_cfg=cfg, input_channels=IN_CHANNELS, num_class=3, class_names=CLASS_NAMES, grid_size=GRID,
                                                  point_cloud_range=np.array(PC_RANGE, np.float32), **kw)
    head.load_state_dict(seeded_head_state(head, seed))
    return head


def golden(golden_dir, _cache={}):
    import os
    if golden_dir not in _cache:
        _cache[golden_dir] = dict(np.load(os.path.join(golden_dir, "multihead_head.npz")))
    return _cache[golden_dir]
