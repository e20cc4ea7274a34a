"""Model-section dictionaries of the reference YAMLs this path is measured on (values copied as data from
detector3d/tools/cfgs/kitti_models/second.yaml:7-86); used by tests, the golden generators and bench.py."""

SECOND_BACKBONE_2D = dict(NAME='BaseBEVBackbone', LAYER_NUMS=[5, 5], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256],
                          UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[256, 256])


def _anchor(name, size, bottom, matched, unmatched):
    return dict(class_name=name, anchor_sizes=[size], anchor_rotations=[0, 1.57], anchor_bottom_heights=[bottom], align_center=False,
                feature_map_stride=8, matched_threshold=matched, unmatched_threshold=unmatched)


SECOND_DENSE_HEAD = dict(
    NAME='AnchorHeadSingle', CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
    ANCHOR_GENERATOR_CONFIG=[_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45),
                             _anchor('Pedestrian', [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
                             _anchor('Cyclist', [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)],
    TARGET_ASSIGNER_CONFIG=dict(NAME='AxisAlignedTargetAssigner', POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False,
                                MATCH_HEIGHT=False, BOX_CODER='ResidualCoder'),
    LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])))

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
KITTI_RANGE = [0, -40, -3, 70.4, 40, 1]

SECOND_POST_PROCESSING = dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, EVAL_METRIC='kitti',
                              NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE='nms_gpu', NMS_THRESH=0.01, NMS_PRE_MAXSIZE=4096,
                                              NMS_POST_MAXSIZE=500))


def second_model_cfg(dynamic_vfe=True):
    """MODEL section of kitti_models/second.yaml; dynamic_vfe swaps MeanVFE (hard voxels from the dataloader) for DynMeanVFE."""
    return dict(NAME='SECONDNet', VFE=dict(NAME='DynMeanVFE' if dynamic_vfe else 'MeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=SECOND_BACKBONE_2D,
                DENSE_HEAD=SECOND_DENSE_HEAD, POST_PROCESSING=SECOND_POST_PROCESSING)


class SyntheticDatasetInfo:
    """The attributes Detector3DTemplate.build_networks reads from a dataset (detector3d_template.py:36-44)."""

    def __init__(self, class_names=CLASS_NAMES, point_cloud_range=KITTI_RANGE, voxel_size=(0.05, 0.05, 0.1), num_point_features=3):
        import numpy as np
        from types import SimpleNamespace
        self.class_names = list(class_names)
        self.point_cloud_range = np.array(point_cloud_range, np.float32)
        self.voxel_size = list(voxel_size)
        self.grid_size = np.round((self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(voxel_size)).astype(np.int64)
        self.point_feature_encoder = SimpleNamespace(num_point_features=num_point_features)
        self.depth_downsample_factor = None

# detector3d/tools/cfgs/kitti_models/pointpillar.yaml:5-60 (values as data)
PP_RANGE = [0, -39.68, -3, 69.12, 39.68, 1]
PP_VOXEL = dict(VOXEL_SIZE=[0.16, 0.16, 4], MAX_POINTS_PER_VOXEL=32, MAX_NUMBER_OF_VOXELS={'train': 16000, 'test': 40000})
PP_VFE = dict(NAME='PillarVFE', WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, USE_NORM=True, NUM_FILTERS=[64])
PP_MAP_TO_BEV = dict(NAME='PointPillarScatter', NUM_BEV_FEATURES=64)
PP_BACKBONE_2D = dict(NAME='BaseBEVBackbone', LAYER_NUMS=[3, 5, 5], LAYER_STRIDES=[2, 2, 2], NUM_FILTERS=[64, 128, 256],
                      UPSAMPLE_STRIDES=[1, 2, 4], NUM_UPSAMPLE_FILTERS=[128, 128, 128])


PP_DENSE_HEAD = dict(SECOND_DENSE_HEAD, ANCHOR_GENERATOR_CONFIG=[dict(a, feature_map_stride=2) for a in SECOND_DENSE_HEAD['ANCHOR_GENERATOR_CONFIG']])


def pointpillar_model_cfg():
    """MODEL section of kitti_models/pointpillar.yaml:48-140 (values as data)."""
    return dict(NAME='PointPillar', VFE=PP_VFE, MAP_TO_BEV=PP_MAP_TO_BEV, BACKBONE_2D=PP_BACKBONE_2D, DENSE_HEAD=PP_DENSE_HEAD,
                POST_PROCESSING=SECOND_POST_PROCESSING)


def _sa(mlps, radii, nsample, factor=None):
    d = dict(MLPS=[list(m) for m in mlps], POOL_RADIUS=list(radii), NSAMPLE=list(nsample))
    if factor is not None:
        d['DOWNSAMPLE_FACTOR'] = factor
    return d


def pvrcnn_cfg(num_keypoints=2048, features_source=('bev', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'raw_points'), roi_per_image=128,
               nms_post_train=512, nms_pre_train=9000, dp_ratio=0.3):
    """PFE / POINT_HEAD / ROI_HEAD sections of detector3d/tools/cfgs/kitti_models/pv_rcnn.yaml:113-219 (values as data)."""
    pfe = dict(NAME='VoxelSetAbstraction', POINT_SOURCE='raw_points', NUM_KEYPOINTS=num_keypoints, NUM_OUTPUT_FEATURES=128, SAMPLE_METHOD='FPS',
               FEATURES_SOURCE=list(features_source),
               SA_LAYER=dict(raw_points=_sa([[16, 16], [16, 16]], [0.4, 0.8], [16, 16]),
                             x_conv1=_sa([[16, 16], [16, 16]], [0.4, 0.8], [16, 16], 1),
                             x_conv2=_sa([[32, 32], [32, 32]], [0.8, 1.2], [16, 32], 2),
                             x_conv3=_sa([[64, 64], [64, 64]], [1.2, 2.4], [16, 32], 4),
                             x_conv4=_sa([[64, 64], [64, 64]], [2.4, 4.8], [16, 32], 8)))
    point_head = dict(NAME='PointHeadSimple', CLS_FC=[256, 256], CLASS_AGNOSTIC=True, USE_POINT_FEATURES_BEFORE_FUSION=True,
                      TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]), LOSS_CONFIG=dict(LOSS_REG='smooth-l1', LOSS_WEIGHTS=dict(point_cls_weight=1.0)))
    roi_head = dict(
        NAME='PVRCNNHead', CLASS_AGNOSTIC=True, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=dp_ratio,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=nms_pre_train, NMS_POST_MAXSIZE=nms_post_train, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(GRID_SIZE=6, MLPS=[[64, 64], [64, 64]], POOL_RADIUS=[0.8, 1.6], NSAMPLE=[16, 16], POOL_METHOD='max_pool'),
        TARGET_CONFIG=dict(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=roi_per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='roi_iou',
                           CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='smooth-l1', CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7)))
    return pfe, point_head, roi_head


def _vector_pool(kind, reduced, post_msg, groups, **extra):
    d = dict(NAME='VectorPoolAggregationModuleMSG', NUM_GROUPS=len(groups), LOCAL_AGGREGATION_TYPE=kind, NUM_REDUCED_CHANNELS=reduced,
             NUM_CHANNELS_OF_LOCAL_AGGREGATION=32, MSG_POST_MLPS=[post_msg], **extra)
    for k, (voxels, dist, nsample, post) in enumerate(groups):
        d[f'GROUP_CFG_{k}'] = dict(NUM_LOCAL_VOXEL=list(voxels), MAX_NEIGHBOR_DISTANCE=dist, NEIGHBOR_NSAMPLE=nsample, POST_MLPS=[post, post])
    return d


# detector3d/tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml:76-140, 160-179 (values as data): the vector-pool SA_LAYERs of the PFE and the
# ROI_GRID_POOL of the PVRCNNHead.  FILTER_NEIGHBOR_WITH_ROI / RADIUS_OF_NEIGHBOR_WITH_ROI: VoxelSetAbstraction's RoI neighbour filter.
PVRCNNPP_SA_LAYER = dict(
    raw_points=_vector_pool('local_interpolation', 2, 32, [((2, 2, 2), 0.2, -1, 32), ((3, 3, 3), 0.4, -1, 32)],
                            FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=2.4),
    x_conv3=_vector_pool('local_interpolation', 32, 128, [((3, 3, 3), 1.2, -1, 64), ((3, 3, 3), 2.4, -1, 64)], DOWNSAMPLE_FACTOR=4,
                         INPUT_CHANNELS=64, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=4.0),
    x_conv4=_vector_pool('local_interpolation', 32, 128, [((3, 3, 3), 2.4, -1, 64), ((3, 3, 3), 4.8, -1, 64)], DOWNSAMPLE_FACTOR=8,
                         INPUT_CHANNELS=64, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=6.4))
PVRCNNPP_ROI_GRID_POOL = _vector_pool('voxel_random_choice', 30, 128, [((3, 3, 3), 0.8, 32, 64), ((3, 3, 3), 1.6, 32, 64)], GRID_SIZE=6)


def pvrcnn_model_cfg(**kw):
    pfe, point_head, roi_head = pvrcnn_cfg(**kw)
    pp = dict(SECOND_POST_PROCESSING, NMS_CONFIG=dict(SECOND_POST_PROCESSING['NMS_CONFIG'], NMS_THRESH=0.1))
    return dict(NAME='PVRCNN', VFE=dict(NAME='DynMeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=SECOND_BACKBONE_2D, DENSE_HEAD=SECOND_DENSE_HEAD,
                PFE=pfe, POINT_HEAD=point_head, ROI_HEAD=roi_head, POST_PROCESSING=pp)

# detector3d/tools/cfgs/kitti_models/voxel_rcnn_car.yaml:32-180 (values as data)
VOXELRCNN_CLASS_NAMES = ['Car']
VOXELRCNN_BACKBONE_2D = dict(NAME='BaseBEVBackbone', LAYER_NUMS=[5, 5], LAYER_STRIDES=[1, 2], NUM_FILTERS=[64, 128], UPSAMPLE_STRIDES=[1, 2],
                             NUM_UPSAMPLE_FILTERS=[128, 128])


def voxelrcnn_cfg(features_source=('x_conv2', 'x_conv3', 'x_conv4'), roi_per_image=128, nms_post_train=512, nms_pre_train=9000, dp_ratio=0.3):
    """ROI_HEAD section of voxel_rcnn_car.yaml:92-166."""
    radius = dict(x_conv2=0.4, x_conv3=0.8, x_conv4=1.6)
    layers = {s: dict(MLPS=[[32, 32]], QUERY_RANGES=[[4, 4, 4]], POOL_RADIUS=[radius[s]], NSAMPLE=[16], POOL_METHOD='max_pool') for s in features_source}
    return dict(
        NAME='VoxelRCNNHead', CLASS_AGNOSTIC=True, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=dp_ratio,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=nms_pre_train, NMS_POST_MAXSIZE=nms_post_train, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, USE_FAST_NMS=False, SCORE_THRESH=0.0, NMS_PRE_MAXSIZE=2048,
                                  NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(FEATURES_SOURCE=list(features_source), PRE_MLP=True, GRID_SIZE=6, POOL_LAYERS=layers),
        TARGET_CONFIG=dict(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=roi_per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='roi_iou',
                           CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='smooth-l1', CORNER_LOSS_REGULARIZATION=True, GRID_3D_IOU_LOSS=False,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, rcnn_iou3d_weight=1.0, code_weights=[1.0] * 7)))


def voxelrcnn_model_cfg(dynamic_vfe=False, **kw):
    """MODEL section of voxel_rcnn_car.yaml (one class: build with num_class=1 and VOXELRCNN_CLASS_NAMES); dynamic_vfe swaps MeanVFE for DynMeanVFE
    as waymo_models/voxel_rcnn_with_centerhead_dyn_voxel.yaml does."""
    head = dict(SECOND_DENSE_HEAD, ANCHOR_GENERATOR_CONFIG=[_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45)])
    pp = dict(SECOND_POST_PROCESSING, SCORE_THRESH=0.3, NMS_CONFIG=dict(SECOND_POST_PROCESSING['NMS_CONFIG'], NMS_THRESH=0.1))
    return dict(NAME='VoxelRCNN', VFE=dict(NAME='DynMeanVFE' if dynamic_vfe else 'MeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=VOXELRCNN_BACKBONE_2D, DENSE_HEAD=head,
                ROI_HEAD=voxelrcnn_cfg(**kw), POST_PROCESSING=pp)


def voxelrcnn_focal_model_cfg(dynamic_vfe=False, backbone=None, use_img=False, img_pretrain="../checkpoints/deeplabv3_resnet50_coco-cd0a2569.pth", **kw):
    """MODEL section of kitti_models/voxel_rcnn_car_focal_multimodal.yaml (:37-187): voxel_rcnn_car.yaml with BACKBONE_3D VoxelBackBone8xFocal.  The yaml
    sets USE_IMG: True with IMG_PRETRAIN at the checkpoint the reference downloads; use_img=True restates that (img_pretrain: a local file, or None
    for a randomly initialised image network), the default leaves the image branch out.  backbone: further BACKBONE_3D keys (TOPK, THRESHOLD,
    MASK_MULTI, SKIP_MASK_KERNEL, SKIP_MASK_KERNEL_IMG, ENLARGE_VOXEL_CHANNELS, last_pad); the yaml leaves them at the class defaults."""
    cfg = voxelrcnn_model_cfg(dynamic_vfe=dynamic_vfe, **kw)
    image = dict(USE_IMG=True, IMG_PRETRAIN=img_pretrain) if use_img else dict(USE_IMG=False)
    cfg['BACKBONE_3D'] = dict(NAME='VoxelBackBone8xFocal', **image, **(backbone or {}))
    return cfg


# detector3d/tools/cfgs/kitti_models/PartA2.yaml:31-170 (values as data)
def parta2_cfg(pool_size=12, max_points_per_voxel=128, num_features=128, roi_per_image=128, nms_post_train=512, nms_pre_train=9000, dp_ratio=0.3,
               shared_fc=(256, 256, 256)):
    """POINT_HEAD / ROI_HEAD sections of PartA2.yaml:95-160."""
    point_head = dict(NAME='PointIntraPartOffsetHead', CLS_FC=[], PART_FC=[], CLASS_AGNOSTIC=True, TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]),
                      LOSS_CONFIG=dict(LOSS_REG='smooth-l1', LOSS_WEIGHTS=dict(point_cls_weight=1.0, point_part_weight=1.0)))
    roi_head = dict(
        NAME='PartA2FCHead', CLASS_AGNOSTIC=True, SHARED_FC=list(shared_fc), CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=dp_ratio,
        SEG_MASK_SCORE_THRESH=0.3,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=nms_pre_train, NMS_POST_MAXSIZE=nms_post_train, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=100, NMS_THRESH=0.7)),
        ROI_AWARE_POOL=dict(POOL_SIZE=pool_size, NUM_FEATURES=num_features, MAX_POINTS_PER_VOXEL=max_points_per_voxel),
        TARGET_CONFIG=dict(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=roi_per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='roi_iou',
                           CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.65),
        LOSS_CONFIG=dict(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='smooth-l1', CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7)))
    return point_head, roi_head


def parta2_model_cfg(dynamic_vfe=False, **kw):
    """MODEL section of kitti_models/PartA2.yaml (its three anchors sit at bottom height -1.78); the keywords size the RoI head like
    voxelrcnn_model_cfg's.  dynamic_vfe swaps MeanVFE for DynMeanVFE."""
    point_head, roi_head = parta2_cfg(**kw)
    head = dict(SECOND_DENSE_HEAD, ANCHOR_GENERATOR_CONFIG=[_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45),
                                                            _anchor('Pedestrian', [0.8, 0.6, 1.73], -1.78, 0.5, 0.35),
                                                            _anchor('Cyclist', [1.76, 0.6, 1.73], -1.78, 0.5, 0.35)])
    pp = dict(SECOND_POST_PROCESSING, NMS_CONFIG=dict(SECOND_POST_PROCESSING['NMS_CONFIG'], NMS_THRESH=0.1))
    return dict(NAME='PartA2Net', VFE=dict(NAME='DynMeanVFE' if dynamic_vfe else 'MeanVFE'), BACKBONE_3D=dict(NAME='UNetV2'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=SECOND_BACKBONE_2D, DENSE_HEAD=head,
                POINT_HEAD=point_head, ROI_HEAD=roi_head, POST_PROCESSING=pp)

# detector3d/tools/cfgs/nuscenes_models/cbgs_voxel0075_res3d_centerpoint.yaml:1-140 (values as data)
NUSC_CLASS_NAMES = ['car', 'truck', 'construction_vehicle', 'bus', 'trailer', 'barrier', 'motorcycle', 'bicycle', 'pedestrian', 'traffic_cone']
CENTER_HEAD = dict(
    NAME='CenterHead', CLASS_AGNOSTIC=False,
    CLASS_NAMES_EACH_HEAD=[['car'], ['truck', 'construction_vehicle'], ['bus', 'trailer'], ['barrier'], ['motorcycle', 'bicycle'],
                           ['pedestrian', 'traffic_cone']],
    SHARED_CONV_CHANNEL=64, USE_BIAS_BEFORE_NORM=True, NUM_HM_CONV=2,
    SEPARATE_HEAD_CFG=dict(HEAD_ORDER=['center', 'center_z', 'dim', 'rot', 'vel'],
                           HEAD_DICT=dict(center=dict(out_channels=2, num_conv=2), center_z=dict(out_channels=1, num_conv=2),
                                          dim=dict(out_channels=3, num_conv=2), rot=dict(out_channels=2, num_conv=2), vel=dict(out_channels=2, num_conv=2))),
    TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=8, NUM_MAX_OBJS=500, GAUSSIAN_OVERLAP=0.1, MIN_RADIUS=2),
    LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=0.25, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0])),
    POST_PROCESSING=dict(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], MAX_OBJ_PER_SAMPLE=500,
                         NMS_CONFIG=dict(NMS_TYPE='nms_gpu', NMS_THRESH=0.2, NMS_PRE_MAXSIZE=1000, NMS_POST_MAXSIZE=83)))


# detector3d/tools/cfgs/kitti_models/second_iou.yaml:88-140 (values as data)
def second_iou_roi_head(in_channel=512, shared_fc=(256, 256), iou_fc=(256, 256), roi_per_image=128, train_post=512, test_post=100):
    return dict(
        NAME='SECONDHead', CLASS_AGNOSTIC=True, SHARED_FC=list(shared_fc), IOU_FC=list(iou_fc), DP_RATIO=0.3,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=train_post, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=1024, NMS_POST_MAXSIZE=test_post, NMS_THRESH=0.7)),
        ROI_GRID_POOL=dict(GRID_SIZE=7, IN_CHANNEL=in_channel, DOWNSAMPLE_RATIO=8),
        TARGET_CONFIG=dict(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=roi_per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                           CLS_SCORE_TYPE='roi_iou', CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8,
                           REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(IOU_LOSS='BinaryCrossEntropy', LOSS_WEIGHTS=dict(rcnn_iou_weight=1.0, code_weights=[1.0] * 7)))


SECOND_IOU_POST = dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, EVAL_METRIC='kitti',
                       NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE='nms_gpu', NMS_THRESH=0.01, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500,
                                       SCORE_TYPE='iou'))


def centerpoint_model_cfg():
    """MODEL section of nuscenes_models/cbgs_voxel0075_res3d_centerpoint.yaml:64-140 (values as data)."""
    return dict(NAME='CenterPoint', VFE=dict(NAME='MeanVFE'), BACKBONE_3D=dict(NAME='VoxelResBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=SECOND_BACKBONE_2D, DENSE_HEAD=CENTER_HEAD,
                POST_PROCESSING=dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], EVAL_METRIC='kitti'))


# detector3d/tools/cfgs/source-nuscenes/pvrcnn.yaml:60-215 (values as data): the SEE-VCN PV-RCNN -- one class, 4096 keypoints, no x_conv1/x_conv2 sources
DA_RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
DA_VOXEL = [0.1, 0.1, 0.15]


def see_pvrcnn_model_cfg(dynamic_vfe=True, **kw):
    kw.setdefault('num_keypoints', 4096)
    kw.setdefault('features_source', ('bev', 'x_conv3', 'x_conv4', 'raw_points'))
    pfe, point_head, roi_head = pvrcnn_cfg(**kw)
    roi_head['NMS_CONFIG']['TEST'] = dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=300, NMS_THRESH=0.85)
    head = dict(SECOND_DENSE_HEAD, ANCHOR_GENERATOR_CONFIG=[dict(_anchor('car', [4.2, 2.0, 1.6], 0, 0.55, 0.4))])
    pp = dict(SECOND_POST_PROCESSING, NMS_CONFIG=dict(SECOND_POST_PROCESSING['NMS_CONFIG'], NMS_THRESH=0.7, NMS_POST_MAXSIZE=500))
    return dict(NAME='PVRCNN', VFE=dict(NAME='DynMeanVFE' if dynamic_vfe else 'MeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=SECOND_BACKBONE_2D, DENSE_HEAD=head,
                PFE=pfe, POINT_HEAD=point_head, ROI_HEAD=roi_head, POST_PROCESSING=pp)


# detector3d/tools/cfgs/kitti_models/pointrcnn.yaml:22-138 and pointrcnn_iou.yaml (values as data)
def pointrcnn_cfg(npoints=(4096, 1024, 256, 64), roi_npoints=(128, 32, -1), num_sampled_points=512, roi_per_image=128, nms_pre_train=9000,
                  nms_post_train=512, nms_pre_test=9000, nms_post_test=100, cls_score_type='cls', use_bn=False):
    """BACKBONE_3D / POINT_HEAD / ROI_HEAD sections of pointrcnn.yaml; cls_score_type='roi_iou' gives pointrcnn_iou.yaml (its CLS_SCORE_TYPE and
    the two classification thresholds are all that differ).  The keywords scale the model down for tests; radii, sample counts and channel
    widths stay the yaml's."""
    assert cls_score_type in ('cls', 'roi_iou') and len(npoints) == 4 and len(roi_npoints) == 3
    backbone = dict(NAME='PointNet2MSG',
                    SA_CONFIG=dict(NPOINTS=list(npoints), RADIUS=[[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]], NSAMPLE=[[16, 32]] * 4,
                                   MLPS=[[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 196, 256], [128, 196, 256]],
                                         [[256, 256, 512], [256, 384, 512]]]),
                    FP_MLPS=[[128, 128], [256, 256], [512, 512], [512, 512]])
    point_head = dict(NAME='PointHeadBox', CLS_FC=[256, 256], REG_FC=[256, 256], CLASS_AGNOSTIC=False, USE_POINT_FEATURES_BEFORE_FUSION=False,
                      TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2], BOX_CODER='PointResidualCoder',
                                         BOX_CODER_CONFIG=dict(use_mean_size=True, mean_size=[[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])),
                      LOSS_CONFIG=dict(LOSS_REG='WeightedSmoothL1Loss', LOSS_WEIGHTS=dict(point_cls_weight=1.0, point_box_weight=1.0, code_weights=[1.0] * 8)))
    fg, bg = (0.6, 0.45) if cls_score_type == 'cls' else (0.7, 0.25)
    roi_head = dict(
        NAME='PointRCNNHead', CLASS_AGNOSTIC=True,
        ROI_POINT_POOL=dict(POOL_EXTRA_WIDTH=[0.0, 0.0, 0.0], NUM_SAMPLED_POINTS=num_sampled_points, DEPTH_NORMALIZER=70.0),
        XYZ_UP_LAYER=[128, 128], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=0.0, USE_BN=use_bn,
        SA_CONFIG=dict(NPOINTS=list(roi_npoints), RADIUS=[0.2, 0.4, 100], NSAMPLE=[16, 16, 16], MLPS=[[128, 128, 128], [128, 128, 256], [256, 256, 512]]),
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=nms_pre_train, NMS_POST_MAXSIZE=nms_post_train, NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE='nms_gpu', MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=nms_pre_test, NMS_POST_MAXSIZE=nms_post_test, NMS_THRESH=0.85)),
        TARGET_CONFIG=dict(BOX_CODER='ResidualCoder', ROI_PER_IMAGE=roi_per_image, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                           CLS_SCORE_TYPE=cls_score_type, CLS_FG_THRESH=fg, CLS_BG_THRESH=bg, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='smooth-l1', CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7)))
    return backbone, point_head, roi_head


def pointrcnn_model_cfg(**kw):
    """MODEL section of kitti_models/pointrcnn.yaml (pointrcnn_iou.yaml with cls_score_type='roi_iou'): no VFE, no BEV branch, no dense head.
    Build it with a dataset of 4 point features (x, y, z, intensity)."""
    backbone, point_head, roi_head = pointrcnn_cfg(**kw)
    pp = dict(SECOND_POST_PROCESSING, NMS_CONFIG=dict(SECOND_POST_PROCESSING['NMS_CONFIG'], NMS_THRESH=0.1))
    return dict(NAME='PointRCNN', BACKBONE_3D=backbone, POINT_HEAD=point_head, ROI_HEAD=roi_head, POST_PROCESSING=pp)


# detector3d/tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml:1-256 (values as data): PV-RCNN++ -- CenterHead proposals, SPC keypoints, vector-pool
# aggregation in the PFE and in the RoI grid pooling.  Range and voxel size of cfgs/dataset_configs/waymo_dataset.yaml are DA_RANGE / DA_VOXEL.
WAYMO_CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
PVRCNNPP_CENTER_HEAD = dict(
    NAME='CenterHead', CLASS_AGNOSTIC=False, CLASS_NAMES_EACH_HEAD=[['Vehicle', 'Pedestrian', 'Cyclist']],
    SHARED_CONV_CHANNEL=64, USE_BIAS_BEFORE_NORM=True, NUM_HM_CONV=2,
    SEPARATE_HEAD_CFG=dict(HEAD_ORDER=['center', 'center_z', 'dim', 'rot'],
                           HEAD_DICT=dict(center=dict(out_channels=2, num_conv=2), center_z=dict(out_channels=1, num_conv=2),
                                          dim=dict(out_channels=3, num_conv=2), rot=dict(out_channels=2, num_conv=2))),
    TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=8, NUM_MAX_OBJS=500, GAUSSIAN_OVERLAP=0.1, MIN_RADIUS=2),
    LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, code_weights=[1.0] * 8)),
    POST_PROCESSING=dict(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[-75.2, -75.2, -2, 75.2, 75.2, 4], MAX_OBJ_PER_SAMPLE=500,
                         NMS_CONFIG=dict(NMS_TYPE='nms_gpu', NMS_THRESH=0.7, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500)))


def pvrcnnpp_cfg(num_keypoints=4096, features_source=('bev', 'x_conv3', 'x_conv4', 'raw_points'), roi_per_image=128, nms_post_train=512,
                 nms_pre_train=9000, dp_ratio=0.3):
    """PFE / POINT_HEAD / ROI_HEAD sections of waymo_models/pv_rcnn_plusplus.yaml:72-241; the size keywords as in pvrcnn_cfg."""
    pfe = dict(NAME='VoxelSetAbstraction', POINT_SOURCE='raw_points', NUM_KEYPOINTS=num_keypoints, NUM_OUTPUT_FEATURES=90, SAMPLE_METHOD='SPC',
               SPC_SAMPLING=dict(NUM_SECTORS=6, SAMPLE_RADIUS_WITH_ROI=1.6), FEATURES_SOURCE=list(features_source),
               SA_LAYER={k: dict(v) for k, v in PVRCNNPP_SA_LAYER.items()})
    _, point_head, roi_head = pvrcnn_cfg(roi_per_image=roi_per_image, nms_post_train=nms_post_train, nms_pre_train=nms_pre_train, dp_ratio=dp_ratio)
    roi_head['NMS_CONFIG']['TEST']['SCORE_THRESH'] = 0.1
    roi_head['ROI_GRID_POOL'] = dict(PVRCNNPP_ROI_GRID_POOL)
    return pfe, point_head, roi_head


def pvrcnnpp_model_cfg(dynamic_vfe=False, **kw):
    pfe, point_head, roi_head = pvrcnnpp_cfg(**kw)
    pp = dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, EVAL_METRIC='waymo',
              NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE='nms_gpu', NMS_THRESH=0.7, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500))
    return dict(NAME='PVRCNNPlusPlus', VFE=dict(NAME='DynMeanVFE' if dynamic_vfe else 'MeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=SECOND_BACKBONE_2D, DENSE_HEAD=PVRCNNPP_CENTER_HEAD,
                PFE=pfe, POINT_HEAD=point_head, ROI_HEAD=roi_head, POST_PROCESSING=pp)


# ------------------------------------------------------------------------------------------------ multi-head anchor detectors (AnchorHeadMulti)
# detector3d/tools/cfgs/nuscenes_models/cbgs_second_multihead.yaml, cbgs_pp_multihead.yaml and kitti_models/second_multihead.yaml, MODEL sections
# (values as data).  The two nuScenes files share anchors (only feature_map_stride differs), heads, coder and losses.
def _mh_anchor(name, size, bottom, matched, unmatched, stride):
    return dict(class_name=name, anchor_sizes=[size], anchor_rotations=[0, 1.57], anchor_bottom_heights=[bottom], align_center=False,
                feature_map_stride=stride, matched_threshold=matched, unmatched_threshold=unmatched)


_NUSC_MH_ANCHORS = [('car', [4.63, 1.97, 1.74], -0.95, 0.6, 0.45), ('truck', [6.93, 2.51, 2.84], -0.6, 0.55, 0.4),
                    ('construction_vehicle', [6.37, 2.85, 3.19], -0.225, 0.5, 0.35), ('bus', [10.5, 2.94, 3.47], -0.085, 0.55, 0.4),
                    ('trailer', [12.29, 2.90, 3.87], 0.115, 0.5, 0.35), ('barrier', [0.50, 2.53, 0.98], -1.33, 0.55, 0.4),
                    ('motorcycle', [2.11, 0.77, 1.47], -1.085, 0.5, 0.3), ('bicycle', [1.70, 0.60, 1.28], -1.18, 0.5, 0.35),
                    ('pedestrian', [0.73, 0.67, 1.77], -0.935, 0.6, 0.4), ('traffic_cone', [0.41, 0.41, 1.07], -1.285, 0.6, 0.4)]
_KITTI_MH_ANCHORS = [('Car', [3.9, 1.6, 1.56], -1.6, 0.6, 0.45), ('Pedestrian', [0.8, 0.6, 1.73], -1.6, 0.5, 0.35),
                     ('Cyclist', [1.76, 0.6, 1.73], -1.6, 0.5, 0.35)]
_MH_TARGET_ASSIGNER = dict(NAME='AxisAlignedTargetAssigner', POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False,
                           BOX_CODER='ResidualCoder')
NUSC_PP_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
NUSC_PP_VOXEL = dict(VOXEL_SIZE=[0.2, 0.2, 8.0], MAX_POINTS_PER_VOXEL=20, MAX_NUMBER_OF_VOXELS={'train': 30000, 'test': 30000})


def _nusc_multihead_dense_head(stride):
    return dict(
        NAME='AnchorHeadMulti', CLASS_AGNOSTIC=False, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2, USE_MULTIHEAD=True,
        SEPARATE_MULTIHEAD=True, ANCHOR_GENERATOR_CONFIG=[_mh_anchor(*a, stride) for a in _NUSC_MH_ANCHORS], SHARED_CONV_NUM_FILTER=64,
        RPN_HEAD_CFGS=[dict(HEAD_CLS_NAME=['car']), dict(HEAD_CLS_NAME=['truck', 'construction_vehicle']), dict(HEAD_CLS_NAME=['bus', 'trailer']),
                       dict(HEAD_CLS_NAME=['barrier']), dict(HEAD_CLS_NAME=['motorcycle', 'bicycle']),
                       dict(HEAD_CLS_NAME=['pedestrian', 'traffic_cone'])],
        SEPARATE_REG_CONFIG=dict(NUM_MIDDLE_CONV=1, NUM_MIDDLE_FILTER=64, REG_LIST=['reg:2', 'height:1', 'size:3', 'angle:2', 'velo:2']),
        TARGET_ASSIGNER_CONFIG=dict(_MH_TARGET_ASSIGNER, BOX_CODER_CONFIG=dict(code_size=9, encode_angle_by_sincos=True)),
        LOSS_CONFIG=dict(REG_LOSS_TYPE='WeightedL1Loss',
                         LOSS_WEIGHTS=dict(pos_cls_weight=1.0, neg_cls_weight=2.0, cls_weight=1.0, loc_weight=0.25, dir_weight=0.2,
                                           code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2])))


def _mh_post_processing(thresh, pre, post, **extra):
    return dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], **extra, SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, EVAL_METRIC='kitti',
                NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=thresh, NMS_PRE_MAXSIZE=pre, NMS_POST_MAXSIZE=post))


def second_multihead_model_cfg(dataset='nuscenes'):
    """MODEL section of nuscenes_models/cbgs_second_multihead.yaml ('nuscenes': 10 classes in 6 heads, 9-d boxes with the sin/cos heading
    code, no direction classifier) or kitti_models/second_multihead.yaml ('kitti': 3 single-class heads, 7-d boxes, direction classifier)."""
    if dataset == 'nuscenes':
        return dict(NAME='SECONDNet', VFE=dict(NAME='MeanVFE'), BACKBONE_3D=dict(NAME='VoxelResBackBone8x'),
                    MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=dict(SECOND_BACKBONE_2D),
                    DENSE_HEAD=_nusc_multihead_dense_head(8), POST_PROCESSING=_mh_post_processing(0.2, 1000, 83))
    assert dataset == 'kitti', dataset
    head = dict(
        NAME='AnchorHeadMulti', CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
        USE_MULTIHEAD=True, SEPARATE_MULTIHEAD=True, ANCHOR_GENERATOR_CONFIG=[_mh_anchor(*a, 8) for a in _KITTI_MH_ANCHORS],
        SHARED_CONV_NUM_FILTER=64, RPN_HEAD_CFGS=[dict(HEAD_CLS_NAME=['Car']), dict(HEAD_CLS_NAME=['Pedestrian']), dict(HEAD_CLS_NAME=['Cyclist'])],
        TARGET_ASSIGNER_CONFIG=dict(_MH_TARGET_ASSIGNER),
        LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])))
    return dict(NAME='SECONDNet', VFE=dict(NAME='MeanVFE'), BACKBONE_3D=dict(NAME='VoxelBackBone8x'),
                MAP_TO_BEV=dict(NAME='HeightCompression', NUM_BEV_FEATURES=256), BACKBONE_2D=dict(SECOND_BACKBONE_2D), DENSE_HEAD=head,
                POST_PROCESSING=_mh_post_processing(0.1, 4096, 500, MULTI_CLASSES_NMS=True))


def pp_multihead_model_cfg():
    """MODEL section of nuscenes_models/cbgs_pp_multihead.yaml (pillars of NUSC_PP_VOXEL over NUSC_PP_RANGE, a BEV backbone whose first
    up-sampling level is a stride-2 convolution, anchors at feature_map_stride 4)."""
    return dict(NAME='PointPillar', VFE=dict(PP_VFE), MAP_TO_BEV=dict(PP_MAP_TO_BEV),
                BACKBONE_2D=dict(NAME='BaseBEVBackbone', LAYER_NUMS=[3, 5, 5], LAYER_STRIDES=[2, 2, 2], NUM_FILTERS=[64, 128, 256],
                                 UPSAMPLE_STRIDES=[0.5, 1, 2], NUM_UPSAMPLE_FILTERS=[128, 128, 128]),
                DENSE_HEAD=_nusc_multihead_dense_head(4), POST_PROCESSING=_mh_post_processing(0.2, 1000, 83))


# detector3d/tools/cfgs/kitti_models/CaDDN.yaml:5-156 (values as data)
CADDN_RANGE = [2, -30.08, -3.0, 46.8, 30.08, 1.0]
CADDN_VOXEL = [0.16, 0.16, 0.16]
CADDN_DEPTH_DOWNSAMPLE_FACTOR = 4
CADDN_PRETRAINED_PATH = '../checkpoints/deeplabv3_resnet101_coco-586e9e4e.pth'


def caddn_model_cfg(backbone_name='ResNet101', pretrained_path=CADDN_PRETRAINED_PATH, feat_channels=64, num_bins=80, depth_min=2.0, depth_max=46.8,
                    disc_mode='LID', layer_nums=(10, 10, 10), sampler_mode='bilinear'):
    """MODEL section of kitti_models/CaDDN.yaml.  The keywords scale the model down for tests (a ResNet50 without a checkpoint, fewer channels,
    bins and BEV layers); the defaults are the YAML's.  The dataset supplies grid_size, point_cloud_range and depth_downsample_factor."""
    vfe = dict(
        NAME='ImageVFE',
        FFN=dict(NAME='DepthFFN',
                 DDN=dict(NAME='DDNDeepLabV3', BACKBONE_NAME=backbone_name, ARGS=dict(feat_extract_layer='layer1', pretrained_path=pretrained_path)),
                 CHANNEL_REDUCE=dict(in_channels=256, out_channels=feat_channels, kernel_size=1, stride=1, bias=False),
                 DISCRETIZE=dict(mode=disc_mode, num_bins=num_bins, depth_min=depth_min, depth_max=depth_max),
                 LOSS=dict(NAME='DDNLoss', ARGS=dict(weight=3.0, alpha=0.25, gamma=2.0, fg_weight=13, bg_weight=1))),
        F2V=dict(NAME='FrustumToVoxel', SAMPLER=dict(mode=sampler_mode, padding_mode='zeros')))
    return dict(NAME='CaDDN', VFE=vfe,
                MAP_TO_BEV=dict(NAME='Conv2DCollapse', NUM_BEV_FEATURES=feat_channels, ARGS=dict(kernel_size=1, stride=1, bias=False)),
                BACKBONE_2D=dict(PP_BACKBONE_2D, LAYER_NUMS=list(layer_nums)), DENSE_HEAD=PP_DENSE_HEAD, POST_PROCESSING=SECOND_POST_PROCESSING)


def pointpillar_newaugs_augmentor_cfg():
    """DATA_CONFIG.DATA_AUGMENTOR of detector3d/tools/cfgs/kitti_models/pointpillar_newaugs.yaml:23-70, values copied as data.  The YAML spells the
    world translation's key WORLD_TRANSLATION_RANGE while the code reads NOISE_TRANSLATE_STD: with that entry enabled the reference raises, and so
    does BatchDataAugmentor unless the caller adds the key."""
    return dict(
        DISABLE_AUG_LIST=['random_world_frustum_dropout', 'random_local_frustum_dropout', 'random_local_translation'],
        AUG_CONFIG_LIST=[
            dict(NAME='gt_sampling', USE_ROAD_PLANE=False, DB_INFO_PATH=['kitti_dbinfos_train.pkl'],
                 PREPARE=dict(filter_by_min_points=['Car:5', 'Pedestrian:5', 'Cyclist:5'], filter_by_difficulty=[-1, 2]),
                 SAMPLE_GROUPS=['Car:15', 'Pedestrian:15', 'Cyclist:15'], NUM_POINT_FEATURES=4, DATABASE_WITH_FAKELIDAR=False,
                 REMOVE_EXTRA_WIDTH=[0.0, 0.0, 0.0], LIMIT_WHOLE_SCENE=False),
            dict(NAME='random_local_rotation', LOCAL_ROT_ANGLE=[-0.15707963267, 0.15707963267]),
            dict(NAME='random_local_scaling', LOCAL_SCALE_RANGE=[0.95, 1.05]),
            dict(NAME='random_world_flip', ALONG_AXIS_LIST=['x']),
            dict(NAME='random_world_rotation', WORLD_ROT_ANGLE=[-0.78539816, 0.78539816]),
            dict(NAME='random_world_scaling', WORLD_SCALE_RANGE=[0.95, 1.05]),
            dict(NAME='random_world_translation', WORLD_TRANSLATION_RANGE=[-0.2, 0.2], ALONG_AXIS_LIST=['x', 'y', 'z']),
            dict(NAME='random_local_translation', LOCAL_TRANSLATION_RANGE=[0.95, 1.05], ALONG_AXIS_LIST=['x', 'y', 'z']),
            dict(NAME='random_world_frustum_dropout', INTENSITY_RANGE=[0, 0.2], DIRECTION=['top']),
            dict(NAME='random_local_frustum_dropout', INTENSITY_RANGE=[0, 0.2], DIRECTION=['top'])])


def pointpillar_pyramid_aug_augmentor_cfg():
    """DATA_CONFIG.DATA_AUGMENTOR of detector3d/tools/cfgs/kitti_models/pointpillar_pyramid_aug.yaml:23-57, values copied as data, with
    USE_ROAD_PLANE=False: road planes are not built (the YAML says True).  The pyramid entry follows gt_sampling, so BatchDataAugmentor runs this
    queue staged: forward() takes one RandomState per scene."""
    return dict(
        DISABLE_AUG_LIST=['placeholder'],
        AUG_CONFIG_LIST=[
            dict(NAME='gt_sampling', USE_ROAD_PLANE=False, DB_INFO_PATH=['kitti_dbinfos_train.pkl'],
                 PREPARE=dict(filter_by_min_points=['Car:5', 'Pedestrian:5', 'Cyclist:5'], filter_by_difficulty=[-1]),
                 SAMPLE_GROUPS=['Car:15', 'Pedestrian:15', 'Cyclist:15'], NUM_POINT_FEATURES=4, DATABASE_WITH_FAKELIDAR=False,
                 REMOVE_EXTRA_WIDTH=[0.0, 0.0, 0.0], LIMIT_WHOLE_SCENE=False),
            dict(NAME='random_world_flip', ALONG_AXIS_LIST=['x']),
            dict(NAME='random_world_rotation', WORLD_ROT_ANGLE=[-0.78539816, 0.78539816]),
            dict(NAME='random_world_scaling', WORLD_SCALE_RANGE=[0.95, 1.05]),
            dict(NAME='random_local_pyramid_aug', DROP_PROB=0.25, SPARSIFY_PROB=0.05, SPARSIFY_MAX_NUM=50, SWAP_PROB=0.1, SWAP_MAX_NUM=50)])
