"""The focal image branch on the CPU: the restatement of tests/focal_image_reference.py against the reference's own Calibration
(tests/golden/focal_image.npz, made by golden/make_focal_image_golden.py), the restated Calibration class against the same file, the 4-tap
statement against F.interpolate in float64, the cases' properties and mask share, the exported symbols, the two pinned refusals and the
construction of the multimodal backbone."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

import focal_image_reference as FI

NEW_SYMBOLS = ("sv_focal_image_pixels", "sv_focal_image_sample", "sv_focal_image_sample_grad_scratch_bytes", "sv_focal_image_sample_grad")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "focal_image.npz"))


@pytest.fixture(scope="module")
def cases():
    return {name: FI.make_case(name) for name in FI.CASE_NAMES}


# ---------------------------------------------------------------------------------------------------------------- 1. restatement vs the golden
@pytest.mark.parametrize("name", FI.CASE_NAMES)
def test_restatement_matches_reference_projection(gold, cases, name):
    case = cases[name]
    coords = case["coords"]
    assert np.array_equal(coords, gold[name + "_coords"])
    centres = FI.centres32(case, coords)
    # cos / sin in fp32 are the one step whose bits a numpy build may change: 4 ulp of 1 on coordinates below 128 m
    np.testing.assert_allclose(centres, gold[name + "_centres"], rtol=0, atol=128 * FI.TRIG_ULPS * 2 ** -23)
    u64, v64, rz, bu, bv = FI.project64(case, case["calibs"], coords)
    mask = FI.pixel_mask(u64, v64, rz, bu, bv)
    keep = ~mask
    ref = gold[name + "_img"]
    u32, v32, _ = FI.project32(case["calibs"], coords, gold[name + "_centres"])
    for got in (ref, np.stack([u32, v32], axis=1)):             # the reference's own float32 result and the restated float32 path
        assert (np.abs(got[keep, 0] - u64[keep]) <= bu[keep]).all() and (np.abs(got[keep, 1] - v64[keep]) <= bv[keep]).all()
        assert np.array_equal(FI.pixels(got[:, 0], got[:, 1], case["image"])[keep], FI.pixels(u64, v64, case["image"])[keep])


# ---------------------------------------------------------------------------------------------------------------- 2. the restated Calibration
def test_restated_calibration_matches_reference(gold):
    from seevcn_amd.pcdet.utils import calibration_kitti as CK
    c = FI.make_calib(FI.KITTI_IMAGE, 0)
    cal = CK.Calibration({"P2": c.P2, "R0": c.R0, "Tr_velo2cam": c.V2C})
    np.testing.assert_allclose([cal.cu, cal.cv, cal.fu, cal.fv, cal.tx, cal.ty], gold["cal_scalars"], rtol=1e-7)
    tol = dict(rtol=1e-5, atol=1e-4)                            # float32 BLAS products: the order of the sums is the build's
    rect = cal.lidar_to_rect(gold["cal_lidar"])
    assert rect.dtype == np.float32
    np.testing.assert_allclose(rect, gold["cal_rect"], **tol)
    img, depth = cal.rect_to_img(gold["cal_rect"])
    np.testing.assert_allclose(img, gold["cal_img"], **tol)
    np.testing.assert_allclose(depth, gold["cal_depth"], **tol)
    img2, depth2 = cal.lidar_to_img(gold["cal_lidar"])
    np.testing.assert_allclose(img2, gold["cal_img"], rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(depth2, gold["cal_depth"], **tol)
    np.testing.assert_allclose(cal.rect_to_lidar(gold["cal_rect"]), gold["cal_back"], **tol)
    np.testing.assert_allclose(cal.rect_to_lidar(gold["cal_rect"]), gold["cal_lidar"], rtol=1e-4, atol=1e-3)         # and it inverts lidar_to_rect
    np.testing.assert_allclose(cal.img_to_rect(gold["cal_img"][:, 0], gold["cal_img"][:, 1], gold["cal_depth"]), gold["cal_unproject"], **tol)
    boxes, corners = cal.corners3d_to_img_boxes(gold["cal_corners"])
    np.testing.assert_allclose(boxes, gold["cal_boxes"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(corners, gold["cal_boxes_corner"], rtol=1e-6, atol=1e-6)
    assert cal.cart_to_hom(gold["cal_lidar"]).shape == (200, 4)
    # the packer: M as lidar_to_rect forms it, P2 behind it, any object with the three matrices
    table = CK.pack_calib_host([c, cal])
    assert table.shape == (2, 24) and table.dtype == np.float32
    M, Merr = FI.calib_matrix(c)
    assert (np.abs(table[0, :12].reshape(4, 3).astype(np.float64) - M) <= Merr).all()
    assert np.array_equal(table[0, 12:].reshape(3, 4), c.P2) and np.array_equal(table[0], table[1])
    assert tuple(CK.pack_calib([c], torch.device("cpu")).shape) == (1, 24)


# ---------------------------------------------------------------------------------------------------------------- 3. the 4-tap statement
@pytest.mark.parametrize("feat,image", [((12, 40), (47, 159)), ((94, 311), (375, 1242)), ((3, 4), (11, 13)), ((12, 40), (12, 40))],
                         ids=["12x40-47x159", "94x311-375x1242", "3x4-11x13", "equal"])
def test_four_taps_equal_interpolate_in_float64(feat, image):
    rng = np.random.RandomState(3)
    features = rng.randn(1, feat[0], feat[1], 2).astype(np.float32)
    pix = np.arange(image[0] * image[1], dtype=np.int32)                 # every pixel of the image
    coords = np.zeros((len(pix), 4), np.int32)
    mine, _ = FI.image_rows64(features, coords, pix, image)
    want = FI.image_rows_interp64(features, coords, pix, image)
    assert np.abs(mine - want).max() <= 1e-12
    if feat != image:
        px, w32, w64 = FI.taps(image, feat, pix)
        assert px.min() >= 0 and px.max() < feat[0] * feat[1]
        assert np.abs(w64.sum(axis=1) - 1).max() <= 1e-15 and np.abs(w32.astype(np.float64) - w64).max() <= 6 * FI.U


# ---------------------------------------------------------------------------------------------------------------- 4. the cases and the mask cap
@pytest.mark.parametrize("name", FI.CASE_NAMES)
def test_cases_hold_their_edges_and_mask_cap(cases, name):
    case = cases[name]
    coords, (H, W) = case["coords"], case["image"]
    u, v, rz, bu, bv = FI.project64(case, case["calibs"], coords)
    mask = FI.pixel_mask(u, v, rz, bu, bv)
    assert mask.mean() <= FI.MASK_CAP, mask.mean()
    pix = FI.pixels(u, v, (H, W))
    keep = ~mask
    assert (pix[keep] >= 0).sum() > 0.5 * len(pix) and (pix[keep] < 0).sum() > 0.1 * len(pix)            # inside and outside voxels
    assert ((u > -1) & (u < 0) & (pix >= 0) & (pix % W == 0) & keep).any()                                # u in (-1, 0) truncates to 0 and stays
    scenes = coords[:, 0]
    if min(case["rows"]) > 0:
        assert (np.diff(scenes) != 0).sum() > len(scenes) / 4                                              # the scenes interleave
    _, longest = FI.grad_loop32(case, pix, case["g_sum"])
    B, h, w, C = case["features"].shape
    hit = np.zeros(B * h * w, bool)
    ok = pix >= 0
    if (h, w) == (H, W):
        hit[scenes[ok] * h * w + pix[ok]] = True
    else:
        px, _, _ = FI.taps((H, W), (h, w), pix[ok])
        hit[(scenes[ok, None] * h * w + px).reshape(-1)] = True
    assert not hit.all()                                                                                   # pixels hit by no voxel
    if name == "ratio":
        assert longest >= 24                                                                               # a pixel hit by dozens of voxels
        assert ((rz < 0) & (pix >= 0) & keep).sum() > 100                                                  # behind the camera, inside the image
        assert case["aug"]["flip_x"] == [True, False] and case["aug"]["flip_y"] == [False, True]
    if name == "tiny":
        assert (scenes == 0).all() and case["B"] == 2 and not case["aug"]                                  # an empty scene, no augmentation key
    present = set()
    for c in FI.CASES:
        present |= {(key, key in c["aug"]) for key in ("noise_scale", "noise_rot", "flip_x", "flip_y")}
    assert len(present) == 8                                                                               # every key present in one case, absent in another


def test_pixels_truncate_and_filter_as_the_reference():
    u = np.array([-0.5, 0.0, 12.99, 13.0, -1.0, 5.5, np.nan, np.inf, 3.2])
    v = np.array([2.5, -0.99, 10.99, 3.0, 3.0, 11.0, 1.0, 1.0, -np.inf])
    assert FI.pixels(u, v, (11, 13)).tolist() == [2 * 13, 0, 10 * 13 + 12, -1, -1, -1, -1, -1, -1]


# ---------------------------------------------------------------------------------------------------------------- 5. the library exports them
def test_library_exports_the_image_entries(hip_lib):
    import seevcn_amd._lib as L
    with open(L.HEADER_PATH) as f:
        protos = L.parse_declarations(f.read())
    for name in NEW_SYMBOLS:
        assert hasattr(hip_lib, name), name
        assert name in L.SIGNATURES and name in protos
    assert hip_lib.sv_focal_image_sample_grad_scratch_bytes(10, 2, 12, 40, 47, 159) > 0
    assert hip_lib.sv_focal_image_sample_grad_scratch_bytes(10, 2, 12, 40, 12, 40) < hip_lib.sv_focal_image_sample_grad_scratch_bytes(10, 2, 12, 40, 47, 159)
    assert hip_lib.sv_focal_image_sample_grad_scratch_bytes(1 << 29, 2, 12, 40, 47, 159) == 0               # 4 n = 2^31
    assert hip_lib.sv_focal_image_sample_grad_scratch_bytes((1 << 29) - 1, 2, 12, 40, 47, 159) > 0
    assert hip_lib.sv_focal_image_sample_grad_scratch_bytes(10, 1 << 11, 1 << 10, 1 << 10, 47, 159) == 0     # B h w = 2^31


# ---------------------------------------------------------------------------------------------------------------- 6. the pinned refusals
def test_pinned_refusals_still_raise():
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv import FocalSparseConv
    from seevcn_amd.pcdet.models.backbones_3d.spconv_backbone_focal import VoxelBackBone8xFocal
    norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    with pytest.raises(NotImplementedError, match="DeepLabV3") as e:
        FocalSparseConv(16, 16, voxel_stride=1, norm_fn=norm_fn, indice_key="f", use_img=True)
    assert "FocalSparseConvMultimodal" in str(e.value)
    with pytest.raises(NotImplementedError, match="DeepLabV3") as e:
        VoxelBackBone8xFocal(dict(NAME="VoxelBackBone8xFocal", USE_IMG=True), 4, [1408, 1600, 40])
    assert "download" in str(e.value)
    with pytest.raises(NotImplementedError, match="DeepLabV3"):
        VoxelBackBone8xFocal(dict(NAME="VoxelBackBone8xFocal", USE_IMG=True, IMG_PRETRAIN="/nonexistent/deeplabv3.pth"), 4, [1408, 1600, 40])


# ---------------------------------------------------------------------------------------------------------------- 7. construction on the CPU
def test_multimodal_backbone_constructs_with_reference_names(tmp_path):
    import seevcn_amd.pcdet.model_cfgs as C
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv.focal_sparse_conv import FocalSparseConv, FocalSparseConvMultimodal
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv.SemanticSeg import PyramidFeat2D
    from seevcn_amd.pcdet.models.backbones_3d.spconv_backbone_focal import VoxelBackBone8xFocal
    assert C.voxelrcnn_focal_model_cfg()["BACKBONE_3D"] == dict(NAME="VoxelBackBone8xFocal", USE_IMG=False)
    cfg = C.voxelrcnn_focal_model_cfg(use_img=True, img_pretrain=None)
    assert cfg["BACKBONE_3D"] == dict(NAME="VoxelBackBone8xFocal", USE_IMG=True, IMG_PRETRAIN=None)
    assert C.voxelrcnn_focal_model_cfg(use_img=True)["BACKBONE_3D"]["IMG_PRETRAIN"].endswith("deeplabv3_resnet50_coco-cd0a2569.pth")
    torch.manual_seed(0)
    m = VoxelBackBone8xFocal(cfg["BACKBONE_3D"], 4, [1408, 1600, 40])
    sd = m.state_dict()
    for key, shape in [("semseg.ifn.model.backbone.conv1.weight", (64, 3, 7, 7)), ("semseg.ifn.model.backbone.layer1.0.conv1.weight", (64, 64, 1, 1)),
                       ("semseg.ifn.model.backbone.layer4.2.conv3.weight", (2048, 512, 1, 1)), ("semseg.ifn.model.classifier.4.weight", (21, 256, 1, 1)),
                       ("semseg.reduce_blocks.0.conv.weight", (16, 256, 1, 1)), ("semseg.reduce_blocks.0.bn.weight", (16,)),
                       ("conv_focal_multimodal.conv.weight", (16, 3, 3, 3, 16)), ("conv_focal_multimodal.bn1.weight", (16,)),
                       ("conv_focal_multimodal.conv_imp.weight", (27, 3, 3, 3, 32))]:
        assert tuple(sd[key].shape) == shape, key
    assert not any("aux_classifier" in k or "semseg.reduce_blocks.0.conv.bias" in k for k in sd)
    layer = m.conv_focal_multimodal
    assert isinstance(layer, FocalSparseConvMultimodal) and isinstance(layer, FocalSparseConv) and isinstance(m.semseg, PyramidFeat2D)
    assert layer.use_img and layer.voxel_stride == 1 and layer.topk is True and layer.skip_mask_kernel is False
    assert layer.conv.indice_key == "spconv_focal_multimodal" and layer.conv_imp.indice_key == "spconv_focal_multimodal_imp"
    assert VoxelBackBone8xFocal(dict(cfg["BACKBONE_3D"], SKIP_MASK_KERNEL_IMG=True), 4, [1408, 1600, 40]).conv_focal_multimodal.skip_mask_kernel is True
    # random initialisation: no normalisation; layer1 features at a quarter of the image, reduced to 16 channels; the ResNet stops behind layer1
    assert not m.semseg.ifn.pretrained and not hasattr(m.semseg.ifn, "norm_mean")
    with torch.no_grad():
        out = m.semseg.eval()(torch.randn(1, 3, 32, 48))
    assert list(out) == ["layer1_feat2d"] and tuple(out["layer1_feat2d"].shape) == (1, 16, 8, 12)
    # an existing file is loaded, and then the images are normalised
    ck = {k[len("semseg.ifn.model."):]: torch.full_like(v, 0.25) for k, v in sd.items() if k.startswith("semseg.ifn.model.backbone.layer1.0.conv1")}
    ck["aux_classifier.0.weight"] = torch.zeros(1)                          # a key the model lacks is ignored, as the reference's strict=False does
    path = str(tmp_path / "deeplab.pth")
    torch.save(ck, path)
    loaded = VoxelBackBone8xFocal(dict(cfg["BACKBONE_3D"], IMG_PRETRAIN=path), 4, [1408, 1600, 40])
    assert loaded.semseg.ifn.pretrained and (loaded.state_dict()["semseg.ifn.model.backbone.layer1.0.conv1.weight"] == 0.25).all()
    assert torch.allclose(loaded.semseg.ifn.norm_mean, torch.tensor([0.485, 0.456, 0.406]))


def test_world_draws_to_batch_and_aug_table():
    from seevcn_amd.pcdet.datasets.augmentor.data_augmentor import world_draws_to_batch
    from seevcn_amd.spconv.focal import image_aug_table
    draws = [[("gt_sampling", None), ("flip_x", True), ("rotation", 0.25), ("scaling", 1.03)], [("flip_x", False), ("rotation", -0.5), ("scaling", 0.97)]]
    got = world_draws_to_batch(draws)
    assert set(got) == {"noise_scale", "noise_rot", "flip_x", "flip_y"}
    assert got["flip_x"].tolist() == [True, False] and got["flip_y"].tolist() == [False, False] and got["flip_x"].dtype == torch.bool
    assert got["noise_rot"].tolist() == [0.25, -0.5] and got["noise_scale"].dtype == torch.float32
    np.testing.assert_array_equal(got["noise_scale"].numpy(), np.array([1.03, 0.97], np.float32))
    table = image_aug_table(got, 2, torch.device("cpu"))
    np.testing.assert_array_equal(table.numpy(), np.array([[1.03, 0.25, 1, 0], [0.97, -0.5, 0, 0]], np.float32))
    np.testing.assert_array_equal(image_aug_table({}, 3, torch.device("cpu")).numpy(), np.tile(np.array([[1, 0, 0, 0]], np.float32), (3, 1)))
