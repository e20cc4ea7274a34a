"""CaDDN's frustum -> voxel sampling on the HIP kernels of csrc/frustum_sample.hip: the sampling grid of FrustumGridGenerator and the fused
create_frustum_features + grid_sample with its order-fixed gradient.  No CPU fallback."""
import ctypes

import torch

from ... import _lib

MODES = {"UD": 0, "LID": 1, "SID": 2}


def _geometry(grid_size, pc_range, disc_cfg):
    X, Y, Z = (int(v) for v in grid_size)
    rng = _lib.host_array(ctypes.c_float, [float(v) for v in pc_range])
    mode = disc_cfg["mode"]
    if mode not in MODES:
        raise NotImplementedError(mode)
    return X, Y, Z, rng, MODES[mode], float(disc_cfg["depth_min"]), float(disc_cfg["depth_max"]), int(disc_cfg["num_bins"])


def _calib(lidar_to_cam, cam_to_img, image_shape):
    _lib.require_cuda(lidar_to_cam, cam_to_img, image_shape)
    B = lidar_to_cam.shape[0]
    assert lidar_to_cam.shape[1:] == (4, 4) and cam_to_img.shape == (B, 3, 4) and image_shape.shape == (B, 2)
    return lidar_to_cam.float().contiguous(), cam_to_img.float().contiguous(), image_shape.to(torch.int32).contiguous()      # device ops, no host read


def frustum_grid(lidar_to_cam, cam_to_img, image_shape, grid_size, pc_range, disc_cfg):
    """(B, X, Y, Z, 3) normalised sampling grid = FrustumGridGenerator.forward"""
    l2c, c2i, ishape = _calib(lidar_to_cam, cam_to_img, image_shape)
    X, Y, Z, rng, mode, dmin, dmax, nbins = _geometry(grid_size, pc_range, disc_cfg)
    B = l2c.shape[0]
    out = torch.empty((B, X, Y, Z, 3), dtype=torch.float32, device=l2c.device)
    _lib.launch("sv_frustum_grid", _lib.ptr(l2c), _lib.ptr(c2i), _lib.ptr(ishape), B, X, Y, Z, rng, mode, dmin, dmax, nbins, _lib.ptr(out))
    return out


def _channels_last_storage(t):
    """the (B, H, W, C) storage of a (B, C, H, W) tensor, without a copy when it is channels_last already"""
    return t.permute(0, 2, 3, 1).contiguous()


class _FrustumToVoxel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image_features, depth_probs, l2c, c2i, ishape, geom):
        X, Y, Z, rng, mode, dmin, dmax, nbins = geom
        f = _channels_last_storage(image_features.float())
        p = _channels_last_storage(depth_probs.float())
        B, H, W, C = f.shape
        assert p.shape == (B, H, W, nbins + 1), "depth_probs must be (B, num_bins + 1, H, W) on the feature map's grid"
        store = torch.empty((B, Y, X, C, Z), dtype=torch.float32, device=f.device)
        _lib.launch("sv_frustum_to_voxel", _lib.ptr(f), _lib.ptr(p), _lib.ptr(l2c), _lib.ptr(c2i), _lib.ptr(ishape), B, C, nbins, H, W, X, Y, Z, rng, mode,
                    dmin, dmax, _lib.ptr(store))
        ctx.save_for_backward(f, p, l2c, c2i, ishape)
        ctx.geom = geom
        return store.permute(0, 3, 4, 1, 2)                                 # (B, C, Z, Y, X), the reference's shape

    @staticmethod
    def backward(ctx, grad):
        f, p, l2c, c2i, ishape = ctx.saved_tensors
        X, Y, Z, rng, mode, dmin, dmax, nbins = ctx.geom
        B, H, W, C = f.shape
        g = grad.float().permute(0, 3, 4, 1, 2).contiguous()                # (B, Y, X, C, Z): a view when the strides match, else one copy
        lib = _lib.load()
        nbytes = lib.sv_frustum_to_voxel_grad_scratch_bytes(B, H, W, X, Y, Z)
        if nbytes == 0:
            raise _lib.SeevcnHipError("sv_frustum_to_voxel_grad: pixel index or tap key exceeds int32")
        scratch = _lib.workspace.scratch("frustum_to_voxel_grad", nbytes, g.device)
        gf = torch.empty_like(f)
        gp = torch.empty_like(p)
        _lib.launch("sv_frustum_to_voxel_grad", _lib.ptr(f), _lib.ptr(p), _lib.ptr(l2c), _lib.ptr(c2i), _lib.ptr(ishape), _lib.ptr(g), B, C, nbins, H, W, X, Y,
                    Z, rng, mode, dmin, dmax, _lib.ptr(scratch), _lib.ptr(gf), _lib.ptr(gp))
        return gf.permute(0, 3, 1, 2), gp.permute(0, 3, 1, 2), None, None, None, None


def frustum_to_voxel(image_features, depth_probs, lidar_to_cam, cam_to_img, image_shape, grid_size, pc_range, disc_cfg):
    """image_features (B, C, H, W), depth_probs (B, num_bins + 1, H, W) -> voxel features (B, C, Z, Y, X) whose storage is ordered (B, Y, X, C, Z):
    grid_sample(depth_probs[:, :-1] * image_features, frustum_grid, bilinear, zeros, align_corners=True) of the reference, without the volume and
    the grid.  Differentiable in image_features and depth_probs."""
    _lib.require_cuda(image_features, depth_probs)
    l2c, c2i, ishape = _calib(lidar_to_cam, cam_to_img, image_shape)
    return _FrustumToVoxel.apply(image_features, depth_probs, l2c, c2i, ishape, _geometry(grid_size, pc_range, disc_cfg))
