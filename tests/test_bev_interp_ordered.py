"""The BEV keypoint interpolation under the order-fixed gradient switch: an NCHW map's gradient is summed by the channel-last entry in the stated
order (tests/bev_reference.py, key order = keypoint, tap) and handed back contiguous in NCHW; with the switch off the NCHW entry (float atomics)
runs as before."""
import numpy as np
import pytest
import torch

import bev_reference as R

B = 2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixed", "cluster"])
def test_hip_nchw_gradient_under_the_ordered_switch(cuda, hip_lib, kind):
    import seevcn_amd
    from seevcn_amd.pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    H, W, C = 16, 12, 64
    g = R.DYADIC
    kps_np = R.make_keypoints(kind, B, H, W, g, seed=0)
    grad_np = np.random.RandomState(100).standard_normal((kps_np.shape[0], C)).astype(np.float32)
    seq = R.grad_sequential_f32(kps_np, grad_np, g, B, C, H, W)                  # (B, H, W, C)
    exact, bound = R.grad_f64(kps_np, grad_np, g, B, C, H, W)
    kps, grad_out = torch.from_numpy(kps_np).to(cuda), torch.from_numpy(grad_np).to(cuda)
    values = torch.from_numpy(np.random.RandomState(5).standard_normal((B, C, H, W)).astype(np.float32)).to(cuda)

    def run():
        leaf = values.clone().requires_grad_(True)
        out = vsa_mod._BevInterp.apply(leaf, kps, g.x_min, g.y_min, g.voxel_x, g.voxel_y, g.stride)
        assert vsa_mod.VoxelSetAbstraction.last_bev_layout == "nchw"              # the forward entry is the NCHW one either way
        out.backward(grad_out)
        return out.detach(), leaf.grad

    plain_out, plain = run()
    with seevcn_amd.set_ordered_gradients(True):
        out1, first = run()
        _, second = run()
    assert torch.equal(out1, plain_out)
    assert first.shape == (B, C, H, W) and first.is_contiguous()
    R.assert_bit_equal(first.permute(0, 2, 3, 1).cpu().numpy(), seq, name="ordered gradient of an NCHW map vs sequential fp32")
    assert torch.equal(first, second)
    R.assert_within_bound(first.permute(0, 2, 3, 1).cpu().numpy(), exact, bound, name="ordered gradient vs float64")
    R.assert_within_bound(plain.permute(0, 2, 3, 1).cpu().numpy(), exact, bound, name="switch off: the NCHW entry (float atomics)")
