"""The model surface of the reference's raycast_surface_from_meshes.py:16-52 on the device: twelve pinhole views of a mesh, thinned with FPS to the
surface the VCN regresses to."""
import numpy as np

from ..utils import misc
from . import raycasting as rc
from .dataset_functions import _cast_cameras

# the eyes of get_object_surface (:36-47), in its order
EYES = [[1, 1, 1], [-1, 1, 1], [1, 1, -1], [-1, 1, -1], [1, -1, 1], [-1, -1, 1], [1, -1, -1], [-1, -1, -1], [0, 0, -1], [0, 0, 1], [-1, 0, 0], [1, 0, 0]]


def _views(scene, eyes, width_px, height_px):
    cams = [rc.pinhole_camera(45, [0, 0, 0], eye, [0, 1, 0], width_px, height_px) for eye in eyes]
    points, _, n_hit, _ = _cast_cameras(scene, cams, None, width_px, height_px)
    return points[:int(n_hit.sum())]


def generate_views(scene, eye, width_px=640, height_px=480):
    """The hit points of one view at fov 45 looking at the origin with up = +y (:16-32), (n, 3) float32 on the device."""
    return _views(scene, [eye], width_px, height_px)


def get_object_surface(scene, complete_pts=16384, width_px=640, height_px=480, return_views=False):
    """The twelve views as one 12-camera launch, concatenated in the reference's order, thinned with misc.fps (:34-52): (complete_pts, 3)."""
    pts = _views(scene, EYES, width_px, height_px)
    surface = misc.fps(pts.unsqueeze(0), complete_pts).squeeze(0)
    return (surface, pts) if return_views else surface
