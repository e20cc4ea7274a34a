"""Ray casting for the VC training set (reference: see/surface_completion/models/vcn/vc_shapenet/): a RaycastingScene on csrc/raycast.hip and the
ray-casting parts of dataset_functions.py and raycast_surface_from_meshes.py."""
from .raycasting import RaycastingScene  # noqa: F401
