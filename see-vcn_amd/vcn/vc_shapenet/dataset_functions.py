"""The ray-casting part of the reference's VC dataset builder (see/surface_completion/models/vcn/vc_shapenet/dataset_functions.py:230-342) on the
device.  The reference's names are kept.  Arrays in, arrays out: a car is a dict with 'vertices' (V, 3) and 'triangles' (F, 3) arrays in place of
the reference's open3d 'mesh', plus its 'label' [x, y, z, l, w, h, yaw] and 'bbox' (8, 3) corner points.  Every function that draws takes an explicit
numpy.random.RandomState and draws in the reference's order.
"""
import numpy as np
import torch

from ... import _lib as L
from . import raycasting as rc
from .raycasting import RaycastingScene


def create_cylinder(radius=1.0, height=2.0, resolution=20, split=4):
    """open3d.geometry.TriangleMesh.create_cylinder as recalled (not checked against open3d): the axis is z, centred at the origin; vertices 0 / 1
    are the top / bottom centres, then split + 1 rings of `resolution` vertices from the top down; two cap fans, then two triangles per band
    cell.  (vertices (resolution * (split + 1) + 2, 3) float64, triangles (resolution * (2 + 2 * split), 3) int64): 102 and 200 by default."""
    v = np.zeros((resolution * (split + 1) + 2, 3), np.float64)
    v[0] = (0, 0, height * 0.5)
    v[1] = (0, 0, -height * 0.5)
    step, h_step = 2 * np.pi / resolution, height / split
    for i in range(split + 1):
        for j in range(resolution):
            theta = step * j
            v[2 + resolution * i + j] = (np.cos(theta) * radius, np.sin(theta) * radius, height * 0.5 - h_step * i)
    f = []
    for j in range(resolution):
        j1 = (j + 1) % resolution
        f.append((0, 2 + j, 2 + j1))
        base = 2 + resolution * split
        f.append((1, base + j1, base + j))
    for i in range(split):
        base1 = 2 + resolution * i
        base2 = base1 + resolution
        for j in range(resolution):
            j1 = (j + 1) % resolution
            f.append((base2 + j, base1 + j1, base1 + j))
            f.append((base2 + j, base2 + j1, base1 + j1))
    return v, np.array(f, np.int64)


def opd_to_boxpts(box):
    """[x, y, z, l, w, h, r] -> the (8, 3) corners (:230-263)."""
    l, w, h = box[3], box[4], box[5]
    rotation = box[6]
    bounding_box = np.array([[l / 2, w / 2, h / 2], [l / 2, -w / 2, h / 2], [-l / 2, w / 2, h / 2], [-l / 2, -w / 2, h / 2],
                             [l / 2, w / 2, -h / 2], [l / 2, -w / 2, -h / 2], [-l / 2, w / 2, -h / 2], [-l / 2, -w / 2, -h / 2]])
    rotation_matrix = np.array([[np.cos(rotation), np.sin(rotation), 0.0], [-np.sin(rotation), np.cos(rotation), 0.0], [0.0, 0.0, 1.0]])
    vcbox = bounding_box @ rotation_matrix
    vcbox += np.asarray(box[:3], np.float64)
    return vcbox


def get_gt_for_zero_yaw(pts):
    """The axis-aligned box of a point set: {'bbox': (8, 3) corners, 'center', 'dims'} (reference utils/misc.py:300-324 without the open3d form)."""
    pts = np.asarray(pts)
    lo, hi = pts.min(0), pts.max(0)
    center = (hi + lo) / 2
    bbox3d = np.array([[hi[0], hi[1], hi[2]], [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]], [lo[0], lo[1], hi[2]],
                       [hi[0], hi[1], lo[2]], [hi[0], lo[1], lo[2]], [lo[0], hi[1], lo[2]], [lo[0], lo[1], lo[2]]])
    return {"bbox": bbox3d, "center": center, "dims": hi - lo}


def draw_scene_obstacles(scene_cars, signs, rng, random_poles_pct=0.3):
    """The draws of populate_scene (:268-306) in the reference's order, on the host: a list of (radius, height, centre (3,)) cylinders, the poles
    beside the first int(len(scene_cars) * random_poles_pct) cars and then the labelled signs.  (The reference overwrites the sign label's z in
    place through a view; here the label is left alone.)"""
    out = []
    num_rand_poles = int(len(scene_cars) * random_poles_pct)
    for i, sc in enumerate(scene_cars):
        if i >= num_rand_poles:
            continue
        car_centre = sc["label"][:3]
        car_height = sc["label"][5]
        pole_radius = rng.uniform(0.03, 0.2)
        pole_height = rng.uniform(1, 4, 1)
        box_min = np.min(sc["bbox"], axis=0)[:2]
        box_max = np.max(sc["bbox"], axis=0)[:2]
        xyall_choice = rng.choice([1, 2, 3])
        if rng.choice([True, False]):
            if xyall_choice == 1:
                pole_xy = np.array([box_max[0], car_centre[1]]) + rng.uniform(0, 0.5)
            elif xyall_choice == 2:
                pole_xy = np.array([car_centre[0], box_max[1]]) + rng.uniform(0, 0.5)
            else:
                pole_xy = box_max + rng.uniform(0, 1, 2)
        else:
            pole_xy = box_min - rng.uniform(0, 1, 2)
        pole_centre = np.concatenate([pole_xy, np.array(car_centre[2] + pole_height / 2 - car_height / 2)])
        out.append((float(pole_radius), float(pole_height.item()), pole_centre))
    if "label" in signs:
        for sign in signs["label"]:
            pole_height = rng.uniform(1, 4, 1)
            pole_centre = np.array(sign[:3], np.float64)
            pole_centre[2] = -2.4 + pole_height.item() / 2
            pole_radius = rng.uniform(0.03, 0.1)
            out.append((float(pole_radius), float(pole_height.item()), pole_centre))
    return out


def _to_device(a, dtype, device):
    return a.to(device=device, dtype=dtype) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(device=device, dtype=dtype)


def populate_scene(scene_cars, signs, rng, random_poles_pct=0.3, device=None):
    """A RaycastingScene of the cars' meshes, a pole cylinder after each of the first cars and a cylinder per labelled sign, in the reference's
    geometry order (:265-308)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    obstacles = draw_scene_obstacles(scene_cars, signs, rng, random_poles_pct)
    num_rand_poles = int(len(scene_cars) * random_poles_pct)
    scene = RaycastingScene()
    for i, sc in enumerate(scene_cars):
        scene.add_triangles(_to_device(sc["vertices"], torch.float32, dev), _to_device(sc["triangles"], torch.int64, dev))
        if i < num_rand_poles:
            radius, height, centre = obstacles[i]
            v, f = create_cylinder(radius=radius, height=height)
            scene.add_triangles(_to_device(v + centre, torch.float32, dev), _to_device(f, torch.int64, dev))
    for radius, height, centre in obstacles[num_rand_poles:]:
        v, f = create_cylinder(radius=radius, height=height)
        scene.add_triangles(_to_device(v + centre, torch.float32, dev), _to_device(f, torch.int64, dev))
    return scene


def _cast_cameras(scene, cams_host, boxes_host, width_px, height_px):
    """All cameras in one launch, one compaction, one host read: (points, obj_points, hit counts, in-box counts)."""
    dev = scene.device
    C = len(cams_host)
    cams = rc.cameras_to_device(cams_host, dev)
    boxes = None if boxes_host is None else torch.from_numpy(np.ascontiguousarray(np.asarray(boxes_host, np.float32).reshape(C, 7))).to(dev)
    ans = scene.cast_pinhole(cams, width_px, height_px)
    points, _, obj_points, counts = rc.hit_points(ans["t_hit"], C, width_px, height_px, cams=cams, boxes=boxes)
    vals = rc.host_ints([counts, scene.status])
    if vals[2 * C + 1]:
        raise L.SeevcnHipError("cast: the traversal stack was full (a path deeper than the key width allows)")
    return points, obj_points, np.asarray(vals[:C], np.int64), np.asarray(vals[C:2 * C], np.int64)


def _split(points, counts):
    ends = np.cumsum(counts)
    return [points[int(e - c):int(e)] for c, e in zip(counts, ends)]


def cast_rays_at_point(scene, point, fov_deg=100, aspect_ratio=2, height_px=640):
    """The hit points of a pinhole image looking from the lidar origin at `point` (:310-323), (n, 3) float32 on the device, in ray order."""
    width_px = aspect_ratio * height_px
    cam = rc.pinhole_camera(fov_deg, point, [0, 0, 0], [0, 0, 1], width_px, height_px)
    points, _, n_hit, _ = _cast_cameras(scene, [cam], None, width_px, height_px)
    return points[:int(n_hit[0])]


def raycast_frame(scene_cars, scene, rng, aspect_ratio=2, height_px=640):
    """raycast_object (:326-342) for every car of a frame at once: each car's fov_deg ~ N(60, 30) is drawn on the host in car order, all cars are
    cast in one launch and compacted once, and one host read returns the counts.  A list of dicts, one per car: 'ray_pts' (n, 3) and 'obj_pts'
    (the points inside the car's label box) on the device, 'num_ray_pts', 'num_obj_pts', 'fov_deg', 'label', 'bbox_pts'."""
    if len(scene_cars) == 0:
        return []
    width_px = aspect_ratio * height_px
    fovs = [rng.normal(60, 30) for _ in scene_cars]
    cams = [rc.pinhole_camera(f, np.asarray(car["label"][:3], np.float64), [0, 0, 0], [0, 0, 1], width_px, height_px) for f, car in zip(fovs, scene_cars)]
    boxes = [np.asarray(car["label"][:7], np.float32) for car in scene_cars]
    points, obj_points, n_hit, n_in = _cast_cameras(scene, cams, boxes, width_px, height_px)
    return [{"ray_pts": p, "obj_pts": q, "num_ray_pts": int(a), "num_obj_pts": int(b), "fov_deg": f, "label": car["label"], "bbox_pts": car.get("bbox")}
            for p, q, a, b, f, car in zip(_split(points, n_hit), _split(obj_points, n_in), n_hit, n_in, fovs, scene_cars)]


def raycast_object(car, scene, rng, aspect_ratio=2, height_px=640):
    """One car (:326-342): the ray-cast part of the reference's dict."""
    return raycast_frame([car], scene, rng, aspect_ratio, height_px)[0]
