"""KITTI dataset support: the AP evaluation (kitti_object_eval_python)."""
