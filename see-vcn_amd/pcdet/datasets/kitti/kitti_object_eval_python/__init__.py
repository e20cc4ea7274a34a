"""KITTI AP evaluation on the GPU: `eval` (matching, thresholds, AP, result string) and `rotate_iou` (overlap kernel binding)."""
