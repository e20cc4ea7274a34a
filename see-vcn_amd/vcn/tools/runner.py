"""Validation and test loops of the VCN with the reference's names (see/surface_completion/models/vcn/tools/runner.py:198-319, :343-549).

Every batch's 30 metric values stay on the device (Metrics.get_device: two library calls, no read); the (batches, 30) table is read ONCE at the end
and folded on the host exactly as the reference folds its per-batch lists: per taxonomy through an AverageMeter (-1 skipped), then over the
taxonomies.

Not built, because they are file or display I/O and no part of the numbers: the TensorBoard images and scalars (val_writer / test_writer), the
.pcd / .pkl / .npy writing of test_vc, the model names of ./data/shapenet_synset_dict.json (the result table prints taxonomy ids), the losses
meter (the reference leaves it commented out) and the multi-input batches (`input_i`, `complete_i`, `gt_boxes_i`: data[0] given as a list), which
raise NotImplementedError.
"""
import numpy as np
import torch

from ..utils import metrics as M
from ..utils.AverageMeter import AverageMeter
from ..utils.metrics import Metrics
from ..utils.transform import cn_to_vc


def print_log(msg, logger=None):
    if logger is None:
        print(msg)
    else:
        logger.info(msg)


def _taxonomy_id(taxonomy_ids):
    return taxonomy_ids[0] if isinstance(taxonomy_ids[0], str) else taxonomy_ids[0].item()


def _batch_metrics_device(base_model, data, widen):
    """One batch through the model and the two metric launches: the (30,) device vector."""
    if isinstance(data[0], list):
        raise NotImplementedError("multi-input batches (input_i / complete_i / gt_boxes_i) are not built")
    label = data[2]
    in_dict = {'input': data[0].cuda(), 'gt_boxes': label['gt_boxes'].cuda(), 'num_pts': label['num_pts'], 'complete': data[1].cuda(),
               'training': False}
    ret_dict = base_model(in_dict)
    if 'coarse' not in ret_dict.keys():
        ret_dict['coarse'] = cn_to_vc(ret_dict['coarse_cn'], in_dict['gt_boxes'])
    if widen and 'dataset' in label.keys() and label['dataset'][0] in ['waymo', 'nuscenes']:
        from ..utils.bbox_utils import get_bbox_from_keypoints
        box = get_bbox_from_keypoints(ret_dict['coarse'], in_dict['gt_boxes'])
        box[:, 4] += 0.25
        ret_dict['pred_box_widened'] = box
    return Metrics.get_device(ret_dict, in_dict)


def _run(base_model, batches, widen):
    """-> (taxonomy id per batch, (batches, 30) list of lists of Python floats) with one host read."""
    base_model.eval()
    taxonomies, vectors = [], []
    with torch.no_grad():
        for taxonomy_ids, model_ids, data in batches:
            taxonomies.append(_taxonomy_id(taxonomy_ids))
            vectors.append(_batch_metrics_device(base_model, data, widen))
    if not vectors:
        return taxonomies, []
    table = M.read(torch.stack(vectors))
    return taxonomies, [[float(v) for v in row] for row in table]


def _print_results(test_metrics, category_metrics, rows, overall, logger):
    print_log('============================ TEST RESULTS ============================', logger=logger)
    print_log('Taxonomy\t#Sample\t' + ''.join(metric + '\t' for metric in test_metrics.items), logger=logger)
    for taxonomy_id in category_metrics:
        msg = str(taxonomy_id) + '\t' + str(category_metrics[taxonomy_id].count(0)) + '\t'
        print_log(msg + ''.join('%.3f \t' % value for value in rows[taxonomy_id]), logger=logger)
    print_log('Overall\t\t' + ''.join('%.3f\t' % value for value in overall), logger=logger)


def validate_vc(base_model, val_batches, epoch=0, config=None, logger=None):
    """The reference's validate_vc on batches `(taxonomy_ids, model_ids, (input, complete, label))`, label = {'gt_boxes' (B,7), 'num_pts' (B)}:
    eval() under no_grad, `coarse_cn` converted through cn_to_vc when `coarse` is absent, metrics averaged per taxonomy and then over the
    taxonomies (runner.py:248-275).  Returns Metrics(config.consider_metric, averages); consider_metric defaults to 'CDL1'."""
    print_log(f"[VALIDATION] Start validating epoch {epoch}", logger=logger)
    test_metrics = AverageMeter(Metrics.names())
    category_metrics = dict()
    taxonomies, table = _run(base_model, val_batches, widen=False)
    for taxonomy_id, _metrics in zip(taxonomies, table):
        if taxonomy_id not in category_metrics:
            category_metrics[taxonomy_id] = AverageMeter(Metrics.names())
        category_metrics[taxonomy_id].update(_metrics)
    for k, v in category_metrics.items():
        test_metrics.update(v.avg())
    print_log('[Validation] EPOCH: %d  Metrics = %s' % (epoch, ['%.4f' % m for m in test_metrics.avg()]), logger=logger)
    _print_results(test_metrics, category_metrics, {k: v.avg() for k, v in category_metrics.items()}, test_metrics.avg(), logger)
    return Metrics(getattr(config, 'consider_metric', None) or 'CDL1', test_metrics.avg())


def test_vc(base_model, test_batches, config=None, logger=None):
    """The reference's test_vc without its file I/O: as validate_vc, plus +0.25 on pred_box[:, 4] for labels whose 'dataset' is 'waymo' or
    'nuscenes', every batch also counted in the overall meter (the reference updates it per batch AND with the taxonomy averages), and the
    rotation names replaced by the median of the positive per-batch values -- in the per-taxonomy rows too, where the reference takes the median
    over ALL batches (runner.py:497-505).  Returns Metrics(config.consider_metric, final values) (the reference returns nothing)."""
    test_metrics = AverageMeter(Metrics.names())
    category_metrics = dict()
    MedianMeter = {name: [] for name in Metrics.names() if 'Rotation' in name}
    taxonomies, table = _run(base_model, test_batches, widen=True)
    for taxonomy_id, _metrics in zip(taxonomies, table):
        test_metrics.update(_metrics)
        if taxonomy_id not in category_metrics:
            category_metrics[taxonomy_id] = AverageMeter(Metrics.names())
        category_metrics[taxonomy_id].update(_metrics)
        for idx, name in enumerate(Metrics.names()):
            if 'Rotation' in name:
                MedianMeter[name].append(_metrics[idx])
    for k, v in category_metrics.items():
        test_metrics.update(v.avg())
    print_log('[TEST] Metrics = %s' % (['%.4f' % m for m in test_metrics.avg()]), logger=logger)

    def with_medians(values):
        for idx, name in enumerate(Metrics.names()):
            if 'Rotation' in name:
                vals = np.array(MedianMeter[name])
                vals = vals[vals > 0.0]
                values[idx] = float(np.median(vals)) if len(vals) else float('nan')
        return values

    final_metrics = with_medians(test_metrics.avg())
    final_category_metrics = {taxonomy_id: with_medians(category_metrics[taxonomy_id].avg()) for taxonomy_id in category_metrics}
    _print_results(test_metrics, category_metrics, final_category_metrics, final_metrics, logger)
    return Metrics(getattr(config, 'consider_metric', None) or 'CDL1', final_metrics)
