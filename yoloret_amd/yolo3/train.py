"""The validation epoch of reference code/yolo3/train.py, forward only: ``_val_step`` (:48-52, the model's logits ->
``_compute_total_loss`` :11-16, the sum of the per-scale YoloLoss values) inside ``_distributed_epoch(dataset, False)`` (:55-75,
the mean over the batches).  Training (``_train_step``, ``fit``) is not built; both tensors ``_train_step`` consumes are: ``yolo3.data.AugmentedDataset``
yields the augmented ``images`` and ``y_true`` on the device, and ``runtime.yolo_loss_grad`` (``yr_yolo_loss_grad``) is the loss's gradient at the logits."""
import torch

from .model import yolo_loss


def validation_loss(model, dataset, anchors, num_scales, ignore_thresh=.5):
    """``model``: images [b,H,W,3] -> the logits of ``num_scales`` scales (yolov3_body's network, a PlanHandle); ``dataset``: an
    iterable of (images, y_true) on the model's device (``yolo3.data.Dataset(...).build()[0]``) -> (val_loss as a Python float,
    terms [n_batches, num_scales, 5] NumPy float32: per batch and scale (loss, giou_loss, confidence_loss, class_loss, ignore_sum)).

    Per batch the loss is the sum over the scales (:13-14); the result is their float32 sum in batch order divided by the number
    of batches (:68-74).  Everything is accumulated on the device and copied once at the end.  The per-scale terms are tensors of
    their own: the model's outputs may be overwritten by its next forward."""
    total, rows = None, []
    for images, y_true in dataset:
        ys = model(images)
        y_true = [y_true] if isinstance(y_true, torch.Tensor) else list(y_true)
        loss, terms = yolo_loss(ys, y_true, anchors, num_scales, ignore_thresh)
        total = loss if total is None else total + loss
        rows.append(terms)
    if not rows:
        raise ValueError('validation_loss: the data set is empty')
    mean = total / torch.full((), float(len(rows)), dtype=total.dtype, device=total.device)      # (a true division, not a reciprocal multiply)
    host = torch.cat([mean.reshape(1)] + [t.reshape(-1) for t in rows]).cpu().numpy()      # the one copy (and synchronisation)
    return float(host[0]), host[1:].reshape(len(rows), num_scales, 5).copy()
