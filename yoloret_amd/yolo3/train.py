"""Reference code/yolo3/train.py on the device.

Validation, forward only: ``_val_step`` (:48-52, the model's logits -> ``_compute_total_loss`` :11-16, the sum of the per-scale
YoloLoss values) inside ``_distributed_epoch(dataset, False)`` (:55-75, the mean over the batches) is ``validation_loss``.

Training of the output convolutions: ``OutputLayerTrainer`` is ``_train_step`` (:18-46) and ``fit`` (:81-128) for the stage reference
code/train.py:150-171 calls "Train with frozen layers first, to get a stable loss" - ``Adam(lr[0], epsilon=1e-8)`` under
``cos_lr_freeze`` - with everything frozen but the three ``*_y`` 1x1 convolutions that produce the logits.  The reference's
``ModelFactory.build`` (code/yolo3/utils.py:392) still carries the lines for that freeze ("freeze all but 2 output layers"), commented
out, so its stage 1 as shipped trains every layer: the frozen-body stage is BUILD-DEFINED, like the oracle.  The body runs as a
feature model in inference mode (what a frozen Keras layer does), the trained layer's forward, its weight gradient and the Adam
update are the kernels of csrc/headtrain.hip, the loss and its gradient at the logits those of csrc/loss.hip.  ``yolo3.data.AugmentedDataset``
yields the augmented ``images`` and ``y_true`` on the device.

Training of every layer: ``DetectorTrainer`` is the same ``_train_step`` and ``fit`` for the reference's stage 2 (code/train.py:150-216, all
layers trainable) on a MobileNetV2 backbone: ``autograd.detector`` differentiates the whole network on the device.

Not built in ``OutputLayerTrainer``: the gradient with respect to the layer's input and anything behind it (no parameter of the body has
a gradient) and BatchNorm in training mode - ``DetectorTrainer`` has both.  Not built in either: ``use_ema``, ``use_adv`` and the gradient
reduction over several devices."""
import math

import numpy as np
import torch

from .. import autograd
from .. import runtime as rt
from .model import output_convs, yolo_loss, yolo_loss_and_grad, yolo_loss_and_grad_from_boxes, yolov3_features


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


def cosine_decay(learning_rate, epoch, epochs):
    """``tf.keras.experimental.CosineDecay(learning_rate, epochs)(epoch)`` (code/train.py:95-97, alpha = 0)."""
    return learning_rate * 0.5 * (1.0 + math.cos(math.pi * min(epoch, epochs) / epochs))


class _Trainer:
    """What the two trainers share: the hyper-parameters, the state's device, the two forms of a step, the Adam update of the flat
    buffers ``w``, ``m``, ``v``, ``g`` and ``fit``.  A trainer adds ``_create(device)`` (the state), ``_step(images, loss_and_grad)``
    (forward, ``loss_and_grad(logits)`` -> (total, terms, d logits), backward, ``_adam()``) and ``commit()``."""

    def __init__(self, model, anchors, num_classes, num_scales, learning_rate, beta_1, beta_2, epsilon, ignore_thresh):
        self.model = model
        self.anchors = np.asarray(anchors, np.float32).reshape(-1, 2)
        self.num_classes, self.num_scales = int(num_classes), int(num_scales)
        self.learning_rate = self.lr = float(learning_rate)
        self.beta_1, self.beta_2, self.epsilon, self.ignore_thresh = float(beta_1), float(beta_2), float(epsilon), ignore_thresh
        self.step = 0           # Adam's t: optimizer.iterations
        self.device = None

    def _ensure(self, device):
        if self.device is None:
            self._create(device)
            self.device = device
        elif device != self.device:
            raise ValueError('%s: the state lives on %s, this batch on %s' % (type(self).__name__, self.device, device))

    def _adam(self):
        self.step += 1
        rt.adam_step(self.w, self.m, self.v, self.g, rt.adam_alpha(self.lr, self.step, self.beta_1, self.beta_2), self.beta_1, self.beta_2, self.epsilon)

    def train_step(self, images, y_true):
        """``_train_step`` (:18-46): the forward -> the loss and its gradient at the logits -> the gradients of everything the trainer
        trains -> one Adam update -> the total loss BEFORE the update, a 0-d float32 device tensor.  Launches only: no host
        synchronisation.  ``y_true``: the label tensors of the scales (``preprocess_true_boxes``' rows) on the images' device."""
        y_true = [y_true] if isinstance(y_true, torch.Tensor) else list(y_true)
        return self._step(images, lambda ys: yolo_loss_and_grad(ys, y_true, self.anchors, self.num_scales, self.ignore_thresh))

    def train_step_from_boxes(self, images, true_boxes):
        """``train_step`` with the labels encoded on the device from ground-truth boxes [B,T,5] (``yolo_loss_and_grad_from_boxes``)."""
        return self._step(images, lambda ys: yolo_loss_and_grad_from_boxes(ys, true_boxes, self.anchors, self.num_classes, self.num_scales,
                                                                           self.ignore_thresh))

    def fit(self, epochs, train_dataset, val_dataset=None, use_ema=False, use_adv=False):
        """``fit`` (:81-128) under ``cos_lr_freeze`` (code/train.py:95-97): epoch e runs at learning_rate * 0.5 * (1 + cos(pi e / epochs));
        the train loss of an epoch is the float32 sum of its batches' losses in order divided by their number (:68-74), formed on the
        device and read once per epoch; ``val_loss`` is ``validation_loss`` of the committed model.  Datasets: iterables of
        (images, y_true) on one device -> (train_losses, val_losses), lists of np.float32 (val_losses empty without a val_dataset)."""
        if use_ema or use_adv:
            raise NotImplementedError('%s.fit: use_ema and use_adv are not built' % type(self).__name__)
        train_losses, val_losses = [], []
        for epoch in range(epochs):
            self.lr = cosine_decay(self.learning_rate, epoch, epochs)
            total, n = None, 0
            for images, y_true in train_dataset:
                loss = self.train_step(images, y_true)
                total = loss if total is None else total + loss
                n += 1
            if n == 0:
                raise ValueError('%s.fit: the training data set is empty' % type(self).__name__)
            mean = total / torch.full((), float(n), dtype=total.dtype, device=total.device)
            train_losses.append(np.float32(mean.item()))
            if val_dataset is not None:
                self.commit()
                val_losses.append(np.float32(validation_loss(self.model, val_dataset, self.anchors, self.num_scales, self.ignore_thresh)[0]))
        self.commit()
        return train_losses, val_losses


class OutputLayerTrainer(_Trainer):
    """Trains the convolutions that produce ``model``'s logits with Keras Adam, the body frozen.

    ``model``: ``yolov3_body``'s float32 ``Model`` with its weights set.  The feature model (``yolov3_features``) is built once and
    given the same body weights.  The ``num_scales`` matrices Wt[cout][round_up(cin, 4)] live in ONE contiguous device tensor
    (``weights`` are views into it), and so do the moments ``m``, ``v`` and the gradient ``grads``: one ``adam_step`` launch covers
    all scales.  They start from the model's ``*_y/kernel`` (Keras layout [1,1,cin,cout]) and are created on the device of the
    first batch.  ``commit()`` writes them back into ``model``."""

    def __init__(self, model, anchors, num_classes, num_scales, learning_rate=1e-3, beta_1=.9, beta_2=.999, epsilon=1e-8, ignore_thresh=.5):
        super().__init__(model, anchors, num_classes, num_scales, learning_rate, beta_1, beta_2, epsilon, ignore_thresh)
        self.features = yolov3_features(model)          # (raises for a 16-bit plan or outputs that are not bias-free 1x1 convs)
        weights = model.get_weights()
        if weights is None:
            raise ValueError('OutputLayerTrainer: the model has no weights (set_weights / load_weights)')
        self.features.set_weights(weights)
        convs = output_convs(model)[:self.num_scales]
        if len(convs) < self.num_scales:
            raise ValueError('OutputLayerTrainer: %d outputs for %d scales' % (len(convs), self.num_scales))
        self.kernel_names = [c.name + '/kernel' for c in convs]
        self.num_anchors = [o.node.attrs['num_anchors'] for o in model.outputs[:self.num_scales]]
        self.dims = []          # (cin, cout, kp) per scale
        for c, a in zip(convs, self.num_anchors):
            cin, cout = c.inputs[0].shape[2], c.output.shape[2]
            if cout != a * (5 + self.num_classes):
                raise ValueError('OutputLayerTrainer: %s has %d filters, %d anchors x (5 + %d classes) expected' % (c.name, cout, a, self.num_classes))
            if not (1 <= cin <= 256 and 1 <= cout <= 256):
                raise ValueError('OutputLayerTrainer: %s is %d -> %d channels; 1..256 are built' % (c.name, cin, cout))
            self.dims.append((cin, cout, (cin + 3) // 4 * 4))
        self._workspace = None

    # ------------------------------------------------------------------ state
    def _views(self, flat):
        out, at = [], 0
        for cin, cout, kp in self.dims:
            out.append(flat[at:at + cout * kp].view(cout, kp))
            at += cout * kp
        return out

    def _create(self, device):
        host = self.model.get_weights()
        flat = np.concatenate([autograd._pack_wt(host[name]).reshape(-1) for name in self.kernel_names])
        self.w = torch.from_numpy(flat).to(device)
        self.m, self.v, self.g = torch.zeros_like(self.w), torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.weights, self.grads = self._views(self.w), self._views(self.g)

    # ------------------------------------------------------------------ one step
    def logits(self, images, features=None):
        """The trained layer's forward on the frozen body's features -> [B,G,G,A,5+C] per scale (fresh tensors)."""
        self._ensure(images.device)
        feats = self.features(images) if features is None else features
        ys = []
        for f, wt, a in zip(feats, self.weights, self.num_anchors):
            y = rt.linear_forward(f, wt)
            ys.append(y.view(tuple(y.shape[:3]) + (a, y.shape[3] // a)))
        return ys

    def _step(self, images, loss_and_grad):
        """features -> logits -> loss and its gradient at the logits -> the weight gradients -> one Adam update"""
        feats = self.features(images)
        total, self.last_terms, dys = loss_and_grad(self.logits(images, feats))
        for f, dy, g, (cin, cout, kp) in zip(feats, dys, self.grads, self.dims):
            need = rt.linear_wgrad_workspace_bytes(f.numel() // cin, cin, cout)
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)        # (calls on one stream are ordered: one workspace serves all scales)
            rt.linear_wgrad(f, dy.reshape(tuple(f.shape[:3]) + (cout,)), out=g, workspace=self._workspace)
        self._adam()
        return total

    # ------------------------------------------------------------------ the loop
    def commit(self):
        """Writes the trained kernels back into ``model`` (``set_weights``), so ``model(images)``, ``YoloModel``, ``MAPCallback`` and
        ``save_weights`` see the trained layer.  One copy to the host (synchronises)."""
        if self.device is None:
            return
        host = self.w.cpu().numpy()
        weights = self.model.get_weights()
        at = 0
        for name, (cin, cout, kp) in zip(self.kernel_names, self.dims):
            weights[name] = autograd._unpack_wt(host[at:at + cout * kp].reshape(cout, kp), cin)
            at += cout * kp
        self.model.set_weights(weights)


class DetectorTrainer(_Trainer):
    """Trains EVERY layer of ``model`` with Keras Adam: the reference's ``_train_step`` (:18-46) as its stage 2 runs it (code/train.py:150-216
    sets ``trainable = True`` on all layers, and stage 1 as shipped freezes none): ``autograd.detector(training=True)`` - the MobileNetV2
    backbone, the RFCR module, the links and the six head blocks, every BatchNorm on the statistics of the batch - -> the sum of
    ``YoloLoss`` over the scales -> the gradients of every kernel, bias, alpha, gamma and beta -> one Adam update.

    ``model``: ``yolov3_body``'s float32 ``Model`` of a MobileNetV2 backbone with its weights set.  All trained tensors are views of ONE
    flat device buffer ``w`` (``params`` holds the views in ``autograd.detector_parameters``' layout), and so are their gradients in ``g``
    and the moments ``m``, ``v``: backward accumulates into the views of ``g`` and one ``adam_step`` launch updates everything; a step
    synchronises with the host nowhere.  The moving statistics live beside them and are updated in place by the forward.  The state is
    created on the device of the first batch.  ``commit()`` writes everything back into ``model``.

    Not built: the EfficientNet backbones (their training forward draws a drop-connect mask), 16-bit plans, ``use_ema``, ``use_adv`` and
    the gradient reduction over several devices."""

    def __init__(self, model, anchors, num_classes, num_scales, learning_rate=1e-3, beta_1=.9, beta_2=.999, epsilon=1e-8, ignore_thresh=.5):
        super().__init__(model, anchors, num_classes, num_scales, learning_rate, beta_1, beta_2, epsilon, ignore_thresh)
        yolov3_features(model)          # (raises for a 16-bit plan or outputs that are not bias-free 1x1 convs)
        weights = model.get_weights()
        if weights is None:
            raise ValueError('DetectorTrainer: the model has no weights (set_weights / load_weights)')
        if 'Conv1/kernel' not in weights:
            raise ValueError('DetectorTrainer: the model has no Conv1/kernel: only the MobileNetV2 backbones are built (an EfficientNet backbone '
                             'draws a drop-connect mask in its training forward, which is missing)')
        if self.num_scales != 3 or len(model.outputs) < 3:
            raise ValueError('DetectorTrainer: %d scales; yolov3_body\'s three are built' % self.num_scales)
        self.num_anchors = [o.node.attrs['num_anchors'] for o in model.outputs[:3]]
        if len(set(self.num_anchors)) != 1:
            raise ValueError('DetectorTrainer: the scales have %s anchors; one number for all is built' % (self.num_anchors,))
        for c, a in zip(output_convs(model)[:3], self.num_anchors):
            if c.output.shape[2] != a * (5 + self.num_classes):
                raise ValueError('DetectorTrainer: %s has %d filters, %d anchors x (5 + %d classes) expected' % (c.name, c.output.shape[2], a, self.num_classes))

    # ------------------------------------------------------------------ state
    @staticmethod
    def _slots(params):
        """[(dictionary, key)] of every tensor of ``detector_parameters``' nest, in a fixed order"""
        out = []
        for d in [params['backbone'], params['neck']['rfcr']] + [v for k, v in params['neck'].items() if k not in ('rfcr', 'cin')]:
            out.extend((d, k) for k, v in d.items() if isinstance(v, torch.Tensor))
        return out

    def _create(self, device):
        self.params = autograd.detector_parameters(self.model, device)
        trained = [(d, k) for d, k in self._slots(self.params) if d[k].requires_grad]
        sizes = [(d[k].numel() + 3) // 4 * 4 for d, k in trained]          # every tensor starts on 16 bytes; the fill is 0 and stays 0 (its gradient is)
        self.w = torch.zeros((sum(sizes),), dtype=torch.float32, device=device)
        self.m, self.v, self.g = torch.zeros_like(self.w), torch.zeros_like(self.w), torch.zeros_like(self.w)
        at = 0
        for (d, k), size in zip(trained, sizes):          # every trained tensor becomes a view of w whose gradient is the same view of g
            n, shape = d[k].numel(), tuple(d[k].shape)
            self.w[at:at + n].copy_(d[k].detach().reshape(-1))
            view = self.w[at:at + n].view(shape).requires_grad_(True)
            view.grad = self.g[at:at + n].view(shape)
            d[k] = view
            at += size
        self.trained = trained

    # ------------------------------------------------------------------ one step
    def logits(self, images, training=False):
        """``autograd.detector`` on the trainer's own parameters -> [B,G,G,A,5+C] per scale.  training=False folds the BatchNorms (it copies
        their vectors to the host: it synchronises) and changes nothing."""
        self._ensure(images.device)
        if training:
            return autograd.detector(images, self.params, True, self.num_anchors[0])
        with torch.no_grad():
            return autograd.detector(images, self.params, False, self.num_anchors[0])

    def _step(self, images, loss_and_grad):
        """the training-mode forward -> the loss and its gradient at the logits -> backward through the neck and the backbone -> one Adam update"""
        ys = self.logits(images, training=True)
        total, self.last_terms, dys = loss_and_grad([y.detach() for y in ys])
        self.g.zero_()          # (backward ADDS into the views of g)
        torch.autograd.backward(ys, [dy.reshape(y.shape) for y, dy in zip(ys, dys)])
        self._adam()
        return total

    # ------------------------------------------------------------------ the loop
    def commit(self):
        """Writes every trained tensor and every moving statistic back into ``model`` (``set_weights`` of ``autograd.detector_weights``), so
        ``model(images)``, ``YoloModel``, ``MAPCallback`` and ``save_weights`` see the trained network.  One copy per half to the host (synchronises)."""
        if self.device is None:
            return
        weights = self.model.get_weights()
        weights.update(autograd.detector_weights(self.params))
        self.model.set_weights(weights)
