"""YOLO-ReT model definition and post-processing - host-side mirror of reference
code/yolo3/model.py for the detection forward path, on MI355X.

Same names, argument order, defaults and return structure as the reference;
``torch`` CUDA tensors replace ``tf.Tensor`` as the container and all arithmetic
runs in the HIP kernels of libyoloret_hip.so (no CPU fallback).

Graph builders (record a ``yoloret_amd.layers`` graph, lowered by ``yoloret_amd.compiler``):
  MobilenetSeparableConv2D :14-30, _make_divisible :32-39,
  make_last_layers_efficientnet_lite :91-115, WeightedSum :117-137, downsample_layer :139-144,
  rfcr_module :146-168, yolov3_body :170-342.
Post-processing (launch HIP kernels): yolo_head :344-371, yolo_correct_boxes :374-399,
  yolo_boxes_and_scores :402-428, yolo_eval :431-491, YoloEval :494-526.
Loss (validation loss from device logits, and its gradient with respect to those logits; no backward through the
network): YoloLoss :585-691 (GIOU branch), yolo_loss, yolo_loss_and_grad.

Batch semantics: the reference folds the batch axis into the box list before NMS
(:425-427) and pins inference to batch 1 (yolo.py:84).  Here a batch means "the
reference applied to each image independently" (SURVEY.md D3): ``yolo_eval`` on a batch
of B>1 returns per-image lists; on B==1 it returns exactly the reference's 3 tensors.
"""
import numpy as np
import torch

from .. import layers as L
from .. import runtime as rt
from ..engine import Model
from ..layers import WeightedSum  # model.py:117-137
from . import efficientnet as _effnet
from .enums import BOX_LOSS
from .efficientnet import BlockArgs, EfficientNetB0, EfficientNetB3, MBConvBlock, get_model_params
from .override import mobilenet_v2
from .utils import compose

AdvLossModel = Model  # yolo3/train.py:10 - on this path only a Model container (model.py:342)


def MobilenetSeparableConv2D(filters, kernel_size, strides=(1, 1), padding='valid', use_bias=True, name='sepconv'):
    """DW kxk + BN + ReLU6 -> 1x1 + BN + ReLU6 (model.py:14-30)."""
    return compose(
        L.DepthwiseConv2D(kernel_size, padding=padding, use_bias=use_bias, strides=strides, name=name + '_dw'),
        L.BatchNormalization(name=name + '_dw_BN'), L.ReLU(6., name=name + '_dw_relu'),
        L.Conv2D(filters, 1, padding='same', use_bias=use_bias, strides=1, name=name + '_pw'),
        L.BatchNormalization(name=name + '_pw_BN'), L.ReLU(6., name=name + '_pw_relu'))


def _make_divisible(v, divisor, min_value=None):
    """model.py:32-39."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def make_last_layers_efficientnet_lite(x, block_args, global_params, quantize=False, name='head'):
    """Head block (model.py:91-115): 1x1->F + BN + ReLU6 -> MBConv(k3,e1,se.25,F->O); y = 1x1 O->O."""
    if global_params.data_format not in (None, 'channels_last'):
        raise ValueError('only channels_last is supported')
    num_filters = block_args.input_filters * block_args.expand_ratio
    x = compose(
        L.Conv2D(num_filters, kernel_size=1, padding='same', use_bias=False, name=name + '_conv'),
        L.BatchNormalization(epsilon=global_params.batch_norm_epsilon, momentum=global_params.batch_norm_momentum,
                             name=name + '_conv_BN'),
        L.ReLU(6., name=name + '_conv_relu'),
        MBConvBlock(block_args, global_params, drop_connect_rate=global_params.drop_connect_rate,
                    quantize=quantize, name=name + '_mb'))(x)
    y = L.Conv2D(block_args.output_filters, kernel_size=1, padding='same', use_bias=False, name=name + '_y')(x)
    return x, y


def downsample_layer(x, stride=2):
    """MaxPooling2D((stride, stride)) (model.py:139-144)."""
    return L.MaxPooling2D((stride, stride))(x)


def rfcr_module(inp_arr):
    """RFCR multi-scale fusion (model.py:146-168)."""
    b1c = L.Conv2D(48, kernel_size=1, padding='same', use_bias=False, name='rfcr_b1c')(inp_arr[0])
    b2c = L.Conv2D(48, kernel_size=1, padding='same', use_bias=False, name='rfcr_b2c')(inp_arr[1])
    b3c = L.Conv2D(48, kernel_size=1, padding='same', use_bias=False, name='rfcr_b3c')(inp_arr[2])
    b4c = L.Conv2D(48, kernel_size=1, padding='same', use_bias=False, name='rfcr_b4c')(inp_arr[3])
    bc = WeightedSum(name='rfcr_wsum')([L.UpSampling2D()(b1c), b2c, downsample_layer(b3c), b4c])
    bc = MobilenetSeparableConv2D(96, kernel_size=(5, 5), use_bias=False, padding='same', name='rfcr_sep')(bc)
    b1 = L.Concatenate()([inp_arr[0], downsample_layer(bc)])
    b2 = L.Concatenate()([inp_arr[1], bc])
    b3 = L.Concatenate()([inp_arr[2], L.UpSampling2D()(bc)])
    return b1, b2, b3


def _conv_bn_relu6(filters, name, bn_name):
    return compose(L.Conv2D(filters, kernel_size=1, padding='same', use_bias=False, name=name),
                   L.BatchNormalization(momentum=0.9, name=bn_name), L.ReLU(6., name=name + '_relu6'))


# (the reference wires B3 only, model.py:205-217; its efficientnet.py:231-244 scales B0 .. B7 and the taps are stage ends, so every width builds)
_EFFNET_BUILDERS = {'efficientnetb%d' % i: getattr(_effnet, 'EfficientNetB%d' % i) for i in range(8)}


def yolov3_body(inputs, model_name, num_anchors, **kwargs):
    """Builds backbone + RFCR + FPN/PANet heads (model.py:170-342) and returns a ``Model``
    mapping images [B,H,W,3] to [y1,y2,y3] = raw logits [B,G,G,num_anchors,num_classes+5]
    for strides 32/16/8.  ``inputs``: ``yoloret_amd.layers.Input(shape=[H,W,3])``.
    ``model_name`` in {'mobilenetv2x75','mobilenetv2x14','efficientnetb3'} as in the reference,
    plus the build-defined 'efficientnetb0' .. 'efficientnetb7' (the other widths of efficientnet.py:231-244) and '<efficientnet>-lite'
    variants.
    kwargs: num_classes, drop_rate, data_format, batch_norm_momentum, batch_norm_epsilon,
    drop_connect_rate (efficientnet.py:259-265); unknown keys raise ValueError."""
    L.reset_names()
    _, global_params, _ = get_model_params('efficientnet-b0', kwargs)
    num_classes = global_params.num_classes
    if global_params.data_format not in (None, 'channels_last'):
        raise ValueError('only data_format="channels_last" is supported')
    if model_name == 'mobilenetv2x75' or model_name == 'mobilenetv2x14':
        alpha = 0.75 if model_name == 'mobilenetv2x75' else 1.4
        backbone = mobilenet_v2(default_batchnorm_momentum=0.9, alpha=alpha, input_tensor=inputs,
                                include_top=False, weights=None)
        b1 = backbone.get_layer('block_15_add').output
        b2 = backbone.get_layer('block_12_add').output
        b3 = backbone.get_layer('block_5_add').output
        b4 = backbone.get_layer('block_2_add').output
    else:
        base, lite = (model_name[:-5], True) if model_name.endswith('-lite') else (model_name, False)
        if base not in _EFFNET_BUILDERS:
            raise ValueError('unknown model_name %r' % (model_name,))
        backbone = _EFFNET_BUILDERS[base](include_top=False, weights=None, input_tensor=inputs, lite=lite)
        # add_17 / add_12 / add_4 / add_2 of B3 (model.py:213-216) == ends of stages 6/5/3/2
        b1 = backbone.get_layer('stage6').output
        b2 = backbone.get_layer('stage5').output
        b3 = backbone.get_layer('stage3').output
        b4 = backbone.get_layer('stage2').output
    b4 = downsample_layer(b4, stride=4)

    b1, b2, b3 = rfcr_module([b1, b2, b3, b4])

    out_filters = num_anchors * (num_classes + 5)
    block_args = BlockArgs(kernel_size=3, num_repeat=1, input_filters=512, output_filters=out_filters,
                           expand_ratio=1, id_skip=True, se_ratio=0.25, strides=[1, 1])
    # top-down pass (fpn=True); with panet=True its y convs are discarded (model.py:240-241,260-261,280-281)
    x, _ = make_last_layers_efficientnet_lite(b1, block_args, global_params, name='td1')
    c1 = x
    x = _conv_bn_relu6(256, 'block_20_conv', 'block_20_BN')(x)
    x = L.Concatenate()([L.UpSampling2D()(x), b2])
    block_args = block_args._replace(input_filters=256)
    x, _ = make_last_layers_efficientnet_lite(x, block_args, global_params, name='td2')
    c2 = x
    x = _conv_bn_relu6(128, 'block_24_conv', 'block_24_BN')(x)
    x = L.Concatenate()([L.UpSampling2D()(x), b3])
    block_args = block_args._replace(input_filters=128)
    x, _ = make_last_layers_efficientnet_lite(x, block_args, global_params, name='td3')
    c3 = x
    # bottom-up pass (panet=True, model.py:283-323)
    x, y3 = make_last_layers_efficientnet_lite(c3, block_args, global_params, name='bu3')
    x = _conv_bn_relu6(128, 'bu3_down_conv', 'bu3_down_BN')(x)
    x = L.Concatenate()([downsample_layer(x), c2])
    block_args = block_args._replace(input_filters=256)
    x, y2 = make_last_layers_efficientnet_lite(x, block_args, global_params, name='bu2')
    x = _conv_bn_relu6(256, 'bu2_down_conv', 'bu2_down_BN')(x)
    x = L.Concatenate()([downsample_layer(x), c1])
    block_args = block_args._replace(input_filters=512)
    x, y1 = make_last_layers_efficientnet_lite(x, block_args, global_params, name='bu1')

    y1 = L.Reshape5(num_anchors, name='y1')(y1)
    y2 = L.Reshape5(num_anchors, name='y2')(y2)
    y3 = L.Reshape5(num_anchors, name='y3')(y3)
    return AdvLossModel(backbone.inputs, [y1, y2, y3])


def output_convs(model):
    """The graph nodes of the convolutions that produce ``model``'s logits, one per output: each output must be
    ``Reshape5 <- 1x1 Conv2D`` with stride 1 and no bias (hence no BatchNorm and no activation between them) - the ``*_y`` convs
    of make_last_layers_efficientnet_lite (model.py:111-114).  Found by walking the graph, not by name.  ValueError otherwise."""
    convs = []
    for i, out in enumerate(model.outputs):
        node = out.node
        if node is None or node.op != 'reshape5':
            raise ValueError('output %d is not a Reshape5 of a convolution\'s logits' % i)
        conv = node.inputs[0].node
        if conv is None or conv.op != 'conv2d' or conv.attrs['k'] != 1 or conv.attrs['stride'] != 1 or conv.attrs['use_bias']:
            raise ValueError('output %d is not produced by a bias-free 1x1 convolution (found %s)' % (i, 'the input' if conv is None else conv.op))
        convs.append(conv)
    return convs


def yolov3_features(model):
    """``Model`` on ``model``'s input whose outputs are the INPUTS of the convolutions that produce ``model``'s logits (``bu1_y``,
    ``bu2_y``, ``bu3_y`` of ``yolov3_body``): dense float32 [B,G,G,cin] per scale.  It is the body a frozen-layers training stage
    (reference code/train.py:150-171) runs in inference mode; its ``param_shapes`` are ``model``'s without the output
    convolutions' kernels, so ``features.set_weights(model.get_weights())`` shares the body weights.  Float32 plans only."""
    if model.dtype != 0:
        raise NotImplementedError('yolov3_features: float32 plans only (the model was built under the %s policy)' % rt.DTYPE_NAME[model.dtype])
    feats = [_own_producer(conv.inputs[0]) for conv in output_convs(model)]
    return Model(model.inputs, feats, dtype='float32')


def _own_producer(t):
    """A tensor equal to ``t`` that nothing else consumes.  A plan writes a model output densely (a channel stride of 75), which no
    op of the plan can read back (sources need a stride that is a multiple of 4) - and the features of ``bu3`` and ``bu2`` also feed
    the bottom-up path.  So the 1x1 convolution that produces a feature (with its BatchNorm and activation, if any) is recorded a
    second time under the SAME layer names, hence the same parameters: the copy feeds the output, the original the rest of the
    graph (the throughput plan runs both as one two-output convolution; an original that nothing else consumes is dead and is
    dropped).  A feature with another kind of producer is returned as it is."""
    chain, x = [], t
    while x.node is not None and x.node.op in ('batchnorm', 'act'):
        chain.append(x.node)
        x = x.node.inputs[0]
    n = x.node
    if n is None or n.op != 'conv2d' or n.attrs['k'] != 1 or n.attrs['stride'] != 1:
        return t
    x = L.Node('conv2d', list(n.inputs), n.output.shape, n.attrs, n.params, n.name).output
    for n in reversed(chain):
        x = L.Node(n.op, [x], n.output.shape, n.attrs, n.params, n.name).output
    return x


# ----------------------------------------------------------------------------- post-processing
def _hw(shape):
    if isinstance(shape, torch.Tensor):
        shape = shape.tolist()
    return int(shape[0]), int(shape[1])


def yolo_head(feats, anchors, input_shape, calc_loss=False):
    """Convert final layer features to bounding box parameters (model.py:344-371).
    feats [B,G,G,A,C+5] CUDA f32; returns (box_xy, box_wh, box_confidence, box_class_probs), or with calc_loss
    (grid, box_xy, box_wh, box_confidence) (:368-369): grid [gh,gw,1,2] float32 holds (x, y) of each cell."""
    box_xy, box_wh, box_confidence, box_class_probs = rt.yolo_head(feats.contiguous(), anchors, _hw(input_shape))
    if calc_loss:
        gh, gw = feats.shape[1:3]
        grid = torch.empty((gh, gw, 1, 2), dtype=torch.float32, device=feats.device)   # :355-360, indices only
        grid[..., 0] = torch.arange(gw, dtype=torch.float32, device=feats.device).reshape(1, gw, 1)
        grid[..., 1] = torch.arange(gh, dtype=torch.float32, device=feats.device).reshape(gh, 1, 1)
        return grid, box_xy, box_wh, box_confidence
    return box_xy, box_wh, box_confidence, box_class_probs


def yolo_correct_boxes(box_xy, box_wh, input_shape, image_shape):
    """Letterbox inverse + clip (model.py:374-399); image_shape (h,w) or one per image."""
    hw = rt.image_hw_tensor(image_shape, box_xy.shape[0], box_xy.device)
    return rt.correct_boxes(box_xy.contiguous(), box_wh.contiguous(), _hw(input_shape), hw)


def yolo_boxes_and_scores(feats, anchors, num_classes, input_shape, image_shape, zoom_feats=None):
    """model.py:402-428.  Returns boxes [B*G*G*A,4] and scores [B*G*G*A,C], batch folded in
    exactly like the reference's reshapes (:425,427)."""
    box_xy, box_wh, _, _, box_scores = rt.yolo_head(feats.contiguous(), anchors, _hw(input_shape),
                                                     with_scores=True)
    if zoom_feats is not None:
        # zoom-in TTA (model.py:408-417): same head on the second set of logits, mapped back with the reference's
        # hard-coded constants, concatenated on the anchor axis.  This per-scale, reference-layout helper glues the
        # two head outputs with elementwise tensor ops (multiply, then add: the same two fp32 roundings); the fused
        # path (yolo_eval / yr_decode_zoom) does it inside the decode kernel.
        xy_z, wh_z, _, _, scores_z = rt.yolo_head(zoom_feats.contiguous(), anchors, _hw(input_shape), with_scores=True)
        xy_z = xy_z * rt.ZOOM_MUL + rt.ZOOM_ADD
        wh_z = wh_z * rt.ZOOM_MUL
        box_xy = torch.cat([box_xy, xy_z], -2)
        box_wh = torch.cat([box_wh, wh_z], -2)
        box_scores = torch.cat([box_scores, scores_z], -2)
    boxes = yolo_correct_boxes(box_xy, box_wh, input_shape, image_shape).reshape(-1, 4)
    return boxes, box_scores.reshape(-1, num_classes)


def yolo_eval(yolo_outputs, anchors, num_scales, num_classes, image_shape, max_boxes=20, score_threshold=.6,
              iou_threshold=.5, zoom_outputs=None):
    """Evaluate YOLO model on given input and return filtered boxes (model.py:431-491).

    yolo_outputs: [y1,y2,y3] CUDA tensors [B,G,G,A,C+5]; image_shape: (h,w) or [B,2].
    B==1: returns (boxes int32 [K,4] (ymin,xmin,ymax,xmax), scores f32 [K], classes int32 [K]),
    class-ascending then NMS pick order.  B>1: returns a list of such triples, one per image."""
    det, cnt = yolo_eval_packed(yolo_outputs, anchors, num_scales, num_classes, image_shape, max_boxes,
                                score_threshold, iou_threshold, zoom_outputs=zoom_outputs)
    res = unpack_detections(det, cnt)
    return res[0] if len(res) == 1 else res


def yolo_eval_packed(yolo_outputs, anchors, num_scales, num_classes, image_shape, max_boxes=20,
                     score_threshold=.6, iou_threshold=.5, zoom_outputs=None):
    """Device-resident form of ``yolo_eval``: decode -> per-(image,class) NMS -> packed records.
    Returns det int32 [B, C*max_boxes, 6] and det_count int32 [B] (layout: include/yoloret_hip.h).
    zoom_outputs: the logits of the zoom-in TTA pass (model.py:454-459); the NMS then runs over 2N boxes."""
    ys = [y.contiguous() for y in yolo_outputs[:num_scales]]
    zs = None if zoom_outputs is None else [z.contiguous() for z in zoom_outputs[:num_scales]]
    b = ys[0].shape[0]
    anchors = np.asarray(anchors, np.float32).reshape(-1, 2)
    input_hw = (ys[0].shape[1] * 32, ys[0].shape[2] * 32)  # model.py:449
    hw = rt.image_hw_tensor(image_shape, b, ys[0].device)
    boxes, scores = rt.decode(ys, anchors, num_classes, hw, input_hw, num_scales, zoom_ys=zs)
    idx, count = rt.nms(boxes, scores, max_boxes, score_threshold, iou_threshold)
    return rt.pack_detections(boxes, scores, idx, count)


def unpack_detections(det, det_count):
    """Packed records -> list of (boxes int32 [K,4], scores f32 [K], classes int32 [K]) on the host side
    of the boundary (one synchronising copy of the counts)."""
    counts = det_count.tolist()
    out = []
    for i, k in enumerate(counts):
        rows = det[i, :k]
        out.append((rows[:, 0:4].contiguous(), rows[:, 4].contiguous().view(torch.float32), rows[:, 5].contiguous()))
    return out


class YoloEval:
    """Keras-layer wrapper around yolo_eval (model.py:494-526)."""

    def __init__(self, anchors, num_scales, num_classes, max_boxes=20, score_threshold=.6, iou_threshold=.5,
                 name=None, **kwargs):
        self.anchors = anchors
        self.num_scales = num_scales
        self.num_classes = num_classes
        self.max_boxes = max_boxes
        self.score_threshold = score_threshold
        self.iou_threshold = iou_threshold
        self.name = name

    def call(self, yolo_outputs, image_shape, zoom_outputs=None):
        return yolo_eval(yolo_outputs, self.anchors, self.num_scales, self.num_classes, image_shape,
                         self.max_boxes, self.score_threshold, self.iou_threshold, zoom_outputs=zoom_outputs)

    __call__ = call

    def get_config(self):
        return {'name': self.name, 'anchors': self.anchors, 'num_scales': self.num_scales,
                'num_classes': self.num_classes, 'max_boxes': self.max_boxes,
                'score_threshold': self.score_threshold, 'iou_threshold': self.iou_threshold}


# ----------------------------------------------------------------------------- loss: forward, and the gradient w.r.t. the logits
class _YoloLossFunction(torch.autograd.Function):
    """``YoloLoss.call`` for logits that require a gradient.  forward is the call of ``yr_yolo_loss`` that ``call`` makes anyway;
    backward RECOMPUTES: nothing but the two inputs is saved, and one call of ``yr_yolo_loss_grad`` with ``grad_output`` as
    its ``upstream`` (read on the device) yields the logits' gradient - no torch arithmetic on either side."""

    @staticmethod
    def forward(ctx, yolo_output, y_true, layer, input_hw):
        terms = rt.yolo_loss(yolo_output, y_true, layer.anchor, input_hw, layer.ignore_thresh)
        ctx.save_for_backward(yolo_output, y_true)
        ctx.anchor, ctx.input_hw, ctx.ignore_thresh = layer.anchor, input_hw, layer.ignore_thresh
        layer.last_terms = terms
        return terms[0]

    @staticmethod
    def backward(ctx, grad_output):
        yolo_output, y_true = ctx.saved_tensors
        upstream = grad_output.to(torch.float32).contiguous()      # (a 0-d float32 tensor on the logits' device already)
        _, dfeats = rt.yolo_loss_grad(yolo_output, y_true, ctx.anchor, ctx.input_hw, ctx.ignore_thresh, upstream=upstream)
        return dfeats, None, None, None


class YoloLoss:
    """The loss of one output scale (model.py:585-691): the GIoU / confidence / class sums of the GIOU branch (:623-671)
    from the logits on the device, in one call of the HIP kernels behind ``yr_yolo_loss``, and the gradient of that scalar
    with respect to the logits (``yr_yolo_loss_grad``); there is no backward through the network.

    ``call(y_true, yolo_output)``: both [B,gh,gw,A,5+C] float32 CUDA tensors (``y_true`` as ``preprocess_true_boxes``
    writes it; a NumPy array is copied to the logits' device) -> the 0-d float32 device tensor ``loss``.
    ``last_terms`` keeps the device tensor [5] = (loss, giou_loss, confidence_loss, class_loss, ignore_sum) of the last
    call.  As in the reference, the labelled boxes a prediction is compared with are those of the whole batch (:643).
    When ``yolo_output.requires_grad``, the same value comes back attached to a ``torch.autograd.Function`` whose backward
    calls ``yr_yolo_loss_grad`` with the incoming gradient as ``upstream``: ``loss.backward()`` fills the logits' ``.grad``.
    ``gradient(y_true, yolo_output, upstream=None)`` -> d loss / d yolo_output (times ``upstream``: a number, or a float32
    tensor of one element on the logits' device) in the shape that was passed; it sets ``last_terms`` and never prints.
    ``print_loss`` prints the reference's line "<idx>: giou conf class ignore_sum" (:671); reading the four numbers
    SYNCHRONISES with the device, so pass ``print_loss=False`` where the loss is evaluated inside a pipeline.
    ``box_loss=BOX_LOSS.MSE`` raises NotImplementedError: the reference's MSE branch reads names that do not exist
    in its scope (:676, :688) and cannot run there either."""

    def __init__(self, idx, anchors, num_scales, ignore_thresh=.5, box_loss=BOX_LOSS.GIOU, print_loss=True):
        if box_loss != BOX_LOSS.GIOU:
            raise NotImplementedError('box_loss=%r: only BOX_LOSS.GIOU runs (the reference\'s MSE branch does not either)' % (box_loss,))
        grid_steps = [32, 16, 8]
        anchor_masks = [[6, 7, 8], [3, 4, 5], [0, 1, 2]][-1 * num_scales:]     # :597-598
        self.idx = idx
        self.ignore_thresh = ignore_thresh
        self.box_loss = box_loss
        self.print_loss = print_loss
        self.grid_step = grid_steps[self.idx]
        self.anchor = np.asarray(anchors, np.float32).reshape(-1, 2)[anchor_masks[idx]]
        self.last_terms = None

    def _inputs(self, y_true, yolo_output):
        """-> (y_true, yolo_output) as [B,gh,gw,A,5+C], input_hw"""
        if not isinstance(yolo_output, torch.Tensor):
            raise ValueError('yolo_output must be a CUDA tensor (the logits of yolov3_body)')
        if not isinstance(y_true, torch.Tensor):
            y_true = torch.as_tensor(np.ascontiguousarray(y_true, np.float32), device=yolo_output.device)
        if yolo_output.dim() == 4 and yolo_output.shape[3] % len(self.anchor) == 0:    # [B,gh,gw,A*(5+C)], as a serialised plan emits it
            yolo_output = yolo_output.reshape(tuple(yolo_output.shape[:3]) + (len(self.anchor), -1))
        if yolo_output.dim() != 5:
            raise ValueError('yolo_output has shape %s, expected [B,gh,gw,A,5+C]' % (tuple(yolo_output.shape),))
        if y_true.dim() == 4 and y_true.numel() == yolo_output.numel():
            y_true = y_true.reshape(yolo_output.shape)
        input_hw = (yolo_output.shape[1] * self.grid_step, yolo_output.shape[2] * self.grid_step)   # :628
        return y_true, yolo_output, input_hw

    def call(self, y_true, yolo_output):
        y_true, yolo_output, input_hw = self._inputs(y_true, yolo_output)
        if yolo_output.requires_grad and torch.is_grad_enabled():
            loss = _YoloLossFunction.apply(yolo_output.contiguous(), y_true.detach().contiguous(), self, input_hw)   # (sets last_terms)
            terms = self.last_terms
        else:
            terms = rt.yolo_loss(yolo_output.contiguous(), y_true.contiguous(), self.anchor, input_hw, self.ignore_thresh)
            self.last_terms = terms
            loss = terms[0]
        if self.print_loss:
            t = terms.tolist()   # (synchronises)
            print('%d: %s %s %s %s' % ((self.idx,) + tuple(str(np.float32(v)) for v in t[1:])))
        return loss

    __call__ = call

    def gradient(self, y_true, yolo_output, upstream=None):
        shape = tuple(yolo_output.shape) if isinstance(yolo_output, torch.Tensor) else None
        y_true, yolo_output, input_hw = self._inputs(y_true, yolo_output)
        if upstream is not None and not isinstance(upstream, torch.Tensor):
            upstream = torch.full((1,), float(upstream), dtype=torch.float32, device=yolo_output.device)
        terms, dfeats = rt.yolo_loss_grad(yolo_output.detach().contiguous(), y_true.detach().contiguous(), self.anchor, input_hw,
                                          self.ignore_thresh, upstream=upstream)
        self.last_terms = terms
        return dfeats.reshape(shape)


def _check_scales(name, yolo_outputs, y_trues, num_scales):
    if len(yolo_outputs) < num_scales or len(y_trues) < num_scales:
        raise ValueError('%s: %d logit tensors and %d label tensors for %d scales' % (name, len(yolo_outputs), len(y_trues), num_scales))


def yolo_loss(yolo_outputs, y_trues, anchors, num_scales, ignore_thresh=.5):
    """The sum the reference forms over its list of per-scale losses: -> (total 0-d float32 device tensor,
    terms [num_scales,5] device tensor, one row of (loss, giou, conf, class, ignore_sum) per scale)."""
    _check_scales('yolo_loss', yolo_outputs, y_trues, num_scales)
    rows = []
    for idx in range(num_scales):
        layer = YoloLoss(idx, anchors, num_scales, ignore_thresh, BOX_LOSS.GIOU, print_loss=False)
        layer(y_trues[idx], yolo_outputs[idx])
        rows.append(layer.last_terms)
    terms = torch.stack(rows)
    return terms[:, 0].sum(), terms


def yolo_loss_and_grad(yolo_outputs, y_trues, anchors, num_scales, ignore_thresh=.5):
    """``yolo_loss`` and the gradient of its total (the sum over the scales, train.py:18-46) with respect to every logit
    tensor, one call of ``yr_yolo_loss_grad`` per scale -> (total, terms, grads): total and terms as ``yolo_loss`` returns
    them (the same bits), grads[i] float32 of the shape of yolo_outputs[i]."""
    _check_scales('yolo_loss_and_grad', yolo_outputs, y_trues, num_scales)
    rows, grads = [], []
    for idx in range(num_scales):
        layer = YoloLoss(idx, anchors, num_scales, ignore_thresh, BOX_LOSS.GIOU, print_loss=False)
        grads.append(layer.gradient(y_trues[idx], yolo_outputs[idx]))
        rows.append(layer.last_terms)
    terms = torch.stack(rows)
    return terms[:, 0].sum(), terms, grads


def _labels_from_boxes(name, yolo_outputs, true_boxes, anchors, num_classes, num_scales):
    from .utils import preprocess_true_boxes_device
    if len(yolo_outputs) < num_scales:
        raise ValueError('%s: %d logit tensors for %d scales' % (name, len(yolo_outputs), num_scales))
    y0 = yolo_outputs[0]
    if not (isinstance(y0, torch.Tensor) and y0.is_cuda and y0.dim() in (4, 5)):
        raise ValueError('yolo_outputs must be CUDA tensors (the logits of yolov3_body)')
    input_hw = (y0.shape[1] * 32, y0.shape[2] * 32)
    with torch.cuda.device(y0.device):
        y_trues = preprocess_true_boxes_device(true_boxes, input_hw, anchors, num_classes, num_scales, device=y0.device)
    return [y_trues] if num_scales == 1 else list(y_trues)


def yolo_loss_from_boxes(yolo_outputs, true_boxes, anchors, num_classes, num_scales, ignore_thresh=.5):
    """``yolo_loss`` from ground-truth boxes instead of encoded labels: true_boxes [B,T,5] rows (x_min, y_min, x_max, y_max,
    class) in pixels of the network input (a NumPy array or a float32 tensor on the logits' device), encoded on the logits'
    device and current stream by the kernels behind ``yr_encode_labels`` - the label tensors never exist on the host.  The
    input shape is derived from the grid of the first output, as YoloLoss does (:628) -> (total, terms) of ``yolo_loss``."""
    y_trues = _labels_from_boxes('yolo_loss_from_boxes', yolo_outputs, true_boxes, anchors, num_classes, num_scales)
    return yolo_loss(yolo_outputs, y_trues, anchors, num_scales, ignore_thresh)


def yolo_loss_and_grad_from_boxes(yolo_outputs, true_boxes, anchors, num_classes, num_scales, ignore_thresh=.5):
    """``yolo_loss_and_grad`` with the labels encoded from ground-truth boxes on the device, as ``yolo_loss_from_boxes``
    does -> (total, terms, grads)."""
    y_trues = _labels_from_boxes('yolo_loss_and_grad_from_boxes', yolo_outputs, true_boxes, anchors, num_classes, num_scales)
    return yolo_loss_and_grad(yolo_outputs, y_trues, anchors, num_scales, ignore_thresh)
