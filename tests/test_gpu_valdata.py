"""The validation data path end to end on the device: a label file -> yolo3.data.Dataset (PIL decode -> one staged copy ->
yr_ingest_batch in VALIDATE mode -> yr_encode_labels) -> yolo3.train.validation_loss, against PIL decode -> tests/valdata_ref.py
-> the host preprocess_true_boxes; and YoloModel.call_packed's ragged ingest against the per-image letterbox it replaces.

The label file names the two committed demo JPEGs and one PNG written here; batch_size 2 gives batches of 2 and 1.  Model and
size are the smallest the loss tests use: MobileNetV2 x0.75 with the oracle's synthetic weights at 96x96, 20 classes."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import valdata_ref as vr
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
HW, C, S = (96, 96), 20, 3


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _build(tmp):
    """-> (label file, decoded images, label rows; the reference's images, boxes, counts and y_true per record), computed once."""
    from PIL import Image
    from yoloret_amd.yolo3.utils import preprocess_true_boxes
    png = tmp / 'third.png'
    Image.fromarray(np.random.RandomState(11).randint(0, 256, size=(61, 45, 3)).astype(np.uint8)).save(str(png))
    paths = [os.path.join(GOLDEN, 'demo_2011_001694.jpg'), os.path.join(GOLDEN, 'demo_2011_002558.jpg'), str(png)]
    decoded = [np.array(Image.open(p).convert('RGB'), dtype=np.uint8) for p in paths]
    rs = np.random.RandomState(12)
    lines, rows = [], []
    for k, (p, im) in enumerate(zip(paths, decoded)):
        ih, iw = im.shape[:2]
        bb = [[int(.1 * iw), int(.2 * ih), int(.6 * iw), int(.9 * ih), 3], [int(.5 * iw), int(.1 * ih), int(.95 * iw), int(.5 * ih), 11],
              [int(.3 * iw), int(.3 * ih), int(.3 * iw) + 2, int(.8 * ih), 5]]          # the third is 2 source pixels wide
        if k == 1:      # more than 20 boxes that pass the filter: the cap
            for _ in range(22):
                x, y = np.sort(rs.randint(0, iw, 2)), np.sort(rs.randint(0, ih, 2))
                bb.append([x[0], y[0], x[1] + 12, y[1] + 12, rs.randint(0, C)])
        if k == 2:
            bb = bb[:2]
        lines.append(p + ' ' + ' '.join('%d %d %d %d %d' % tuple(r) for r in bb))
        rows.append(np.asarray(bb, np.float32))
    labels = tmp / 'val_3.txt'
    labels.write_text('\n'.join(lines) + '\n')
    ref_img, ref_box, ref_kept, ref_y = [], [], [], []
    for im, bb in zip(decoded, rows):
        ref_img.append(vr.validate_image(im, HW))
        out, kept, info = vr.map_boxes(bb, im.shape[0], im.shape[1], HW)
        ref_box.append(out)
        ref_kept.append(kept)
        ref_y.append(preprocess_true_boxes(out, HW, ANCHORS, C, S))
    assert ref_kept[1] == 20 and ref_kept[2] == 2 and ref_kept[0] in (2, 3)
    assert len({im.shape[:2] for im in decoded}) == 3
    return str(labels), decoded, rows, ref_img, ref_box, ref_kept, ref_y


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return _build(tmp_path_factory.mktemp('valdata'))


def _dataset(labels, dev):
    from yoloret_amd.yolo3.data import Dataset
    from yoloret_amd.yolo3.enums import DATASET_MODE
    return Dataset(labels, 2, ANCHORS, C, HW, S, mode=DATASET_MODE.VALIDATE, device=dev)


@pytest.fixture(scope='module')
def net():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from oracle import model as om, params
    from yoloret_amd import layers as L
    from yoloret_amd.yolo3 import model as m
    n = m.yolov3_body(L.Input(shape=[HW[0], HW[1], 3]), 'mobilenetv2x75', 3, num_classes=C)
    P = params.ParamStore(1234)
    om.yolov3_body(P, params.synthetic_images(1, HW[0], HW[1]), 'mobilenetv2x75', 3, C)      # (draws the synthetic weights)
    n.set_weights(P.values)
    return n


def test_dataset_batches_equal_the_reference_in_bytes(dev, setup):
    labels, decoded, rows, ref_img, ref_box, ref_kept, ref_y = setup
    ds = _dataset(labels, dev)
    it, num = ds.build()
    assert num == 3
    at = 0
    sizes = []
    for x, y_true in it:
        b = x.shape[0]
        sizes.append(b)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (b, 96, 96, 3) and isinstance(y_true, tuple) and len(y_true) == S
        boxes_out, kept = ds.last_boxes
        torch.cuda.synchronize()
        assert kept.cpu().tolist() == ref_kept[at:at + b] and tuple(boxes_out.shape) == (b, 20, 5)
        for i in range(b):
            assert np.array_equal(_bits(x[i]), _bits(ref_img[at + i])), 'image %d' % (at + i)
            assert np.array_equal(_bits(boxes_out[i]), _bits(ref_box[at + i])), 'boxes of image %d' % (at + i)
        for s in range(S):
            want = np.stack([ref_y[at + i][s] for i in range(b)])
            assert y_true[s].is_cuda and tuple(y_true[s].shape) == want.shape
            assert np.array_equal(_bits(y_true[s]), _bits(want)), 'y_true scale %d of batch at %d' % (s, at)
        at += b
    assert sizes == [2, 1] and at == 3
    assert sum(int((y[s][..., 4] != 0).sum()) for y in ref_y for s in range(S)) >= 5
    # a second pass gives the same batches
    again = [x.clone() for x, _ in it]
    assert [a.shape[0] for a in again] == [2, 1] and np.array_equal(_bits(again[1][0]), _bits(ref_img[2]))


def test_validation_loss_equals_the_composition_by_hand(dev, setup, net):
    from tests.test_gpu_loss import _check_against_reference
    from yoloret_amd.yolo3.model import yolo_loss
    from yoloret_amd.yolo3.train import validation_loss
    labels = setup[0]
    it, _ = _dataset(labels, dev).build()
    val_loss, terms = validation_loss(net, it, ANCHORS, S)
    assert isinstance(val_loss, float) and terms.shape == (2, S, 5) and terms.dtype == np.float32
    # by hand: model(x), yolo_loss and a mean, batch by batch, everything fetched before the next forward
    totals, kept = [], []
    for x, y_true in _dataset(labels, dev).build()[0]:
        ys = net(x)
        total, t = yolo_loss(ys, list(y_true), ANCHORS, S)
        torch.cuda.synchronize()
        totals.append(np.float32(total.item()))
        kept.append((t.cpu().numpy(), [y.cpu().numpy() for y in ys], [y.cpu().numpy() for y in y_true]))
    acc = np.float32(0)
    for t in totals:
        acc = np.float32(acc + t)
    want = np.float32(acc / np.float32(len(totals)))
    print('val_loss %r, by hand %r, per batch %s' % (val_loss, float(want), totals))
    assert val_loss == float(want) and np.isfinite(val_loss) and val_loss > 0
    for b, (t, logits, y_trues) in enumerate(kept):
        assert np.array_equal(_bits(terms[b]), _bits(t))
        for s in range(S):
            lg = logits[s].reshape(y_trues[s].shape)
            _check_against_reference(terms[b, s], lg, y_trues[s], s, 'batch %d scale %d' % (b, s))
    with pytest.raises(ValueError, match='empty'):
        validation_loss(net, [], ANCHORS, S)


def test_call_packed_equals_the_per_image_letterbox(dev, setup):
    from yoloret_amd import runtime as rt
    from yoloret_amd.yolo import YoloModel
    from yoloret_amd.yolo3.model import unpack_detections, yolov3_body
    decoded = setup[1]
    body = partial(yolov3_body, model_name='mobilenetv2x75', num_anchors=3, num_classes=C)
    ym = YoloModel(body, 9, 3, ['c%d' % i for i in range(C)], 'synthetic:3', ANCHORS, HW, score=0.2, nms=0.5, device=dev)
    for batch in (decoded, decoded[2:], decoded[:2]):      # a second and third call reuse the staging buffer
        det, cnt = ym.call_packed(batch)
        det, cnt = det.clone(), cnt.clone()
        x = torch.empty((len(batch), 96, 96, 3), dtype=torch.float32, device=dev)
        for i, im in enumerate(batch):
            rt.letterbox(torch.from_numpy(im).to(dev), HW, out=x[i])
        image_hw = rt.image_hw_tensor(np.asarray([im.shape[:2] for im in batch], np.int32), len(batch), dev)
        want = unpack_detections(*ym._pipe(x, image_hw))
        got = unpack_detections(det, cnt)
        torch.cuda.synchronize()
        print('call_packed: %d images, detections per image %s' % (len(batch), cnt.cpu().tolist()))
        assert len(got) == len(want) == len(batch)
        for g, w in zip(got, want):
            assert all(torch.equal(a, b) for a, b in zip(g, w))
        # ... and the network input itself: the staged ragged ingest against the loop
        staged = rt.ingest_batch(*ym._stager.upload(batch, HW, rt.INGEST_LETTERBOX), HW)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(staged), _bits(x))
