"""VOC mAP with the matching on the GPU (MAPCallback(on_device=True) -> YoloModel.call_packed -> DeviceEvaluator -> yr_voc_match)
against the host path, on the setup of tests/test_gpu_yolo.py::test_map_callback_through_the_hip_model: the MobileNetV2 x0.75
synthetic model at 96x96, three PNGs of different sizes, labels taken from the detector's own output.  All comparisons exact."""
from functools import partial

import numpy as np
import pytest
import torch

from tests.test_gpu_yolo import _png
from tests.util import ANCHORS

pytestmark = pytest.mark.gpu

NAMES = ['c%d' % i for i in range(20)]


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from yoloret_amd.yolo import YoloModel
    from yoloret_amd.yolo3.map import parse_text
    from yoloret_amd.yolo3.model import yolov3_body
    tmp = tmp_path_factory.mktemp('map_device')
    body = partial(yolov3_body, model_name='mobilenetv2x75', num_anchors=3, num_classes=20)
    ym = YoloModel(body, 9, 3, NAMES, 'synthetic:3', ANCHORS, (96, 96), score=0.2, nms=0.5)
    rng = np.random.default_rng(4)
    images, lines, truth = [], [], {}
    for i, (h, w) in enumerate([(80, 120), (96, 96), (60, 50)]):
        path = tmp / ('img%d.png' % i)
        path.write_bytes(_png(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
        images.append(path.read_bytes())
        boxes, scores, classes = [t.cpu().numpy() for t in ym([images[-1]])]
        assert len(boxes) > 0
        rows = [[b[1], b[0], b[3], b[2], c] for b, c in zip(boxes.tolist(), classes.tolist())]      # (xmin, ymin, xmax, ymax, label)
        lines.append(str(path) + ' ' + ' '.join('%d %d %d %d %d' % tuple(int(v) for v in r) for r in rows))
        truth[i] = parse_text(lines[-1])[1]
    labels = tmp / 'labels.txt'
    labels.write_text('\n'.join(lines) + '\n')
    return ym, images, truth, str(labels)


def _rows(results, first):
    """triples of the model -> rows of evaluate_detections, image indices from `first`"""
    pred = []
    for i, (boxes, scores, classes) in enumerate(results):
        pred += [[first + i, c, s, b[1], b[0], b[3], b[2]] for b, s, c in zip(boxes.cpu().numpy().tolist(), scores.cpu().numpy(), classes.cpu().numpy().tolist())]
    return pred


def test_call_packed_is_call_before_unpacking(setup):
    from yoloret_amd.yolo3.model import unpack_detections
    ym, images = setup[0], setup[1]
    for batch in ([images[0]], images):
        det, cnt = ym.call_packed(batch)
        assert det.dtype == torch.int32 and tuple(det.shape) == (len(batch), 20 * 20, 6) and tuple(cnt.shape) == (len(batch),) and det.is_cuda
        got = unpack_detections(det, cnt)
        want = ym(batch)
        want = [want] if len(batch) == 1 else want
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert all(torch.equal(a, b) for a, b in zip(g, w)) and len(g[1]) > 0


def test_on_device_equals_the_host_path_image_by_image(setup):
    from yoloret_amd.yolo3.map import MAPCallback
    ym, _, _, labels = setup
    host = MAPCallback(labels, (96, 96), NAMES, iou=0.5)
    host.set_model(ym)
    want = host.calculate_aps()
    cb = MAPCallback(labels, (96, 96), NAMES, iou=0.5, batch_size=1, on_device=True)
    cb.set_model(ym)
    got = cb.calculate_aps()
    assert got == want and all(type(got[c]) is type(want[c]) for c in want) and cb.seconds_per_image > 0
    assert max(want.values()) > 0.9


def test_batches_of_two_and_one(setup, capsys):
    """batch_size=2 over three records: the APs of evaluate_detections over the rows of ym([a, b]) and ym([c]) - the same grouping,
    since another batch size may select another plan, whose logits may differ in the last bits"""
    from yoloret_amd.yolo3.map import MAPCallback, evaluate_detections
    ym, images, truth, labels = setup
    pred = _rows(ym(images[:2]), 0) + _rows([ym(images[2:])], 2)
    want = evaluate_detections(pred, truth, 20, 0.5)
    cb = MAPCallback(labels, (96, 96), NAMES, iou=0.5, batch_size=2, on_device=True)
    cb.set_model(ym)
    got = cb.calculate_aps()
    assert got == want and all(type(got[c]) is type(want[c]) for c in want)
    logs = cb.on_train_end({})
    assert logs['mAP'] == float(np.mean([want[c] for c in want])) and 'mAP: ' in capsys.readouterr().out
