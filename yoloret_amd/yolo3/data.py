"""The data paths - mirror of reference code/yolo3/data.py: label file -> batches of (images, y_true) on the GPU.
``Dataset`` is the validation path, ``mode=VALIDATE`` / ``TEST`` (both ``train=False``: one fixed letterbox per image);
``AugmentedDataset`` is the training path (``train=True``: shuffled records, get_random_data's augmentation).

``Dataset(...)`` has the reference's constructor (:151-167) plus ``device`` and ``root``; ``build()`` (:172-200) returns
``(iterable, num)`` and raises its errors.  Per batch only the JPEG / PNG decode (PIL) and the text parse stay on the host:

    map.parse_text -> PIL decode -> runtime.RaggedStager (one pinned buffer, one copy)
                   -> runtime.ingest_batch(INGEST_VALIDATE): get_random_data(train=False) for images AND boxes (utils.py:239-295)
                   -> runtime.encode_labels: preprocess_true_boxes (utils.py:298-376)

``AugmentedDataset`` runs runtime.augment_batch in place of ingest_batch and, with ``apply_jpeg=True``, runtime.jpeg_roundtrip_batch
(random_jpeg_quality, utils.py:228-230) behind it.

Differences that are deliberate:
  * iteration is deterministic - files sorted, lines in order, batches of ``batch_size`` with a shorter last one.  The reference's
    ``interleave(cycle_length=AUTOTUNE)`` leaves the order open, and the loss depends on which images share a batch (the labelled
    boxes are gathered over the whole batch, model.py:643);
  * ``Dataset(mode=TRAIN)`` still raises NotImplementedError: the training path is a class of its own, ``AugmentedDataset``, with
    its seed and the augmentation's parameters in the constructor.  ``zoom_in=True`` (the experimental branch of
    utils.py:243-245,279-283) is not built.  TFRecord files need TensorFlow's proto parser (as in map.py).
"""
import glob
import os

import numpy as np

from .enums import DATASET_MODE
from .map import parse_text

MAX_BOXES = 20      # get_random_data's max_boxes (utils.py:142)


def decode_image(path):
    """tf.io.decode_image(tf.io.read_file(path), channels=3) on the host (data.py:73-75) -> uint8 [h,w,3]; the /255 of
    dtype=float32 happens in the ingest kernel."""
    from PIL import Image
    with Image.open(path) as img:
        return np.array(img.convert('RGB'), dtype=np.uint8)


class _Batches:
    """The iterable ``Dataset.build`` returns: every pass reads the label files again and yields (images, y_true)."""

    def __init__(self, dataset, files):
        self.dataset, self.files = dataset, files

    def __iter__(self):
        for records in self.dataset.record_batches(self.files):
            yield self.dataset.load_batch(records)


class Dataset(object):
    def __init__(self, glob_path, batch_size, anchors=None, num_classes=None, input_shape=None, num_scales=None,
                 mode=DATASET_MODE.TRAIN, zoom_in=False, device=None, root=None):
        self.glob_path = glob_path
        self.batch_size = batch_size
        self.input_shape = input_shape
        self.anchors = anchors
        self.num_classes = num_classes
        self.num_scales = num_scales
        self.mode = mode
        self.zoom_in = zoom_in
        self.device = device
        self.root = root
        self.last_boxes = None      # (boxes_out [b,20,5], kept [b]) of the last batch, on the device
        self._stager = None

    def _get_num_from_name(self, name):
        return int(name.split('/')[-1].split('.')[0].split('_')[-1])

    def _label_files(self):
        """-> (the files ``glob_path`` matches, the number of records their names promise): data.py:172-183."""
        files = sorted(glob.glob(self.glob_path))
        if len(files) == 0:
            raise ValueError('No file found')
        try:
            num = sum(self._get_num_from_name(f) for f in files)
        except Exception:
            raise ValueError('Please format file name like <name>_<number>.<extension>')
        if any(f.endswith(('.tfrecord', '.tfrecords')) for f in files):
            raise NotImplementedError('TFRecord label files need TensorFlow; use the text format')
        return files, num

    @staticmethod
    def _text_files(files):
        txts = [f for f in files if f.endswith('.txt')]
        if not txts:
            raise ValueError('No .txt label file among %d matching files' % len(files))
        return txts

    def build(self, split=None):
        if self.glob_path is None:
            return None, 0
        files, num = self._label_files()
        if self.mode == DATASET_MODE.TRAIN:
            raise NotImplementedError('Dataset(mode=TRAIN): the TRAIN data path is yolo3.data.AugmentedDataset; Dataset takes DATASET_MODE.VALIDATE or TEST')
        if self.mode not in (DATASET_MODE.VALIDATE, DATASET_MODE.TEST):
            raise ValueError('Dataset: mode must be a DATASET_MODE, not %r' % (self.mode,))
        if self.zoom_in:
            raise NotImplementedError('Dataset(zoom_in=True): the zoom-in branch of get_random_data is not built')
        return _Batches(self, self._text_files(files)), num

    # ------------------------------------------------------------------------- host side
    def records(self, files):
        """(image path, float32 [n,5] rows (xmin, ymin, xmax, ymax, label)) per non-empty line, files and lines in order."""
        for f in files:
            with open(f) as fh:
                for line in fh:
                    if line.strip():
                        yield parse_text(line)

    def record_batches(self, files):
        """Lists of ``batch_size`` records, the last one shorter."""
        size = max(int(self.batch_size), 1)
        batch = []
        for rec in self.records(files):
            batch.append(rec)
            if len(batch) == size:
                yield batch
                batch = []
        if batch:
            yield batch

    def decode_batch(self, records):
        """What stays on the host per batch: -> (decoded uint8 images, float32 [b,max_in,5] rows padded with zeros, int32 [b] counts)."""
        from .. import runtime as rt
        images = [decode_image(path if self.root is None else os.path.join(self.root, path)) for path, _ in records]
        counts = np.asarray([bb.shape[0] for _, bb in records], np.int32)
        if counts.max() > rt.INGEST_MAX_BOXES:
            raise ValueError('Dataset: %s has %d boxes, at most %d are supported' % (records[int(counts.argmax())][0], counts.max(), rt.INGEST_MAX_BOXES))
        boxes = np.zeros((len(records), max(1, int(counts.max())), 5), np.float32)
        for i, (_, bb) in enumerate(records):
            boxes[i, :bb.shape[0]] = bb
        return images, boxes, counts

    # ------------------------------------------------------------------------- device side
    def load_batch(self, records):
        """One batch of records -> (images [b,H,W,3] float32, y_true tuple of num_scales tensors [b,gh,gw,3,5+C]) on the device."""
        import torch
        from .. import runtime as rt
        dev = torch.device(self.device if self.device is not None else 'cuda:0')
        if self._stager is None or self._stager.device != dev:
            self._stager = rt.RaggedStager(dev)
        images, boxes, counts = self.decode_batch(records)
        packed, table = self._stager.upload(images, self.input_shape, rt.INGEST_VALIDATE)
        x, boxes_out, kept = rt.ingest_batch(packed, table, self.input_shape, boxes=torch.from_numpy(boxes).to(dev),
                                             box_count=torch.from_numpy(counts).to(dev), max_boxes=MAX_BOXES)
        self.last_boxes = (boxes_out, kept)
        y_true = rt.encode_labels(boxes_out, self.input_shape, self.anchors, self.num_classes, self.num_scales)
        return x, tuple(y_true)


class _AugmentedBatches:
    """The iterable ``AugmentedDataset.build`` returns: every pass shuffles the records and draws new augmentations."""

    def __init__(self, dataset, files, rng, jpeg_rng=None):
        self.dataset, self.files, self.rng, self.jpeg_rng = dataset, files, rng, jpeg_rng

    def __iter__(self):
        for records, draws in self.dataset.epoch_plan(self.files, self.rng):
            jpeg_draws = self.jpeg_rng.random(len(records), dtype=np.float32) if self.dataset.jpeg else None
            yield self.dataset.load_batch(records, draws, jpeg_draws)


class AugmentedDataset(Dataset):
    """The training data path: ``Dataset(mode=TRAIN)`` of the reference (data.py:172-200 with ``shuffle(train_num)``, parse_text
    calling ``get_random_data(train=True)``).  Per pass the records are permuted and ten uniforms per image are drawn, both from one
    ``np.random.Generator`` seeded with ``seed`` in ``build()``: the same seed yields the same batches, byte for byte, and every
    further pass of one iterable a new order and new draws.  Per batch the host decodes (PIL) and stages once; the device does the
    rest: ``runtime.augment_batch`` (utils.py:170-227, 258-293), ``runtime.jpeg_roundtrip_batch`` (:228-230) when switched on, then
    ``runtime.encode_labels``.

    The augmentation's keyword arguments are ``yolo3.utils.get_random_data_device``'s: jitter, min_scale, max_scale, min_gamma,
    max_gamma, flip, hue, sat, cont are honoured; val, noise, blur, zoom_in raise NotImplementedError when switched on.

    ``apply_jpeg=True`` is the reference's default behaviour: ``random_jpeg_quality`` with the bounds ``min_jpeg_quality`` /
    ``max_jpeg_quality`` (80 / 100) as the last image step, run iff min < max.  The default here is False - the bytes of every batch
    stay what they were before the step was built, and the bounds are accepted and unused.  The qualities come from a second
    generator, ``np.random.default_rng((seed, 1))`` made in ``build()``, one float32 uniform per image in batch order: records, the
    ten draws, boxes and y_true of a seed do not depend on the switch.  ``last_quality`` holds the last batch's qualities."""

    def __init__(self, glob_path, batch_size, anchors=None, num_classes=None, input_shape=None, num_scales=None, seed=0, device=None,
                 root=None, min_scale=0.25, max_scale=2, jitter=0.3, min_gamma=0.8, max_gamma=2, blur=False, flip=True, hue=.5, sat=.5,
                 val=0., cont=.1, noise=0, min_jpeg_quality=80, max_jpeg_quality=100, zoom_in=False, apply_jpeg=False):
        from .utils import _augment_params, _check_jpeg_bounds
        super().__init__(glob_path, batch_size, anchors, num_classes, input_shape, num_scales, mode=DATASET_MODE.TRAIN, zoom_in=zoom_in,
                         device=device, root=root)
        self.seed = seed
        self.flip = flip
        self.params = _augment_params(min_scale, max_scale, jitter, min_gamma, max_gamma, blur, hue, sat, val, cont, noise, zoom_in)
        self.last_draws = None      # float32 [b,10] of the last batch
        self.jpeg = bool(apply_jpeg) and min_jpeg_quality < max_jpeg_quality      # utils.py:228
        self.jpeg_bounds = (min_jpeg_quality, max_jpeg_quality)
        if self.jpeg:
            _check_jpeg_bounds(min_jpeg_quality, max_jpeg_quality)
        self.last_quality = None    # int32 [b] of the last batch (apply_jpeg=True)

    def build(self, split=None):
        if self.glob_path is None:
            return None, 0
        files, num = self._label_files()
        return _AugmentedBatches(self, self._text_files(files), np.random.default_rng(self.seed),
                                 np.random.default_rng((self.seed, 1) if self.seed is not None else None)), num

    def epoch_plan(self, files, rng):
        """One pass, host only: [(records, draws float32 [b,10])] - the records permuted (the reference's shuffle over the whole
        set), cut into batches of ``batch_size`` with a shorter last one, each batch with its images' ten draws."""
        records = list(self.records(files))
        order = rng.permutation(len(records))
        size = max(int(self.batch_size), 1)
        plan = []
        for at in range(0, len(order), size):
            batch = [records[i] for i in order[at:at + size]]
            plan.append((batch, rng.random((len(batch), 10), dtype=np.float32)))
        return plan

    def load_batch(self, records, draws, jpeg_draws=None):
        """One batch of records and its draws (``jpeg_draws``: float32 [b], needed with apply_jpeg=True) -> (images [b,H,W,3] float32,
        y_true tuple) on the device."""
        import torch
        from .. import runtime as rt
        from .utils import get_random_data_device, random_jpeg_quality_device
        if self.jpeg and jpeg_draws is None:
            raise ValueError('AugmentedDataset.load_batch: apply_jpeg=True needs the batch\'s jpeg_draws')
        dev = torch.device(self.device if self.device is not None else 'cuda:0')
        if self._stager is None or self._stager.device != dev:
            self._stager = rt.RaggedStager(dev)
        images, boxes, counts = self.decode_batch(records)
        x, boxes_out, kept = get_random_data_device(images, boxes, counts, self.input_shape, draws=draws, flip=self.flip, max_boxes=MAX_BOXES,
                                                    device=dev, stager=self._stager, **self.params)
        self.last_boxes, self.last_draws = (boxes_out, kept), draws
        if self.jpeg:
            _, self.last_quality = random_jpeg_quality_device(x, self.jpeg_bounds[0], self.jpeg_bounds[1], draws=jpeg_draws)
        y_true = rt.encode_labels(boxes_out, self.input_shape, self.anchors, self.num_classes, self.num_scales)
        return x, tuple(y_true)
