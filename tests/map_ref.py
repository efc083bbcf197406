"""Reference for the device matcher (yr_voc_match, yoloret_amd/csrc/vocmatch.hip): the greedy loop of the reference's
MAPCallback.calculate_aps (code/yolo3/map.py:157-215) with the verdict recorded per detection row, written as a plain loop in the
reference's GLOBAL order (all detections of a class over the whole data set, by score) - not in the per-image order the kernel
uses, and sharing no code with the kernel or with yolo3.map.aps_from_flags.

Also here: the recipe of the random cases (`random_case`), the list of cases the GPU tests run (`CASES`) and `case_statistics`,
so that what makes a case worth running - claims, score ties, argmax ties - is checked for its seed without a GPU
(tests/test_map_flags_host.py)."""
import numpy as np

FILLER_DET = -77           # every word of a det row at or beyond det_count
IOUS = (.5, .3)

# (B, C, max_boxes, max_gt, fractional ground truth, seed); rows = C * max_boxes.  The seeds were chosen on the CPU so that
# `required_statistics` holds at both thresholds of IOUS (tests/test_map_flags_host.py asserts it).
CASES = [
    (3, 2, 3, 5, False, 13),
    (5, 3, 20, 70, False, 1),
    (4, 20, 4, 130, True, 2),
    (6, 5, 8, 64, False, 3),       # max_gt is exactly one 64-lane chunk
    (2, 1, 66, 1, False, 12),      # one class with more rows than a wave
    (2, 80, 20, 40, False, 5),     # rows = 1600
]


def _iou(bbgt, bb):
    """float64 IoU of one box (left, top, right, bottom) against rows (xmin, ymin, xmax, ymax), VOC +1 convention."""
    iw = np.maximum(np.minimum(bbgt[:, 2], bb[2]) - np.maximum(bbgt[:, 0], bb[0]) + 1.0, 0.0)
    ih = np.maximum(np.minimum(bbgt[:, 3], bb[3]) - np.maximum(bbgt[:, 1], bb[1]) + 1.0, 0.0)
    inter = iw * ih
    uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (bbgt[:, 2] - bbgt[:, 0] + 1.0) * (bbgt[:, 3] - bbgt[:, 1] + 1.0) - inter
    return inter / uni


def _walk(det, det_count, gt, gt_count, num_classes, iou):
    det = np.asarray(det, np.int32)
    det_count = np.asarray(det_count).reshape(-1)
    gt_count = np.asarray(gt_count).reshape(-1)
    batch, rows = det.shape[0], det.shape[1]
    flags = np.full((batch, rows), -1, np.int32)
    npos = np.zeros((batch, num_classes), np.int32)
    stats = {'true_positives': 0, 'claimed_false_positives': 0, 'tied_groups': 0, 'argmax_ties': 0}
    for cls in range(num_classes):
        boxes, claimed = {}, {}
        for b in range(batch):
            g = np.asarray(gt[b][:gt_count[b]], np.float64).reshape(-1, 5) if gt_count[b] else np.zeros((0, 5))
            boxes[b] = g[g[:, 4] == cls, :4]
            claimed[b] = np.zeros(boxes[b].shape[0], bool)
            npos[b, cls] = boxes[b].shape[0]
        where, score = [], []
        for b in range(batch):
            group = []
            for r in range(int(det_count[b])):
                if det[b, r, 5] == cls:
                    where.append((b, r))
                    score.append(float(det[b, r, 4:5].view(np.float32)[0]))
                    group.append(score[-1])
            stats['tied_groups'] += len(set(group)) < len(group)
        order = np.argsort(-np.asarray(score, np.float64), kind='stable')
        for j in order:
            b, r = where[j]
            ymin, xmin, ymax, xmax = (float(v) for v in det[b, r, :4])
            verdict = 0
            if boxes[b].shape[0]:
                ov = _iou(boxes[b], (xmin, ymin, xmax, ymax))
                jmax = int(np.argmax(ov))
                if ov[jmax] > iou:
                    stats['argmax_ties'] += int((ov == ov[jmax]).sum() >= 2)
                    if claimed[b][jmax]:
                        stats['claimed_false_positives'] += 1
                    else:
                        claimed[b][jmax] = True
                        verdict = 1
            flags[b, r] = verdict
            stats['true_positives'] += verdict
    return flags, npos, stats


def reference_flags(det, det_count, gt, gt_count, num_classes, iou):
    """NumPy det [B,rows,6] int32 (packed records), det_count [B], gt [B,G,5] float32, gt_count [B] -> (flags [B,rows] int32,
    npos [B,num_classes] int32) as include/yoloret_hip.h defines them for yr_voc_match."""
    return _walk(det, det_count, gt, gt_count, num_classes, iou)[:2]


def case_statistics(det, det_count, gt, gt_count, num_classes, iou):
    """{'true_positives', 'claimed_false_positives' (best box above the threshold but already taken), 'tied_groups' ((image, class)
    groups containing equal scores), 'argmax_ties' (detections whose best IoU, above the threshold, is reached by two or more
    ground-truth boxes)}."""
    return _walk(det, det_count, gt, gt_count, num_classes, iou)[2]


def required_statistics(batch, num_classes, max_gt):
    """What a random case must show to be worth running: 5 true positives, 3 claimed false positives, 3 groups with score ties and
    2 argmax ties - capped by what the shape admits: an image has at most max_gt true positives, there are at most
    batch * num_classes groups, and an argmax tie needs two ground-truth boxes in one image (the shape (2, 1, 66, 1) admits
    2 true positives, 2 groups and no argmax tie)."""
    return {'true_positives': min(5, batch * max_gt), 'claimed_false_positives': 3, 'tied_groups': min(3, batch * num_classes),
            'argmax_ties': 2 if max_gt >= 2 else 0}


def to_host_inputs(det, det_count, gt, gt_count):
    """The same data as the arguments of yolo3.map.evaluate_detections: (pred_res rows [image, class, score, left, top, right,
    bottom] in (image, row) order, true_res {image: [n,5]})."""
    det = np.asarray(det, np.int32)
    pred, true = [], {}
    for b in range(det.shape[0]):
        for r in range(int(det_count[b])):
            ymin, xmin, ymax, xmax = (int(v) for v in det[b, r, :4])
            pred.append([b, int(det[b, r, 5]), det[b, r, 4:5].view(np.float32)[0], xmin, ymin, xmax, ymax])
        true[b] = np.asarray(gt[b][:gt_count[b]], np.float32).reshape(-1, 5)
    return pred, true


def make_det(rows_per_image, rows):
    """[[(ymin, xmin, ymax, xmax, score, class), ...] per image] -> det [B,rows,6] int32 (filler beyond the counts), det_count."""
    det = np.full((len(rows_per_image), rows, 6), FILLER_DET, np.int32)
    cnt = np.zeros(len(rows_per_image), np.int32)
    for b, rs in enumerate(rows_per_image):
        cnt[b] = len(rs)
        for r, (ymin, xmin, ymax, xmax, score, cls) in enumerate(rs):
            det[b, r, :4] = (ymin, xmin, ymax, xmax)
            det[b, r, 4] = np.float32(score).view(np.int32)
            det[b, r, 5] = cls
    return det, cnt


def make_gt(boxes_per_image, max_gt=None):
    """[[(xmin, ymin, xmax, ymax, label), ...] per image] -> gt [B,G,5] float32 (NaN beyond the counts), gt_count."""
    g = max([len(bs) for bs in boxes_per_image] + [1]) if max_gt is None else max_gt
    gt = np.full((len(boxes_per_image), g, 5), np.nan, np.float32)
    cnt = np.zeros(len(boxes_per_image), np.int32)
    for b, bs in enumerate(boxes_per_image):
        cnt[b] = len(bs)
        if len(bs):
            gt[b, :len(bs)] = np.asarray(bs, np.float32).reshape(-1, 5)
    return gt, cnt


def random_case(batch, num_classes, max_boxes, max_gt, fractional, seed):
    """-> det [B, C*max_boxes, 6] int32, det_count [B], gt [B,max_gt,5] float32, gt_count [B].
    Most detections are a jitter by a few pixels of a labelled box of their own class, drawn mostly from a few 'hot' boxes, so
    that boxes are claimed and claimed again; scores are multiples of 1/8 (ties); ground-truth boxes are duplicated (argmax
    ties); labels -1, C and c + 0.5 are mixed in; row order is random; rows beyond the counts hold the fillers."""
    rng = np.random.RandomState(seed)
    rows = num_classes * max_boxes
    dets, gts = [], []
    for b in range(batch):
        ngt = max_gt if b == 0 else int(rng.randint(max_gt // 2, max_gt + 1))
        boxes = []
        for _ in range(ngt):
            if boxes and rng.rand() < .2:
                boxes.append(boxes[rng.randint(len(boxes))])         # a duplicate, label included
                continue
            x, y = rng.randint(0, 300, 2)
            w, h = rng.randint(8, 90, 2)
            box = np.array([x, y, x + w, y + h], np.float64)
            if fractional:
                box = box + np.round(rng.rand(4) * 16) / 16 * np.array([0, 0, 1, 1]) + rng.randint(0, 16) / 16
            label = float(rng.randint(num_classes))
            u = rng.rand()
            if u < .04:
                label = -1.0
            elif u < .08:
                label = float(num_classes)
            elif u < .12:
                label += .5
            boxes.append((box[0], box[1], box[2], box[3], label))
        usable = [bx for bx in boxes if 0 <= bx[4] < num_classes and bx[4] == int(bx[4])]
        hot = usable[:4]
        n = int(rng.randint(rows // 2, rows + 1)) if b else rows
        rs = []
        for _ in range(n):
            score = rng.randint(1, 9) / 8.0
            u = rng.rand()
            if usable and u < .85:
                src = hot[rng.randint(len(hot))] if rng.rand() < .6 else usable[rng.randint(len(usable))]
                j = rng.randint(-3, 4, 4) if rng.rand() < .7 else np.zeros(4, int)
                xmin, ymin = int(src[0]) + j[0], int(src[1]) + j[1]
                xmax, ymax = max(int(src[2]) + j[2], xmin), max(int(src[3]) + j[3], ymin)
                cls = int(src[4])
            else:
                xmin, ymin = rng.randint(0, 300, 2)
                xmax, ymax = xmin + rng.randint(0, 90), ymin + rng.randint(0, 90)
                cls = int(rng.randint(num_classes))
                if u > .97:
                    cls = -1 if rng.rand() < .5 else num_classes
            rs.append((ymin, xmin, ymax, xmax, score, cls))
        dets.append(rs)
        gts.append(boxes)
    det, det_count = make_det(dets, rows)
    gt, gt_count = make_gt(gts, max_gt)
    return det, det_count, gt, gt_count
