"""AP and Boundary AP of one-record-per-image instance results in plain-loop Python, restated from COCOeval's published algorithm for
this task's shape: one label instance and at most one record an image (train.InstanceAPMeter; unpinned: the reference has no instance
metric).  tests/test_instance_eval.py holds this file to hand-derived answers first.  Not a test module.

A row is (cat, score, area, cls_label, pair): the record's class, score and area, the label's class, and the six counters
(|p&g|, |p|, |g|, |bp&bg|, |bp|, |bg|).  Rows come in insertion order."""
import math

THRESHOLDS = [50 + 5 * j for j in range(10)]             # in hundredths: t = (50 + 5 j) / 100


def passes(n, a, b, t100):
    """IoU = n / (a + b - n) >= t100 / 100 in integers; a measure whose union is 0 is 0 and passes nothing."""
    u = a + b - n
    return u > 0 and 100 * n >= t100 * u


def is_tp(row, k, t100, boundary):
    cat, score, area, cls, pair = row
    if pair[2] <= 0 or cls != k:                         # no label instance, or one of another class
        return False
    if not passes(pair[0], pair[1], pair[2], t100):
        return False
    return passes(pair[3], pair[4], pair[5], t100) if boundary else True


def rank_key(score):
    return -math.inf if math.isnan(score) else score     # a NaN score ranks last


def ap_one(rows, k, t100, boundary):
    """AP of class k at one threshold, or None where no label instance has class k."""
    n_gt = 0
    for row in rows:
        if row[4][2] > 0 and row[3] == k:
            n_gt += 1
    if n_gt == 0:
        return None
    recs = [row for row in rows if row[2] > 0 and row[0] == k]
    # descending score, ties in insertion order: an insertion sort that never passes an equal key
    ranked = []
    for row in recs:
        at = len(ranked)
        while at > 0 and rank_key(ranked[at - 1][1]) < rank_key(row[1]):
            at -= 1
        ranked.insert(at, row)
    tp, fp, cum_tp, prec = 0, 0, [], []
    for row in ranked:
        if is_tp(row, k, t100, boundary):
            tp += 1
        else:
            fp += 1
        cum_tp.append(tp)
        prec.append(tp / (tp + fp))
    for i in range(len(prec) - 2, -1, -1):               # non-increasing from the right
        if prec[i] < prec[i + 1]:
            prec[i] = prec[i + 1]
    samples = []
    for q in range(101):                                 # recall q / 100: the first rank with cum_tp / n_gt >= q / 100, in integers
        at = 0
        while at < len(cum_tp) and 100 * cum_tp[at] < q * n_gt:
            at += 1
        samples.append(prec[at] if at < len(prec) else 0.0)
    return math.fsum(samples) / 101


def mean(vals):
    return math.fsum(vals) / len(vals) if vals else float("nan")


def evaluate(rows, num_class):
    rows = [(int(c), float(s), int(a), int(l), [int(v) for v in p]) for c, s, a, l, p in rows]
    res = {}
    for boundary, name in ((False, "AP"), (True, "bAP")):
        table = {}                                       # (k, t100) -> AP
        for k in range(num_class):
            for t in THRESHOLDS:
                v = ap_one(rows, k, t, boundary)
                if v is not None:
                    table[(k, t)] = v
        res[name] = mean([v for (k, t), v in sorted(table.items())])
        res[name + "50"] = mean([v for (k, t), v in sorted(table.items()) if t == 50])
        res[name + "75"] = mean([v for (k, t), v in sorted(table.items()) if t == 75])
    ious, bious = [], []
    for row in rows:
        n, a, b, bn, ba, bb = row[4]
        if b > 0:
            u, bu = a + b - n, ba + bb - bn
            ious.append(n / u if u > 0 else 0.0)
            bious.append(bn / bu if bu > 0 else 0.0)
    res["mIoU"], res["mBIoU"] = mean(ious), mean(bious)
    res["n_images"] = len(rows)
    res["n_records"] = sum(1 for row in rows if row[2] > 0)
    res["cls_acc"] = mean([1.0 if row[0] == row[3] else 0.0 for row in rows])
    return res
