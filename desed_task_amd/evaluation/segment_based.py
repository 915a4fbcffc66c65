"""Segment-based evaluation of score tables -- the role of `sed_scores_eval.segment_based` in the 2024 recipe
(recipes/dcase2024_task4_baseline/local/sed_trainer_pretrained.py:693-747 and :1216-1263; third party, absent from the
reference tree and not a dependency of this package, like the other evaluators it restates).  Same call shape:
`best_fscore(scores, ground_truth, audio_durations, segment_length=1.0)` and `auroc(..., max_fpr=None)`, first return value a
dict {event_class: value, "macro_average" | "mean": value}.

Definitions (written from the package's documented behaviour; its exact conventions cannot be checked offline):
  * a clip of duration d has ceil(d / L) segments, segment k = [k L, min((k + 1) L, d));
  * segment k is positive for class c when a ground-truth c event overlaps it with positive length;
  * the score of segment k is the maximum of the score rows that overlap it with positive length (0 when none does) -- the
    reduction of `sed_segment_scores` mode 1.  A table already at segment resolution (one row per segment, the overlap-added
    MAESTRO tables of the test path) therefore passes through unchanged;
  * `best_fscore`: per class, the largest F1 over the thresholds at the distinct segment scores, detection = score >= threshold;
    the returned threshold is the highest one that reaches it.  A class without a positive segment scores 0.  Macro = mean.
  * `auroc`: per class ROC AUC, tied scores counted half (trapezoids over the distinct thresholds).  With `max_fpr` the area for
    FPR <= max_fpr, the ROC linearly interpolated at max_fpr, divided by max_fpr (a READING of the package's normalisation);
    `mcclish_correction=True` gives sklearn's standardised partial AUC instead.  A class without positive or without negative
    segments is NaN and left out of "mean".
"""
import math

import numpy as np


def _table(df):
    """(timestamps (n + 1), event classes, scores (n, NC)) of a score table (onset, offset, classes...)."""
    classes = [c for c in df.columns if c not in ("onset", "offset")]
    on, off = df["onset"].to_numpy(np.float64), df["offset"].to_numpy(np.float64)
    ts = np.concatenate([on, off[-1:]])
    return ts, classes, df[classes].to_numpy(np.float64)


def segment_max(ts, arr, duration, segment_length=1.0):
    """(ceil(duration / L), NC) segment scores: the maximum of the rows overlapping each segment with positive length."""
    n_seg = math.ceil(duration / segment_length)
    on = np.arange(n_seg) * segment_length
    off = np.minimum(on + segment_length, duration)
    lo = np.searchsorted(ts[1:], on, side="right")            # first row with end > segment onset
    hi = np.searchsorted(ts[:-1], off, side="left")           # rows starting before the segment end
    out = np.zeros((n_seg, arr.shape[1]))
    for k in range(n_seg):
        if hi[k] > lo[k]:
            out[k] = arr[lo[k]:hi[k]].max(0)
    return out


def segment_targets(events, duration, event_classes, segment_length=1.0):
    """(ceil(duration / L), NC) bool: segment k positive for class c when a c event overlaps it with positive length."""
    n_seg = math.ceil(duration / segment_length)
    on = np.arange(n_seg) * segment_length
    off = np.minimum(on + segment_length, duration)
    col = {c: i for i, c in enumerate(event_classes)}
    y = np.zeros((n_seg, len(event_classes)), dtype=bool)
    for ev_on, ev_off, label in events:
        if label in col:
            y[:, col[label]] |= (ev_on < off) & (ev_off > on)
    return y


def segment_scores_and_targets(scores, ground_truth, audio_durations, segment_length=1.0):
    """-> (event classes, scores (n_segments_total, NC), targets (n_segments_total, NC)) over the clips of `scores`."""
    classes, s_all, y_all = None, [], []
    for clip_id, df in scores.items():
        ts, cls, arr = _table(df)
        if classes is None:
            classes = cls
        elif cls != classes:
            raise ValueError("score tables disagree on the event classes")
        dur = float(audio_durations[clip_id])
        s_all.append(segment_max(ts, arr, dur, segment_length))
        y_all.append(segment_targets(ground_truth[clip_id], dur, classes, segment_length))
    if classes is None:
        raise ValueError("no score tables")
    return classes, np.concatenate(s_all), np.concatenate(y_all)


def _counts(s, y):
    """Distinct thresholds in descending order and the (tp, fp) counts of `score >= threshold` at each."""
    order = np.argsort(-s, kind="mergesort")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]       # last index of every group of equal scores
    tp = np.cumsum(y)[last]
    fp = np.cumsum(~y)[last]
    return s[last], tp, fp


def best_fscore(scores, ground_truth, audio_durations, segment_length=1.0):
    """-> (f, precision, recall, thresholds, stats): per class and "macro_average" (the mean over classes)."""
    return best_fscore_of_segments(*segment_scores_and_targets(scores, ground_truth, audio_durations, segment_length))


def best_fscore_of_segments(classes, s, y):
    """best_fscore on the output of segment_scores_and_targets."""
    f, p, r, thr, stats = {}, {}, {}, {}, {}
    for i, c in enumerate(classes):
        n_pos = int(y[:, i].sum())
        th, tp, fp = _counts(s[:, i], y[:, i])
        f1 = 2 * tp / np.maximum(tp + fp + n_pos, 1)
        j = int(np.argmax(f1))
        f[c] = float(f1[j]) if n_pos > 0 else 0.0
        p[c] = float(tp[j] / max(tp[j] + fp[j], 1))
        r[c] = float(tp[j] / n_pos) if n_pos > 0 else 0.0
        thr[c] = float(th[j])
        stats[c] = {"tps": int(tp[j]), "fps": int(fp[j]), "n_ref": n_pos}
    for d in (f, p, r):
        d["macro_average"] = float(np.mean([d[c] for c in classes]))
    return f, p, r, thr, stats


def _roc(s, y):
    th, tp, fp = _counts(s, y)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    tpr = np.r_[0.0, tp / max(n_pos, 1)]
    fpr = np.r_[0.0, fp / max(n_neg, 1)]
    return fpr, tpr, np.r_[np.inf, th], n_pos, n_neg


def _area(fpr, tpr, max_fpr, mcclish_correction):
    if max_fpr is None or max_fpr >= 1:
        return float(np.trapezoid(tpr, fpr))
    stop = int(np.searchsorted(fpr, max_fpr, side="right"))
    x = np.r_[fpr[:stop], max_fpr]
    yv = np.r_[tpr[:stop], np.interp(max_fpr, fpr[stop - 1:stop + 1], tpr[stop - 1:stop + 1])]
    area = float(np.trapezoid(yv, x))
    if mcclish_correction:
        min_area, max_area = 0.5 * max_fpr ** 2, max_fpr
        return 0.5 * (1 + (area - min_area) / (max_area - min_area))
    return area / max_fpr


def auroc(scores, ground_truth, audio_durations, segment_length=1.0, max_fpr=None, mcclish_correction=False):
    """-> (auc, roc_curves): auc per class and "mean" (over the classes with a defined value); roc_curves per class
    (fpr, tpr, thresholds)."""
    return auroc_of_segments(*segment_scores_and_targets(scores, ground_truth, audio_durations, segment_length), max_fpr=max_fpr,
                             mcclish_correction=mcclish_correction)


def auroc_of_segments(classes, s, y, max_fpr=None, mcclish_correction=False):
    """auroc on the output of segment_scores_and_targets."""
    auc, curves = {}, {}
    for i, c in enumerate(classes):
        fpr, tpr, th, n_pos, n_neg = _roc(s[:, i], y[:, i])
        curves[c] = (fpr, tpr, th)
        auc[c] = _area(fpr, tpr, max_fpr, mcclish_correction) if n_pos > 0 and n_neg > 0 else float("nan")
    vals = [auc[c] for c in classes if not np.isnan(auc[c])]
    auc["mean"] = float(np.mean(vals)) if vals else float("nan")
    return auc, curves
