"""Collar (event-based), segment-based and intersection-based F1 with the per-clip work on the device (csrc/sed_f1.hip,
`sed_f1_counts`): the opt-in counterpart of evaluation_measures.log_sedeval_metrics and compute_per_intersection_macro_f1, which
stay the default and the yardstick.

The host evaluators decode every clip into a pandas frame of events and then walk (file, class) pairs in Python.  Here the
median-filtered scores stay in a psds_device.ScoreBuffer; `DecodedScores(buffer, threshold)` stands for the frame that
`batched_decode_preds` would have built at that threshold, and one kernel launch counts, per (threshold, clip, class), the eight
integers the F scores are made of (include/sed_hip.h).  The sums over clips are torch reductions on the scores' device; from the
per-class sums on, the scores come out of the host classes' own formulas (`sed_eval_metrics._f_measure` / `_nanmean`,
`PSDSEval._macro_f_tail`), so equal integers give equal values.

Who is counted follows the host: sed_eval walks the files of the reference table (a scored clip that is not listed is ignored, a
listed file that was never scored adds its reference counts and no detections); PSDSEval counts detections in every file that has
a duration and ground truth from the whole table.  Limits of the kernel: T <= 256 frames, <= 32 classes, <= 8 thresholds, at most
SED_F1_MAX_EVENTS ground-truth events per (clip, class) and SED_F1_MAX_CELLS raster cells; beyond them the call raises, there is
no host fallback.
"""
import math
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from .. import _lib
from .psds import PSDSEval
from .psds_device import ScoreBuffer, _event_table, _event_table_on, _score_columns
from .sed_eval_metrics import _f_measure, _nanmean

_LIMITS = _lib.header_constants()
MAX_EVENTS, MAX_CELLS, MAX_THR = _LIMITS["SED_F1_MAX_EVENTS"], _LIMITS["SED_F1_MAX_CELLS"], _LIMITS["SED_F1_MAX_THR"]
FIELDS = ("n_sys", "collar_tp", "seg_ref", "seg_sys", "seg_tp", "int_tp", "int_fp", "reserved")


class DecodedScores:
    """A ScoreBuffer seen at one decision threshold: what `batched_decode_preds(..., thresholds=[threshold])` returns as
    `prediction_dfs[threshold]` for the same clips, without building it.  `classes` selects score columns by name and `ids` clips
    (default: all of the buffer's, in insertion order): the 2024 recipe scores the DESED columns of the DESED clips."""

    def __init__(self, buffer, threshold, classes=None, ids=None):
        if not isinstance(buffer, ScoreBuffer):
            raise TypeError("DecodedScores wraps a psds_device.ScoreBuffer")
        self.buffer, self.threshold = buffer, float(threshold)
        self.classes = None if classes is None else list(classes)
        self.ids = None if ids is None else list(ids)
        missing = [a for a in self.ids or [] if a not in buffer]
        if missing:
            raise ValueError("clips without scores: %s" % missing[:3])

    def clip_ids(self):
        return list(self.buffer) if self.ids is None else list(self.ids)

    def _scores(self):
        """-> (ids, class names, (N, T, NC) device scores) of the clips."""
        ids = self.clip_ids()
        return (ids,) + _score_columns(self.buffer, ids, self.classes)

    @property
    def empty(self):
        """True when no clip has a run of `score > threshold` (the frame would have no rows)."""
        if not self.clip_ids():
            return True
        _, _, scores = self._scores()
        return not bool((scores > torch.tensor(self.threshold, dtype=torch.float32, device=scores.device)).any())

    def to_dataframe(self):
        """The event_label / onset / offset / filename frame of `batched_decode_preds`: id + ".wav", clip-major in insertion order,
        then class-major, then time order."""
        from ..postprocess import threshold_events
        cols = ["event_label", "onset", "offset", "filename"]
        if not self.clip_ids():
            return pd.DataFrame({c: [] for c in cols}, columns=cols)
        ids, classes, scores = self._scores()
        counts, events = threshold_events(scores, [self.threshold])
        valid = np.arange(events.shape[3])[None, None, :] < counts[0][..., None]
        j, c, e = np.nonzero(valid)
        ts = np.asarray(self.buffer.timestamps, dtype=np.float64)
        return pd.DataFrame({"event_label": np.asarray(classes, dtype=object)[c], "onset": ts[events[0, j, c, e, 0]],
                             "offset": ts[events[0, j, c, e, 1]],
                             "filename": np.asarray([a + ".wav" for a in ids], dtype=object)[j]}, columns=cols)


def f1_counts_kernel(scores, thr, ts, ev_ptr, ev_on, ev_off, clip_dur, t_collar, percentage_of_length, time_resolution, dtc, gtc,
                     cttc, out=None):
    """The kernel: scores (N, T, NC) fp32, thr (n_thr) fp32, ts (T + 1) / ev_on / ev_off / clip_dur float64, ev_ptr (N * NC + 1)
    int32, all on the device -> counts (n_thr, N, NC, 8) int32.  `out`: the tensor to write into (tests)."""
    _lib.check_tensor(scores, "scores")
    N, T, NC = scores.shape
    if out is None:
        out = torch.empty(thr.numel(), N, NC, 8, dtype=torch.int32, device=scores.device)
    _lib.get().call("sed_f1_counts", scores.data_ptr(), thr.data_ptr(), ts.data_ptr(), ev_ptr.data_ptr(), ev_on.data_ptr(),
                    ev_off.data_ptr(), clip_dur.data_ptr(), N, T, NC, thr.numel(), float(t_collar), float(percentage_of_length),
                    float(time_resolution), float(dtc), float(gtc), float(cttc), out.data_ptr(), _lib.stream_ptr(scores))
    return out


def f1_counts(buffer, thresholds, ground_truth, audio_durations, classes=None, t_collar=0.2, percentage_of_length=0.2,
              time_resolution=1.0, dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3, ids=None):
    """One launch (per SED_F1_MAX_THR thresholds) over the clips `ids` of `buffer` (default: all, in insertion order).
    ground_truth {audio_id: [(onset, offset, label), ...]} and audio_durations {audio_id: seconds} may list other clips and miss
    some: a clip without ground truth has no events, a clip without a duration cannot have false positives.  -> dict: `counts`
    (n_thr, N, NC, 8) int32 on the device (the fields: FIELDS), `ids`, `classes`, and `sums`, the per-class int64 sums over clips
    as numpy (n_thr, NC, 8): fields 0-4 over the clips listed in `ground_truth`, fields 5-6 over the clips with a duration,
    field 7 = the runs of all evaluated clips."""
    ids = list(buffer) if ids is None else list(ids)
    if not ids:
        raise ValueError("no clips to evaluate")
    thresholds = [float(t) for t in thresholds]
    classes, scores = _score_columns(buffer, ids, classes)
    dev = scores.device
    table = _event_table({a: ground_truth.get(a, []) for a in ids}, ids, classes)
    if len(table["ptr"]) > 1 and int(np.diff(table["ptr"]).max()) > MAX_EVENTS:
        raise ValueError("more than %d ground-truth events of one class in one clip" % MAX_EVENTS)
    last = max(float(buffer.timestamps[-1]), float(table["off"].max()) if len(table["off"]) else 0.0)
    if math.ceil(last / time_resolution) > MAX_CELLS or (len(table["on"]) and float(table["on"].min()) < 0.0):
        raise ValueError("the clips span more than %d segments of %g s (or an event starts before 0)" % (MAX_CELLS, time_resolution))
    ev_ptr, ev_on, ev_off = _event_table_on(table, dev)
    listed = np.array([a in ground_truth for a in ids])
    timed = np.array([a in audio_durations for a in ids])
    durs = np.array([float(audio_durations[a]) if a in audio_durations else 0.0 for a in ids], dtype=np.float64)
    ts = torch.from_numpy(np.ascontiguousarray(buffer.timestamps, dtype=np.float64)).to(dev)
    thr, durs_dev = torch.tensor(thresholds, dtype=torch.float32, device=dev), torch.from_numpy(durs).to(dev)
    counts = torch.empty(len(thresholds), len(ids), len(classes), 8, dtype=torch.int32, device=dev)
    for k in range(0, len(thresholds), MAX_THR):                  # one launch serves MAX_THR thresholds: the recipes pass 1 to 3
        f1_counts_kernel(scores, thr[k:k + MAX_THR], ts, ev_ptr, ev_on, ev_off, durs_dev, t_collar, percentage_of_length,
                         time_resolution, dtc_threshold, gtc_threshold, cttc_threshold, out=counts[k:k + MAX_THR])
    mask = torch.from_numpy(np.stack([listed] * 5 + [timed] * 2 + [np.ones(len(ids), dtype=bool)], 1)).to(dev)      # (N, 8)
    src = torch.cat((counts[..., :7], counts[..., :1]), -1).to(torch.int64)
    sums = (src * mask[None, :, None, :]).sum(1)
    return {"counts": counts, "ids": ids, "classes": classes, "sums": sums.cpu().numpy()}


def _table(ground_truth):
    return ground_truth if isinstance(ground_truth, pd.DataFrame) else pd.read_csv(ground_truth, sep="\t")


def _events_by_id(gt):
    """{audio_id: [(onset, offset, label), ...]} in table order for the files named <audio_id>.wav (the names `DecodedScores` gives
    its clips), rows without a label dropped; plus the names of every file of the table, rows without a label included."""
    out = {}
    for f, on, off, lab in zip(gt["filename"], gt["onset"], gt["offset"], gt["event_label"]):
        f = str(f)
        events = out.setdefault(f, [])
        if not pd.isna(lab):
            events.append((float(on), float(off), lab))
    by_id = {f[:-4]: ev for f, ev in out.items() if f.endswith(".wav") and Path(f).name == f}
    return by_id, out


def sedeval_f1(predictions, ground_truth, t_collar=0.2, percentage_of_length=0.2, time_resolution=1.0):
    """log_sedeval_metrics on a DecodedScores: (event macro-F1, event micro-F1, segment macro-F1, segment micro-F1) over the files
    of `ground_truth` (a TSV path or the table)."""
    if predictions.empty:
        return 0.0, 0.0, 0.0, 0.0
    by_id, by_file = _events_by_id(_table(ground_truth))
    res = f1_counts(predictions.buffer, [predictions.threshold], by_id, {}, classes=predictions.classes, t_collar=t_collar,
                    percentage_of_length=percentage_of_length, time_resolution=time_resolution, ids=predictions.ids)
    classes, sums = res["classes"], res["sums"][0]
    cidx = {c: i for i, c in enumerate(classes)}
    n_ref, seg_ref_unscored = np.zeros(len(classes)), np.zeros(len(classes))
    scored = {a + ".wav" for a in res["ids"]}
    ref_labels = set()
    for f, events in by_file.items():
        cells = {}
        for on, off, lab in events:
            ref_labels.add(lab)
            if lab not in cidx:
                raise ValueError("ground-truth label %r has no score column" % (lab,))
            n_ref[cidx[lab]] += 1
            if f not in scored:              # a listed file that was never scored: its reference raster, no detections
                cells.setdefault(lab, set()).update(range(int(math.floor(on * 1 / time_resolution)),
                                                          int(math.ceil(off * 1 / time_resolution))))
        for lab, s in cells.items():
            seg_ref_unscored[cidx[lab]] += len(s)
    # the class list of evaluation_measures._classes: reference labels and detected labels (of any clip), sorted
    labels = sorted(ref_labels | {c for c in classes if sums[cidx[c], 7] > 0})
    sel = [cidx[c] for c in labels]
    ev = {k: sums[sel, i].astype(np.float64) for k, i in (("Nsys", 0), ("Ntp", 1))}
    ev["Nref"] = n_ref[sel]
    seg = {"Nref": sums[sel, 2] + seg_ref_unscored[sel], "Nsys": sums[sel, 3].astype(np.float64), "Ntp": sums[sel, 4].astype(np.float64)}
    out = []
    for m, handling in ((ev, "zero_score"), (seg, None)):
        macro = _nanmean([_f_measure(float(m["Ntp"][i]), float(m["Nref"][i]), float(m["Nsys"][i]), handling)["f_measure"]
                          for i in range(len(labels))]) if labels else float("nan")
        micro = _f_measure(float(m["Ntp"].sum()), float(m["Nref"].sum()), float(m["Nsys"].sum()), handling)["f_measure"]
        out += [macro, micro]
    return tuple(out)


def intersection_macro_f1(prediction_dfs, ground_truth, durations, dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3):
    """compute_per_intersection_macro_f1 on {threshold key: DecodedScores}, all of one ScoreBuffer: the mean over the thresholds of
    the intersection-based macro F1.  `ground_truth` / `durations`: TSV paths or the tables."""
    decoded = list(prediction_dfs.values())
    if not decoded:
        return np.mean([])
    if any(not isinstance(d, DecodedScores) or d.buffer is not decoded[0].buffer or d.classes != decoded[0].classes
           or d.ids != decoded[0].ids for d in decoded):
        raise ValueError("the DecodedScores of one call must share one ScoreBuffer and one selection of classes and clips")
    psds = PSDSEval(ground_truth=_table(ground_truth), metadata=_table(durations), dtc_threshold=dtc_threshold,
                    gtc_threshold=gtc_threshold, cttc_threshold=cttc_threshold)
    buffer = decoded[0].buffer
    if not decoded[0].clip_ids():
        return np.mean([0 for _ in decoded])
    by_id, _ = _events_by_id(psds.ground_truth)
    dur = {f[:-4]: float(d) for f, d in zip(psds.metadata.filename, psds._file_dur) if str(f).endswith(".wav") and Path(f).name == f}
    res = f1_counts(buffer, [d.threshold for d in decoded], by_id, dur, classes=decoded[0].classes, dtc_threshold=dtc_threshold,
                    gtc_threshold=gtc_threshold, cttc_threshold=cttc_threshold, ids=decoded[0].ids)
    names = psds.class_names[:-1]
    # a class annotated only in files that were never scored may have no score column: no detections, so no counts
    sel = [res["classes"].index(c) if c in res["classes"] else -1 for c in names]
    have = np.array([i >= 0 for i in sel])
    values = []
    for k in range(len(decoded)):
        sums = res["sums"][k]
        if sums[:, 7].sum() == 0:                       # an empty frame: the host skips the evaluation
            values.append(0)
            continue
        tp, fp = (np.where(have, sums[sel, i], 0).astype(np.float64) for i in (5, 6))
        with np.errstate(divide="ignore", invalid="ignore"):
            tpr = tp / psds._n_gt[:-1]
        f1, _ = PSDSEval._macro_f_tail(tp, fp, tpr, names)
        values.append(0.0 if np.isnan(f1) else f1)
    return np.mean(values)
