"""Threshold-free PSDS with the per-clip work on the device (csrc/sed_psds.hip, `sed_psds_steps`): the opt-in counterpart of
psds_scores.psds_from_scores, which stays the yardstick.

The host evaluator walks (clip, class) pairs in Python; what it computes per pair -- the distinct scores and the true-positive,
false-positive and cross-trigger counts as step functions of the threshold (`_clip_class_steps`) -- is independent across pairs and
is one workgroup each here.  The filtered scores never leave the device: `postprocess.batched_decode_preds(device_scores=<a
ScoreBuffer>)` appends them where it would build one pandas table per clip.  Merging the per-clip jumps into data-set level counts
is a sort and an integer cumulative sum per class (torch, on the scores' device); from the counts on, the PSD-ROC, the effective
TPR and the area are psds_scores._psd_roc_tail -- the same code as the host path.

Counts are integers, so the two paths differ only where an overlap sits within rounding of its threshold (the kernel takes
overlaps as closed-form interval intersections, the host sums them frame by frame); away from such ties the results are equal.
Limits of the kernel: T <= 256 frames, <= 32 classes, one clip length per buffer; beyond them the call raises, there is no host
fallback.
"""
import numpy as np
import torch

from .. import _lib
from .psds import PSDSEval
from .psds_scores import _psd_roc_tail


class ScoreBuffer:
    """Post-processed scores of many clips, kept on the device: what the `{audio_id: DataFrame}` score-table dicts hold on the host.
    One frame count and one class list per buffer."""

    def __init__(self, event_classes=None, timestamps=None):
        self.event_classes = None if event_classes is None else list(event_classes)
        self.timestamps = None if timestamps is None else np.asarray(timestamps, dtype=np.float64)
        self._chunks = []
        self._where = {}                     # audio_id -> (chunk, row); a later append of the same id wins, like dict.update
        self._cat = None

    def __len__(self):
        return len(self._where)

    def __iter__(self):
        return iter(self._where)

    def __contains__(self, audio_id):
        return audio_id in self._where

    def append(self, scores_btc, audio_ids, timestamps=None, event_classes=None):
        """scores_btc (B, T, NC) fp32 on the device (postprocess._btc layout), one audio id per row.  `timestamps` (T + 1 frame
        boundaries) and `event_classes` are taken on the first call that gives them and must not change afterwards."""
        _lib.check_tensor(scores_btc, "scores")
        if scores_btc.dim() != 3 or scores_btc.dtype != torch.float32:
            raise ValueError("scores must be (clips, frames, classes) float32")
        audio_ids = list(audio_ids)
        if len(audio_ids) != scores_btc.shape[0]:
            raise ValueError("one audio id per clip")
        if timestamps is not None:
            timestamps = np.asarray(timestamps, dtype=np.float64)
            if self.timestamps is None:
                self.timestamps = timestamps
            elif not np.array_equal(self.timestamps, timestamps):
                raise ValueError("a ScoreBuffer holds clips of one length: the frame boundaries changed")
        if event_classes is not None:
            if self.event_classes is None:
                self.event_classes = list(event_classes)
            elif self.event_classes != list(event_classes):
                raise ValueError("a ScoreBuffer holds one class list")
        if self._chunks and tuple(self._chunks[0].shape[1:]) != tuple(scores_btc.shape[1:]):
            raise ValueError("a ScoreBuffer holds one (frames, classes) shape: got %s after %s"
                             % (tuple(scores_btc.shape[1:]), tuple(self._chunks[0].shape[1:])))
        if self.timestamps is not None and len(self.timestamps) != scores_btc.shape[1] + 1:
            raise ValueError("scores must have n_frames + 1 timestamps")
        if self.event_classes is not None and len(self.event_classes) != scores_btc.shape[2]:
            raise ValueError("scores must have one column per event class")
        if not audio_ids:
            return
        self._chunks.append(scores_btc.detach().clone())     # (a copy: the caller's tensor may be a view of a reused output buffer)
        k = len(self._chunks) - 1
        for j, a in enumerate(audio_ids):
            self._where[a] = (k, j)
        self._cat = None

    def rows(self, audio_ids):
        """(len(audio_ids), T, NC) contiguous device tensor of the given clips, in that order."""
        if not self._chunks:
            raise ValueError("the ScoreBuffer is empty")
        if self._cat is None:
            self._cat = (self._chunks[0] if len(self._chunks) == 1 else torch.cat(self._chunks, 0),
                         np.concatenate(([0], np.cumsum([c.shape[0] for c in self._chunks]))))
        cat, start = self._cat
        idx = [int(start[k]) + j for k, j in (self._where[a] for a in audio_ids)]
        return cat.index_select(0, torch.tensor(idx, dtype=torch.long, device=cat.device)).contiguous()

    def to_tables(self):
        """{audio_id: DataFrame(onset, offset, <classes>)}: the tables `create_score_dataframe` builds from the same scores."""
        from ..postprocess import create_score_dataframe
        if self.timestamps is None or self.event_classes is None:
            raise ValueError("the ScoreBuffer has no timestamps / event classes")
        ids = list(self._where)
        if not ids:
            return {}
        host = self.rows(ids).cpu().numpy()
        return {a: create_score_dataframe(host[j], self.timestamps, self.event_classes) for j, a in enumerate(ids)}


_EVENT_TABLES = {}        # (classes, ((audio_id, events), ...)) -> host table; a handful of ground truths per run
_EVENT_TABLES_MAX = 8


def _event_table(ground_truth, ids, classes):
    """CSR table of the ground truth, ordered by (clip, class) and inside a class in the order of the ground-truth list, with the
    per-class event counts and durations accumulated in the host path's order.  Built once per (ground truth, id order)."""
    key = (tuple(classes), tuple((a, tuple((float(o), float(f), l) for o, f, l in ground_truth[a])) for a in ids))
    hit = _EVENT_TABLES.get(key)
    if hit is not None:
        return hit
    nc = len(classes)
    cidx = {c: i for i, c in enumerate(classes)}
    n_gt, gt_dur = np.zeros(nc), np.zeros(nc)
    ptr = np.zeros(len(ids) * nc + 1, dtype=np.int64)
    on, off = [], []
    for n, (_, events) in enumerate(key[1]):
        per_class = [[] for _ in range(nc)]
        for o, f, l in events:
            if l not in cidx:
                raise ValueError("ground-truth label %r has no score column" % (l,))
            per_class[cidx[l]].append((o, f))
            n_gt[cidx[l]] += 1
            gt_dur[cidx[l]] += f - o
        for c in range(nc):
            for o, f in per_class[c]:
                on.append(o)
                off.append(f)
            ptr[n * nc + c + 1] = len(on)
    if len(on) >= 2 ** 31:
        raise ValueError("too many ground-truth events")
    table = {"ptr": ptr.astype(np.int32), "on": np.asarray(on, dtype=np.float64), "off": np.asarray(off, dtype=np.float64),
             "n_gt": n_gt, "gt_dur": gt_dur, "dev": {}}
    if len(_EVENT_TABLES) >= _EVENT_TABLES_MAX:
        _EVENT_TABLES.pop(next(iter(_EVENT_TABLES)))
    _EVENT_TABLES[key] = table
    return table


def _event_table_on(table, device):
    key = str(device)
    if key not in table["dev"]:
        table["dev"][key] = tuple(torch.from_numpy(table[k]).to(device) for k in ("ptr", "on", "off"))
    return table["dev"][key]


def _score_columns(buffer, ids, classes):
    """-> (class names, (len(ids), T, NC) contiguous device scores) of the clips `ids`: all columns of the buffer, or the columns
    `classes` names, in that order.  NaN scores are refused."""
    if buffer.event_classes is None or buffer.timestamps is None:
        raise ValueError("the ScoreBuffer has no timestamps / event classes")
    scores = buffer.rows(ids)
    if classes is None:
        classes = list(buffer.event_classes)
    else:
        classes = list(classes)
        unknown = [c for c in classes if c not in buffer.event_classes]
        if unknown:
            raise ValueError("classes without a score column: %s" % unknown[:3])
        cols = torch.tensor([buffer.event_classes.index(c) for c in classes], dtype=torch.long, device=scores.device)
        scores = scores.index_select(2, cols).contiguous()
    if bool(torch.isnan(scores).any()):
        raise ValueError("the scores hold NaN")
    return classes, scores


def psds_steps(scores, ts, ev_ptr, ev_on, ev_off, clip_dur, dtc, gtc, cttc, count_ct, out=None):
    """The kernel: scores (N, T, NC) fp32, ts (T + 1) / ev_on / ev_off / clip_dur float64, ev_ptr (N * NC + 1) int32, all on the
    device.  cttc None: no cross-trigger threshold.  -> dict of device tensors n_u, tp0, fp0 (N, NC) int32, u (N, NC, T) fp32, dtp,
    dfp (N, NC, T) int32 and, with count_ct, ct0 (N, NC, NC), dct (N, NC, T, NC) int32.  `out`: tensors to write into (tests)."""
    _lib.check_tensor(scores, "scores")
    N, T, NC = scores.shape
    dev = scores.device
    if out is None:
        i32 = dict(dtype=torch.int32, device=dev)
        out = {"n_u": torch.empty(N, NC, **i32), "u": torch.empty(N, NC, T, dtype=torch.float32, device=dev),
               "tp0": torch.empty(N, NC, **i32), "fp0": torch.empty(N, NC, **i32),
               "dtp": torch.empty(N, NC, T, **i32), "dfp": torch.empty(N, NC, T, **i32)}
        if count_ct:
            out["ct0"] = torch.empty(N, NC, NC, **i32)
            out["dct"] = torch.empty(N, NC, T, NC, **i32)
    ptr = lambda k: out[k].data_ptr() if k in out else None      # noqa: E731
    _lib.get().call("sed_psds_steps", scores.data_ptr(), ts.data_ptr(), ev_ptr.data_ptr(), ev_on.data_ptr(), ev_off.data_ptr(),
                    clip_dur.data_ptr(), N, T, NC, float(dtc), float(gtc), 0.0 if cttc is None else float(cttc),
                    1 if cttc is None else 0, 1 if count_ct else 0, ptr("n_u"), ptr("u"), ptr("tp0"), ptr("fp0"), ptr("ct0"),
                    ptr("dtp"), ptr("dfp"), ptr("dct"), _lib.stream_ptr(scores))
    return out


def _merged_counts(steps, c, use_ct):
    """Data-set level counts of class c from the per-clip jumps: (tp, fp, ctc) float64 numpy, row 0 = threshold below all scores,
    then the operating point after ALL jumps at each distinct score value, ascending."""
    n_u = steps["n_u"][:, c]                                           # (N)
    N, _, T = steps["u"].shape
    live = (torch.arange(T, device=n_u.device)[None, :] < n_u[:, None]).reshape(-1).nonzero().squeeze(1)
    thr = steps["u"][:, c].reshape(-1)[live]                           # clip order, ascending inside a clip: the host's concatenation
    thr, order = torch.sort(thr, stable=True)
    sel = live[order]                                                  # flat (clip, jump) positions in threshold order
    last = torch.ones(thr.numel(), dtype=torch.bool, device=thr.device)
    if thr.numel() > 1:
        last[:-1] = thr[1:] != thr[:-1]
    last = last.nonzero().squeeze(1)
    narrow = torch.int32 if N * T < 2 ** 31 else torch.int64           # a count never exceeds the number of runs: halves the copy

    def counts(base, jumps):
        """base () or (classes), jumps (N * T) or (N * T, classes) -> (points + 1) or (points + 1, classes)."""
        j = jumps[sel]
        if j.dim() == 2:
            j = j.t().contiguous()                                     # scan along the contiguous axis
        run = torch.cumsum(j, -1, dtype=torch.int64)[..., last] + base.to(torch.int64)[..., None]
        run = torch.cat((base.to(torch.int64)[..., None], run), -1).to(narrow)
        if run.dim() == 2:
            run = run.t().contiguous()                                 # (points + 1, classes), C order like the host path's
        return run.cpu().numpy().astype(np.float64)

    tp = counts(steps["tp0"][:, c].sum(), steps["dtp"][:, c].reshape(-1))
    fp = counts(steps["fp0"][:, c].sum(), steps["dfp"][:, c].reshape(-1))
    ctc = None
    if use_ct:
        nc = steps["ct0"].shape[2]
        ctc = counts(steps["ct0"][:, c].sum(0), steps["dct"][:, c].reshape(-1, nc))
    return tp, fp, ctc


def psds_from_score_buffer(buffer, ground_truth, audio_durations, dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3,
                           alpha_ct=0.0, alpha_st=0.0, unit_of_time="hour", max_efpr=100.0, classes=None):
    """psds_scores.psds_from_scores on a ScoreBuffer: same arguments, same 4-tuple, same errors; the clips `sorted(ground_truth)`
    are evaluated.  `classes` selects score columns by name (the DESED subset of the 2024 recipe); default: all of the buffer's."""
    if cttc_threshold is None and alpha_ct != 0:
        raise ValueError("cross triggers need a cttc_threshold")
    if alpha_st < 0 or not 0 <= alpha_ct <= 1:
        raise ValueError("alpha_st must be >= 0 and alpha_ct in [0, 1]")
    ids = sorted(ground_truth.keys())
    missing = [i for i in ids if i not in buffer or i not in audio_durations]
    if missing:
        raise ValueError("scores / durations missing for %d clips, e.g. %s" % (len(missing), missing[:3]))
    if not ids:
        raise ValueError("no clips to evaluate")
    classes, scores = _score_columns(buffer, ids, classes)
    dev = scores.device
    nsec = PSDSEval.secs_in_uot[unit_of_time]
    use_ct = cttc_threshold is not None and alpha_ct > 0
    table = _event_table(ground_truth, ids, classes)
    total_dur = 0.0
    durs = np.empty(len(ids), dtype=np.float64)
    for n, a in enumerate(ids):
        durs[n] = float(audio_durations[a])
        total_dur += durs[n]
    if total_dur <= 0:
        raise ValueError("the evaluated clips have no duration")
    ev_ptr, ev_on, ev_off = _event_table_on(table, dev)
    ts = torch.from_numpy(np.ascontiguousarray(buffer.timestamps, dtype=np.float64)).to(dev)
    steps = psds_steps(scores, ts, ev_ptr, ev_on, ev_off, torch.from_numpy(durs).to(dev), dtc_threshold, gtc_threshold,
                       cttc_threshold, use_ct)
    return _psd_roc_tail(classes, lambda c: _merged_counts(steps, c, use_ct), table["n_gt"], table["gt_dur"], total_dur, nsec,
                         use_ct, alpha_ct, alpha_st, max_efpr)
