"""Inference post-processing on the device: the batched counterpart of
recipes/dcase2023_task4_baseline/local/utils.py:16-73 (`batched_decode_preds`).

The reference loops over the clips of a batch on the host: `.cpu().numpy()`, scipy median filter, one threshold at a
time, `ManyHotEncoder.decode_strong` per clip.  Here the whole batch is median-filtered in one launch, all thresholds are
applied and turned into [onset_frame, offset_frame) regions in a second launch, and the host receives two compact integer
arrays with ONE synchronising copy; only the frame -> seconds conversion and the DataFrame assembly stay on the host.

`batched_decode_preds` keeps the reference's signature and return value (scores_raw, scores_postprocessed,
prediction_dfs).  `create_score_dataframe` (sed_scores_eval, third party, absent from the reference tree) is restated
below from its documented output format: columns onset, offset, then one column per event class.

The 2024 recipe (recipes/dcase2024_task4_baseline/local/utils.py:30-99) passes `median_filter` as a callable instead: None (no
filtering) or desed_task.utils.postprocess.ClassWiseMedianFilter (one window length per class).  `ClassWiseMedianFilter` below
is that class; handed to `batched_decode_preds` it runs as ONE device launch per batch (`median_filter_classwise`).
`segment_scores` turns frame scores into segment scores on the device (the 2024 test path's MAESTRO scoring)."""
import numbers
from pathlib import Path

import numpy as np
import torch

from . import _lib


def _btc(strong_preds):
    """(B, NC, T) reference-shaped posteriors -> contiguous (B, T, NC) (free when it already is our transposed view)."""
    if strong_preds.dim() != 3:
        raise ValueError("strong predictions must be (batch, classes, frames)")
    x = strong_preds.detach().transpose(1, 2)
    return x.contiguous().float()


def median_filter_scores(scores_btc, win=7):
    """scipy.ndimage.median_filter(scores[b], (win, 1)) for every clip b; scores (B, T, NC) on the GPU."""
    _lib.check_tensor(scores_btc, "scores")
    B, T, NC = scores_btc.shape
    out = torch.empty_like(scores_btc)
    _lib.get().call("sed_median_filter", scores_btc.data_ptr(), out.data_ptr(), B, T, NC, int(win), _lib.stream_ptr(scores_btc))
    return out


class ClassWiseMedianFilter:
    """desed_task/utils/postprocess.py:5-18: `filter_lens[c]` is the median window (frames) of class c.  Called on a (T, NC)
    numpy array it is the reference's host filter -- scipy.ndimage.median_filter(x[:, c:c+1], (filter_lens[c], 1)) per class.
    `batched_decode_preds(median_filter=<this>)` runs the same filter for the whole batch on the device instead."""

    def __init__(self, filter_lens=(1, 1, 1)):
        self.filter_lens = filter_lens
        self._dev = {}

    def __call__(self, x, **kwargs):
        from scipy.ndimage import median_filter
        out = []
        for c in range(x.shape[-1]):
            out.append(median_filter(x[..., c][..., None], (self.filter_lens[c], 1))[:, 0])
        return np.stack(out, -1)

    def device_windows(self, device):
        """The window lengths as an int32 tensor on `device` (made once per device)."""
        key = (str(device), tuple(int(w) for w in self.filter_lens))
        if key not in self._dev:
            self._dev = {key: torch.tensor(key[1], dtype=torch.int32, device=device)}
        return self._dev[key]


def median_filter_classwise(scores_btc, wins):
    """ClassWiseMedianFilter(wins) applied to every clip of scores (B, T, NC) in one launch: bit-exact with scipy.  wins: NC
    window lengths (sequence, or a ClassWiseMedianFilter), each 1 .. 64; a longer one is refused by the kernel
    (SED_ERR_UNSUPPORTED) -- there is no host path."""
    _lib.check_tensor(scores_btc, "scores")
    B, T, NC = scores_btc.shape
    filt = wins if isinstance(wins, ClassWiseMedianFilter) else ClassWiseMedianFilter(list(wins))
    lens = [int(w) for w in filt.filter_lens]
    if len(lens) != NC:
        raise ValueError("ClassWiseMedianFilter has %d window lengths for %d classes" % (len(lens), NC))
    if min(lens) < 1:
        raise ValueError("median window lengths must be >= 1")
    out = torch.empty_like(scores_btc)
    w_dev = filt.device_windows(scores_btc.device)
    _lib.get().call("sed_median_filter_classwise", scores_btc.data_ptr(), out.data_ptr(), w_dev.data_ptr(), B, T, NC, max(lens),
                    _lib.stream_ptr(scores_btc))
    return out


def segment_scores(scores_btc, clip_len, frame_hop, segment_length=1.0, n_seg=None, mode=0):
    """(B, T, NC) frame scores -> (B, n_seg, NC) segment scores on the device.  Frame i = [i * frame_hop, (i + 1) * frame_hop);
    clip b has ceil(clip_len[b] / segment_length) segments (the rest of its rows are 0).  mode 0: the overlap-weighted mean of
    the 2024 recipe's _get_segment_scores (sed_trainer_pretrained.py:1457-1490); mode 1: the maximum over overlapping frames."""
    import math
    _lib.check_tensor(scores_btc, "scores")
    B, T, NC = scores_btc.shape
    lens = torch.as_tensor(clip_len, dtype=torch.float32).reshape(-1)
    if lens.numel() != B:
        raise ValueError("one clip length per clip")
    if n_seg is None:
        n_seg = max([math.ceil(float(v) / segment_length) for v in lens.tolist()] + [1])
    lens = lens.to(scores_btc.device)
    out = torch.empty(B, int(n_seg), NC, dtype=torch.float32, device=scores_btc.device)
    _lib.get().call("sed_segment_scores", scores_btc.data_ptr(), lens.data_ptr(), out.data_ptr(), B, T, NC, float(frame_hop),
                    float(segment_length), int(n_seg), int(mode), _lib.stream_ptr(scores_btc))
    return out


def threshold_events(scores_btc, thresholds, true_len=None):
    """-> counts (n_thr, B, NC) and events (n_thr, B, NC, max_events, 2) int32 numpy arrays: the contiguous regions of
    `scores > threshold` per (threshold, clip, class) in frames.  One device->host copy."""
    _lib.check_tensor(scores_btc, "scores")
    B, T, NC = scores_btc.shape
    dev = scores_btc.device
    thr = torch.tensor([float(t) for t in thresholds], dtype=torch.float32, device=dev)
    n_thr = thr.numel()
    max_events = (T + 1) // 2
    counts = torch.empty(n_thr, B, NC, dtype=torch.int32, device=dev)
    events = torch.empty(n_thr, B, NC, max_events, 2, dtype=torch.int32, device=dev)
    tl = None
    if true_len is not None:
        tl = torch.as_tensor(true_len, dtype=torch.int32).to(dev)
    _lib.get().call("sed_threshold_events", scores_btc.data_ptr(), thr.data_ptr(), tl.data_ptr() if tl is not None else None,
                    counts.data_ptr(), events.data_ptr(), B, T, NC, n_thr, max_events, _lib.stream_ptr(scores_btc))
    return counts.cpu().numpy(), events.cpu().numpy()


def create_score_dataframe(scores, timestamps, event_classes):
    """sed_scores_eval.base_modules.scores.create_score_dataframe: rows = frames, columns onset / offset / classes."""
    import pandas as pd
    scores = np.asarray(scores)
    timestamps = np.asarray(timestamps)
    if scores.shape != (len(timestamps) - 1, len(event_classes)):
        raise ValueError("scores must be (n_frames, n_classes) with n_frames + 1 timestamps")
    return pd.DataFrame(np.concatenate((timestamps[:-1, None], timestamps[1:, None], scores), axis=1),
                        columns=["onset", "offset"] + list(event_classes))


def _filter_batch(scores, median_filter):
    """The post-processing filter of `batched_decode_preds` on (B, T, NC) device scores: int = one window for all classes
    (2023), None = none (2024 default), ClassWiseMedianFilter = one window per class (2024) -- both on the device; any other
    callable runs per clip on the host, as in the reference (utils.py:77 of the 2024 recipe)."""
    if median_filter is None:
        return scores
    if isinstance(median_filter, numbers.Number):
        return median_filter_scores(scores, median_filter)
    if isinstance(median_filter, ClassWiseMedianFilter):
        return median_filter_classwise(scores, median_filter)
    if not callable(median_filter):
        raise TypeError("median_filter must be an int window, None, or a callable on (frames, classes) arrays")
    x = scores.cpu().numpy()
    filt = np.stack([median_filter(x[j]) for j in range(x.shape[0])]).astype(np.float32)
    return torch.from_numpy(filt).to(scores.device)


def batched_decode_preds(strong_preds, filenames, encoder, thresholds=[0.5], median_filter=7, pad_indx=None,  # noqa: B006
                         device_scores=None):
    """Reference signature and return value (utils.py:16-73); `median_filter` is the window length as there, or (2024 recipe)
    None / a ClassWiseMedianFilter / any callable on a clip's (frames, classes) array.  `thresholds=[]` (the 2024 validation)
    returns the score tables and an empty dict of decodings.

    Knowing deviation: with `pad_indx` the reference crops `c_scores[:true_len]` BEFORE transposing, i.e. along the class axis
    of the (NC, T) tensor (utils.py:48-52) -- an inert slip, since no caller of the 2023 recipe passes `pad_indx`.  Here
    `pad_indx` crops the time axis, which is what the argument documents.

    `device_scores` (an evaluation.psds_device.ScoreBuffer): the filtered scores are appended there and stay on the device; the two
    score-table dicts come back empty -- neither the tables nor the two host copies that feed them are made.  One clip length per
    buffer, so not together with `pad_indx`."""
    import pandas as pd
    if device_scores is not None and pad_indx is not None:
        raise ValueError("device_scores keeps clips of one length: it cannot be combined with pad_indx")
    scores = _btc(strong_preds)                                   # (B, T, NC)
    B, T, NC = scores.shape
    true_len = None
    if pad_indx is not None:
        true_len = [int(T * float(pad_indx[j])) for j in range(B)]
    if true_len is not None and any(n != T for n in true_len):
        # the reference crops each clip BEFORE filtering, so the reflection happens at the clip's own end: filter per length
        filt = torch.empty_like(scores)
        for n in sorted(set(true_len)):
            rows = [j for j in range(B) if true_len[j] == n]
            if n > 0:
                filt[rows, :n] = _filter_batch(scores[rows, :n].contiguous(), median_filter)
    else:
        filt = _filter_batch(scores, median_filter)
    if len(thresholds) == 0:
        counts, events = np.zeros((0, B, NC), dtype=np.int32), np.zeros((0, B, NC, 1, 2), dtype=np.int32)
    else:
        counts, events = threshold_events(filt, thresholds, true_len)
    scores_raw, scores_post = {}, {}
    audio_ids = [Path(f).stem for f in filenames]
    if device_scores is not None:
        device_scores.append(filt, audio_ids, timestamps=encoder._frame_to_time(np.arange(T + 1)), event_classes=encoder.labels)
    else:
        raw_np, filt_np = scores.cpu().numpy(), filt.cpu().numpy()
        for j in range(B):
            n = T if true_len is None else true_len[j]
            ts = encoder._frame_to_time(np.arange(n + 1))
            scores_raw[audio_ids[j]] = create_score_dataframe(raw_np[j, :n], ts, encoder.labels)
            scores_post[audio_ids[j]] = create_score_dataframe(filt_np[j, :n], ts, encoder.labels)
    # all regions of all thresholds at once; np.nonzero walks (threshold, clip, class, region) in C order, which is the
    # reference's row order per threshold: clip-major, then decode_strong's class-major / time order
    valid = np.arange(events.shape[3])[None, None, None, :] < counts[..., None]
    k, j, c, e = np.nonzero(valid)
    onset = np.asarray(encoder._frame_to_time(events[k, j, c, e, 0]), dtype=np.float64)
    offset = np.asarray(encoder._frame_to_time(events[k, j, c, e, 1]), dtype=np.float64)
    label_arr = np.asarray(list(encoder.labels), dtype=object)
    file_arr = np.asarray([a + ".wav" for a in audio_ids], dtype=object)
    bounds = np.searchsorted(k, np.arange(len(thresholds) + 1))
    prediction_dfs = {}
    for i, th in enumerate(thresholds):
        sl = slice(bounds[i], bounds[i + 1])
        prediction_dfs[th] = pd.DataFrame({"event_label": label_arr[c[sl]], "onset": onset[sl], "offset": offset[sl],
                                           "filename": file_arr[j[sl]]}, columns=["event_label", "onset", "offset", "filename"])
    return scores_raw, scores_post, prediction_dfs


def write_sed_scores(scores, storage_path):
    """sed_scores_eval.io.write_sed_scores: one `<audio_id>.tsv` score table per clip under `storage_path`."""
    import os
    os.makedirs(storage_path, exist_ok=True)
    for audio_id, df in scores.items():
        df.to_csv(os.path.join(storage_path, audio_id + ".tsv"), sep="\t", index=False)
