"""MAESTRO scoring helpers of the 2024 recipe (recipes/dcase2024_task4_baseline/local/sed_trainer_pretrained.py:1366-1490),
restated: the real MAESTRO recordings are scored as 10 s clips named `<file>-<onset cs>-<offset cs>`; ground truth and
segment scores are put back together per recording.

  * merge_overlapping_events   (:1384-1403): per clip and class, events sorted; an event that starts at or before the current
                                end extends it.  Events as [onset, offset, class] lists; the dict is updated in place and returned.
  * merge_maestro_ground_truth (:1366-1381): clip events shifted by the clip onset -- whole seconds, int(onset_cs) // 100, as
                                there -- gathered per recording, then merged.
  * segment_scores_and_overlap_add (:1406-1455): the mean score of every 1 s segment of every clip (the overlap-weighted mean of
                                _get_segment_scores, computed for all clips in one device launch: postprocess.segment_scores
                                mode 0), then per recording the sum of the clips' segment scores over the number of clips
                                that cover each segment.
"""
from collections import defaultdict
from math import ceil

import numpy as np


def merge_overlapping_events(ground_truth_events):
    for clip_id, events in ground_truth_events.items():
        per_class = defaultdict(list)
        for ev in events:
            per_class[ev[2]].append(ev)
        merged_all = []
        for _, evs in per_class.items():
            merged, end = [], -1e6
            for ev in sorted(evs):
                if ev[0] > end:
                    merged.append(list(ev))
                else:
                    merged[-1][1] = max(end, ev[1])
                end = merged[-1][1]
            merged_all.extend(merged)
        ground_truth_events[clip_id] = merged_all
    return ground_truth_events


def _clip_span(clip_id):
    file_id, on, off = clip_id.rsplit("-", maxsplit=2)
    return file_id, on, off


def merge_maestro_ground_truth(clip_ground_truth):
    per_file = defaultdict(list)
    for clip_id, events in clip_ground_truth.items():
        file_id, on, _ = _clip_span(clip_id)
        shift = int(on) // 100
        per_file[file_id].extend((shift + a, shift + b, c) for a, b, c in events)
    return merge_overlapping_events(per_file)


def segment_scores_and_overlap_add(frame_scores, audio_durations, event_classes, segment_length=1.0, device=None):
    """frame_scores {clip_id: score table}; audio_durations {file_id: seconds} -> {file_id: segment score table}.
    The clips' columns `event_classes` go to the device in one (n_clips, T, NC) tensor per frame count."""
    import torch
    from ..postprocess import create_score_dataframe, segment_scores
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    clips = list(frame_scores.keys())
    keys = ["onset", "offset"] + list(event_classes)
    by_len = defaultdict(list)
    for cid in clips:
        by_len[len(frame_scores[cid])].append(cid)
    seg = {}
    for _, group in by_len.items():
        arr = np.stack([frame_scores[cid][keys[2:]].to_numpy(np.float32) for cid in group])
        onsets = frame_scores[group[0]]["onset"].to_numpy(np.float64)
        hop = float(onsets[1] - onsets[0]) if len(onsets) > 1 else float(frame_scores[group[0]]["offset"].iloc[0])
        lens = []
        for cid in group:
            _, on, off = _clip_span(cid)
            lens.append(float(off) / 100 - float(on) / 100)
        # the reference scores every clip with its own segment count (np.arange(0, clip_length, 1.0))
        out = segment_scores(torch.from_numpy(arr).to(device), lens, hop, segment_length, mode=0).cpu().numpy()
        for i, cid in enumerate(group):
            seg[cid] = out[i, :ceil(lens[i] / segment_length)].astype(np.float64)
    sums, counts = {}, {}
    for cid in clips:
        file_id, on, _ = _clip_span(cid)
        if file_id not in sums:
            sums[file_id] = np.zeros((ceil(audio_durations[file_id] / segment_length), len(event_classes)))
            counts[file_id] = np.zeros_like(sums[file_id])
        k = int((float(on) / 100) // segment_length)
        s = seg[cid]
        n = len(sums[file_id][k:k + len(s)])
        sums[file_id][k:k + n] += s[:n]
        counts[file_id][k:k + n] += 1
    return {file_id: create_score_dataframe(
        sums[file_id] / np.maximum(counts[file_id], 1),
        np.minimum(np.arange(0.0, audio_durations[file_id] + segment_length, segment_length), audio_durations[file_id]),
        list(event_classes)) for file_id in sums}
