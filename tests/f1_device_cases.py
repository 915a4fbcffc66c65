"""Cases for the collar / segment / intersection F1 counts on the device (desed_task_amd/evaluation/f1_device.py, csrc/sed_f1.hip),
device-agnostic like psds_device_cases.py: dev = "cpu" on the fiber emulator, "cuda" on the MI355X.

The yardstick is the host code on the frame `DecodedScores.to_dataframe()` builds: per (threshold, clip, class) the eight fields are
recomputed from `EventBasedMetrics`, `SegmentBasedMetrics` and `PSDSEval._evaluate_detections` on that pair's rows, end to end from
`log_sedeval_metrics` and `compute_per_intersection_macro_f1`.  The reference frame of a case is decoded once on the host
(`host_frame`) and every device test first checks that `to_dataframe()` equals it row for row.

Tolerances: the fields are integers out of the same IEEE double operations and are compared exactly (the builder asserts per case
that the host intersection counts do not move when dtc / gtc / cttc are scaled by 1 -+ 1e-9, so no ratio sum sits on its threshold);
the F scores come out of shared formulas from equal integers and get 1e-12 absolute, a bound that is derived and not measured.
"""
import contextlib
import functools
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

from desed_task_amd import _lib
from desed_task_amd.evaluation import evaluation_measures as EM
from desed_task_amd.evaluation import f1_device as F
from desed_task_amd.evaluation import psds_device as D
from desed_task_amd.evaluation import sed_eval_metrics as SE
from desed_task_amd.evaluation.psds import PSDSEval, Thresholds
from tests import parity_cases as P
from tests import psds_device_cases as M
from tests.resident_cases import CANARY, Framed, sync

T_COLLAR, PCT, RES = 0.2, 0.2, 1.0
DTC, GTC, CTTC = 0.5, 0.5, 0.3
# name: (clips, frames, classes, quantisation levels or None, seed, thresholds)
SHAPES = {
    "a": (5, 156, 10, None, 201, (0.3, 0.5)),       # the recipe's clip
    "b": (4, 157, 4, 16, 202, (0.3, 0.5)),          # odd length; 16 levels k / 16: scores equal to 0.5 exactly (strict >)
    "c": (4, 7, 3, None, 203, (0.3, 0.5)),
    "d": (4, 1, 2, None, 204, (0.3, 0.5)),          # a single frame
    "e": (3, 64, 27, None, 205, (0.3, 0.5)),        # the 2024 class count
    "f": (6, 156, 4, None, 206, (0.3, 0.5)),        # edge contents, see _edge_contents
    "g": (48, 156, 10, None, 207, (0.3, 0.5)),      # two validation batches (GPU only)
    "h": (3, 40, 9, None, 208, (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)),     # n_thr = 8: 72 columns, two column groups per clip
}
CPU_CASES = ("a", "b", "c", "d", "e", "f", "h")
GPU_CASES = CPU_CASES + ("g",)
MAX_RUNS = 78                                        # (156 + 1) / 2: the run-list capacity at the recipe's clip length


def _scores(rng, N, T, NC, levels):
    from scipy.ndimage import median_filter
    x = rng.random_sample((N, T, NC)).astype(np.float32)
    if T >= 7:
        x = np.stack([median_filter(x[n], (7, 1)) for n in range(N)])
    if levels:
        x = (np.floor(x * levels) / levels).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


MATCH_B, MATCH_C = (0.5262, 0.8142), (0.4385, 0.6225)


def _edge_contents(rng, c):
    """Case f.  Clip 0: class 0 entirely above the thresholds (one run, offset ts[T]), class 1 entirely below, class 2 alternating
    every frame (78 runs: the run-list capacity), class 3 THE MATCHING CASE: events B then C, runs on frames [7, 10) and [11, 15)
    only (at 0.4: detected at 0.3, not at 0.5).  Clip 1: 10 events of class 2, two overlapping events of class 0.  Clip 2: 9.5 s
    long with a run of classes 0 and 1 across its end.  Class 1 has no ground truth; class 3 is never detected at 0.5 and holds
    scores equal to 0.5 exactly.  Clip 4's only row has no label, clip 5 is not in the table, and the table lists a clip that was
    never scored."""
    labels, ids, s, T = c["labels"], c["ids"], c["scores"], c["scores"].shape[1]
    length = float(c["ts"][-1])
    s[:, :, 3] = (np.floor(s[:, :, 3] * 8) / 16).astype(np.float32)              # {0, 1/16 .. 7/16}: below 0.5
    s[3, 20:31, 3] = np.float32(0.5)                                              # equal to the threshold: not a detection
    s[0, :, 0], s[0, :, 1] = 1.0, 0.0
    s[0, 0::2, 2], s[0, 1::2, 2] = 1.0, 0.0
    s[0, :, 3] = 0.0
    s[0, 7:10, 3] = s[0, 11:15, 3] = np.float32(0.4)
    s[2, 140:T, 0] = s[2, 140:T, 1] = 1.0
    gt = c["gt"]
    for a in ids:
        gt[a] = [(o, f, l) for o, f, l in gt[a] if l not in (labels[1], labels[3])]
    # (0.1234, 8.1): 1.884 s before the offset of class 0's single run -- outside 20 % of the event's length, inside 20 % of the run's
    gt[ids[0]] = ([(o, f, l) for o, f, l in gt[ids[0]] if l != labels[3]]
                  + [MATCH_B + (labels[3],), MATCH_C + (labels[3],), (0.1234, 8.1, labels[0])])
    many = []
    for _ in range(10):
        on = float(rng.uniform(0.0, 0.9 * length))
        many.append((on, on + float(rng.uniform(0.02 * length, 0.08 * length)), labels[2]))
    gt[ids[1]] = many + [(1.0123, 3.0456, labels[0]), (2.0111, 4.0789, labels[0])]
    gt[ids[3]] = gt[ids[3]] + [(1.3217, 2.0123, labels[3])]
    gt[ids[4]] = []
    c["dur"][ids[2]] = 9.5
    c["unlisted"] = [ids[5]]
    c["unscored"] = {"never_scored_f": [(0.5111, 2.25, labels[0]), (3.0, 4.5, labels[2])]}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: scores (N, T, NC) fp32, ts, ids, labels, thresholds, gt {id: events}, dur {id: seconds}, the reference / duration
    tables as the recipes' TSV files hold them, the host frames per threshold and the host fields per (threshold, clip, class)."""
    N, T, NC, levels, seed, thresholds = SHAPES[name]
    rng = np.random.RandomState(seed)
    ts = M._timestamps(T)
    labels = ["c%02d" % i for i in range(NC)]
    ids = ["clip_%s_%02d" % (name, (7 * n + 3) % N) for n in range(N)]          # not in sorted order
    assert len(set(ids)) == N
    c = {"name": name, "scores": _scores(rng, N, T, NC, levels), "ts": ts, "ids": ids, "labels": labels, "thresholds": list(thresholds),
         "gt": {a: M._events(rng, rng.randint(0, 6), float(ts[-1]), labels) for a in ids}, "dur": {a: 10.0 for a in ids},
         "unlisted": [], "unscored": {}}
    if name == "f":
        _edge_contents(rng, c)
    if name == "b":
        assert (c["scores"] == np.float32(0.5)).any(), "case b must hold scores equal to a threshold"
    rows = []
    for a in ids + list(c["unscored"]):
        if a in c["unlisted"]:
            continue
        events = c["gt"][a] if a in c["gt"] else c["unscored"][a]
        rows += [(a + ".wav", o, f, l) for o, f, l in events] or [(a + ".wav", np.nan, np.nan, np.nan)]
    c["gt_df"] = pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])
    c["dur_df"] = pd.DataFrame([(a + ".wav", c["dur"].get(a, 10.0)) for a in ids + list(c["unscored"])], columns=["filename", "duration"])
    for a in c["unlisted"]:
        c["gt"][a] = []
    c["frames"] = {th: host_frame(c["scores"], ts, ids, labels, th) for th in thresholds}
    c["host"] = host_fields(c)
    if name == "f":
        _edge_preconditions(c)
    return c


def host_frame(scores, ts, ids, labels, th):
    """The detections at `score > th` (fp32) as batched_decode_preds lists them: clip-major, class-major, time order."""
    rows = []
    for n, a in enumerate(ids):
        on = np.pad(scores[n] > np.float32(th), ((1, 1), (0, 0)))
        d = np.diff(on.astype(np.int8), axis=0)
        for k in range(scores.shape[2]):
            starts, ends = np.nonzero(d[:, k] == 1)[0], np.nonzero(d[:, k] == -1)[0]
            rows += [(labels[k], float(ts[i]), float(ts[j]), a + ".wav") for i, j in zip(starts, ends)]
    return pd.DataFrame(rows, columns=["event_label", "onset", "offset", "filename"])


def _psds_of(c):
    """One PSDSEval over the case's tables plus a file that gives every label a ground-truth event (a label without one is unknown
    to PSDSEval and its detections would be dropped); a pair's detections are then evaluated alone."""
    extra = pd.DataFrame([("__every_label__.wav", 0.0, 1.0, l) for l in c["labels"]], columns=["filename", "onset", "offset", "event_label"])
    meta = pd.concat([c["dur_df"], pd.DataFrame([("__every_label__.wav", 10.0)], columns=["filename", "duration"])], ignore_index=True)
    return PSDSEval(ground_truth=pd.concat([c["gt_df"], extra], ignore_index=True), metadata=meta, dtc_threshold=DTC, gtc_threshold=GTC,
                    cttc_threshold=CTTC)


def _pair_intersection(psds, fname, label, dets, scale=1.0):
    k = psds._cls[label]
    d = dict(file=np.full(len(dets), psds._files[fname], np.int64), on=np.array([o for o, _ in dets], np.float64),
             off=np.array([f for _, f in dets], np.float64), lab=np.full(len(dets), k, np.int64))
    psds.threshold = Thresholds(dtc=DTC * scale, gtc=GTC * scale, cttc=CTTC * scale)
    counts = psds._evaluate_detections(d)[0]
    psds.threshold = Thresholds(dtc=DTC, gtc=GTC, cttc=CTTC)
    return int(counts[k, k]), int(counts[k, -1])


def host_fields(c):
    """(n_thr, N, NC, 8) int64 by the host classes, one (threshold, clip, class) at a time, after the stability precondition."""
    N, T, NC = c["scores"].shape
    out = np.zeros((len(c["thresholds"]), N, NC, 8), dtype=np.int64)
    psds = _psds_of(c)
    for k, th in enumerate(c["thresholds"]):
        by_pair = {}
        for r in c["frames"][th].itertuples():
            by_pair.setdefault((r.filename, r.event_label), []).append((r.onset, r.offset))
        for n, a in enumerate(c["ids"]):
            for j, lab in enumerate(c["labels"]):
                dets = by_pair.get((a + ".wav", lab), [])
                ref = [{"onset": o, "offset": f, "event_label": l} for o, f, l in c["gt"][a] if l == lab]
                est = [{"onset": o, "offset": f, "event_label": lab} for o, f in dets]
                ev = SE.EventBasedMetrics([lab], t_collar=T_COLLAR, percentage_of_length=PCT, empty_system_output_handling="zero_score")
                ev.evaluate(ref, est)
                seg = SE.SegmentBasedMetrics([lab], time_resolution=RES)
                seg.evaluate(ref, est)
                w = seg.class_wise[lab]
                tp, fp = _pair_intersection(psds, a + ".wav", lab, dets)
                for scale in (1.0 - 1e-9, 1.0 + 1e-9):
                    assert _pair_intersection(psds, a + ".wav", lab, dets, scale) == (tp, fp), \
                        "case %s, %s / %s at %s is not stable under a 1e-9 change of dtc / gtc / cttc" % (c["name"], a, lab, th)
                assert ev.class_wise[lab]["Nsys"] == len(dets) and ev.class_wise[lab]["Nref"] == len(ref)
                out[k, n, j] = (len(dets), ev.class_wise[lab]["Ntp"], w["Nref"], w["Nsys"], w["Ntp"], tp, fp, 0)
    return out


def _pairs(c, k):
    """(n, j, reference events, runs) of every (clip, class) at threshold k."""
    th = c["thresholds"][k]
    by_pair = {}
    for r in c["frames"][th].itertuples():
        by_pair.setdefault((r.filename, r.event_label), []).append((r.onset, r.offset))
    for n, a in enumerate(c["ids"]):
        for j, lab in enumerate(c["labels"]):
            yield n, j, [(o, f) for o, f, l in c["gt"][a] if l == lab], by_pair.get((a + ".wav", lab), [])


def _time_match(ref, run, length=None, use_max=True):
    if math.fabs(ref[0] - run[0]) > T_COLLAR:
        return False
    tol = PCT * ((ref[1] - ref[0]) if length is None else length)
    return math.fabs(ref[1] - run[1]) <= (max(T_COLLAR, tol) if use_max else tol)


def _edge_preconditions(c):
    """What case f must contain, asserted with host code before anything is compared."""
    ids, labels, k03 = c["ids"], c["labels"], c["thresholds"].index(0.3)
    # the matching case: maximum 2, first fit in event order 1
    runs = [(r.onset, r.offset) for r in c["frames"][0.3].itertuples() if r.filename == ids[0] + ".wav" and r.event_label == labels[3]]
    assert runs == [(float(c["ts"][7]), float(c["ts"][10])), (float(c["ts"][11]), float(c["ts"][15]))]
    adj = [[i for i, run in enumerate(runs) if _time_match(ev, run)] for ev in (MATCH_B, MATCH_C)]
    assert adj == [[0, 1], [0]]
    assert SE._max_bipartite_matching(adj, 2)[0] == 2 and c["host"][k03, 0, 3, 1] == 2
    assert model_fields(c, matching="first_fit")[k03, 0, 3, 1] == 1
    assert c["host"][:, :, :, 0].max() == MAX_RUNS, "some pair must reach the run-list capacity"
    assert any(sum(_time_match(ev, run) for run in runs) > 1 for k in range(len(c["thresholds"])) for _, _, evs, runs in _pairs(c, k)
               for ev in evs), "some event must be adjacent to more than one run"
    assert c["host"][c["thresholds"].index(0.5), :, 3, 0].sum() == 0, "class 3 is never detected at 0.5"
    assert len(c["frames"][0.5]) and c["frames"][0.5].offset.max() == float(c["ts"][-1])


def model_fields(c, matching="greedy", strict=True, offset_length="event", use_max=True, raster_end=math.ceil):
    """The kernel's algorithm in Python, with the switches of the discrimination test: `matching` "greedy" (smallest hi first) or
    "first_fit" (events in order take their first free run), `strict` False = `>=` at the threshold, `offset_length` "run" = the
    offset collar from the run's length, `use_max` False = no max(t_collar, ...), `raster_end` math.floor = cells [floor, floor)."""
    N, T, NC = c["scores"].shape
    ts = c["ts"]
    out = np.zeros((len(c["thresholds"]), N, NC, 8), dtype=np.int64)
    for k, th in enumerate(c["thresholds"]):
        for n, a in enumerate(c["ids"]):
            for j, lab in enumerate(c["labels"]):
                col = c["scores"][n, :, j]
                on = np.pad(col > np.float32(th) if strict else col >= np.float32(th), (1, 1))
                d = np.diff(on.astype(np.int8))
                runs = [(float(ts[i]), float(ts[e])) for i, e in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0])]
                evs = [(o, f) for o, f, l in c["gt"][a] if l == lab]
                adj = [[i for i, run in enumerate(runs)
                        if _time_match(ev, run, None if offset_length == "event" else run[1] - run[0], use_max)] for ev in evs]
                if offset_length == "event":
                    assert all(v == list(range(v[0], v[-1] + 1)) for v in adj if v), "an event's runs must be a contiguous range"
                tp, used = 0, set()
                if matching == "first_fit":
                    for v in adj:
                        free = [i for i in v if i not in used]
                        if free:
                            used.add(free[0])
                            tp += 1
                else:
                    for i in range(len(runs)):
                        open_ = [(v[-1], e) for e, v in enumerate(adj) if e not in used and v and v[0] <= i <= v[-1]]
                        if open_:
                            used.add(min(open_)[1])
                            tp += 1
                cells = lambda iv: {x for o, f in iv for x in range(int(math.floor(o / RES)), int(raster_end(f / RES)))}      # noqa: E731
                ref_cells, sys_cells = cells(evs), cells(runs)
                relevant, fp = [], 0
                for o, f in runs:
                    ratios = [(min(f, gf) - max(o, go)) / (f - o) for go, gf in evs if min(f, gf) - max(o, go) > 0]
                    rel = bool(ratios) and sum(ratios, 0.0) >= DTC
                    relevant.append(rel)
                    w = min(f, c["dur"][a]) - max(o, 0.0)
                    if not rel and w > 0 and w / (f - o) >= CTTC:
                        fp += 1
                hit = 0
                for go, gf in evs:
                    ratios = [(min(f, gf) - max(o, go)) / (gf - go) for (o, f), rel in zip(runs, relevant) if rel and min(f, gf) - max(o, go) > 0]
                    hit += bool(ratios) and sum(ratios, 0.0) >= GTC
                out[k, n, j] = (len(runs), tp, len(ref_cells), len(sys_cells), len(ref_cells & sys_cells), hit, fp, 0)
    return out


def case_discrimination():
    """Assertion 6, host only: the Python model of the kernel equals the host fields on every CPU case, and on the edge case each
    lazy variant changes at least one field."""
    for name in CPU_CASES:
        c = case(name)
        assert np.array_equal(model_fields(c), c["host"]), name
    c = case("f")
    for what, kw in (("first-fit matching", dict(matching="first_fit")), (">= at the threshold", dict(strict=False)),
                     ("the run's length in the offset collar", dict(offset_length="run")), ("no max(t_collar, ...)", dict(use_max=False)),
                     ("floor for ceil in the raster", dict(raster_end=math.floor))):
        assert not np.array_equal(model_fields(c, **kw), c["host"]), "%s changes no field of case f" % what


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def _device_inputs(dev, c, scores=None, thresholds=None):
    ids = c["ids"]
    table = D._event_table({a: c["gt"][a] for a in ids}, ids, c["labels"])
    ev_ptr, ev_on, ev_off = D._event_table_on(table, torch.device(dev))
    scores = P.to(dev, torch.from_numpy(np.ascontiguousarray(c["scores"] if scores is None else scores)))
    thr = P.to(dev, torch.tensor(c["thresholds"] if thresholds is None else thresholds, dtype=torch.float32))
    ts = P.to(dev, torch.from_numpy(np.ascontiguousarray(c["ts"])))
    dur = P.to(dev, torch.tensor([c["dur"][a] for a in ids], dtype=torch.float64))
    return scores, thr, ts, ev_ptr, ev_on, ev_off, dur


def fill_buffer(dev, c, chunks=2):
    """A ScoreBuffer holding the case's clips in case order, appended in `chunks` batches; the first clip is appended twice, the first
    time with other scores (the later row must win)."""
    buf = D.ScoreBuffer()
    N = len(c["ids"])
    buf.append(P.to(dev, torch.from_numpy(np.ascontiguousarray(1.0 - c["scores"][:1]))), c["ids"][:1], timestamps=c["ts"],
               event_classes=c["labels"])
    edges = np.linspace(0, N, chunks + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            buf.append(P.to(dev, torch.from_numpy(np.ascontiguousarray(c["scores"][a:b]))), c["ids"][a:b], timestamps=c["ts"],
                       event_classes=c["labels"])
    return buf


def case_kernel(dev, name):
    """Assertion 1: all eight fields of every (threshold, clip, class) equal the host's; canary frames intact; two launches write
    identical bytes."""
    c = case(name)
    N, T, NC = c["scores"].shape
    n_thr = len(c["thresholds"])
    inputs = _device_inputs(dev, c)
    runs = []
    for _ in range(2):
        frame = Framed(dev, n_thr * N * NC, 8, torch.int32)
        F.f1_counts_kernel(*inputs, T_COLLAR, PCT, RES, DTC, GTC, CTTC, out=frame.body.view(n_thr, N, NC, 8))
        sync(dev)
        frame.assert_guards("counts of case %s" % name)
        runs.append(frame.buf.cpu())
    assert torch.equal(runs[0], runs[1]), "two launches differ"
    got = frame.body.view(n_thr, N, NC, 8).cpu().numpy().astype(np.int64)
    bad = np.argwhere(got != c["host"])
    assert len(bad) == 0, ("case %s: (threshold, clip, class, field) %s: kernel %s, host %s"
                           % (name, bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(c["host"][tuple(b)]) for b in bad[:5]]))
    assert not got[..., 7].any()


def case_dataframe(dev, name):
    """Assertion 2: `to_dataframe()` equals the concatenated `decoded[th]` of batched_decode_preds on the same batches, row for row
    (and the host-decoded frame the yardsticks were computed on); `.empty` is the frame's."""
    from pandas.testing import assert_frame_equal
    from desed_task_amd import postprocess as PP
    c = case(name)
    N = len(c["ids"])
    enc = P._Encoder(c["labels"], audio_len=10)
    buf = D.ScoreBuffer()
    decoded = {th: [] for th in c["thresholds"]}
    edges = np.linspace(0, N, 3).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        strong = P.to(dev, torch.from_numpy(np.ascontiguousarray(c["scores"][a:b].transpose(0, 2, 1))))
        files = ["/data/synth_val/%s.wav" % i for i in c["ids"][a:b]]
        _, _, dfs = PP.batched_decode_preds(strong, files, enc, thresholds=c["thresholds"], median_filter=None, device_scores=buf)
        for th in c["thresholds"]:
            decoded[th].append(dfs[th])
    for th in c["thresholds"] + [2.0]:
        dec = F.DecodedScores(buf, th)
        got = dec.to_dataframe()
        if th == 2.0:
            assert dec.empty and got.empty and list(got.columns) == ["event_label", "onset", "offset", "filename"]
            continue
        ref = pd.concat(decoded[th], ignore_index=True)
        assert_frame_equal(got, ref, check_exact=True)
        assert_frame_equal(got, c["frames"][th], check_exact=True)
        assert dec.empty == ref.empty


def _host_end_to_end(c, frames, tmp, gt_df=None, dur_df=None):
    """The host functions on the frames: ({threshold: 4-tuple}, intersection macro F1)."""
    gt_path, dur_path = os.path.join(tmp, "gt.tsv"), os.path.join(tmp, "dur.tsv")
    (c["gt_df"] if gt_df is None else gt_df).to_csv(gt_path, sep="\t", index=False)
    (c["dur_df"] if dur_df is None else dur_df).to_csv(dur_path, sep="\t", index=False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)           # PSDSEval: detections of labels absent from the ground truth
        return ({th: EM.log_sedeval_metrics(df, gt_path) for th, df in frames.items()},
                EM.compute_per_intersection_macro_f1(frames, gt_path, dur_path), gt_path, dur_path)


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12


def case_end_to_end(dev, name, tmp):
    """Assertion 3: the sed_eval 4-tuple per threshold and the intersection macro F1 equal the host functions' values within 1e-12,
    through the public functions; with an empty threshold among the others, and with all thresholds empty."""
    c = case(name)
    buf = fill_buffer(dev, c)
    assert list(buf) == c["ids"]
    frames = dict(c["frames"])
    frames[2.0] = host_frame(c["scores"], c["ts"], c["ids"], c["labels"], 2.0)
    assert frames[2.0].empty
    ref4, ref_inter, gt_path, dur_path = _host_end_to_end(c, frames, tmp)
    assert ref4[2.0] == (0.0, 0.0, 0.0, 0.0)
    for th in frames:
        got = EM.log_sedeval_metrics(F.DecodedScores(buf, th), gt_path)
        assert len(got) == 4 and all(_close(g, r) for g, r in zip(got, ref4[th])), (name, th, got, ref4[th])
    got = EM.compute_per_intersection_macro_f1({th: F.DecodedScores(buf, th) for th in frames}, gt_path, dur_path)
    assert _close(got, ref_inter), (name, got, ref_inter)
    some = [v for th in c["thresholds"] for v in ref4[th]] + [ref_inter]
    assert name in ("c", "d") or any(v > 0 for v in some), "case %s scores nothing: it would not discriminate" % name
    # all thresholds empty
    empty = {2.0: frames[2.0], 3.0: frames[2.0]}
    assert EM.compute_per_intersection_macro_f1(empty, gt_path, dur_path) == 0
    assert EM.compute_per_intersection_macro_f1({th: F.DecodedScores(buf, th) for th in empty}, c["gt_df"], c["dur_df"]) == 0
    # the per-clip tensor and the sums of f1_counts
    by_id, _ = F._events_by_id(c["gt_df"])
    res = F.f1_counts(buf, c["thresholds"], by_id, {a: c["dur"][a] for a in c["ids"]})
    assert res["ids"] == c["ids"] and res["classes"] == c["labels"] and res["sums"].dtype == np.int64
    assert np.array_equal(res["counts"].cpu().numpy(), c["host"])
    listed = np.array([a not in c["unlisted"] for a in c["ids"]])
    assert np.array_equal(res["sums"][..., :5], c["host"][:, listed][..., :5].sum(1))
    assert np.array_equal(res["sums"][..., 5:7], c["host"][..., 5:7].sum(1)) and np.array_equal(res["sums"][..., 7], c["host"][..., 0].sum(1))


def case_written_reports(dev, tmp):
    """With `save_dir` log_sedeval_metrics writes the same two report files from a DecodedScores as from the frame."""
    c = case("f")
    buf = fill_buffer(dev, c)
    gt_path = os.path.join(tmp, "gt.tsv")
    c["gt_df"].to_csv(gt_path, sep="\t", index=False)
    host = EM.log_sedeval_metrics(c["frames"][0.5], gt_path, os.path.join(tmp, "host"))
    got = EM.log_sedeval_metrics(F.DecodedScores(buf, 0.5), gt_path, os.path.join(tmp, "dev"))
    assert got == host
    for f in ("event_f1.txt", "segment_f1.txt"):
        assert open(os.path.join(tmp, "host", f), "rb").read() == open(os.path.join(tmp, "dev", f), "rb").read(), f


def case_class_subset(dev, tmp):
    """`classes=` / `ids=`: seven columns of a 27-class buffer in another order than the buffer's, and two of its three clips."""
    c = case("e")
    sub = [c["labels"][i] for i in (9, 0, 3, 4, 20, 26, 11)]
    ids = [c["ids"][2], c["ids"][0]]
    rng = np.random.RandomState(9)
    gt_df = pd.DataFrame([(a + ".wav", o, f, sub[(i + n) % len(sub)]) for n, a in enumerate(ids)
                          for i, (o, f, _) in enumerate(M._events(rng, 4, float(c["ts"][-1]), sub))],
                         columns=["filename", "onset", "offset", "event_label"])
    dur_df = pd.DataFrame([(a + ".wav", 10.0) for a in ids], columns=["filename", "duration"])
    cols = [c["labels"].index(l) for l in sub]
    rows = [c["ids"].index(a) for a in ids]
    frames = {th: host_frame(c["scores"][rows][:, :, cols], c["ts"], ids, sub, th) for th in c["thresholds"]}
    ref4, ref_inter, gt_path, dur_path = _host_end_to_end(c, frames, tmp, gt_df, dur_df)
    buf = fill_buffer(dev, c)
    from pandas.testing import assert_frame_equal
    for th in frames:
        dec = F.DecodedScores(buf, th, classes=sub, ids=ids)
        assert_frame_equal(dec.to_dataframe(), frames[th], check_exact=True)
        got = EM.log_sedeval_metrics(dec, gt_path)
        assert all(_close(g, r) for g, r in zip(got, ref4[th])) and ref4[th][2] > 0, (th, got, ref4[th])
    got = EM.compute_per_intersection_macro_f1({th: F.DecodedScores(buf, th, classes=sub, ids=ids) for th in frames}, gt_path, dur_path)
    assert _close(got, ref_inter) and ref_inter > 0, (got, ref_inter)
    with pytest.raises(ValueError, match="classes without a score column"):
        F.DecodedScores(buf, 0.5, classes=["unknown"]).to_dataframe()
    with pytest.raises(ValueError, match="clips without scores"):
        F.DecodedScores(buf, 0.5, ids=["unknown"])


def case_errors(dev):
    """Assertion 4."""
    c = case("c")
    by_id, _ = F._events_by_id(c["gt_df"])
    dur = dict(c["dur"])
    nan = c["scores"].copy()
    nan[1, 2, 0] = np.nan
    buf = D.ScoreBuffer()
    buf.append(P.to(dev, torch.from_numpy(nan)), c["ids"], timestamps=c["ts"], event_classes=c["labels"])
    with pytest.raises(ValueError, match="NaN"):
        F.f1_counts(buf, [0.5], by_id, dur)
    buf = fill_buffer(dev, c)
    a0 = c["ids"][0]
    with pytest.raises(ValueError, match="has no score column"):
        F.f1_counts(buf, [0.5], dict(by_id, **{a0: [(0.0, 0.1, "unknown")]}), dur)
    with pytest.raises(ValueError, match="has no score column"):
        EM.log_sedeval_metrics(F.DecodedScores(buf, 0.0), pd.concat([c["gt_df"], pd.DataFrame(
            [("elsewhere.wav", 0.0, 0.1, "unknown")], columns=list(c["gt_df"].columns))], ignore_index=True))
    calls = []
    real = _lib.get().call
    _lib.get().call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        many = [(0.01 * i, 0.01 * i + 0.2, c["labels"][1]) for i in range(F.MAX_EVENTS + 1)]
        with pytest.raises(ValueError, match="more than %d ground-truth events" % F.MAX_EVENTS):
            F.f1_counts(buf, [0.5], dict(by_id, **{a0: many}), dur)
        F.f1_counts(buf, [0.5], dict(by_id, **{a0: many[:-1]}), dur)                           # exactly the limit is served
        assert calls.count("sed_f1_counts") == 1
        with pytest.raises(ValueError, match="more than %d segments" % F.MAX_CELLS):
            F.f1_counts(buf, [0.5], dict(by_id, **{a0: [(0.5, F.MAX_CELLS + 0.001, c["labels"][0])]}), dur)
        with pytest.raises(ValueError, match="more than %d segments" % F.MAX_CELLS):
            F.f1_counts(buf, [0.5], by_id, dur, time_resolution=0.005)             # 7 frames of 64 ms: 90 cells
        assert calls.count("sed_f1_counts") == 1, "the limits must be refused before any launch"
    finally:
        del _lib.get().call
    # beyond the kernel's limits: refused, and the framed output is untouched
    for T, NC, n_thr in ((257, 2, 1), (4, 33, 1), (4, 2, 9)):
        scores = P.to(dev, torch.rand(2, T, NC))
        i32, f64 = dict(dtype=torch.int32), dict(dtype=torch.float64)
        args = (scores, P.to(dev, torch.linspace(0.1, 0.9, n_thr)), P.to(dev, torch.arange(T + 1, **f64) * 0.064),
                P.to(dev, torch.zeros(2 * NC + 1, **i32)), P.to(dev, torch.zeros(1, **f64)), P.to(dev, torch.zeros(1, **f64)),
                P.to(dev, torch.full((2,), 10.0, **f64)))
        frame = Framed(dev, n_thr * 2 * NC, 8, torch.int32)
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            F.f1_counts_kernel(*args, T_COLLAR, PCT, RES, DTC, GTC, CTTC, out=frame.body.view(n_thr, 2, NC, 8))
        sync(dev)
        assert bool((frame.buf.cpu() == CANARY).all()), (T, NC, n_thr)
    # the flag needs its partner
    task = P.build_task(dev, (1, 1, 2), _state_dict(), dropout=0.5, specaug=True, rampup=100)
    task.hparams["training"].update(device_f1=True, device_psds=False)
    with pytest.raises(ValueError, match="training.device_f1 needs training.device_psds"):
        task.validation_epoch_end([])


def _state_dict():
    from oracle import sed_oracle as O
    return O.make_state_dict(seed=7)


# ---- trainer hooks -------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def count_library_calls():
    """Every call into the bound kernel library by name, while the context is open."""
    calls = []
    lib = _lib.get()
    real = lib.call

    def counted(name, *args):
        calls.append(name)
        return real(name, *args)
    lib.call = counted
    try:
        yield calls
    finally:
        del lib.call


VAL_KEYS = ["val/obj_metric"] + ["val/synth/%s/%s" % (who, k) for who in ("student", "teacher") for k in ("event_f1_macro", "intersection_f1_macro")]


def _run_2023(dev, cfg, out_dir, flag, obj_type, test_epoch):
    import yaml
    from oracle import sed_oracle as O
    bs, n_samp = (1, 1, 2), 16000 + 1024
    B = sum(bs)
    n_out = (1 + n_samp // 256) // 4
    data = yaml.safe_load(open(cfg))["data"]
    task = P.build_task(dev, bs, _state_dict(), dropout=0.5, specaug=True, rampup=100)
    task.hparams["data"] = data
    task.hparams["training"].update(val_thresholds=[0.3, 0.5], median_window=7, n_test_thresholds=10, device_psds=True, device_f1=flag,
                                    obj_metric_synth_type=obj_type)
    task.hparams["log_dir"] = out_dir
    task.encoder = P._Encoder(M.DESED_CLASSES, audio_len=n_samp / 16000.0)
    task.eval()
    val = sorted(os.listdir(data["synth_val_folder"]))
    weak = sorted(os.listdir(data["weak_folder"]))
    with count_library_calls() as calls:
        for step in range(2):
            names = ([os.path.join(data["synth_val_folder"], f) for f in val[2 * step:2 * step + 2]]
                     + [os.path.join(data["weak_folder"], f) for f in weak[2 * step:2 * step + 2]])
            audio, labels = O.synth_audio(B, n_samp, seed=21 + step), O.synth_labels(bs, 10, n_out, seed=5 + step)
            task.validation_step((P.to(dev, audio), P.to(dev, labels), None, names, None), step)
    # two models x two steps decode on the device with the flag off; with it on the region kernel never runs
    assert calls.count("sed_threshold_events") == (0 if flag else 4), calls.count("sed_threshold_events")
    assert calls.count("sed_median_filter") == 4
    for buf in (task.val_buffer_student_synth, task.val_buffer_teacher_synth):
        assert sorted(buf) == [0.3, 0.5] and all(df.empty for df in buf.values()) == flag
    assert len(task.val_scores_device_buffer_student) == 4 and len(task.val_scores_device_buffer_teacher) == 4
    with count_library_calls() as calls:
        task.validation_epoch_end([])
    # per model one launch for all thresholds of the intersection F1, and one at 0.5 unless nothing is detected there
    assert (2 <= calls.count("sed_f1_counts") <= 4) if flag else "sed_f1_counts" not in calls, calls
    logged = {k: float(task.logged[k]) for k in VAL_KEYS}
    assert all(df.empty for df in task.val_buffer_student_synth.values()) and len(task.val_scores_device_buffer_student) == 0
    written = []
    if test_epoch:
        names = [os.path.join(data["test_folder"], f) for f in sorted(os.listdir(data["test_folder"]))]
        audio, labels = O.synth_audio(B, n_samp, seed=31), O.synth_labels(bs, 10, n_out, seed=7)
        task.test_step((P.to(dev, audio), P.to(dev, labels), None, names, None), 0)
        res = task.on_test_epoch_end()
        logged.update({k: float(v) for k, v in res.items()})
        written = sorted(os.path.relpath(os.path.join(r, f), out_dir) for r, _, fs in os.walk(out_dir) for f in fs)
    return logged, written


def case_hooks_2023(dev, tmp, obj_type):
    """Assertion 5, 2023 trainer (the pretrained trainer inherits these hooks), both runs with `training.device_psds` on: with
    `training.device_f1` the validation steps launch no region kernel and build no frames, the epoch end logs what it logs without
    the flag, and (obj_type None) the test epoch, which the flag does not touch, logs and writes the same."""
    from tests import mini_desed
    with M._recipe_stand_in(tmp) as recipe:
        cfg = mini_desed.build(tmp, recipe)
    runs = {flag: _run_2023(dev, cfg, os.path.join(tmp, "exp_%d" % flag), flag, obj_type, obj_type is None) for flag in (False, True)}
    (off, files_off), (on, files_on) = runs[False], runs[True]
    assert set(off) == set(on) and set(VAL_KEYS) <= set(on)
    for k in off:
        assert abs(off[k] - on[k]) <= (1e-12 if k in VAL_KEYS else 0.0), (k, off[k], on[k])
    assert files_off == files_on and (obj_type is not None or any("event_f1" in f for f in files_on))
    for rel in files_off:
        a, b = (open(os.path.join(tmp, "exp_%d" % flag, rel), "rb").read() for flag in (0, 1))
        assert a == b, rel


def case_hooks_2024(dev, tmp):
    """Assertion 5, 2024 trainer: the intersection and collar F1 keys of a validation epoch and of a test epoch with
    `training.device_f1` on equal those with it off (both with `training.device_psds` on); every other key does not move."""
    from tests import eval2024_cases as E
    real_task = E._task

    def flagged(f1):
        def make(dev_, n_samp):
            task = real_task(dev_, n_samp)
            task.hparams["training"].update(device_psds=True, device_f1=f1)
            return task
        return make
    keys = (["val/%s/%s_f1_macro_thres05/sed_scores_eval" % (who, k) for who in ("student", "teacher") for k in ("intersection", "collar")]
            + ["test/%s/%s_f1_macro_thres05/sed_scores_eval" % (who, k) for who in ("student", "teacher") for k in ("intersection", "collar")])
    got = {}
    for f1 in (False, True):
        E._task = flagged(f1)
        try:
            with count_library_calls() as calls:
                d = os.path.join(tmp, "v%d" % f1)
                os.makedirs(d)
                val = M._validate_2024(dev, d, True)
                n_val = calls.count("sed_f1_counts")
                d = os.path.join(tmp, "t%d" % f1)
                os.makedirs(d)
                res = E.case_test_2024(dev, d)
        finally:
            E._task = real_task
        n_test = calls.count("sed_f1_counts") - n_val
        assert (2 <= n_val <= 4 and 2 <= n_test <= 4) if f1 else (n_val, n_test) == (0, 0), (n_val, n_test)
        got[f1] = dict(val, **{k: float(v) for k, v in res.items()})
    assert set(keys) <= set(got[True]) and any(got[False][k] > 0 for k in keys)
    for k in got[False]:
        a, b = got[False][k], got[True][k]
        assert (abs(a - b) <= 1e-12) if k in keys else (a == b or (np.isnan(a) and np.isnan(b))), (k, a, b)
