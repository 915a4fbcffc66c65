#!/usr/bin/env python
"""Threshold-free PSDS: the device path (evaluation/psds_device.py, `sed_psds_steps`) against the host path
(evaluation/psds_scores.py) on synthetic validation sets of the recipe's shape.

    python tools/bench_psds.py [--out FILE.json] [--clips 2500 1168]

One driver process; every step that opens the GPU is a child process under its own `timeout`, and the driver stops at the first
step that fails.  Steps, per set size:
    device   kernel time of sed_psds_steps (HIP events, median of 20 launches) and wall time of the whole
             psds_from_score_buffer call (median of 5), scenario 1 and 2
    host     psds_from_scores on the same scores, one run per scenario -- and the two values side by side
    split    (largest set only) the components of a 2023 `validation_epoch_end`, with training.device_psds off and on
The workload is seeded: 1-4 off-grid ground-truth events per clip, 156 frames x 10 classes, scores = uniform noise raised inside
the events, through the median filter (window 7) of batched_decode_preds.  Prints one JSON document."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T, NC, BATCH = 156, 10, 24
SCENARIOS = {"scenario1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0, alpha_st=1),
             "scenario2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1)}


class _Encoder:
    """The two members of the recipe's ManyHotEncoder that batched_decode_preds touches (10 s clips, 64 ms frames)."""
    labels = ["c%02d" % i for i in range(NC)]

    @staticmethod
    def _frame_to_time(frame):
        import numpy as np
        return np.clip(frame * 4 / (16000 / 256), a_min=0, a_max=10)


def workload(n_clips, tables):
    """-> (ScoreBuffer, score tables or None, decoded events at 0.5, ground truth, durations), seeded."""
    import numpy as np
    import pandas as pd
    import torch
    from desed_task_amd.evaluation.psds_device import ScoreBuffer
    from desed_task_amd.postprocess import batched_decode_preds
    rng = np.random.RandomState(2023)
    g = torch.Generator().manual_seed(2023)
    ids = ["clip%05d" % i for i in range(n_clips)]
    gt = {}
    for i in ids:
        ev = []
        for _ in range(rng.randint(1, 5)):
            on = float(rng.uniform(0.0, 8.0))
            ev.append((on, min(on + float(rng.uniform(0.3, 4.0)), 10.0), _Encoder.labels[rng.randint(NC)]))
        gt[i] = ev
    buf, post, decoded = ScoreBuffer(), {}, []
    for a in range(0, n_clips, BATCH):
        # a detector that is right more often than not: uniform noise in [0, 0.65), raised by 0.35 inside the events
        strong = 0.65 * torch.rand(min(BATCH, n_clips - a), NC, T, generator=g)
        for j, i in enumerate(ids[a:a + BATCH]):
            for on, off, label in gt[i]:
                strong[j, _Encoder.labels.index(label), int(on / 0.064):int(off / 0.064) + 1] += 0.35
        strong = strong.cuda()
        files = ["/synth_val/%s.wav" % i for i in ids[a:a + BATCH]]
        _, _, dfs = batched_decode_preds(strong, files, _Encoder, thresholds=[0.5], median_filter=7, device_scores=buf)
        decoded.append(dfs[0.5])
        if tables:
            post.update(batched_decode_preds(strong, files, _Encoder, thresholds=[], median_filter=7)[1])
    return buf, (post if tables else None), pd.concat(decoded, ignore_index=True), gt, {i: 10.0 for i in ids}


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def step_device(n_clips):
    import torch
    from desed_task_amd.evaluation import psds_device as D
    buf, _, _, gt, dur = workload(n_clips, tables=False)
    out = {"clips": n_clips}
    for name, kw in SCENARIOS.items():
        # the kernel alone, on the inputs the call hands it
        ids = sorted(gt)
        scores = buf.rows(ids)
        table = D._event_table(gt, ids, buf.event_classes)
        ev = D._event_table_on(table, scores.device)
        ts = torch.from_numpy(buf.timestamps).cuda()
        durs = torch.tensor([dur[a] for a in ids], dtype=torch.float64).cuda()
        use_ct = kw["cttc_threshold"] is not None and kw["alpha_ct"] > 0
        args = (scores, ts) + ev + (durs, kw["dtc_threshold"], kw["gtc_threshold"], kw["cttc_threshold"], use_ct)
        steps = D.psds_steps(*args)
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            D.psds_steps(*args, out=steps)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        D.psds_from_score_buffer(buf, gt, dur, **kw)                  # warm: event table cached, as from the second epoch on
        wall = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value = D.psds_from_score_buffer(buf, gt, dur, **kw)[0]
            wall.append((time.perf_counter() - t0) * 1e3)
        # where one call spends its time: the per-class merge (device sort + cumulative sum + the copy of the kept operating points,
        # which synchronises) against everything else (gather, launch, the shared numpy tail)
        merge, real_merge = [0.0], D._merged_counts

        def timed_merge(*a, **k):
            t = time.perf_counter()
            r = real_merge(*a, **k)
            merge[0] += (time.perf_counter() - t) * 1e3
            return r
        D._merged_counts = timed_merge
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            D.psds_from_score_buffer(buf, gt, dur, **kw)
            split_total = (time.perf_counter() - t0) * 1e3
        finally:
            D._merged_counts = real_merge
        D._EVENT_TABLES.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.psds_from_score_buffer(buf, gt, dur, **kw)
        cold = (time.perf_counter() - t0) * 1e3
        out[name] = {"kernel_ms_median_of_20": _median(ms), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                     "call_ms_median_of_5": _median(wall), "call_ms_min": min(wall), "call_ms_max": max(wall),
                     "call_ms_first_with_event_table_build": cold, "psds": value,
                     "one_call_split_ms": {"total": split_total, "merge_and_copy": merge[0], "rest_incl_shared_tail": split_total - merge[0]}}
    return out


def step_host(n_clips):
    from desed_task_amd.evaluation.psds_device import psds_from_score_buffer
    from desed_task_amd.evaluation.psds_scores import psds_from_scores
    buf, _, _, gt, dur = workload(n_clips, tables=False)
    t0 = time.perf_counter()
    tables = buf.to_tables()
    out = {"clips": n_clips, "to_tables_s": time.perf_counter() - t0}
    for name, kw in SCENARIOS.items():
        t0 = time.perf_counter()
        value = psds_from_scores(tables, gt, dur, **kw)[0]
        out[name] = {"host_s_one_run": time.perf_counter() - t0, "psds_host": value,
                     "psds_device": psds_from_score_buffer(buf, gt, dur, **kw)[0]}
        out[name]["abs_difference"] = abs(out[name]["psds_host"] - out[name]["psds_device"])
    return out


def step_split(n_clips):
    """The calls of SEDTask4.validation_epoch_end (2023), one by one, on one model's buffers: the threshold-free PSDS from the
    tables (flag off) and from the device buffer (flag on), then what both settings share."""
    import pandas as pd
    import torch
    from desed_task_amd.evaluation.evaluation_measures import (compute_per_intersection_macro_f1, compute_psds_from_scores,
                                                               log_sedeval_metrics)
    buf, tables, decoded, gt, dur = workload(n_clips, tables=True)
    out = {"clips": n_clips}
    with tempfile.TemporaryDirectory() as tmp:
        tsv, dur_tsv = os.path.join(tmp, "gt.tsv"), os.path.join(tmp, "dur.tsv")
        pd.DataFrame([(a + ".wav", o, f, l) for a, ev in gt.items() for o, f, l in ev],
                     columns=["filename", "onset", "offset", "event_label"]).to_csv(tsv, sep="\t", index=False)
        pd.DataFrame([(a + ".wav", d) for a, d in dur.items()], columns=["filename", "duration"]).to_csv(dur_tsv, sep="\t", index=False)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        kw = SCENARIOS["scenario1"]
        out["psds1_sed_scores_eval_flag_off_s"] = timed(lambda: compute_psds_from_scores(tables, gt, dur, **kw))
        compute_psds_from_scores(buf, gt, dur, **kw)
        out["psds1_sed_scores_eval_flag_on_s"] = timed(lambda: compute_psds_from_scores(buf, gt, dur, **kw))
        out["intersection_f1_student_s"] = timed(lambda: compute_per_intersection_macro_f1({0.5: decoded}, tsv, dur_tsv))
        out["event_f1_student_s"] = timed(lambda: log_sedeval_metrics(decoded, tsv))
        out["note"] = "validation_epoch_end runs the intersection and event F1 twice (student, teacher) and the PSDS once"
        shared = 2 * (out["intersection_f1_student_s"] + out["event_f1_student_s"])
        out["epoch_end_flag_off_s"] = out["psds1_sed_scores_eval_flag_off_s"] + shared
        out["epoch_end_flag_on_s"] = out["psds1_sed_scores_eval_flag_on_s"] + shared
    return out


STEPS = {"device": (step_device, 240), "host": (step_host, 420), "split": (step_split, 540)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, nargs="+", default=[2500, 1168])
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "bench_psds.py measures on the GPU: there is no CPU path"
        print("RESULT " + json.dumps(STEPS[a.step][0](a.clips[0])), flush=True)
        return 0
    from desed_task_amd import build
    doc = {"source_rev": build.source_rev(), "frames": T, "classes": NC, "steps": []}
    plan = [(s, n) for n in a.clips for s in ("device", "host")] + [("split", max(a.clips))]
    for step, n in plan:
        limit = STEPS[step][1]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--clips", str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            doc["failed"] = {"step": step, "clips": n, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            break                                               # nothing more is started on the GPU after a failure
        doc["steps"].append(dict(json.loads(lines[-1][7:]), step=step))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 1 if "failed" in doc else 0


if __name__ == "__main__":
    sys.exit(main())
