#!/usr/bin/env python
"""Collar / segment / intersection F1: the device path (evaluation/f1_device.py, `sed_f1_counts`) against the host path
(evaluation_measures.log_sedeval_metrics, compute_per_intersection_macro_f1) on synthetic validation sets of the recipe's shape.

    python tools/bench_f1.py [--out FILE.json] [--md profiles/f1_device.md] [--clips 2500 1168]

One driver process; every step that opens the GPU is a child process under its own `timeout`, and the driver stops at the first
step that fails.  Steps, per set size:
    device   kernel time of sed_f1_counts (HIP events, median of 20 launches, one and three thresholds) and wall time of the two
             whole calls on DecodedScores (median of 5)
    host     the two host functions on the frames batched_decode_preds built from the same scores, one run each -- and the values
             side by side
    split    (largest set only) the components of a 2023 `validation_epoch_end` with training.device_f1 off and on, both with
             training.device_psds on, and what a validation step spends on decoding with and without the flag
The workload is bench_psds.py's (seeded): 1-4 off-grid ground-truth events per clip, 156 frames x 10 classes, scores = uniform noise
raised inside the events, through the median filter (window 7) of batched_decode_preds; val_thresholds = [0.5] as in the recipe's
default.yaml.  Prints one JSON document; --md also writes the tables as Markdown."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("bench_psds", os.path.join(ROOT, "tools", "bench_psds.py"))
bench_psds = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench_psds)
T, NC, BATCH, _Encoder, _median = bench_psds.T, bench_psds.NC, bench_psds.BATCH, bench_psds._Encoder, bench_psds._median
F1_KW = dict(t_collar=0.2, percentage_of_length=0.2, time_resolution=1.0, dtc=0.5, gtc=0.5, cttc=0.3)


def _tsvs(tmp, gt, dur):
    import pandas as pd
    tsv, dur_tsv = os.path.join(tmp, "gt.tsv"), os.path.join(tmp, "dur.tsv")
    pd.DataFrame([(a + ".wav", o, f, l) for a, ev in gt.items() for o, f, l in ev],
                 columns=["filename", "onset", "offset", "event_label"]).to_csv(tsv, sep="\t", index=False)
    pd.DataFrame([(a + ".wav", d) for a, d in dur.items()], columns=["filename", "duration"]).to_csv(dur_tsv, sep="\t", index=False)
    return tsv, dur_tsv


def _timed(fn, n=1):
    import torch
    out, value = [], None
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out, value


def step_device(n_clips):
    import torch
    from desed_task_amd.evaluation import f1_device as F
    from desed_task_amd.evaluation import psds_device as D
    from desed_task_amd.evaluation.evaluation_measures import compute_per_intersection_macro_f1, log_sedeval_metrics
    buf, _, _, gt, dur = bench_psds.workload(n_clips, tables=False)
    out = {"clips": n_clips}
    ids = list(buf)
    scores = buf.rows(ids)
    ev = D._event_table_on(D._event_table(gt, ids, buf.event_classes), scores.device)
    ts = torch.from_numpy(buf.timestamps).cuda()
    durs = torch.tensor([dur[a] for a in ids], dtype=torch.float64).cuda()
    for n_thr, ths in ((1, [0.5]), (3, [0.3, 0.5, 0.7])):
        thr = torch.tensor(ths, dtype=torch.float32).cuda()
        args = (scores, thr, ts) + ev + (durs,) + tuple(F1_KW.values())
        counts = F.f1_counts_kernel(*args)
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            F.f1_counts_kernel(*args, out=counts)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out["kernel_%d_thr" % n_thr] = {"ms_median_of_20": _median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    with tempfile.TemporaryDirectory() as tmp:
        tsv, dur_tsv = _tsvs(tmp, gt, dur)
        dec = F.DecodedScores(buf, 0.5)
        D._EVENT_TABLES.clear()
        first, _ = _timed(lambda: log_sedeval_metrics(dec, tsv))
        wall, value = _timed(lambda: log_sedeval_metrics(dec, tsv), 5)
        out["log_sedeval_metrics"] = {"call_ms_median_of_5": _median(wall) * 1e3, "call_ms_min": min(wall) * 1e3, "call_ms_max": max(wall) * 1e3,
                                      "call_ms_first_with_event_table_build": first[0] * 1e3, "value": list(value)}
        wall, value = _timed(lambda: compute_per_intersection_macro_f1({0.5: dec}, tsv, dur_tsv), 5)
        out["compute_per_intersection_macro_f1"] = {"call_ms_median_of_5": _median(wall) * 1e3, "call_ms_min": min(wall) * 1e3,
                                                    "call_ms_max": max(wall) * 1e3, "value": float(value)}
    return out


def step_host(n_clips):
    from desed_task_amd.evaluation.evaluation_measures import compute_per_intersection_macro_f1, log_sedeval_metrics
    buf, _, decoded, gt, dur = bench_psds.workload(n_clips, tables=False)
    out = {"clips": n_clips, "detections": len(decoded)}
    with tempfile.TemporaryDirectory() as tmp:
        tsv, dur_tsv = _tsvs(tmp, gt, dur)
        wall, value = _timed(lambda: log_sedeval_metrics(decoded, tsv))
        out["log_sedeval_metrics"] = {"host_s_one_run": wall[0], "value": list(value)}
        wall, value = _timed(lambda: compute_per_intersection_macro_f1({0.5: decoded}, tsv, dur_tsv))
        out["compute_per_intersection_macro_f1"] = {"host_s_one_run": wall[0], "value": float(value)}
    return out


def step_split(n_clips):
    """The calls of SEDTask4.validation_epoch_end (2023), one by one, on one model's buffers, with training.device_psds on: the two F1
    functions on the decoded frames (device_f1 off) and on DecodedScores (on); and one validation step's decoding of a batch."""
    import torch
    from desed_task_amd.evaluation.evaluation_measures import (compute_per_intersection_macro_f1, compute_psds_from_scores,
                                                               log_sedeval_metrics)
    from desed_task_amd.evaluation.f1_device import DecodedScores
    from desed_task_amd.evaluation.psds_device import ScoreBuffer
    from desed_task_amd.postprocess import batched_decode_preds
    buf, _, decoded, gt, dur = bench_psds.workload(n_clips, tables=False)
    out = {"clips": n_clips}
    with tempfile.TemporaryDirectory() as tmp:
        tsv, dur_tsv = _tsvs(tmp, gt, dur)
        kw = bench_psds.SCENARIOS["scenario1"]
        compute_psds_from_scores(buf, gt, dur, **kw)
        out["psds1_sed_scores_eval_s"] = _timed(lambda: compute_psds_from_scores(buf, gt, dur, **kw))[0][0]
        out["intersection_f1_flag_off_s"] = _timed(lambda: compute_per_intersection_macro_f1({0.5: decoded}, tsv, dur_tsv))[0][0]
        out["event_f1_flag_off_s"] = _timed(lambda: log_sedeval_metrics(decoded, tsv))[0][0]
        dec = {0.5: DecodedScores(buf, 0.5)}
        compute_per_intersection_macro_f1(dec, tsv, dur_tsv)
        out["intersection_f1_flag_on_s"] = _median(_timed(lambda: compute_per_intersection_macro_f1(dec, tsv, dur_tsv), 5)[0])
        out["event_f1_flag_on_s"] = _median(_timed(lambda: log_sedeval_metrics(dec[0.5], tsv), 5)[0])
        out["note"] = "validation_epoch_end runs the intersection and event F1 twice (student, teacher) and the PSDS once"
        for flag in ("off", "on"):
            out["epoch_end_flag_%s_s" % flag] = out["psds1_sed_scores_eval_s"] + 2 * (out["intersection_f1_flag_%s_s" % flag]
                                                                                     + out["event_f1_flag_%s_s" % flag])
    # one validation step's post-processing of one model's batch: filter + regions + copy + frame against filter only
    g = torch.Generator().manual_seed(7)
    strong = torch.rand(BATCH, NC, T, generator=g).cuda()
    files = ["/synth_val/b%02d.wav" % i for i in range(BATCH)]
    for name, ths in (("off", [0.5]), ("on", [])):
        fn = lambda: batched_decode_preds(strong, files, _Encoder, thresholds=ths, median_filter=7, device_scores=ScoreBuffer())      # noqa: E731
        fn()
        out["decode_step_flag_%s_ms" % name] = _median(_timed(fn, 20)[0]) * 1e3
    out["validation_batches"] = -(-n_clips // BATCH)
    return out


STEPS = {"device": (step_device, 240), "host": (step_host, 300), "split": (step_split, 420)}


def markdown(doc):
    by = {}
    for s in doc["steps"]:
        by[s["step"], s["clips"]] = s
    sizes = sorted({n for _, n in by}, reverse=True)
    L = ["# Collar, segment and intersection F1: device path against host path", "",
         "`python tools/bench_f1.py --md profiles/f1_device.md`, one single-GPU MI355X box, one run, library source revision `%s`"
         % doc["source_rev"],
         "(`desed_task_amd.build.source_rev()`).  The workload is `tools/bench_psds.py`'s: seeded validation sets of the recipe's shape, %d"
         % doc["frames"],
         "frames x %d classes, 1-4 off-grid ground-truth events per clip, median-filtered (window 7) on the device, decoded at 0.5.  Every"
         % doc["classes"],
         "GPU step ran as its own process under its own time limit.  The host figures are the host functions (the path this feature",
         "leaves unchanged and the default) on the frames `batched_decode_preds` built, on the same box, ONE run each; the device figures",
         "are medians with their range.", "", "## Kernel", "",
         "| clips | thresholds | `sed_f1_counts`, HIP events, median of 20 (min - max) |", "|---|---|---|"]
    for n in sizes:
        d = by.get(("device", n))
        for k in (1, 3):
            if d:
                v = d["kernel_%d_thr" % k]
                L.append("| %d | %d | %.3f ms (%.3f - %.3f) |" % (n, k, v["ms_median_of_20"], v["ms_min"], v["ms_max"]))
    L += ["", "## Whole calls", "",
          "| clips | function | on `DecodedScores`, wall, median of 5 (min - max) | first call (builds the event table) | host, one run | value device | value host |",
          "|---|---|---|---|---|---|---|"]
    for n in sizes:
        d, h = by.get(("device", n)), by.get(("host", n))
        if not (d and h):
            continue
        for fn in ("log_sedeval_metrics", "compute_per_intersection_macro_f1"):
            v, w = d[fn], h[fn]
            first = "%.1f ms" % v["call_ms_first_with_event_table_build"] if "call_ms_first_with_event_table_build" in v else "-"
            L.append("| %d | `%s` | %.1f ms (%.1f - %.1f) | %s | %.3f s | %s | %s |"
                     % (n, fn, v["call_ms_median_of_5"], v["call_ms_min"], v["call_ms_max"], first, w["host_s_one_run"], v["value"], w["value"]))
    s = next((by[k] for k in by if k[0] == "split"), None)
    if s:
        L += ["", "## A 2023 `validation_epoch_end`, by component (%d clips, one model's buffers, `training.device_psds: True` in both columns)"
              % s["clips"], "", "| component | `device_f1` off | `training.device_f1: True` |", "|---|---|---|",
              "| `compute_psds_from_scores` (scenario 1, student, on the ScoreBuffer) | %.3f s | %.3f s |" % ((s["psds1_sed_scores_eval_s"],) * 2),
              "| `compute_per_intersection_macro_f1` (one threshold), per model | %.3f s | %.3f s |"
              % (s["intersection_f1_flag_off_s"], s["intersection_f1_flag_on_s"]),
              "| `log_sedeval_metrics` (event-based F1), per model | %.3f s | %.3f s |" % (s["event_f1_flag_off_s"], s["event_f1_flag_on_s"]),
              "| sum as the hook runs them (PSDS once, the two F1s for student and teacher) | %.3f s | %.3f s |"
              % (s["epoch_end_flag_off_s"], s["epoch_end_flag_on_s"]),
              "| `batched_decode_preds` of one validation batch (%d clips), per model and step (median of 20) | %.2f ms | %.2f ms |"
              % (BATCH, s["decode_step_flag_off_ms"], s["decode_step_flag_on_ms"]),
              "", "The flag-off F1 figures are one run each, the flag-on ones medians of 5.  A validation epoch at this size has %d batches, each"
              % s["validation_batches"], "decoded for two models."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, nargs="+", default=[2500, 1168])
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None, help="also write the tables as Markdown to this file")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "bench_f1.py measures on the GPU: there is no CPU path"
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
    for path, body in ((a.out, text + "\n"), (a.md, None if "failed" in doc else markdown(doc))):
        if path and body:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 1 if "failed" in doc else 0


if __name__ == "__main__":
    sys.exit(main())
