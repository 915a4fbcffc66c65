#!/usr/bin/env python3
"""Decode cost of the 2024 recipe's validation / test batch on one MI355X: HIP-event times at batch_size_val
24 x 156 frames x 27 classes with the recipe's class-wise windows (confs/pretrained.yaml net.median_filter) of
  * sed_median_filter_classwise (one launch);
  * postprocess.batched_decode_preds(median_filter=ClassWiseMedianFilter) as validation calls it (no thresholds) and as the test
    step calls it (n_test_thresholds 50 + 0.5), host table assembly included;
  * the reference's per-clip host loop: ClassWiseMedianFilter (scipy) on each clip's (156, 27) array, after one device->host copy;
  * sed_segment_scores mode 0 (10 s clips -> 10 segments).
Prints one JSON line: the median over `--reps` repetitions after `--warmup`, in milliseconds.

    python tools/eval2024_timing.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from desed_task_amd import postprocess as PP  # noqa: E402

RECIPE_WINS = [3, 9, 9, 5, 5, 5, 9, 7, 11, 9, 7, 3, 9, 13, 7, 1, 13, 3, 13, 7, 5, 5, 1, 13, 17, 13, 15]


class _Encoder:
    labels = ["c%02d" % c for c in range(27)]

    @staticmethod
    def _frame_to_time(frame):
        return np.clip(frame * 4 / (16000 / 256), 0, 10.0)


def _events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    strong = torch.rand(24, 27, 156, generator=g).to(dev)                 # (B, NC, T) as the model returns it
    scores = strong.transpose(1, 2).contiguous()
    filt = PP.ClassWiseMedianFilter(RECIPE_WINS)
    files = ["/d/v/clip%02d.wav" % j for j in range(24)]
    enc = _Encoder()
    n = 50
    test_ths = list(np.arange(1 / (n * 2), 1, 1 / n)) + [0.5]
    lens = torch.full((24,), 10.0)
    out = {"shape": [24, 156, 27], "windows": RECIPE_WINS, "reps": args.reps}
    out["classwise_filter_kernel_ms"] = _events(lambda: PP.median_filter_classwise(scores, filt), args.reps, args.warmup)
    out["segment_kernel_ms"] = _events(lambda: PP.segment_scores(scores, lens, 0.064, 1.0, n_seg=10), args.reps, args.warmup)
    out["decode_validation_ms"] = _events(lambda: PP.batched_decode_preds(strong, files, enc, thresholds=[], median_filter=filt),
                                          args.reps, args.warmup)
    out["decode_test_51_thresholds_ms"] = _events(
        lambda: PP.batched_decode_preds(strong, files, enc, thresholds=test_ths, median_filter=filt), max(5, args.reps // 5), 2)

    def host_loop():
        x = strong.detach().cpu().numpy()
        for j in range(x.shape[0]):
            filt(x[j].T)
    out["host_scipy_filter_loop_ms"] = _events(host_loop, args.reps, args.warmup)
    t0 = time.perf_counter()
    host_loop()
    out["host_scipy_filter_loop_wall_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
