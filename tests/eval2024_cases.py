"""Cases of the 2024 recipe's validation / test path shared by the CPU (emulator, tests/test_eval_2024.py) and GPU
(tests/test_gpu_eval_2024.py) suites: the class-wise median filter and segment kernels against the reference fixture
(golden/golden_post2024.npz), and the 2024 trainer's validation / test hooks end to end on a miniature in-memory set."""
import copy
import os

import numpy as np
import pandas as pd
import torch

from oracle import sed_oracle as O
from tests import parity_cases as P

HERE = os.path.dirname(os.path.abspath(__file__))
# recipes/dcase2024_task4_baseline/confs/pretrained.yaml net.median_filter (also recorded in the fixture as wins_recipe)
RECIPE_WINS = [3, 9, 9, 5, 5, 5, 9, 7, 11, 9, 7, 3, 9, 13, 7, 1, 13, 3, 13, 7, 5, 5, 1, 13, 17, 13, 15]
VAL_KEYS = {"val/weak/student/loss_weak", "val/weak/teacher/loss_weak", "val/synth/student/loss_strong",
            "val/synth/teacher/loss_strong"}
EPOCH_KEYS = {"val/obj_metric", "val/student/weak_f1_macro_thres05/torchmetrics", "val/teacher/weak_f1_macro_thres05/torchmetrics",
              "val/student/intersection_f1_macro_thres05/sed_scores_eval", "val/teacher/intersection_f1_macro_thres05/sed_scores_eval",
              "val/student/collar_f1_macro_thres05/sed_scores_eval", "val/teacher/collar_f1_macro_thres05/sed_scores_eval",
              "val/student/psds1/sed_scores_eval", "val/teacher/psds1/sed_scores_eval",
              "val/student/segment_f1_macro_thresopt/sed_scores_eval", "val/student/segment_mauc/sed_scores_eval",
              "val/student/segment_mpauc/sed_scores_eval", "val/teacher/segment_f1_macro_thresopt/sed_scores_eval",
              "val/teacher/segment_mauc/sed_scores_eval", "val/teacher/segment_mpauc/sed_scores_eval"}
TEST_KEYS = {"test/%s/%s" % (who, k) for who in ("student", "teacher") for k in (
    "psds1/psds_eval", "psds2/psds_eval", "intersection_f1_macro_thres05/psds_eval", "collar_f1_macro_thres05/sed_eval",
    "psds1/sed_scores_eval", "psds2/sed_scores_eval", "intersection_f1_macro_thres05/sed_scores_eval",
    "collar_f1_macro_thres05/sed_scores_eval", "segment_f1_macro_thresopt/sed_scores_eval", "segment_mauc/sed_scores_eval",
    "segment_mpauc/sed_scores_eval")}
DESED = ["d%02d" % i for i in range(10)]
MAESTRO = ["m%02d" % i for i in range(17)]


def golden():
    return np.load(os.path.join(HERE, "golden", "golden_post2024.npz"))


def codes_to_scores(codes):
    return codes.astype(np.float32) / np.float32(255)


def case_kernels_vs_fixture(dev, G):
    """Both kernels at the recipe's shape (batch_size_val 24 x 156 frames x 27 classes) against the reference's outputs."""
    from desed_task_amd import postprocess as PP
    x = codes_to_scores(G["x_codes"])
    assert list(G["wins_recipe"]) == RECIPE_WINS
    for xs, wins, ref in ((x, G["wins_recipe"], G["med_recipe"]), (x[:4], G["wins_wide"], G["med_wide"]),
                          (x[:3, :5], G["wins_short"], G["med_short"])):
        y = PP.median_filter_classwise(P.to(dev, torch.from_numpy(np.ascontiguousarray(xs))), list(wins)).cpu().numpy()
        assert np.array_equal(y, codes_to_scores(ref)), "class-wise median filter differs from the reference"
    seg = PP.segment_scores(P.to(dev, torch.from_numpy(x)), G["seg_clip_len"], 0.064, 1.0, mode=0).cpu().numpy()
    assert seg.shape == (24, 10, 27)
    assert np.abs(seg - G["seg_mean"]).max() <= 1e-6
    # mode 1: the maximum over the frames overlapping [k, min(k + 1, clip_len)) with positive length
    mx = PP.segment_scores(P.to(dev, torch.from_numpy(x)), G["seg_clip_len"], 0.064, 1.0, mode=1).cpu().numpy()
    t = np.arange(157) * 0.064
    for b in range(24):
        n = int(np.ceil(G["seg_clip_len"][b]))
        for k in range(10):
            if k >= n:
                assert (mx[b, k] == 0).all()
                continue
            sel = (t[1:] > k) & (t[:-1] < min(k + 1.0, G["seg_clip_len"][b]))
            assert np.array_equal(mx[b, k], x[b, sel].max(0))


def case_host_filter_equivalence(dev, B=48, T=156, NC=27, seed=3):
    """Windows up to 31 (odd and even) at B = 48, and windows up to 16 / 64 with up to 40 classes, against the host
    ClassWiseMedianFilter, bit-exact; and batched_decode_preds(median_filter=ClassWiseMedianFilter) against the per-clip host loop."""
    from desed_task_amd import postprocess as PP
    rng = np.random.default_rng(seed)
    x = rng.random((B, T, NC), dtype=np.float32)
    x[:, ::4] = np.round(x[:, ::4] * 8) / 8                                    # ties
    wins = [int(w) for w in rng.integers(1, 32, size=NC)]
    wins[0], wins[1] = 31, 2
    filt = PP.ClassWiseMedianFilter(wins)
    y = PP.median_filter_classwise(P.to(dev, torch.from_numpy(x)), filt).cpu().numpy()
    ref = np.stack([filt(x[b]) for b in range(B)])
    assert np.array_equal(y, ref)
    # every sort tier (N = 16 / 32 / 64 slots, chosen by the largest window), more than one 32-class block, T < w
    for nc, w_hi, t in ((27, 16, T), (40, 64, T), (40, 33, 7), (35, 12, 1)):
        xt = rng.random((6, t, nc), dtype=np.float32)
        xt[:, ::3] = np.round(xt[:, ::3] * 8) / 8
        wt = [int(w) for w in rng.integers(1, w_hi + 1, size=nc)]
        wt[-1] = w_hi
        ft = PP.ClassWiseMedianFilter(wt)
        yt = PP.median_filter_classwise(P.to(dev, torch.from_numpy(xt)), ft).cpu().numpy()
        assert np.array_equal(yt, np.stack([ft(xt[b]) for b in range(6)])), (nc, w_hi, t)
    with np_raises(RuntimeError):
        PP.median_filter_classwise(P.to(dev, torch.from_numpy(x[:1])), [65] + [3] * (NC - 1))   # past the kernel's window
    # decoding: the device filter vs the same filter run per clip on the host (a plain callable takes the host path)
    enc = P._Encoder(["c%02d" % c for c in range(NC)], audio_len=10.0)
    strong = P.to(dev, torch.from_numpy(x[:8]).transpose(1, 2))               # (B, NC, T) as the model returns it
    files = ["/d/x/a%d.wav" % j for j in range(8)]
    dev_out = PP.batched_decode_preds(strong, files, enc, thresholds=[0.3, 0.5], median_filter=filt)
    host_out = PP.batched_decode_preds(strong, files, enc, thresholds=[0.3, 0.5], median_filter=lambda a: filt(a))
    for d, h in zip(dev_out[:2], host_out[:2]):
        assert d.keys() == h.keys() and all(d[k].equals(h[k]) for k in d)
    for th in (0.3, 0.5):
        assert dev_out[2][th].equals(host_out[2][th]) and len(dev_out[2][th]) > 0
    raw, post, dec = PP.batched_decode_preds(strong, files, enc, thresholds=[], median_filter=None)
    assert dec == {} and all(raw[k].equals(post[k]) for k in raw)


class np_raises:
    def __init__(self, exc):
        self.exc = exc

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, self.exc), "expected %s" % self.exc
        return True


def _decode(arr, ts, classes, th=0.5):
    """(label, onset s, offset s) of the regions of `arr > th` per column (the ground truth the model's own scores earn)."""
    rows = []
    for c, on, off in O.decode_events(arr.astype(np.float32), np.float32(th)):
        rows.append((classes[c], float(ts[on]), float(ts[off])))
    return rows


def _task(dev, n_samp):
    task = P.build_task_2024(dev, bs=(1, 1, 1, 1, 1), dropout=0.0, dropstep=0.0)
    task.eval()
    task.encoder = P._Encoder(DESED + MAESTRO, audio_len=n_samp / 16000.0)
    from desed_task_amd.postprocess import ClassWiseMedianFilter
    task.median_filter = ClassWiseMedianFilter(RECIPE_WINS)
    return task


def _batch(dev, files, n_samp, te, seed):
    B = len(files)
    audio = O.synth_audio(B, n_samp, seed=seed)
    n_out = (1 + n_samp // 256) // 4
    labels = (O.lcg_fill((B, 27, n_out), seed + 1, 0.5, 0.5) < 0.1).float()
    emb = O.lcg_fill((B, 768, te), seed + 2, 1.0)
    valid = torch.zeros(B, 27, dtype=torch.bool)
    for j, f in enumerate(files):
        valid[j, 10:] = "maestro" in f
        valid[j, :10] = "maestro" not in f
    return audio, labels, emb, valid, (P.to(dev, audio), P.to(dev, labels), None, files, P.to(dev, emb), P.to(dev, valid))


def case_validation_2024(dev, tmp, n_samp=16000 * 2 + 1024, te=53, check_oracle=True):
    """validation_step + validation_epoch_end of the 2024 trainer: posteriors vs the oracle's eval-mode forward, score tables vs
    the host filter of the task's own posteriors, the logged key sets, the objective recomputed from the buffers, and perfect
    intersection / collar / segment F1 when the ground truth is the 0.5 decoding of the model's own scores."""
    from desed_task_amd.evaluation import segment_based
    from desed_task_amd.evaluation.evaluation_measures import compute_psds_from_scores
    from desed_task_amd.postprocess import ClassWiseMedianFilter
    task = _task(dev, n_samp)
    files = (["/d/synth_val/s%d.wav" % i for i in range(3)] + ["/d/maestro_train/m%d.wav" % i for i in range(3)]
             + ["/d/weak/w%d.wav" % i for i in range(2)] + ["/d/other/u0.wav"])
    task.hparams["data"] = {"weak_folder": "/d/weak", "synth_val_folder": "/d/synth_val/", "real_maestro_train_folder": "/d/maestro_train"}
    audio, labels, emb, valid, batch = _batch(dev, files, n_samp, te, seed=41)
    task.validation_step(batch, 0)
    assert set(task.logged) == VAL_KEYS
    strong_own = task._eval_forward(batch[0], batch[4], batch[5])[0].transpose(1, 2).cpu().numpy()        # (B, T, NC)
    filt = ClassWiseMedianFilter(RECIPE_WINS)
    strong_ids = [os.path.basename(f)[:-4] for f in files[:6]]
    assert set(task.val_buffer_sed_scores_eval_student) == set(strong_ids)
    for j, aid in enumerate(strong_ids):
        tab = task.val_buffer_sed_scores_eval_student[aid]
        assert list(tab.columns) == ["onset", "offset"] + DESED + MAESTRO
        assert np.array_equal(tab.values[:, 2:].astype(np.float32), filt(strong_own[j]))       # device filter == host filter
    if check_oracle:
        feats = O.scale_minmax(O.take_log(O.mel_spectrogram(audio)))
        sd = {k: v.detach().cpu() for k, v in task.sed_student.state_dict().items()}
        strong_o, weak_o = O.crnn_forward(sd, feats, training=False, embeddings=emb, classes_mask=valid)
        assert np.abs(strong_own - strong_o.transpose(1, 2).numpy()).max() < 1e-3
        lw = (labels[6:8].sum(-1) >= 1).float()
        ref_w = torch.nn.functional.binary_cross_entropy(weak_o[6:8], lw).item()
        assert abs(float(task.logged["val/weak/student/loss_weak"]) - ref_w) < 1e-3
    # ---- ground truth = the 0.5 decoding of the student's own post-processed scores ----
    ts = task.encoder._frame_to_time(np.arange(strong_own.shape[1] + 1))
    dur = n_samp / 16000.0
    synth_rows, maestro_rows, maestro_classes = [], [], set()
    for aid in strong_ids:
        arr = task.val_buffer_sed_scores_eval_student[aid].values[:, 2:]
        if aid.startswith("s"):
            ev = _decode(arr[:, :10], ts, DESED)
            synth_rows += [(aid + ".wav", a, b, c) for c, a, b in ev] or [(aid + ".wav", np.nan, np.nan, np.nan)]
        else:
            ev = _decode(arr[:, 10:], ts, MAESTRO)
            maestro_rows += [(aid + ".wav", a, b, c, 1.0) for c, a, b in ev]
            maestro_classes |= {c for c, _, _ in ev}
            maestro_rows.append((aid + ".wav", 0.0, dur, "m16", 0.4))                # low confidence: dropped
    assert len(synth_rows) > 3 and maestro_classes, "the random-init posteriors must cross 0.5 for this case to bite"
    maestro_eval = sorted(maestro_classes)[:6]
    maestro_rows += [(r[0], 0.0, dur, c, 1.0) for r in maestro_rows[:1] for c in MAESTRO if c not in maestro_eval][:2]  # not evaluated
    task.hparams["class_labels"] = {"desed": DESED, "maestro_real": MAESTRO, "maestro_real_eval": set(maestro_eval)}
    gt = pd.DataFrame(synth_rows, columns=["filename", "onset", "offset", "event_label"])
    paths = {k: os.path.join(tmp, k + ".tsv") for k in ("synth_val_tsv", "synth_val_dur", "real_maestro_train_tsv")}
    gt.to_csv(paths["synth_val_tsv"], sep="\t", index=False)
    pd.DataFrame({"filename": ["s%d.wav" % i for i in range(3)], "duration": dur}).to_csv(paths["synth_val_dur"], sep="\t", index=False)
    pd.DataFrame(maestro_rows, columns=["filename", "onset", "offset", "event_label", "confidence"]).to_csv(
        paths["real_maestro_train_tsv"], sep="\t", index=False)
    task.hparams["data"].update(paths)
    saved = copy.deepcopy((task.val_buffer_sed_scores_eval_student, task.val_buffer_sed_scores_eval_teacher,
                           task.get_weak_student_f1_seg_macro, task.get_weak_teacher_f1_seg_macro))
    task.logged.clear()
    obj = task.validation_epoch_end(None)
    assert set(task.logged) == EPOCH_KEYS
    L = {k: float(v) for k, v in task.logged.items()}
    for who in ("student", "teacher"):
        assert L[f"val/{who}/intersection_f1_macro_thres05/sed_scores_eval"] == 1.0
        assert L[f"val/{who}/collar_f1_macro_thres05/sed_scores_eval"] == 1.0
        assert L[f"val/{who}/segment_f1_macro_thresopt/sed_scores_eval"] == 1.0
        assert 0.0 < L[f"val/{who}/psds1/sed_scores_eval"] <= 1.0
    assert task.val_buffer_sed_scores_eval_student == {} and task.get_weak_student_f1_seg_macro.tp is None
    # the objective, recomputed from the buffers: weak F1 + PSDS1 (default synth type) + mpAUC (default MAESTRO type)
    buf, weak = saved[0], saved[2]
    gt_d = {a: [(r.onset, r.offset, r.event_label) for r in gt[gt.filename == a + ".wav"].itertuples()] for a in ("s0", "s1", "s2")}
    gt_d = {a: e for a, e in gt_d.items() if e and not pd.isna(e[0][2])}
    psds1 = compute_psds_from_scores({a: buf[a][["onset", "offset"] + DESED] for a in gt_d}, gt_d, {a: dur for a in gt_d},
                                     dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0, alpha_st=1)
    mrows = [r for r in maestro_rows if r[4] > 0.5 and r[3] in maestro_eval]
    from desed_task_amd.evaluation.maestro import merge_overlapping_events
    mgt = merge_overlapping_events({a[:-4]: [(r[1], r[2], r[3]) for r in mrows if r[0] == a] for a in sorted({r[0] for r in mrows})})
    mdur = {a: max(e[1] for e in evs) for a, evs in mgt.items()}
    mp = segment_based.auroc({a: buf[a][["onset", "offset"] + maestro_eval] for a in mgt}, mgt, mdur, max_fpr=0.1)[0]["mean"]
    expect = float(weak.compute()) + psds1 + mp
    assert abs(float(obj) - expect) < 1e-6 and abs(L["val/obj_metric"] - expect) < 1e-6
    # the other objective types: intersection F1 + best segment F1 ("fmo"; "mpauc" selects it too, as in the reference).
    # fast_dev_run changes nothing (the recipe validates on the whole set then; the buffers hold MAESTRO clips the DESED
    # tables do not list)
    for mtype, fast in (("fmo", False), ("mpauc", True)):
        (task.val_buffer_sed_scores_eval_student, task.val_buffer_sed_scores_eval_teacher, task.get_weak_student_f1_seg_macro,
         task.get_weak_teacher_f1_seg_macro) = copy.deepcopy(saved)
        task.hparams["training"].update(obj_metric_synth_type="intersection", obj_metric_maestro_type=mtype)
        task.fast_dev_run = fast
        obj = task.validation_epoch_end(None)
        assert abs(float(obj) - (float(weak.compute()) + 2.0)) < 1e-6
    task.fast_dev_run = False
    return task


def case_test_2024(dev, tmp, n_samp=16000 * 2 + 1024, te=53):
    """test_step x2 + on_test_epoch_end: the 22 keys, the MAESTRO segment tables (device segment means, overlap-add per
    recording) against the same computation restated on the host, and evaluation=True writing only the score tables."""
    task = _task(dev, n_samp)
    task.fast_dev_run = True            # as train_pretrained.py --fast_dev_run: the metrics still run on the whole test set
    task.hparams["training"]["n_test_thresholds"] = 10
    task.hparams["log_dir"] = str(tmp)
    files_all = []
    # MAESTRO validation clips "<recording>-<onset cs>-<offset cs>": three overlapping 2 s clips of one 4 s recording
    batches = [["/d/test/t0.wav", "/d/test/t1.wav", "/d/maestro_val/recA-0-200.wav"],
               ["/d/test/t2.wav", "/d/maestro_val/recA-100-300.wav", "/d/maestro_val/recA-200-400.wav"]]
    for step, files in enumerate(batches):
        batch = _batch(dev, files, n_samp, te, seed=51 + 7 * step)[-1]
        task.test_step(batch, step)
        files_all += files
    assert {"test/student/loss_strong", "test/teacher/loss_strong"} <= set(task.logged)
    post = task.test_buffer_sed_scores_eval_student
    ts = task.encoder._frame_to_time(np.arange(len(post["t0"]) + 1))
    dur = n_samp / 16000.0
    rows, mrows = [], []
    for f in files_all:
        aid = os.path.basename(f)[:-4]
        arr = post[aid].values[:, 2:]
        if aid.startswith("t"):
            ev = _decode(arr[:, :10], ts, DESED)
            rows += [(aid + ".wav", a, b, c) for c, a, b in ev] or [(aid + ".wav", np.nan, np.nan, np.nan)]
        else:
            on = int(aid.split("-")[1]) / 100
            mrows += [(aid + ".wav", a, b, c, 1.0) for c, a, b in _decode(arr[:, 10:], ts, MAESTRO)]
            mrows.append((aid + ".wav", 0.5, 1.5, "m00", 1.0))
    data = {k: os.path.join(str(tmp), k + ".tsv") for k in ("test_tsv", "test_dur", "real_maestro_val_tsv", "real_maestro_val_dur")}
    pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"]).to_csv(data["test_tsv"], sep="\t", index=False)
    pd.DataFrame({"filename": ["t%d.wav" % i for i in range(3)], "duration": dur}).to_csv(data["test_dur"], sep="\t", index=False)
    pd.DataFrame(mrows, columns=["filename", "onset", "offset", "event_label", "confidence"]).to_csv(
        data["real_maestro_val_tsv"], sep="\t", index=False)
    pd.DataFrame({"filename": ["recA.wav"], "duration": [4.0]}).to_csv(data["real_maestro_val_dur"], sep="\t", index=False)
    task.hparams["data"] = data
    task.hparams["class_labels"] = {"desed": DESED, "maestro_real": MAESTRO, "maestro_real_eval": {"m00", "m01", "m02"}}
    saved = copy.deepcopy(task.test_buffer_sed_scores_eval_student)
    res = task.on_test_epoch_end()
    assert set(res) == TEST_KEYS and all(np.isfinite(float(v)) for k, v in res.items() if "mauc" not in k and "mpauc" not in k)
    assert res["test/student/intersection_f1_macro_thres05/sed_scores_eval"] == 1.0
    assert res["test/student/collar_f1_macro_thres05/sed_scores_eval"] == 1.0
    # the written MAESTRO segment table of the recording vs the reference's arithmetic restated on the host (float64)
    tab = pd.read_csv(os.path.join(str(tmp), "metrics_test", "student", "maestro", "postprocessed", "recA.tsv"), sep="\t")
    assert list(tab.columns) == ["onset", "offset"] + MAESTRO and len(tab) == 4
    acc, cnt = np.zeros((4, 17)), np.zeros((4, 17))
    for aid in ("recA-0-200", "recA-100-300", "recA-200-400"):
        arr = saved[aid][MAESTRO].to_numpy(np.float64)
        k0 = int(aid.split("-")[1]) // 100
        for k in range(2):
            w = np.minimum(ts[1:], k + 1.0) - np.maximum(ts[:-1], float(k))
            sel = (ts[1:] > k) & (ts[:-1] < k + 1.0)
            acc[k0 + k] += (w[sel, None] * arr[sel]).sum(0) / w[sel].sum()
            cnt[k0 + k] += 1
    assert np.abs(tab[MAESTRO].to_numpy() - acc / np.maximum(cnt, 1)).max() < 1e-6
    # evaluation=True: only the score tables
    task2 = _task(dev, n_samp)
    task2.evaluation = True
    task2.hparams["training"]["n_test_thresholds"] = 10
    out = os.path.join(str(tmp), "eval")
    task2.hparams["log_dir"] = out
    task2.test_step(_batch(dev, batches[0], n_samp, te, seed=51)[-1], 0)
    assert "test/student/loss_strong" not in task2.logged
    assert task2.on_test_epoch_end() == {}
    written = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert written == sorted(os.path.join("metrics_test", "%s_scores" % who, kind, a + ".tsv") for who in ("student", "teacher")
                             for kind in ("unprocessed", "postprocessed") for a in ("t0", "t1", "recA-0-200"))
    return res
