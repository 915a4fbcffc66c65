"""CPU checks of the 2024 recipe's validation / test path (no GPU: the kernels run in the fiber emulator, tests/emu): the class-wise
median filter and the segment kernel against the reference fixture (golden/golden_post2024.npz, tests/golden/make_golden_post2024.py),
the MAESTRO helpers, the segment-based evaluator against sklearn and a brute-force sweep, and the 2024 trainer's hooks on a
miniature in-memory set."""
import numpy as np
import pytest
import torch

from tests import eval2024_cases as C
from tests.emu_support import emu  # noqa: F401


@pytest.fixture(scope="module")
def G():
    return C.golden()


def test_classwise_filter_and_segment_kernel_vs_reference_fixture(emu, G):  # noqa: F811
    C.case_kernels_vs_fixture("cpu", G)


def test_classwise_filter_equals_host_filter_and_decoding(emu):  # noqa: F811
    C.case_host_filter_equivalence("cpu", B=6, T=40)


def test_host_classwise_filter_is_the_reference_filter(G):
    from desed_task_amd.postprocess import ClassWiseMedianFilter
    x = C.codes_to_scores(G["x_codes"])
    for b in range(3):
        assert np.array_equal(ClassWiseMedianFilter(list(G["wins_recipe"]))(x[b]), C.codes_to_scores(G["med_recipe"][b]))
    assert np.array_equal(ClassWiseMedianFilter(list(G["wins_short"]))(x[0, :5]), C.codes_to_scores(G["med_short"][0]))


def test_alias_module_serves_the_filter():
    import importlib
    import sys
    import os
    sys.path.insert(0, os.path.join(C.HERE, "..", "desed_task_amd", "drop_in"))
    try:
        for k in [k for k in sys.modules if k == "desed_task" or k.startswith("desed_task.")]:
            del sys.modules[k]
        m = importlib.import_module("desed_task.utils.postprocess")
        from desed_task_amd.postprocess import ClassWiseMedianFilter
        assert m.ClassWiseMedianFilter is ClassWiseMedianFilter
    finally:
        sys.path.pop(0)
        for k in [k for k in sys.modules if k == "desed_task" or k.startswith("desed_task.")]:
            del sys.modules[k]


def _events(files, events, labels):
    out = {}
    for f, (a, b), c in zip(files, events, labels):
        out.setdefault(str(f), []).append((float(a), float(b), str(c)))
    return out


def test_maestro_merge_helpers_vs_reference_fixture(G):
    from desed_task_amd.evaluation.maestro import merge_maestro_ground_truth, merge_overlapping_events
    clip_gt = _events(G["gt_clip_ids"], G["gt_clip_events"], G["gt_clip_labels"])
    got = merge_maestro_ground_truth({k: list(v) for k, v in clip_gt.items()})
    rows = sorted((f, float(a), float(b), c) for f, evs in got.items() for a, b, c in evs)
    assert rows == sorted(zip(G["merged_files"].tolist(), *np.asarray(G["merged_events"]).T.tolist(), G["merged_labels"].tolist()))
    got = merge_overlapping_events({k: list(v) for k, v in clip_gt.items()})
    rows = sorted((f, float(a), float(b), c) for f, evs in got.items() for a, b, c in evs)
    assert rows == sorted(zip(G["clipmerged_ids"].tolist(), *np.asarray(G["clipmerged_events"]).T.tolist(),
                              G["clipmerged_labels"].tolist()))


def test_overlap_add_vs_reference_fixture(emu, G):  # noqa: F811
    from desed_task_amd.evaluation.maestro import segment_scores_and_overlap_add
    from desed_task_amd.postprocess import create_score_dataframe
    x = C.codes_to_scores(G["x_codes"])
    classes = ["c%02d" % c for c in range(27)]
    ts = np.arange(157) * 4 / (16000 / 256)
    frames = {str(cid): create_score_dataframe(x[i].astype(np.float64), ts, classes) for i, cid in enumerate(G["ola_ids"])}
    dur = {"recA": float(G["ola_durations"][0]), "recB": float(G["ola_durations"][1])}
    out = segment_scores_and_overlap_add(frames, dur, classes, 1.0, device=torch.device("cpu"))
    for rec in ("recA", "recB"):
        ref = G["ola_" + rec]
        got = out[rec][["onset", "offset"] + classes].to_numpy()
        assert got.shape == ref.shape
        assert np.array_equal(got[:, :2], ref[:, :2]) and np.abs(got[:, 2:] - ref[:, 2:]).max() <= 1e-6


def _random_tables(rng, n_clips=6, dur=10.0, classes=("a", "b", "c")):
    from desed_task_amd.postprocess import create_score_dataframe
    scores, gt, durs = {}, {}, {}
    for i in range(n_clips):
        d = dur - 0.5 * (i % 2)
        ts = np.minimum(np.arange(158) * 0.064, d) if i % 3 == 0 else np.arange(157) * 0.064
        n = len(ts) - 1
        arr = np.round(rng.random((n, len(classes))) * 20) / 20                     # ties
        scores["clip%d" % i] = create_score_dataframe(arr, ts, list(classes))
        evs = []
        for c in classes:
            for _ in range(rng.integers(0, 3)):
                a = float(rng.uniform(0, d - 0.5))
                evs.append((a, float(min(d, a + rng.uniform(0.05, 3))), c))
        gt["clip%d" % i], durs["clip%d" % i] = evs, d
    return scores, gt, durs


def test_segment_auroc_vs_sklearn():
    from sklearn.metrics import roc_auc_score
    from desed_task_amd.evaluation import segment_based as S
    rng = np.random.default_rng(5)
    scores, gt, durs = _random_tables(rng)
    classes, s, y = S.segment_scores_and_targets(scores, gt, durs, 1.0)
    assert s.shape == (sum(int(np.ceil(d)) for d in durs.values()), 3)
    auc = S.auroc(scores, gt, durs)[0]
    auc_mc = S.auroc(scores, gt, durs, max_fpr=0.1, mcclish_correction=True)[0]
    pauc = S.auroc(scores, gt, durs, max_fpr=0.1)[0]
    for i, c in enumerate(classes):
        assert 0 < y[:, i].sum() < len(y)
        assert abs(auc[c] - roc_auc_score(y[:, i], s[:, i])) < 1e-12
        assert abs(auc_mc[c] - roc_auc_score(y[:, i], s[:, i], max_fpr=0.1)) < 1e-12
        # the un-corrected partial area / max_fpr, from sklearn's own ROC points
        from sklearn.metrics import roc_curve
        fpr, tpr, _ = roc_curve(y[:, i], s[:, i], drop_intermediate=False)
        stop = np.searchsorted(fpr, 0.1, "right")
        xs = np.r_[fpr[:stop], 0.1]
        ys = np.r_[tpr[:stop], np.interp(0.1, fpr[stop - 1:stop + 1], tpr[stop - 1:stop + 1])]
        assert abs(pauc[c] - np.trapezoid(ys, xs) / 0.1) < 1e-12
    assert abs(auc["mean"] - np.mean([auc[c] for c in classes])) < 1e-15


def test_segment_best_fscore_vs_brute_force():
    from desed_task_amd.evaluation import segment_based as S
    rng = np.random.default_rng(8)
    scores, gt, durs = _random_tables(rng)
    classes, s, y = S.segment_scores_and_targets(scores, gt, durs, 1.0)
    f, p, r, thr, _ = S.best_fscore(scores, gt, durs)
    for i, c in enumerate(classes):
        best = 0.0
        for th in np.unique(s[:, i]):
            det = s[:, i] >= th
            tp, fp, fn = (det & y[:, i]).sum(), (det & ~y[:, i]).sum(), (~det & y[:, i]).sum()
            best = max(best, 2 * tp / (2 * tp + fp + fn))
        assert abs(f[c] - best) < 1e-12
        det = s[:, i] >= thr[c]
        assert abs(2 * (det & y[:, i]).sum() / (det.sum() + y[:, i].sum()) - best) < 1e-12
    assert abs(f["macro_average"] - np.mean([f[c] for c in classes])) < 1e-15
    # a perfect score table (1 on positive segments, 0 elsewhere) scores 1; a class without positives scores 0
    from desed_task_amd.postprocess import create_score_dataframe
    perfect = {}
    for k, df in scores.items():
        n = int(np.ceil(durs[k]))
        ts = np.minimum(np.arange(n + 1, dtype=float), durs[k])
        perfect[k] = create_score_dataframe(S.segment_targets(gt[k], durs[k], classes).astype(float), ts, classes)
    assert S.best_fscore(perfect, gt, durs)[0]["macro_average"] == 1.0
    assert S.auroc(perfect, gt, durs)[0]["mean"] == 1.0
    empty = {k: [e for e in v if e[2] != "a"] for k, v in gt.items()}
    assert S.best_fscore(scores, empty, durs)[0]["a"] == 0.0


def test_segment_max_reduction_passes_segment_tables_through():
    from desed_task_amd.evaluation.segment_based import segment_max
    rng = np.random.default_rng(1)
    arr = rng.random((5, 2))
    ts = np.minimum(np.arange(6, dtype=float), 4.3)
    assert np.array_equal(segment_max(ts, arr, 4.3, 1.0), arr)


def test_validation_hooks_2024(emu, tmp_path):  # noqa: F811
    C.case_validation_2024("cpu", str(tmp_path), check_oracle=True)


def test_test_hooks_2024(emu, tmp_path):  # noqa: F811
    C.case_test_2024("cpu", tmp_path)


def test_2024_hooks_refuse_e2e_and_bad_batches(emu):  # noqa: F811
    task = C._task("cpu", 16000 * 2 + 1024)
    with pytest.raises(ValueError):
        task.validation_step((None,) * 4, 0)
    task.hparams["pretrained"]["e2e"] = True
    with pytest.raises(NotImplementedError):
        task.test_step((None,) * 6, 0)
