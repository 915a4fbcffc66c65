"""Cases for the threshold-free PSDS on the device (desed_task_amd/evaluation/psds_device.py, csrc/sed_psds.hip), device-agnostic like
resident_cases.py: dev = "cpu" on the fiber emulator, "cuda" on the MI355X.  The yardstick is the host evaluator,
evaluation/psds_scores.py (`_clip_class_steps` per clip and class, `psds_from_scores` end to end), computed once per case and shared.

Inputs: fp32 uniform scores, median-filtered with window 7 when T >= 7, optionally quantised (ties); per clip 0-5 ground-truth events
with OFF-GRID onsets from a seeded generator, some offsets clipped to the clip end.  Ground truth aligned to frame boundaries would
manufacture exact ties between an overlap and its threshold (dtc = 0.5 or 0.1), where the last bit of the summation order decides a
count; the builder asserts for EVERY case and setting that the host result does not move when dtc / gtc / cttc are scaled by
1 -+ 1e-9, so the integer counts compared below are well defined.

Tolerances: counts and jumps are integers and compared exactly; the ROC arrays come out of the same tail code from equal integers and
are compared element for element; the PSDS values get 1e-12 absolute, a bound that follows from that and is not measured.
"""
import contextlib
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from desed_task_amd.evaluation import psds_device as D
from desed_task_amd.evaluation import psds_scores as H
from tests import parity_cases as P
from tests.resident_cases import Framed, sync

SETTINGS = {
    "scenario1": dict(dtc_threshold=0.7, gtc_threshold=0.7, cttc_threshold=None, alpha_ct=0.0, alpha_st=1.0),
    "scenario2": dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1.0),
    "mid": dict(dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3, alpha_ct=0.0, alpha_st=0.0),
}
# name: (clips, frames, classes, quantisation levels or None, seed)
SHAPES = {
    "a": (5, 156, 10, None, 101),        # the recipe's clip
    "b": (4, 157, 4, 16, 102),           # odd length, rows no multiple of a wave, many ties
    "c": (4, 7, 3, 8, 103),              # fewer distinct scores than a wave
    "d": (4, 1, 2, None, 104),           # a single frame
    "e": (3, 64, 27, None, 105),         # the 2024 class count: 26 cross-trigger columns
    "f": (5, 156, 4, None, 106),         # edge contents, see _edge_contents
    "g": (48, 156, 10, None, 107),       # two validation batches (GPU only)
}
CPU_CASES = ("a", "b", "c", "d", "e", "f")
GPU_CASES = CPU_CASES + ("g",)


def _timestamps(T):
    """The boundaries the trainers pass: ManyHotEncoder._frame_to_time of the 2023 recipe (64 ms frames, clipped to the 10 s clip)."""
    return np.asarray(P._Encoder([], audio_len=10)._frame_to_time(np.arange(T + 1)), dtype=np.float64)


def _scores(rng, N, T, NC, levels):
    from scipy.ndimage import median_filter
    x = rng.random_sample((N, T, NC)).astype(np.float32)
    if T >= 7:
        x = np.stack([median_filter(x[n], (7, 1)) for n in range(N)])
    if levels:
        x = (np.round(x * (levels - 1)) / (levels - 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def _events(rng, n_events, length, labels, clip_some=True):
    ev = []
    for _ in range(n_events):
        on = float(rng.uniform(0.0, 0.8 * length))
        off = on + float(rng.uniform(0.05 * length, 0.4 * length))
        if clip_some and off > length:
            off = float(length)                                       # an offset clipped to the clip end
        ev.append((on, off, labels[rng.randint(len(labels))]))
    return ev


def _edge_contents(rng, case):
    """Case f: a clip whose scores are all equal (n_u = 1), a clip with no events, a class with >= 9 events in one clip (the host's
    pairwise-sum path), a clip shorter than ts[T] (partial overlap with the clip), and a last event that ends after ts[T]."""
    labels, length = case["labels"], float(case["ts"][-1])
    ids = case["ids"]
    case["scores"][0] = np.float32(0.375)
    case["gt"][ids[1]] = []
    many = []
    for _ in range(10):
        on = float(rng.uniform(0.0, 0.9 * length))
        many.append((on, on + float(rng.uniform(0.02 * length, 0.08 * length)), labels[2]))
    case["gt"][ids[2]] = many + _events(rng, 2, length, labels[:2])
    case["dur"][ids[3]] = 9.5
    case["gt"][ids[4]] = _events(rng, 3, length, labels)[:2] + [(0.9 * length + 0.0123, length + 0.777, labels[1])]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: scores (N, T, NC) fp32, ts, ids, labels, gt {id: events}, dur {id: seconds}; plus the host results per setting
    (`host`: the 4-tuple of psds_from_scores on the tables) -- after the stability precondition."""
    N, T, NC, levels, seed = SHAPES[name]
    rng = np.random.RandomState(seed)
    ts = _timestamps(T)
    labels = ["c%02d" % i for i in range(NC)]
    ids = ["clip_%s_%02d" % (name, (7 * n + 3) % N) for n in range(N)]          # not in sorted order
    assert len(set(ids)) == N
    c = {"name": name, "scores": _scores(rng, N, T, NC, levels), "ts": ts, "ids": ids, "labels": labels,
         "gt": {a: _events(rng, rng.randint(0, 6), float(ts[-1]), labels) for a in ids}, "dur": {a: 10.0 for a in ids}}
    if name == "f":
        _edge_contents(rng, c)
    c["tables"] = tables_of(c)
    c["host"] = {sname: stable_host_result(c["tables"], c["gt"], c["dur"], kw, "case %s / %s" % (name, sname))
                 for sname, kw in SETTINGS.items()}
    return c


def stable_host_result(tables, gt, dur, kw, what):
    """psds_from_scores, after the precondition: no overlap sits within 1e-9 (relative) of its threshold, so the counts are the same
    for either summation order."""
    res = [H.psds_from_scores(tables, gt, dur, **_scaled(kw, f)) for f in (1.0 - 1e-9, 1.0, 1.0 + 1e-9)]
    for r in (res[0], res[2]):
        assert r[0] == res[1][0], "%s is not stable under a 1e-9 change of the thresholds" % what
        assert all(np.array_equal(r[3][k][0], res[1][3][k][0]) and np.array_equal(r[3][k][1], res[1][3][k][1]) for k in res[1][3])
    return res[1]


def _scaled(kw, f):
    out = dict(kw)
    for k in ("dtc_threshold", "gtc_threshold", "cttc_threshold"):
        if out[k] is not None:
            out[k] = out[k] * f
    return out


def tables_of(c):
    from desed_task_amd.postprocess import create_score_dataframe
    return {a: create_score_dataframe(c["scores"][n], c["ts"], c["labels"]) for n, a in enumerate(c["ids"])}


def host_steps(c, kw):
    """{(clip position in sorted order, class): (u, tp, fp, ct full-width)} by psds_scores._clip_class_steps, with the inputs
    psds_from_scores hands it."""
    ts, labels = c["ts"], c["labels"]
    nc = len(labels)
    use_ct = kw["cttc_threshold"] is not None and kw["alpha_ct"] > 0
    out = {}
    for n, aid in enumerate(sorted(c["ids"])):
        S = c["scores"][c["ids"].index(aid)].astype(np.float64)
        per_class = [[(o, f) for o, f, l in c["gt"][aid] if l == lab] for lab in labels]
        ov_gt = [np.stack([H._frame_overlap(ts, o, f) for o, f in ev], 1) if ev else np.zeros((len(S), 0)) for ev in per_class]
        ov_cls = np.stack([g.sum(1) for g in ov_gt], 1)
        ov_world = H._frame_overlap(ts, 0.0, float(c["dur"][aid]))
        for k in range(nc):
            others = [j for j in range(nc) if j != k] if use_ct else []
            u, tp, fp, ct = H._clip_class_steps(S[:, k], ts, ov_cls[:, k], ov_gt[k], np.array([f - o for o, f in per_class[k]]),
                                                ov_cls[:, others], ov_world, kw["dtc_threshold"], kw["gtc_threshold"],
                                                kw["cttc_threshold"])
            full = np.zeros((len(tp), nc))
            full[:, others] = ct
            out[n, k] = (u, tp, fp, full)
    return out


def _device_inputs(dev, c, kw):
    ids = sorted(c["ids"])
    table = D._event_table(c["gt"], ids, c["labels"])
    ev_ptr, ev_on, ev_off = D._event_table_on(table, torch.device(dev))
    scores = P.to(dev, torch.from_numpy(np.ascontiguousarray(c["scores"][[c["ids"].index(a) for a in ids]])))
    ts = P.to(dev, torch.from_numpy(c["ts"]))
    dur = P.to(dev, torch.tensor([c["dur"][a] for a in ids], dtype=torch.float64))
    return scores, ts, ev_ptr, ev_on, ev_off, dur


def _framed_outputs(dev, N, T, NC, use_ct):
    f = {"n_u": Framed(dev, N, NC, torch.int32), "u": Framed(dev, N * NC, T, torch.float32), "tp0": Framed(dev, N, NC, torch.int32),
         "fp0": Framed(dev, N, NC, torch.int32), "dtp": Framed(dev, N * NC, T, torch.int32), "dfp": Framed(dev, N * NC, T, torch.int32)}
    if use_ct:
        f["ct0"] = Framed(dev, N * NC, NC, torch.int32)
        f["dct"] = Framed(dev, N * NC, T * NC, torch.int32)
    shapes = {"n_u": (N, NC), "u": (N, NC, T), "tp0": (N, NC), "fp0": (N, NC), "dtp": (N, NC, T), "dfp": (N, NC, T), "ct0": (N, NC, NC),
              "dct": (N, NC, T, NC)}
    return f, {k: v.body.view(shapes[k]) for k, v in f.items()}


def case_kernel(dev, name, sname):
    """Assertion 1: per (clip, class) the distinct scores, the row-0 counts and the integer jumps of the kernel equal those of
    _clip_class_steps; canary frames intact; a second launch writes identical bytes."""
    c, kw = case(name), SETTINGS[sname]
    N, T, NC = c["scores"].shape
    use_ct = kw["cttc_threshold"] is not None and kw["alpha_ct"] > 0
    inputs = _device_inputs(dev, c, kw)
    runs = []
    for _ in range(2):
        frames, out = _framed_outputs(dev, N, T, NC, use_ct)
        D.psds_steps(*inputs, kw["dtc_threshold"], kw["gtc_threshold"], kw["cttc_threshold"], use_ct, out=out)
        sync(dev)
        for k, fr in frames.items():
            fr.assert_guards("%s of case %s / %s" % (k, name, sname))
        runs.append({k: fr.buf.cpu() for k, fr in frames.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), "%s: two launches differ" % k
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ref = host_steps(c, kw)
    ids = sorted(c["ids"])
    for n in range(N):
        col_src = c["scores"][c["ids"].index(ids[n])]
        for k in range(NC):
            what = "case %s / %s, clip %d, class %d" % (name, sname, n, k)
            u, tp, fp, ct = ref[n, k]
            uniq = np.unique(col_src[:, k])
            n_u = int(got["n_u"][n, k])
            assert uniq.dtype == np.float32 and n_u == len(uniq) == len(u), what
            assert np.array_equal(got["u"][n, k, :n_u], uniq), what
            assert np.array_equal(got["u"][n, k, :n_u].astype(np.float64), u), what
            assert got["tp0"][n, k] == tp[0] and got["fp0"][n, k] == fp[0], (what, got["tp0"][n, k], tp[0], got["fp0"][n, k], fp[0])
            assert np.array_equal(got["dtp"][n, k, :n_u], np.diff(tp)), (what, "dtp")
            assert np.array_equal(got["dfp"][n, k, :n_u], np.diff(fp)), (what, "dfp")
            assert not got["dtp"][n, k, n_u:].any() and not got["dfp"][n, k, n_u:].any(), what
            if use_ct:
                assert np.array_equal(got["ct0"][n, k], ct[0]) and got["ct0"][n, k, k] == 0, (what, "ct0")
                assert np.array_equal(got["dct"][n, k, :n_u], np.diff(ct, axis=0)), (what, "dct")
                assert not got["dct"][n, k, n_u:].any(), what


def fill_buffer(dev, c, chunks=2, labels=None):
    """A ScoreBuffer holding the case's clips, appended in `chunks` batches; the first clip is appended twice, the first time with
    other scores (the later row must win, like dict.update)."""
    buf = D.ScoreBuffer()
    N = len(c["ids"])
    stale = P.to(dev, torch.from_numpy(np.ascontiguousarray(1.0 - c["scores"][:1])))
    buf.append(stale, c["ids"][:1], timestamps=c["ts"], event_classes=labels or c["labels"])
    edges = np.linspace(0, N, chunks + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            buf.append(P.to(dev, torch.from_numpy(np.ascontiguousarray(c["scores"][a:b]))), c["ids"][a:b], timestamps=c["ts"],
                       event_classes=labels or c["labels"])
    return buf


def _assert_same_result(got, ref, labels, what):
    for k in labels:
        assert np.array_equal(got[3][k][0], ref[3][k][0]), (what, k, "eFPR")
        assert np.array_equal(got[3][k][1], ref[3][k][1]), (what, k, "TPR")
    assert abs(got[0] - ref[0]) <= 1e-12, (what, got[0], ref[0])
    assert set(got[1]) == set(ref[1])
    for k in ref[1]:
        assert abs(got[1][k] - ref[1][k]) <= 1e-12, (what, k)
    assert np.array_equal(got[2][0], ref[2][0]) and np.abs(got[2][1] - ref[2][1]).max() <= 1e-12, what


def case_end_to_end(dev, name, sname):
    """Assertion 2: psds_from_score_buffer against psds_from_scores on the buffer's own tables."""
    from pandas.testing import assert_frame_equal
    c, kw = case(name), SETTINGS[sname]
    buf = fill_buffer(dev, c)
    assert len(buf) == len(c["ids"]) and set(buf) == set(c["ids"])
    tables = buf.to_tables()
    assert list(tables) == c["ids"]
    for a in c["ids"]:
        assert_frame_equal(tables[a], c["tables"][a], check_exact=True)
    got = D.psds_from_score_buffer(buf, c["gt"], c["dur"], **kw)
    _assert_same_result(got, c["host"][sname], c["labels"], "case %s / %s" % (name, sname))
    assert 0.0 <= got[0] <= 1.0


def case_class_subset(dev):
    """`classes=`: the DESED columns of a 27-class buffer, in another order than the buffer's, through compute_psds_from_scores."""
    from desed_task_amd.evaluation.evaluation_measures import compute_psds_from_scores
    c = case("e")
    sub = [c["labels"][i] for i in (9, 0, 3, 4, 20, 26, 11)]
    gt = {a: [(o, f, sub[(i + n) % len(sub)]) for i, (o, f, _) in enumerate(c["gt"][a])] for n, a in enumerate(c["ids"])}
    gt = {a: ev for a, ev in gt.items() if ev}
    assert len(gt) >= 1
    dur = {a: c["dur"][a] for a in gt}
    buf = fill_buffer(dev, c)
    for sname, kw in SETTINGS.items():
        ref = stable_host_result({a: c["tables"][a][["onset", "offset"] + sub] for a in gt}, gt, dur, kw, "subset / %s" % sname)
        got = D.psds_from_score_buffer(buf, gt, dur, classes=sub, **kw)
        _assert_same_result(got, ref, sub, "subset / %s" % sname)
        assert abs(compute_psds_from_scores(buf, gt, dur, classes=sub, **kw) - ref[0]) <= 1e-12


def case_tables(dev, tmp):
    """Assertion 3: with `device_scores` batched_decode_preds builds no tables; the buffer's tables equal the ones it builds without,
    the decoded events are the same, and compute_psds_from_scores writes the same files from either."""
    from pandas.testing import assert_frame_equal
    from desed_task_amd import postprocess as PP
    from desed_task_amd.evaluation.evaluation_measures import compute_psds_from_scores
    B, T, NC = 5, 156, 10
    g = torch.Generator().manual_seed(3)
    strong = P.to(dev, torch.rand(B, NC, T, generator=g))
    enc = P._Encoder(["c%d" % i for i in range(NC)])
    files = ["/data/synth/clip_%d.wav" % i for i in range(B)]
    raw, post, dfs = PP.batched_decode_preds(strong, files, enc, thresholds=[0.3, 0.5], median_filter=7)
    buf = D.ScoreBuffer()
    raw_d, post_d, dfs_d = PP.batched_decode_preds(strong, files, enc, thresholds=[0.3, 0.5], median_filter=7, device_scores=buf)
    assert raw_d == {} and post_d == {} and len(raw) == len(post) == B
    tables = buf.to_tables()
    assert list(tables) == list(post)
    for a in post:
        assert_frame_equal(tables[a], post[a], check_exact=True)
    for th in (0.3, 0.5):
        assert_frame_equal(dfs_d[th], dfs[th], check_exact=True)
    # the same files with save_dir
    rng = np.random.RandomState(5)
    gt = {a: _events(rng, 2, 9.984, enc.labels) for a in post}
    dur = {a: 10.0 for a in post}
    kw = SETTINGS["scenario2"]
    v_host = compute_psds_from_scores(post, gt, dur, save_dir=os.path.join(tmp, "host"), **kw)
    v_dev = compute_psds_from_scores(buf, gt, dur, save_dir=os.path.join(tmp, "dev"), **kw)
    assert abs(v_host - v_dev) <= 1e-12
    listing = lambda d: sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)      # noqa: E731
    assert listing(os.path.join(tmp, "host")) == listing(os.path.join(tmp, "dev")) and len(listing(os.path.join(tmp, "dev"))) == B + 1
    for rel in listing(os.path.join(tmp, "host")):
        assert open(os.path.join(tmp, "host", rel), "rb").read() == open(os.path.join(tmp, "dev", rel), "rb").read(), rel


def case_errors(dev):
    """Assertion 4."""
    from desed_task_amd import postprocess as PP
    c = case("c")
    for T, NC in ((257, 2), (4, 33)):
        buf = D.ScoreBuffer()
        ids = ["x0", "x1"]
        buf.append(P.to(dev, torch.rand(2, T, NC)), ids, timestamps=np.arange(T + 1) * 0.064, event_classes=["k%d" % i for i in range(NC)])
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            D.psds_from_score_buffer(buf, {a: [(0.01, 0.05, "k1")] for a in ids}, {a: 1.0 for a in ids})
    nan = c["scores"].copy()
    nan[1, 2, 0] = np.nan
    buf = D.ScoreBuffer()
    buf.append(P.to(dev, torch.from_numpy(nan)), c["ids"], timestamps=c["ts"], event_classes=c["labels"])
    with pytest.raises(ValueError, match="NaN"):
        D.psds_from_score_buffer(buf, c["gt"], c["dur"])
    buf = fill_buffer(dev, c)
    gt = dict(c["gt"])
    gt["absent"] = []
    with pytest.raises(ValueError, match="missing for 1 clips"):
        D.psds_from_score_buffer(buf, gt, dict(c["dur"], absent=1.0))
    with pytest.raises(ValueError, match="missing for 1 clips"):
        D.psds_from_score_buffer(buf, c["gt"], {a: d for a, d in c["dur"].items() if a != c["ids"][0]})
    with pytest.raises(ValueError, match="has no score column"):
        D.psds_from_score_buffer(buf, dict(c["gt"], **{c["ids"][0]: [(0.0, 0.1, "unknown")]}), c["dur"])
    with pytest.raises(ValueError, match="cross triggers need a cttc_threshold"):
        D.psds_from_score_buffer(buf, c["gt"], c["dur"], cttc_threshold=None, alpha_ct=0.5)
    enc = P._Encoder(["c%d" % i for i in range(3)])
    with pytest.raises(ValueError, match="pad_indx"):
        PP.batched_decode_preds(P.to(dev, torch.rand(2, 3, 20)), ["/d/a.wav", "/d/b.wav"], enc, device_scores=D.ScoreBuffer(),
                                pad_indx=torch.tensor([1.0, 0.5]))
    with pytest.raises(ValueError, match="one \\(frames, classes\\) shape"):
        buf.append(P.to(dev, torch.rand(1, 9, 3)), ["other"])


# ---- trainer hooks -------------------------------------------------------------------------------------------------------------------
DESED_CLASSES = ["Alarm_bell_ringing", "Blender", "Cat", "Dishes", "Dog", "Electric_shaver_toothbrush", "Frying", "Running_water",
                 "Speech", "Vacuum_cleaner"]


@contextlib.contextmanager
def _recipe_stand_in(tmp):
    """tests/mini_desed.py takes two things from a recipe checkout: `local.classes_dict.classes_labels` and confs/default.yaml.
    Stand-ins for both, so that the miniature also builds where no recipe is installed (the GPU host)."""
    import collections
    import yaml
    recipe = os.path.join(tmp, "recipe")
    os.makedirs(os.path.join(recipe, "confs"), exist_ok=True)
    with open(os.path.join(recipe, "confs", "default.yaml"), "w") as f:
        yaml.safe_dump({"data": {}, "training": {}, "scaler": {}}, f)
    saved = {k: sys.modules.get(k) for k in ("local", "local.classes_dict")}
    pkg, mod = types.ModuleType("local"), types.ModuleType("local.classes_dict")
    pkg.__path__ = []
    mod.classes_labels = collections.OrderedDict((c, i) for i, c in enumerate(DESED_CLASSES))
    pkg.classes_dict = mod
    sys.modules["local"], sys.modules["local.classes_dict"] = pkg, mod
    try:
        yield recipe
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@contextlib.contextmanager
def _count_device_calls():
    """How often the device path ran (the hooks must really take it with the flag on, and never with it off)."""
    calls = []
    real = D.psds_from_score_buffer

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    D.psds_from_score_buffer = counted
    try:
        yield calls
    finally:
        D.psds_from_score_buffer = real


def _run_2023(dev, cfg, out_dir, flag):
    import yaml
    from oracle import sed_oracle as O
    bs, n_samp = (1, 1, 2), 16000 + 1024
    B = sum(bs)
    n_out = (1 + n_samp // 256) // 4
    data = yaml.safe_load(open(cfg))["data"]
    task = P.build_task(dev, bs, O.make_state_dict(seed=7), dropout=0.5, specaug=True, rampup=100)
    task.hparams["data"] = data
    task.hparams["training"].update(val_thresholds=[0.3, 0.5], median_window=7, n_test_thresholds=10, device_psds=flag)
    task.hparams["log_dir"] = out_dir
    task.encoder = P._Encoder(DESED_CLASSES, audio_len=n_samp / 16000.0)
    task.eval()
    val = sorted(os.listdir(data["synth_val_folder"]))
    weak = sorted(os.listdir(data["weak_folder"]))
    assert len(val) == 4
    for step in range(2):
        names = ([os.path.join(data["synth_val_folder"], f) for f in val[2 * step:2 * step + 2]]
                 + [os.path.join(data["weak_folder"], f) for f in weak[2 * step:2 * step + 2]])
        audio, labels = O.synth_audio(B, n_samp, seed=21 + step), O.synth_labels(bs, 10, n_out, seed=5 + step)
        task.validation_step((P.to(dev, audio), P.to(dev, labels), None, names, None), step)
    if flag:
        assert task.val_scores_postprocessed_buffer_student_synth == {} and task.val_scores_postprocessed_buffer_teacher_synth == {}
        assert len(task.val_scores_device_buffer_student) == 4
    else:
        assert len(task.val_scores_postprocessed_buffer_student_synth) == 4 and task.val_scores_device_buffer_student is None
    task.validation_epoch_end([])
    logged = {k: float(task.logged[k]) for k in ("val/obj_metric", "val/synth/student/psds1_sed_scores_eval")}
    assert task.val_scores_postprocessed_buffer_student_synth == {}
    assert (len(task.val_scores_device_buffer_student) == 0) if flag else (task.val_scores_device_buffer_student is None)
    names = [os.path.join(data["test_folder"], f) for f in sorted(os.listdir(data["test_folder"]))]
    assert len(names) == B
    audio, labels = O.synth_audio(B, n_samp, seed=31), O.synth_labels(bs, 10, n_out, seed=7)
    task.test_step((P.to(dev, audio), P.to(dev, labels), None, names, None), 0)
    res = task.on_test_epoch_end()
    for who in ("student", "teacher"):
        for k in ("psds1_sed_scores_eval", "psds2_sed_scores_eval"):
            logged["test/%s/%s" % (who, k)] = float(res["test/%s/%s" % (who, k)])
    written = sorted(os.path.relpath(os.path.join(r, f), out_dir) for r, _, fs in os.walk(out_dir) for f in fs)
    return logged, written


def case_hooks_2023(dev, tmp):
    """Assertion 5, 2023 trainer (the pretrained trainer inherits these hooks): validation and test epochs over the miniature DESED
    of tests/mini_desed.py with `training.device_psds` on log what they log with it off, and write the same files."""
    from tests import mini_desed
    with _recipe_stand_in(tmp) as recipe:
        cfg = mini_desed.build(tmp, recipe)
    runs = {}
    for flag in (False, True):
        out_dir = os.path.join(tmp, "exp_%d" % flag)
        with _count_device_calls() as calls:
            runs[flag] = _run_2023(dev, cfg, out_dir, flag)
        assert len(calls) == (5 if flag else 0), calls              # validation: student; test: two scenarios x two models
    (off, files_off), (on, files_on) = runs[False], runs[True]
    assert set(off) == set(on) and len(on) == 6
    for k in off:
        assert abs(off[k] - on[k]) <= 1e-12, (k, off[k], on[k])
    assert files_off == files_on and any("scores" in f for f in files_on)
    for rel in files_off:
        a, b = (open(os.path.join(tmp, "exp_%d" % flag, rel), "rb").read() for flag in (0, 1))
        assert a == b, rel


def _validate_2024(dev, tmp, flag, n_samp=16000 * 2 + 1024, te=53):
    """One validation batch and epoch end of the 2024 trainer on the in-memory miniature of eval2024_cases (ground truth = the 0.5
    decoding of the student's own tables, which this trainer builds with the flag on too)."""
    import pandas as pd
    from tests import eval2024_cases as E
    task = E._task(dev, n_samp)
    task.hparams["training"]["device_psds"] = flag
    files = (["/d/synth_val/s%d.wav" % i for i in range(3)] + ["/d/maestro_train/m%d.wav" % i for i in range(3)]
             + ["/d/weak/w%d.wav" % i for i in range(2)] + ["/d/other/u0.wav"])
    task.hparams["data"] = {"weak_folder": "/d/weak", "synth_val_folder": "/d/synth_val/", "real_maestro_train_folder": "/d/maestro_train"}
    task.validation_step(E._batch(dev, files, n_samp, te, seed=41)[-1], 0)
    tables = task.val_buffer_sed_scores_eval_student
    assert len(tables) == 6
    assert (len(task.val_scores_device_buffer_student) == 6) if flag else (task.val_scores_device_buffer_student is None)
    ts = task.encoder._frame_to_time(np.arange(len(tables["s0"]) + 1))
    dur = n_samp / 16000.0
    synth_rows, maestro_rows, maestro_classes = [], [], set()
    for aid in sorted(tables):
        arr = tables[aid].values[:, 2:]
        if aid.startswith("s"):
            ev = E._decode(arr[:, :10], ts, E.DESED)
            synth_rows += [(aid + ".wav", a, b, c) for c, a, b in ev] or [(aid + ".wav", np.nan, np.nan, np.nan)]
        else:
            ev = E._decode(arr[:, 10:], ts, E.MAESTRO)
            maestro_rows += [(aid + ".wav", a, b, c, 1.0) for c, a, b in ev]
            maestro_classes |= {c for c, _, _ in ev}
    assert len(synth_rows) > 3 and maestro_classes
    task.hparams["class_labels"] = {"desed": E.DESED, "maestro_real": E.MAESTRO, "maestro_real_eval": set(sorted(maestro_classes)[:6])}
    paths = {k: os.path.join(tmp, k + ".tsv") for k in ("synth_val_tsv", "synth_val_dur", "real_maestro_train_tsv")}
    pd.DataFrame(synth_rows, columns=["filename", "onset", "offset", "event_label"]).to_csv(paths["synth_val_tsv"], sep="\t", index=False)
    pd.DataFrame({"filename": ["s%d.wav" % i for i in range(3)], "duration": dur}).to_csv(paths["synth_val_dur"], sep="\t", index=False)
    pd.DataFrame(maestro_rows, columns=["filename", "onset", "offset", "event_label", "confidence"]).to_csv(
        paths["real_maestro_train_tsv"], sep="\t", index=False)
    task.hparams["data"].update(paths)
    task.logged.clear()
    task.validation_epoch_end(None)
    assert set(task.logged) == E.EPOCH_KEYS
    assert task.val_buffer_sed_scores_eval_student == {}
    assert (len(task.val_scores_device_buffer_student) == 0) if flag else (task.val_scores_device_buffer_student is None)
    return {k: float(v) for k, v in task.logged.items()}


def case_hooks_2024(dev, tmp):
    """Assertion 5, 2024 trainer: the six threshold-free PSDS keys (validation: student, teacher; test: two scenarios x two models)
    with the flag on equal those with it off; its other metrics still read the tables and do not move either."""
    from tests import eval2024_cases as E
    real_task = E._task

    def flagged(dev_, n_samp):
        task = real_task(dev_, n_samp)
        task.hparams["training"]["device_psds"] = True
        return task
    keys_val = ["val/%s/psds1/sed_scores_eval" % who for who in ("student", "teacher")]
    keys_test = ["test/%s/%s/sed_scores_eval" % (who, s) for who in ("student", "teacher") for s in ("psds1", "psds2")]
    got = {}
    for flag in (False, True):
        with _count_device_calls() as calls:
            d = os.path.join(tmp, "v%d" % flag)
            os.makedirs(d)
            val = _validate_2024(dev, d, flag)
            n_val = len(calls)
            d = os.path.join(tmp, "t%d" % flag)
            os.makedirs(d)
            E._task = flagged if flag else real_task
            try:
                res = E.case_test_2024(dev, d)
            finally:
                E._task = real_task
        assert (n_val, len(calls) - n_val) == ((2, 4) if flag else (0, 0)), (n_val, len(calls))
        got[flag] = dict(val, **{k: float(v) for k, v in res.items()})
    for k in keys_val + keys_test:
        assert abs(got[False][k] - got[True][k]) <= 1e-12, (k, got[False][k], got[True][k])
    for k in got[False]:                                                # every other key: untouched code, same tables
        assert got[False][k] == got[True][k] or (np.isnan(got[False][k]) and np.isnan(got[True][k])) or k in keys_val + keys_test, k
