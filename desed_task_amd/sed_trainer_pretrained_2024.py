"""Drop-in for the training step of the 2024 recipe's trainer, recipes/dcase2024_task4_baseline/local/sed_trainer_pretrained.py
(SURVEY 8f rank 3): the mean-teacher step over FIVE data sets per batch -- [MAESTRO | synthetic | strong real | weak |
unlabelled] -- with frozen embeddings, per-clip `valid_class_mask`, mixup inside each data set and consistency losses on
everything but MAESTRO (:318-430).

Same surface as the reference class for the step: constructor (with `pretrained_model`), `mel_spec`, `scaler`, `take_log`,
`detect(mel_feats, model, embeddings=None, **kwargs)`, `apply_mixup`, `training_step`, the EMA / scheduler hooks and the nine
logged keys.  Batches are `(audio, labels, padded_indxs, embeddings, valid_class_mask)` (:333-335).

Reference behaviours kept on purpose: the labels of a data-set group are mixed TWICE when embeddings are present -- once with
the features' (c, perm), once more with the embeddings' own draw (:283-301); the weak labels are derived after mixup (:354);
`train/student/tot_supervised` logs the strong consistency loss (:415); the consistency weight stops ramping at
`training.epoch_decay` (:393-396).

Validation and test (:441-1300): batches `(audio, labels, padded_indxs, filenames, embeddings, valid_class_mask)`; the eval-mode
forward of both models (with `classes_mask` in validation, without it in test, as there), the class-wise median filter of
`net.median_filter` and the decoding on the device (postprocess.batched_decode_preds with a ClassWiseMedianFilter: one launch per
model and batch); the epoch-end metrics on this package's host evaluators -- DESED synth-val PSDS1 / intersection F1 / collar F1,
MAESTRO segment best F1 / mAUC / mpAUC (evaluation/segment_based.py) after the per-recording overlap-add of device segment means
(evaluation/maestro.py) -- with the reference's logged keys, objective selection and score-file layout.  The intersection and
collar F1 at 0.5 of sed_scores_eval are computed from the score tables decoded at `score > 0.5` by psds.PSDSEval and
sed_eval_metrics.EventBasedMetrics.  The codecarbon energy keys are not produced.

Class names: `class_labels={"desed": ..., "maestro_real": ..., "maestro_real_eval": ...}` given to the constructor or as
hparams["class_labels"]; else the recipe's own `local.classes_dict` (reachable when the recipe directory is on the path).

Not built: `pretrained.e2e` in this (2024) trainer -- it raises, as the reference's does (:305-309).  The recipe's own `net:` section (n_RNN_cell 192, 27 classes, dropstep_recurrent) is what the parity
fixtures use.
"""
import os
import random
from pathlib import Path

import numpy as np
import torch

from . import features
from . import graph as _graph
from .data_augm import MixupBatch, mixup_inplace_
from .ops import MeanTeacherLossFn
from .sed_trainer_pretrained import SEDTask4 as _SEDTask4


class SEDTask4(_SEDTask4):
    # `current_epoch` is LightningModule's read-only property under real Lightning; the stand-in base (sed_trainer._Base) carries
    # a plain attribute that a hand-written loop may set.  Nothing is defined here so that neither is shadowed.

    def __init__(self, hparams, encoder, sed_student, pretrained_model=None, opt=None, train_data=None, valid_data=None,
                 test_data=None, train_sampler=None, scheduler=None, fast_dev_run=False, evaluation=False, sed_teacher=None,
                 class_labels=None):
        super().__init__(hparams, encoder, sed_student, pretrained_model=pretrained_model, opt=opt, train_data=train_data,
                         valid_data=valid_data, test_data=test_data, train_sampler=train_sampler, scheduler=scheduler,
                         fast_dev_run=fast_dev_run, evaluation=evaluation, sed_teacher=sed_teacher)
        from .postprocess import ClassWiseMedianFilter
        # :70 -- net.median_filter, one window per class (confs/pretrained.yaml); a configuration without it decodes unfiltered
        wins = self.hparams.get("net", {}).get("median_filter")
        self.median_filter = ClassWiseMedianFilter(wins) if wins is not None else None
        self._class_labels = class_labels

    def detect(self, mel_feats, model, embeddings=None, **kwargs):
        x = self.scaled_logmel(mel_feats)
        if embeddings is None:
            return model(x, **kwargs)
        return model(x, embeddings=embeddings, **kwargs)

    def _unpack_batch(self, batch):
        if self.hparams["pretrained"]["e2e"]:
            raise NotImplementedError                       # as the reference (:306-316)
        if len(batch) not in (5, 6):
            raise ValueError("the 2024 recipe expects batches (audio, labels, padded_indxs, embeddings, valid_class_mask) for "
                             "training and (audio, labels, padded_indxs, filenames, embeddings, valid_class_mask) for validation / test")
        return batch

    def apply_mixup(self, features_, embeddings, labels, start_indx, stop_indx, dyn=None, gate=None, batches=(None, None)):
        """Mixup inside one data set, in place (:283-301): features + labels, then embeddings + labels again (second draw).
        batches: two MixupBatch objects -- the first-draw mixups of all data sets go out as one launch, the second-draw ones as
        another (the labels of a group are mixed by both draws, in this order)."""
        mixup_type = self.hparams["training"].get("mixup")
        sl = slice(start_indx, stop_indx)
        if stop_indx <= start_indx:
            return features_, embeddings, labels
        mixup_inplace_(features_[sl], labels[sl], mixup_label_type=mixup_type, dyn=dyn, gate=gate, batch=batches[0])
        if embeddings is not None:
            mixup_inplace_(embeddings[sl], labels[sl], mixup_label_type=mixup_type, dyn=dyn, gate=gate, batch=batches[1])
        return features_, embeddings, labels

    # ---- pipelined front half (SEDTask4.launch_prefetch, round 4) ---------------------------------------------------------------
    # The 2024 front half is mel -> mixup inside each data set (features + labels, then embeddings + labels again) -> weak labels
    # -> log / min-max.  Announced one step early it works on COPIES of the announced labels and embeddings (the hand-over buffers
    # `_pro["labels"]`, `_pro["embeddings"]`), so the caller's tensors are only read.
    prefetched_batch_fields = (1, 3)    # labels and embeddings come out of the hand-over buffers

    def next_batch_extras(self, next_batch):
        if len(next_batch) < 4 or next_batch[3] is None:
            raise ValueError("the 2024 step expects batches (audio, labels, padded_indxs, embeddings, valid_class_mask)")
        return {"embeddings": next_batch[3]}

    def _group_bounds(self):
        return tuple(int(v) for v in np.cumsum(self.hparams["training"]["batch_size"]))

    def _front_2024(self, audio, labels, embeddings, fresh=False, x_into_pro=False):
        """mel -> per-data-set mixup of (features, labels) and (embeddings, labels), in place on the tensors given -> weak labels
        (after mixup, :354) -> log / min-max (:318-356).  Host draws in the reference's order.  -> (x, labels_weak)"""
        features_ = self._features(audio, fresh)
        indx_maestro, indx_synth, indx_strong, indx_weak, indx_unlabelled = self._group_bounds()
        if indx_weak > features_.shape[0]:
            raise ValueError("batch smaller than the configured data-set sizes")
        mixup_type = self.hparams["training"].get("mixup")
        groups = ((indx_strong, indx_weak), (indx_maestro, indx_strong), (0, indx_maestro))          # :341-351, in this order
        dyn = _graph.active()
        if dyn is not None and mixup_type is not None:
            def flip():
                dyn.state["mixup"] = self.hparams["training"]["mixup_prob"] > random.random()
            dyn.host(flip)
            gate = lambda: dyn.state["mixup"]       # noqa: E731
            mbs = (MixupBatch(), MixupBatch())
            for a, b in groups:
                self.apply_mixup(features_, embeddings, labels, a, b, dyn=dyn, gate=gate, batches=mbs)
            mbs[0].launch()
            mbs[1].launch()
        elif mixup_type is not None and self.hparams["training"]["mixup_prob"] > random.random():
            mbs = (MixupBatch(), MixupBatch())
            for a, b in groups:
                self.apply_mixup(features_, embeddings, labels, a, b, batches=mbs)
            mbs[0].launch()
            mbs[1].launch()
        labels_weak = features.weak_labels(labels[indx_strong:indx_weak])       # after mixup (:354); class masking: loss kernel
        x_out = self._pro_buffer("x", features_) if x_into_pro else None
        return self.scaled_logmel(features_, out=x_out), labels_weak

    @staticmethod
    def _dense_embeddings(embeddings):
        embeddings = embeddings.float()
        return embeddings if embeddings.is_contiguous() else embeddings.contiguous()

    def _prefetch_front(self, audio, labels, extras):
        lab = self._pro_buffer("labels", labels)
        lab.copy_(labels)
        src = self._dense_embeddings(extras["embeddings"])
        emb = self._pro_buffer("embeddings", src)
        emb.copy_(src)
        return self._front_2024(audio, lab, emb, fresh=True, x_into_pro=True)

    def _training_step(self, batch, batch_indx):
        audio, labels, padded_indxs, embeddings, valid_class_mask = self._unpack_batch(batch)
        indx_maestro, indx_synth, indx_strong, indx_weak, indx_unlabelled = self._group_bounds()
        valid = (valid_class_mask != 0).to(torch.uint8).contiguous()
        dyn = _graph.active()
        pro = self._pro if (self._pro is not None and self._pro["ready"]) else None
        if pro is not None:
            # the previous step ran this step's front half and the teacher's CNN forward under its backward
            pro["ready"] = False
            if pro["labels"].shape != labels.shape or pro["embeddings"].shape != embeddings.shape:
                raise RuntimeError("the prefetched front half does not match this batch's shape")
            x, ht = pro["x"], pro["ht"]               # (x: volatile, the student's CNN copies it in its prologue launch)
            labels, labels_weak, embeddings = pro["labels"], pro["labels_weak"], pro["embeddings"]
        else:
            embeddings = self._dense_embeddings(embeddings)
            x, labels_weak = self._front_2024(audio, labels, embeddings)
            ht = None
        strong_s, weak_s, strong_t, weak_t = self._forward_pair(x, ht, embeddings, volatile_x=pro is not None, classes_mask=valid)

        sched = self.scheduler["scheduler"]
        const_max = self.hparams["training"]["const_max"]
        decay = self.hparams["training"].get("epoch_decay", float("inf"))

        def weight_now():
            return const_max * sched._get_scaling_factor() if self.current_epoch < decay else const_max
        weight = dyn.scalar(dyn.F_LOSS_W, weight_now) if dyn is not None else weight_now()
        scalars, tot_loss = MeanTeacherLossFn.apply(strong_s.transpose(1, 2), weak_s, strong_t.transpose(1, 2), weak_t, labels,
                                                    labels_weak, indx_strong, indx_weak - indx_strong, weight, self.selfsup_bce,
                                                    indx_maestro, valid)
        loss_strong, loss_weak, _, _, strong_self, weak_self, tot_self_loss, _ = scalars.unbind(0)
        lr = lambda: self.opt.param_groups[-1]["lr"] if self.opt is not None else 0.0      # noqa: E731
        self.log("train/student/loss_strong", loss_strong.detach())
        self.log("train/student/loss_weak", loss_weak.detach())
        if dyn is not None:
            dyn.host(lambda: (self.log("train/step", sched.step_num, prog_bar=True), self.log("train/lr", lr(), prog_bar=True)))
        self.log("train/step", sched.step_num, prog_bar=True)
        self.log("train/student/tot_self_loss", tot_self_loss, prog_bar=True)
        self.log("train/weight", weight.tensor if dyn is not None else weight)
        self.log("train/student/tot_supervised", strong_self.detach(), prog_bar=True)      # sic (reference :415)
        self.log("train/student/weak_self_sup_loss", weak_self.detach())
        self.log("train/student/strong_self_sup_loss", strong_self.detach())
        self.log("train/lr", lr(), prog_bar=True)
        self.last_outputs = (strong_s, weak_s, strong_t, weak_t)
        return tot_loss

    # ---- validation / test of the 2024 recipe (:441-1300) ----------------------------------------------------------------------
    def class_lists(self):
        """(DESED classes, MAESTRO real classes, evaluated MAESTRO real classes), each sorted as the reference sorts them."""
        cl = self._class_labels if self._class_labels is not None else self.hparams.get("class_labels")
        if cl is None:
            try:
                from local.classes_dict import (classes_labels_desed, classes_labels_maestro_real,
                                                classes_labels_maestro_real_eval)
            except ImportError as e:
                raise RuntimeError("the 2024 metrics need the class names: pass class_labels={'desed': ..., 'maestro_real': ..., "
                                   "'maestro_real_eval': ...} or put the recipe directory (local/classes_dict.py) on the path") from e
            cl = {"desed": classes_labels_desed, "maestro_real": classes_labels_maestro_real,
                  "maestro_real_eval": classes_labels_maestro_real_eval}
        return sorted(cl["desed"]), sorted(cl["maestro_real"]), sorted(cl["maestro_real_eval"])

    def _val_state(self):
        """Buffers of :120-137, created on first use (the training-only configurations carry no val keys)."""
        if not hasattr(self, "val_buffer_sed_scores_eval_student"):
            self.val_buffer_sed_scores_eval_student = {}
            self.val_buffer_sed_scores_eval_teacher = {}
            self.get_weak_student_f1_seg_macro = _SEDTask4._MacroF1()
            self.get_weak_teacher_f1_seg_macro = _SEDTask4._MacroF1()
        if not hasattr(self, "val_scores_device_buffer_student"):
            self._reset_device_scores("val")

    def _append_device_scores(self, dev_buf, preds, filenames):
        """`training.device_psds`: the filtered scores of a batch also go to a ScoreBuffer, which only the threshold-free PSDS reads;
        the other metrics of this recipe read the score tables, so those are still built."""
        from .postprocess import _btc, _filter_batch
        if dev_buf is None:
            return
        scores = _filter_batch(_btc(preds), self.median_filter)
        dev_buf.append(scores, [Path(f).stem for f in filenames], timestamps=self.encoder._frame_to_time(np.arange(scores.shape[1] + 1)),
                       event_classes=self.encoder.labels)

    def _eval_forward(self, audio, embeddings, classes_mask=None):
        """Eval-mode forward of student and teacher on the same features (the reference's two `detect` calls)."""
        kw = {} if classes_mask is None else {"classes_mask": classes_mask}
        with torch.no_grad():
            x = self.scaled_logmel(self.mel_spec(audio))
            embeddings = self._dense_embeddings(embeddings)
            strong_s, weak_s = self.sed_student(x, embeddings=embeddings, **kw)
            strong_t, weak_t = self.sed_teacher(x, embeddings=embeddings, **kw)
        return strong_s, weak_s, strong_t, weak_t

    def validation_step(self, batch, batch_indx):
        """:441-573: weak BCE + macro F1 on the weak clips, strong BCE on the synth-val and MAESTRO-train clips, whose
        class-wise median-filtered score tables (no thresholds) go to the buffers -- one filter launch per model."""
        from .postprocess import batched_decode_preds
        audio, labels, padded_indxs, filenames, embeddings, valid_class_mask = self._unpack_batch(batch)
        self._val_state()
        strong_s, weak_s, strong_t, weak_t = self._eval_forward(audio, embeddings, valid_class_mask)
        data = self.hparams["data"]
        bce = torch.nn.functional.binary_cross_entropy
        strong_dirs = [str(Path(data["synth_val_folder"])), str(Path(data["real_maestro_train_folder"]))]
        is_weak = [str(Path(f).parent) == str(Path(data["weak_folder"])) for f in filenames]
        is_strong = [str(Path(f).parent) in strong_dirs for f in filenames]
        mask_weak = torch.tensor(is_weak, device=audio.device)
        mask_strong = torch.tensor(is_strong, device=audio.device)
        if any(is_weak):
            labels_weak = (torch.sum(labels[mask_weak], -1) >= 1).float()
            self.log("val/weak/student/loss_weak", bce(weak_s[mask_weak], labels_weak))
            self.log("val/weak/teacher/loss_weak", bce(weak_t[mask_weak], labels_weak))
            self.get_weak_student_f1_seg_macro(weak_s[mask_weak], labels_weak.long())
            self.get_weak_teacher_f1_seg_macro(weak_t[mask_weak], labels_weak.long())
        if any(is_strong):
            self.log("val/synth/student/loss_strong", bce(strong_s[mask_strong], labels[mask_strong]))
            self.log("val/synth/teacher/loss_strong", bce(strong_t[mask_strong], labels[mask_strong]))
            filenames_strong = [f for f, m in zip(filenames, is_strong) if m]
            for preds, buf, dev_buf in ((strong_s, self.val_buffer_sed_scores_eval_student, self.val_scores_device_buffer_student),
                                        (strong_t, self.val_buffer_sed_scores_eval_teacher, self.val_scores_device_buffer_teacher)):
                _, scores_post, _ = batched_decode_preds(preds[mask_strong], filenames_strong, self.encoder,
                                                         median_filter=self.median_filter, thresholds=[])
                buf.update(scores_post)
                self._append_device_scores(dev_buf, preds[mask_strong], filenames_strong)
        return

    @staticmethod
    def _detections(scores, threshold=0.5):
        """Events of the score tables at `score > threshold`: filename (id + .wav) / onset / offset / event_label rows."""
        import pandas as pd
        from .evaluation.segment_based import _table
        rows = []
        for clip_id, df in scores.items():
            ts, classes, arr = _table(df)
            on = np.pad(arr > threshold, ((1, 1), (0, 0)))
            d = np.diff(on.astype(np.int8), axis=0)
            for c in range(arr.shape[1]):
                starts, ends = np.nonzero(d[:, c] == 1)[0], np.nonzero(d[:, c] == -1)[0]
                rows.extend((clip_id + ".wav", ts[a], ts[b], classes[c]) for a, b in zip(starts, ends))
        return pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])

    @staticmethod
    def _event_table(ground_truth, durations):
        import pandas as pd
        gt = pd.DataFrame([(k + ".wav", a, b, c) for k, evs in ground_truth.items() for a, b, c in evs],
                          columns=["filename", "onset", "offset", "event_label"])
        meta = pd.DataFrame([(k + ".wav", durations[k]) for k in ground_truth], columns=["filename", "duration"])
        return gt, meta

    def _desed_f1_at_05(self, scores, ground_truth, durations, dev_buf=None):
        """sed_scores_eval's intersection_based.fscore (dtc = gtc = 0.5) and collar_based.fscore (200 ms collar, 20 % offset
        rate) macro averages at threshold 0.5 (:617-636), on psds.PSDSEval and sed_eval_metrics.EventBasedMetrics.  With
        `training.device_f1` the detections are not decoded: both scores are counted from `dev_buf`, the DESED columns of the
        scored clips, by the `sed_f1_counts` kernel (evaluation/f1_device.py)."""
        from .evaluation.evaluation_measures import compute_per_intersection_macro_f1, event_based_evaluation_df
        gt, meta = self._event_table(ground_truth, durations)
        if dev_buf is not None and self._device_f1():
            from .evaluation.f1_device import DecodedScores, sedeval_f1
            det = DecodedScores(dev_buf, 0.5, classes=self.class_lists()[0], ids=list(scores))
            inter = compute_per_intersection_macro_f1({"0.5": det}, gt, meta, dtc_threshold=0.5, gtc_threshold=0.5)
            if det.empty:
                return float(inter), 0.0
            return float(inter), float(sedeval_f1(det, gt, t_collar=0.2, percentage_of_length=0.2)[0])
        det = self._detections(scores, 0.5)
        inter = compute_per_intersection_macro_f1({"0.5": det}, gt, meta, dtc_threshold=0.5, gtc_threshold=0.5)
        if det.empty:
            return float(inter), 0.0
        ev = event_based_evaluation_df(gt, det, t_collar=0.2, percentage_of_length=0.2)
        return float(inter), float(ev.results()["class_wise_average"]["f_measure"]["f_measure"])

    def _desed_scores(self, buffer, tsv, dur):
        """DESED ground truth without empty clips, and the DESED columns of those clips' score tables (:588-612, :1045-1065).
        Unlike the 2023 trainer this ignores fast_dev_run, as the 2024 reference does: its buffers also hold MAESTRO clips,
        which the DESED tables do not list, and the recipe validates on the whole set under --fast_dev_run."""
        from .evaluation.psds_scores import read_audio_durations, read_ground_truth_events
        desed, _, _ = self.class_lists()
        ground_truth = {k: gt for k, gt in read_ground_truth_events(tsv).items() if len(gt) > 0}
        durations = read_audio_durations(dur)
        durations = {k: durations[k] for k in ground_truth}
        keys = ["onset", "offset"] + desed
        return {k: buffer[k][keys] for k in ground_truth}, ground_truth, durations

    def _psds_from_scores(self, tables, dev_buf, ground_truth, durations, **kw):
        """compute_psds_from_scores on the DESED score tables, or with `training.device_psds` on the ScoreBuffer with the DESED
        columns selected (the tables are then only what `save_dir` writes)."""
        from .evaluation.evaluation_measures import compute_psds_from_scores
        if dev_buf is None:
            return compute_psds_from_scores(tables, ground_truth, durations, **kw)
        return compute_psds_from_scores(dev_buf, ground_truth, durations, classes=self.class_lists()[0], tables=tables, **kw)

    def _maestro_gt(self, tsv, eval_classes):
        import pandas as pd
        from .evaluation.psds_scores import read_ground_truth_events
        df = pd.read_csv(tsv, sep="\t")
        df = df[df.confidence > 0.5]
        return read_ground_truth_events(df[df.event_label.isin(eval_classes)])

    def _segment_metrics(self, scores, ground_truth, durations):
        """Segment best F1 (macro), mAUC and mpAUC (max_fpr 0.1) at 1 s segments; the segments are scored once for all three."""
        from .evaluation import segment_based as S
        seg = S.segment_scores_and_targets(scores, ground_truth, durations, segment_length=1.0)
        return (S.best_fscore_of_segments(*seg)[0]["macro_average"], S.auroc_of_segments(*seg)[0]["mean"],
                S.auroc_of_segments(*seg, max_fpr=0.1)[0]["mean"])

    def validation_epoch_end(self, outputs=None):
        """:575-821 -- same metrics, objective selection, logged keys and buffer resets."""
        from .evaluation.maestro import merge_overlapping_events
        self._val_state()
        data = self.hparams["data"]
        _, _, maestro_eval = self.class_lists()
        weak_student_f1_macro = self.get_weak_student_f1_seg_macro.compute()
        weak_teacher_f1_macro = self.get_weak_teacher_f1_seg_macro.compute()
        res = {}
        for who, buf, dev_buf in (("student", self.val_buffer_sed_scores_eval_student, self.val_scores_device_buffer_student),
                                  ("teacher", self.val_buffer_sed_scores_eval_teacher, self.val_scores_device_buffer_teacher)):
            scores, gt, dur = self._desed_scores(buf, data["synth_val_tsv"], data["synth_val_dur"])
            res[who, "psds1"] = self._psds_from_scores(scores, dev_buf, gt, dur, dtc_threshold=0.7, gtc_threshold=0.7,
                                                       cttc_threshold=None, alpha_ct=0, alpha_st=1)
            res[who, "inter"], res[who, "collar"] = self._desed_f1_at_05(scores, gt, dur, dev_buf)
        maestro_gt = {k: v for k, v in self._maestro_gt(data["real_maestro_train_tsv"], maestro_eval).items()
                      if k in self.val_buffer_sed_scores_eval_student}
        maestro_gt = merge_overlapping_events(maestro_gt)
        maestro_dur = {k: sorted(evs, key=lambda e: e[1])[-1][1] for k, evs in maestro_gt.items()}       # last offset (:690)
        keys = ["onset", "offset"] + maestro_eval
        for who, buf in (("student", self.val_buffer_sed_scores_eval_student), ("teacher", self.val_buffer_sed_scores_eval_teacher)):
            scores = {k: buf[k][keys] for k in maestro_gt}
            res[who, "fmo"], res[who, "mauc"], res[who, "mpauc"] = self._segment_metrics(scores, maestro_gt, maestro_dur)

        synth_type = self.hparams["training"].get("obj_metric_synth_type")
        synth_key = {None: "psds1", "psds": "psds1", "collar": "collar", "intersection": "inter"}.get(synth_type)
        if synth_key is None:
            raise NotImplementedError(f"obj_metric_synth_type: {synth_type} not implemented.")
        maestro_type = self.hparams["training"].get("obj_metric_maestro_type")
        # "mpauc" selects the best-threshold F1, as in the reference (:765-766)
        maestro_key = {None: "mpauc", "fmo": "fmo", "mauc": "mauc", "mpauc": "fmo"}.get(maestro_type)
        if maestro_key is None:
            raise NotImplementedError(f"obj_metric_maestro_type: {maestro_type} not implemented.")
        obj_metric = torch.tensor(float(weak_student_f1_macro) + float(res["student", synth_key]) + float(res["student", maestro_key]))
        self.log("val/obj_metric", obj_metric, prog_bar=True)
        self.log("val/student/weak_f1_macro_thres05/torchmetrics", weak_student_f1_macro)
        self.log("val/teacher/weak_f1_macro_thres05/torchmetrics", weak_teacher_f1_macro)
        for who in ("student", "teacher"):
            self.log(f"val/{who}/intersection_f1_macro_thres05/sed_scores_eval", res[who, "inter"])
        for who in ("student", "teacher"):
            self.log(f"val/{who}/collar_f1_macro_thres05/sed_scores_eval", res[who, "collar"])
        for who in ("student", "teacher"):
            self.log(f"val/{who}/psds1/sed_scores_eval", res[who, "psds1"])
        for who in ("student", "teacher"):
            self.log(f"val/{who}/segment_f1_macro_thresopt/sed_scores_eval", res[who, "fmo"])
            self.log(f"val/{who}/segment_mauc/sed_scores_eval", res[who, "mauc"])
            self.log(f"val/{who}/segment_mpauc/sed_scores_eval", res[who, "mpauc"])
        self.val_buffer_sed_scores_eval_student = {}
        self.val_buffer_sed_scores_eval_teacher = {}
        self._reset_device_scores("val")
        self.get_weak_student_f1_seg_macro.reset()
        self.get_weak_teacher_f1_seg_macro.reset()
        return obj_metric

    def _test_state(self):
        """Buffers of :139-155, created on first use."""
        if not hasattr(self, "test_buffer_psds_eval_student"):
            import pandas as pd
            n = self.hparams["training"]["n_test_thresholds"]
            ths = np.arange(1 / (n * 2), 1, 1 / n)
            self.test_buffer_psds_eval_student = {k: pd.DataFrame() for k in ths}
            self.test_buffer_psds_eval_teacher = {k: pd.DataFrame() for k in ths}
            self.test_buffer_sed_scores_eval_student = {}
            self.test_buffer_sed_scores_eval_teacher = {}
            self.test_buffer_sed_scores_eval_unprocessed_student = {}
            self.test_buffer_sed_scores_eval_unprocessed_teacher = {}
            self.test_buffer_detections_thres05_student = pd.DataFrame()
            self.test_buffer_detections_thres05_teacher = pd.DataFrame()
        if not hasattr(self, "test_scores_device_buffer_student"):
            self._reset_device_scores("test")

    def test_step(self, batch, batch_indx):
        """:828-922: posteriors without classes_mask, class-wise filtered and decoded at the n_test_thresholds + 0.5 on the
        device (one filter and one region launch per model and batch)."""
        import pandas as pd
        from .postprocess import batched_decode_preds
        audio, labels, padded_indxs, filenames, embeddings, valid_class_mask = self._unpack_batch(batch)
        self._test_state()
        strong_s, weak_s, strong_t, weak_t = self._eval_forward(audio, embeddings)
        if not self.evaluation:
            bce = torch.nn.functional.binary_cross_entropy
            self.log("test/student/loss_strong", bce(strong_s, labels))
            self.log("test/teacher/loss_strong", bce(strong_t, labels))
        for who, preds in (("student", strong_s), ("teacher", strong_t)):
            psds_buf = getattr(self, f"test_buffer_psds_eval_{who}")
            raw, post, decoded = batched_decode_preds(preds, filenames, self.encoder, median_filter=self.median_filter,
                                                      thresholds=list(psds_buf.keys()) + [0.5])
            getattr(self, f"test_buffer_sed_scores_eval_unprocessed_{who}").update(raw)
            getattr(self, f"test_buffer_sed_scores_eval_{who}").update(post)
            self._append_device_scores(getattr(self, f"test_scores_device_buffer_{who}"), preds, filenames)
            for th in psds_buf.keys():
                psds_buf[th] = pd.concat([psds_buf[th], decoded[th]], ignore_index=True)
            name = f"test_buffer_detections_thres05_{who}"
            setattr(self, name, pd.concat([getattr(self, name), decoded[0.5]]))

    def on_test_epoch_end(self):
        """:924-1300.  `evaluation=True`: only the score tables are written ({student,teacher}_scores/{unprocessed,postprocessed}).
        Otherwise the 22 `test/...` keys; the MAESTRO segment score tables are written under {student,teacher}/maestro/postprocessed."""
        import pandas as pd
        from .evaluation.evaluation_measures import (compute_per_intersection_macro_f1, compute_psds_from_operating_points,
                                                     log_sedeval_metrics)
        from .evaluation.maestro import merge_maestro_ground_truth, segment_scores_and_overlap_add
        from .evaluation.psds_scores import read_audio_durations
        from .postprocess import write_sed_scores
        self._test_state()
        save_dir = os.path.join(self.exp_dir, "metrics_test")
        results = {}
        if self.evaluation:
            for who in ("student", "teacher"):
                for kind, buf in (("unprocessed", getattr(self, f"test_buffer_sed_scores_eval_unprocessed_{who}")),
                                  ("postprocessed", getattr(self, f"test_buffer_sed_scores_eval_{who}"))):
                    write_sed_scores(buf, os.path.join(save_dir, f"{who}_scores", kind))
                    print(f"\n{kind} scores for {who} saved in: {os.path.join(save_dir, who + '_scores', kind)}")
        else:
            data = self.hparams["data"]
            _, maestro_real, maestro_eval = self.class_lists()
            psds1 = dict(dtc_threshold=0.7, gtc_threshold=0.7, alpha_ct=0, alpha_st=1)
            psds2 = dict(dtc_threshold=0.1, gtc_threshold=0.1, cttc_threshold=0.3, alpha_ct=0.5, alpha_st=1)
            # MAESTRO ground truth per recording (:1146-1172)
            maestro_dur_all = read_audio_durations(data["real_maestro_val_dur"])
            maestro_clip_ids = list(dict.fromkeys(f[:-4] for f in pd.read_csv(data["real_maestro_val_tsv"], sep="\t")["filename"]))
            maestro_gt = merge_maestro_ground_truth(self._maestro_gt(data["real_maestro_val_tsv"], maestro_eval))
            maestro_dur = {k: maestro_dur_all[k] for k in maestro_gt}
            keys_eval = ["onset", "offset"] + maestro_eval
            for who in ("student", "teacher"):
                buf = getattr(self, f"test_buffer_psds_eval_{who}")
                buf05 = getattr(self, f"test_buffer_detections_thres05_{who}")
                post = getattr(self, f"test_buffer_sed_scores_eval_{who}")
                d = os.path.join(save_dir, who)
                results[f"test/{who}/psds1/psds_eval"] = compute_psds_from_operating_points(
                    buf, data["test_tsv"], data["test_dur"], save_dir=os.path.join(d, "scenario1"), **psds1)
                results[f"test/{who}/psds2/psds_eval"] = compute_psds_from_operating_points(
                    buf, data["test_tsv"], data["test_dur"], save_dir=os.path.join(d, "scenario2"), **psds2)
                results[f"test/{who}/intersection_f1_macro_thres05/psds_eval"] = compute_per_intersection_macro_f1(
                    {"0.5": buf05}, data["test_tsv"], data["test_dur"])
                results[f"test/{who}/collar_f1_macro_thres05/sed_eval"] = log_sedeval_metrics(buf05, data["test_tsv"], d)[0]
                scores, gt, dur = self._desed_scores(post, data["test_tsv"], data["test_dur"])
                dev_buf = getattr(self, f"test_scores_device_buffer_{who}")
                results[f"test/{who}/psds1/sed_scores_eval"] = self._psds_from_scores(
                    scores, dev_buf, gt, dur, cttc_threshold=None, save_dir=os.path.join(d, "scenario1"), **psds1)
                results[f"test/{who}/psds2/sed_scores_eval"] = self._psds_from_scores(
                    scores, dev_buf, gt, dur, save_dir=os.path.join(d, "scenario2"), **psds2)
                (results[f"test/{who}/intersection_f1_macro_thres05/sed_scores_eval"],
                 results[f"test/{who}/collar_f1_macro_thres05/sed_scores_eval"]) = self._desed_f1_at_05(scores, gt, dur, dev_buf)
                # MAESTRO: device segment means per clip, overlap-add per recording (:1174-1214)
                seg = segment_scores_and_overlap_add({k: post[k] for k in maestro_clip_ids}, maestro_dur, maestro_real,
                                                     segment_length=1.0, device=self._eval_device())
                write_sed_scores(seg, os.path.join(d, "maestro", "postprocessed"))
                seg = {k: df[keys_eval] for k, df in seg.items()}
                (results[f"test/{who}/segment_f1_macro_thresopt/sed_scores_eval"],
                 results[f"test/{who}/segment_mauc/sed_scores_eval"],
                 results[f"test/{who}/segment_mpauc/sed_scores_eval"]) = self._segment_metrics(seg, maestro_gt, maestro_dur)
            order = ["psds1/psds_eval", "psds2/psds_eval", "intersection_f1_macro_thres05/psds_eval", "collar_f1_macro_thres05/sed_eval",
                     "psds1/sed_scores_eval", "psds2/sed_scores_eval", "intersection_f1_macro_thres05/sed_scores_eval",
                     "collar_f1_macro_thres05/sed_scores_eval", "segment_f1_macro_thresopt/sed_scores_eval",
                     "segment_mauc/sed_scores_eval", "segment_mpauc/sed_scores_eval"]
            results = {f"test/{who}/{k}": results[f"test/{who}/{k}"] for k in order for who in ("student", "teacher")}
        logger = getattr(self, "logger", None)
        if logger is not None:
            logger.log_metrics(results)
            logger.log_hyperparams(self.hparams, results)
        for key in results.keys():
            self.log(key, results[key], prog_bar=True, logger=True)
        return results

    def _eval_device(self):
        p = next(self.sed_student.parameters(), None)
        return p.device if p is not None else torch.device("cuda", torch.cuda.current_device())
