"""Drop-in for the pretrained-embeddings trainer, recipes/dcase2023_task4_baseline/local/sed_trainer_pretrained.py
(SURVEY 8f rank 3): the same mean-teacher step with frozen per-clip embeddings (BEATs: 768 x 496) handed to the student and
the teacher (`detect(features, model, embeddings)`, :276-280), fused into the CRNN by K14 + `cat_tf`
(nnet/CRNN.py, `use_embeddings=True, aggregation_type="pool1d"`).

`pretrained.e2e: False` -- embeddings pre-computed and delivered with the batch `(audio, labels, padded_indxs, embeddings)`
(:291-292; validation / test: `(..., filenames, embeddings)`).

`pretrained.e2e: True` with `freezed: True` (:63-65, :291-312, :405-423, :668-686) -- batches arrive without embeddings,
`(audio, labels, padded_indxs)` / `(audio, labels, padded_indxs, filenames)`, and the frozen extractor `pretrained_model` runs
inside the step: once per step, the same tensor for student and teacher, not mixed up.  It is a registered submodule (its weights
are in `state_dict()` under `pretrained_model.`, as in the reference), kept in eval mode, without gradients, in neither the optimizer
nor the EMA.  A `desed_task_amd.beats.BEATsModel` hands over its token-major output where it lies (`embeddings(audio, "frame")`,
read by sed_embcat_tokens_fwd) and is part of the captured whole step.  It runs serially at the head of the step, in the pipelined
step too: on the prefetch branch beside the backward pass it was measured slower (profiles/e2e_step.md), so the front half stays as
it is and a replayed step reads its own waveforms (`step_reads_waveforms`).  Any other module with the reference's dict surface
(`pretrained_model(audio)[embedding_type]`) runs eagerly (`_whole_step_blockers`).
Refused: `freezed: False` (no extractor backward exists), `e2e: True` without a `pretrained_model`, `net.embedding_type` other
than "frame" (`aggregation_type: global` is refused by the CRNN).

Everything else (losses, EMA, scheduler, logged keys, validation / test scoring) is inherited unchanged from
sed_trainer.SEDTask4, as in the reference where the two files differ only by the `embeddings` plumbing.
"""
import torch

from . import graph as _graph
from .beats import BEATsModel
from .sed_trainer import SEDTask4 as _SEDTask4


class SEDTask4(_SEDTask4):
    _e2e = False

    def __init__(self, hparams, encoder, sed_student, pretrained_model=None, opt=None, train_data=None, valid_data=None,
                 test_data=None, train_sampler=None, scheduler=None, fast_dev_run=False, evaluation=False, sed_teacher=None):
        pre = hparams.get("pretrained", {}) or {}
        e2e = bool(pre.get("e2e", False))
        if e2e:
            if not pre.get("freezed", False):
                raise NotImplementedError("pretrained.freezed must be True with pretrained.e2e: training the extractor inside the "
                                          "step is not built (no extractor backward exists)")
            if pretrained_model is None:
                raise ValueError("pretrained.e2e: True needs the extractor: SEDTask4(..., pretrained_model=BEATsModel(...))")
            kind = (hparams.get("net", {}) or {}).get("embedding_type", "global")
            if kind != "frame":
                raise NotImplementedError("net.embedding_type: %r with pretrained.e2e: the step is built for 'frame' embeddings "
                                          "(aggregation_type pool1d / interpolate)" % (kind,))
        super().__init__(hparams, encoder, sed_student, opt=opt, train_data=train_data, valid_data=valid_data,
                         test_data=test_data, train_sampler=train_sampler, scheduler=scheduler, fast_dev_run=fast_dev_run,
                         evaluation=evaluation, sed_teacher=sed_teacher)
        self._e2e = e2e
        if e2e:
            self.pretrained_model = pretrained_model            # (:63-64: a submodule, so its weights are in the state dict)
            pretrained_model.eval()
            for p in pretrained_model.parameters():
                p.requires_grad_(False)

    def train(self, mode=True):
        super().train(mode)
        if self._e2e:
            self.pretrained_model.eval()                        # frozen: the trainer's .train() / .eval() sweeps do not reach it
        return self

    # ---- e2e: the frozen extractor inside the step ------------------------------------------------------------------------
    def _extract(self, audio):
        """Frame embeddings (B, E, Te) of the waveforms (:305-312): once per step, before the front half."""
        pm = self.pretrained_model
        if pm.training:
            pm.eval()                                           # :307-309
        kind = self.hparams["net"]["embedding_type"]
        with torch.no_grad():
            if isinstance(pm, BEATsModel):
                # the view of its token-major output, no copy; its host draws are made by _extractor_draws()
                return pm.embeddings(audio, kind, host_draws=False)
            return pm(audio)[kind].detach()

    def _extractor_draws(self):
        """The numpy draws the reference extractor's forward makes (BEATs.host_draws), at the place of the step's host-draw order
        where the reference runs it: in front of the mixup draws (:305-330).  They belong to the FRONT half, so that a front half
        prefetched one step early consumes the same stream as the inline order; a captured step re-runs them before every replay.
        A foreign extractor makes its own draws when it is called."""
        pm = self.pretrained_model
        if isinstance(pm, BEATsModel):
            dyn = _graph.active()
            if dyn is not None:
                dyn.host(pm.model.host_draws)
            else:
                pm.model.host_draws()

    def _front(self, audio, labels, fresh=False, x_into_pro=False):
        if self._e2e:
            self._extractor_draws()
        return super()._front(audio, labels, fresh=fresh, x_into_pro=x_into_pro)

    @property
    def step_reads_waveforms(self):
        """The step itself reads batch[0] -- also when its front half was prefetched (graph.GraphedStepDriver then refreshes the
        waveforms' static buffer before every replay, which a pipelined step otherwise never reads)."""
        return self._e2e

    def _batch_embeddings(self, batch):
        if self._e2e:
            return self._extract(batch[0])
        if len(batch) < 4 or batch[3] is None:
            raise ValueError("the pretrained step expects batches (audio, labels, padded_indxs, embeddings)")
        return batch[3]

    # validation / test batches of the pretrained recipe are (audio, labels, padded_indxs, filenames, embeddings)
    def _eval_embeddings(self, batch):
        if self._e2e:
            self._extractor_draws()
            return self._extract(batch[0])                      # (audio, labels, padded_indxs, filenames), :405-423, :668-686
        if len(batch) < 5 or batch[4] is None:
            raise ValueError("the pretrained validation / test step expects (audio, labels, padded_indxs, filenames, embeddings)")
        return batch[4]
