"""`pretrained.e2e: True` -- the frozen BEATs extractor inside the 2023 `pretrained` training step -- layer by layer: the
token-major embedding-fusion kernel (sed_embcat_tokens_fwd) against its twin and against float64, the layout dispatch of
ops.EmbCatFn, and sed_trainer_pretrained.SEDTask4 with `pretrained_model=` against the step on pre-computed embeddings, the
oracle composition, the reference fixture, validation / test, the pipelined and the captured step, and the refusals.  One set of
cases for the CPU emulator (tests/test_emu_e2e.py) and the MI355X (tests/test_gpu_e2e.py).

Small step: batch sizes (2, 2, 2); clips of 400 + 255 * 160 = 41 200 samples = 256 fbank frames = 16 x 8 = 128 tokens, and 161 mel
frames = 40 CRNN frames (ragged, overlapping 128 -> 40 windows of 4); 6 x 128 = 768 extractor rows (the tile-image Linears run);
BEATS_ITER3_CFG with two encoder layers.  Both runners use these shapes and step counts.
"""
import functools
import os
import random

import numpy as np
import torch

from desed_task_amd import _lib
from oracle import beats_oracle as BO
from oracle import sed_oracle as O
from tests import parity_cases as P
from tests.contraction_cases import CANARY, Frame, SED_ERR_ARG, SED_ERR_UNSUPPORTED, rc, stream, sync

HERE = os.path.dirname(os.path.abspath(__file__))
BS = (2, 2, 2)
N_SAMP = 400 + 255 * 160


def n_tok(n_samp):
    return ((1 + (n_samp - 400) // 160) // 16) * 8


def n_out(n_samp):
    return (1 + n_samp // 256) // 4


U24 = 2.0 ** -24
to = P.to

# (B, T, Te, C, E): the recipe's ragged 51 -> 16, the small step's 128 -> 40, one frame / odd E (element-wise path), Te < T
# (repeated windows), Te = T (windows of one), and E % 4 == 0 behind a C that is no multiple of 4 (vector loads, element-wise stores)
KERNEL_SHAPES = ((3, 16, 51, 128, 768), (2, 40, 128, 128, 768), (1, 1, 7, 5, 70), (2, 16, 7, 128, 70), (2, 16, 16, 8, 64),
                 (2, 5, 9, 6, 8))


def _seed_all(dev, s=101):
    from desed_task_amd import ops as _ops
    random.seed(41)
    np.random.seed(s)
    torch.manual_seed(s)
    if dev != "cpu":
        torch.cuda.manual_seed(s)
    _ops.reseed_dropout()


def _tmask(B, T):
    """dropstep spans (B, 4) [x0, x1, e0, e1): a full embedding span, an empty one, a partial one."""
    rows = [[1, min(T, 3), 0, T], [0, 0, 2, 2], [0, T, 1, min(T, 3)]]
    return torch.tensor([rows[b % 3] for b in range(B)], dtype=torch.int32)


def _kernel_inputs(B, T, Te, C, E):
    x = O.lcg_fill((B, T, C), 1 + T, 1.0)
    tok = O.lcg_fill((B, Te, E), 2 + Te, 1.0)
    return x, tok


def _run_entry(dev, entry, x, src, B, T, Te, C, E, seed, thr24, dscale, seed_dev, tmask, mode, misalign=0):
    """One forward call into a canary-framed z (B T, C + E); src: the embeddings in the entry's own layout -> (z, frame)."""
    W = C + E
    zf = Frame(dev, B * T, W, misalign=misalign)
    sf = Frame(dev, src.shape[0] * src.shape[1], src.shape[2], misalign=misalign).put(src.reshape(-1, src.shape[2]))
    xd = to(dev, x).contiguous()
    code = rc(entry, xd.data_ptr(), sf.ptr(), zf.ptr(), B, T, Te, C, E, seed, thr24, dscale,
              seed_dev.data_ptr() if seed_dev is not None else None, tmask.data_ptr() if tmask is not None else None, mode, stream(dev))
    sync(dev)
    assert code == 0, (entry, code)
    zf.assert_frame("%s z %r" % (entry, (B, T, Te, C, E)))
    sf.assert_frame("%s embeddings %r" % (entry, (B, T, Te, C, E)))
    return zf.get().view(B, T, W)


def case_kernel_equals_twin(dev, shape):
    """1: sed_embcat_tokens_fwd on tok (B, Te, E) == sed_embcat_fwd on its transposed copy, bit for bit, in a canary frame: both
    modes, dropout off / on (p = 0.5, seed + seed_dev), without / with dropstep spans (full, empty, partial), 16-byte aligned and
    one float off (the element-wise path, element-wise stores)."""
    from desed_task_amd import ops
    B, T, Te, C, E = shape
    x, tok = _kernel_inputs(*shape)
    emb = tok.transpose(1, 2).contiguous()
    seed_dev = to(dev, torch.tensor([977], dtype=torch.int32))
    n = 0
    for mode in (0, 1):
        for p in (0.0, 0.5):
            thr24, dscale = ops.dropout_params(p)
            for tmask in (None, to(dev, _tmask(B, T))):
                for mis in (0, 1):
                    args = (B, T, Te, C, E, 4242 if p else 0, thr24, dscale, seed_dev if p else None, tmask, mode, mis)
                    z_twin = _run_entry(dev, "sed_embcat_fwd", x, emb, *args)
                    z_tok = _run_entry(dev, "sed_embcat_tokens_fwd", x, tok, *args)
                    same = z_twin.view(torch.int32) == z_tok.view(torch.int32)
                    assert bool(same.all()), ("bits differ", shape, mode, p, tmask is not None, mis, int((~same).sum()))
                    n += 1
    return n


def case_kernel_vs_float64(dev, shape):
    """2: the pooled columns against float64 pooling of the same tokens, per element within
    1.01 (n + 1) / n 2^-24 sum|x_i| dscale for a window of n rows (n - 1 additions, one division, one scale); dropped elements are 0
    and follow the documented mask; the x columns are exact copies (scaled by a power of two or by 1)."""
    from desed_task_amd import ops
    B, T, Te, C, E = shape
    x, tok = _kernel_inputs(*shape)
    t64 = tok.double()
    t = torch.arange(T)
    lo, hi = (t * Te) // T, ((t + 1) * Te + T - 1) // T
    ref = torch.stack([t64[:, int(a):int(b)].mean(1) for a, b in zip(lo, hi)], 1)                       # (B, T, E)
    mag = torch.stack([t64[:, int(a):int(b)].abs().sum(1) for a, b in zip(lo, hi)], 1)
    cnt = (hi - lo).double().view(1, T, 1)
    worst = 0.0
    for p, seed in ((0.0, 0), (0.5, 77)):
        thr24, dscale = ops.dropout_params(p)
        z = _run_entry(dev, "sed_embcat_tokens_fwd", x, tok, B, T, Te, C, E, seed, thr24, dscale, None, None, 0)
        keep = P.np_keep_mask((B, T, C + E), seed, p) if p else torch.ones(B, T, C + E)
        keep = torch.as_tensor(keep).double()
        bound = 1.01 * (cnt + 1) / cnt * U24 * mag * dscale
        err = (z[..., C:].double() - ref * dscale * keep[..., C:]).abs()
        assert bool((err <= bound).all()), (shape, p, float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert torch.equal(z[..., :C].double(), x.double() * dscale * keep[..., :C]), (shape, p)
    # mode 1: the nearest-exact source row itself
    z = _run_entry(dev, "sed_embcat_tokens_fwd", x, tok, B, T, Te, C, E, 0, 0, 1.0, None, None, 1)
    src = torch.clamp(((2 * t + 1) * Te) // (2 * T), max=Te - 1)
    assert torch.equal(z[..., C:], tok[:, src]), shape
    return worst


def case_kernel_refusals(dev):
    """3: the twin's codes: bad mode, E / C / Te < 1 -> SED_ERR_ARG; B T (C + E) >= 2^32, (T + 1) Te + T >= 2^31, C > 2^20 ->
    SED_ERR_UNSUPPORTED; an empty batch is a no-op.  Nothing is launched: z keeps its canaries."""
    zf = Frame(dev, 4, 16)
    buf = to(dev, torch.zeros(64))
    s = stream(dev)
    rows = [((2, 4, 4, 4, 4, 2), SED_ERR_ARG), ((2, 4, 4, 4, 4, -1), SED_ERR_ARG), ((2, 4, 4, 4, 0, 0), SED_ERR_ARG),
            ((2, 4, 4, 0, 4, 0), SED_ERR_ARG), ((2, 4, 0, 4, 4, 0), SED_ERR_ARG),
            ((1 << 12, 1 << 10, 4, 128, 896, 0), SED_ERR_UNSUPPORTED),           # B T (C + E) = 2^32
            ((1, 1 << 16, 1 << 15, 4, 4, 0), SED_ERR_UNSUPPORTED),               # T Te = 2^31
            ((1, 4, 4, (1 << 20) + 1, 4, 0), SED_ERR_UNSUPPORTED),
            ((0, 4, 4, 4, 4, 0), 0), ((2, 0, 4, 4, 4, 0), 0)]
    for (B, T, Te, C, E, mode), want in rows:
        for entry in ("sed_embcat_tokens_fwd", "sed_embcat_fwd"):
            got = rc(entry, buf.data_ptr(), buf.data_ptr(), zf.ptr(), B, T, Te, C, E, 0, 0, 1.0, None, None, mode, s)
            assert got == want, (entry, (B, T, Te, C, E, mode), got, want)
    sync(dev)
    assert bool((zf.buf.cpu() == CANARY).all())


class _Calls:
    """Records (entry, args) of every lib.call while active."""

    def __enter__(self):
        self.lib = _lib.get()
        self.seen = []
        orig = self.lib.call

        def call(name, *a):
            self.seen.append((name, a))
            return orig(name, *a)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        del self.lib.call

    def names(self):
        return [n for n, _ in self.seen]


def case_dispatch(dev):
    """4: EmbCatFn on the (B, E, Te) view of token-major storage (and a clone() of it) calls sed_embcat_tokens_fwd on the storage
    itself -- no copy; a contiguous (B, E, Te) tensor calls sed_embcat_fwd.  CRNN forward + backward in train mode with dropout and
    dropstep on: posteriors and every parameter gradient are bit-equal between the view and its contiguous copy."""
    from desed_task_amd import ops
    from desed_task_amd.nnet.CRNN import CRNN
    B, T, Te, C, E = 2, 16, 51, 128, 768
    x, tok = _kernel_inputs(B, T, Te, C, E)
    w, b = O.lcg_fill((C, C + E), 3, 0.03), O.lcg_fill((C,), 4, 0.1)
    tok_d = to(dev, tok)
    view = tok_d.transpose(1, 2)
    cfg = dict(dropout_p=0.5, apply_dropout=True, seed=99)
    outs = []
    for emb, entry in ((view, "sed_embcat_tokens_fwd"), (view.clone(), "sed_embcat_tokens_fwd"), (view.contiguous(), "sed_embcat_fwd")):
        with _Calls() as calls:
            outs.append(ops.EmbCatFn.apply(to(dev, x), emb, to(dev, w), to(dev, b), cfg).cpu())
        hit = [a for n, a in calls.seen if n.startswith("sed_embcat")]
        assert [n for n in calls.names() if n.startswith("sed_embcat")] == [entry], calls.names()
        assert hit[0][1] == emb.data_ptr(), "the embeddings were copied"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # a half-precision or otherwise strided tensor goes the old way
    with _Calls() as calls:
        ops.EmbCatFn.apply(to(dev, x), view.double(), to(dev, w), to(dev, b), cfg)
    assert "sed_embcat_fwd" in calls.names() and "sed_embcat_tokens_fwd" not in calls.names()
    # ---- the CRNN on both layouts ----
    sd = O.make_state_dict(seed=7, embedding_size=768)
    ncfg = dict(P.pretrained_net_config(), dropout=0.5, dropstep_recurrent=0.3)
    xin = O.lcg_fill((2, 128, 64), 41, 0.5, 0.5)
    res = []
    for layout in ("view", "dense"):
        net = CRNN(**ncfg)
        net.load_state_dict({k: v.clone() for k, v in sd.items()})
        net = net.to(dev) if dev != "cpu" else net
        net.train()
        _seed_all(dev, 55)
        emb = view if layout == "view" else view.contiguous()
        with _Calls() as calls:
            strong, weak = net(to(dev, xin), embeddings=emb)
        assert ("sed_embcat_tokens_fwd" in calls.names()) == (layout == "view")
        (strong.sum() + (weak * weak).sum()).backward()
        res.append((strong.detach().cpu(), weak.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert set(res[0][2]) == set(res[1][2]) and len(res[0][2]) > 40
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[1][2][n]), n


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
BEATS_CFG = dict(BO.BEATS_ITER3_CFG, encoder_layers=2)


@functools.lru_cache(maxsize=None)
def _beats_sd():
    return BO.make_beats_state_dict(BEATS_CFG, seed=5)


def make_extractor(dev, precision=None):
    from desed_task_amd.beats import BEATsModel
    ex = BEATsModel(checkpoint={"cfg": dict(BEATS_CFG), "model": {k: v.clone() for k, v in _beats_sd().items()}}, precision=precision)
    return ex.to(dev) if dev != "cpu" else ex


@functools.lru_cache(maxsize=None)
def small_batches(n_samp=N_SAMP, n=7):
    """n batches (audio (6, n_samp), labels (6, 10, CRNN frames)) of the small step."""
    B = sum(BS)
    return tuple((O.synth_audio(B, n_samp, seed=700 + 13 * i), O.synth_labels(BS, 10, n_out(n_samp), seed=5 + i)) for i in range(n))


def make_config(e2e, dropout=0.5):
    config = P.recipe_config(BS)
    config["net"] = dict(P.pretrained_net_config(), dropout=dropout)
    config["pretrained"] = {"e2e": bool(e2e), "freezed": True, "model": "beats"}
    return config


def build_task(dev, e2e, extractor=None, dropout=0.5, specaug=True, rampup=100, config=None):
    from desed_task_amd.arena import FusedAdam
    from desed_task_amd.nnet.CRNN import CRNN
    from desed_task_amd.sed_trainer_pretrained import SEDTask4
    from desed_task_amd.utils.schedulers import ExponentialWarmup
    config = make_config(e2e, dropout) if config is None else config
    extra = {} if specaug else {"specaugm_t_p": 0.0, "specaugm_f_p": 0.0}
    student = CRNN(**config["net"], **extra)
    student.load_state_dict({k: v.clone() for k, v in O.make_state_dict(seed=7, embedding_size=768).items()})
    student = student.to(dev) if dev != "cpu" else student
    opt = FusedAdam(student.parameters(), lr=1e-3, betas=(0.9, 0.999), arena=student.arena)
    sched = {"scheduler": ExponentialWarmup(opt, 1e-3, rampup), "interval": "step"}

    class Enc:
        labels = list(range(10))
    task = SEDTask4(config, Enc(), student, pretrained_model=extractor, opt=opt, scheduler=sched)
    task.whole_step = False
    task.train()
    if dev != "cpu":
        task.to(dev)
        opt.arena = task.sed_student.arena
    return task


def _logged(task, loss=None):
    got = {k: (float(v) if not torch.is_tensor(v) else float(v.detach().cpu())) for k, v in task.logged.items()}
    if loss is not None:
        got["loss"] = float(loss.detach().cpu())
    return got


def _state(task):
    return (task.sed_student.arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone())


def case_e2e_equals_precomputed(dev, steps=3, n_samp=N_SAMP):
    """5: `e2e: True` on (audio, labels, None) == `e2e: False` on (audio, labels, None, extractor(audio)["frame"]): same weights,
    same host seeds, three optimiser steps through StepDriver with mixup, dropout and SpecAugment on -- loss, every logged scalar,
    the four posterior tensors and every parameter (student and teacher) bit-equal."""
    from desed_task_amd.launcher import StepDriver
    res = []
    for e2e in (True, False):
        ex = make_extractor(dev)
        task = build_task(dev, e2e, ex if e2e else None)
        driver = StepDriver(task, world_size=1)
        _seed_all(dev)
        hist = []
        for step in range(steps):
            audio, labels = (to(dev, t.clone()) for t in small_batches(n_samp)[step])
            if e2e:
                with _Calls() as calls:
                    loss = driver.run_step((audio, labels, None), step)
                assert calls.names().count("sed_embcat_tokens_fwd") == 2 and "sed_embcat_fwd" not in calls.names()
                assert calls.names().count("sed_kaldi_fbank") == 1, "the extractor runs once per step"
            else:
                loss = driver.run_step((audio, labels, None, ex(audio)["frame"]), step)
            hist.append((_logged(task, loss), [t.detach().cpu().clone() for t in task.last_outputs]))
        res.append((hist, _state(task)))
    (h0, s0), (h1, s1) = res
    for (l0, o0), (l1, o1) in zip(h0, h1):
        assert l0 == l1, (l0, l1)
        assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])
    assert not torch.equal(s0[0], s0[1])
    return h0[-1][0]["loss"]


def case_e2e_vs_oracle(dev, n_samp=N_SAMP):
    """6: the e2e step against oracle(BEATs) -> oracle(step) -> optimizer_step on the same waveforms (dropout / SpecAugment off,
    mixup draws pinned), with case_beats_chain_2024's bounds: embeddings 5e-4 of the scale on the 99.9 % quantile and 1e-2 on the
    maximum (the fbank conditioning documented there), logged scalars 2e-5 + 2e-4 |v|, posteriors 1e-3, gradients 2e-4 (maximum) /
    2e-5 (median) of grad_error_stats.
    Measured on the MI355X at the small step's shapes (returned as a dict): embeddings 2.1e-5 (maximum) / 6.3e-6 (99.9 % quantile)
    of the scale, logged scalars 1.2e-7, posteriors 7.2e-7, gradients 7.4e-6 (maximum) / 0 (median)."""
    from desed_task_amd.launcher import StepDriver
    audio, labels = small_batches(n_samp)[0]
    sd = O.make_state_dict(seed=7, embedding_size=768)
    ex = make_extractor(dev)
    task = build_task(dev, True, ex, dropout=0.0, specaug=False)
    driver = StepDriver(task, world_size=1)
    with torch.no_grad():
        emb_o = BO.beats_embeddings(_beats_sd(), BEATS_CFG, audio)["frame"]
    emb_d = ex.embeddings(to(dev, audio), "frame")
    assert tuple(emb_d.shape) == (sum(BS), 768, n_tok(n_samp)) and emb_d.transpose(1, 2).is_contiguous()
    d_emb = (emb_d.cpu() - emb_o).abs()
    scale = max(1.0, emb_o.abs().max().item())
    e_emb, q_emb = d_emb.max().item(), torch.quantile(d_emb.flatten()[::7], 0.999).item()
    assert q_emb < 5e-4 * scale and e_emb < 1e-2 * scale, (q_emb, e_emb)
    orc = O.OracleTrainer(sd, batch_sizes=BS, lr=1e-3, rampup_len=100)
    random.seed(4); np.random.seed(100); torch.manual_seed(100)
    assert random.random() < 0.5
    for _ in range(BEATS_CFG["encoder_layers"]):
        np.random.random()                 # the extractor's per-layer draws precede the mixup draws (BEATs.host_draws), as in the reference
    cw = np.random.beta(0.2, 0.2); pw = torch.randperm(BS[1]); cs = np.random.beta(0.2, 0.2); ps = torch.randperm(BS[0])
    mix = dict(c_weak=cw, perm_weak=pw, c_strong=cs, perm_strong=ps)
    random.seed(4); np.random.seed(100); torch.manual_seed(100)
    loss = driver.run_step((to(dev, audio.clone()), to(dev, labels.clone()), None), 0)
    tot, logs = orc.training_step(audio, labels.clone(), mix=mix, embeddings=emb_o)
    ref_grads = orc.optimizer_step(tot)
    got = _logged(task, loss)
    logs["loss"] = tot.item()
    worst = {"emb_max": e_emb / scale, "emb_q999": q_emb / scale, "log": 0.0, "post": 0.0, "grad_max": 0.0, "grad_med": 0.0}
    for k in sorted(logs):
        worst["log"] = max(worst["log"], abs(got[k] - logs[k]))
        assert abs(got[k] - logs[k]) <= 2e-5 + 2e-4 * abs(logs[k]), "%s: hip %.8g oracle %.8g" % (k, got[k], logs[k])
    for a, name in zip([t.detach().cpu() for t in task.last_outputs], ("strong_s", "weak_s", "strong_t", "weak_t")):
        err = (a - orc.last[name]).abs().max().item()
        worst["post"] = max(worst["post"], err)
        assert err < 1e-3, (name, err)
    hip_params = dict(task.sed_student.named_parameters())
    for k in O.param_keys(sd):
        if k.startswith("cnn.cnn.conv") and k.endswith(".bias"):
            continue
        emax, emed = P.grad_error_stats(hip_params[k].grad.detach().cpu(), ref_grads[k])
        worst["grad_max"], worst["grad_med"] = max(worst["grad_max"], emax), max(worst["grad_med"], emed)
        assert emax <= 2e-4 and emed <= 2e-5, "grad %s: %.2e / %.2e" % (k, emax, emed)
    return worst


GOLDEN = os.path.join(HERE, "golden", "golden_e2e.npz")
GOLDEN_MIX_SEED = 100


def case_e2e_vs_reference_golden(dev):
    """7: three e2e steps (Lightning hook order, dropout 0, SpecAugment off, mixup coin on and its draws seeded per step) against what
    the reference's 2023 `local.sed_trainer_pretrained.SEDTask4` with `e2e: True` and the reference BEATsModel recorded on the same
    small step (tests/golden/make_golden_e2e.py): every logged scalar and the loss within 2e-5 + 2e-4 |v|, the strided posteriors
    within 1e-3 (case 6's bounds), and the state-dict keys under `pretrained_model.` exactly.  The reference extractor tosses its
    LayerDrop coin (`np.random.random()` per layer) in eval mode too, in front of the mixup draws: steps with a non-trivial mixup
    permutation only agree because BEATs.host_draws makes the same draws.  Measured on the MI355X: scalars 1.8e-6, posteriors 4.1e-6."""
    from desed_task_amd.launcher import StepDriver
    g = np.load(GOLDEN, allow_pickle=False)
    ex = make_extractor(dev)
    task = build_task(dev, True, ex, dropout=0.0, specaug=False)
    keys = sorted(k for k in task.state_dict() if k.startswith("pretrained_model."))
    ref_keys = str(g["pretrained_keys"]).split("\n")
    assert keys == ref_keys, sorted(set(keys) ^ set(ref_keys))
    driver = StepDriver(task, world_size=1)
    names = str(g["log_names"]).split("\n")
    assert len(names) == 12 and g["logs"].shape == (3, 12) and g["posteriors"].shape == (3, 144)
    worst = {"log": 0.0, "post": 0.0}
    for step in range(g["logs"].shape[0]):
        audio, labels = small_batches()[step]
        random.seed(4); np.random.seed(GOLDEN_MIX_SEED + step); torch.manual_seed(GOLDEN_MIX_SEED + step)
        loss = driver.run_step((to(dev, audio.clone()), to(dev, labels.clone()), None), step)
        got = _logged(task, loss)
        for k, ref in zip(names, g["logs"][step]):
            worst["log"] = max(worst["log"], abs(got[k] - float(ref)))
            assert abs(got[k] - float(ref)) <= 2e-5 + 2e-4 * abs(float(ref)), "step %d %s: hip %.8g reference %.8g" % (step, k, got[k], ref)
        s_s, w_s, s_t, w_t = [t.detach().cpu().numpy() for t in task.last_outputs]
        row = np.concatenate([s_s[:, ::4, ::19].ravel(), w_s[:, ::4].ravel(), s_t[:, ::4, ::19].ravel(), w_t[:, ::4].ravel()])
        err = float(np.abs(row - g["posteriors"][step]).max())
        worst["post"] = max(worst["post"], err)
        assert err < 1e-3, (step, err)
    return worst


def _eval_setup(task, n_samp):
    task.hparams["data"] = {"weak_folder": "/d/weak", "synth_val_folder": "/d/synth_val"}
    task.hparams["training"].update(val_thresholds=[0.3, 0.5], median_window=7, n_test_thresholds=5)
    task.encoder = P._Encoder(["c%d" % i for i in range(10)], audio_len=n_samp / 16000.0)
    task.eval()


def _frames_equal(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        return all(_frames_equal(a[k], b[k]) for k in a)
    return a.equals(b)


def case_validation_and_test(dev, n_samp=N_SAMP):
    """8: validation_step / test_step on (audio, labels, padded_indxs, filenames) with `e2e: True` leave the buffers and the logged
    values of the `e2e: False` task fed (..., filenames, extractor(audio)["frame"]), exactly."""
    audio, labels = small_batches(n_samp)[1]
    files = ["/d/synth_val/s%d.wav" % i for i in range(2)] + ["/d/weak/w%d.wav" % i for i in range(2)] + ["/d/other/u%d.wav" % i for i in range(2)]
    tasks = []
    for e2e in (True, False):
        ex = make_extractor(dev)
        task = build_task(dev, e2e, ex if e2e else None)
        _eval_setup(task, n_samp)
        if e2e:
            task.pretrained_model.train()            # (Lightning's .train() / .eval() sweep: the step puts the extractor back)
        a, l = to(dev, audio), to(dev, labels)
        extra = () if e2e else (ex(a)["frame"],)
        task.validation_step((a, l, None, files) + extra, 0)
        val_logs = _logged(task)
        task.test_step((a, l, None, files) + extra, 0)
        tasks.append((task, val_logs, _logged(task)))
        if e2e:
            assert not task.pretrained_model.training
    (t0, v0, l0), (t1, v1, l1) = tasks
    assert v0 == v1 and l0 == l1 and "val/synth/student/loss_strong" in v0 and "test/student/loss_strong" in l0
    for name in ("val_buffer_student_synth", "val_buffer_teacher_synth", "val_scores_postprocessed_buffer_student_synth",
                 "val_scores_postprocessed_buffer_teacher_synth", "test_psds_buffer_student", "test_psds_buffer_teacher",
                 "test_scores_raw_buffer_student", "test_scores_raw_buffer_teacher", "test_scores_postprocessed_buffer_student",
                 "test_scores_postprocessed_buffer_teacher", "decoded_student_05_buffer", "decoded_teacher_05_buffer"):
        assert _frames_equal(getattr(t0, name), getattr(t1, name)), name
    assert len(t0.test_scores_raw_buffer_student) == 6
    for t in (t0.get_weak_student_f1_seg_macro, t0.get_weak_teacher_f1_seg_macro):
        assert t.tp is not None


def case_pipelined(dev, graph=False, steps=5, epoch_end=2, n_samp=N_SAMP):
    """9: the e2e step with its front half -- mel, mixup, log / min-max, the teacher's CNN forward -- pipelined under the previous
    step's backward (prefetch "teacher") and the extractor at the head of the step == the unpipelined eager StepDriver, bit for bit
    in loss and parameters, over DIFFERENT batches (a replay that ran the extractor on stale waveforms would differ) with dropout,
    SpecAugment and mixup on.  Step `epoch_end` announces no next batch (an epoch end); the step after it is re-primed inline; the
    last step announces none either.  graph=True: GraphedStepDriver, capture after one warm-up step; from the second replay on
    nothing falls back to eager launches except the two steps that announce nothing."""
    from desed_task_amd import graph as G
    from desed_task_amd.launcher import StepDriver
    batches = [tuple(to(dev, t) for t in b) for b in small_batches(n_samp)[:steps]]
    originals = [(a.clone(), l.clone()) for a, l in batches]
    results = []
    for mode in ("plain", "pipelined"):
        task = build_task(dev, True, make_extractor(dev))
        pf = "teacher" if mode == "pipelined" else None
        if graph and mode == "pipelined":
            driver = G.GraphedStepDriver(task, world_size=1, warmup=1, prefetch=pf)
        else:
            driver = StepDriver(task, world_size=1, prefetch=pf)
        _seed_all(dev)
        losses, fallbacks = [], []
        for step in range(steps):
            a, l = batches[step]
            if mode == "pipelined":
                nxt = None if (step == epoch_end or step + 1 == steps) else (batches[step + 1][0], batches[step + 1][1], None)
                # (a step whose front half runs inline -- the first, the one after the epoch end -- mixes ITS labels in place, like
                #  the plain step: it gets a copy; what is announced as next_batch is the original tensor, which is only read)
                loss = driver.run_step((a, l.clone(), None), step, next_batch=nxt)
                fallbacks.append(getattr(driver, "eager_fallbacks", 0))
            else:
                loss = driver.run_step((a, l.clone(), None), step)
            losses.append(float(loss.detach()))
        if dev != "cpu":
            torch.cuda.synchronize()
        if mode == "pipelined":
            for (a, l), (ao, lo) in zip(batches, originals):
                assert torch.equal(a, ao) and torch.equal(l, lo), "an announced tensor was modified in place"
            if graph:
                assert task._pro.get("frozen") and driver.graph is not None
                # step 0 eager (warm-up), step 1 the capture, then replays: only the steps that announce nothing run eagerly
                want = [0, 0] + [sum(1 for s in range(2, k + 1) if s == epoch_end or s + 1 == steps) for k in range(2, steps)]
                assert fallbacks == want, (fallbacks, want)
                assert driver.reprimes == 1, driver.reprimes
        results.append((losses, _state(task)))
    (l0, s0), (l1, s1) = results
    assert l0 == l1, (l0, l1)
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])
    return l0


class ForeignExtractor(torch.nn.Module):
    """A plain module with the reference's dict surface (no `embeddings` method): BEATsModel.forward behind it."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def case_refusals_and_surface(dev, n_samp=N_SAMP):
    """10: `freezed: False` and `net.embedding_type != "frame"` raise NotImplementedError, `e2e: True` without a model ValueError,
    each naming its key; a foreign extractor runs the eager step (bit-equal to the BEATsModel's) and is named by
    `_whole_step_blockers`; the extractor's parameters are frozen, in the state dict, in neither optimizer nor EMA; the alias import
    resolves to desed_task_amd.beats."""
    import importlib
    import sys
    import pytest
    from desed_task_amd import beats
    from desed_task_amd.launcher import StepDriver
    ex = make_extractor(dev)
    cfg = make_config(True)
    cfg["pretrained"]["freezed"] = False
    with pytest.raises(NotImplementedError, match="pretrained.freezed"):
        build_task(dev, True, ex, config=cfg)
    with pytest.raises(ValueError, match="pretrained_model"):
        build_task(dev, True, None)
    cfg = make_config(True)
    cfg["net"]["embedding_type"] = "global"
    with pytest.raises(NotImplementedError, match="net.embedding_type"):
        build_task(dev, True, ex, config=cfg)
    with pytest.raises(ValueError, match="kind"):
        ex.embeddings(None, "token")
    # surface
    task = build_task(dev, True, ex)
    plain = build_task(dev, False)
    assert task.pretrained_model is ex and not ex.training
    assert all(not p.requires_grad for p in ex.parameters())
    sd_keys = set(task.state_dict())
    assert {"pretrained_model." + k for k in ex.state_dict()} <= sd_keys and "pretrained_model.model.encoder.layer_norm.weight" in sd_keys
    ids = {id(p) for p in ex.parameters()}
    for t in (task, plain):
        t._opt_ids = [id(p) for grp in t.opt.param_groups for p in grp["params"]]
    assert not ids & set(task._opt_ids) and len(task._opt_ids) == len(plain._opt_ids)
    assert [n for n, _ in task.sed_student.named_parameters()] == [n for n, _ in plain.sed_student.named_parameters()]
    assert [n for n, _ in task.sed_teacher.named_parameters()] == [n for n, _ in plain.sed_teacher.named_parameters()]
    assert task.sed_student.arena.flat.numel() == plain.sed_student.arena.flat.numel()
    assert task._whole_step_blockers() is None
    # a foreign extractor: eager step, same numbers
    res = []
    for foreign in (True, False):
        e = make_extractor(dev)
        t = build_task(dev, True, ForeignExtractor(e) if foreign else e)
        why = t._whole_step_blockers()
        assert (why is not None and "BEATsModel" in why) if foreign else why is None
        if foreign:
            t.whole_step = True
            with pytest.raises(RuntimeError, match="BEATsModel"):
                t._whole_step_on()
            t.whole_step, t._whole_ok = None, None
            assert not t._whole_step_on()                       # auto: the eager step
            t.whole_step = False
        driver = StepDriver(t, world_size=1)
        _seed_all(dev)
        audio, labels = (to(dev, x.clone()) for x in small_batches(n_samp)[0])
        loss = driver.run_step((audio, labels, None), 0)
        res.append((float(loss.detach()), _state(t)))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1][0], res[1][1][0])
    # "global" computes the mean only; forward keeps both entries
    audio = to(dev, small_batches(n_samp)[0][0])
    both = ex(audio)
    assert torch.equal(ex.embeddings(audio, "global"), both["global"]) and torch.equal(ex.embeddings(audio, "frame"), both["frame"])
    # alias modules
    drop_in = os.path.join(os.path.dirname(HERE), "desed_task_amd", "drop_in")
    saved = {k: v for k, v in sys.modules.items() if k == "local" or k.startswith("local.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, drop_in)
    try:
        mod = importlib.import_module("local.beats.BEATs")
        assert mod.BEATsModel is beats.BEATsModel and mod.BEATs is beats.BEATs and mod.BEATsConfig is beats.BEATsConfig
    finally:
        sys.path.remove(drop_in)
        for k in [k for k in sys.modules if k == "local" or k.startswith("local.")]:
            del sys.modules[k]
        sys.modules.update(saved)
