"""Cases for n_RNN_cell = 256 (the widest value of the 2024 recipe's hyper-parameter search): the streamed-weight BiGRU recurrence,
the head at D = 512, the CRNN against the reference module's recorded outputs (tests/golden/golden_rnn256.npz) and the training
step.  Run on the emulator by tests/test_emu_rnn256.py and on the GPU by tests/test_gpu_z_rnn256.py; the per-width cases of
tests/parity_cases.py are called with H = 256 / D = 512, the cases that hard-code 192 there are repeated here for 256."""
import contextlib
import os
import random

import numpy as np
import torch

from oracle import sed_oracle as O
from tests import parity_cases as P
from tests.parity_cases import to

H = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rnn256.npz")


def golden():
    return np.load(GOLDEN)


@contextlib.contextmanager
def wide_recurrence(on=True):
    """n_RNN_cell = 256 is opt-in (ops.GRU_WIDE); the switch is put back, so the modules that run after this one see the default."""
    from desed_task_amd import ops
    prev = ops.GRU_WIDE
    ops.GRU_WIDE = on
    try:
        yield
    finally:
        ops.GRU_WIDE = prev


# ------------------------------------------------------------------------------------------------
# 1. one BiGRU layer against torch's fp32 GRU (output, dX, the eight parameter gradients)
# ------------------------------------------------------------------------------------------------
# (B, T, I): layer 0 with a partial first staging chunk (the kernels stage 2 steps); layer 1; two full chunks + a partial one for any
# chunk length <= 8; an odd batch
EMU_BIGRU_SHAPES = ((2, 7, 128), (1, 10, 512), (1, 19, 128), (3, 5, 128))
GPU_BIGRU_SHAPES = ((4, 156, 128), (3, 156, 512))


def case_bigru(dev, B, T, I):
    P.case_bigru(dev, B=B, T=T, I=I, tol=5e-5 if T >= 156 else 2e-5, H=H)


# ------------------------------------------------------------------------------------------------
# 2. head at D = 512
# ------------------------------------------------------------------------------------------------
def case_head(dev, NC, p=0.5, B=2, T=70):
    P.case_head_dropout(dev, B=B, T=T, p=p, seed=9, D=2 * H, NC=NC)


def case_head_masked(dev, NC=27, B=3, T=37):
    """classes_valid + pad_mask inside the D = 512 head kernels against torch ops (CRNN.py:160-175: -1e30 fills before the class
    softmax, outputs of the classes a clip's data set does not annotate zeroed after the pooling)."""
    from desed_task_amd.ops import HeadFn
    D = 2 * H
    x = O.lcg_fill((B, T, D), 71, 1.0)
    w1 = O.lcg_fill((NC, D), 72, 1.0 / 16); b1 = O.lcg_fill((NC,), 73, 0.1)
    w2 = O.lcg_fill((NC, D), 74, 1.0 / 16); b2 = O.lcg_fill((NC,), 75, 0.1)
    gs = O.lcg_fill((B, T, NC), 76, 1.0); gw = O.lcg_fill((B, NC), 77, 1.0)
    valid = torch.ones(B, NC, dtype=torch.bool)
    valid[0, NC // 3:] = False; valid[1, :NC // 3] = False
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[0, T - 9:] = True; pad[2, T - 1:] = True
    ref_in = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    strong = torch.sigmoid(torch.nn.functional.linear(ref_in[0], ref_in[1], ref_in[2]))
    logit = torch.nn.functional.linear(ref_in[0], ref_in[3], ref_in[4])
    logit = logit.masked_fill(pad[:, :, None], -1e30).masked_fill(~valid[:, None, :], -1e30)
    sof = torch.softmax(logit, dim=-1).clamp(min=1e-7, max=1)
    weak = ((strong * sof).sum(1) / sof.sum(1)).masked_fill(~valid, 0.0)
    strong = strong.masked_fill(~valid[:, None, :], 0.0)
    ((strong * gs).sum() + (weak * gw).sum()).backward()
    hip_in = [to(dev, t).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    cfg = dict(dropout_p=0.0, apply_dropout=False, seed=0, classes_valid=to(dev, valid.to(torch.uint8)).contiguous(),
               pad_mask=to(dev, pad.to(torch.uint8)).contiguous())
    s_h, w_h = HeadFn.apply(*hip_in, cfg)
    ((s_h * to(dev, gs)).sum() + (w_h * to(dev, gw)).sum()).backward()
    assert (s_h.detach().cpu() - strong.detach()).abs().max().item() < 2e-6
    assert (w_h.detach().cpu() - weak.detach()).abs().max().item() < 2e-6
    assert float(s_h.detach()[0, :, NC // 3:].abs().max()) == 0.0 and float(w_h.detach()[1, :NC // 3].abs().max()) == 0.0
    for nm, a, b in zip(("dx", "dW1", "db1", "dW2", "db2"), hip_in, ref_in):
        emax, _ = P.grad_error_stats(a.grad.detach().cpu(), b.grad)
        assert emax < 5e-5, "%s: %.3e" % (nm, emax)


def case_backward_entries_whole_and_split(dev, NC=27):
    """sed_head_bwd at D = 512 and sed_gru_bwd at H = 256 in one call == the records-only call + sed_head_bwd_reduce /
    sed_gru_bias_reduce, bit for bit (tests/parity_cases.py::case_backward_entries_whole_and_split at the new widths)."""
    from desed_task_amd import _lib
    lib = _lib.get()
    f32 = dict(device=dev, dtype=torch.float32)
    st = None if dev == "cpu" else torch.cuda.current_stream().cuda_stream
    nan = float("nan")
    B, T, D = 3, 70, 2 * H
    x = to(dev, O.lcg_fill((B, T, D), 3, 1.0)); w1 = to(dev, O.lcg_fill((NC, D), 4, 0.05)); w2 = to(dev, O.lcg_fill((NC, D), 5, 0.05))
    b1 = to(dev, O.lcg_fill((NC,), 6, 0.1)); b2 = to(dev, O.lcg_fill((NC,), 7, 0.1))
    strong, psoft = torch.empty(B, T, NC, **f32), torch.empty(B, T, NC, **f32)
    weak, den = torch.empty(B, NC, **f32), torch.empty(B, NC, **f32)
    seed, thr24, dscale = 1234, 1 << 23, 2.0
    lib.call("sed_head_fwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), strong.data_ptr(), psoft.data_ptr(),
             weak.data_ptr(), den.data_ptr(), B, T, D, NC, seed, thr24, dscale, None, None, None, st)
    ds = to(dev, O.lcg_fill((B, T, NC), 8, 1.0)); dw = to(dev, O.lcg_fill((B, NC), 9, 1.0))
    n_scr = int(lib.value("sed_head_bwd_scratch_floats", B, T, D, NC))
    assert n_scr == B * ((T + 31) // 32) * (2 * NC * D + 2 * NC)
    outs = []
    for split in (False, True):
        dx = torch.full((B, T, D), nan, **f32)
        g = [torch.full((NC, D), nan, **f32), torch.full((NC, D), nan, **f32), torch.full((NC,), nan, **f32), torch.full((NC,), nan, **f32)]
        scr = torch.full((n_scr,), nan, **f32)
        ptrs = [None] * 4 if split else [t.data_ptr() for t in g]
        lib.call("sed_head_bwd", x.data_ptr(), w1.data_ptr(), w2.data_ptr(), strong.data_ptr(), psoft.data_ptr(), weak.data_ptr(),
                 den.data_ptr(), ds.data_ptr(), dw.data_ptr(), dx.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], B, T, D, NC, seed, thr24,
                 dscale, None, None, None, scr.data_ptr(), st)
        if split:
            assert all(bool(torch.isnan(t).all()) for t in g)          # untouched until the second half runs
            lib.call("sed_head_bwd_reduce", scr.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), B, T, D, NC, st)
        outs.append([dx.cpu()] + [t.cpu() for t in g])
    for a, b_ in zip(*outs):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b_)
    # ---- BiGRU recurrence ----
    B, T = 3, 9
    gi = to(dev, O.lcg_fill((B, T, 2, 3 * H), 11, 0.5))
    whh = [to(dev, O.lcg_fill((3 * H, H), 12 + d, 0.06)) for d in range(2)]
    bhh = [to(dev, O.lcg_fill((3 * H,), 14 + d, 0.1)) for d in range(2)]
    out, saved = torch.empty(B, T, 2 * H, **f32), torch.empty(B, T, 2, 4, H, **f32)
    lib.call("sed_gru_fwd", gi.data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), bhh[0].data_ptr(), bhh[1].data_ptr(), out.data_ptr(),
             saved.data_ptr(), B, T, H, st)
    # inference (saved == NULL) writes the same output
    out2 = torch.full((B, T, 2 * H), nan, **f32)
    lib.call("sed_gru_fwd", gi.data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), bhh[0].data_ptr(), bhh[1].data_ptr(), out2.data_ptr(),
             None, B, T, H, st)
    assert torch.equal(out.cpu(), out2.cpu())
    dout = to(dev, O.lcg_fill((B, T, 2 * H), 16, 1.0))
    outs = []
    for split in (False, True):
        dgi, dgh = torch.full((B, T, 2, 3 * H), nan, **f32), torch.full((B, T, 2, 3 * H), nan, **f32)
        hprev = torch.full((B, T, 2, H), nan, **f32)
        db = [torch.full((3 * H,), nan, **f32) for _ in range(4)]
        scr = torch.full((2 * B * 6 * H,), nan, **f32)
        ptrs = [None] * 4 if split else [t.data_ptr() for t in db]
        lib.call("sed_gru_bwd", dout.data_ptr(), out.data_ptr(), saved.data_ptr(), whh[0].data_ptr(), whh[1].data_ptr(), dgi.data_ptr(),
                 dgh.data_ptr(), hprev.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], B, T, H, scr.data_ptr(), st)
        if split:
            assert all(bool(torch.isnan(t).all()) for t in db)
            lib.call("sed_gru_bias_reduce", scr.data_ptr(), db[0].data_ptr(), db[1].data_ptr(), db[2].data_ptr(), db[3].data_ptr(), B, H, st)
        outs.append([dgi.cpu(), dgh.cpu(), hprev.cpu()] + [t.cpu() for t in db])
    for a, b_ in zip(*outs):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b_)
    # the bias gradients are the column sums of what the recurrence wrote
    dgi, dgh = outs[0][0].double(), outs[0][1].double()
    for d in range(2):
        for got, ref in ((outs[0][3 + d], dgi[:, :, d].sum((0, 1))), (outs[0][5 + d], dgh[:, :, d].sum((0, 1)))):
            assert (got.double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------
# 3. the module against the reference itself (tests/golden/make_golden_rnn256.py)
# ------------------------------------------------------------------------------------------------
def net_config_2024():
    return dict(P.net_config_2024(), n_RNN_cell=H)


def case_crnn_vs_reference_golden(dev, G):
    """tests/parity_cases.py::case_crnn_masks_vs_reference_golden at n_RNN_cell = 256, same tolerances: train-mode posteriors 2e-5,
    loss, every gradient norm 2e-3, two gradient slices 1e-4; with and without embeddings."""
    from desed_task_amd.nnet.CRNN import CRNN
    xin, emb, cm, pad = P.golden_emb2_inputs()
    for tag, use_emb in (("a", True), ("b", False)):
        cfg = dict(net_config_2024(), dropout=0.0, use_embeddings=use_emb)
        sd = O.make_state_dict(seed=7, nclass=27, embedding_size=768 if use_emb else None, hidden=H)
        net = CRNN(**cfg)
        assert [n for n, _ in net.named_parameters()] == list(G[tag + "_param_names"])
        net.load_state_dict({k: v.clone() for k, v in sd.items()})
        net = net.to(dev) if dev != "cpu" else net
        net.train()
        spans = [torch.from_numpy(s.astype(np.int32)) for s in G[tag + "_dropstep"]]
        order = iter(spans)
        net._dropstep_bounds = lambda B, n_time, device, _o=order: next(_o).to(device).contiguous()      # the reference's own draws
        strong, weak = net(to(dev, xin), pad_mask=to(dev, pad), embeddings=to(dev, emb) if use_emb else None, classes_mask=to(dev, cm))
        assert np.abs(strong.detach().cpu().numpy() - G[tag + "_strong"]).max() < 2e-5, tag
        assert np.abs(weak.detach().cpu().numpy() - G[tag + "_weak"]).max() < 2e-5, tag
        assert float(strong.detach()[0, 10:].abs().max()) == 0.0 and float(weak.detach()[1, :10].abs().max()) == 0.0
        tgt_s = to(dev, (O.lcg_fill(tuple(strong.shape), 31, 0.5, 0.5) < 0.2).float())
        tgt_w = to(dev, (O.lcg_fill(tuple(weak.shape), 32, 0.5, 0.5) < 0.3).float())
        loss = torch.nn.functional.binary_cross_entropy(strong, tgt_s) + torch.nn.functional.binary_cross_entropy(weak, tgt_w)
        assert abs(loss.item() - float(G[tag + "_loss"][0])) < 2e-5 * float(G[tag + "_loss"][0]), tag
        loss.backward()
        params = dict(net.named_parameters())
        for n, ref in zip(list(G[tag + "_param_names"]), G[tag + "_grad_norms"]):
            if n.startswith("cnn.cnn.conv") and n.endswith(".bias"):
                continue
            assert abs(params[n].grad.norm().item() - ref) <= 2e-3 * ref + 1e-7, (tag, n)
        got = params["dense_softmax.weight"].grad.detach().cpu().numpy()[:, ::8]
        ref = G[tag + "_grad__dense_softmax.weight"]
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-7, tag
        got = params["cnn.cnn.conv6.weight"].grad.detach().cpu().numpy().reshape(-1)[:512]
        ref = G[tag + "_grad__cnn.cnn.conv6.weight"]
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-7, tag


def case_oracle_vs_reference_golden(G):
    """oracle.crnn_forward at hidden = 256 == the reference module (CPU only; tests/test_oracle_golden.py does this for 192)."""
    xin, emb, cm, pad = P.golden_emb2_inputs()
    for tag, use_emb in (("a", True), ("b", False)):
        sd = O.make_state_dict(seed=7, nclass=27, embedding_size=768 if use_emb else None, hidden=H)
        assert O.param_keys(sd) == list(G[tag + "_param_names"])
        keys = O.param_keys(sd)
        for k in keys:
            sd[k].requires_grad_(True)
        sp = [torch.from_numpy(s.astype(np.int64)) for s in G[tag + "_dropstep"]]
        ds = ((sp[0][:, 0], sp[0][:, 1]), (sp[1][:, 0], sp[1][:, 1])) if use_emb else (sp[0][:, 0], sp[0][:, 1])
        strong, weak = O.crnn_forward(sd, xin, training=True, embeddings=emb if use_emb else None, classes_mask=cm, pad_mask=pad, dropstep=ds)
        assert np.abs(strong.detach().numpy() - G[tag + "_strong"]).max() < 1e-6
        assert np.abs(weak.detach().numpy() - G[tag + "_weak"]).max() < 1e-6
        tgt_s = (O.lcg_fill(tuple(strong.shape), 31, 0.5, 0.5) < 0.2).float()
        tgt_w = (O.lcg_fill(tuple(weak.shape), 32, 0.5, 0.5) < 0.3).float()
        loss = torch.nn.functional.binary_cross_entropy(strong, tgt_s) + torch.nn.functional.binary_cross_entropy(weak, tgt_w)
        assert abs(loss.item() - G[tag + "_loss"][0]) < 1e-5
        grads = torch.autograd.grad(loss, [sd[k] for k in keys])
        np.testing.assert_allclose(np.array([g.norm().item() for g in grads]), G[tag + "_grad_norms"], rtol=2e-3, atol=1e-7)


# ------------------------------------------------------------------------------------------------
# 4. the step
# ------------------------------------------------------------------------------------------------
def build_task_2024(dev, bs=(2, 1, 1, 2, 2), nclass=27, dropout=0.5, dropstep=0.3, seed=7):
    """tests/parity_cases.py::build_task_2024 with n_RNN_cell = 256 (that function hard-codes 192)."""
    from desed_task_amd.arena import FusedAdam
    from desed_task_amd.nnet.CRNN import CRNN
    from desed_task_amd.sed_trainer_pretrained_2024 import SEDTask4
    from desed_task_amd.utils.schedulers import ExponentialWarmup
    config = P.recipe_config(bs)
    config["training"].update(mixup_prob=0.5, epoch_decay=100)
    config["net"] = dict(net_config_2024(), dropout=dropout, dropstep_recurrent=dropstep)
    if dropout > 0:
        config["net"].update(specaugm_t_p=0.2, specaugm_f_p=0.2)
    config["pretrained"] = {"e2e": False, "freezed": True, "model": "beats"}
    sd = O.make_state_dict(seed=seed, nclass=nclass, embedding_size=768, hidden=H)
    student = CRNN(**config["net"])
    student.load_state_dict({k: v.clone() for k, v in sd.items()})
    student = student.to(dev) if dev != "cpu" else student
    opt = FusedAdam(student.parameters(), lr=1e-3, betas=(0.9, 0.999), arena=student)
    sched = {"scheduler": ExponentialWarmup(opt, 1e-3, 5), "interval": "step"}

    class Enc:
        labels = list(range(nclass))
    task = SEDTask4(config, Enc(), student, None, opt=opt, scheduler=sched)
    task.whole_step = False
    task.train()
    if dev != "cpu":
        task.to(dev)
    return task


def batches_2024(dev, steps, bs=(2, 1, 1, 2, 2), nclass=27, n_samp=16000 + 1024, te=31):
    B = sum(bs)
    n_out = (1 + n_samp // 256) // 4
    ns = bs[0] + bs[1] + bs[2]
    batches = []
    for i in range(steps):
        audio = O.synth_audio(B, n_samp, seed=700 + 13 * i)
        labels = (O.lcg_fill((B, nclass, n_out), 50 + i, 0.5, 0.5) < 0.1).float()
        labels[ns:ns + bs[3], :, 1:] = 0.0
        labels[ns + bs[3]:] = 0.0
        emb = O.lcg_fill((B, 768, te), 90 + i, 1.0)
        valid = torch.zeros(B, nclass, dtype=torch.bool)
        valid[:bs[0], 10:] = True
        valid[bs[0]:, :10] = True
        batches.append(tuple(to(dev, t) for t in (audio, labels, emb, valid)))
    return batches


def case_step_2024_three_drivers(dev, graph, steps=5, repeat_plain=False):
    """The 2024 five-data-set step at n_RNN_cell = 256, dropout + SpecAugment + dropstep + mixup on, `steps` steps: StepDriver ==
    StepDriver(prefetch="teacher") and (graph=True) GraphedStepDriver == GraphedStepDriver(prefetch="teacher") through warm-up,
    capture, replays and the eager fall-back at the end -- losses, student arena and teacher arena equal bit for bit, the two pairs
    tests/parity_cases.py::case_prefetch_2024_equals_unpipelined compares at 192.  repeat_plain: the plain eager run twice.
    (The eager and the captured step agree bit for bit only when every step is re-seeded -- the captured step takes its per-step
    seeds from device memory: case_step_eager_equals_graph below, the protocol of parity_cases.case_step_bit_reproducible.)"""
    from desed_task_amd import graph as G_
    from desed_task_amd import ops as _ops
    from desed_task_amd.launcher import StepDriver
    bs = (2, 1, 1, 2, 2)
    batches = batches_2024(dev, steps, bs)
    originals = [(b[1].clone(), b[2].clone()) for b in batches]
    modes = ["plain"] + (["plain"] if repeat_plain else []) + ["pipelined"] + (["graph plain", "graph pipelined"] if graph else [])
    results = []
    for mode in modes:
        task = build_task_2024(dev, bs)
        assert task.sed_student.rnn.rnn.hidden_size == H
        pf = "teacher" if mode.endswith("pipelined") else None
        if mode.startswith("graph"):
            driver = G_.GraphedStepDriver(task, world_size=1, warmup=1, prefetch=pf)
        else:
            driver = StepDriver(task, world_size=1, prefetch=pf)
        random.seed(41); np.random.seed(101); torch.manual_seed(101)
        if dev != "cpu":
            torch.cuda.manual_seed(101)
        _ops.reseed_dropout()
        losses = []
        for step in range(steps):
            a, l, e, v = batches[step]
            if pf is None:
                loss = driver.run_step((a, l.clone(), None, e.clone(), v), step)      # (the plain step mixes its batch in place)
            else:
                nxt = (batches[step + 1][0], batches[step + 1][1], None, batches[step + 1][2], batches[step + 1][3]) if step + 1 < steps else None
                loss = driver.run_step((a, l, None, e, v), step, next_batch=nxt)
            losses.append(float(loss.detach()))
        if dev != "cpu":
            torch.cuda.synchronize()
        if pf is not None:
            for b, (lo, eo) in zip(batches[1:], originals[1:]):
                assert torch.equal(b[1], lo) and torch.equal(b[2], eo), "an announced tensor was modified in place"
        if mode == "graph pipelined":
            assert driver.graph is not None and driver.eager_fallbacks == 1
        assert all(np.isfinite(losses)), losses
        results.append((mode, losses, task.sed_student.arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone()))
    first = {}
    for mode, l1, s1, t1 in results:
        _, l0, s0, t0 = first.setdefault(mode.startswith("graph"), (mode, l1, s1, t1))
        assert l0 == l1, (mode, l0, l1)
        assert torch.equal(s0, s1) and torch.equal(t0, t1), mode
    return results[0][1]


def case_step_2024_eager_equals_graph(dev, steps=4):
    """The same 2024 step, every step re-seeded (the protocol of parity_cases.case_step_bit_reproducible): StepDriver and
    GraphedStepDriver (eager warm-up, capture, replays) leave the same losses and the same student / teacher bits."""
    from desed_task_amd import graph as G_
    from desed_task_amd import ops
    from desed_task_amd.launcher import StepDriver
    bs = (2, 1, 1, 2, 2)
    batches = batches_2024(dev, steps, bs)
    finals = []
    for mode in ("eager", "graph"):
        task = build_task_2024(dev, bs)
        driver = StepDriver(task, world_size=1) if mode == "eager" else G_.GraphedStepDriver(task, world_size=1, warmup=1)
        losses = []
        for step in range(steps):
            random.seed(40 + step); np.random.seed(100 + step); torch.manual_seed(100 + step); torch.cuda.manual_seed(100 + step)
            ops.reseed_dropout()
            a, l, e, v = batches[step]
            losses.append(float(driver.run_step((a, l.clone(), None, e.clone(), v), step).detach()))
        torch.cuda.synchronize()
        if mode == "graph":
            assert driver.graph is not None
        finals.append((losses, task.sed_student.arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone()))
    assert finals[0][0] == finals[1][0], (finals[0][0], finals[1][0])
    assert torch.equal(finals[0][1], finals[1][1]) and torch.equal(finals[0][2], finals[1][2])


def build_task_2023(dev, bs, sd, dropout=0.0, specaug=False, rampup=100):
    """tests/parity_cases.py::build_task (2023 recipe: 10 classes, no embeddings, two GRU layers) with n_RNN_cell = 256."""
    from desed_task_amd.arena import FusedAdam
    from desed_task_amd.nnet.CRNN import CRNN
    from desed_task_amd.sed_trainer import SEDTask4
    from desed_task_amd.utils.schedulers import ExponentialWarmup
    config = P.recipe_config(bs)
    config["net"] = dict(config["net"], n_RNN_cell=H, dropout=dropout)
    student = CRNN(**config["net"], **({} if specaug else {"specaugm_t_p": 0.0, "specaugm_f_p": 0.0}))
    student.load_state_dict({k: v.clone() for k, v in sd.items()})
    student = student.to(dev) if dev != "cpu" else student
    opt = FusedAdam(student.parameters(), lr=1e-3, betas=(0.9, 0.999), arena=student.arena)
    sched = {"scheduler": ExponentialWarmup(opt, 1e-3, rampup), "interval": "step"}

    class Enc:
        labels = list(range(10))
    task = SEDTask4(config, Enc(), student, opt=opt, scheduler=sched)
    task.whole_step = False
    task.train()
    if dev != "cpu":
        task.to(dev)
        opt.arena = task.sed_student.arena      # .to() rebuilt the arenas
    return task


def case_step_eager_equals_graph(dev, steps=3, n_samp=16000 + 1024):
    """tests/parity_cases.py::case_step_bit_reproducible at n_RNN_cell = 256 (two GRU layers, dropout + SpecAugment + mixup on, every
    step re-seeded): two eager runs and the hipGraph driver (eager warm-up, capture, replay) leave the SAME BITS -- loss, student,
    teacher, gradient.  The replayed launches of the streamed-weight recurrences are the eager ones."""
    from desed_task_amd import graph as G_
    from desed_task_amd import ops
    from desed_task_amd.launcher import StepDriver
    bs = (1, 1, 2)
    sd = O.make_state_dict(seed=7, hidden=H)
    audio = to(dev, O.synth_audio(sum(bs), n_samp, seed=77))
    labels = to(dev, O.synth_labels(bs, 10, (1 + n_samp // 256) // 4, seed=5))
    finals = []
    for mode in ("eager", "eager", "graph"):
        task = build_task_2023(dev, bs, sd, dropout=0.5, specaug=True, rampup=5)
        driver = StepDriver(task, world_size=1) if mode == "eager" else G_.GraphedStepDriver(task, world_size=1, warmup=1)
        for step in range(steps):
            random.seed(40 + step); np.random.seed(100 + step); torch.manual_seed(100 + step)
            ops.reseed_dropout()
            loss = driver.run_step((audio, labels.clone(), None, None), step)
        torch.cuda.synchronize()
        if mode == "graph":
            assert driver.graph is not None
        finals.append((float(loss.detach()), task.sed_student.arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone(),
                       task.sed_student.arena.flat_grad.detach().cpu().clone()))
    for name, other in (("second eager run", finals[1]), ("hipGraph replay", finals[2])):
        assert finals[0][0] == other[0], (name, finals[0][0], other[0])
        for what, a, b_ in zip(("student", "teacher", "gradient"), finals[0][1:], other[1:]):
            assert torch.equal(a, b_), "%s: %s differs (max %.3e, %d elements)" % (name, what, (a - b_).abs().max().item(), int((a != b_).sum()))


def case_training_step_2023_vs_oracle(dev, bs=(1, 1, 2), n_samp=16000 + 1024, steps=2):
    """A 2023-style task (10 classes, no embeddings, TWO GRU layers: layer 1 at I = 512) at n_RNN_cell = 256 against
    oracle.OracleTrainer over two optimisation steps, at the tolerances of tests/parity_cases.py::case_training_step (its oracle
    comparison at 128): gradients elementwise (1e-4 of the tensor's maximum at step 0, 3e-2 later; medians 1e-5 / 2e-3), the logged
    scalars 2e-5 + 2e-4, posteriors 1e-3, parameters as update vectors."""
    from desed_task_amd.launcher import StepDriver
    B = sum(bs)
    sd = O.make_state_dict(seed=7, hidden=H)
    keys = O.param_keys(sd)
    assert "rnn.rnn.weight_ih_l1" in keys and tuple(sd["rnn.rnn.weight_ih_l1"].shape) == (3 * H, 2 * H)
    audio = O.synth_audio(B, n_samp, seed=77)
    n_out = (1 + n_samp // 256) // 4
    labels = O.synth_labels(bs, 10, n_out, seed=5)
    task = build_task_2023(dev, bs, sd)
    driver = StepDriver(task, world_size=1)
    orc = O.OracleTrainer(sd, batch_sizes=bs, lr=1e-3, rampup_len=100)
    for step in range(steps):
        random.seed(4); np.random.seed(100 + step); torch.manual_seed(100 + step)
        assert random.random() < 0.5
        cw = np.random.beta(0.2, 0.2); pw = torch.randperm(bs[1]); cs = np.random.beta(0.2, 0.2); ps = torch.randperm(bs[0])
        mix = dict(c_weak=cw, perm_weak=pw, c_strong=cs, perm_strong=ps)
        random.seed(4); np.random.seed(100 + step); torch.manual_seed(100 + step)
        loss = driver.run_step((to(dev, audio.clone()), to(dev, labels.clone()), None, None), step)
        tot, logs = orc.training_step(audio, labels, mix=mix)
        ref_grads = orc.optimizer_step(tot)
        hip_params = dict(task.sed_student.named_parameters())
        for k in keys:
            if k.startswith("cnn.cnn.conv") and k.endswith(".bias"):
                continue                                   # analytically zero under train-mode BatchNorm
            g, r = hip_params[k].grad.detach().cpu(), ref_grads[k]
            rel = 1e-4 if step == 0 else 3e-2
            assert (g - r).abs().max().item() <= rel * r.abs().max().item() + 5e-8, "step %d grad %s" % (step, k)
            _, emed = P.grad_error_stats(g, r)
            assert emed <= (1e-5 if step == 0 else 2e-3), "step %d grad %s: median error %.3e" % (step, k, emed)
        got = {k: (float(v) if not torch.is_tensor(v) else float(v.detach().cpu())) for k, v in task.logged.items()}
        got["loss"] = float(loss.detach().cpu())
        logs["loss"] = tot.item()
        for k in sorted(logs):
            a, b = got[k], logs[k]
            assert abs(a - b) <= 2e-5 + 2e-4 * abs(b), "step %d %s: hip %.8g oracle %.8g" % (step, k, a, b)
        s_s, w_s, s_t, w_t = [t.detach().cpu() for t in task.last_outputs]
        assert (s_s - orc.last["strong_s"]).abs().max().item() < 1e-3
        assert (w_s - orc.last["weak_s"]).abs().max().item() < 1e-3
        assert (s_t - orc.last["strong_t"]).abs().max().item() < 1e-3
        assert (w_t - orc.last["weak_t"]).abs().max().item() < 1e-3
    st = dict(task.sed_student.named_parameters())
    tt = dict(task.sed_teacher.named_parameters())
    for k in keys:
        if k.startswith("cnn.cnn.conv") and k.endswith(".bias"):
            continue
        if ref_grads[k].abs().max().item() < 1e-4:
            continue        # gradient at rounding-noise level relative to Adam's normalisation
        for mine, theirs, what in ((st[k].detach().cpu(), orc.student[k].detach(), "student"),
                                   (tt[k].detach().cpu(), orc.teacher[k], "teacher")):
            upd = (theirs - sd[k].detach()).norm().item()
            err = (mine - theirs).norm().item()
            assert err <= 0.15 * upd + 1e-6, "%s %s: |err| %.3e vs |update| %.3e" % (what, k, err, upd)
            med_err = (mine - theirs).abs().median().item()
            med_upd = (theirs - sd[k].detach()).abs().median().item()
            assert med_err <= 0.01 * med_upd + 1e-8, "%s %s: median |err| %.3e vs median |update| %.3e" % (what, k, med_err, med_upd)


# ------------------------------------------------------------------------------------------------
# 5. refusals stay refusals
# ------------------------------------------------------------------------------------------------
def case_refusals(dev):
    from desed_task_amd import _lib
    from desed_task_amd.nnet.CRNN import CRNN
    with wide_recurrence(False):                                 # the default: 256 is refused as it always was, and says how to opt in
        try:
            CRNN(**dict(P.recipe_config()["net"], n_RNN_cell=H))
            raise AssertionError("n_RNN_cell = 256 must be refused without the switch")
        except NotImplementedError as e:
            assert "SED_GRU_WIDE" in str(e), str(e)
    with wide_recurrence(True):
        assert CRNN(**dict(P.recipe_config()["net"], n_RNN_cell=H)).rnn.rnn.hidden_size == H
    for n in (64, 320):
        try:
            CRNN(**dict(P.recipe_config()["net"], n_RNN_cell=n))
            raise AssertionError("n_RNN_cell = %d must be refused" % n)
        except NotImplementedError as e:
            assert all(w in str(e) for w in ("128", "192", "256")), str(e)
    dll = _lib.get()._dll                                       # (lib.call raises on a non-zero return code)
    st = 0 if dev == "cpu" else torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 12, device=dev, dtype=torch.float32)
    p = buf.data_ptr()
    assert dll.sed_gru_fwd(p, p, p, p, p, p, p, 1, 2, 320, st) == -3
    assert dll.sed_head_fwd(p, p, p, p, p, p, p, p, p, 1, 2, 640, 10, 0, 0, 1.0, None, None, None, st) == -3
    assert float(buf.abs().max()) == 0.0
