"""Gradient-norm clipping on the data-parallel path, CPU: world_size 2, gloo, kernels through the fiber emulator (pattern of
test_ddp_gloo.py).  The clip sits behind the exchange: its norm is that of the MEAN gradient over the ranks (the 1 / world factor that
Adam folds in), so both ranks form the same coefficient and stay bit-identical."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import random
    from tests.emu_support import bind_emulator
    bind_emulator()
    from oracle import sed_oracle as O
    from tests import parity_cases as P
    from desed_task_amd.launcher import StepDriver, init_distributed
    r, _, w = init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    bs, n_samp = (1, 1, 1), 8192 + 1024
    sd = O.make_state_dict(seed=7)
    audio = O.synth_audio(3, n_samp, seed=100 + rank)           # different clips per rank
    labels = O.synth_labels(bs, 10, (1 + n_samp // 256) // 4, seed=5 + rank)

    def seed():
        random.seed(4); np.random.seed(7); torch.manual_seed(7)

    def mean_norm64(local):
        both = [torch.zeros_like(local) for _ in range(world)]
        dist.all_gather(both, local)
        return math.sqrt(float((((both[0].double() + both[1].double()) / world) ** 2).sum())), both

    # a first pass without the driver: the size of the mean gradient, to place the threshold where the branch is certain
    seed()
    task = P.build_task("cpu", bs, sd, dropout=0.0, specaug=False, rampup=100)
    loss = task.training_step((audio.clone(), labels.clone(), None, None), 0)
    task.opt.zero_grad(set_to_none=True)
    loss.backward()
    estimate, _ = mean_norm64(task.sed_student.arena.gather_grads().clone())
    clip = round(0.5 * estimate, 6)

    def run(overlap, record):
        seed()
        t = P.build_task("cpu", bs, sd, dropout=0.0, specaug=False, rampup=100)
        t.hparams["training"]["gradient_clip"] = clip
        d = StepDriver(t, world_size=world, overlap_allreduce=overlap)
        assert d.clip == clip and t.opt.max_grad_norm == clip and t.opt.grad_scale == 1.0 / world
        local = []
        if record:                                   # the rank's own gradient, as the step produced it, BEFORE the exchange
            orig = d.allreduce_grads

            def spy():
                local.append(t.sed_student.arena.gather_grads().clone())
                orig()
            d.allreduce_grads = spy
        d.run_step((audio.clone(), labels.clone(), None, None), 0)
        st = t.opt._flat_state
        return dict(flat=t.sed_student.arena.flat.clone(), m=st["m"].clone(), v=st["v"].clone(), clip=t.opt.last_clip.clone(),
                    log=list(d.bucket_log), local=local[0] if local else None, numel=t.sed_student.arena.numel)

    blocking = run(False, True)
    assert blocking["log"] == [("AB", 0, blocking["numel"])]
    norm64, locals_ = mean_norm64(blocking["local"])
    bucketed = run(None, False)
    assert [tag for tag, _, _ in bucketed["log"]] == ["A", "B"]
    for k in ("flat", "m", "v", "clip"):
        assert torch.equal(blocking[k], bucketed[k]), "overlap on / off differ in " + k
    # an unclipped step from the same state, for the size of the effect
    seed()
    t0 = P.build_task("cpu", bs, sd, dropout=0.0, specaug=False, rampup=100)
    StepDriver(t0, world_size=world, overlap_allreduce=False).run_step((audio.clone(), labels.clone(), None, None), 0)
    gathered = {}
    for k in ("flat", "m", "v", "clip"):
        both = [torch.zeros_like(blocking[k]) for _ in range(world)]
        dist.all_gather(both, blocking[k])
        gathered[k] = both
    if rank == 0:
        torch.save(dict(gathered=gathered, norm64=norm64, clip=clip, numel=blocking["numel"], locals=locals_,
                        m_unclipped=t0.opt._flat_state["m"].clone()), os.path.join(out_dir, "r0.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_rank_clip_of_the_mean_gradient(tmp_path):
    """Both ranks end with identical arenas and moments; last_clip[0] is the float64 norm of the MEAN of the two ranks' local gradients
    (recorded inside the step, before the exchange) within clip_cases' bound for `total` (2 ((d + 1) / 2 + 1) u, + 1 u for the sum of
    the two ranks that the exchange rounds); the coefficient clips (threshold = half the norm) within 2 e_coef; the blocking and the
    bucketed exchange give equal bits (asserted in the workers); exp_avg is coef x the unclipped step's."""
    from tests import clip_cases as C
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    d = torch.load(os.path.join(str(tmp_path), "r0.pt"))
    g0, g1 = d["locals"]
    assert (g0 - g1).abs().max() > 1e-6                                    # ranks really saw different data
    for k in ("flat", "m", "v", "clip"):
        assert torch.equal(d["gathered"][k][0], d["gathered"][k][1]), k    # bit-identical across ranks
    total, coef = [float(x) for x in d["gathered"]["clip"][0]]
    n, norm64, clip = d["numel"], d["norm64"], d["clip"]
    print("two ranks: norm %.9g (float64 %.9g), coef %.9g, threshold %g" % (total, norm64, coef, clip))
    assert abs(total - norm64) <= 2 * ((C.depth(n) + 1) / 2 + 2) * C.U24 * norm64, (total, norm64)
    coef64 = C.f32(clip) / (norm64 + C.f32(1e-6))
    assert coef < 1.0 and abs(coef - coef64) <= 2 * (C.e_coef(n) + C.U24) * coef64, (coef, coef64)
    # exp_avg after one step is (1 - b1) g coef: linear in the coefficient
    m, m_u = d["gathered"]["m"][0].double(), d["m_unclipped"].double()
    assert ((m - coef64 * m_u).abs() <= 2 * (6 * C.U24 + C.e_coef(n)) * m_u.abs() + 1e-300).all()
    assert float(m_u.abs().max()) > 0
