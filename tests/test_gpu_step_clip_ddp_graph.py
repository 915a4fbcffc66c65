"""GPU: the clipped whole step with the gradient exchange CAPTURED (SED_DDP_GRAPH_EXCHANGE=1), rehearsed on a one-rank RCCL group
(pattern of test_gpu_ddp_graph.py): all-reduce, the norm launch and the clipped Adam launch are nodes of the one graph behind
SEDTask4.training_step, and the sums over one rank change no bit -- so it must equal the plain clipped whole step exactly."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    for k in ("SED_DIST_BACKEND", "SED_DDP_OVERLAP", "SED_DDP_REHEARSE", "SED_DDP_GRAPH_EXCHANGE"):
        os.environ.pop(k, None)
    from tests import clip_cases as C
    from desed_task_amd import graph as G
    from desed_task_amd.launcher import init_distributed
    seen = []
    orig = G.GraphedStepDriver.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        seen.append((self.eager.exchange, self.capture_exchange, self.eager.clip))

    G.GraphedStepDriver.__init__ = spy
    clip = C.ACTIVE[False]
    plain = C._surface_run("cuda", "whole", clip, epochs=2, per_epoch=3)
    assert seen == [(False, False, clip)], seen
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      SED_DDP_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", SED_DDP_GRAPH_EXCHANGE="1")
    init_distributed()
    assert dist.is_initialized() and dist.get_backend() == "nccl"
    captured = C._surface_run("cuda", "whole", clip, epochs=2, per_epoch=3)
    assert seen[1:] == [(True, True, clip)], seen
    C._same(captured, plain, "exchange captured vs the plain clipped whole step")
    assert len(plain["clips"]) == 6
    for a, b in zip(captured["clips"], plain["clips"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a[1]) < 1.0, (a, b)
    torch.cuda.synchronize()
    open(os.path.join(out_dir, "clip_rehearsal_ok"), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_clipped_whole_step_with_the_exchange_captured_rccl_rehearsal(tmp_path):
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    assert os.path.exists(os.path.join(str(tmp_path), "clip_rehearsal_ok"))
