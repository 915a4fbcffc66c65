"""What in-kernel gradient clipping buys behind Lightning's hook order: the 2024 recipe's training step at the recipe's sizes
(tools/bench_2024.py's workload) with `training.gradient_clip` set, driven by the stand-in trainer loop (tests/lightning_order.Trainer:
Lightning 1.9's automatic-optimisation order, the optimizer a plain torch.optim.Adam that SEDTask4 adopts).

On a tree whose FusedAdam clips (max_grad_norm) the loop's gradient-clipping slot calls SEDTask4.configure_gradient_clipping and the
step runs in whole-step mode (captured, pipelined, clipped inside the fused Adam).  On a tree without it -- the script is written to run
there too, for the comparison -- `gradient_clip > 0` blocks whole-step mode, the hooks run one by one and the slot calls
torch.nn.utils.clip_grad_norm_ as Lightning would.    python tools/clip_surface_timing.py [--gradient-clip 5.0] [--steps 40]"""
import json, os, random, sys, time
sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from desed_task_amd.arena import FusedAdam
from desed_task_amd.lookahead import BatchList
from desed_task_amd.nnet.CRNN import CRNN
from desed_task_amd.sed_trainer_pretrained_2024 import SEDTask4
from desed_task_amd.utils.schedulers import ExponentialWarmup
from bench import recipe_config
from tests.lightning_order import Trainer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


CLIP, K, W = arg("--gradient-clip", 5.0), arg("--steps", 40), 10
BS, NCLASS = (12, 6, 6, 12, 24), 27
dev = torch.device("cuda", 0)
torch.manual_seed(1); np.random.seed(1); random.seed(1)
config = recipe_config()
config["training"].update(batch_size=list(BS), mixup="soft", mixup_prob=0.5, epoch_decay=100, const_max=2, gradient_clip=CLIP)
config["net"].update(dropout=0.5, rnn_layers=1, nclass=NCLASS, n_RNN_cell=192, dropstep_recurrent=0.3, dropstep_recurrent_len=16,
                     use_embeddings=True, embedding_size=768, embedding_type="frame", aggregation_type="pool1d")
config["pretrained"] = {"e2e": False, "freezed": True, "model": "beats"}
student = CRNN(**config["net"]).to(dev)
opt = torch.optim.Adam(student.parameters(), 1e-3, betas=(0.9, 0.999))
sched = {"scheduler": ExponentialWarmup(opt, 1e-3, 50 * 118), "interval": "step"}
B = sum(BS)
g = torch.Generator(device=dev).manual_seed(5)
audio = 0.1 * torch.randn(B, 160000, device=dev, generator=g)
labels = (torch.rand(B, NCLASS, 156, device=dev, generator=g) < 0.1).float()
ns = BS[0] + BS[1] + BS[2]
labels[ns:ns + BS[3], :, 1:] = 0.0
labels[ns + BS[3]:] = 0.0
emb = torch.randn(B, 768, 496, device=dev, generator=g)
valid = torch.zeros(B, NCLASS, dtype=torch.bool, device=dev)
valid[:BS[0], 10:] = True
valid[BS[0]:, :10] = True


class Clips(BatchList):         # a loader hands out fresh tensors: the step mixes labels and embeddings in place
    def __getitem__(self, i):
        return (audio, labels.clone(), [1.0] * B, emb.clone(), valid)


class Enc:
    labels = list(range(NCLASS))


task = SEDTask4(config, Enc(), student, None, opt=opt, scheduler=sched, train_data=Clips([None] * (W + K))).to(dev)
task.train()
fused = hasattr(FusedAdam, "max_grad_norm")
if CLIP > 0:
    if fused:
        task.on_before_optimizer_step = lambda o, idx: task.configure_gradient_clipping(o, idx, CLIP, "norm")
    else:
        params = list(task.sed_student.parameters())
        task.on_before_optimizer_step = lambda o, idx: torch.nn.utils.clip_grad_norm_(params, CLIP)
marks = {}


def on_step(tr, model, i):
    if i == W - 1:
        torch.cuda.synchronize()
        marks["t0"] = time.perf_counter()


tr = Trainer(max_epochs=1, on_step=on_step)
tr.fit(task)
torch.cuda.synchronize()
dt = (time.perf_counter() - marks["t0"]) / K
drv = getattr(task, "_driver", None)
lc = getattr(task.opt, "last_clip", None)
print(json.dumps({"workload": "dcase2024 pretrained.yaml step, batch 60, behind the Lightning-order trainer loop", "gradient_clip": CLIP,
                  "path": ("whole step (captured)" if getattr(drv, "graph", None) is not None else "whole step (eager)") if drv is not None
                  else "hook by hook", "clipping": ("fused (sed_grad_sqnorm + sed_adam_step_clipped)" if fused else "torch.nn.utils.clip_grad_norm_") if CLIP > 0 else "off",
                  "last_clip": [float(x) for x in lc.cpu()] if lc is not None else None,
                  "ms_per_step": round(dt * 1e3, 3), "clips_per_s": round(B / dt, 1), "steps": K, "loss": round(float(tr.losses[-1]), 5)}))
