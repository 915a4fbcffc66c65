"""`pretrained.e2e: True`: the 2023 `pretrained` training step with the frozen BEATs extractor inside it, at the recipe's sizes
(recipes/dcase2023_task4_baseline/confs/pretrained.yaml: batch [12, 12, 24] = 48 clips of 10 s, 768 x 496 frame embeddings,
iter3 extractor with 12 layers), random weights, synthetic audio.  Secondary workload: not the headline metric of bench.py.
    python tools/bench_e2e.py [--rounds 5] [--steps 10] [--layers 12]
One JSON line per mode and extractor precision ("bf16x3", "bf16"):
  (a)  e2e_step        the captured e2e whole step (pipelined front half; the extractor serially at the head of the step)
  (b)  resident_step   the existing captured step on embeddings that are resident in HBM (no extractor at all)
  (c)  extractor       BEATsModel.embeddings(audio, "frame") alone
  (d)  hand_chain      extractor(audio)["frame"], then (b)'s step on it: what a user could already run by hand; both ends synchronised
The modes alternate inside one process, `--rounds` rounds of `--steps` steps each; ms_per_step is the median over the rounds and
`spread_ms` their max - min."""
import json, os, random, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from desed_task_amd import build as _build
from desed_task_amd.arena import FusedAdam
from desed_task_amd.beats import BEATsModel
from desed_task_amd.graph import GraphedStepDriver
from desed_task_amd.nnet.CRNN import CRNN
from desed_task_amd.sed_trainer_pretrained import SEDTask4
from desed_task_amd.utils.schedulers import ExponentialWarmup
from bench import recipe_config


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, STEPS, LAYERS = arg("--rounds", 5), arg("--steps", 10), arg("--layers", 12)
BS = (12, 12, 24)
B = sum(BS)
CFG = dict(input_patch_size=16, embed_dim=512, conv_bias=False, encoder_layers=LAYERS, encoder_embed_dim=768, encoder_ffn_embed_dim=3072,
           encoder_attention_heads=12, activation_fn="gelu", layer_norm_first=False, deep_norm=True, conv_pos=128, conv_pos_groups=16,
           relative_position_embedding=True, num_buckets=320, max_distance=800, gru_rel_pos=True, dropout=0.0, attention_dropout=0.0,
           encoder_layerdrop=0.0)
dev = torch.device("cuda", 0)
torch.manual_seed(1); np.random.seed(1); random.seed(1)
g = torch.Generator(device=dev).manual_seed(5)
audio = 0.1 * torch.randn(B, 160000, device=dev, generator=g)
labels = (torch.rand(B, 10, 156, device=dev, generator=g) < 0.1).float()
labels[BS[0]:BS[0] + BS[1], :, 1:] = 0.0
labels[BS[0] + BS[1]:] = 0.0


class Enc:
    labels = list(range(10))


def make_task(e2e, extractor):
    config = recipe_config()
    config["training"].update(batch_size=list(BS))
    config["net"].update(use_embeddings=True, embedding_size=768, embedding_type="frame", aggregation_type="pool1d")
    config["pretrained"] = {"e2e": e2e, "freezed": True, "model": "beats"}
    student = CRNN(**config["net"]).to(dev)
    opt = FusedAdam(student.parameters(), lr=1e-3, betas=(0.9, 0.999), arena=student.arena)
    sched = {"scheduler": ExponentialWarmup(opt, 1e-3, 50 * 118), "interval": "step"}
    task = SEDTask4(config, Enc(), student, pretrained_model=extractor if e2e else None, opt=opt, scheduler=sched).to(dev)
    opt.arena = task.sed_student.arena
    task.train()
    return task


def make_modes(precision):
    torch.manual_seed(0)
    sd = None
    extractors = []
    for _ in range(2):              # one for the e2e task, one for the hand chain: same weights
        ex = BEATsModel(checkpoint={"cfg": dict(CFG), "model": sd} if sd is not None else _random_checkpoint(), precision=precision).to(dev)
        sd = sd if sd is not None else {k: v.detach().cpu() for k, v in ex.model.state_dict().items()}
        extractors.append(ex)
    t_a, t_b = make_task(True, extractors[0]), make_task(False, None)
    d_a, d_b = (GraphedStepDriver(t, world_size=1, warmup=3, prefetch="teacher") for t in (t_a, t_b))
    chain = extractors[1]
    emb = chain(audio)["frame"]
    state = {"emb": emb}

    def step_e2e(driver):
        return lambda i: driver.run_step((audio, labels, None), i, next_batch=(audio, labels, None))

    def step_b(i, emb_=None):
        # resident embeddings: once captured, the graph's own input buffer (a loader would write there): no staging copy
        e = emb_ if emb_ is not None else (d_b.input_buffers()[3] if d_b.graph is not None else state["emb"])
        return d_b.run_step((audio, labels, None, e), i, next_batch=(audio, labels, None, e))

    def step_c(i):
        return chain.embeddings(audio, "frame")

    def step_d(i):
        return step_b(i, chain(audio)["frame"])
    return {"e2e_step": step_e2e(d_a), "resident_step": step_b, "extractor": step_c, "hand_chain": step_d}, (d_a, d_b)


def _random_checkpoint():
    from desed_task_amd.beats import BEATs, BEATsConfig
    return {"cfg": dict(CFG), "model": BEATs(BEATsConfig(CFG)).state_dict()}


def timed(fn, i0, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i0 + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for precision in ("bf16x3", "bf16"):
    modes, drivers = make_modes(precision)
    for name, fn in modes.items():          # warm-up: the eager steps, the capture, a few replays
        for i in range(8):
            fn(i)
        torch.cuda.synchronize()
    n = 8
    times = {name: [] for name in modes}
    for r in range(ROUNDS):
        for name, fn in modes.items():
            times[name].append(timed(fn, n, STEPS))
        n += STEPS
    for name in modes:
        ts = times[name]
        print(json.dumps({"mode": name, "extractor_precision": precision, "layers": LAYERS, "clips": B,
                          "workload": "dcase2023 pretrained.yaml, batch 48 = [12,12,24] x 10 s, BEATs iter3 (%d layers) -> 768 x 496" % LAYERS,
                          "ms_per_step": round(statistics.median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3),
                          "rounds_ms": [round(t, 3) for t in ts], "steps_per_round": STEPS,
                          "clips_per_s": round(B / statistics.median(ts) * 1e3, 1),
                          "eager_fallbacks": [d.eager_fallbacks for d in drivers], "library_rev": _build.source_rev()}), flush=True)
    del modes, drivers
    torch.cuda.empty_cache()
