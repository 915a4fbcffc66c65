"""What the DATA PATH costs the 2023 training step (B = 48 clips of 10 s, confs/default.yaml), through the Lightning-order loop
(tests/lightning_order.Trainer over train_dataloader(), whole-step mode: the captured step), in ONE process:
  (a)  ready_batches     ready device batches handed out from the captured step's own input buffers (lookahead.BatchList): bench.py's
                         `--surface lightning` figure.  Measured twice per round (first and last), as the yardstick and its spread
  (b)  resident_set      resident.ResidentTrainSet over a synthetic 2 000-clip int16 pool: one gather launch per batch
  (c)  dataloader        the same clips behind a map-style data set and the DataLoader SEDTask4 builds for it, with the recipe's
                         num_workers = 6: what a run has today, minus the wav decoding (the clips sit decoded in host memory)
plus, by HIP events, the gather launch alone and the step driver's copy of an announced batch into the captured step's static inputs
(mode (a) hands out those buffers themselves, so only (b) and (c) pay that copy), and the host time of one resident item.
    python tools/bench_resident.py [--rounds 5] [--steps 32] [--clips 2000] [--workers 6]
One JSON line per mode, then one summary line with the check  (b) - (a) <= gather + 2 * |a1 - a2|  ("the loader adds its kernel and
nothing else on the host").  Every mode runs one epoch of 8 + steps + 1 batches per round; the `steps` timed ones follow the 8 that
re-prime the pipeline after the previous epoch's end, and the epoch's last batch (no successor: the eager fall-back) lies behind them.
ms_per_step is the median over the rounds.  `--rehearse`: tiny sizes on the CPU emulator, to check the plumbing -- not a measurement."""
import json, os, random, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from desed_task_amd import _lib, build as _build
from desed_task_amd import resident as R
from desed_task_amd.lookahead import BatchList


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REHEARSE = "--rehearse" in sys.argv
ROUNDS, STEPS, CLIPS, WORKERS = arg("--rounds", 5), arg("--steps", 32), arg("--clips", 2000), arg("--workers", 6)
SKIP = 8
if REHEARSE:
    from tests.emu_support import bind_emulator
    bind_emulator()
    bench.BATCH, bench.N_SAMPLES = (1, 1, 2), 2048 + 1024
    bench.N_FRAMES_OUT = (1 + bench.N_SAMPLES // 256) // 4
    ROUNDS, STEPS, CLIPS, WORKERS, SKIP = 1, 2, 16 * (4 + 2 + 1), 2, 4
    dev = torch.device("cpu")
elif not torch.cuda.is_available():
    raise SystemExit("tools/bench_resident.py needs the MI355X (no GPU visible); --rehearse checks the plumbing on the CPU emulator")
else:
    dev = torch.device("cuda", 0)
from tests.lightning_order import Trainer          # noqa: E402
from tests.resident_cases import GroupedBatches    # noqa: E402  (the stand-in for the recipe's concat batch sampler)

BS = bench.BATCH
B, L, T = sum(BS), bench.N_SAMPLES, bench.N_FRAMES_OUT
EPOCH = SKIP + STEPS + 1
if min((CLIPS // 4) // BS[0], (CLIPS // 4) // BS[1], (CLIPS // 2) // BS[2]) < EPOCH:
    raise SystemExit("--clips %d gives fewer than the %d batches of an epoch" % (CLIPS, EPOCH))


def sync():
    if dev.type == "cuda":
        torch.cuda.synchronize()


class Clips(torch.utils.data.Dataset):
    """`n` decoded 16-bit clips in host memory with the reference's item contract [audio, labels (C, T), [ratio]]."""

    def __init__(self, n, role, seed):
        rng = np.random.RandomState(seed)
        self.pcm = torch.from_numpy(rng.randint(-3277, 3277, size=(n, L)).astype(np.int16))
        g = torch.Generator().manual_seed(seed)
        self.labels = torch.zeros(n, 10, T, dtype=torch.uint8)
        if role == "strong":
            self.labels[:] = torch.rand(n, 10, T, generator=g) < 0.1
        elif role == "weak":
            self.labels[:, :, 0] = torch.rand(n, 10, generator=g) < 0.2

    def __len__(self):
        return self.pcm.shape[0]

    def __getitem__(self, i):
        return [self.pcm[i].float() / 32768.0, self.labels[i].float(), [1.0]]


def make_task(num_workers=0):
    from desed_task_amd.nnet.CRNN import CRNN
    from desed_task_amd.sed_trainer import SEDTask4
    from desed_task_amd.utils.schedulers import ExponentialWarmup
    config = bench.recipe_config()
    config["training"]["num_workers"] = num_workers
    torch.manual_seed(1234)
    student = CRNN(**config["net"]).to(dev)
    opt = torch.optim.Adam(student.parameters(), 1e-3, betas=(0.9, 0.999))
    sched = {"scheduler": ExponentialWarmup(opt, 1e-3, 50 * 118), "interval": "step"}

    class Enc:
        labels = list(range(10))
    task = SEDTask4(config, Enc(), student, opt=opt, scheduler=sched).to(dev)
    opt.arena = task.sed_student.arena
    task.whole_step, task.whole_step_warmup = True, 3
    task.train()
    return task


def epoch(task):
    """One epoch of the Lightning-order loop -> ms per step over steps SKIP .. SKIP + STEPS - 1 (both ends synchronised)."""
    marks = {}

    def on_step(tr, model, i):
        if i + 1 == SKIP:
            sync()
            marks["t0"] = time.perf_counter()
        elif i + 1 == SKIP + STEPS:
            sync()
            marks["t1"] = time.perf_counter()
    tr = Trainer(max_epochs=1, limit_train_batches=EPOCH, on_step=on_step).fit(task)
    sync()
    assert tr.global_step == EPOCH, (tr.global_step, EPOCH)
    return (marks["t1"] - marks["t0"]) / STEPS * 1e3


torch.manual_seed(1); np.random.seed(1); random.seed(1)
parts = [Clips(CLIPS // 4, "strong", 11), Clips(CLIPS // 4, "weak", 12), Clips(CLIPS // 2, "unlabeled", 13)]
data = torch.utils.data.ConcatDataset(parts)


def sampler():
    return GroupedBatches([torch.utils.data.RandomSampler(p) for p in parts], BS)


# (a): bench.py's ready batches -- after the capture the clips live in the captured step's own input buffers
audio, labels = bench.synthetic_batch(dev, 1234)
task_a = make_task()
ready = {"audio": audio, "labels": None}


class Ready(BatchList):
    def __getitem__(self, i):
        return (ready["audio"], labels.clone() if ready["labels"] is None else ready["labels"], [1.0] * B)


task_a.train_data = Ready([None] * EPOCH)
epoch(task_a)
drv = task_a._driver
if getattr(drv, "graph", None) is not None:
    ready["audio"] = drv.next_audio_buffer()
    ready["audio"].copy_(audio)
    ready["labels"] = drv.next_label_buffer()
    if ready["labels"] is not None:
        ready["labels"].copy_(labels)

# (b): the resident set
t0 = time.perf_counter()
pool = R.ResidentPool.from_dataset(data, dev, num_workers=0)
sync()
pool_s = time.perf_counter() - t0
task_b = make_task()
task_b.train_data = R.ResidentTrainSet(pool, sampler())
epoch(task_b)

# (c): the DataLoader of today
task_c = make_task(num_workers=WORKERS)
task_c.train_data, task_c.train_sampler = data, sampler()
epoch(task_c)

modes = [("ready_batches_1", task_a), ("resident_set", task_b), ("dataloader", task_c), ("ready_batches_2", task_a)]
times = {name: [] for name, _ in modes}
for r in range(ROUNDS):
    for name, task in modes:
        times[name].append(epoch(task))

# the gather launch alone: one event pair per launch, on the ring slots in turn
ts = task_b.train_data
gather_us = staging_us = item_host_us = None
gather_bytes = sum(B * s.length * (s.data.element_size() + (1 if s.kind == R.KIND_U8 else 4)) for s in pool.streams)
if dev.type == "cuda":
    pairs = []
    for k in range(110):
        lo = ts._offsets[k % (len(ts._offsets) - 1)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ts._ring.gather(k % ts.R, ts._table[lo:lo + B], B)
        e1.record()
        pairs.append((e0, e1))
    sync()
    gather_us = statistics.median(a.elapsed_time(b) * 1e3 for a, b in pairs[10:])
    # ... and what the step driver then does with a batch that is not in its own buffers: the copy of the announced batch (waveforms and
    # labels) into the captured step's static inputs, timed the same way on tensors of the same shapes
    src = ts._ring.out[0]
    dst = [torch.empty_like(t) for t in src]
    pairs = []
    for k in range(110):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d_, s_ in zip(dst, src):
            d_.copy_(s_, non_blocking=True)
        e1.record()
        pairs.append((e0, e1))
    sync()
    staging_us = statistics.median(a.elapsed_time(b) * 1e3 for a, b in pairs[10:])
    # ... and the host's share of one item (launch, ratio indexing, tuple): enqueue only, no synchronisation
    ts[0]
    sync()
    t0 = time.perf_counter()
    for k in range(1, 33):
        ts[k]
    item_host_us = (time.perf_counter() - t0) / 32 * 1e6
    sync()

med = {name: statistics.median(v) for name, v in times.items()}
for name, task in modes:
    d = task._driver
    print(json.dumps({"mode": name, "workload": "dcase2023 default.yaml, batch %d = %s x %d samples, Lightning-order loop, whole-step mode" % (B, list(BS), L),
                      "ms_per_step": round(med[name], 4), "spread_ms": round(max(times[name]) - min(times[name]), 4),
                      "rounds_ms": [round(t, 4) for t in times[name]], "steps_per_round": STEPS, "clips_per_s": round(B / med[name] * 1e3, 1),
                      "captured": getattr(d, "graph", None) is not None, "num_workers": task.num_workers,
                      "library_rev": _build.source_rev()}), flush=True)
a = 0.5 * (med["ready_batches_1"] + med["ready_batches_2"])
a_spread = abs(med["ready_batches_1"] - med["ready_batches_2"])
added = med["resident_set"] - a
allowed = None if gather_us is None else gather_us * 1e-3 + 2 * a_spread
print(json.dumps({"summary": "resident data", "rehearsal_not_a_measurement": REHEARSE, "a_ms": round(a, 4), "a_spread_ms": round(a_spread, 4),
                  "b_ms": round(med["resident_set"], 4), "c_ms": round(med["dataloader"], 4), "b_minus_a_ms": round(added, 4),
                  "gather_event_us": None if gather_us is None else round(gather_us, 2), "gather_bytes": gather_bytes,
                  "gather_GBps": None if gather_us is None else round(gather_bytes / gather_us * 1e-3, 1),
                  "staging_copy_event_us": None if staging_us is None else round(staging_us, 2),
                  "item_host_us": None if item_host_us is None else round(item_host_us, 2),
                  "hbm_achievable_GBps": 6300.0, "allowed_ms": None if allowed is None else round(allowed, 4),
                  "check_b_minus_a_le_gather_plus_2_spread": None if allowed is None else bool(added <= allowed),
                  "pool": pool.describe(), "pool_build_s": round(pool_s, 2), "device": torch.cuda.get_device_name(0) if dev.type == "cuda" else "cpu emulator",
                  "library": os.path.basename(_lib.get().path)}), flush=True)
