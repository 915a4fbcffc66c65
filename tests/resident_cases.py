"""Cases for the resident training set (desed_task_amd/resident.py, csrc/sed_data.hip), device-agnostic like parity_cases.py: dev = "cpu"
on the fiber emulator, "cuda" on the MI355X.  Every comparison is BIT-EXACT: the gather copies (int16 -> float is float(x) * 2^-15,
exact), so the expected values are plain torch indexing of the pools / the toy data sets and no tolerance appears anywhere.

Outputs of the direct kernel cases live inside byte buffers filled with 0xA5 (`Framed`): 4 KiB + 64 guard bytes on either side must be
intact after every launch.
"""
import random
import struct

import numpy as np
import pytest
import torch
from torch.utils.data import ConcatDataset, DataLoader, Dataset, RandomSampler

from desed_task_amd import _lib
from desed_task_amd import resident as R
from desed_task_amd.lookahead import LookaheadLoader

GUARD = 4096 + 64
CANARY = 0xA5
ROW_LENGTHS = (1, 3, 7, 8, 4095, 15999, 16000)       # 7 fp32: no row after the first is 16-byte aligned; 15999: alternating
N_ROWS = (1, 5, 48)
POOL_ROWS = 9
KINDS = (R.KIND_I16_TO_F32, R.KIND_F32, R.KIND_U8_TO_F32, R.KIND_U8)
_IN = {R.KIND_I16_TO_F32: torch.int16, R.KIND_F32: torch.float32, R.KIND_U8_TO_F32: torch.uint8, R.KIND_U8: torch.uint8}
_OUT = {R.KIND_I16_TO_F32: torch.float32, R.KIND_F32: torch.float32, R.KIND_U8_TO_F32: torch.float32, R.KIND_U8: torch.uint8}


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


class Framed:
    """(rows, length) elements of `dtype`, dense, 16-byte aligned, between two guard regions of canary bytes."""

    def __init__(self, dev, rows, length, dtype):
        self.nbytes = rows * length * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + self.nbytes,), CANARY, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
        self.body = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(rows, length)

    def assert_guards(self, what):
        host = self.buf.cpu()
        assert bool((host[:GUARD] == CANARY).all()), "%s: bytes BEFORE the output were written" % what
        assert bool((host[GUARD + self.nbytes:] == CANARY).all()), "%s: bytes BEHIND the output were written" % what


def make_pool(kind, length, seed, dev):
    """POOL_ROWS rows with the padded stride; the padding holds values no output may show."""
    g = torch.Generator().manual_seed(seed)
    dt = _IN[kind]
    stride = R.padded_stride(length, dt)
    assert stride >= length and (stride * torch.empty((), dtype=dt).element_size()) % 16 == 0
    if kind == R.KIND_I16_TO_F32:
        pool = torch.randint(-32768, 32768, (POOL_ROWS, stride), generator=g, dtype=torch.int32).to(torch.int16)
        pool[0, 0], pool[POOL_ROWS - 1, 0], pool[3, 0] = -32768, 32767, 0
        if length >= 3:
            pool[5, 0], pool[5, 1], pool[5, 2] = 32767, -32768, 0
            pool[POOL_ROWS - 1, length - 1] = -32768
        pool[:, length:] = 12345
    elif kind == R.KIND_F32:
        pool = torch.randn(POOL_ROWS, stride, generator=g)
        pool[:, length:] = float("nan")
    elif kind == R.KIND_U8_TO_F32:
        pool = torch.randint(0, 2, (POOL_ROWS, stride), generator=g, dtype=torch.uint8)
        pool[:, length:] = 77
    else:
        pool = torch.randint(0, 2, (POOL_ROWS, stride), generator=g, dtype=torch.uint8)
        pool[:, length:] = 99
    return pool.to(dev), stride


def expected(kind, pool_host, idx, length):
    rows = pool_host[torch.tensor(idx, dtype=torch.long), :length]
    if kind == R.KIND_I16_TO_F32:
        return rows.to(torch.float32) / 32768.0
    if kind == R.KIND_U8_TO_F32:
        return rows.to(torch.float32)
    return rows.clone()


def index_lists(n_rows, seed):
    """Indices that repeat and that hit row 0 and the last row."""
    if n_rows == 1:
        return [[0], [POOL_ROWS - 1]]
    if n_rows == 5:
        return [[POOL_ROWS - 1, 0, 3, 3, POOL_ROWS - 1]]
    idx = torch.randint(0, POOL_ROWS, (n_rows,), generator=torch.Generator().manual_seed(seed)).tolist()
    idx[0], idx[1], idx[2], idx[3] = 0, POOL_ROWS - 1, 4, 4
    return [idx]


def launch(dev, streams, idx):
    """streams: [(kind, pool (device), stride, length)] -> [Framed] written by ONE launch."""
    n_rows = len(idx)
    outs = [Framed(dev, n_rows, length, _OUT[kind]) for kind, _, _, length in streams]
    table = b"".join(struct.pack("<QQqii", pool.data_ptr(), o.body.data_ptr(), stride, length, kind)
                     for (kind, pool, stride, length), o in zip(streams, outs))
    desc = torch.frombuffer(bytearray(table), dtype=torch.uint8).clone().to(dev)
    idx_dev = torch.tensor(idx, dtype=torch.int32).to(dev)
    chunks = sum((length + R.CHUNK - 1) // R.CHUNK for _, _, _, length in streams)
    R.batch_gather(desc, len(streams), idx_dev, n_rows, chunks)
    sync(dev)
    return outs


def case_kernel_one_stream(dev, length):
    """Every kind alone, every n_rows, at one row length."""
    for kind in KINDS:
        pool, stride = make_pool(kind, length, 1000 * kind + length, dev)
        host = pool.cpu()
        before = host.clone()
        for n_rows in N_ROWS:
            for idx in index_lists(n_rows, 7 * length + n_rows):
                (out,) = launch(dev, [(kind, pool, stride, length)], idx)
                what = "kind %d, L %d, rows %d" % (kind, length, n_rows)
                got, ref = out.body.cpu(), expected(kind, host, idx, length)
                assert got.dtype == ref.dtype and got.shape == ref.shape
                if got.dtype == torch.float32:          # bit for bit (NaN-proof, -0.0-proof)
                    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), what
                else:
                    assert torch.equal(got, ref), what
                out.assert_guards(what)
        assert torch.equal(pool.cpu().view(torch.uint8), before.view(torch.uint8)), "the pool was written"


def case_kernel_four_streams(dev):
    """All four streams in one launch with different row lengths (one of them just past a chunk), 5 and 48 rows."""
    specs = [(R.KIND_I16_TO_F32, 1601), (R.KIND_U8_TO_F32, 100), (R.KIND_F32, R.CHUNK + 4), (R.KIND_U8, 10)]
    streams, hosts = [], []
    for kind, length in specs:
        pool, stride = make_pool(kind, length, 31 * kind + length, dev)
        streams.append((kind, pool, stride, length))
        hosts.append(pool.cpu())
    for n_rows in (5, 48):
        (idx,) = index_lists(n_rows, 99)
        outs = launch(dev, streams, idx)
        for (kind, _, _, length), host, out in zip(streams, hosts, outs):
            got, ref = out.body.cpu(), expected(kind, host, idx, length)
            assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), ("four streams", kind, n_rows)
            out.assert_guards("four streams, kind %d" % kind)
    # n_rows = 0 launches nothing; a malformed call is refused by the entry point
    lib = _lib.get()
    desc = torch.zeros(R.DESC_BYTES, dtype=torch.uint8, device=dev)
    idx0 = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = 0 if dev == "cpu" else torch.cuda.current_stream().cuda_stream
    assert lib._dll.sed_batch_gather(desc.data_ptr(), 1, idx0.data_ptr(), 0, 1, stream) == 0
    assert lib._dll.sed_batch_gather(desc.data_ptr(), 5, idx0.data_ptr(), 1, 1, stream) == -1
    assert lib._dll.sed_batch_gather(desc.data_ptr(), 0, idx0.data_ptr(), 1, 1, stream) == -1
    assert lib._dll.sed_batch_gather(desc.data_ptr(), 1, idx0.data_ptr(), 1, 0, stream) == -1
    sync(dev)


# ---- toy data sets with the reference's item contract ----------------------------------------------------------------------------
class ToySet(Dataset):
    """[audio (L,), labels (C, T), [ratio], (file name), (embeddings), (class mask)], deterministic.  role: "strong" | "weak" | "unlabeled"."""

    def __init__(self, n, length, role, seed, classes=10, frames=10, emb=None, mask=False, names=None, lengths=None):
        g = torch.Generator().manual_seed(seed)
        self.audio = [torch.randint(-32768, 32768, (length if lengths is None else lengths[i],), generator=g).float() / 32768.0 for i in range(n)]
        lab = (torch.rand(n, classes, frames, generator=g) < 0.25).float()
        if role == "weak":
            lab[:, :, 1:] = 0.0
        elif role == "unlabeled":
            lab[:] = 0.0
        self.labels = lab
        self.ratio = [0.5 + 0.5 * (i + 1) / n for i in range(n)]
        self.emb = torch.randn((n,) + tuple(emb), generator=g) if emb is not None else None
        self.mask = (torch.rand(n, classes, generator=g) < 0.5) if mask else None
        self.names = names

    def __len__(self):
        return len(self.audio)

    def __getitem__(self, i):
        out = [self.audio[i].clone(), self.labels[i].clone(), [self.ratio[i]]]
        if self.names is not None:
            out.append(self.names[i])
        if self.emb is not None:
            out.append(self.emb[i].clone())
        if self.mask is not None:
            out.append(self.mask[i].clone())
        return out


def toy_parts(length=1600, frames=10, emb=None, mask=False, seed=0):
    return [ToySet(3, length, "strong", seed + 1, frames=frames, emb=emb, mask=mask), ToySet(5, length, "weak", seed + 2, frames=frames, emb=emb, mask=mask),
            ToySet(8, length, "unlabeled", seed + 3, frames=frames, emb=emb, mask=mask)]


class GroupedBatches:
    """A batch = sizes[j] fresh draws from sampler j for every part j, as indices into the concatenation of the parts; an epoch ends
    with the part that runs out first.  (A stand-in written for these tests, for the recipe's concat batch sampler.)"""

    def __init__(self, samplers, sizes):
        self.samplers, self.sizes = list(samplers), list(sizes)
        self.first = [0]
        for s in self.samplers[:-1]:
            self.first.append(self.first[-1] + len(s))

    def __len__(self):
        return min(len(s) // b for s, b in zip(self.samplers, self.sizes))

    def __iter__(self):
        draws = [iter(s) for s in self.samplers]
        for _ in range(len(self)):
            batch = []
            for d, b, f in zip(draws, self.sizes, self.first):
                batch.extend(f + int(next(d)) for _ in range(b))
            yield batch


def grouped(parts, sizes):
    return GroupedBatches([RandomSampler(p) for p in parts], sizes)


def assert_same_batch(got, ref, what):
    """`got` from a resident set, `ref` from default_collate: same elements, values, dtypes, shapes (the [ratio] element included)."""
    assert len(got) == len(ref), (what, len(got), len(ref))
    for j, (a, b) in enumerate(zip(got, ref)):
        if torch.is_tensor(b):
            assert torch.is_tensor(a) and a.dtype == b.dtype and a.shape == b.shape, (what, j, a.dtype, b.dtype, a.shape, b.shape)
            assert torch.equal(a.cpu().contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (what, "element", j)
        elif isinstance(b, (list, tuple)) and b and torch.is_tensor(b[0]):
            assert isinstance(a, (list, tuple)) and len(a) == len(b), (what, j)
            for x, y in zip(a, b):
                assert x.device.type == "cpu" and x.dtype == y.dtype == torch.float64 and x.shape == y.shape and torch.equal(x, y), (what, j)
        else:
            assert list(a) == list(b), (what, j, a, b)


# ---- pool building -----------------------------------------------------------------------------------------------------------------
def case_pool_building(dev):
    parts = toy_parts(emb=(4, 6), mask=True)
    ds = ConcatDataset(parts)
    pool = R.ResidentPool.from_dataset(ds, dev)
    assert pool.n_clips == 16 and [s.name for s in pool.streams] == ["audio", "labels", "embeddings", "mask"]
    assert [s.kind for s in pool.streams] == [R.KIND_I16_TO_F32, R.KIND_U8_TO_F32, R.KIND_F32, R.KIND_U8]
    assert pool.nbytes == 16 * (1600 * 2 + 112 + 24 * 4 + 16) and "audio int16" in pool.describe() and "16 clips" in pool.describe()
    audio = pool.stream("audio").data.cpu()[:, :1600].float() / 32768.0
    for i in range(16):
        item = ds[i]
        assert torch.equal(audio[i], item[0]), "clip %d does not come back bit for bit" % i
        assert torch.equal(pool.stream("labels").data.cpu()[i, :100].float().view(10, 10), item[1])
        assert float(pool.ratios[i, 0]) == item[2][0]
    # one sample of 2^-16: "auto" goes to fp32 (also when the clip comes late: the int16 rows already stored are widened exactly)
    for where in (0, 9):
        parts2 = toy_parts()
        p, i = (0, where) if where < 3 else (2, where - 8)
        parts2[p].audio[i][5] = 2.0 ** -16
        ds2 = ConcatDataset(parts2)
        pool2 = R.ResidentPool.from_dataset(ds2, dev)
        assert pool2.stream("audio").kind == R.KIND_F32 and "audio float32" in pool2.describe()
        stored = pool2.stream("audio").data.cpu()[:, :1600]
        for k in range(16):
            assert torch.equal(stored[k], ds2[k][0]), (where, k)
        with pytest.raises(ValueError, match="lose bits"):
            R.ResidentPool.from_dataset(ds2, dev, audio_storage="int16")
    # out-of-range sample: 1.0 is 32768 / 32768
    parts3 = toy_parts()
    parts3[1].audio[2][0] = 1.0
    assert R.ResidentPool.from_dataset(ConcatDataset(parts3), dev).stream("audio").kind == R.KIND_F32
    assert R.ResidentPool.from_dataset(ds, dev, audio_storage="float32").stream("audio").kind == R.KIND_F32
    # labels containing 0.5 go to fp32
    parts4 = toy_parts()
    parts4[1].labels[3, 2, 0] = 0.5
    ds4 = ConcatDataset(parts4)
    pool4 = R.ResidentPool.from_dataset(ds4, dev)
    assert pool4.stream("labels").kind == R.KIND_F32 and pool4.stream("audio").kind == R.KIND_I16_TO_F32
    lab = pool4.stream("labels").data.cpu()[:, :100].view(16, 10, 10)
    for k in range(16):
        assert torch.equal(lab[k], ds4[k][1])
    # unequal lengths, file names
    with pytest.raises(ValueError, match="same\\s+length"):
        R.ResidentPool.from_dataset(ToySet(4, 1600, "strong", 5, lengths=[1600, 1600, 1500, 1600]), dev)
    named = ToySet(4, 1600, "strong", 5, names=["/d/a%d.wav" % i for i in range(4)])
    with pytest.raises(ValueError, match="file name"):
        R.ResidentPool.from_dataset(named, dev)
    # a tiny max_bytes raises before anything is allocated
    made = []
    orig = R.Stream.__init__

    def spy(self, *a, **k):
        made.append(a[0])
        orig(self, *a, **k)
    R.Stream.__init__ = spy
    try:
        with pytest.raises(MemoryError, match=r"needs %d bytes.*max_bytes is 1000\b" % pool.nbytes):
            R.ResidentPool.from_dataset(ds, dev, max_bytes=1000)
        assert made == []
        R.ResidentPool.from_dataset(ds, dev, max_bytes=pool.nbytes)
        assert made == ["audio", "labels", "embeddings", "mask"]
    finally:
        R.Stream.__init__ = orig


# ---- index guard -------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records the names of the library calls made while it is active."""

    def __enter__(self):
        self.lib, self.calls = _lib.get(), []
        orig = self.lib.call

        def call(name, *args):
            self.calls.append(name)
            return orig(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        del self.lib.call
        return False


def case_index_guard(dev):
    pool = R.ResidentPool.from_dataset(ConcatDataset(toy_parts()), dev)
    with _Spy() as spy:
        for bad in (pool.n_clips, -1):
            ts = R.ResidentTrainSet(pool, [[0, 1], [2, bad], [3, 4]])
            with pytest.raises(IndexError, match="out of range"):
                ts[0]
        assert spy.calls == [], spy.calls               # nothing was launched (nor anything else called)
        ts = R.ResidentTrainSet(pool, [[0, pool.n_clips - 1]])
        ts[0]
        assert spy.calls == ["sed_batch_gather"]
    sync(dev)


# ---- same batches as a DataLoader -----------------------------------------------------------------------------------------------
def case_same_batches_as_dataloader(dev, extras):
    parts = toy_parts(emb=(4, 6) if extras else None, mask=extras)
    ds = ConcatDataset(parts)
    pool = R.ResidentPool.from_dataset(ds, dev)
    sizes = (1, 2, 2)
    torch.manual_seed(1234)
    plain = DataLoader(ds, batch_sampler=grouped(parts, sizes))
    ref_epochs, ref_states = [], []
    for _ in range(2):
        ref_epochs.append(list(plain))
        ref_states.append(torch.get_rng_state())
    assert len(ref_epochs[0]) == 2 and not torch.equal(ref_epochs[0][0][0], ref_epochs[1][0][0])
    torch.manual_seed(1234)
    loader = LookaheadLoader(R.ResidentTrainSet(pool, grouped(parts, sizes)), batch_size=None)
    assert len(loader) == len(plain)
    for e in range(2):
        n = 0
        for k, batch in enumerate(loader):
            sync(dev)
            assert batch[0].device.type == torch.device(dev).type
            assert_same_batch(batch, ref_epochs[e][k], "epoch %d batch %d" % (e, k))
            n += 1
        assert n == len(ref_epochs[e])
        assert torch.equal(torch.get_rng_state(), ref_states[e]), "torch's RNG state differs after epoch %d" % e


# ---- ring ---------------------------------------------------------------------------------------------------------------------------
def case_ring(dev):
    parts = toy_parts()
    ds = ConcatDataset(parts)
    pool = R.ResidentPool.from_dataset(ds, dev)
    ring = R.ResidentTrainSet.R
    held = LookaheadLoader.MAX_HELD
    assert ring == held + 2
    batches = [[(3 * k) % 16, (5 * k + 1) % 16] for k in range(2 * ring + 3)]
    loader = LookaheadLoader(R.ResidentTrainSet(pool, batches), batch_size=None)
    window, ptrs = [], []
    for k, batch in enumerate(loader):
        ptrs.append(batch[0].data_ptr())
        window.append((k, batch))
        window = window[-held:]                          # hold MAX_HELD consecutive batches while fetching on
        sync(dev)
        for j, b in window:
            ref = torch.stack([ds[i][0] for i in batches[j]])
            assert torch.equal(b[0].cpu(), ref), "batch %d was overwritten while batch %d was fetched" % (j, k)
            assert torch.equal(b[1].cpu(), torch.stack([ds[i][1] for i in batches[j]]))
    assert len(ptrs) == len(batches) and len(set(ptrs[:ring])) == ring
    assert all(ptrs[k] == ptrs[k + ring] for k in range(len(ptrs) - ring))


# ---- through the step --------------------------------------------------------------------------------------------------------------
def case_through_the_step(dev, pretrained=False, epochs=2, length=16000):
    """The Lightning-order loop in whole-step mode over the resident set == over the plain loader of the same toy data, bit for bit:
    every loss, weights, BatchNorm buffers, Adam moments, the logged values.  3 batches per epoch of (1, 1, 2) clips."""
    from desed_task_amd import ops as _ops
    from oracle import sed_oracle as O
    from tests import parity_cases as P
    from tests.lightning_order import Trainer
    sizes = (1, 1, 2)
    frames = (1 + length // 256) // 4
    parts = toy_parts(length=length, frames=frames, emb=(768, 31) if pretrained else None, seed=40)
    ds = ConcatDataset(parts)
    sd = O.make_state_dict(seed=7, **({"embedding_size": 768} if pretrained else {}))

    def state(task):
        out = [task.sed_student.arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone()]
        for model in (task.sed_student, task.sed_teacher):
            for i in range(7):
                bn = getattr(model.cnn.cnn, "batchnorm%d" % i)
                out += [bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone()]
        osd = task.opt.state_dict()
        out += [torch.cat([osd["state"][i]["exp_avg"].reshape(-1).cpu() for i in sorted(osd["state"])]),
                torch.cat([osd["state"][i]["exp_avg_sq"].reshape(-1).cpu() for i in sorted(osd["state"])]),
                torch.tensor([float(osd["state"][0]["step"]), float(task.scheduler["scheduler"].step_num)])]
        return out

    results = {}
    for mode in ("plain", "resident"):
        task = P.build_task(dev, sizes, sd, dropout=0.5, specaug=True, rampup=5, torch_adam=True, whole_step=True, pretrained=pretrained)
        task.whole_step_warmup = 1
        if mode == "plain":
            task.train_data, task.train_sampler = ds, grouped(parts, sizes)
        else:
            pool = R.ResidentPool.from_dataset(ds, dev)
            assert pool.stream("audio").kind == R.KIND_I16_TO_F32 and pool.stream("labels").kind == R.KIND_U8_TO_F32
            task.train_data, task.train_sampler = R.ResidentTrainSet(pool, grouped(parts, sizes)), None
        random.seed(41); np.random.seed(101); torch.manual_seed(101)
        if dev != "cpu":
            torch.cuda.manual_seed(101)
        _ops.reseed_dropout()
        tr = Trainer(max_epochs=epochs, device=torch.device(dev))
        tr.fit(task)
        sync(dev)
        assert tr.global_step == epochs * 3
        assert isinstance(task.train_loader, LookaheadLoader)
        assert (task.train_loader.dataset is task.train_data) and (task.train_loader.batch_sampler is None) == (mode == "resident")
        drv = task._driver
        assert drv is not None
        if dev != "cpu":                                 # the captured path: eager only where an epoch ends
            assert drv.graph is not None and drv.eager_fallbacks == epochs, (drv.eager_fallbacks, epochs)
        results[mode] = ([float(l) for l in tr.losses], state(task), {k: float(v) for k, v in task.logged.items()})
    ref, got = results["plain"], results["resident"]
    assert got[0] == ref[0], (got[0], ref[0])
    assert len(set(ref[0])) == len(ref[0])               # (six different losses: the batches do differ)
    for a, b in zip(got[1], ref[1]):
        assert torch.equal(a, b)
    assert got[2] == ref[2] and len(ref[2]) >= 9, (got[2], ref[2])
    return ref[0]


# ---- eval set -----------------------------------------------------------------------------------------------------------------------
def case_eval_set(dev, length=16000):
    """Sequential batches with a short last one, file names where return_filename puts them; validation_step logs the same values
    and fills the same score buffers as over the plain loader."""
    from oracle import sed_oracle as O
    from tests import parity_cases as P
    frames = (1 + length // 256) // 4
    names = ["/d/synth_val/s%d.wav" % i for i in range(4)] + ["/d/weak/w%d.wav" % i for i in range(4)]
    parts = [ToySet(4, length, "strong", 71, frames=frames, names=names[:4]), ToySet(4, length, "weak", 72, frames=frames, names=names[4:])]
    ds = ConcatDataset(parts)
    collected = []
    pool = R.ResidentPool.from_dataset(ds, dev, filenames=collected)
    assert collected == names
    with pytest.raises(ValueError, match="file names for"):
        R.ResidentEvalSet(pool, 3, names[:-1])
    ev = R.ResidentEvalSet(pool, 3, collected)
    plain = DataLoader(ds, batch_size=3, shuffle=False, drop_last=False)
    assert len(ev) == len(plain) == 3
    ref_batches = list(plain)
    for k in range(3):
        got = ev[k]
        sync(dev)
        assert got[0].shape[0] == (3, 3, 2)[k] and list(got[3]) == names[3 * k:3 * k + 3]
        assert_same_batch(got, ref_batches[k], "eval batch %d" % k)
    with pytest.raises(IndexError):
        ev[3]
    # validation_step over both
    sd = O.make_state_dict(seed=7)
    logs = {}
    for mode in ("plain", "resident"):
        task = P.build_task(dev, (1, 1, 2), sd, dropout=0.5, specaug=True, rampup=100)
        task.hparams["data"] = {"weak_folder": "/d/weak", "synth_val_folder": "/d/synth_val"}
        task.hparams["training"].update(val_thresholds=[0.3, 0.5], median_window=7, batch_size_val=3)
        task.encoder = P._Encoder(["c%d" % i for i in range(10)], audio_len=length / 16000.0)
        task.valid_data = ds if mode == "plain" else R.ResidentEvalSet(pool, 3, collected)
        task.eval()
        seen = []
        loader = task.val_dataloader()
        assert len(loader) == 3
        with torch.no_grad():
            for k, batch in enumerate(loader):
                task.validation_step(task.transfer_batch_to_device(batch, torch.device(dev), 0), k)
                sync(dev)
                seen.append({key: float(v) for key, v in task.logged.items()})
        scores = {a: df.values.copy() for a, df in task.val_scores_postprocessed_buffer_student_synth.items()}
        logs[mode] = (seen, scores, float(task.get_weak_student_f1_seg_macro.compute()))
    assert logs["plain"][0] == logs["resident"][0] and any("val/synth/student/loss_strong" in d for d in logs["plain"][0])
    assert sorted(logs["plain"][1]) == sorted(logs["resident"][1]) == ["s%d" % i for i in range(4)]
    for a in logs["plain"][1]:
        assert np.array_equal(logs["plain"][1][a], logs["resident"][1][a]), a
    assert logs["plain"][2] == logs["resident"][2]
