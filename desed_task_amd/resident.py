"""A training set that lives in HBM: the data set is read ONCE, through the reference's own map-style data sets, into device pools,
and every batch is then assembled by one launch of `sed_batch_gather` (csrc/sed_data.hip) from an index table -- no DataLoader, no
decoding, no collate and no host-to-device copy per step.  Opt-in: `python -m desed_task_amd.launcher --resident_data`
(`training.resident_data: True`), or build the classes by hand and pass them to SEDTask4 as `train_data` / `valid_data`.

    pool  = ResidentPool.from_dataset(ConcatDataset([synth, weak, unlabeled]), device)      # one pass, index order
    train = ResidentTrainSet(pool, batch_sampler)       # SEDTask4(train_data=train, train_sampler=None): `yields_batches`
    valid = ResidentEvalSet(pool_val, batch_size_val, filenames)

Item contract (desed_task/dataio/datasets.py:187-237, :303-352, :395-433): [audio (L,), labels (C, T), [ratio], (file name),
(embeddings), (class mask)].  One pool per stream, rows padded to a multiple of 16 bytes:
    audio       int16 when every sample of every clip is k / 32768 with integer k in [-32768, 32767] -- what torchaudio.load yields for
                16-bit PCM, reproduced exactly by float(k) * 2^-15 --, else fp32
    labels      uint8 when every value is 0 or 1, else fp32
    embeddings  fp32
    class mask  uint8 (bool)
and the [ratio] values stay on the host.  A batch is what default_collate makes of the items: (audio (B, L) f32, labels (B, C, T) f32,
[float64 host tensor of B ratios], (embeddings), (mask bool)), elements the data set does not have omitted.

A resident set is a SNAPSHOT: whatever the data set draws in `__getitem__` -- the reference's random crop of a clip longer than
`pad_to` (datasets.py:33-41), and a strong clip's labels with it -- is drawn once, at the read, and kept for the run.

Batches are written into a ring of R = LookaheadLoader.MAX_HELD + 2 pre-allocated buffers (the look-ahead loader holds up to MAX_HELD
batches; one more is being fetched), so the per-step host work is one launch: no allocation, no synchronisation, and the epoch's
index table is validated on the host (0 <= idx < clips: the kernel checks nothing) and uploaded once per epoch.
"""
import struct

import torch

from . import _lib
from .lookahead import LookaheadLoader

_C = _lib.header_constants()
KIND_I16_TO_F32, KIND_F32, KIND_U8_TO_F32, KIND_U8 = (_C["SED_GATHER_I16_TO_F32"], _C["SED_GATHER_F32"], _C["SED_GATHER_U8_TO_F32"],
                                                       _C["SED_GATHER_U8"])
CHUNK, MAX_STREAMS, DESC_BYTES = _C["SED_GATHER_CHUNK"], _C["SED_GATHER_MAX_STREAMS"], _C["SED_GATHER_DESC_BYTES"]
_POOL_DTYPE = {KIND_I16_TO_F32: torch.int16, KIND_F32: torch.float32, KIND_U8_TO_F32: torch.uint8, KIND_U8: torch.uint8}
_KIND_NAME = {KIND_I16_TO_F32: "int16", KIND_F32: "float32", KIND_U8_TO_F32: "uint8", KIND_U8: "bool"}


def padded_stride(length, dtype):
    """Elements between pool rows: the row length rounded up to a multiple of 16 bytes."""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    return (int(length) + per16 - 1) // per16 * per16


def batch_gather(desc, n_streams, idx, n_rows, chunks_per_row):
    """One launch on the current stream (see include/sed_hip.h).  desc: uint8 device tensor of descriptors; idx: int32 device tensor."""
    _lib.check_tensor(desc, "desc")
    _lib.check_tensor(idx, "idx")
    _lib.get().call("sed_batch_gather", desc.data_ptr(), int(n_streams), idx.data_ptr(), int(n_rows), int(chunks_per_row),
                    _lib.stream_ptr(idx))


class Stream:
    """One pool: `rows` x `stride` elements of the kind's storage type on the device, `shape` = an item's shape (length = its numel)."""

    def __init__(self, name, kind, shape, rows, device):
        self.name, self.kind, self.shape = name, kind, tuple(int(s) for s in shape)
        self.length = 1
        for s in self.shape:
            self.length *= s
        if self.length < 1:
            raise ValueError("resident pool: the %s of an item is empty" % name)
        self.stride = padded_stride(self.length, _POOL_DTYPE[kind])
        self.data = torch.zeros((rows, self.stride), dtype=_POOL_DTYPE[kind], device=device)

    @staticmethod
    def planned_bytes(kind, shape, rows):
        n = 1
        for s in shape:
            n *= int(s)
        dt = _POOL_DTYPE[kind]
        return rows * padded_stride(n, dt) * torch.empty((), dtype=dt).element_size()

    @property
    def nbytes(self):
        return self.data.numel() * self.data.element_size()

    @property
    def out_dtype(self):
        return torch.bool if self.kind == KIND_U8 else torch.float32

    @property
    def chunks(self):
        return (self.length + CHUNK - 1) // CHUNK

    def widen(self):
        """int16 / uint8 storage -> fp32, values kept exactly (on the device)."""
        old = self.data
        scale = 1.0 / 32768.0 if self.kind == KIND_I16_TO_F32 else 1.0
        self.kind = KIND_F32
        self.stride = padded_stride(self.length, torch.float32)
        self.data = torch.zeros((old.shape[0], self.stride), dtype=torch.float32, device=old.device)
        self.data[:, :self.length] = old[:, :self.length].to(torch.float32) * scale


def _int16_exact(x):
    """Is every sample of x (fp32) an integer multiple of 2^-15 inside the int16 range?  (x * 32768 is exact in fp32.)"""
    y = x * 32768.0
    return bool(((y == y.round()) & (y >= -32768.0) & (y <= 32767.0)).all())


def _default_max_bytes(device):
    device = torch.device(device)
    if device.type == "cuda":
        return torch.cuda.mem_get_info(device)[0] // 2
    import os
    try:
        return os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE") // 2
    except (ValueError, OSError):       # pragma: no cover
        return None


class ResidentPool:
    """The device pools of one data set (all of it: every rank of a data-parallel run holds the whole pool)."""

    def __init__(self, streams, ratios, device):
        self.streams, self.ratios, self.device = streams, ratios, torch.device(device)
        self.n_clips = int(ratios.shape[0])

    def __len__(self):
        return self.n_clips

    @property
    def nbytes(self):
        return sum(s.nbytes for s in self.streams)

    def describe(self):
        return "%d clips, %d bytes (%s)" % (self.n_clips, self.nbytes, ", ".join("%s %s" % (s.name, _KIND_NAME[s.kind]) for s in self.streams))

    def stream(self, name):
        for s in self.streams:
            if s.name == name:
                return s
        return None

    @classmethod
    def from_dataset(cls, dataset, device, num_workers=0, audio_storage="auto", max_bytes=None, filenames=None):
        """Iterate `dataset` exactly once, in index order, and upload its items.  audio_storage: "auto" | "int16" | "float32".
        max_bytes: refuse a larger footprint (default: half of the device's free memory now).  filenames: a list that receives the
        items' file names (data sets built with return_filename=True, for ResidentEvalSet); without it such items are refused."""
        if audio_storage not in ("auto", "int16", "float32"):
            raise ValueError("audio_storage must be 'auto', 'int16' or 'float32', got %r" % (audio_storage,))
        device = torch.device(device)
        n = len(dataset)
        if n < 1:
            raise ValueError("resident pool: the data set is empty")
        if max_bytes is None:
            max_bytes = _default_max_bytes(device)
        loader = torch.utils.data.DataLoader(dataset, batch_size=None, shuffle=False, num_workers=num_workers)
        streams, ratios = None, None

        def check_budget(kinds_shapes, what):
            need = sum(Stream.planned_bytes(k, shp, n) for _, k, shp in kinds_shapes)
            if max_bytes is not None and need > max_bytes:
                raise MemoryError("resident pool: %s needs %d bytes for %d clips but max_bytes is %d" % (what, need, n, max_bytes))

        for i, item in enumerate(loader):
            parts = cls._split_item(item, i)
            if parts["filename"] is not None:
                if filenames is None:
                    raise ValueError("resident pool: item %d carries a file name (%r); a training pool takes data sets built without "
                                     "return_filename -- pass filenames=[] to collect them for a ResidentEvalSet" % (i, parts["filename"]))
                filenames.append(parts["filename"])
            audio = parts["audio"]
            exact = audio_storage != "float32" and _int16_exact(audio)
            if audio_storage == "int16" and not exact:
                raise ValueError("resident pool: audio_storage='int16' would lose bits: clip %d has samples that are not k / 32768 with "
                                 "integer k in [-32768, 32767]" % i)
            binary = bool(((parts["labels"] == 0) | (parts["labels"] == 1)).all())
            if streams is None:
                plan = [("audio", KIND_I16_TO_F32 if exact else KIND_F32, audio.shape),
                        ("labels", KIND_U8_TO_F32 if binary else KIND_F32, parts["labels"].shape)]
                if parts["embeddings"] is not None:
                    plan.append(("embeddings", KIND_F32, parts["embeddings"].shape))
                if parts["mask"] is not None:
                    plan.append(("mask", KIND_U8, parts["mask"].shape))
                check_budget(plan, "the pool")              # (before anything is allocated)
                streams = [Stream(name, kind, shape, n, device) for name, kind, shape in plan]
                ratios = torch.zeros((n, len(parts["ratio"])), dtype=torch.float64)
            by_name = {s.name: s for s in streams}
            have = {k for k in ("audio", "labels", "embeddings", "mask") if parts[k] is not None}
            if have != set(by_name):
                raise ValueError("resident pool: item %d has elements %s but item 0 had %s" % (i, sorted(have), sorted(by_name)))
            for name, s in by_name.items():
                if tuple(parts[name].shape) != s.shape:
                    raise ValueError("resident pool: the %s of item %d has shape %s but item 0 had %s: every clip must have the same "
                                     "length (build the data sets with pad_to)" % (name, i, tuple(parts[name].shape), s.shape))
            if len(parts["ratio"]) != ratios.shape[1]:
                raise ValueError("resident pool: item %d has %d ratio values, item 0 had %d" % (i, len(parts["ratio"]), ratios.shape[1]))
            for name, ok in (("audio", exact), ("labels", binary)):
                s = by_name[name]
                if s.kind != KIND_F32 and not ok:           # the first value this storage cannot hold: the pool goes to fp32, exactly
                    check_budget([(t.name, KIND_F32 if t is s else t.kind, t.shape) for t in streams], "the pool with fp32 %s" % name)
                    s.widen()
            ratios[i] = torch.as_tensor([float(r) for r in parts["ratio"]], dtype=torch.float64)
            for name, s in by_name.items():
                v = parts[name].reshape(-1)
                if s.kind == KIND_I16_TO_F32:
                    v = (v * 32768.0).to(torch.int16)
                elif s.kind in (KIND_U8_TO_F32, KIND_U8):
                    v = v.to(torch.uint8)
                else:
                    v = v.to(torch.float32)
                s.data[i, :s.length].copy_(v)
        if streams is None or i + 1 != n:
            raise ValueError("resident pool: the data set yielded %d items, len() says %d" % (0 if streams is None else i + 1, n))
        return cls(streams, ratios, device)

    @staticmethod
    def _split_item(item, i):
        if not isinstance(item, (list, tuple)) or len(item) < 3:
            raise ValueError("resident pool: item %d is not [audio, labels, [ratio], ...] (desed_task/dataio/datasets.py)" % i)
        audio, labels, ratio = item[0], item[1], item[2]
        if not (torch.is_tensor(audio) and audio.dim() == 1 and audio.is_floating_point()):
            raise ValueError("resident pool: element 0 of item %d must be a 1-D float waveform, got %s" % (
                i, tuple(audio.shape) if torch.is_tensor(audio) else type(audio).__name__))
        if not (torch.is_tensor(labels) and labels.dim() == 2):
            raise ValueError("resident pool: element 1 of item %d must be a (classes, frames) label matrix" % i)
        if torch.is_tensor(ratio):
            ratio = ratio.reshape(-1).tolist()
        if not isinstance(ratio, (list, tuple)):
            raise ValueError("resident pool: element 2 of item %d must be the [ratio] list of pad_audio" % i)
        out = {"audio": audio.float(), "labels": labels.float(), "ratio": list(ratio), "filename": None, "embeddings": None, "mask": None}
        for extra in item[3:]:
            if isinstance(extra, str) and out["filename"] is None and out["embeddings"] is None and out["mask"] is None:
                out["filename"] = extra
            elif torch.is_tensor(extra) and extra.dtype == torch.bool and out["mask"] is None:
                out["mask"] = extra
            elif torch.is_tensor(extra) and extra.is_floating_point() and out["embeddings"] is None and out["mask"] is None:
                out["embeddings"] = extra.float()
            else:
                raise ValueError("resident pool: item %d has an element this contract does not know (%s)" % (
                    i, type(extra).__name__ if not torch.is_tensor(extra) else "tensor %s %s" % (extra.dtype, tuple(extra.shape))))
        return out


class _Ring:
    """R slots of pre-allocated batch buffers for one pool, and the slot's descriptor tables in device memory (built once)."""

    def __init__(self, pool, rows, slots):
        self.pool, self.rows, self.slots = pool, int(rows), int(slots)
        dev = pool.device
        self.out = [[torch.empty((self.rows,) + s.shape, dtype=s.out_dtype, device=dev) for s in pool.streams] for _ in range(slots)]
        self.n_streams = len(pool.streams)
        assert 1 <= self.n_streams <= MAX_STREAMS
        self.chunks_per_row = sum(s.chunks for s in pool.streams)
        table = bytearray()
        for slot in range(slots):
            for s, o in zip(pool.streams, self.out[slot]):
                table += struct.pack("<QQqii", s.data.data_ptr(), o.data_ptr(), s.stride, s.length, s.kind)
        assert len(table) == slots * self.n_streams * DESC_BYTES
        self.desc = torch.frombuffer(table, dtype=torch.uint8).clone().view(slots, self.n_streams * DESC_BYTES).to(dev)

    def gather(self, slot, idx_dev, n_rows):
        """-> the slot's tensors (their first n_rows rows), written by one launch on the current stream."""
        if n_rows > self.rows or idx_dev.numel() < n_rows:
            raise ValueError("resident ring: %d rows asked for, the slot holds %d and the index window %d" % (n_rows, self.rows, idx_dev.numel()))
        batch_gather(self.desc[slot], self.n_streams, idx_dev, n_rows, self.chunks_per_row)
        outs = self.out[slot]
        return outs if n_rows == self.rows else [o[:n_rows] for o in outs]


def _validated_table(batches, n_clips):
    """The epoch's batches as one int32 host table + the offsets of its batches; raises unless 0 <= idx < n_clips everywhere."""
    offsets = [0]
    for b in batches:
        offsets.append(offsets[-1] + len(b))
    flat = torch.tensor([int(i) for b in batches for i in b], dtype=torch.int64)
    if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= n_clips):
        bad = flat[(flat < 0) | (flat >= n_clips)]
        raise IndexError("resident set: the sampler yielded index %d, the pool holds clips 0 .. %d (%d indices out of range): nothing "
                         "was launched" % (int(bad[0]), n_clips - 1, bad.numel()))
    return flat.to(torch.int32), offsets


def _assemble(pool, outs, ratios, filenames=None):
    """default_collate's order: audio, labels, [ratios], (file names), (embeddings), (mask)."""
    by = dict(zip((s.name for s in pool.streams), outs))
    batch = [by["audio"], by["labels"], [ratios[:, j].contiguous() for j in range(ratios.shape[1])]]
    if filenames is not None:
        batch.append(filenames)
    for name in ("embeddings", "mask"):
        if name in by:
            batch.append(by[name])
    return tuple(batch)


class ResidentTrainSet(torch.utils.data.Dataset):
    """Item k = batch k of the current epoch, gathered on the device.  Item 0 draws the epoch from the batch sampler -- exactly what a
    DataLoader would consume of it, so torch's RNG stream is the one of `DataLoader(dataset, batch_sampler=batch_sampler)`."""
    yields_batches = True
    R = LookaheadLoader.MAX_HELD + 2

    def __init__(self, pool, batch_sampler):
        self.pool, self.batch_sampler = pool, batch_sampler
        self._ring = None
        self._table = self._offsets = None
        self._served = 0            # batches handed out so far, over all epochs: the ring position

    def __len__(self):
        return len(self.batch_sampler)

    def set_epoch(self, epoch):
        if hasattr(self.batch_sampler, "set_epoch"):
            self.batch_sampler.set_epoch(epoch)

    def __iter__(self):
        for k in range(len(self)):
            yield self[k]

    def _draw_epoch(self):
        batches = [list(b) for b in iter(self.batch_sampler)]
        host, self._offsets = _validated_table(batches, self.pool.n_clips)
        if not batches:
            raise IndexError("resident set: the batch sampler yielded no batch")
        rows = max(len(b) for b in batches)
        if self._ring is None or self._ring.rows < rows:
            self._ring = _Ring(self.pool, rows, self.R)
        self._host = host
        self._table = host.to(self.pool.device)         # once per epoch

    def __getitem__(self, k):
        if k == 0:
            self._draw_epoch()
        if self._table is None or not 0 <= k < len(self._offsets) - 1:
            raise IndexError("resident set: batch %d of an epoch of %d" % (k, 0 if self._offsets is None else len(self._offsets) - 1))
        lo, hi = self._offsets[k], self._offsets[k + 1]
        outs = self._ring.gather(self._served % self.R, self._table[lo:hi], hi - lo)
        self._served += 1
        return _assemble(self.pool, outs, self.pool.ratios[self._host[lo:hi].long()])


class ResidentEvalSet(torch.utils.data.Dataset):
    """`valid_data` from a pool: item k = clips [k * batch_size, (k + 1) * batch_size) in pool order (the last batch may be short),
    with the file names where `return_filename=True` puts them."""
    yields_batches = True
    R = 2

    def __init__(self, pool, batch_size, filenames=None):
        if filenames is not None and len(filenames) != pool.n_clips:
            raise ValueError("resident eval set: %d file names for %d clips" % (len(filenames), pool.n_clips))
        self.pool, self.batch_size = pool, int(batch_size)
        self.filenames = list(filenames) if filenames is not None else None
        self._ring = _Ring(pool, min(self.batch_size, pool.n_clips), self.R)
        self._table = torch.arange(pool.n_clips, dtype=torch.int32).to(pool.device)
        self._served = 0

    def __len__(self):
        return (self.pool.n_clips + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for k in range(len(self)):
            yield self[k]

    def __getitem__(self, k):
        if not 0 <= k < len(self):
            raise IndexError("resident eval set: batch %d of %d" % (k, len(self)))
        lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, self.pool.n_clips)
        outs = self._ring.gather(self._served % self.R, self._table[lo:hi], hi - lo)
        self._served += 1
        return _assemble(self.pool, outs, self.pool.ratios[lo:hi], None if self.filenames is None else self.filenames[lo:hi])
