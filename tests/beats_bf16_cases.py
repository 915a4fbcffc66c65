"""Cases for the single-product "bf16" mode of the frozen BEATs extractor (`BEATs.set_precision("bf16")`, the eight *_bf16x1 entries of
include/sed_hip.h under "the extractor's single-product mode").  Device-agnostic like bf16_mode_cases.py: dev = "cpu" runs the
fiber-emulator build, "cuda" the library on the MI355X.

The mode: both operands of every contraction rounded once to bf16 (r16), one MFMA per product, fp32 accumulation; bias, GELU, softmax,
LayerNorm and residuals in fp32.  So the model of a contraction entry is the float64 contraction of the ROUNDED operands, and against it
only the fp32 accumulation is left: the tier-B bound of contraction_cases.py, BETA (sqrt(K) + 2) 2^-24 S.  Through GELU (Lipschitz
constant 1.13) the bound is 1.13 x that + 8 * 2^-24 (1 + |GELU(pre)|) for the fp32 erff and epilogue roundings.

The single-product tile image, restated here on the host (`tile_image1`) from the text at sed_split_tiles_bf16x1's prototype:
X (R, K), K % 32 == 0 -> ceil(R / 256) * (K / 32) blocks in (row panel, K tile) order; block = [k half (k / 16) & 1][256 rows][16] bf16 bit
patterns of bf16(x); the 8-k octet o of row r of a half sits at slot o ^ ((r >> 3) & 1); rows >= R are zero; ceil(R / 256) * 256 * K words.

Bit equality: a three-product entry whose operands are bf16 values already has lo = 0 and adds exact zeros to the same ascending-k chain of
hi * hi MFMAs, so the Linear and position-convolution twins must torch.equal it there.

Measured (largest |err| / bound; all runs in profiles/bf16_beats.md, "Test figures"):
                                      MI355X      CPU emulator
  Linear entries (generic, tiles)      0.067          0.095
  split2 (first half, sum)             0.091          0.121
  position convolution                 0.005          0.011
  attention (four cases)               0.277          0.277
  extractor vs fixture, max / E_max  1.03 (2 layers), 0.97 (12 layers); emulator 1.03, 1.05 -- the bound is 2
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as TF

from desed_task_amd import _lib
from tests import contraction_cases as C

BETA, U24 = C.BETA, C.U24
NEW_ENTRIES = ("sed_linear_bf16x1", "sed_split_tiles_bf16x1", "sed_layernorm_tiles_bf16x1", "sed_linear_tiles_bf16x1",
               "sed_linear_tiles_out_bf16x1", "sed_linear_tiles_split2_bf16x1", "sed_posconv_bf16x1", "sed_attention_relpos_bf16x1")
LINEAR_SHAPES = ((300, 256, 64, 0), (513, 512, 96, 1), (256, 256, 32, 1), (700, 768, 160, 0), (2100, 256, 64, 0))      # (M, N, K, act)
IMAGE_SHAPES = ((300, 64), (513, 96), (256, 32), (2100, 64))                                                            # (R, K)
LN_SHAPES = ((300, 256), (513, 768), (70, 1024))                                                                        # (M, D)
ATTN_SHAPES = ((2, 100, 2), (1, 130, 2))                                                                                # (B, T, H)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS = {}
ICANARY = 0x5A5B                      # canary of the 16-bit image buffers


def r16(t):
    """fp32 -> rounded once to bf16 (round to nearest even), back in fp32."""
    return t.bfloat16().float()


def to(dev, *ts):
    out = tuple(t.to(dev).contiguous() for t in ts)
    return out if len(out) > 1 else out[0]


def gelu64(v):
    return TF.gelu(v.double())


# ---- the image, restated ------------------------------------------------------------------------------------------------------------
def bits_to_image1(bits):
    """(P * 256, K) int16 bf16 bit patterns -> the single-product image (int16, P * 256 * K words)."""
    rows_all, K = bits.shape
    Pn = rows_all // 256
    v = bits.view(Pn, 256, K // 32, 2, 2, 8)                                       # (panel, row, K tile, half, octet, 8)
    sw = ((torch.arange(256) >> 3) & 1).view(1, 256, 1, 1, 1, 1)
    octs = torch.arange(2).view(1, 1, 1, 1, 2, 1)
    src = (octs ^ sw).expand(Pn, 256, K // 32, 2, 2, 8)                             # slot s holds octet s ^ sw
    img = torch.gather(v, 4, src.contiguous())
    return img.permute(0, 2, 3, 1, 4, 5).contiguous().view(-1)                     # (panel, K tile, half, row, slot, 8)


def tile_image1(X):
    """X (R, K) float32 on the host -> its single-product image: r16(X), rows >= R zero."""
    R, K = X.shape
    Pn = (R + 255) // 256
    Xp = torch.zeros(Pn * 256, K)
    Xp[:R] = X
    return bits_to_image1(Xp.to(torch.bfloat16).view(torch.int16))


def image1_to_bits(img, R, K):
    """Inverse of bits_to_image1: -> (ceil(R / 256) * 256, K) int16 bit patterns (the padded rows included)."""
    Pn = (R + 255) // 256
    v = img.view(Pn, K // 32, 2, 256, 2, 8)                                        # (panel, K tile, half, row, slot, 8)
    sw = ((torch.arange(256) >> 3) & 1).view(1, 1, 1, 256, 1, 1)
    octs = torch.arange(2).view(1, 1, 1, 1, 2, 1)
    src = (octs ^ sw).expand(Pn, K // 32, 2, 256, 2, 8)                             # octet o sits in slot o ^ sw
    b = torch.gather(v, 4, src.contiguous())                                        # (panel, K tile, half, row, octet, 8)
    return b.permute(0, 3, 1, 2, 4, 5).contiguous().view(Pn * 256, K)


def image3_hi_bits(img3, R, K):
    """The hi plane of a THREE-product image (parity_cases.tile_image's layout: (panel, k / 16, plane, row, slot, 8)) as (P * 256, K) bits."""
    Pn = (R + 255) // 256
    v = img3.view(Pn, K // 16, 2, 256, 2, 8)[:, :, 0]                               # (panel, K tile of 16, row, slot, 8)
    sw = ((torch.arange(256) >> 3) & 1).view(1, 1, 256, 1, 1)
    octs = torch.arange(2).view(1, 1, 1, 2, 1)
    src = (octs ^ sw).expand(Pn, K // 16, 256, 2, 8)
    b = torch.gather(v, 3, src.contiguous())                                        # (panel, K tile, row, octet, 8)
    return b.permute(0, 2, 1, 3, 4).contiguous().view(Pn * 256, K)


class IFrame:
    """n 16-bit words inside a canary-filled int16 buffer (16-byte aligned window, 4 096 canaries on either side)."""
    GUARD = 4096

    def __init__(self, dev, n, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * self.GUARD,), ICANARY, dtype=torch.int16, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        if fill is not None:
            self.view().fill_(fill)

    def view(self):
        return self.buf[self.GUARD:self.GUARD + self.n]

    def ptr(self):
        return self.view().data_ptr()

    def get(self):
        return self.view().cpu().clone()

    def assert_frame(self, what):
        b = self.buf.cpu()
        bad = int((b[:self.GUARD] != ICANARY).sum()) + int((b[self.GUARD + self.n:] != ICANARY).sum())
        assert bad == 0, "%s: %d canaries around the image overwritten" % (what, bad)


def words1(R, K):
    return ((R + 255) // 256) * 256 * K


# ---- 1. the feature exists ----------------------------------------------------------------------------------------------------------
def tiny_checkpoint(layers=1):
    from oracle import beats_oracle as BO
    cfg = dict(BO.BEATS_ITER3_CFG, encoder_layers=layers)
    return {"cfg": cfg, "model": BO.make_beats_state_dict(cfg, seed=3)}


def case_mode_exists(lib_path):
    """The eight entries are in the header and in nm -D of the library; BEATsModel(precision="bf16") constructs; "f32" raises ValueError
    naming the two modes; SED_BEATS_PRECISION is honoured when no argument is given."""
    import subprocess
    from desed_task_amd.beats import BEATsModel, BEATs, BEATsConfig
    protos = _lib.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos, name
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert set(NEW_ENTRIES) <= exported, sorted(set(NEW_ENTRIES) - exported)
    ck = tiny_checkpoint()
    saved = os.environ.pop("SED_BEATS_PRECISION", None)
    try:
        m = BEATsModel(checkpoint=ck, precision="bf16")
        keys = list(m.state_dict().keys())
        assert m.model.precision == "bf16"
        assert BEATsModel(checkpoint=ck).model.precision == "bf16x3"                   # the default stays the three-product mode
        for bad in ("f32", "bf16x1", 16):
            for call in (lambda: m.set_precision(bad), lambda: m.model.set_precision(bad), lambda: BEATsModel(checkpoint=ck, precision=bad)):
                try:
                    call()
                    raise AssertionError("precision %r must be refused" % (bad,))
                except ValueError as e:
                    assert "bf16x3" in str(e) and "'bf16'" in str(e), str(e)
        assert m.model.precision == "bf16"                                             # a refused mode changes nothing
        m.set_precision("bf16x3")
        assert m.model.precision == "bf16x3" and list(m.state_dict().keys()) == keys
        os.environ["SED_BEATS_PRECISION"] = "bf16"
        assert BEATsModel(checkpoint=ck).model.precision == "bf16"
        assert BEATs(BEATsConfig(ck["cfg"])).precision == "bf16"
        assert BEATsModel(checkpoint=ck, precision="bf16x3").model.precision == "bf16x3"    # an argument wins over the environment
        assert m.set_precision(None).model.precision == "bf16"
        os.environ["SED_BEATS_PRECISION"] = "f32"
        try:
            BEATsModel(checkpoint=ck)
            raise AssertionError("SED_BEATS_PRECISION=f32 must be refused")
        except ValueError:
            pass
    finally:
        os.environ.pop("SED_BEATS_PRECISION", None)
        if saved is not None:
            os.environ["SED_BEATS_PRECISION"] = saved


# ---- 2. images ------------------------------------------------------------------------------------------------------------------------
def case_split_tiles(dev):
    lib = _lib.get()
    g = torch.Generator().manual_seed(41)
    for (R, K) in IMAGE_SHAPES:
        X = torch.randn(R, K, generator=g) * 10.0 ** (torch.rand(R, 1, generator=g) * 4 - 2)
        Xd = to(dev, X)
        fr = IFrame(dev, words1(R, K))
        lib.call("sed_split_tiles_bf16x1", Xd.data_ptr(), fr.ptr(), R, K, C.stream(dev))
        C.sync(dev)
        assert torch.equal(fr.get(), tile_image1(X)), (R, K, "image differs from the host restatement of r16(x)")
        fr.assert_frame("sed_split_tiles_bf16x1 (%d, %d)" % (R, K))
        assert torch.equal(image1_to_bits(fr.get(), R, K)[:R].view(torch.bfloat16).float(), r16(X))      # (the inverse used by the other cases)
    Xd = to(dev, torch.randn(64, 48, generator=g))
    fr = IFrame(dev, words1(64, 64))
    assert C.rc("sed_split_tiles_bf16x1", Xd.data_ptr(), fr.ptr(), 64, 48, C.stream(dev)) == C.SED_ERR_UNSUPPORTED, "K % 32 != 0 must be refused"
    assert C.rc("sed_split_tiles_bf16x1", Xd.data_ptr(), fr.ptr(), 64, 16, C.stream(dev)) == C.SED_ERR_UNSUPPORTED, "K % 32 != 0 must be refused"
    assert C.rc("sed_split_tiles_bf16x1", None, fr.ptr(), 64, 32, C.stream(dev)) == C.SED_ERR_ARG
    C.sync(dev)
    assert bool((fr.get() == ICANARY).all()), "a refused call wrote"


def case_layernorm_tiles(dev):
    lib = _lib.get()
    g = torch.Generator().manual_seed(14)
    for (M, D) in LN_SHAPES:
        x, x2, res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
        gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
        xd, x2d, rd, gd, bd = to(dev, x, x2, res, gamma, beta)
        st = C.stream(dev)
        for (use2, user, alpha) in ((False, False, 1.0), (True, True, 1.7), (False, True, 0.5)):
            args = (xd.data_ptr(), x2d.data_ptr() if use2 else None, rd.data_ptr() if user else None, float(alpha), gd.data_ptr(), bd.data_ptr())
            y3 = C.Frame(dev, M, D)
            yt3 = torch.zeros(2 * words1(M, D), dtype=torch.int16, device=dev)
            lib.call("sed_layernorm_tiles", *args, y3.ptr(), yt3.data_ptr(), M, D, 1e-5, st)
            y1 = C.Frame(dev, M, D)
            fr = IFrame(dev, words1(M, D), fill=0)
            lib.call("sed_layernorm_tiles_bf16x1", *args, y1.ptr(), fr.ptr(), M, D, 1e-5, st)
            C.sync(dev)
            what = "sed_layernorm_tiles_bf16x1 (%d, %d) x2=%s res=%s" % (M, D, use2, user)
            y1.assert_frame(what)
            fr.assert_frame(what)
            y = y1.get()
            assert torch.equal(y, y3.get()), what + ": y differs from sed_layernorm_tiles' y"
            pre = x.double() + (x2.double() if use2 else 0) + (alpha * res.double() if user else 0)
            ref = TF.layer_norm(pre, (D,), gamma.double(), beta.double(), 1e-5)
            assert (y.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item()), what
            assert torch.equal(fr.get(), tile_image1(y)), what + ": image differs from the host restatement of r16(y)"
    # (every D the entry takes is a multiple of 256: there is no K % 32 != 0 to refuse here; an unsupported D is)
    assert C.rc("sed_layernorm_tiles_bf16x1", xd.data_ptr(), None, None, 1.0, gd.data_ptr(), bd.data_ptr(), y1.ptr(), fr.ptr(), 4, 96, 1e-5, st) == C.SED_ERR_UNSUPPORTED


# ---- 3 - 6. Linear entries ---------------------------------------------------------------------------------------------------------------
class LinearData:
    """Seeded operands of one table row and the float64 models on the rounded operands.  Built once per row, never modified."""
    _cache = {}

    @classmethod
    def get(cls, row, rounded=False):
        key = (row, rounded)
        if key not in cls._cache:
            cls._cache[key] = cls(row, rounded)
        return cls._cache[key]

    def __init__(self, row, rounded):
        M, N, K, act = row
        g = torch.Generator().manual_seed(5000 + M + 3 * N + 7 * K + act)
        self.row = row
        self.A = torch.randn(M, K, generator=g)
        self.W = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.bias = torch.randn(N, generator=g)
        if rounded:
            self.A, self.W = r16(self.A), r16(self.W)
        self._m = {}

    def model(self, bias=True, khalf=False, rnd=True):
        """(pre, out, bound): pre = f(A) . f(W)^T (+ bias) in float64 over all of K or its first half, out = act(pre), bound per element."""
        key = (bias, khalf, rnd)
        if key not in self._m:
            M, N, K, act = self.row
            kk = K // 2 if khalf else K
            f = r16 if rnd else (lambda t: t)
            a, w = f(self.A)[:, :kk].double(), f(self.W)[:, :kk].double()
            pre = a @ w.t() + (self.bias.double() if bias else 0.0)
            S = r16(self.A)[:, :kk].double().abs() @ r16(self.W)[:, :kk].double().abs().t() + (self.bias.double().abs() if bias else 0.0)
            if act:
                out = gelu64(pre)
                bound = 1.13 * BETA * C.tier_b_unit(kk, S) + 8 * U24 * (1.0 + out.abs())
            else:
                out, bound = pre, BETA * C.tier_b_unit(kk, S)
            self._m[key] = (pre, out, bound)
        return self._m[key]


def _check(dev, what, got, out, bound):
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err = (got.double() - out).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("[beats bf16] %s %s: |err| / bound max %.3f" % (dev, what, ratio))
    STATS[(dev, what.split(" ")[0])] = max(STATS.get((dev, what.split(" ")[0]), 0.0), ratio)
    assert ratio <= 1.0, "%s: %d of %d elements outside the bound, worst |err| / bound = %.3f" % (what, int((err > bound).sum()), err.numel(), ratio)


def linear_images(dev, d, sfx="_bf16x1"):
    """The activation's and the weight's tile images of a row (device int16 tensors), by the library's own split entry."""
    M, N, K, act = d.row
    lib = _lib.get()
    Ad, Wd = to(dev, d.A, d.W)
    pl = 1 if sfx == "_bf16x1" else 2
    At = torch.full((pl * words1(M, K),), 77, dtype=torch.int16, device=dev)
    Wt = torch.full((pl * words1(N, K),), 77, dtype=torch.int16, device=dev)
    lib.call("sed_split_tiles" + sfx, Ad.data_ptr(), At.data_ptr(), M, K, C.stream(dev))
    lib.call("sed_split_tiles" + sfx, Wd.data_ptr(), Wt.data_ptr(), N, K, C.stream(dev))
    return At, Wt


def run_linear_entries(dev, d, sfx="_bf16x1"):
    """Every fp32-output run of a row through the `sfx` family: {name: host tensor}; frames checked."""
    M, N, K, act = d.row
    lib = _lib.get()
    st = C.stream(dev)
    Ad, Wd, bd = to(dev, d.A, d.W, d.bias)
    At, Wt = linear_images(dev, d, sfx)
    out = {}

    def run(name, entry, *args, rows=M):
        fr = C.Frame(dev, rows, N)
        lib.call(entry, *[a if a != "OUT" else fr.ptr() for a in args])
        C.sync(dev)
        fr.assert_frame("%s%s %s %s" % (entry, "", d.row, name))
        out[name] = fr.get()

    run("generic", "sed_linear" + sfx, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), "OUT", M, N, K, act, st)
    run("generic nobias", "sed_linear" + sfx, Ad.data_ptr(), Wd.data_ptr(), None, "OUT", M, N, K, act, st)
    run("tiles", "sed_linear_tiles" + sfx, At.data_ptr(), Wt.data_ptr(), bd.data_ptr(), "OUT", M, N, K, act, st)
    run("tiles nobias", "sed_linear_tiles" + sfx, At.data_ptr(), Wt.data_ptr(), None, "OUT", M, N, K, act, st)
    _lib.set_tuning("linear_tiles", 16)             # 16 workgroups: every workgroup walks several tiles (tile hand-over, DMA cursor)
    try:
        run("tiles 16wg", "sed_linear_tiles" + sfx, At.data_ptr(), Wt.data_ptr(), bd.data_ptr(), "OUT", M, N, K, act, st)
    finally:
        _lib.set_tuning("linear_tiles", 0)
    if (K // 32) % 2 == 0 and not act:
        run("split2", "sed_linear_tiles_split2" + sfx, At.data_ptr(), Wt.data_ptr(), bd.data_ptr(), "OUT", M, N, K, st, rows=2 * M)
    return out


def case_linear_entries(dev, row):
    d = LinearData.get(row)
    M, N, K, act = row
    out = run_linear_entries(dev, d)
    for name, got in out.items():
        what = "%s %s %s" % ("sed_linear_tiles_bf16x1" if "tiles" in name or name == "split2" else "sed_linear_bf16x1", row, name)
        if name == "split2":
            _, o1, b1 = d.model(True, khalf=True)
            _check(dev, what.replace("tiles_", "tiles_split2_") + " first half", got[:M], o1, b1)
            _, o, b = d.model(True)
            _check(dev, what.replace("tiles_", "tiles_split2_") + " sum", got[:M] + got[M:], o, b)
        else:
            _, o, b = d.model("nobias" not in name)
            _check(dev, what, got, o, b)


def case_linear_refusals(dev):
    d = LinearData.get(LINEAR_SHAPES[2])
    M, N, K, act = d.row
    At, Wt = linear_images(dev, d)
    fr = C.Frame(dev, 2 * M, N)
    st = C.stream(dev)
    assert C.rc("sed_linear_tiles_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, 128, K, 0, st) == C.SED_ERR_UNSUPPORTED, "N % 256 != 0"
    assert C.rc("sed_linear_tiles_out_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, 128, K, 0, st) == C.SED_ERR_UNSUPPORTED, "N % 256 != 0"
    assert C.rc("sed_linear_tiles_split2_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, 128, 64, st) == C.SED_ERR_UNSUPPORTED, "N % 256 != 0"
    assert C.rc("sed_linear_tiles_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, N, 48, 0, st) == C.SED_ERR_UNSUPPORTED, "K % 32 != 0"
    assert C.rc("sed_linear_tiles_split2_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, N, K, st) == C.SED_ERR_UNSUPPORTED, "(K / 32) odd"
    assert C.rc("sed_linear_tiles_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, N, K, 2, st) == C.SED_ERR_ARG, "act = 2"
    assert C.rc("sed_linear_bf16x1", At.data_ptr(), Wt.data_ptr(), None, fr.ptr(), M, N, K, 2, st) == C.SED_ERR_ARG, "act = 2"
    assert C.rc("sed_linear_tiles_bf16x1", None, Wt.data_ptr(), None, fr.ptr(), M, N, K, 0, st) == C.SED_ERR_ARG, "null image"
    C.sync(dev)
    fr.assert_frame("refused calls")
    assert bool((fr.bits() == C.CANARY_BITS).all()), "a refused call wrote"


def run_linear_out(dev, d, sfx="_bf16x1"):
    M, N, K, act = d.row
    At, Wt = linear_images(dev, d, sfx)
    bd = to(dev, d.bias)
    fr = IFrame(dev, (1 if sfx == "_bf16x1" else 2) * words1(M, N))
    _lib.get().call("sed_linear_tiles_out" + sfx, At.data_ptr(), Wt.data_ptr(), bd.data_ptr(), fr.ptr(), M, N, K, act, C.stream(dev))
    C.sync(dev)
    fr.assert_frame("sed_linear_tiles_out%s %s" % (sfx, d.row))
    return fr.get()


def r16_of_float64(v):
    """float64 -> the nearest bf16 number (ties to even), as float64, without an fp32 rounding in between."""
    step = _bf16_step(v)
    return torch.where(v == 0, v, torch.round(v / step.clamp_min(1e-300)) * step)


def boundary_allowance(got, out, bound):
    """got: fp32 values that are bf16 numbers; out: the float64 model before its rounding.  -> (ok, used).  ok: got is the bf16 rounding of
    SOME value within `bound` of out, i.e. r16(out - bound) <= got <= r16(out + bound) (rounding is monotone).  Wherever the bf16 step at
    out exceeds the bound -- every element but GELU's far negative tail -- this is exactly "r16(out), or its neighbour where out lies within
    the bound of the rounding boundary between the two".  In GELU's tail (pre < -4.5: |GELU| < 1e-5, 1 + erf cancels) and where a product
    cancels to nearly zero the bf16 grid (step < 1e-7) is finer than the fp32 error the Linear bound allows for, and several steps fit inside it
    (case_linear_out_image refuses more than one step wherever |out| > 1e-4).  used = the elements where got is
    not r16(out): all of them count against the 2 % cap."""
    t = r16_of_float64(out)
    g = got.double()
    ok = (g >= r16_of_float64(out - bound)) & (g <= r16_of_float64(out + bound))
    return ok, g != t


def _bf16_step(v):
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-300)))
    return torch.where(v == 0, torch.zeros_like(v), 2.0 ** (e - 7))


def case_linear_out_image(dev, row, max_fraction=0.02):
    """sed_linear_tiles_out_bf16x1: the image decodes to r16(act(pre)) exactly, except where act(pre) lies within the Linear bound of a bf16
    rounding boundary (boundary_allowance) -- on at most 2 % of the elements of the row."""
    d = LinearData.get(row)
    M, N, K, act = row
    img = run_linear_out(dev, d)
    got = image1_to_bits(img, M, N)[:M].view(torch.bfloat16).float()
    _, out, bound = d.model(True)
    ok, used = boundary_allowance(got, out, bound)
    frac = float(used.double().mean())
    one_step = (got.double() - r16_of_float64(out)).abs() <= torch.maximum(_bf16_step(out), _bf16_step(got.double())) * 1.0000001
    print("[beats bf16] %s sed_linear_tiles_out_bf16x1 %s: %d wrong, boundary allowance used on %.3f %% of the elements (%d of them by more "
          "than one bf16 step, largest |out| there %.2e)" % (dev, row, int((~ok).sum()), 100 * frac, int((used & ~one_step).sum()),
                                                             float(out[used & ~one_step].abs().max()) if bool((used & ~one_step).any()) else 0.0))
    assert not bool((used & ~one_step & (out.abs() > 1e-4)).any()), "more than one bf16 step away outside GELU's far tail"
    assert bool(ok.all()), "%s: %d elements are not r16(act(pre))" % (row, int((~ok).sum()))
    assert frac <= max_fraction, (row, frac)


def case_linear_bit_equal(dev, row):
    """On operands that are bf16 values already, every fp32-output run equals its three-product twin bit for bit, and the x1 output image is
    the re-tiled hi plane of the x3 output image."""
    d = LinearData.get(row, rounded=True)
    M, N, K, act = row
    one, three = run_linear_entries(dev, d, "_bf16x1"), run_linear_entries(dev, d, "_bf16x3")
    assert set(one) == set(three) and len(one) >= 5
    for name in one:
        assert torch.equal(one[name], three[name]), "%s %s: differs from the three-product twin on bf16 operands (%d elements)" % (
            row, name, int((one[name] != three[name]).sum()))
    img1, img3 = run_linear_out(dev, d, "_bf16x1"), run_linear_out(dev, d, "_bf16x3")
    assert torch.equal(img1, bits_to_image1(image3_hi_bits(img3, M, N))), "%s: output image is not the re-tiled hi plane of the x3 image" % (row,)


DISCRIMINATION_ROWS = LINEAR_SHAPES + ((64, 256, 768, 0), (64, 256, 3072, 1))          # + the extractor's two K depths


def case_linear_discrimination(min_fraction=0.25):
    """No kernel: the float64 product of the UNROUNDED operands leaves the bound on >= a quarter of the elements of every row."""
    for row in DISCRIMINATION_ROWS:
        d = LinearData.get(row)
        _, out, bound = d.model(True)
        _, out_u, _ = d.model(True, rnd=False)
        frac = float(((out_u - out).abs() > bound).double().mean())
        print("[beats bf16] discrimination %s: %.1f %% of the elements outside the bound" % (row, 100 * frac))
        assert frac >= min_fraction, "%s: the unrounded model is outside the bound in only %.1f %% of the elements" % (row, 100 * frac)


def case_linear_plain_fp32_chain_is_inside():
    """No kernel: a plain fp32 product of the rounded operands (nothing from the library) sits well inside the bounds."""
    for row in DISCRIMINATION_ROWS:
        d = LinearData.get(row)
        _, out, bound = d.model(True)
        pre32 = r16(d.A) @ r16(d.W).t() + d.bias
        got = TF.gelu(pre32) if row[3] else pre32
        ratio = float(((got.double() - out).abs() / bound).max())
        assert ratio <= 0.5, (row, ratio)


# ---- 7. position convolution ----------------------------------------------------------------------------------------------------------
def posconv_problem(rounded=False, B=2, T=100, groups=2, K=128):
    torch.manual_seed(5)
    CG = 48
    D = CG * groups
    x = torch.randn(B, T, D) * 0.8
    w = torch.randn(D, CG, K) / np.sqrt(CG * K) * 3.0                   # Conv1d weight (out, in / groups, k)
    bias = torch.randn(D) * 0.1
    if rounded:
        x, w = r16(x), r16(w)
    return x, w, bias, (B, T, D, K, groups)


def run_posconv(dev, x, w, bias, dims, sfx):
    B, T, D, K, groups = dims
    CG = D // groups
    wt = w.view(groups, CG, CG, K).permute(0, 3, 1, 2).contiguous()        # (groups, K, co, ci)
    w_hi = wt.to(torch.bfloat16)
    if sfx == "_bf16x1":
        planes = w_hi.contiguous().view(torch.int16)
    else:
        planes = torch.stack((w_hi, (wt - w_hi.float()).to(torch.bfloat16))).contiguous().view(torch.int16)
    xd, pd, bd = to(dev, x, planes, bias)
    y = C.Frame(dev, B * T, D)
    _lib.get().call("sed_posconv" + sfx, xd.data_ptr(), pd.data_ptr(), bd.data_ptr(), y.ptr(), B, T, D, K, groups, C.stream(dev))
    C.sync(dev)
    y.assert_frame("sed_posconv" + sfx)
    return y.get().view(B, T, D)


def case_posconv(dev):
    x, w, bias, dims = posconv_problem()
    B, T, D, K, groups = dims
    conv = TF.conv1d(r16(x).double().transpose(1, 2), r16(w).double(), bias.double(), padding=K // 2, groups=groups)[:, :, :T].transpose(1, 2)
    S = TF.conv1d(r16(x).double().abs().transpose(1, 2), r16(w).double().abs(), bias.double().abs(), padding=K // 2, groups=groups)[:, :, :T].transpose(1, 2)
    g = gelu64(conv)
    ref = x.double() + g
    bound = 1.13 * BETA * C.tier_b_unit(K * 48, S) + 8 * U24 * (1.0 + g.abs())
    got = run_posconv(dev, x, w, bias, dims, "_bf16x1")
    _check(dev, "sed_posconv_bf16x1 B=%d T=%d groups=%d K=%d" % (B, T, groups, K), got, ref, bound)
    # discrimination (no kernel): the unrounded convolution leaves this bound on most elements
    conv_u = TF.conv1d(x.double().transpose(1, 2), w.double(), bias.double(), padding=K // 2, groups=groups)[:, :, :T].transpose(1, 2)
    assert float(((x.double() + gelu64(conv_u) - ref).abs() > bound).double().mean()) >= 0.25


def case_posconv_bit_equal(dev):
    x, w, bias, dims = posconv_problem(rounded=True)
    one, three = run_posconv(dev, x, w, bias, dims, "_bf16x1"), run_posconv(dev, x, w, bias, dims, "_bf16x3")
    assert torch.equal(one, three), "sed_posconv_bf16x1 differs from sed_posconv_bf16x3 on bf16 operands (%d elements)" % int((one != three).sum())


# ---- 8. attention ---------------------------------------------------------------------------------------------------------------------
def case_attention(dev, B, T, H, bias):
    """gated = bias: the float64 model with r16(q * fp32(scale log2 e)), r16(k), r16(v) and exact probabilities; bias and gate (on the
    unrounded q) as in parity_cases.case_attention_relpos.  Bound 2^-8 sum_s p_s |v_s| + 2e-5 max(1, |ref|max): pins correctness, does not
    tell one product from three (P's rounding dominates) -- that evidence is the MFMA count in the ISA, profiles/bf16_beats.md."""
    gated = bias
    torch.manual_seed(3)
    hd, D = 64, 64 * H
    qkv = torch.randn(B * T, 3 * D) * 0.7
    relb = torch.randn(H, 2 * T - 1) * 0.5 if bias else None
    gw, gb, ga = (torch.randn(8, hd) * 0.2, torch.randn(8) * 0.1, torch.randn(H) * 0.5 + 1.0) if gated else (None, None, None)
    heads = lambda t: t.view(B, T, H, hd).permute(0, 2, 1, 3)                               # noqa: E731
    qf, kf, vf = heads(qkv[:, :D]), heads(qkv[:, D:2 * D]), heads(qkv[:, 2 * D:])
    qs = torch.tensor(1.44269504088896341, dtype=torch.float32) * torch.tensor(0.125, dtype=torch.float32)      # fp32(scale log2 e)
    q2 = r16(qf * qs).double()                                                              # fp32 product, rounded once
    k, v = r16(kf).double(), r16(vf).double()
    sc = (q2 @ k.transpose(-1, -2)) * math.log(2.0)                                         # base-2 scores back in natural units
    if bias:
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1                   # [t][s] -> s - t + T - 1
        bm = relb.double()[:, idx]                                                          # (H, T, T)
        gate = torch.ones(B, H, T, dtype=torch.float64)
        if gated:
            proj = qf.double() @ gw.double().t() + gb.double()                              # (B, H, T, 8), on the unrounded q
            g_a, g_b = torch.sigmoid(proj[..., :4].sum(-1)), torch.sigmoid(proj[..., 4:].sum(-1))
            gate = g_a * (g_b * ga.double()[None, :, None] - 1.0) + 2.0
        sc = sc + gate[..., None] * bm[None]
    p = torch.softmax(sc, -1)
    unheads = lambda t: t.permute(0, 2, 1, 3).reshape(B * T, D)                             # noqa: E731
    ref = unheads(p @ v)
    bound = 2.0 ** -8 * unheads(p @ v.abs()) + 2e-5 * max(1.0, ref.abs().max().item())
    out = C.Frame(dev, B * T, D)
    qd = to(dev, qkv)
    dv = [to(dev, t) if t is not None else None for t in (relb, gw, gb, ga)]
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    _lib.get().call("sed_attention_relpos_bf16x1", qd.data_ptr(), ptr(dv[0]), ptr(dv[1]), ptr(dv[2]), ptr(dv[3]), out.ptr(), B, T, H, hd, C.stream(dev))
    C.sync(dev)
    out.assert_frame("sed_attention_relpos_bf16x1")
    _check(dev, "sed_attention_relpos_bf16x1 B=%d T=%d H=%d bias=%s" % (B, T, H, bias), out.get(), ref, bound)
    assert C.rc("sed_attention_relpos_bf16x1", qd.data_ptr(), None, None, None, None, out.ptr(), B, T, H, 32, C.stream(dev)) == C.SED_ERR_UNSUPPORTED


# ---- 9. the extractor against the reference fixtures --------------------------------------------------------------------------------------
class _RoundOperands(torch.overrides.TorchFunctionMode):
    """Rounds both operands of every F.linear (except the 8-output grep_linear), F.conv1d, F.conv2d and matrix product once to bf16."""

    def __init__(self):
        super().__init__()
        self.count = {"linear": 0, "conv": 0, "matmul": 0, "gate": 0}

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is TF.linear:
            if args[1].shape[0] == 8:
                self.count["gate"] += 1
            else:
                self.count["linear"] += 1
                args = (r16(args[0]), r16(args[1])) + tuple(args[2:])
        elif func in (TF.conv1d, TF.conv2d):
            self.count["conv"] += 1
            args = (r16(args[0]), r16(args[1])) + tuple(args[2:])
        elif func in (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__, torch.bmm):
            self.count["matmul"] += 1
            args = (r16(args[0]), r16(args[1])) + tuple(args[2:])
        return func(*args, **kwargs)


_ORACLE = {}


def rounded_oracle(which):
    """The oracle's beats_forward with rounded contraction operands (the yardstick of the mode), computed once per fixture:
    (features, audio, cfg, sd)."""
    if which not in _ORACLE:
        from oracle import beats_oracle as BO
        from oracle import sed_oracle as O
        if which == 2:
            G = np.load(os.path.join(GOLDEN, "golden_beats.npz"))
            cfg = dict(BO.BEATS_ITER3_CFG, encoder_layers=int(G["cfg_layers"][0]))
            sd = BO.make_beats_state_dict(cfg, seed=3)
            audio = O.synth_audio(2, 400 + 255 * 160, seed=21)
        else:
            G = np.load(os.path.join(GOLDEN, "golden_beats12.npz"))
            cfg = dict(BO.BEATS_ITER3_CFG)
            sd = BO.make_beats_state_dict(cfg, seed=5)
            audio = O.synth_audio(1, 160000, seed=23)
        with torch.no_grad():
            fb = BO.beats_preprocess(audio)                       # (outside the mode: the fbank is not under it)
            mode = _RoundOperands()
            with mode:
                feats = BO.beats_forward(sd, cfg, fb)
        L = cfg["encoder_layers"]
        assert mode.count == {"linear": 1 + 6 * L, "conv": 2, "matmul": 2 * L, "gate": L}, mode.count
        _ORACLE[which] = (feats.numpy(), audio, cfg, sd, G)
    return _ORACLE[which]


def _distance(which, feats, G):
    """(max, rms, scale) of the distance of (B, T, 768) features from the fixture (the 12-layer fixture holds two strided views)."""
    if which == 2:
        ref = G["features"]
        d = feats - ref
        return float(np.abs(d).max()), float(np.sqrt((d.astype(np.float64) ** 2).mean())), max(1.0, float(np.abs(ref).max()))
    d1, d2 = feats[:, :, ::4] - G["features_ch4"], feats[:, ::8, :] - G["features_tok8"]
    both = np.concatenate((d1.reshape(-1), d2.reshape(-1))).astype(np.float64)
    return float(np.abs(both).max()), float(np.sqrt((both ** 2).mean())), max(1.0, float(G["abs_max"][0]))


def case_extractor(dev, which):
    """which = 2: golden_beats.npz (2 layers, 2 clips, 128 tokens); 12: golden_beats12.npz (12 layers, 1 clip, 496 tokens)."""
    from desed_task_amd.beats import BEATs, BEATsConfig
    o_feats, audio, cfg, sd, G = rounded_oracle(which)
    e_max, e_rms, scale = _distance(which, o_feats, G)

    def build():
        m = BEATs(BEATsConfig(cfg))
        m.load_state_dict(sd)
        m = m.to(dev) if dev != "cpu" else m
        return m.eval().set_precision("bf16x3")

    model = build().set_precision("bf16")
    ad = to(dev, audio)
    feats = model.extract_features(ad)[0].cpu().numpy()
    k_max, k_rms, _ = _distance(which, feats, G)
    print("[beats bf16] %s extractor %d layers: rounded oracle vs fixture max %.3e rms %.3e; kernels vs fixture max %.3e rms %.3e (scale %.3f)" % (
        dev, cfg["encoder_layers"], e_max, e_rms, k_max, k_rms, scale))
    STATS[(dev, "extractor%d" % which)] = (e_max, e_rms, k_max, k_rms, scale)
    assert np.isfinite(feats).all()
    assert k_max > 3e-4 * scale, "the mode is not on: the kernels are within the three-product tolerance of the fixture (%.3e)" % k_max
    assert k_max <= 2 * e_max and k_rms <= 2 * e_rms, "kernels vs fixture max %.3e rms %.3e against 2 x the rounded oracle's %.3e / %.3e" % (
        k_max, k_rms, e_max, e_rms)
    # back to the default on the SAME module: the bits of a freshly built default module (no stale copies; the default is untouched)
    again = model.set_precision("bf16x3").extract_features(ad)[0].cpu()
    fresh = build().extract_features(ad)[0].cpu()
    assert torch.equal(again, fresh), "set_precision('bf16x3') after 'bf16' differs from a fresh default module in %d elements" % int((again != fresh).sum())
    d_max, _, _ = _distance(which, fresh.numpy(), G)
    assert d_max < 3e-4 * scale, d_max
    # ... and every derived copy carries its mode: the other mode's keys are still there, none was shared
    keys = [k for k in list(model._packed["linear"]) + list(model._packed) + list(model._relb) if isinstance(k, tuple)]
    assert {k[1] for k in keys if k[0] in ("tiles", "wpos", "images")} == {"bf16", "bf16x3"}, keys


# ---- 10. GPU only: reproducibility of the pipelined Linear at production depth ------------------------------------------------------------
def case_linear_tiles_reproducible(dev, reps=100):
    """M = 23 808; (N, K, act) = (2304, 768, 0) and (768, 3072, 1): `reps` launches of sed_linear_tiles_bf16x1 must each torch.equal the first,
    whose first 512 rows are checked against the model.  Screens for a mis-ordered stage (a rare wrong tile), not a fault hunt."""
    lib = _lib.get()
    g = torch.Generator().manual_seed(13)
    M = 23808
    for (N, K, act) in ((2304, 768, 0), (768, 3072, 1)):
        A, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
        Ad, Wd, bd = to(dev, A, W, bias)
        st = C.stream(dev)
        At = torch.empty(words1(M, K), dtype=torch.int16, device=dev)
        Wt = torch.empty(words1(N, K), dtype=torch.int16, device=dev)
        lib.call("sed_split_tiles_bf16x1", Ad.data_ptr(), At.data_ptr(), M, K, st)
        lib.call("sed_split_tiles_bf16x1", Wd.data_ptr(), Wt.data_ptr(), N, K, st)
        C0 = torch.empty(M, N, device=dev)
        lib.call("sed_linear_tiles_bf16x1", At.data_ptr(), Wt.data_ptr(), bd.data_ptr(), C0.data_ptr(), M, N, K, act, st)
        a, w = r16(A[:512]).double(), r16(W).double()
        pre = a @ w.t() + bias.double()
        S = a.abs() @ w.abs().t() + bias.double().abs()
        if act:
            out = gelu64(pre)
            bound = 1.13 * BETA * C.tier_b_unit(K, S) + 8 * U24 * (1.0 + out.abs())
        else:
            out, bound = pre, BETA * C.tier_b_unit(K, S)
        _check(dev, "sed_linear_tiles_bf16x1 (23808, %d, %d, %d) first 512 rows" % (N, K, act), C0[:512].cpu(), out, bound)
        Cn = torch.empty_like(C0)
        bad = 0
        for _ in range(reps):
            lib.call("sed_linear_tiles_bf16x1", At.data_ptr(), Wt.data_ptr(), bd.data_ptr(), Cn.data_ptr(), M, N, K, act, st)
            bad += int(not torch.equal(Cn, C0))
        C.sync(dev)
        assert bad == 0, (N, K, "launches that differ from the first", bad, "of", reps)
