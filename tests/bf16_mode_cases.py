"""Cases for the single-product "bf16" arithmetic mode (the *_bf16x1 entries of include/sed_hip.h and everything above them).
Device-agnostic like contraction_cases.py / parity_cases.py: dev = "cpu" runs the fiber-emulator build, "cuda" the library on the MI355X.

Contraction entries (GEMMs, 3x3 convolution forward / data gradient / BN-folded data gradient, weight gradient):
  model  = the float64 contraction of A.to(bfloat16) and B.to(bfloat16) (+ bias, + C_in), i.e. both operands rounded once;
  bound  = BETA (sqrt(K) + 2) 2^-24 (|A| . |B| + |bias| + |C_in|) per element, BETA = 2.4 -- the tier-B bound contraction_cases.py derives
           from a plain fp32 reference accumulation: against this model the only error left is the fp32 accumulation;
  frames = every output and scratch buffer sits in a canary frame that must come back intact.
`case_discrimination` shows on the CPU that the bound tells one product from three: with the UNROUNDED operands as the model at least a
quarter of the elements of every table row leave it.

Bit-equality: the single-product instantiations keep the tiling and the k order of the three-product ones, and a three-product entry whose
operands are bf16 values has lo = 0 and adds exact zeros to the same hi*hi chain -- so on pre-rounded operands a *_bf16x1 entry must
torch.equal its *_bf16x3 twin.  (GEMM rows whose slices are summed by float atomics are left out of this check: their twin is not
bit-reproducible against itself.)

BN-folded data gradient: the model forms dy in float64 from dz, y and the statistics and rounds it once.  The kernel forms the same dy in
fp32 (8 roundings: |dy32 - dy64| <= 8 2^-24 istd (|dz| + |m1| + |xhat m2|) =: e_form) and rounds THAT; where dy64 lies within e_form of a
bf16 rounding boundary the two roundings may legitimately differ by one bf16 step.  Those elements (a few per case) add
step(dy) * |W| to the bound of the outputs they reach; every other output keeps the plain bound.
"""
import math

import torch
import torch.nn.functional as TF

from desed_task_amd import _lib
from tests import contraction_cases as C

BETA, U24 = C.BETA, C.U24
CONV_SHAPES = ((16, 32, 64), (32, 64, 32), (64, 128, 16), (128, 128, 8), (128, 128, 2), (128, 128, 1))      # (CIN, COUT, F)
CONV_B, CONV_T = 2, 13
STATS = {}


def r16(t):
    """fp32 -> rounded once to bf16 (round to nearest even), back in fp32."""
    return t.bfloat16().float()


def x1(entry):
    assert entry.endswith("_bf16x3"), entry
    return entry[:-1] + "1"


# ---- 1. the feature exists ----------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("sed_conv_pack_multi_bf16x1", "sed_cnn_prologue_bf16x1", "sed_conv3x3_bf16x1", "sed_conv3x3_bf16x1_bnbwd",
               "sed_conv_wgrad_bf16x1", "sed_gemm_bf16x1", "sed_gemm_pair_bf16x1", "sed_gemm_kcat_bf16x1",
               "sed_gemm_kcat_splitk_bf16x1", "sed_gemm_pair_splitk_bf16x1", "sed_gemm_splitk_bf16x1")


def case_mode_exists(lib_path):
    """CNN(conv_precision="bf16") constructs, gemm_entry names an entry of the library, the header lists the entries, nm -D shows them."""
    import subprocess
    from desed_task_amd import ops
    from desed_task_amd.nnet.CNN import CNN
    from desed_task_amd.nnet.CRNN import CRNN
    cnn = CNN(1, activation="glu", conv_dropout=0.5, kernel_size=[3] * 2, padding=[1] * 2, stride=[1] * 2, nb_filters=[16, 32],
              pooling=[(2, 2), (2, 2)], conv_precision="bf16")
    assert cnn.conv_precision == "bf16"
    protos = _lib.parse_header()
    for pair in (True, False):
        assert ops.gemm_entry({"gemm_precision": "bf16"}, pair=pair) in protos
    assert ops.gemm_entry({"gemm_precision": "bf16"}) == "sed_gemm_pair_bf16x1"
    for name in NEW_ENTRIES:
        assert name in protos, name
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert set(NEW_ENTRIES) <= exported, sorted(set(NEW_ENTRIES) - exported)
    net = CRNN(n_in_channel=1, nclass=10, attention=True, activation="glu", dropout=0.5, n_RNN_cell=128, n_layers_RNN=2,
               kernel_size=[3] * 2, padding=[1] * 2, stride=[1] * 2, nb_filters=[16, 32], pooling=[(2, 2), (2, 2)])
    keys = list(net.state_dict().keys())
    net.set_precision("bf16")
    assert (net.cnn.conv_precision, net.gemm_precision) == ("bf16", "bf16") and list(net.state_dict().keys()) == keys


def case_precision_key():
    """`training.precision` -> mode: 32 / "32" / "32-true" nothing, "bf16" / "bf16-mixed" the mode, 16 / "16" / "16-mixed" / 64 nothing + ONE warning."""
    import warnings
    from desed_task_amd import ops
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert [ops.precision_mode(v) for v in (32, "32", "32-true")] == [None] * 3
        assert [ops.precision_mode(v) for v in ("bf16", "bf16-mixed")] == ["bf16"] * 2
    for v in (16, "16", "16-mixed", 64):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert ops.precision_mode(v) is None
        assert len(w) == 1 and "bf16" in str(w[0].message) and "32" in str(w[0].message), (v, [str(i.message) for i in w])


# ---- 2 / 3. GEMM entries --------------------------------------------------------------------------------------------------------------
def gemm_rows():
    """The split-bf16 rows contraction_cases already has for the six entry families: plain and pair (three layouts, ragged M / N / K,
    atomics, accumulate, the 128-column tile, mixed magnitudes), and every deterministic split-K row -- among them the kcat rows whose
    B operand changes tensors on a slice boundary and INSIDE a slice (160-wide slices over ksplit = 384)."""
    return [r for r in C.table_plain() if r["entry"].endswith("_bf16x3")] + C.table_splitk() + kcat_rows()


def kcat_rows():
    """The plain K-concatenated entry (one slice; no table of contraction_cases holds it: its rows there are the caller-shaped ones): the
    kcat shapes of table_splitk through sed_gemm_kcat_bf16x3 / _bf16x1 -- K crossing ksplit at and between tile boundaries of the walk,
    ragged M / N, padded leading dimensions, mixed magnitudes, ksplit = 32 (the first tile alone comes from B0), K % 32 != 0."""
    kc = "sed_gemm_kcat_bf16x3"
    w = dict(kernel="bf16x3", ntn=2, slices=1, atomic=False)
    return [C.G(kc, 132, 128, 768, 0, 0, ksplit=384, bias=False, pad=(4, 4, 4), want=w),
            C.G(kc, 280, 72, 96, 0, 0, ksplit=64, bias=False, pad=(0, 4, 4), mixed=True, want=w),
            C.G(kc, 36, 40, 1000, 0, 0, ksplit=512, bias=False, want=w),
            C.G(kc, 132, 72, 100, 0, 0, ksplit=32, bias=False, pad=(4, 0, 8), want=w)]


def _round_problem(prob):
    """Make every operand of the problem a bf16 value (frames and host copies alike)."""
    for f in {id(f): f for f, _ in prob.fA + prob.fB}.values():
        m = f.mask.to(f.buf.device)
        f.buf[m] = r16(f.buf[m])
    prob.A = [r16(t) for t in prob.A]
    prob.B = [r16(t) for t in prob.B]
    prob.snap = {k: f.bits() for k, f in prob.inputs.items()}


def _run_gemm(dev, row, prob, mir, entry):
    lib = _lib.get()
    what = C.describe(dict(row, entry=entry))
    prob.new_outputs()
    prob.fill_c("rand" if row["acc"] else ("zero" if mir["atomic"] else "canary"))
    scr = None
    if "splitk" in entry:
        scr = C.vec_frame(dev, int(lib.value("sed_gemm_splitk_scratch_floats", row["M"], row["N"], row["K"], row["split"])))
        scr.fill(3.25)
    args = C.call_args(row, prob.ptrs(), C.stream(dev), scr.ptr() if scr is not None else None)
    lib.call(entry, *args)
    C.sync(dev)
    prob.assert_clean(what, scr)
    return [prob.out(i) for i in range(prob.nb)]


def _gemm_terms(row, prob, i):
    a, b = prob.op(i)
    extra = torch.zeros(row["M"], row["N"], dtype=torch.float64)
    mag = torch.zeros_like(extra)
    if prob.bias[i] is not None:
        extra += prob.bias[i].double()[None, :]
        mag += prob.bias[i].double().abs()[None, :]
    if row["acc"]:
        extra += prob.Cin[i].double()
        mag += prob.Cin[i].double().abs()
    return a, b, extra, mag


def case_gemm_entries(dev, rows=None, first_seed=700):
    for n, row in enumerate(gemm_rows() if rows is None else rows):
        prob = C.Problem(dev, row, first_seed + n)
        mir = C.mirror(row["entry"], row["M"], row["N"], row["K"], row["lda"], row["ldb"], row["ta"], row["tb"], row["split"], row["acc"],
                       prob.aligned())
        C.check_want(row, mir)                      # the twin takes the same tile / slice branch: same dispatch code
        assert mir["kernel"] == "bf16x3", mir
        entry = x1(row["entry"])
        what = C.describe(dict(row, entry=entry))
        outs = _run_gemm(dev, row, prob, mir, entry)
        for i in range(prob.nb):
            a, b, extra, mag = _gemm_terms(row, prob, i)
            model = r16(a).double() @ r16(b).double() + extra
            S = a.abs().double() @ b.abs().double() + mag
            ratio = (outs[i].double() - model).abs() / C.tier_b_unit(row["K"], S).clamp_min(1e-300)
            rmax = float(ratio.max())
            print("[bf16 mode] %s %s problem %d: ratio %.3f (BETA %.2f)" % (dev, what, i, rmax, BETA))
            assert torch.isfinite(outs[i]).all() and rmax <= BETA, "%s problem %d: %d of %d elements above BETA, largest ratio %.3f" % (
                what, i, int((ratio > BETA).sum()), ratio.numel(), rmax)
            STATS[(dev, "gemm")] = max(STATS.get((dev, "gemm"), 0.0), rmax)


def case_gemm_bit_equal(dev, rows=None, first_seed=900):
    """On pre-rounded operands every *_bf16x1 entry returns the bits of its *_bf16x3 twin (tiling and k order were kept)."""
    done = 0
    for n, row in enumerate(gemm_rows() if rows is None else rows):
        prob = C.Problem(dev, row, first_seed + n)
        mir = C.mirror(row["entry"], row["M"], row["N"], row["K"], row["lda"], row["ldb"], row["ta"], row["tb"], row["split"], row["acc"],
                       prob.aligned())
        if mir["atomic"] and mir["slices"] > 1:
            continue                                # float atomics from several slices: the twin does not equal itself run to run
        _round_problem(prob)
        want = _run_gemm(dev, row, prob, mir, row["entry"])
        got = _run_gemm(dev, row, prob, mir, x1(row["entry"]))
        for i in range(prob.nb):
            assert torch.equal(got[i], want[i]), "%s: differs from its three-product twin on bf16 operands (problem %d, %d elements)" % (
                C.describe(row), i, int((got[i] != want[i]).sum()))
        done += 1
    assert done >= 24 or rows is not None, done


def case_gemm_discrimination(min_fraction=0.25):
    """No kernel: the model with the UNROUNDED operands is outside the bound in >= 25 % of the elements of every row."""
    for n, row in enumerate(gemm_rows()):
        a, b = C._host_problem(row, n)
        S = a.abs().double() @ b.abs().double()
        delta = (a.double() @ b.double() - r16(a).double() @ r16(b).double()).abs()
        frac = float((delta > BETA * C.tier_b_unit(row["K"], S)).double().mean())
        assert frac >= min_fraction, "%s: the unrounded model is outside the bound in only %.0f %% of the elements" % (C.describe(row), 100 * frac)


# ---- 2 / 3. convolution entries -----------------------------------------------------------------------------------------------------
class ConvData:
    """Seeded operands of one (CIN, COUT, F) block at B = 2, T = 13 (ragged tiles in T, zero padding on every side) and the float64
    models / magnitude sums of its four contractions.  Built once per shape and shared (host tensors, never modified)."""
    _cache = {}

    @classmethod
    def get(cls, shape, rounded=False):
        key = (shape, rounded)
        if key not in cls._cache:
            cls._cache[key] = cls(shape, rounded)
        return cls._cache[key]

    def __init__(self, shape, rounded):
        CIN, COUT, F = shape
        B, T = CONV_B, CONV_T
        self.dims = (B, T, F, CIN, COUT)
        g = torch.Generator().manual_seed(4000 + CIN + 3 * COUT + 7 * F)
        rnd = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
        self.x = rnd(B, T, F, CIN)
        self.w = rnd(COUT, CIN, 3, 3) / math.sqrt(9 * CIN)
        self.bias = rnd(COUT) * 0.3
        self.dy = rnd(B, T, F, COUT) * 10.0 ** (torch.rand(COUT, generator=g) * 3 - 2)          # gradients: mixed magnitudes per channel
        # BN-folded entry: dz, the saved pre-BN output ybn, mean | invstd, gamma, dgamma, dbeta of the block's COUT channels
        self.dz = rnd(B, T, F, COUT)
        self.ybn = rnd(B, T, F, COUT) * 1.5 + 0.3
        self.stats = torch.cat((rnd(COUT) * 0.3, 0.5 + torch.rand(COUT, generator=g)))
        self.gamma = 1.0 + 0.25 * rnd(COUT)
        n = B * T * F
        self.dgamma = rnd(COUT) * math.sqrt(n)
        self.dbeta = rnd(COUT) * math.sqrt(n)
        if rounded:                                  # bit-equality runs: every contraction operand is a bf16 value; the BN constants are
            self.x, self.w, self.dy, self.dz = r16(self.x), r16(self.w), r16(self.dy), r16(self.dz)   # chosen so that dy = invstd dz exactly
            self.gamma = torch.zeros(COUT)
            self.stats = torch.cat((self.stats[:COUT], 2.0 ** torch.randint(-1, 2, (COUT,), generator=g).float()))
        self.inv_count = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))

    @staticmethod
    def nchw(t):
        return t.permute(0, 3, 1, 2).contiguous().double()

    @staticmethod
    def nhwc(t):
        return t.permute(0, 2, 3, 1).contiguous()

    def fwd_model(self, rnd=True):
        f = r16 if rnd else (lambda t: t)
        y = TF.conv2d(self.nchw(f(self.x)), f(self.w).double(), self.bias.double(), padding=1)
        S = TF.conv2d(self.nchw(self.x).abs(), self.w.double().abs(), self.bias.double().abs(), padding=1)
        return self.nhwc(y), self.nhwc(S), 9 * self.dims[3]

    def dgrad_model(self, dy, rnd=True, w_abs_of=None):
        f = r16 if rnd else (lambda t: t)
        dx = TF.conv_transpose2d(self.nchw(f(dy)), f(self.w).double(), padding=1)
        S = TF.conv_transpose2d(self.nchw(dy).abs(), self.w.double().abs(), padding=1)
        return self.nhwc(dx), self.nhwc(S), 9 * self.dims[4]

    def wgrad_model(self, rnd=True):
        f = r16 if rnd else (lambda t: t)
        B, T, F, CIN, COUT = self.dims
        dw = torch.nn.grad.conv2d_weight(self.nchw(f(self.x)), (COUT, CIN, 3, 3), self.nchw(f(self.dy)), padding=1)
        S = torch.nn.grad.conv2d_weight(self.nchw(self.x).abs(), (COUT, CIN, 3, 3), self.nchw(self.dy).abs(), padding=1)
        return dw, S, B * T * F

    def bn_dy64(self):
        """dy = invstd (dz - m1 - (ybn - mean) invstd m2) in float64 from the fp32 inputs, and the bound e_form of its fp32 formation."""
        COUT = self.dims[4]
        mean, istd = self.stats[:COUT].double(), self.stats[COUT:].double()
        m1 = self.gamma.double() * self.dbeta.double() * self.inv_count
        m2 = self.gamma.double() * self.dgamma.double() * self.inv_count
        t2 = (self.ybn.double() - mean) * istd * m2
        dy = istd * (self.dz.double() - m1 - t2)
        e_form = 8 * U24 * istd * (self.dz.double().abs() + m1.abs() + t2.abs())
        return dy, e_form


def _dev_frame(dev, t):
    """A contiguous (..., C) host tensor as a canary-framed device buffer (rows x C, dense)."""
    rows = t.numel() // t.shape[-1]
    return C.Frame(dev, rows, t.shape[-1]).put(t.reshape(rows, t.shape[-1]))


def _out_frame(dev, rows, cols):
    return C.Frame(dev, rows, cols)


def _vec(dev, t):
    return C.vec_frame(dev, t.numel()).put(t.reshape(1, -1))


def _packs(dev, d, precision):
    from desed_task_amd import ops
    return ops.pack_conv_weights([d.w.to(dev)], True, precision)[0]


def _check(dev, what, got, model, S, K, extra=None):
    assert torch.isfinite(got).all(), what + ": non-finite output"
    bound = BETA * C.tier_b_unit(K, S.double())
    if extra is not None:
        bound = bound + extra
    err = (got.double() - model).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("[bf16 mode] %s %s: |err| / bound max %.3f (K = %d)" % (dev, what, ratio, K))
    assert ratio <= 1.0, "%s: %d of %d elements outside the bound, worst |err| / bound = %.3f" % (what, int((err > bound).sum()), err.numel(), ratio)
    STATS[(dev, "conv")] = max(STATS.get((dev, "conv"), 0.0), ratio)


def conv_supported(shape):
    """The implicit-GEMM convolution kernels (all precisions) are built for F >= 2: at F = 1 the forward / data-gradient entries refuse
    (rc -3) like their twins, and only the weight gradient -- which is built for every power-of-two F -- is compared."""
    return shape[2] >= 2


def run_conv_entries(dev, d, sfx):
    """All four contractions of the block through the entries with suffix `sfx` ("_bf16x1" / "_bf16x3") on framed buffers.
    -> dict of host outputs (fwd, partial, dgrad, bn_dx, bn_dy, bn_dbias, wgrad), or the return codes where the shape is refused."""
    lib = _lib.get()
    B, T, F, CIN, COUT = d.dims
    st = C.stream(dev)
    out = {}
    wf, wd = _packs(dev, d, "bf16" if sfx == "_bf16x1" else "bf16x3")
    fx, fdy = _dev_frame(dev, d.x), _dev_frame(dev, d.dy)
    ins = [fx, fdy]
    npix = B * T * F
    if conv_supported((CIN, COUT, F)):
        fb = _vec(dev, d.bias)
        nblk = int(lib.value("sed_conv_fwd_blocks_bf16", B, T, F, CIN, COUT))
        fy, fpart = _out_frame(dev, npix, COUT), C.vec_frame(dev, 2 * COUT * nblk)
        lib.call("sed_conv3x3" + sfx, fx.ptr(), wf.data_ptr(), fb.ptr(), fy.ptr(), fpart.ptr(), B, T, F, CIN, COUT, st)
        fdx = _out_frame(dev, npix, CIN)
        lib.call("sed_conv3x3" + sfx, fdy.ptr(), wd.data_ptr(), None, fdx.ptr(), None, B, T, F, COUT, CIN, st)
        fdz, fyb = _dev_frame(dev, d.dz), _dev_frame(dev, d.ybn)
        fst, fga, fdg, fdb = _vec(dev, d.stats), _vec(dev, d.gamma), _vec(dev, d.dgamma), _vec(dev, d.dbeta)
        fbx, fby, fbb = _out_frame(dev, npix, CIN), _out_frame(dev, npix, COUT), C.vec_frame(dev, COUT)
        lib.call("sed_conv3x3%s_bnbwd" % sfx, fdz.ptr(), fyb.ptr(), fst.ptr(), fga.ptr(), fdg.ptr(), fdb.ptr(), wd.data_ptr(), fbx.ptr(),
                 fby.ptr(), fbb.ptr(), B, T, F, COUT, CIN, st)
        C.sync(dev)
        for name, f in (("y", fy), ("partial", fpart), ("dx", fdx), ("bn dx", fbx), ("bn dy_out", fby), ("bn dbias", fbb)):
            f.assert_frame("conv%s %s %s" % (sfx, d.dims, name))
        out.update(fwd=fy.get().view(B, T, F, COUT), partial=fpart.get().view(2 * COUT, nblk), dgrad=fdx.get().view(B, T, F, CIN),
                   bn_dx=fbx.get().view(B, T, F, CIN), bn_dy=fby.get().view(B, T, F, COUT), bn_dbias=fbb.get().flatten())
        ins += [fb, fdz, fyb, fst, fga, fdg, fdb]
    else:
        y = torch.empty(npix * COUT, device=dev)
        out["rc_fwd"] = C.rc("sed_conv3x3" + sfx, fx.ptr(), wf.data_ptr(), None, y.data_ptr(), None, B, T, F, CIN, COUT, st)
    nscr = int(lib.value("sed_conv_wgrad_scratch_floats", B, T, F, CIN, COUT))
    fscr, fdw = C.vec_frame(dev, nscr), C.vec_frame(dev, COUT * CIN * 9)
    lib.call("sed_conv_wgrad" + sfx, fx.ptr(), fdy.ptr(), fscr.ptr(), fdw.ptr(), B, T, F, CIN, COUT, st)
    C.sync(dev)
    fscr.assert_frame("wgrad%s %s scratch" % (sfx, d.dims))
    fdw.assert_frame("wgrad%s %s dW" % (sfx, d.dims))
    out["wgrad"] = fdw.get().view(COUT, CIN, 3, 3)
    for f in ins:
        f.assert_frame("conv%s %s: an input frame" % (sfx, d.dims))
    return out


def bf16_step(v):
    """Spacing of the bf16 grid at |v| (float64 tensor), 0 at 0."""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-300)))
    return torch.where(v == 0, torch.zeros_like(v), 2.0 ** (e - 7))


def check_conv_outputs(dev, d, out, tag=""):
    B, T, F, CIN, COUT = d.dims
    what = "conv (%d -> %d, F = %d)%s" % (CIN, COUT, F, tag)
    if "fwd" in out:
        model, S, K = d.fwd_model()
        _check(dev, what + " forward", out["fwd"], model, S, K)
        # the statistics epilogue: per-workgroup sums of y and y^2 over the workgroup's pixels, fp32
        y = out["fwd"].double().reshape(-1, COUT)
        n = y.shape[0]
        sums = out["partial"].double().sum(1)
        assert ((sums[:COUT] - y.sum(0)).abs() <= (n + 2) * U24 * y.abs().sum(0)).all(), what + ": partial sums"
        assert ((sums[COUT:] - (y * y).sum(0)).abs() <= (n + 4) * U24 * (y * y).sum(0)).all(), what + ": partial sums of squares"
        model, S, K = d.dgrad_model(d.dy)
        _check(dev, what + " data gradient", out["dgrad"], model, S, K)
        # BN-folded: dy_out is the fp32 formation; the contraction model rounds the float64 dy once (see the module docstring)
        dy64, e_form = d.bn_dy64()
        assert ((out["bn_dy"].double() - dy64).abs() <= e_form).all(), what + ": dy_out is not the BatchNorm backward of dz"
        assert torch.equal(out["bn_dbias"], torch.zeros(COUT)), what + ": dbias"
        step = bf16_step(dy64)
        q = dy64 / step.clamp_min(1e-300)
        to_mid = ((q - torch.floor(q)) - 0.5).abs() * step
        amb = (to_mid <= e_form) & (step > 0)
        extra = d.nhwc(TF.conv_transpose2d(d.nchw((amb.double() * step).float()), r16(d.w).double().abs(), padding=1))
        print("[bf16 mode] %s: %d of %d formed dy within e_form of a rounding boundary" % (what, int(amb.sum()), amb.numel()))
        # an element is ambiguous with probability ~ 2 e_form / step ~ 2^-12 (|dz| + |m1| + |xhat m2|) istd / |dy|: a few per ten thousand.
        # One per cent would mean the extra term is no longer the exception it is reasoned to be.
        assert float(amb.double().mean()) <= 0.01, what + ": %d of %d formed dy are ambiguous" % (int(amb.sum()), amb.numel())
        dyr = dy64.float()
        model = d.nhwc(TF.conv_transpose2d(d.nchw(r16(dyr)), r16(d.w).double(), padding=1))
        S = d.nhwc(TF.conv_transpose2d(dy64.permute(0, 3, 1, 2).abs(), d.w.double().abs(), padding=1))
        _check(dev, what + " BN-folded data gradient", out["bn_dx"], model, S, 9 * COUT, extra=extra)
    else:
        assert out["rc_fwd"] == C.SED_ERR_UNSUPPORTED, out
    model, S, K = d.wgrad_model()
    _check(dev, what + " weight gradient", out["wgrad"], model, S, K)


class tuning:
    """with tuning(key, value): a kernel tuning override of the bound library for the duration of the block."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        _lib.set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        _lib.set_tuning(self.key, 0)
        return False


def case_conv_entries(dev, shape):
    d = ConvData.get(shape)
    check_conv_outputs(dev, d, run_conv_entries(dev, d, "_bf16x1"))


def case_conv_walks(dev):
    """A persistent workgroup that walks several tiles (convb_tpw = 3 on the single-chunk 16 -> 32 layer: forward, and the 32 -> 16 data
    gradients), a narrow weight-gradient workgroup that owns several tiles (wgrad_cap = 3), and the one-tap wide weight gradient that the
    kernel-row form otherwise shadows at F >= 8 (wgrad_wide = 1)."""
    d = ConvData.get(CONV_SHAPES[0])
    with tuning("convb_tpw", 3):
        check_conv_outputs(dev, d, run_conv_entries(dev, d, "_bf16x1"), " convb_tpw=3")
    with tuning("wgrad_cap", 3):
        check_conv_outputs(dev, d, run_conv_entries(dev, d, "_bf16x1"), " wgrad_cap=3")
    d = ConvData.get(CONV_SHAPES[2])
    with tuning("wgrad_wide", 1):
        check_conv_outputs(dev, d, run_conv_entries(dev, d, "_bf16x1"), " wgrad_wide=1")


def case_conv_bit_equal(dev, shape):
    """Pre-rounded operands (and BatchNorm constants under which the formed dy is a bf16 value: gamma = 0, invstd a power of two): every
    *_bf16x1 output equals its *_bf16x3 twin's bits; on general operands the fp32 dy_out of the two BN-folded entries is the same."""
    d = ConvData.get(shape, rounded=True)
    a, b = run_conv_entries(dev, d, "_bf16x1"), run_conv_entries(dev, d, "_bf16x3")
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("rc"):
            assert a[k] == b[k] == C.SED_ERR_UNSUPPORTED
        else:
            assert torch.equal(a[k], b[k]), "conv %s %s: differs from the three-product twin on bf16 operands (%d elements)" % (
                shape, k, int((a[k] != b[k]).sum()))
    if conv_supported(shape):
        d = ConvData.get(shape)
        a, b = run_conv_entries(dev, d, "_bf16x1"), run_conv_entries(dev, d, "_bf16x3")
        assert torch.equal(a["bn_dy"], b["bn_dy"])
        assert not torch.equal(a["fwd"], b["fwd"])          # (and on general operands the two modes do differ)


def case_conv_discrimination(min_fraction=0.25):
    """No kernel: for every shape and contraction the model on UNROUNDED operands leaves the bound in >= 25 % of the elements."""
    for shape in CONV_SHAPES:
        d = ConvData.get(shape)
        pairs = [("weight gradient", d.wgrad_model(True), d.wgrad_model(False))]
        if conv_supported(shape):
            pairs += [("forward", d.fwd_model(True), d.fwd_model(False)),
                      ("data gradient", d.dgrad_model(d.dy, True), d.dgrad_model(d.dy, False))]
        for name, (m1, S, K), (m0, _, _) in pairs:
            frac = float(((m1 - m0).abs() > BETA * C.tier_b_unit(K, S.double())).double().mean())
            assert frac >= min_fraction, "conv %s %s: the unrounded model is outside the bound in only %.0f %% of the elements" % (shape, name, 100 * frac)


def case_prologue_packs(dev):
    """sed_cnn_prologue_bf16x1 writes the packs of sed_conv_pack_multi_bf16x1 (bit for bit); those are the hi planes of the three-product
    packs, slab by slab, and nothing is written behind them."""
    from desed_task_amd import ops
    g = torch.Generator().manual_seed(5)
    shapes = [(32, 16), (64, 32), (128, 64), (128, 128)]
    ws = [(torch.randn(co, ci, 3, 3, generator=g) * 0.2).to(dev) for co, ci in shapes]
    want = ops.pack_conv_weights(ws, True, "bf16")
    src = torch.randn(1003, generator=g).to(dev)
    dst = torch.full((1003,), float("nan"), device=dev)
    got = ops.pack_conv_weights(ws, True, "bf16", prologue={"copy": (src, dst)})
    three = ops.pack_conv_weights(ws, True, "bf16x3")
    assert torch.equal(dst.cpu(), src.cpu())
    for (gf, gd), (wf, wd), (tf, td), (co, ci) in zip(got, want, three, shapes):
        n = 9 * co * ci                                  # bf16 elements of the hi planes = half of the buffer's 2 n shorts
        for one, ref, full, rows, ck in ((gf, wf, tf, co, _slab_ck(co, ci)), (gd, wd, td, ci, _slab_ck(ci, co))):
            a, r, t = (z.cpu().view(torch.int16)[:2 * n] for z in (one, ref, full))
            assert torch.equal(a[:n], r[:n])
            # three-product slabs are [tap * chunk][hi | lo][rows][CK]: their hi halves, in order, are the single-product slabs
            slabs = t.view(-1, 2, rows * ck)
            assert torch.equal(slabs[:, 0].reshape(-1), a[:n]), (co, ci)


def _slab_ck(cout, cin):
    """convb_ck of csrc/sed_conv_bf16.hip for the forward slabs of a (cin -> cout) convolution."""
    ck = 16 if (cin, cout) in ((64, 128), (128, 64)) else 32
    return min(cin, ck)


# ---- 4 - 6. module and step level ----------------------------------------------------------------------------------------------------
class Recorder:
    """The call recorder of tests/test_emu_contractions.py: every lib.call name issued inside the block."""

    def __enter__(self):
        self.lib, self.names = _lib.get(), []
        self.orig = self.lib.call

        def spy(name, *a):
            a = self.before(name, a) or a
            self.names.append(name)
            return self.orig(name, *a)
        self.lib.call = spy
        return self

    def before(self, name, args):
        """-> replacement argument tuple, or None to pass the arguments on as they are"""
        return None

    def __exit__(self, *exc):
        self.lib.call = self.orig
        return False

    def new_entries(self):
        return sorted({n for n in self.names if "_bf16x1" in n})

    def three_product_contractions(self):
        return sorted({n for n in self.names if "_bf16x3" in n and n.startswith(("sed_conv", "sed_gemm"))})


def _view(ptr, n, dev):
    """n floats at a raw address as a tensor (no copy)."""
    if dev == "cpu":
        import ctypes
        return torch.frombuffer((ctypes.c_float * n).from_address(ptr), dtype=torch.float32)

    class _Span:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Span(), device="cuda")


class RoundInFront(Recorder):
    """The single-product numerics on the THREE-product kernels: every operand of a conv / weight-gradient / K7 GEMM contraction is
    replaced, right before the launch that reads it, by a COPY rounded to bf16 (lo = 0: hi*hi + hi*lo + lo*hi collapses to hi*hi) -- the
    technique of parity_cases.case_b48_forward_vs_oracle(single_bf16=True), extended to the backward contractions and the BiGRU GEMMs.
    The originals stay as they are (layer 0's hidden states, which the fp32 recurrence backward reads, the master weights, dgi), so the
    rounding points are exactly those of the mode.  The copies live until the block ends.  The conv weights are packed before the
    first launch: the caller rounds the master weights of blocks 1.. up front (nothing else reads them during the step)."""

    def __init__(self, dev):
        self.dev, self.keep = dev, []

    def __exit__(self, *exc):
        C.sync(self.dev)
        self.keep = []
        return Recorder.__exit__(self, *exc)

    def _copy(self, ptr, n):
        """-> address of a bf16-rounded copy of the n floats at ptr (16-byte aligned like every torch allocation)"""
        c = r16(_view(ptr, int(n), self.dev))
        self.keep.append(c)
        return c.data_ptr()

    def _mat(self, ptr, rows, cols, ld):
        return self._copy(ptr, (rows - 1) * ld + cols)

    def before(self, name, a):
        a = list(a)
        if name == "sed_conv3x3_bf16x3":
            a[0] = self._copy(a[0], a[5] * a[6] * a[7] * a[8])
        elif name == "sed_conv_wgrad_bf16x3":
            npix = a[4] * a[5] * a[6]
            a[0], a[1] = self._copy(a[0], npix * a[7]), self._copy(a[1], npix * a[8])
        elif name in ("sed_gemm_pair_bf16x3", "sed_gemm_pair_splitk_bf16x3"):
            o = 8 if name == "sed_gemm_pair_bf16x3" else 6
            M, N, K, lda, ldb, _, ta, tb = a[o:o + 8]
            for i in (0, 1):
                a[i] = self._mat(a[i], K if ta else M, M if ta else K, lda)
            for i in (2, 3):
                a[i] = self._mat(a[i], N if tb else K, K if tb else N, ldb)
        elif name in ("sed_gemm_kcat_bf16x3", "sed_gemm_kcat_splitk_bf16x3"):
            M, N, K, ks, lda, ldb = a[4:10]
            a[0] = self._mat(a[0], M, K, lda)
            a[1], a[2] = self._mat(a[1], ks, N, ldb), self._mat(a[2], K - ks, N, ldb)
        elif "_bf16x3" in name and name.startswith(("sed_conv3x3", "sed_gemm")):
            raise AssertionError("RoundInFront does not know " + name)
        else:
            return None
        return tuple(a)


MISSING = object()


class hparams_precision:
    """with hparams_precision(v): every task the parity_cases builders make carries training.precision = v (MISSING: no such key) --
    through hparams only, as a recipe YAML would."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from tests import parity_cases as P
        self.P, self.orig = P, P.recipe_config

        def recipe_config(*a, **k):
            c = self.orig(*a, **k)
            if self.value is not MISSING:
                c["training"]["precision"] = self.value
            return c
        P.recipe_config = recipe_config

    def __exit__(self, *exc):
        self.P.recipe_config = self.orig
        return False


def _seed(dev, s):
    import random
    import numpy as np
    from desed_task_amd import ops
    random.seed(s); np.random.seed(s + 60); torch.manual_seed(s + 60)
    if dev != "cpu":
        torch.cuda.manual_seed(s + 60)
    ops.reseed_dropout()


def case_module_vs_oracle(dev, bs=(4, 4, 8), n_samp=16000 + 1024):
    """One forward + backward of the 16-clip [4,4,8] step of 1 s clips in "bf16" mode against the fp32 oracle (e_new), next to the same
    errors of the three-product kernels with every contraction operand rounded in front of them (e_emul: identical rounding points, only
    the accumulation order may differ -> e_new <= 2 e_emul per output) and of the default split-bf16 path (e_x3: the mode is really on
    when e_new >= 10 e_x3).  -> (e_new, e_emul, e_x3) as {output: error}; posteriors: max abs, gradients: max error / max |reference|."""
    import random
    import numpy as np
    from desed_task_amd import ops
    from desed_task_amd.launcher import StepDriver
    from tests import parity_cases as P
    O = P.O
    torch.set_num_threads(min(32, torch.get_num_threads()))
    B = sum(bs)
    sd = O.make_state_dict(seed=11)
    audio = O.synth_audio(B, n_samp, seed=3)
    labels = O.synth_labels(bs, 10, (1 + n_samp // 256) // 4, seed=9)
    orc = O.OracleTrainer(sd, batch_sizes=bs, lr=1e-3, rampup_len=100)
    random.seed(4); np.random.seed(7); torch.manual_seed(7)
    assert random.random() < 0.5
    cw = np.random.beta(0.2, 0.2); pw = torch.randperm(bs[1]); cs = np.random.beta(0.2, 0.2); ps = torch.randperm(bs[0])
    tot, _ = orc.training_step(audio, labels, mix=dict(c_weak=cw, perm_weak=pw, c_strong=cs, perm_strong=ps))
    ref_grads = orc.optimizer_step(tot)
    ref_post = {k: orc.last[k].clone() for k in ("strong_s", "weak_s", "strong_t", "weak_t")}

    def run(mode):
        with hparams_precision("bf16" if mode == "bf16" else MISSING):
            task = P.build_task(dev, bs, sd, dropout=0.0, specaug=False, rampup=100)
        driver = StepDriver(task, world_size=1)
        fold = ops.BN_BWD_FOLD
        ctx = Recorder()
        if mode == "emul":
            ops.BN_BWD_FOLD = False        # dy as a tensor of its own, so that it can be rounded in front of its two readers
            with torch.no_grad():
                for net in (task.sed_student, task.sed_teacher):
                    for i in range(1, 7):
                        w = getattr(net.cnn.cnn, "conv%d" % i).weight
                        w.copy_(r16(w))
            ctx = RoundInFront(dev)
        try:
            random.seed(4); np.random.seed(7); torch.manual_seed(7)
            with ctx as rec:
                loss = driver.run_step((P.to(dev, audio.clone()), P.to(dev, labels.clone()), None, None), 0)
                C.sync(dev)
        finally:
            ops.BN_BWD_FOLD = fold
        assert math.isfinite(float(loss.detach()))
        if mode == "bf16":
            assert rec.new_entries() and not rec.three_product_contractions(), (rec.new_entries(), rec.three_product_contractions())
        else:
            assert not rec.new_entries()
        err = {}
        for a, name in zip([t.detach().cpu() for t in task.last_outputs], ("strong_s", "weak_s", "strong_t", "weak_t")):
            assert torch.isfinite(a).all(), name
            err[name] = (a - ref_post[name]).abs().max().item()
        params = dict(task.sed_student.named_parameters())
        for k in O.PARAM_KEYS:
            if k.startswith("cnn.cnn.conv") and k.endswith(".bias"):
                continue                   # analytically zero under training-mode BatchNorm
            g, r = params[k].grad.detach().cpu(), ref_grads[k]
            assert torch.isfinite(g).all(), k
            err["d " + k] = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-30)
        return err
    e_new, e_emul, e_x3 = run("bf16"), run("emul"), run("x3")
    post = ("strong_s", "weak_s", "strong_t", "weak_t")
    gmax = lambda e: max(v for k, v in e.items() if k.startswith("d "))                       # noqa: E731
    pmax = lambda e: max(e[k] for k in post)                                                 # noqa: E731
    print("[bf16 mode] %s posterior error vs oracle: bf16 %s | emulated %s | bf16x3 %s" % (
        dev, {k: "%.2e" % e_new[k] for k in post}, {k: "%.2e" % e_emul[k] for k in post}, {k: "%.2e" % e_x3[k] for k in post}))
    print("[bf16 mode] %s largest gradient error / max |grad|: bf16 %.3e | emulated %.3e | bf16x3 %.3e" % (dev, gmax(e_new), gmax(e_emul), gmax(e_x3)))
    for k in e_new:
        print("[bf16 mode]   %-34s bf16 %.3e  emulated %.3e  bf16x3 %.3e" % (k, e_new[k], e_emul[k], e_x3[k]))
        assert e_new[k] <= 2 * e_emul[k], "%s: bf16 mode %.3e, three-product kernels on rounded operands %.3e" % (k, e_new[k], e_emul[k])
    # the mode is really on: per output, an error 10 x that of the split-bf16 path or more.  Left out: the four head tensors (dense,
    # dense_softmax) -- the head's contractions are not under the mode, and the default path's own dense_softmax.bias error is of the
    # size of the mode's
    for k in e_new:
        if k.startswith(("d dense.", "d dense_softmax.")):
            continue
        assert e_new[k] >= 10 * e_x3[k], "%s: bf16 mode %.3e, bf16x3 %.3e: is the mode on?" % (k, e_new[k], e_x3[k])
    return e_new, e_emul, e_x3


def _batches(dev, year, steps, n_samp, te=9):
    from tests import parity_cases as P
    O = P.O
    n_out = (1 + n_samp // 256) // 4
    out = []
    if year == 2023:
        bs = (1, 1, 2)
        for i in range(steps):
            out.append((P.to(dev, O.synth_audio(sum(bs), n_samp, seed=300 + 11 * i)), P.to(dev, O.synth_labels(bs, 10, n_out, seed=20 + i))))
        return out
    bs, nclass = (2, 1, 1, 2, 2), 27
    B, ns = sum(bs), bs[0] + bs[1] + bs[2]
    for i in range(steps):
        labels = (O.lcg_fill((B, nclass, n_out), 50 + i, 0.5, 0.5) < 0.1).float()
        labels[ns:ns + bs[3], :, 1:] = 0.0
        labels[ns + bs[3]:] = 0.0
        valid = torch.zeros(B, nclass, dtype=torch.bool)
        valid[:bs[0], 10:] = True
        valid[bs[0]:, :10] = True
        out.append(tuple(P.to(dev, t) for t in (O.synth_audio(B, n_samp, seed=700 + 13 * i), labels, O.lcg_fill((B, 768, te), 90 + i, 1.0), valid)))
    return out


_RUNS = {}


def run_steps(dev, year, precision, kind="eager", steps=3, n_samp=2048 + 1024, fresh=False):
    """`steps` different batches through a task whose hparams carry training.precision = `precision`, dropout + SpecAugment + mixup
    (+ dropstep, 2024) on.  kind: "eager" (StepDriver), "captured" (GPU: GraphedStepDriver -- one eager step, the capture, replays;
    emulator: every step under graph.DynArgs, the same launches with their arguments read from memory), "pipelined" (StepDriver with
    prefetch "teacher").  -> dict(losses, student, teacher, grads, names); cached per argument tuple unless fresh."""
    from desed_task_amd import graph as G
    from desed_task_amd.launcher import StepDriver
    from tests import parity_cases as P
    key = (dev, year, str(precision), kind, steps, n_samp)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    batches = _batches(dev, year, steps, n_samp)
    with hparams_precision(precision):
        task = P.build_task(dev, (1, 1, 2), P.O.make_state_dict(seed=7), dropout=0.5, specaug=True, rampup=5) if year == 2023 \
            else P.build_task_2024(dev)
    dyn = None
    if kind == "captured" and dev != "cpu":
        driver = G.GraphedStepDriver(task, world_size=1, warmup=1)
    elif kind == "captured":
        driver, dyn = StepDriver(task, world_size=1, ema_side_stream=False), G.DynArgs(dev)
    else:
        driver = StepDriver(task, world_size=1, prefetch="teacher" if kind == "pipelined" else None)
    _seed(dev, 41)
    losses = []
    with Recorder() as rec:
        for step in range(steps):
            b = batches[step]
            nxt = None
            if year == 2023:
                batch = (b[0], b[1].clone(), None, None)
                if kind == "pipelined" and step + 1 < steps:
                    nxt = (batches[step + 1][0], batches[step + 1][1].clone(), None, None)
            else:
                batch = (b[0], b[1].clone(), None, b[2].clone(), b[3])
                if kind == "pipelined" and step + 1 < steps:
                    n = batches[step + 1]
                    nxt = (n[0], n[1].clone(), None, n[2].clone(), n[3])
            if kind == "pipelined":
                loss = driver.run_step(batch, step, next_batch=nxt)
            elif dyn is not None:
                with G.dyn_step(dyn):
                    loss = driver.run_step(batch, step)
            else:
                loss = driver.run_step(batch, step)
            losses.append(float(loss.detach()))
        C.sync(dev)
    out = dict(losses=losses, student=task.sed_student.arena.flat.detach().cpu().clone(),
               teacher=task.sed_teacher.arena.flat.detach().cpu().clone(),
               grads=task.sed_student.arena.flat_grad.detach().cpu().clone(), names=rec.names, mode=task.precision_mode)
    assert all(math.isfinite(v) for v in losses) and torch.isfinite(out["student"]).all() and out["grads"].abs().max().item() > 0
    _RUNS[key] = out
    return out


def assert_same_bits(a, b, what):
    assert a["losses"] == b["losses"], (what, a["losses"], b["losses"])
    for k in ("student", "teacher", "grads"):
        assert torch.equal(a[k], b[k]), "%s: %s differ in %d elements" % (what, k, int((a[k] != b[k]).sum()))


def case_step_bf16(dev, year, steps=3, n_samp=2048 + 1024):
    """training.precision: "bf16" through hparams only: the mode is on for student and teacher, the captured step == the eager step,
    two seeded runs are bit-identical, the pipelined ("teacher") step == the unpipelined one."""
    eager = run_steps(dev, year, "bf16", "eager", steps, n_samp)
    assert eager["mode"] == "bf16"
    used = {n for n in eager["names"] if "_bf16x1" in n}
    want = {"sed_cnn_prologue_bf16x1", "sed_conv3x3_bf16x1", "sed_conv3x3_bf16x1_bnbwd", "sed_conv_wgrad_bf16x1", "sed_gemm_pair_bf16x1",
            "sed_gemm_pair_splitk_bf16x1"} | ({"sed_gemm_bf16x1", "sed_gemm_splitk_bf16x1"} if year == 2024 else set())
    assert want <= used, sorted(want - used)
    assert not [n for n in eager["names"] if "_bf16x3" in n and n.startswith(("sed_conv", "sed_gemm"))]
    assert_same_bits(eager, run_steps(dev, year, "bf16", "eager", steps, n_samp, fresh=True), "%d: two seeded runs" % year)
    assert_same_bits(eager, run_steps(dev, year, "bf16", "captured", steps, n_samp), "%d: captured vs eager" % year)
    assert_same_bits(eager, run_steps(dev, year, "bf16", "pipelined", steps, n_samp), "%d: pipelined vs unpipelined" % year)
    default = run_steps(dev, year, 32, "eager", steps, n_samp)
    assert not torch.equal(eager["student"], default["student"])            # (and the mode does change the arithmetic)


def case_precision_16_warns_and_changes_nothing(dev, year, steps=2, n_samp=2048 + 1024):
    import warnings
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r16_ = run_steps(dev, year, 16, "eager", steps, n_samp, fresh=True)
    msgs = [str(i.message) for i in w if "training.precision" in str(i.message)]
    assert len(msgs) == 1 and "bf16" in msgs[0], msgs
    r32 = run_steps(dev, year, 32, "eager", steps, n_samp)
    assert r16_["mode"] is None and not [n for n in r16_["names"] if "_bf16x1" in n]
    assert_same_bits(r16_, r32, "%d: precision 16 vs 32" % year)


def case_default_untouched(dev, year, steps=2, n_samp=2048 + 1024):
    """precision: 32 and no precision key at all: identical initial state, same batches -> identical bits; neither calls a new entry."""
    a, b = run_steps(dev, year, 32, "eager", steps, n_samp), run_steps(dev, year, MISSING, "eager", steps, n_samp)
    assert a["mode"] is None and b["mode"] is None
    assert_same_bits(a, b, "%d: precision 32 vs no key" % year)
    for r in (a, b):
        assert not [n for n in r["names"] if "_bf16x1" in n]
        assert "sed_conv3x3_bf16x3" in r["names"] and "sed_gemm_pair_bf16x3" in r["names"]


def case_validation_bf16(dev, year, tmp=None, n_samp=16000 * 2 + 1024):
    """A validation step of a task built with training.precision: "bf16" runs student and teacher in the mode (eval forward: the
    single-product convolutions and input projections), with finite losses close to the default mode's."""
    from tests import parity_cases as P
    O = P.O
    logged = {}
    for prec in ("bf16", 32):
        with hparams_precision(prec):
            if year == 2023:
                bs = (1, 1, 2)
                task = P.build_task(dev, bs, O.make_state_dict(seed=7), dropout=0.5, specaug=True, rampup=100)
                task.hparams["data"] = {"weak_folder": "/d/weak", "synth_val_folder": "/d/synth_val"}
                task.hparams["training"].update(val_thresholds=[0.5], median_window=7)
                task.encoder = P._Encoder(["c%d" % i for i in range(10)], audio_len=n_samp / 16000.0)
                task.eval()
                files = ["/d/synth_val/s0.wav", "/d/synth_val/s1.wav", "/d/weak/w0.wav", "/d/weak/w1.wav"]
                audio = O.synth_audio(4, n_samp, seed=21)
                labels = O.synth_labels(bs, 10, (1 + n_samp // 256) // 4, seed=5)
                batch = (P.to(dev, audio), P.to(dev, labels), None, files, None)
                keys = ("val/weak/student/loss_weak", "val/synth/student/loss_strong", "val/weak/teacher/loss_weak", "val/synth/teacher/loss_strong")
            else:
                from tests import eval2024_cases as E
                task = E._task(dev, n_samp)
                files = ["/d/synth_val/s0.wav", "/d/maestro_train/m0.wav", "/d/weak/w0.wav", "/d/weak/w1.wav"]
                task.hparams["data"] = {"weak_folder": "/d/weak", "synth_val_folder": "/d/synth_val/", "real_maestro_train_folder": "/d/maestro_train"}
                batch = E._batch(dev, files, n_samp, 53, seed=41)[4]
                keys = ("val/weak/student/loss_weak", "val/weak/teacher/loss_weak")
        with Recorder() as rec:
            task.validation_step(batch, 0)
            C.sync(dev)
        if prec == "bf16":
            assert task.sed_teacher.cnn.conv_precision == "bf16" and task.sed_teacher.gemm_precision == "bf16"
            assert {"sed_conv3x3_bf16x1", "sed_gemm_pair_bf16x1"} <= set(rec.names) and not rec.three_product_contractions(), sorted(set(rec.names))
        else:
            assert not rec.new_entries()
        logged[prec] = {k: float(task.logged[k]) for k in keys}
        assert all(math.isfinite(v) for v in logged[prec].values()), logged[prec]
    for k in logged[32]:
        # bf16 operands: 2^-9 relative per rounded operand; the BCE of posteriors that move by a few 1e-3 moves by about as much
        # (no "the two differ" check on these scalars: a mean of a few clipped BCE terms can legitimately round to the same fp32 value
        #  in both modes; that the mode is on is what the call recorder above shows)
        assert abs(logged["bf16"][k] - logged[32][k]) <= 2e-2 * max(1.0, abs(logged[32][k])), (k, logged)
