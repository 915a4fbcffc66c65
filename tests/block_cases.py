"""Direct numerical cases for the activation half of the CNN block: sed_glu_fwd / sed_glu_bwd (csrc/sed_glu.hip, every kernel behind the
two dispatches), sed_bn_finalize, sed_bn_bwd_apply, sed_conv0_fwd / sed_conv0_wgrad (csrc/sed_conv.hip), sed_block0_fwd /
sed_block0_bwd (csrc/sed_block0.hip) and the exact-f32 convolution twins sed_conv3x3 / sed_conv_wgrad, each against a float64
restatement on the host.  Device-agnostic like contraction_cases.py: dev = "cpu" on the fiber emulator, "cuda" on the MI355X.

Every operand, output and scratch buffer is a canary frame (contraction_cases.Frame); scratch is framed at exactly the size the library's
own *_scratch_floats / sed_conv_fwd_blocks report.  After a call the canaries are intact and the inputs bit-unchanged.

Models are plain torch in float64 from the fp32 inputs; the backward entries are float64 autograd through the forward formula with
xhat = (y - mean) invstd as the leaf (so that the leaf's gradient IS dz = dL/d xhat).  BatchNorm statistics are INPUTS of these entries:
the BatchNorm backward of block 0 (and of sed_conv0_wgrad with fuse_bn) is the entries' own expression dy = invstd (dz - gamma dbeta / N -
xhat gamma dgamma / N) evaluated in float64, not autograd through a batch-norm with statistics of its own.

Bounds are per element: |got - model| <= c 2^-24 S + C_SPLIT S_split.  S is the model's formula with absolute values in every sum and
product, carried through the epilogue to first order.  A contraction over K terms contributes (sqrt(K) + 2) x the magnitudes that are
summed (tier_b_unit's form: K = C for the gate linear, K = N pixels for the reductions, K = 9 for layer 0's convolution) and, once
each, the error its terms already carry:
    S_xn   = |y| |scale| + |shift|   (forward)         S_xhat = (S_y + |mean|) invstd,  S_xn = |gamma| S_xhat + |beta|   (backward)
    S_lin  = (sqrt(C) + 2) |xn| . |Wg|^T + S_xn . |Wg|^T + |bg|
    S_r    = S_lin s + |lin| s (1 + (1 - s) S_xn)                          s = sigmoid(xn): d s / s = (1 - s) d xn
    S_out  = pool(keep dscale S_r)
    S_dlin = |g| s (1 + (1 - s) S_xn)                                      g = unpooled gout keep dscale / window
    S_e    = |g| s (1 - s) (S_lin + |lin| (2 + S_xn))
    S_dxn  = (sqrt(C) + 2) |dlin| . |Wg| + S_dlin . |Wg| + S_e,   S_dz = |gamma| S_dxn
    S_dbeta  = (sqrt(N) + 2) sum |dxn| + sum S_dxn             S_dgamma = (sqrt(N) + 2) sum |dxn xhat| + sum (S_dxn |xhat| + |dxn| S_xhat)
    S_dbg    = (sqrt(N) + 2) sum |dlin| + sum S_dlin           S_dWg    = (sqrt(N) + 2) |dlin|^T |xn| + S_dlin^T |xn| + |dlin|^T S_xn
    layer 0: S_y = 5 |x| * |W| + |bias| (S_y = |y| where y is an input);  dW = sum_p x_tap dy,  dy = invstd (dz - m1 - xhat m2):
    S_dW   = (sqrt(N) + 2) sum |x_tap| invstd (|dz| + |m1| + |xhat m2|) + sum |x_tap| invstd (S_dz + S_m1 + S_xhat |m2| + |xhat| S_m2),
             S_m1 = |gamma| S_dbeta / N,  S_m2 = |gamma| S_dgamma / N
(with the offset-3 input of block 0 the mean of y is many standard deviations from zero, so S_xhat ~ 100 |xhat|: that is the conditioning of
xhat = (y - mean) invstd in fp32, and everything downstream of the gate inherits it.)
S_split propagates, the same way, what the split-bf16 kernels do at 2^-16: the three contractions xn . Wg^T, dlin . Wg, dlin^T . xn (tier A
of contraction_cases: xn is formed in fp32 on the device, so the exact three-product model is not available), and -- backward only --
xhat itself, which those kernels keep as a bf16 pair hi + lo and form the sigmoid's argument and the dgamma products from.

The constant c of each family is 4 x the largest ratio |m32 - m64| / (2^-24 S) that the SAME formula evaluated by plain fp32 torch (nothing
from the library) shows over the family's rows (all of them: the GPU-only rows too, on one thread), rounded up to two significant digits;
test_emu_blocks.py::test_constants_follow_from_the_fp32_restatement recomputes them and asserts equality.
sed_bn_finalize reduces in double: its bounds are counts of fp32 roundings read off the kernel's expressions (FINALIZE_ROUNDINGS);
sed_bn_bwd_apply uses the e_form bound of bf16_mode_cases.ConvData.bn_dy64 (8 roundings); the exact-f32 convolution twins use
contraction_cases' BETA on the unrounded model.

Measured (seeded operands of the tables; kernel figures are the largest |err| / bound, 1.0 = the bound):
                      fp32 restatement r_ref   c       CPU emulator    MI355X
    glu_fwd                  0.500            2.1         0.302         0.302
    glu_bwd                  1.884            7.6         0.338         0.338
    conv0_fwd                0.683            2.8         0.244         0.244
    conv0_wgrad              0.190            0.77        0.236         0.236
    block0_fwd               0.325            1.4         0.235         0.280     (MI355X: the B = 2, T = 626, F = 128 row)
    block0_bwd               0.191            0.77        0.266         0.168
    bn_finalize         (rounding counts)                 0.967         0.967
    bn_bwd_apply        (e_form)                          0.807         0.807
    conv3x3 / conv_wgrad, exact f32 (BETA)                0.247         0.247
(the exact-f32 MFMA is a k-ordered fmaf chain on both devices: where no atomics or device transcendentals decide, the figures agree.)
The full-length block-0 row (B = 2, T = 626, F = 128, 160 256 pixels) on the MI355X: dW at 4.1e-5 of the bound with centring (median
|err| / |dW| 1.4e-6) and 5.7e-5 without (0.8e-6; block0_nocenter = 1, printed, not asserted): per-workgroup fp32 sums over 16 x 128
pixels and a double reduction leave nothing for the centring to win at this length.
"""
import contextlib
import math
import os
import re

import torch
import torch.nn.functional as TF

from desed_task_amd import _lib
from tests.contraction_cases import (CANARY, CANARY_BITS, C_SPLIT, Frame, SED_ERR_ARG, SED_ERR_UNSUPPORTED, STATS, U24, rc, stream, sync,
                                     tier_b_unit, vec_frame)
from tests.parity_cases import np_keep_mask
from tests import bf16_mode_cases as M
from tests.bf16_mode_cases import ConvData, tuning


SEED = 1234
EPS = 1e-3
MOMENTUM = 0.99
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")

# c per family = 4 x r_ref of the fp32 restatement rounded up to two significant digits (see the docstring); case_constants()
# recomputes them and asserts equality.
C_FAMILY = {"glu_fwd": 2.1, "glu_bwd": 7.6, "conv0_fwd": 2.8, "conv0_wgrad": 0.77, "block0_fwd": 1.4, "block0_bwd": 0.77}

# sed_bn_finalize (bn_finalize_kernel, sed_conv.hip): fp32 roundings per output; the reduction itself is in double.
#   training: mean = (float)m                                   1 on |m|
#             invstd = (float)(1 / sqrt(var + eps))             1 on invstd
#             scale = g * invstd                                invstd 1 + product 1 = 2 on |scale|
#             shift = b - mean * scale                          mean 1 + scale 2 + product 1 = 4 on |mean scale|, subtraction 1 on |shift|
#                                                               <= |b| + 5 |mean scale|
#             running = (1 - mom) * r + mom * new               (1 - mom) 1 + product 1 = 2 on the first term, new 1 + product 1 = 2 on the
#                                                               second, sum 1 on the result <= 3 (|first| + |second|)
#   eval:     mean = running_mean                               0: the same bits
#             invstd = 1 / sqrtf(rv + eps)                      sum 1 (halved by the root) + root 1 + division 1 <= 3
#             scale                                             3 + 1 = 4;   shift <= |b| + 6 |mean scale|
FINALIZE_ROUNDINGS = {"train": dict(mean=1, invstd=1, scale=2, shift_b=1, shift_ms=5, running=3),
                      "eval": dict(mean=0, invstd=3, scale=4, shift_b=1, shift_ms=6, running=0)}


def k_of(K):
    """sqrt(K) + 2: tier_b_unit's factor for a contraction over K terms."""
    return tier_b_unit(K, 1.0) / U24


# ---- small helpers -----------------------------------------------------------------------------------------------------------------
def fmat(dev, t):
    """A contiguous (..., C) host tensor as a framed device buffer (rows x C)."""
    rows = t.numel() // t.shape[-1] if t.numel() else 0
    if rows == 0:
        return Frame(dev, 0, max(int(t.shape[-1]), 4))
    return Frame(dev, rows, t.shape[-1]).put(t.reshape(rows, t.shape[-1]))


def fvec(dev, t):
    return vec_frame(dev, t.numel()).put(t.reshape(1, -1))


def fout(dev, rows, cols):
    return Frame(dev, rows, cols) if rows > 0 else Frame(dev, 0, max(cols, 4))


class Inputs:
    """The input frames (and plain tensors) of one call: bit-unchanged afterwards, canaries intact."""

    def __init__(self, **kw):
        self.items = {k: v for k, v in kw.items() if v is not None}
        self.snap = {k: (v.bits() if isinstance(v, Frame) else v.cpu().clone()) for k, v in self.items.items()}

    def check(self, what):
        for k, v in self.items.items():
            now = v.bits() if isinstance(v, Frame) else v.cpu()
            assert torch.equal(now, self.snap[k]), "%s: input %s changed" % (what, k)


def untouched(frame):
    return bool((frame.buf.cpu().view(torch.int32) == CANARY_BITS).all())


def dropout_args(p):
    return (int(round(p * (1 << 24))) if p > 0 else 0), (float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)) if p > 0 else 1.0)


def keep_scaled(shape, seed, p, dt):
    thr, dscale = dropout_args(p)
    k = np_keep_mask(shape, seed, p) if p > 0 else torch.ones(shape)
    return (k * dscale).to(dt)


def pool(r, PT, PF, mut=None):
    B, T, F, C = r.shape
    To, Fo = T // PT, F // PF
    o = r[:, :To * PT, :Fo * PF].reshape(B, To, PT, Fo, PF, C).sum((2, 4)) * (1.0 / (PT * PF))
    if mut == "divisor" and o.numel():
        scale = torch.ones_like(o)
        scale[-1, -1, -1] = (PT * PF) / (PT * PF - 1.0) if PT * PF > 1 else 2.0
        o = o * scale
    return o


def unpool(g, T, F, PT, PF):
    """(B, To, Fo, C) -> (B, T, F, C): each window's value at every pixel of the window, 0 on the rows / bins the pooling drops."""
    B, To, Fo, C = g.shape
    u = torch.zeros(B, T, F, C, dtype=g.dtype)
    if To and Fo:
        u[:, :To * PT, :Fo * PF] = g[:, :, None, :, None, :].expand(B, To, PT, Fo, PF, C).reshape(B, To * PT, Fo * PF, C)
    return u


def spread(g, C):
    """Per-channel magnitudes over three decades (as ConvData.dy)."""
    return 10.0 ** (torch.rand(C, generator=g) * 3 - 2)


def bn_params(g, C):
    """mean (|.| >= 0.3), invstd in [0.5, 1.5], gamma with negative values and one exact zero, beta up to +- 2."""
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    mean = sign * (0.3 + 0.5 * torch.rand(C, generator=g))
    invstd = 0.5 + torch.rand(C, generator=g)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    gamma[1], gamma[2], gamma[5] = -0.75, 0.0, -1.25
    beta = torch.rand(C, generator=g) * 4 - 2
    beta[0], beta[3] = 2.0, -2.0
    return mean, invstd, gamma, beta


def stats_of(mean, invstd, gamma, beta):
    scale = gamma * invstd
    return torch.cat((mean, invstd, scale, beta - mean * scale))


def ratio_of(got, model, bound):
    """max |got - model| / bound with 0 / 0 = 0 and x / 0 = inf."""
    err = (got.double() - model.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def check(dev, fam, what, got, model, bound):
    assert torch.isfinite(got).all(), what + ": non-finite output"
    assert got.shape == model.shape, (what, got.shape, model.shape)
    r = ratio_of(got, model, bound)
    print("[blocks] %s %s %s: |err| / bound max %.3f" % (dev, fam, what, r))
    err = (got.double() - model.double()).abs()
    assert r <= 1.0, "%s %s: %d of %d elements outside the bound, worst |err| / bound = %.3f" % (
        fam, what, int((err > bound).sum()), err.numel(), r)
    STATS[(dev, fam)] = max(STATS.get((dev, fam), 0.0), r)
    return r


def leaves_bound(model, mutant, bound):
    """Fraction of the elements in which the mutated model leaves the bound around the model."""
    if model.numel() == 0:
        return 0.0
    return float(((mutant.double() - model.double()).abs() > bound).double().mean())


# ---- the GLU chain (shared by the GLU and block-0 families) ---------------------------------------------------------------------------
def bf16_hi_lo(x):
    hi = x.float().bfloat16().float()
    return hi, (x.float() - hi).bfloat16().float()


def glu_out(xn, Wg, bg, ks, PT, PF, mut=None):
    """pool(dropout(Linear(xn) * sigmoid(xn))) in xn's dtype; ks = keep mask * dscale."""
    lin = xn @ Wg.t() + bg
    if mut == "split_product":                           # the xn_lo . Wg_hi product of the split-bf16 gate linear dropped
        xl, wh = bf16_hi_lo(xn.detach())[1], bf16_hi_lo(Wg.detach())[0]
        lin = lin - (xl.to(xn.dtype) @ wh.to(xn.dtype).t())
    return pool(lin * torch.sigmoid(xn) * ks, PT, PF, mut)


def glu_fwd_mags(xn, S_xn, Wg, bg, ks, PT, PF):
    """-> S_out, S_split_out (float64)."""
    C = Wg.shape[0]
    kc = k_of(C)
    lin = xn @ Wg.t() + bg
    s = torch.sigmoid(xn)
    S_lin = kc * (xn.abs() @ Wg.abs().t()) + S_xn @ Wg.abs().t() + bg.abs()
    S_r = S_lin * s + lin.abs() * s * (1 + (1 - s) * S_xn)
    Sp = (xn.abs() @ Wg.abs().t()) * s
    return pool(ks * S_r, PT, PF), pool(ks * Sp, PT, PF)


def glu_backward(xhat, gamma, beta, Wg, bg, ks, gout, PT, PF, mut=None):
    """autograd through out = glu_out(gamma xhat + beta): -> dz (= d / d xhat), dWg, dbg, dgamma, dbeta, in xhat's dtype."""
    leaves = [t.clone().requires_grad_(True) for t in (xhat, gamma, beta, Wg, bg)]
    out = glu_out(leaves[1] * leaves[0] + leaves[2], leaves[3], leaves[4], ks, PT, PF, mut if mut == "divisor" else None)
    if out.numel():
        out.backward(gout.to(out.dtype))
    g = [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]
    return dict(dz=g[0], dgamma=g[1], dbeta=g[2], dWg=g[3], dbg=g[4])


def glu_bwd_mags(xhat, S_xh, gamma, beta, Wg, bg, ks, gout, PT, PF):
    """-> (S, S_split) dicts over dz, dWg, dbg, dgamma, dbeta, and the per-pixel S_dxn (float64)."""
    B, T, F, C = xhat.shape
    N = B * T * F
    kc, kn = k_of(C), k_of(N)
    xn = gamma * xhat + beta
    S_xn = gamma.abs() * S_xh + beta.abs()
    lin = xn @ Wg.t() + bg
    S_lin = kc * (xn.abs() @ Wg.abs().t()) + S_xn @ Wg.abs().t() + bg.abs()
    s = torch.sigmoid(xn)
    gs = unpool(gout.double(), T, F, PT, PF) * ks / (PT * PF)
    g = gs.abs()
    dlin = g * s
    dxn = (gs * s) @ Wg + gs * lin * s * (1 - s)
    S_dlin = g * s * (1 + (1 - s) * S_xn)
    S_e = g * s * (1 - s) * (S_lin + lin.abs() * (2 + S_xn))
    S_dxn = kc * (dlin @ Wg.abs()) + S_dlin @ Wg.abs() + S_e
    # a reduction over the N pixels: (sqrt(N) + 2) on the magnitudes that are summed, the terms' own errors once each
    flat = lambda t: t.reshape(N, C)                                                                  # noqa: E731
    S = dict(dz=gamma.abs() * S_dxn, dbeta=kn * dxn.abs().sum((0, 1, 2)) + S_dxn.sum((0, 1, 2)),
             dgamma=kn * (dxn * xhat).abs().sum((0, 1, 2)) + (S_dxn * xhat.abs() + dxn.abs() * S_xh).sum((0, 1, 2)),
             dbg=kn * dlin.sum((0, 1, 2)) + S_dlin.sum((0, 1, 2)),
             dWg=kn * (flat(dlin).t() @ flat(xn.abs())) + flat(S_dlin).t() @ flat(xn.abs()) + flat(dlin).t() @ flat(S_xn))
    # split-bf16 kernels: the three contractions at C_SPLIT each, and xhat itself kept as a bf16 pair hi + lo (|xhat - hi - lo| <=
    # 2^-16 |xhat|) from which the sigmoid's argument and the dgamma products are formed
    Sp_xn = gamma.abs() * xhat.abs()
    Sp_dlin = g * s * (1 - s) * Sp_xn
    Sp_e = g * s * (1 - s) * (xn.abs() @ Wg.abs().t() + lin.abs() * Sp_xn)
    Sp_dxn = (dlin + Sp_dlin) @ Wg.abs() + Sp_e
    Sp = dict(dz=gamma.abs() * Sp_dxn, dbeta=Sp_dxn.sum((0, 1, 2)), dgamma=((Sp_dxn + dxn.abs()) * xhat.abs()).sum((0, 1, 2)),
              dbg=Sp_dlin.sum((0, 1, 2)),
              dWg=dlin.reshape(N, C).t() @ (Sp_xn + beta.abs()).reshape(N, C) + Sp_dlin.reshape(N, C).t() @ xn.abs().reshape(N, C))
    return S, Sp, dict(dz=gamma.abs() * dxn.abs())


# ---- family 1: sed_glu_fwd / sed_glu_bwd ------------------------------------------------------------------------------------------
class GluData:
    """Seeded operands of one (C, PT, PF, B, T, F) problem and its cached float64 models (host tensors, never modified)."""
    _cache = {}

    @classmethod
    def get(cls, C, PT, PF, B, T, F):
        key = (C, PT, PF, B, T, F)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, C, PT, PF, B, T, F):
        self.key = (C, PT, PF, B, T, F)
        g = torch.Generator().manual_seed(7000 + C + 3 * T + 11 * F + 101 * B)
        self.mean, self.invstd, self.gamma, self.beta = bn_params(g, C)
        self.y = self.mean + torch.randn(B, T, F, C, generator=g) / self.invstd
        self.stats = stats_of(self.mean, self.invstd, self.gamma, self.beta)
        self.Wg = torch.randn(C, C, generator=g) / math.sqrt(C)
        self.bg = torch.randn(C, generator=g) * 0.3
        self.gout = torch.randn(B, T // PT, F // PF, C, generator=g) * spread(g, C)
        self._models = {}

    def ks(self, p, seed, dt=torch.float64):
        C, PT, PF, B, T, F = self.key
        return keep_scaled((B, T, F, C), seed, p, dt)

    def fwd(self, p, seed=SEED, dt=torch.float64, mut=None):
        C, PT, PF, B, T, F = self.key
        scale, shift = self.stats[2 * C:3 * C].to(dt), self.stats[3 * C:].to(dt)
        return glu_out(self.y.to(dt) * scale + shift, self.Wg.to(dt), self.bg.to(dt), self.ks(p, seed, dt), PT, PF, mut)

    def bwd(self, p, seed=SEED, dt=torch.float64, mut=None):
        C, PT, PF, B, T, F = self.key
        xhat = (self.y.to(dt) - self.mean.to(dt)) * self.invstd.to(dt)
        return glu_backward(xhat, self.gamma.to(dt), self.beta.to(dt), self.Wg.to(dt), self.bg.to(dt), self.ks(p, seed, dt),
                            self.gout.to(dt), PT, PF, mut)

    def models(self, p, seed=SEED):
        """-> dict(out, S_out, Sp_out, bwd, S, Sp): the float64 models and magnitude sums at dropout p."""
        k = (p, seed)
        if k not in self._models:
            C, PT, PF, B, T, F = self.key
            d = torch.float64
            ks = self.ks(p, seed)
            scale, shift = self.stats[2 * C:3 * C].to(d), self.stats[3 * C:].to(d)
            xn = self.y.to(d) * scale + shift
            S_out, Sp_out = glu_fwd_mags(xn, self.y.to(d).abs() * scale.abs() + shift.abs(), self.Wg.to(d), self.bg.to(d), ks, PT, PF)
            xhat = (self.y.to(d) - self.mean.to(d)) * self.invstd.to(d)
            S_xh = (self.y.to(d).abs() + self.mean.to(d).abs()) * self.invstd.to(d)
            S, Sp, _ = glu_bwd_mags(xhat, S_xh, self.gamma.to(d), self.beta.to(d), self.Wg.to(d), self.bg.to(d), ks, self.gout, PT, PF)
            self._models[k] = dict(out=self.fwd(p, seed), S_out=S_out, Sp_out=Sp_out, bwd=self.bwd(p, seed), S=S, Sp=Sp,
                                   keep_any=pool((ks > 0).double(), PT, PF) > 0)
        return self._models[k]


def R(C, B, T, F, split=0, cap=0, f128=0, b128=0, p0=False, gpu_only=False):
    PT, PF = (2, 2) if C <= 32 else (1, 2)
    return dict(C=C, PT=PT, PF=PF, B=B, T=T, F=F, split=split, cap=cap, f128=f128, b128=b128, p0=p0, gpu_only=gpu_only)


def glu_rows():
    rows = []
    # glu16: nine pooled rows at (3, 7) -- the last workgroup (four rows) is ragged and the odd T needs the zero-tail launch
    for F in (8, 16):
        rows += [R(16, 3, 7, F, p0=F == 8), R(16, 2, 8, F), R(16, 1, 2, F)]
    # glu16, looped: 8 200 pooled rows = 2 050 workgroups of four: the forward (cap 2 048) gives two workgroups a second iteration, the
    # backward (cap 1 024) every workgroup a second and two of them a third
    rows.append(R(16, 2, 8200, 8, gpu_only=True))
    # the generic fall-back (C = 32 at F = 8 is out of reach of every block-level test: sed_conv3x3 has no 16 -> 32 kernel at F = 8)
    rows += [R(16, 3, 6, 4), R(16, 3, 7, 4, p0=True), R(32, 3, 6, 2), R(32, 3, 7, 2), R(32, 3, 6, 8, p0=True), R(32, 3, 7, 8)]
    # glu32; at T = 7 the kernel zeroes the dropped frame itself, at T = 1 the zero-tail launch does and nothing else runs
    rows += [R(32, 3, 1, 16), R(32, 3, 6, 16, cap=2), R(32, 3, 7, 16, p0=True), R(32, 3, 1, 32, cap=2), R(32, 3, 6, 32), R(32, 3, 7, 32, cap=2)]
    # wide: 624 pixels at (3, 13, 16) -- five 128-row tiles at C = 64, ten 64-row tiles at C = 128, the last one ragged; glu_grid_cap = 3
    # there gives the three workgroups unequal shares (2, 2, 1 / 4, 3, 3 tiles) in every forward and backward instantiation
    # (case_rows_reach_every_kernel asserts it).  78 pixels at (3, 13, 2) and one pixel pair at (1, 1, 2) are a tile or two: no cap.
    for split in (0, 1):
        rows += [R(64, 3, 13, 16, split=split, p0=True), R(64, 3, 13, 16, split=split, cap=3, p0=split == 1), R(64, 3, 13, 2, split=split),
                 R(64, 1, 1, 2, split=split)]
    rows += [R(128, 3, 13, 16), R(128, 3, 13, 16, cap=3, p0=True), R(128, 3, 13, 2), R(128, 1, 1, 2)]
    rows += [R(128, 3, 13, 16, split=1, p0=True), R(128, 3, 13, 16, split=1, cap=3),
             R(128, 3, 13, 16, split=1, cap=3, f128=1, b128=1, p0=True), R(128, 3, 13, 16, split=1, cap=3, f128=3, b128=3),
             R(128, 3, 13, 2, split=1), R(128, 3, 13, 2, split=1, f128=3, b128=1), R(128, 3, 13, 2, split=1, f128=1, b128=3),
             R(128, 1, 1, 2, split=1), R(128, 1, 1, 2, split=1, f128=3, b128=1), R(128, 1, 1, 2, split=1, f128=1, b128=3)]
    return rows


def glu_kernels(row):
    """The kernels sed_glu_fwd / sed_glu_bwd launch for a row, restated from the dispatch conditions of the two host functions
    (sed_glu.hip) -> (forward list, backward list, backward runs the gate linear on the split-bf16 MFMA)."""
    C, PT, PF, B, T, F = (row[k] for k in ("C", "PT", "PF", "B", "T", "F"))
    split, f128, b128 = row["split"], row["f128"], row["b128"]
    fwd, bwd, bsplit = [], [], False
    narrow16 = C == 16 and PT == 2 and PF == 2 and F % 8 == 0
    narrow32 = C == 32 and PT == 2 and PF == 2 and F % 16 == 0
    if narrow16:
        fwd = ["glu16_fwd_kernel"] if B * (T // 2) * (F // 8) > 0 else []
    elif narrow32:
        fwd = ["glu32_fwd_kernel"] if B * (T // 2) > 0 else []
    elif PT == 1 and PF == 2 and C in (64, 128):
        if split and C == 128 and f128 != 1:
            fwd = ["glu128_fwd_c_kernel<%s>" % ("true" if f128 == 3 else "false")]
        else:
            fwd = ["glu_wide_fwd_b_kernel" if split else "glu_wide_fwd_kernel"]
    else:
        fwd = ["glu_fwd_kernel"] if B * (T // PT) * (F // PF) > 0 else []
    if PT == 1 and PF == 2 and C in (64, 128):
        bsplit = bool(split) and not (C == 128 and b128 == 3)
        if bsplit and C == 128 and b128 != 1:
            bwd = ["glu128_bwd_c_kernel"]
        else:
            bwd = ["glu_wide_bwd_b_kernel" if bsplit else "glu_wide_bwd_kernel"]
        bwd.append("glu_bwd_reduce_kernel")
    else:
        if T % PT != 0 and not (narrow32 and T >= 2):
            bwd.append("glu_zero_tail_kernel")
        if narrow16 or narrow32:
            if B * (T // 2) > 0:
                bwd += ["glu16_bwd_kernel" if C == 16 else "glu32_bwd_kernel", "glu_bwd_reduce_kernel"]
        elif B * (T // PT) * (F // PF) > 0:
            bwd.append("glu_bwd_kernel")
    return fwd, bwd, bsplit


def row_tuning(row):
    st = contextlib.ExitStack()
    for key, k in (("glu_grid_cap", "cap"), ("glu_fwd128", "f128"), ("glu_bwd128_split", "b128"), ("block0_nocenter", "nocenter")):
        if row.get(k):
            st.enter_context(tuning(key, row[k]))
    return st


def describe_glu(row):
    return "glu C=%d B=%d T=%d F=%d split=%d cap=%d fwd128=%d bwd128=%d" % tuple(row[k] for k in ("C", "B", "T", "F", "split", "cap", "f128", "b128"))


def call_glu(dev, row, p, seed=SEED, seed_dev=None):
    """sed_glu_fwd + sed_glu_bwd on framed buffers -> dict of host outputs."""
    lib = _lib.get()
    C, PT, PF, B, T, F = (row[k] for k in ("C", "PT", "PF", "B", "T", "F"))
    d = GluData.get(C, PT, PF, B, T, F)
    what = describe_glu(row) + " p=%g" % p
    st = stream(dev)
    thr24, dscale = dropout_args(p)
    fy, fst, fw, fb, fga, fbe, fgo = (fmat(dev, d.y), fvec(dev, d.stats), fmat(dev, d.Wg), fvec(dev, d.bg), fvec(dev, d.gamma),
                                      fvec(dev, d.beta), fmat(dev, d.gout))
    sd = torch.tensor([seed_dev], dtype=torch.int32, device=dev) if seed_dev is not None else None
    ins = Inputs(y=fy, stats=fst, Wg=fw, bg=fb, gamma=fga, beta=fbe, gout=fgo, seed_dev=sd)
    sdp = sd.data_ptr() if sd is not None else None
    npo = B * (T // PT) * (F // PF)
    fo = fout(dev, npo, C)
    fdz = fout(dev, B * T * F, C)
    fdw, fdb, fdg, fdbe = fout(dev, C, C), vec_frame(dev, C), vec_frame(dev, C), vec_frame(dev, C)
    nscr = int(lib.value("sed_glu_bwd_scratch_floats", B, T, F, C, PT, PF))
    fscr = vec_frame(dev, nscr)
    with row_tuning(row):
        lib.call("sed_glu_fwd", fy.ptr(), fst.ptr(), fw.ptr(), fb.ptr(), fo.ptr(), B, T, F, C, PT, PF, seed, thr24, dscale, sdp, row["split"], st)
        lib.call("sed_glu_bwd", fy.ptr(), fst.ptr(), fga.ptr(), fbe.ptr(), fw.ptr(), fb.ptr(), fgo.ptr(), fdz.ptr(), fdw.ptr(), fdb.ptr(),
                 fdg.ptr(), fdbe.ptr(), fscr.ptr() if nscr else None, B, T, F, C, PT, PF, seed, thr24, dscale, sdp, row["split"], st)
        sync(dev)
    for name, f in (("out", fo), ("dz", fdz), ("dWg", fdw), ("dbg", fdb), ("dgamma", fdg), ("dbeta", fdbe), ("scratch", fscr)):
        f.assert_frame(what + ": " + name)
    ins.check(what)
    To, Fo = T // PT, F // PF
    return dict(out=fo.get().view(B, To, Fo, C) if npo else torch.zeros(B, To, Fo, C), dz=fdz.get().view(B, T, F, C), dWg=fdw.get(),
                dbg=fdb.get().flatten(), dgamma=fdg.get().flatten(), dbeta=fdbe.get().flatten())


def check_glu(dev, row, p, got, seed=SEED):
    C, PT, PF, B, T, F = (row[k] for k in ("C", "PT", "PF", "B", "T", "F"))
    m = GluData.get(C, PT, PF, B, T, F).models(p, seed)
    what = describe_glu(row) + " p=%g" % p
    _, _, bsplit = glu_kernels(row)
    cs_f = C_SPLIT if row["split"] and C >= 64 else 0.0
    cs_b = C_SPLIT if bsplit else 0.0
    check(dev, "glu_fwd", what + " out", got["out"], m["out"], C_FAMILY["glu_fwd"] * U24 * m["S_out"] + cs_f * m["Sp_out"])
    # the zero pattern of the pooled output is the mask's: a window is exactly zero iff none of its elements is kept
    assert torch.equal(got["out"] == 0, ~m["keep_any"] | (m["out"] == 0)), what + ": zero pattern of out differs from the keep mask's"
    for k in ("dz", "dWg", "dbg", "dgamma", "dbeta"):
        check(dev, "glu_bwd", what + " " + k, got[k], m["bwd"][k], C_FAMILY["glu_bwd"] * U24 * m["S"][k] + cs_b * m["Sp"][k])


def case_glu(dev, rows=None, gpu_only=False):
    rows = glu_rows() if rows is None else rows
    for row in rows:
        if row["gpu_only"] != gpu_only:
            continue
        for p in ((0.5, 0.0) if row["p0"] else (0.5,)):
            check_glu(dev, row, p, call_glu(dev, row, p))


def case_glu_seed_dev(dev):
    """seed in device memory: the bits of the host-seed form with the summed seed (one row per entry point; both entries run per row)."""
    for row in (R(16, 3, 7, 8), R(128, 3, 13, 16, split=1)):
        a = call_glu(dev, row, 0.5, seed=SEED - 77, seed_dev=77)
        b = call_glu(dev, row, 0.5, seed=SEED)
        for k in ("out", "dz"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), describe_glu(row) + ": seed_dev form differs in " + k
        for k in ("dWg", "dbg", "dgamma", "dbeta"):       # fixed-order reductions on these rows: the same bits too
            assert torch.equal(a[k], b[k]), describe_glu(row) + ": seed_dev form differs in " + k


# ---- family 2: sed_bn_finalize ----------------------------------------------------------------------------------------------------
FINALIZE_ROWS = [(C, nb) for C in (16, 128) for nb in (1, 63, 1024, 1025, 2500)]


class FinalizeData:
    _cache = {}

    @classmethod
    def get(cls, C, nb):
        if (C, nb) not in cls._cache:
            cls._cache[(C, nb)] = cls(C, nb)
        return cls._cache[(C, nb)]

    def __init__(self, C, nb):
        g = torch.Generator().manual_seed(8000 + C + 7 * nb)
        per = 4.0                                                   # pixels per partial
        self.C, self.nb, self.count = C, nb, float(per * nb + 1)     # (count - 1 != count in fp32: 10 001 at most)
        mean, invstd, self.gamma, self.beta = bn_params(g, C)
        var = 1.0 / invstd ** 2
        s1 = per * (mean[:, None] + torch.randn(C, nb, generator=g) * var.sqrt()[:, None] * 0.5)
        s2 = per * ((var + mean ** 2)[:, None] * (1 + 0.2 * torch.rand(C, nb, generator=g))) * self.count / (per * nb)
        # channel 4 is constant: its partials give E[y^2] - m^2 < 0 (sums of squares rounded down by a few ulp)
        v = 0.375
        s1[4] = per * v * self.count / (per * nb)
        s2[4] = per * v * v * self.count / (per * nb) * (1 - 2.0 ** -20)
        self.partial = torch.cat((s1, s2)).float().contiguous()      # [2 C][nb]
        self.rm = torch.randn(C, generator=g) * 0.4
        self.rv = 0.3 + torch.rand(C, generator=g)

    def model(self, training, mut=None):
        """-> float64 dict(stats (4, C), rm, rv) and the bounds dict of the same shapes."""
        C, d = self.C, torch.float64
        mom, eps = float(torch.tensor(MOMENTUM, dtype=torch.float32)), float(torch.tensor(EPS, dtype=torch.float32))
        g, b, rm, rv = self.gamma.to(d), self.beta.to(d), self.rm.to(d), self.rv.to(d)
        R_ = FINALIZE_ROUNDINGS["train" if training else "eval"]
        if training:
            a, q = self.partial.to(d)[:C].sum(1), self.partial.to(d)[C:].sum(1)
            aa, qa = self.partial.to(d)[:C].abs().sum(1), self.partial.to(d)[C:].abs().sum(1)
            m = a / self.count
            var = (q / self.count - m * m).clamp_min(0.0)
            invstd = 1.0 / torch.sqrt(var + eps)
            # the double reduction: any order of nb + 3 additions, the division and the square
            dvar = (self.nb + 6) * 2.0 ** -53 * (qa / self.count + 2 * (aa / self.count) ** 2)
            dm = (self.nb + 2) * 2.0 ** -53 * aa / self.count
            dinv = 0.5 * invstd * dvar / (var + eps) + 2.0 ** -52 * invstd
            unb = var * (self.count / ((self.count if mut == "count" else self.count - 1.0)))
            nrm, nrv = (1 - mom) * rm + mom * m, (1 - mom) * rv + mom * unb
            brm = R_["running"] * U24 * (((1 - mom) * rm).abs() + (mom * m).abs()) + dm
            brv = R_["running"] * U24 * (((1 - mom) * rv).abs() + (mom * unb).abs()) + dvar * 1.01
        else:
            m, invstd = rm, 1.0 / torch.sqrt(rv + eps)
            dm, dinv = torch.zeros(C, dtype=d), torch.zeros(C, dtype=d)
            nrm, nrv, brm, brv = rm, rv, torch.zeros(C, dtype=d), torch.zeros(C, dtype=d)
        sc = g * invstd
        stats = torch.stack((m, invstd, sc, b - m * sc))
        bounds = torch.stack((R_["mean"] * U24 * m.abs() + dm, R_["invstd"] * U24 * invstd + dinv,
                              R_["scale"] * U24 * sc.abs() + g.abs() * dinv,
                              U24 * (R_["shift_b"] * b.abs() + R_["shift_ms"] * (m * sc).abs()) + (m * g).abs() * dinv + sc.abs() * dm))
        return dict(stats=stats, rm=nrm, rv=nrv), dict(stats=bounds, rm=brm, rv=brv)


def call_finalize(dev, d, training, update):
    lib = _lib.get()
    C, nb = d.C, d.nb
    fp, fg, fb = fmat(dev, d.partial), fvec(dev, d.gamma), fvec(dev, d.beta)
    frm, frv, fs = fvec(dev, d.rm), fvec(dev, d.rv), vec_frame(dev, 4 * C)
    ins = Inputs(partial=fp, gamma=fg, beta=fb)
    lib.call("sed_bn_finalize", fp.ptr(), nb, C, d.count, fg.ptr(), fb.ptr(), frm.ptr(), frv.ptr(), MOMENTUM, EPS, fs.ptr(), training, update,
             stream(dev))
    sync(dev)
    what = "bn_finalize C=%d nblocks=%d training=%d update=%d" % (C, nb, training, update)
    for f in (frm, frv, fs):
        f.assert_frame(what)
    ins.check(what)
    return what, dict(stats=fs.get().view(4, C), rm=frm.get().flatten(), rv=frv.get().flatten())


def case_finalize(dev):
    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    for C, nb in FINALIZE_ROWS:
        d = FinalizeData.get(C, nb)
        for training, update in ((1, 1), (1, 0), (0, 0), (0, 1)):
            what, got = call_finalize(dev, d, training, update)
            model, bound = d.model(training)
            check(dev, "bn_finalize", what + " stats", got["stats"], model["stats"], bound["stats"])
            if training and update:
                check(dev, "bn_finalize", what + " running_mean", got["rm"], model["rm"], bound["rm"])
                check(dev, "bn_finalize", what + " running_var", got["rv"], model["rv"], bound["rv"])
            else:                                     # not asked to update (or eval): the running buffers keep their bits
                assert torch.equal(got["rm"], d.rm) and torch.equal(got["rv"], d.rv), what + ": running statistics changed"
            if training:                              # the constant channel: variance clamped at 0
                q, a = d.partial.double()[C + 4].sum() / d.count, d.partial.double()[4].sum() / d.count
                assert float(q - a * a) < 0, "the constant channel's partials no longer give a negative variance"
                assert abs(float(got["stats"][1, 4]) - 1.0 / math.sqrt(eps32)) <= U24 / math.sqrt(eps32), what + ": var < 0 clamp"
            else:
                assert torch.equal(got["stats"][0], d.rm), what + ": eval mean is not the running mean's bits"


# ---- family 3: sed_bn_bwd_apply ---------------------------------------------------------------------------------------------------
def apply_rows(gpu):
    rows = [(C, 3 * (256 // (C // 4)) + 5) for C in (16, 32, 64, 128)]
    if gpu:     # just above the grid cap: 4 096 workgroups of 256 / (C / 4) pixels, a second trip of the grid-stride loop for 13 of them
        rows += [(C, 4096 * (256 // (C // 4)) + 12 * (256 // (C // 4)) + 3) for C in (16, 32, 64, 128)]
    return rows


class ApplyData:
    def __init__(self, C, npix):
        g = torch.Generator().manual_seed(9000 + C + npix % 1000)
        self.C, self.npix = C, npix
        mean, invstd, self.gamma, _ = bn_params(g, C)
        self.stats = torch.cat((mean, invstd))                      # (the kernel reads mean | invstd only)
        self.dz = torch.randn(npix, C, generator=g) * spread(g, C)
        self.ybn = mean + torch.randn(npix, C, generator=g) / invstd
        self.dgamma = torch.randn(C, generator=g) * math.sqrt(npix)
        self.dbeta = torch.randn(C, generator=g) * math.sqrt(npix)
        self.inv_count = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(npix), dtype=torch.float32))
        self.dims = (1, 1, npix, C, C)

    def model(self, training, mut=None):
        C = self.C
        if training:
            dy, e = ConvData.bn_dy64(self)
            return dy, e, torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        istd = self.stats[C:2 * C].double()
        db = istd * self.gamma.double() * self.dbeta.double()
        if mut == "dbias0":
            db = torch.zeros_like(db)
        # eval: dy = invstd * dz, one rounding (e_form with m1 = m2 = 0 allows 8); dbias = invstd * gamma * dbeta, two roundings
        return istd * self.dz.double(), 8 * U24 * istd * self.dz.double().abs(), db, 2 * U24 * (istd * self.gamma.double() * self.dbeta.double()).abs()


def call_apply(dev, d, training):
    lib = _lib.get()
    fy, fdz, fst, fga, fdg, fdb = fmat(dev, d.ybn), fmat(dev, d.dz), fvec(dev, d.stats), fvec(dev, d.gamma), fvec(dev, d.dgamma), fvec(dev, d.dbeta)
    fbias = vec_frame(dev, d.C)
    ins = Inputs(y=fy, stats=fst, gamma=fga, dgamma=fdg, dbeta=fdb)
    lib.call("sed_bn_bwd_apply", fy.ptr(), fdz.ptr(), fst.ptr(), fga.ptr(), fdg.ptr(), fdb.ptr(), fbias.ptr(), d.npix, d.C, training, stream(dev))
    sync(dev)
    what = "bn_bwd_apply C=%d npix=%d training=%d" % (d.C, d.npix, training)
    fdz.assert_frame(what + " dz")
    fbias.assert_frame(what + " dbias")
    ins.check(what)
    return what, fdz.get(), fbias.get().flatten()


def case_apply(dev, gpu=False):
    for C, npix in apply_rows(gpu):
        d = ApplyData(C, npix)
        for training in (1, 0):
            what, dy, dbias = call_apply(dev, d, training)
            m_dy, e_dy, m_db, e_db = d.model(training)
            check(dev, "bn_bwd_apply", what + " dy", dy, m_dy, e_dy)
            if training:
                assert torch.equal(dbias, torch.zeros(C)), what + ": dbias is not exactly zero"
            else:
                check(dev, "bn_bwd_apply", what + " dbias", dbias, m_db, e_db)


def case_apply_equals_folded_entry(dev):
    """At the ConvData shapes the fp32 dy_out of sed_conv3x3_bf16x3_bnbwd is this kernel's output bit for bit (ops.py relies on it)."""
    lib = _lib.get()
    for shape in M.CONV_SHAPES:
        if not M.conv_supported(shape):
            continue
        d = ConvData.get(shape)
        B, T, F, CIN, COUT = d.dims
        folded = M.run_conv_entries(dev, d, "_bf16x3")["bn_dy"]
        fy, fdz, fst, fga, fdg, fdb = fmat(dev, d.ybn), fmat(dev, d.dz), fvec(dev, d.stats), fvec(dev, d.gamma), fvec(dev, d.dgamma), fvec(dev, d.dbeta)
        fbias = vec_frame(dev, COUT)
        lib.call("sed_bn_bwd_apply", fy.ptr(), fdz.ptr(), fst.ptr(), fga.ptr(), fdg.ptr(), fdb.ptr(), fbias.ptr(), B * T * F, COUT, 1, stream(dev))
        sync(dev)
        fdz.assert_frame("bn_bwd_apply at %s" % (shape,))
        assert torch.equal(fdz.get().view(B, T, F, COUT).view(torch.int32), folded.view(torch.int32)), \
            "conv %s: dy_out of the BN-folded data gradient is not sed_bn_bwd_apply's output" % (shape,)


# ---- families 4 and 5: layer 0 -----------------------------------------------------------------------------------------------------
def specaug_bounds(B, T, F, which=0):
    """Per-clip [f0, f1, t0, t1): a band at bin 0 with a time band across the 16-row tile edge, a band up to bin F beside an empty time
    band, a clip without any mask (set 0); an empty frequency band beside a time band, a band up to bin F with a time band across
    the edge, one bin and no time band (set 1)."""
    sets = ([[0, 2, 14, 18], [F - 3, F, 2, 2], [0, 0, 0, 0]], [[2, 2, 1, 4], [F - 2, F, 15, 17], [0, 1, 0, 0]])
    return torch.tensor([sets[which][b % 3] for b in range(B)], dtype=torch.int32)


def specaug_mask(bounds, B, T, F, mut=None):
    m = torch.ones(B, T, F, dtype=torch.float64)
    if bounds is None:
        return m
    f, t = torch.arange(F)[None, :], torch.arange(T)[:, None]
    for b in range(B):
        f0, f1, t0, t1 = (int(v) for v in bounds[0 if mut == "clip0" else b])
        m[b] = (~(((f >= f0) & (f < f1)) | ((t >= t0) & (t < t1)))).double()
    return m


class Layer0Data:
    """Seeded operands of block 0 at (B, T, F): x with a non-zero mean (offset 3, spread 0.2, as scaled log-mel has), per-clip SpecAugment
    bounds, host BatchNorm statistics of the masked convolution's output (float64, rounded once), mixed-magnitude gradients."""
    _cache = {}

    @classmethod
    def get(cls, B, T, F, which=0):
        key = (B, T, F, which)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, B, T, F, which):
        self.dims = (B, T, F)
        C = 16
        g = torch.Generator().manual_seed(6000 + 5 * T + 13 * F + which)
        self.x = 3.0 + 0.2 * torch.randn(B, T, F, generator=g)
        self.bounds = specaug_bounds(B, T, F, which) if which >= 0 else None
        self.W = torch.randn(C, 1, 3, 3, generator=g) / 3.0
        self.bias = torch.randn(C, generator=g) * 0.3
        _, _, self.gamma, self.beta = bn_params(g, C)
        self.Wg = torch.randn(C, C, generator=g) / 4.0
        self.bg = torch.randn(C, generator=g) * 0.3
        self.gout = torch.randn(B, T // 2, F // 2, C, generator=g) * spread(g, C)
        self.dy = torch.randn(B, T, F, C, generator=g) * spread(g, C)
        y = self.conv()
        n = B * T * F
        mean = y.sum((0, 1, 2)) / n
        var = ((y * y).sum((0, 1, 2)) / n - mean * mean).clamp_min(0.0)
        self.mean, self.invstd = mean.float(), (1.0 / torch.sqrt(var + EPS)).float()
        self.stats = stats_of(self.mean, self.invstd, self.gamma, self.beta)
        self.inv_count = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(B), dtype=torch.float32) * float(T) * float(F)))
        self._models = {}

    def xm(self, dt=torch.float64, mut=None):
        B, T, F = self.dims
        return self.x.to(dt) * specaug_mask(self.bounds, B, T, F, mut).to(dt)

    def conv(self, dt=torch.float64, mut=None):
        """y (B, T, F, 16): the K = 9 convolution of the masked input."""
        return TF.conv2d(self.xm(dt, mut)[:, None], self.W.to(dt), self.bias.to(dt), padding=1).permute(0, 2, 3, 1).contiguous()

    def S_y(self):
        return k_of(9) * TF.conv2d(self.xm().abs()[:, None], self.W.double().abs(), None, padding=1).permute(0, 2, 3, 1) + self.bias.double().abs()

    def wgrad(self, dy, dt=torch.float64, mut=None, drop_last=False, drop_t=-1):
        """dW (16, 1, 3, 3) = correlation of the masked input with dy (B, T, F, 16); drop_last: without the last pixel of frame drop_t of
        the last clip (the last pixel of the last, ragged, tile)."""
        B, T, F = self.dims
        dy = dy.to(dt)
        if drop_last:
            dy = dy.clone()
            dy[-1, drop_t, -1] = 0
        return torch.nn.grad.conv2d_weight(self.xm(dt, mut)[:, None], (16, 1, 3, 3), dy.permute(0, 3, 1, 2).contiguous(), padding=1)

    def bn_dy(self, dz, y, dgamma, dbeta, dt=torch.float64, inv_count=None):
        """dy = invstd (dz - m1 - (y - mean) invstd m2) and the magnitude istd (|dz| + |m1| + |t2|).  inv_count: the fp32 1 / (B T F)
        that sed_conv0_wgrad takes (default), or the exact one of sed_block0_bwd, whose final kernel divides by the count in double."""
        mean, istd = self.mean.to(dt), self.invstd.to(dt)
        inv = self.inv_count if inv_count is None else inv_count
        m1 = self.gamma.to(dt) * dbeta.to(dt) * inv
        m2 = self.gamma.to(dt) * dgamma.to(dt) * inv
        t2 = (y.to(dt) - mean) * istd * m2
        return istd * (dz.to(dt) - m1 - t2), istd * (dz.to(dt).abs() + m1.abs() + t2.abs())

    # -- block 0 --
    def block_fwd(self, stats, p, seed=SEED, dt=torch.float64, mut=None):
        B, T, F = self.dims
        C = 16
        ks = keep_scaled((B, T, F, C), seed + (1 if mut == "seed" else 0), p, dt)
        xn = self.conv(dt, mut) * stats[2 * C:3 * C].to(dt) + stats[3 * C:].to(dt)
        return glu_out(xn, self.Wg.to(dt), self.bg.to(dt), ks, 2, 2, mut)

    def block_fwd_mag(self, stats, p, seed=SEED):
        B, T, F = self.dims
        C, d = 16, torch.float64
        ks = keep_scaled((B, T, F, C), seed, p, d)
        scale, shift = stats[2 * C:3 * C].to(d), stats[3 * C:].to(d)
        xn = self.conv() * scale + shift
        S, _ = glu_fwd_mags(xn, self.S_y() * scale.abs() + shift.abs(), self.Wg.to(d), self.bg.to(d), ks, 2, 2)
        return S, pool((ks > 0).double(), 2, 2) > 0

    def block_bwd(self, p, seed=SEED, dt=torch.float64, mut=None):
        B, T, F = self.dims
        C = 16
        ks = keep_scaled((B, T, F, C), seed + (1 if mut == "seed" else 0), p, dt)
        y = self.conv(dt, mut)
        xhat = (y - self.mean.to(dt)) * self.invstd.to(dt)
        g = glu_backward(xhat, self.gamma.to(dt), self.beta.to(dt), self.Wg.to(dt), self.bg.to(dt), ks, self.gout.to(dt), 2, 2, mut)
        dz = g.pop("dz")
        if mut == "dropped_rows" and T % 2:
            dz = dz.clone()
            dz[:, T - 1] = dz[:, T - 2]
        dy, _ = self.bn_dy(dz, y, g["dgamma"], g["dbeta"], dt, inv_count=1.0 / (B * T * F))
        # (last_pixel: the last pixel that has a pooled gradient, i.e. of the last frame the floor pooling keeps)
        g["dW"] = self.wgrad(dy, dt, mut, drop_last=mut == "last_pixel", drop_t=(T // 2) * 2 - 1)
        g["dbias"] = torch.zeros(C, dtype=dt)
        return g

    def block_bwd_mag(self, p, seed=SEED):
        B, T, F = self.dims
        C, d, N = 16, torch.float64, B * T * F
        kn = k_of(N)
        ks = keep_scaled((B, T, F, C), seed, p, d)
        y = self.conv()
        mean, istd, gam = self.mean.to(d), self.invstd.to(d), self.gamma.to(d)
        xhat = (y - mean) * istd
        S_xh = (self.S_y() + mean.abs()) * istd
        S, _, mags = glu_bwd_mags(xhat, S_xh, gam, self.beta.to(d), self.Wg.to(d), self.bg.to(d), ks, self.gout, 2, 2)
        g = self.block_bwd(p, seed)
        m2 = gam * g["dgamma"] / N
        S_m1, S_m2 = gam.abs() * S["dbeta"] / N, gam.abs() * S["dgamma"] / N
        # dW = sum_p x_tap dy: (sqrt(N) + 2) on the magnitudes |x_tap| istd (|dz| + |m1| + |xhat m2|) that are summed, and once the error
        # each dy carries: that of dz, of the two batch means and of xhat
        form = istd * (S["dz"] + S_m1 + S_xh * m2.abs() + xhat.abs() * S_m2)
        _, mag = self.bn_dy(torch.zeros_like(y), y, g["dgamma"], g["dbeta"], inv_count=1.0 / N)
        acc = istd * mags["dz"] + mag
        cw = lambda t: torch.nn.grad.conv2d_weight(self.xm().abs()[:, None], (16, 1, 3, 3), t.permute(0, 3, 1, 2).contiguous(), padding=1)   # noqa: E731
        S = dict(S, dW=kn * cw(acc) + cw(form), dbias=torch.zeros(C, dtype=d))
        S.pop("dz")
        return S

    def block_models(self, p, seed=SEED):
        k = (p, seed)
        if k not in self._models:
            S_out, keep_any = self.block_fwd_mag(self.stats, p, seed)
            self._models[k] = dict(out=self.block_fwd(self.stats, p, seed), S_out=S_out, keep_any=keep_any, bwd=self.block_bwd(p, seed),
                                   S=self.block_bwd_mag(p, seed))
        return self._models[k]


CONV0_ROWS = [(F, T, which) for F in (4, 8, 128) for T, which in ((1, 0), (15, 1), (17, 0), (33, -1))] + [(8, 33, 1), (128, 17, 1)]


def call_conv0(dev, d, with_y=True):
    lib = _lib.get()
    B, T, F = d.dims
    nblk = int(lib.value("sed_conv_fwd_blocks", B, T, F, 1, 16))
    assert nblk == B * ((T + 15) // 16)
    fx, fw, fb = fmat(dev, d.x), fvec(dev, d.W), fvec(dev, d.bias)
    bd = d.bounds.to(dev) if d.bounds is not None else None
    fy, fp = fout(dev, B * T * F, 16), fout(dev, 32, nblk)
    ins = Inputs(x=fx, W=fw, bias=fb, bounds=bd)
    lib.call("sed_conv0_fwd", fx.ptr(), fw.ptr(), fb.ptr(), bd.data_ptr() if bd is not None else None, fy.ptr() if with_y else None, fp.ptr(),
             B, T, F, 16, stream(dev))
    sync(dev)
    what = "conv0 B=%d T=%d F=%d bounds=%s y=%d" % (B, T, F, "none" if bd is None else "per clip", with_y)
    fy.assert_frame(what + " y")
    fp.assert_frame(what + " partial")
    ins.check(what)
    if not with_y:
        assert untouched(fy), what + ": y written"
    return what, fy.get().view(B, T, F, 16), fp.get()


def conv0_stat_bounds(y, by):
    """The partial rows' sums against sum y, sum y^2 of a float64 y known to by: check_conv_outputs' bound + the propagated by."""
    n = y.shape[0]
    return ((n + 2) * U24 * y.abs().sum(0) + by.sum(0), (n + 4) * U24 * (y * y).sum(0) + (2 * y.abs() * by + by * by).sum(0))


def case_conv0_fwd(dev):
    for F, T, which in CONV0_ROWS:
        d = Layer0Data.get(3, T, F, which)
        model, S = d.conv(), d.S_y()
        what, y, part = call_conv0(dev, d)
        bound = C_FAMILY["conv0_fwd"] * U24 * S
        check(dev, "conv0_fwd", what, y, model, bound)
        sums = part.double().sum(1)
        y2 = y.double().reshape(-1, 16)
        b1, b2 = conv0_stat_bounds(y2, torch.zeros_like(y2))
        assert ((sums[:16] - y2.sum(0)).abs() <= b1).all(), what + ": partial sums"
        assert ((sums[16:] - (y2 * y2).sum(0)).abs() <= b2).all(), what + ": partial sums of squares"
        what, _, part0 = call_conv0(dev, d, with_y=False)
        sums = part0.double().sum(1)
        m2 = model.reshape(-1, 16)
        b1, b2 = conv0_stat_bounds(m2, bound.reshape(-1, 16))
        assert ((sums[:16] - m2.sum(0)).abs() <= b1).all(), what + ": partial sums of the y = NULL form"
        assert ((sums[16:] - (m2 * m2).sum(0)).abs() <= b2).all(), what + ": partial sums of squares of the y = NULL form"


def conv0_wgrad_models(d):
    """-> {fuse_bn: (model, bound without c, dy)} for sed_conv0_wgrad; the fused form gets dz = d.dy, y = the float64 conv rounded once."""
    B, T, F = d.dims
    kn = k_of(B * T * F)
    xa = d.xm().abs()[:, None]
    cw = lambda t: torch.nn.grad.conv2d_weight(xa, (16, 1, 3, 3), t.permute(0, 3, 1, 2).contiguous(), padding=1)   # noqa: E731
    out = {0: (d.wgrad(d.dy), kn * cw(d.dy.double().abs()), None)}
    y32 = d.conv().float()
    g = torch.Generator().manual_seed(77 + T + F)
    dgamma, dbeta = torch.randn(16, generator=g) * math.sqrt(B * T * F), torch.randn(16, generator=g) * math.sqrt(B * T * F)
    dy, mag = d.bn_dy(d.dy, y32, dgamma, dbeta)
    out[1] = (d.wgrad(dy), (kn + 8.0 / C_FAMILY["conv0_wgrad"]) * cw(mag), (y32, dgamma, dbeta))
    return out


def case_conv0_wgrad(dev):
    lib = _lib.get()
    for F, T, which in CONV0_ROWS:
        d = Layer0Data.get(3, T, F, which)
        B = 3
        models = conv0_wgrad_models(d)
        for fuse in (0, 1):
            model, S, extra = models[fuse]
            fx, fdy = fmat(dev, d.x), fmat(dev, d.dy)
            bd = d.bounds.to(dev) if d.bounds is not None else None
            fdw, fdb = vec_frame(dev, 144), vec_frame(dev, 16)
            ins = Inputs(x=fx, dyz=fdy, bounds=bd)
            args = [None] * 5
            if fuse:
                y32, dgamma, dbeta = extra
                fr = [fmat(dev, y32), fvec(dev, d.stats), fvec(dev, d.gamma), fvec(dev, dgamma), fvec(dev, dbeta)]
                ins2 = Inputs(y=fr[0], stats=fr[1], gamma=fr[2], dgamma=fr[3], dbeta=fr[4])
                args = [f.ptr() for f in fr]
            lib.call("sed_conv0_wgrad", fx.ptr(), bd.data_ptr() if bd is not None else None, fdy.ptr(), *args, fdw.ptr(), fdb.ptr(), B, T, F, 16,
                     fuse, 1, stream(dev))
            sync(dev)
            what = "conv0_wgrad T=%d F=%d bounds=%d fuse_bn=%d" % (T, F, which, fuse)
            fdw.assert_frame(what + " dW")
            fdb.assert_frame(what + " dbias")
            ins.check(what)
            if fuse:
                ins2.check(what)
                assert torch.equal(fdb.get().flatten(), torch.zeros(16)), what + ": dbias is not zero"
            else:
                assert untouched(fdb), what + ": dbias written without fuse_bn"
            check(dev, "conv0_wgrad", what, fdw.get().view(16, 1, 3, 3), model, C_FAMILY["conv0_wgrad"] * U24 * S)


def B0(F, T, cap=0, nocenter=0, which=0, p0=False, B=3, gpu_only=False):
    return dict(B=B, T=T, F=F, cap=cap, nocenter=nocenter, which=which, p0=p0, gpu_only=gpu_only)


def block0_rows():
    """F x T in full (T = 2 / 15: one tile; 16: one full tile; 17 / 33: a one-row tile behind full ones, and the frame the floor pooling
    drops); glu_grid_cap = 2 and block0_nocenter = 1 go round so that each meets every F and every T; the bounds set (-1: null) and
    p = 0 go round too."""
    rows, i = [], 0
    for F in (8, 16, 128):
        for T in (2, 15, 16, 17, 33):
            rows.append(B0(F, T, cap=(0, 2)[i % 2], nocenter=int(i % 3 == 1), which=(0, 1, -1)[i % 3], p0=i % 4 == 0))
            i += 1
    return rows + [B0(128, 626, B=2, gpu_only=True), B0(128, 626, B=2, nocenter=1, gpu_only=True)]


def describe_b0(row):
    return "block0 B=%d T=%d F=%d cap=%d nocenter=%d bounds=%d" % tuple(row[k] for k in ("B", "T", "F", "cap", "nocenter", "which"))


def call_block0_fwd(dev, d, stats, p, seed=SEED, seed_dev=None):
    lib = _lib.get()
    B, T, F = d.dims
    thr24, dscale = dropout_args(p)
    fx, fw, fb, fst, fwg, fbg = fmat(dev, d.x), fvec(dev, d.W), fvec(dev, d.bias), fvec(dev, stats), fmat(dev, d.Wg), fvec(dev, d.bg)
    bd = d.bounds.to(dev) if d.bounds is not None else None
    sd = torch.tensor([seed_dev], dtype=torch.int32, device=dev) if seed_dev is not None else None
    fo = fout(dev, B * (T // 2) * (F // 2), 16)
    ins = Inputs(x=fx, W=fw, bias=fb, stats=fst, Wg=fwg, bg=fbg, bounds=bd, seed_dev=sd)
    lib.call("sed_block0_fwd", fx.ptr(), fw.ptr(), fb.ptr(), bd.data_ptr() if bd is not None else None, fst.ptr(), fwg.ptr(), fbg.ptr(),
             fo.ptr(), B, T, F, seed, thr24, dscale, sd.data_ptr() if sd is not None else None, stream(dev))
    sync(dev)
    fo.assert_frame("block0_fwd %s out" % (d.dims,))
    ins.check("block0_fwd %s" % (d.dims,))
    return fo.get().view(B, T // 2, F // 2, 16)


def call_block0_bwd(dev, d, p, seed=SEED, seed_dev=None):
    lib = _lib.get()
    B, T, F = d.dims
    thr24, dscale = dropout_args(p)
    fx, fw, fb, fst, fwg, fbg = fmat(dev, d.x), fvec(dev, d.W), fvec(dev, d.bias), fvec(dev, d.stats), fmat(dev, d.Wg), fvec(dev, d.bg)
    fga, fbe, fgo = fvec(dev, d.gamma), fvec(dev, d.beta), fmat(dev, d.gout)
    bd = d.bounds.to(dev) if d.bounds is not None else None
    sd = torch.tensor([seed_dev], dtype=torch.int32, device=dev) if seed_dev is not None else None
    ins = Inputs(x=fx, W=fw, bias=fb, stats=fst, Wg=fwg, bg=fbg, gamma=fga, beta=fbe, gout=fgo, bounds=bd, seed_dev=sd)
    outs = dict(dW=vec_frame(dev, 144), dbias=vec_frame(dev, 16), dgamma=vec_frame(dev, 16), dbeta=vec_frame(dev, 16), dWg=fout(dev, 16, 16),
                dbg=vec_frame(dev, 16))
    nscr = int(lib.value("sed_block0_bwd_scratch_floats", B, T, F))
    fscr = vec_frame(dev, nscr)
    lib.call("sed_block0_bwd", fx.ptr(), fw.ptr(), fb.ptr(), bd.data_ptr() if bd is not None else None, fst.ptr(), fga.ptr(), fbe.ptr(),
             fwg.ptr(), fbg.ptr(), fgo.ptr(), outs["dW"].ptr(), outs["dbias"].ptr(), outs["dgamma"].ptr(), outs["dbeta"].ptr(),
             outs["dWg"].ptr(), outs["dbg"].ptr(), fscr.ptr(), B, T, F, seed, thr24, dscale, sd.data_ptr() if sd is not None else None,
             stream(dev))
    sync(dev)
    what = "block0_bwd %s" % (d.dims,)
    for k, f in outs.items():
        f.assert_frame(what + " " + k)
    fscr.assert_frame(what + " scratch")
    ins.check(what)
    got = {k: f.get() for k, f in outs.items()}
    got["dW"] = got["dW"].view(16, 1, 3, 3)
    for k in ("dbias", "dgamma", "dbeta", "dbg"):
        got[k] = got[k].flatten()
    return got


def unfused_chain(dev, d, p, seed=SEED):
    """sed_conv0_fwd -> sed_bn_finalize (training) -> sed_glu_fwd on plain framed buffers: -> (stats, out)."""
    lib = _lib.get()
    B, T, F = d.dims
    st = stream(dev)
    thr24, dscale = dropout_args(p)
    _, y, part = call_conv0(dev, d)
    nblk = part.shape[1]
    fp, fg, fb = fmat(dev, part), fvec(dev, d.gamma), fvec(dev, d.beta)
    frm, frv, fs = fvec(dev, torch.zeros(16)), fvec(dev, torch.ones(16)), vec_frame(dev, 64)
    lib.call("sed_bn_finalize", fp.ptr(), nblk, 16, float(B * T * F), fg.ptr(), fb.ptr(), frm.ptr(), frv.ptr(), MOMENTUM, EPS, fs.ptr(), 1, 1, st)
    fy, fwg, fbg = fmat(dev, y), fmat(dev, d.Wg), fvec(dev, d.bg)
    fo = fout(dev, B * (T // 2) * (F // 2), 16)
    lib.call("sed_glu_fwd", fy.ptr(), fs.ptr(), fwg.ptr(), fbg.ptr(), fo.ptr(), B, T, F, 16, 2, 2, seed, thr24, dscale, None, 0, st)
    sync(dev)
    fo.assert_frame("unfused chain out")
    return fs.get().flatten(), fo.get().view(B, T // 2, F // 2, 16)


def case_block0(dev, gpu_only=False):
    for row in block0_rows():
        if row["gpu_only"] != gpu_only:
            continue
        d = Layer0Data.get(row["B"], row["T"], row["F"], row["which"])
        what = describe_b0(row)
        for p in ((0.5, 0.0) if row["p0"] else (0.5,)):
            m = d.block_models(p)
            with row_tuning(row):
                out = call_block0_fwd(dev, d, d.stats, p)
                got = call_block0_bwd(dev, d, p)
            if not row["nocenter"] or not row["gpu_only"]:
                check(dev, "block0_fwd", what + " p=%g out" % p, out, m["out"], C_FAMILY["block0_fwd"] * U24 * m["S_out"])
                assert torch.equal(out == 0, ~m["keep_any"] | (m["out"] == 0)), what + ": zero pattern of out differs from the keep mask's"
                for k in ("dW", "dgamma", "dbeta", "dWg", "dbg"):
                    check(dev, "block0_bwd", what + " p=%g %s" % (p, k), got[k], m["bwd"][k], C_FAMILY["block0_bwd"] * U24 * m["S"][k])
            if row["gpu_only"]:     # the full-length rows: dW with and without centring, in figures (the second is printed, not asserted)
                r = ratio_of(got["dW"], m["bwd"]["dW"], C_FAMILY["block0_bwd"] * U24 * m["S"]["dW"])
                rel = float(((got["dW"].double() - m["bwd"]["dW"]).abs() / m["bwd"]["dW"].abs().clamp_min(1e-300)).median())
                print("[blocks] %s %s: dW |err| / bound %.3e, median |err| / |dW| %.3e (%s)" % (
                    dev, what, r, rel, "WITHOUT centring, not asserted" if row["nocenter"] else "centred"))
            assert torch.equal(got["dbias"], torch.zeros(16)), what + ": dbias"


def case_block0_chain_and_eval(dev):
    """(a) the dropout zero pattern of the fused forward is the unfused chain's, and the chain's statistics are the host's within
    family 2's bound + the partials' own; (b) eval: statistics from sed_bn_finalize's eval branch, forward against the model on them;
    (c) the seed_dev forms of the two block-0 entries."""
    for T, F in ((17, 16), (33, 128)):
        d = Layer0Data.get(3, T, F, 0)
        stats_chain, out_chain = unfused_chain(dev, d, 0.5)
        out = call_block0_fwd(dev, d, stats_chain, 0.5)
        assert torch.equal(out == 0, out_chain == 0), "block0 T=%d F=%d: dropout zero pattern differs from the unfused chain's" % (T, F)
        S, _ = d.block_fwd_mag(stats_chain, 0.5)
        model = d.block_fwd(stats_chain, 0.5)
        check(dev, "block0_fwd", "T=%d F=%d on the chain's statistics" % (T, F), out, model, C_FAMILY["block0_fwd"] * U24 * S)
        check(dev, "glu_fwd", "unfused chain T=%d F=%d" % (T, F), out_chain, model, C_FAMILY["block0_fwd"] * U24 * S)
        # mean / invstd of the chain against the host's: fp32 partial sums of n values -> (n + 4) 2^-24 relative on E|y|, E y^2
        n = 3 * T * F
        y = d.conv()
        e1, e2 = (n + 4) * U24 * y.abs().mean((0, 1, 2)), (n + 4) * U24 * (y * y).mean((0, 1, 2))
        mean64 = y.mean((0, 1, 2))
        var64 = (y * y).mean((0, 1, 2)) - mean64 ** 2
        assert ((stats_chain[:16].double() - mean64).abs() <= e1 + U24 * mean64.abs()).all(), "chain mean"
        dvar = e2 + 2 * mean64.abs() * e1
        inv64 = 1 / torch.sqrt(var64 + EPS)
        assert ((stats_chain[16:32].double() - inv64).abs() <= 0.5 * inv64 * dvar / (var64 + EPS) * 1.01 + U24 * inv64).all(), "chain invstd"
        # eval
        lib = _lib.get()
        g = torch.Generator().manual_seed(5)
        rm, rv = d.mean + 0.05 * torch.randn(16, generator=g), 1 / d.invstd ** 2 * (1 + 0.1 * torch.rand(16, generator=g))
        fg, fb, frm, frv, fs = fvec(dev, d.gamma), fvec(dev, d.beta), fvec(dev, rm), fvec(dev, rv), vec_frame(dev, 64)
        lib.call("sed_bn_finalize", None, 0, 16, float(n), fg.ptr(), fb.ptr(), frm.ptr(), frv.ptr(), MOMENTUM, EPS, fs.ptr(), 0, 0, stream(dev))
        sync(dev)
        stats_eval = fs.get().flatten()
        out = call_block0_fwd(dev, d, stats_eval, 0.0)
        S, _ = d.block_fwd_mag(stats_eval, 0.0)
        check(dev, "block0_fwd", "T=%d F=%d eval" % (T, F), out, d.block_fwd(stats_eval, 0.0), C_FAMILY["block0_fwd"] * U24 * S)
    d = Layer0Data.get(3, 17, 16, 0)
    a, b = call_block0_fwd(dev, d, d.stats, 0.5, seed=SEED - 5, seed_dev=5), call_block0_fwd(dev, d, d.stats, 0.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "block0_fwd: seed_dev form"
    a, b = call_block0_bwd(dev, d, 0.5, seed=SEED - 5, seed_dev=5), call_block0_bwd(dev, d, 0.5)
    for k in a:
        assert torch.equal(a[k], b[k]), "block0_bwd: seed_dev form differs in " + k


# ---- family 6: the exact-f32 convolution twins ------------------------------------------------------------------------------------
def case_conv_f32(dev, shape):
    """sed_conv3x3 / sed_conv_wgrad over ConvData with the unrounded float64 model and the exact-f32 bound (tier B, c_split = 0)."""
    lib = _lib.get()
    from desed_task_amd import ops
    d = ConvData.get(shape)
    B, T, F, CIN, COUT = d.dims
    st = stream(dev)
    what = "conv f32 (%d -> %d, F = %d)" % (CIN, COUT, F)
    fx, fdy = fmat(dev, d.x), fmat(dev, d.dy)
    ins = Inputs(x=fx, dy=fdy)
    if M.conv_supported(shape):
        wf, wd = ops.pack_conv_weights([d.w.to(dev)], True, "f32")[0]
        fb = fvec(dev, d.bias)
        nblk = int(lib.value("sed_conv_fwd_blocks", B, T, F, CIN, COUT))
        fy, fpart = fout(dev, B * T * F, COUT), vec_frame(dev, 2 * COUT * nblk)
        lib.call("sed_conv3x3", fx.ptr(), wf.data_ptr(), fb.ptr(), fy.ptr(), fpart.ptr(), B, T, F, CIN, COUT, st)
        fdx = fout(dev, B * T * F, CIN)
        lib.call("sed_conv3x3", fdy.ptr(), wd.data_ptr(), None, fdx.ptr(), None, B, T, F, COUT, CIN, st)
        sync(dev)
        for name, f in (("y", fy), ("partial", fpart), ("dx", fdx)):
            f.assert_frame(what + " " + name)
        model, S, K = d.fwd_model(rnd=False)
        y = fy.get().view(B, T, F, COUT)
        M._check(dev, what + " forward", y, model, S, K)
        y2 = y.double().reshape(-1, COUT)
        sums = fpart.get().view(2 * COUT, nblk).double().sum(1)
        b1, b2 = conv0_stat_bounds(y2, torch.zeros_like(y2))
        assert ((sums[:COUT] - y2.sum(0)).abs() <= b1).all(), what + ": partial sums"
        assert ((sums[COUT:] - (y2 * y2).sum(0)).abs() <= b2).all(), what + ": partial sums of squares"
        model, S, K = d.dgrad_model(d.dy, rnd=False)
        M._check(dev, what + " data gradient", fdx.get().view(B, T, F, CIN), model, S, K)
    else:
        y = torch.empty(B * T * F * COUT, device=dev)
        assert rc("sed_conv3x3", fx.ptr(), fx.ptr(), None, y.data_ptr(), None, B, T, F, CIN, COUT, st) == SED_ERR_UNSUPPORTED
    nscr = int(lib.value("sed_conv_wgrad_scratch_floats", B, T, F, CIN, COUT))
    fscr, fdw = vec_frame(dev, nscr), vec_frame(dev, COUT * CIN * 9)
    lib.call("sed_conv_wgrad", fx.ptr(), fdy.ptr(), fscr.ptr(), fdw.ptr(), B, T, F, CIN, COUT, st)
    sync(dev)
    fscr.assert_frame(what + " wgrad scratch")
    fdw.assert_frame(what + " dW")
    ins.check(what)
    model, S, K = d.wgrad_model(rnd=False)
    M._check(dev, what + " weight gradient", fdw.get().view(COUT, CIN, 3, 3), model, S, K)


# ---- the error contract -----------------------------------------------------------------------------------------------------------
def case_error_contract(dev):
    lib = _lib.get()
    st = stream(dev)
    big = torch.full((1 << 16,), CANARY, device=dev)
    p = big.data_ptr()

    def clean():
        ok = bool((big == CANARY).all())
        big.fill_(CANARY)
        return ok
    # F % PF != 0, unsupported C or pooling: refused before anything is written (T = 3: not even the rows the floor pooling drops)
    for C, PT, PF, F in ((16, 2, 2, 7), (64, 1, 2, 3), (48, 2, 2, 8), (16, 1, 2, 8), (256, 1, 2, 8), (64, 2, 2, 8)):
        for T in (2, 3):
            assert rc("sed_glu_fwd", p, p, p, p, p, 1, T, F, C, PT, PF, 1, 0, 1.0, None, 0, st) == SED_ERR_UNSUPPORTED, (C, PT, PF, F)
            fz = [vec_frame(dev, 1 << 16) for _ in range(5)]
            assert rc("sed_glu_bwd", p, p, p, p, p, p, p, fz[0].ptr(), fz[1].ptr(), fz[2].ptr(), fz[3].ptr(), fz[4].ptr(), None, 1, T, F, C, PT, PF,
                      1, 0, 1.0, None, 0, st) == SED_ERR_UNSUPPORTED, (C, PT, PF, F)
            sync(dev)
            for f in fz:
                assert untouched(f), "refused sed_glu_bwd (C=%d PT=%d PF=%d F=%d T=%d) wrote to an output" % (C, PT, PF, F, T)
    assert clean()
    assert rc("sed_bn_bwd_apply", p, p, p, p, p, p, p, 10, 48, 1, st) == SED_ERR_UNSUPPORTED
    assert rc("sed_bn_finalize", p, 1, 0, 4.0, p, p, p, p, MOMENTUM, EPS, p, 1, 1, st) == SED_ERR_ARG
    assert rc("sed_bn_finalize", p, 1, -3, 4.0, p, p, p, p, MOMENTUM, EPS, p, 1, 1, st) == SED_ERR_ARG
    for F in (0, 4, 12, 136, 256):
        assert rc("sed_block0_fwd", p, p, p, None, p, p, p, p, 1, 4, F, 1, 0, 1.0, None, st) == SED_ERR_UNSUPPORTED, F
        assert rc("sed_block0_bwd", p, p, p, None, p, p, p, p, p, p, p, p, p, p, p, p, p, 1, 4, F, 1, 0, 1.0, None, st) == SED_ERR_UNSUPPORTED, F
    sync(dev)
    assert clean(), "a refused call wrote"
    # null scratch where one is needed
    for C, PT, PF, F in ((16, 2, 2, 8), (32, 2, 2, 16), (64, 1, 2, 2), (128, 1, 2, 2)):
        for split in (0, 1):
            assert rc("sed_glu_bwd", p, p, p, p, p, p, p, p, p, p, p, p, None, 1, 2, F, C, PT, PF, 1, 0, 1.0, None, split, st) == SED_ERR_ARG
    assert rc("sed_block0_bwd", p, p, p, None, p, p, p, p, p, p, p, p, p, p, p, p, None, 1, 4, 8, 1, 0, 1.0, None, st) == SED_ERR_ARG
    sync(dev)
    assert clean(), "a call refused for its null scratch wrote"
    # B = 0, and T < PT: SED_OK, the four reductions zeroed, the dropped rows of dz zeroed, nothing else written
    for C, PT, PF, F, split in ((16, 2, 2, 8, 0), (16, 2, 2, 4, 0), (32, 2, 2, 16, 0), (32, 2, 2, 8, 0), (64, 1, 2, 2, 1), (128, 1, 2, 2, 0),
                                (128, 1, 2, 2, 1)):
        for B, T in ((0, 7), (0, 6), (2, 1)):
            if PT == 1 and B > 0:
                continue                        # (1, 2) pooling: T = 1 is a window
            fo = vec_frame(dev, 4096)
            assert rc("sed_glu_fwd", p, p, p, p, fo.ptr(), B, T, F, C, PT, PF, 1, 0, 1.0, None, split, st) == 0
            fdz = fout(dev, max(B * T * F, 1), C)
            fr = [fout(dev, C, C), vec_frame(dev, C), vec_frame(dev, C), vec_frame(dev, C)]
            nscr = int(lib.value("sed_glu_bwd_scratch_floats", B, T, F, C, PT, PF))
            fscr = vec_frame(dev, nscr)
            assert rc("sed_glu_bwd", p, p, p, p, p, p, p, fdz.ptr(), fr[0].ptr(), fr[1].ptr(), fr[2].ptr(), fr[3].ptr(), fscr.ptr(), B, T, F, C,
                      PT, PF, 1, 0, 1.0, None, split, st) == 0, (C, B, T)
            sync(dev)
            what = "empty glu C=%d F=%d B=%d T=%d" % (C, F, B, T)
            assert untouched(fo), what + ": out written"
            assert untouched(fscr), what + ": scratch written"
            for f in fr:
                f.assert_frame(what)
                assert not f.get().any(), what + ": a reduction is not zero"
            fdz.assert_frame(what)
            if B > 0:
                assert not fdz.get().any(), what + ": dropped rows of dz not zeroed"
            else:
                assert untouched(fdz), what + ": dz written"
            # the call leaves no error behind for the next one
            assert rc("sed_bn_finalize", p, 1, 0, 4.0, p, p, p, p, MOMENTUM, EPS, p, 1, 1, st) == SED_ERR_ARG
            d = FinalizeData.get(16, 1)
            call_finalize(dev, d, 1, 0)
    assert clean()
    assert rc("sed_bn_bwd_apply", p, p, p, p, p, p, p, 0, 16, 1, st) == 0
    for B, T in ((0, 4), (2, 1)):
        fo = vec_frame(dev, 4096)
        assert rc("sed_block0_fwd", p, p, p, None, p, p, p, fo.ptr(), B, T, 8, 1, 0, 1.0, None, st) == 0
        outs = [vec_frame(dev, n) for n in (144, 16, 16, 16, 256, 16)]
        fscr = vec_frame(dev, int(lib.value("sed_block0_bwd_scratch_floats", B, T, 8)))
        assert rc("sed_block0_bwd", p, p, p, None, p, p, p, p, p, p, *[f.ptr() for f in outs], fscr.ptr(), B, T, 8, 1, 0, 1.0, None, st) == 0
        sync(dev)
        assert untouched(fo) and untouched(fscr), "empty block0: out or scratch written"
        for f in outs:
            f.assert_frame("empty block0")
            assert not f.get().any(), "empty block0: a gradient is not zero"
    sync(dev)
    assert clean(), "an empty call wrote through an input pointer"


# ---- which kernel every row launches ----------------------------------------------------------------------------------------------
def global_kernels(source):
    """Names of the __global__ functions of a csrc file."""
    text = open(os.path.join(CSRC, source)).read()
    return set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text))


def launch_table(gpu=True):
    """[(row description, [kernels])] for every row of the families, GPU-only rows included when gpu."""
    table = []
    for row in glu_rows():
        if row["gpu_only"] and not gpu:
            continue
        fwd, bwd, _ = glu_kernels(row)
        table.append((describe_glu(row), fwd + bwd))
    table += [("bn_finalize C=%d nblocks=%d" % r, ["bn_finalize_kernel"]) for r in FINALIZE_ROWS]
    table += [("bn_bwd_apply C=%d npix=%d" % r, ["bn_bwd_apply_kernel"]) for r in apply_rows(gpu)]
    table += [("conv0 F=%d T=%d bounds=%d" % r, ["conv0_kernel", "conv0_wgrad_kernel"]) for r in CONV0_ROWS]
    for row in block0_rows():
        if row["gpu_only"] and not gpu:
            continue
        table.append((describe_b0(row), ["block0_fwd_kernel", "block0_bwd_kernel", "block0_bwd_reduce_kernel", "block0_bwd_final_kernel"]
                      if row["T"] >= 2 else []))
    return table


ENTRIES = ("sed_glu_fwd", "sed_glu_bwd", "sed_bn_finalize", "sed_bn_bwd_apply", "sed_block0_fwd", "sed_block0_bwd", "sed_conv0_fwd",
           "sed_conv0_wgrad")


def case_rows_reach_every_kernel(gpu=True):
    """Static: the rows' kernels, derived from the dispatch conditions, cover every __global__ function of sed_glu.hip and sed_block0.hip
    (both instantiations of glu128_fwd_c_kernel), and this module calls each of the eight entry points."""
    reached = set()
    for _, ks in launch_table(gpu):
        reached.update(ks)
    names = {k.split("<")[0] for k in reached}
    need = global_kernels("sed_glu.hip") | global_kernels("sed_block0.hip")
    assert need and "glu16_bwd_kernel" in need and "block0_bwd_kernel" in need, need
    assert not need - names, "kernels no row launches: %s" % sorted(need - names)
    assert {"glu128_fwd_c_kernel<true>", "glu128_fwd_c_kernel<false>"} <= reached
    # every C the templated kernels are instantiated for
    inst = set()
    for row in glu_rows():
        fwd, bwd, _ = glu_kernels(row)
        inst.update((k, row["C"]) for k in fwd + bwd)
    for k, cs in (("glu_fwd_kernel", (16, 32)), ("glu_bwd_kernel", (16, 32)), ("glu_wide_fwd_kernel", (64, 128)), ("glu_wide_bwd_kernel", (64, 128)),
                  ("glu_wide_fwd_b_kernel", (64, 128)), ("glu_wide_bwd_b_kernel", (64, 128)), ("glu_bwd_reduce_kernel", (16, 32, 64, 128))):
        assert {(k, c) for c in cs} <= inst, (k, cs)
    # every wide instantiation has a row in which a workgroup walks several tiles and the shares are unequal (the persistent loop's
    # prefetch of the next tile and the per-workgroup partial over tiles): launch_glu_wide_fwd / launch_glu_wide_bwd restated
    walked = set()
    for row in glu_rows():
        if row["C"] < 64:
            continue
        tile_rows = 32 * (8 // (row["C"] // 32))
        ntiles = -(-row["B"] * row["T"] * row["F"] // tile_rows)
        fwd, bwd, _ = glu_kernels(row)
        for k, dflt in ((fwd[0], 512), (bwd[0], 256)):
            grid = min(ntiles, row["cap"] if row["cap"] > 0 else dflt)
            if ntiles > grid and ntiles % grid != 0:
                walked.add((k, row["C"]))
    wide = {(k, c) for k, c in inst if "wide" in k or "glu128" in k}
    assert len(wide) == 11 and wide == walked, "wide kernels without a multi-tile row: %s" % sorted(wide - walked)
    src = open(os.path.abspath(__file__)).read()
    for e in ENTRIES:
        assert '"%s"' % e in src, e


# ---- the constants and the discrimination condition (no kernel involved) ----------------------------------------------------------
def _r(m32, m64, S):
    return ratio_of(m32, m64, U24 * S)


def measure_constants(gpu_rows=True):
    """-> {family: largest ratio of the fp32 restatement against the float64 model, in units of 2^-24 S}.  On one thread: torch's fp32
    reductions split their sums by thread, and the figure is to be the same wherever the test runs."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _measure_constants(gpu_rows)
    finally:
        torch.set_num_threads(threads)


def _measure_constants(gpu_rows):
    worst = dict.fromkeys(C_FAMILY, 0.0)
    f32 = torch.float32
    seen = set()
    for row in glu_rows():
        key = tuple(row[k] for k in ("C", "PT", "PF", "B", "T", "F"))
        if key in seen or (row["gpu_only"] and not gpu_rows):
            continue
        seen.add(key)
        d = GluData.get(*key)
        for p in (0.5, 0.0):
            m = d.models(p)
            worst["glu_fwd"] = max(worst["glu_fwd"], _r(d.fwd(p, dt=f32), m["out"], m["S_out"]))
            b32 = d.bwd(p, dt=f32)
            for k, v in b32.items():
                worst["glu_bwd"] = max(worst["glu_bwd"], _r(v, m["bwd"][k], m["S"][k]))
    for F, T, which in CONV0_ROWS:
        d = Layer0Data.get(3, T, F, which)
        worst["conv0_fwd"] = max(worst["conv0_fwd"], _r(d.conv(f32), d.conv(), d.S_y()))
        kn = k_of(3 * T * F)
        S = kn * torch.nn.grad.conv2d_weight(d.xm().abs()[:, None], (16, 1, 3, 3), d.dy.double().abs().permute(0, 3, 1, 2).contiguous(), padding=1)
        worst["conv0_wgrad"] = max(worst["conv0_wgrad"], _r(d.wgrad(d.dy, f32), d.wgrad(d.dy), S))
    for row in block0_rows():
        if row["gpu_only"] and not gpu_rows:
            continue
        d = Layer0Data.get(row["B"], row["T"], row["F"], row["which"])
        for p in (0.5, 0.0):
            m = d.block_models(p)
            worst["block0_fwd"] = max(worst["block0_fwd"], _r(d.block_fwd(d.stats, p, dt=f32), m["out"], m["S_out"]))
            b32 = d.block_bwd(p, dt=f32)
            for k in ("dW", "dgamma", "dbeta", "dWg", "dbg"):
                worst["block0_bwd"] = max(worst["block0_bwd"], _r(b32[k], m["bwd"][k], m["S"][k]))
    return worst


def two_digits_up(x):
    """x rounded up to two significant digits."""
    unit = 10.0 ** (math.floor(math.log10(x)) - 1)
    return round(math.ceil(x / unit - 1e-9) * unit, 12)


def case_constants():
    """The committed c of every family is exactly 4 x the fp32 restatement's largest ratio, rounded up to two significant digits.
    The ratio is taken over ALL rows of the family, the GPU-only ones included (8 200 pooled GLU rows; B = 2, T = 626, F = 128 of block
    0): they are most of this test's time, and they set c from rows on which the emulator suite runs no kernel -- the same c must
    hold where those rows do run."""
    worst = measure_constants()
    print("fp32 restatement, largest ratio per family:", {k: round(v, 4) for k, v in worst.items()})
    for k, v in worst.items():
        assert C_FAMILY[k] == two_digits_up(4 * v), "c[%s] = %s, 4 x r_ref = %.4f -> %s" % (k, C_FAMILY[k], 4 * v, two_digits_up(4 * v))


def _must_leave(name, model, mutant, bound, min_fraction=0.0):
    frac = leaves_bound(model, mutant, bound)
    print("[blocks] discrimination %s: outside the bound in %.1f %% of %d elements" % (name, 100 * frac, model.numel()))
    assert frac > 0 and frac >= min_fraction, "%s: the mutated model leaves the bound in only %.2f %% of the elements" % (name, 100 * frac)


def case_discrimination(min_fraction=0.25):
    """No kernel: every listed mutation of the float64 model leaves the bound (global mutations in >= 25 % of the elements)."""
    d64 = torch.float64
    # ---- GLU: one narrow and one wide shape, with and without the split terms ----
    for (C, PT, PF, B, T, F), split in (((16, 2, 2, 3, 7, 8), 0), ((32, 2, 2, 3, 7, 16), 0), ((64, 1, 2, 3, 13, 16), 1), ((128, 1, 2, 3, 13, 16), 1)):
        d = GluData.get(C, PT, PF, B, T, F)
        m = d.models(0.5)
        cs = C_SPLIT if split else 0.0
        tag = "glu C=%d " % C
        b_out = C_FAMILY["glu_fwd"] * U24 * m["S_out"] + cs * m["Sp_out"]
        bb = {k: C_FAMILY["glu_bwd"] * U24 * m["S"][k] + cs * m["Sp"][k] for k in m["S"]}
        _must_leave(tag + "out, keep mask of seed + 1", m["out"], d.fwd(0.5, SEED + 1), b_out, min_fraction)
        other = d.bwd(0.5, SEED + 1)
        for k in ("dz", "dWg"):
            _must_leave(tag + k + ", keep mask of seed + 1", m["bwd"][k], other[k], bb[k], min_fraction)
        _must_leave(tag + "out, one window's divisor", m["out"], d.fwd(0.5, mut="divisor"), b_out)
        _must_leave(tag + "dz, one window's divisor", m["bwd"]["dz"], d.bwd(0.5, mut="divisor")["dz"], bb["dz"])
        # the last pixel of the last (ragged) tile dropped from each reduction
        last = GluDataLastPixel(d)
        for k in ("dWg", "dbg", "dgamma", "dbeta"):
            _must_leave(tag + k + ", last pixel dropped", m["bwd"][k], m["bwd"][k] - last.contribution(0.5)[k], bb[k])
        if T % PT:
            dz = m["bwd"]["dz"].clone()
            dz[:, T - 1] = dz[:, T - 2]
            _must_leave(tag + "dz, dropped frames given a gradient", m["bwd"]["dz"], dz, bb["dz"])
        # dWg without its beta . dbg term (the split kernels' correction after the accumulation)
        nobeta = m["bwd"]["dWg"] - m["bwd"]["dbg"][:, None] * d.beta.to(d64)[None, :]
        _must_leave(tag + "dWg without beta dbg", m["bwd"]["dWg"], nobeta, bb["dWg"], min_fraction)
        if split:
            _must_leave(tag + "out, one split product dropped", m["out"], d.fwd(0.5, mut="split_product"), b_out, min_fraction)
    # ---- sed_bn_finalize: count instead of count - 1 ----
    for C, nb in FINALIZE_ROWS:
        d = FinalizeData.get(C, nb)
        model, bound = d.model(1)
        _must_leave("bn_finalize C=%d nblocks=%d, count for count - 1" % (C, nb), model["rv"], d.model(1, "count")[0]["rv"], bound["rv"], min_fraction)
    # ---- sed_bn_bwd_apply: eval-mode dbias = 0 ----
    for C, npix in apply_rows(False):
        d = ApplyData(C, npix)
        _, _, db, e = d.model(0)
        _must_leave("bn_bwd_apply C=%d eval dbias = 0" % C, db, d.model(0, "dbias0")[2], e, min_fraction)
    # ---- layer 0 ----
    for T, F in ((17, 8), (33, 128)):
        d = Layer0Data.get(3, T, F, 0)
        tag = "layer 0 T=%d F=%d " % (T, F)
        b_y = C_FAMILY["conv0_fwd"] * U24 * d.S_y()
        _must_leave(tag + "y, clip 0's bounds for every clip", d.conv(), d.conv(mut="clip0"), b_y)
        wm = conv0_wgrad_models(d)
        for fuse in (0, 1):
            model, S, extra = wm[fuse]
            bound = C_FAMILY["conv0_wgrad"] * U24 * S
            dy = d.dy if fuse == 0 else d.bn_dy(d.dy, extra[0], extra[1], extra[2])[0]
            _must_leave(tag + "conv0 dW fuse_bn=%d, clip 0's bounds" % fuse, model, d.wgrad(dy, mut="clip0"), bound, min_fraction)
            _must_leave(tag + "conv0 dW fuse_bn=%d, last pixel dropped" % fuse, model, d.wgrad(dy, drop_last=True), bound)
        m = d.block_models(0.5)
        b_out = C_FAMILY["block0_fwd"] * U24 * m["S_out"]
        bb = {k: C_FAMILY["block0_bwd"] * U24 * m["S"][k] for k in ("dW", "dgamma", "dbeta", "dWg", "dbg")}
        _must_leave(tag + "block0 out, clip 0's bounds", m["out"], d.block_fwd(d.stats, 0.5, mut="clip0"), b_out)
        _must_leave(tag + "block0 out, keep mask of seed + 1", m["out"], d.block_fwd(d.stats, 0.5, mut="seed"), b_out, min_fraction)
        _must_leave(tag + "block0 out, one window's divisor", m["out"], d.block_fwd(d.stats, 0.5, mut="divisor"), b_out)
        for mut, ks, frac in (("clip0", ("dW", "dWg"), 0.0), ("seed", ("dW", "dWg"), min_fraction), ("divisor", ("dW", "dWg"), 0.0),
                              ("last_pixel", ("dW",), 0.0), ("dropped_rows", ("dW",), 0.0)):
            other = d.block_bwd(0.5, mut=mut)
            for k in ks:
                _must_leave(tag + "block0 %s, %s" % (k, mut), m["bwd"][k], other[k], bb[k], frac)


class GluDataLastPixel:
    """The contribution of the last pooled pixel (last clip, last kept frame, last bin) to the four reductions of the GLU backward: the
    backward of the same problem with gout zero everywhere but in that pixel's window, restricted to that pixel."""

    def __init__(self, d):
        self.d = d

    def contribution(self, p):
        d = self.d
        C, PT, PF, B, T, F = d.key
        dt = torch.float64
        xhat = (d.y.to(dt) - d.mean.to(dt)) * d.invstd.to(dt)
        ks = d.ks(p, SEED).clone()
        only = torch.zeros_like(ks)
        t, f = (T // PT) * PT - 1, (F // PF) * PF - 1
        only[-1, t, f] = ks[-1, t, f]
        return glu_backward(xhat, d.gamma.to(dt), d.beta.to(dt), d.Wg.to(dt), d.bg.to(dt), only, d.gout.to(dt), PT, PF)


def report_ratios(dev):
    """Prints what check() recorded (the figures of the docstring and DESIGN.md); check() itself asserts each of them."""
    mine = {k[1]: round(v, 3) for k, v in STATS.items() if k[0] == dev and k[1] in set(C_FAMILY) | {"bn_finalize", "bn_bwd_apply"}}
    print("[blocks] largest |err| / bound per family on %s:" % dev, mine, "c:", C_FAMILY)
