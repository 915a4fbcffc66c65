"""Direct numerical cases for the dense GEMM entry points (csrc/sed_gemm_bf16.hip, the exact-f32 twins and sed_colsum in
csrc/sed_gru.hip) and the parameter-arena kernels (csrc/sed_optim.hip), each against a float64 restatement on the host.
Device-agnostic like parity_cases.py: dev = "cpu" on the fiber emulator, "cuda" on the MI355X.

Every operand and every output is a 16-byte aligned window of a larger buffer filled with a canary value (`Frame`): at least one whole
row of the leading dimension + 8 floats before and after, and the ld - cols gap columns.  After a call the canaries of outputs and
scratch must be bit-identical and the inputs unchanged.

Bounds are per element, with S = |opA(A)| . |opB(B)| + |bias| + |C_in| (float64):
  tier A (derived, any summation order):  |C - ref|   <= (c_split + (K + slices + 2) 2^-24) S,  c_split = 3 * 2^-16 for split-bf16
          (|x - hi| <= 2^-8 |x|, |x - hi - lo| <= 2^-16 |x|: the dropped lo*lo and the two residual terms are each <= 2^-16 |a||b|), 0 for f32;
  tier B (accumulation only):             |C - model| <= BETA (sqrt(K) + 2) 2^-24 S,  model = the float64 value of Ah.Bh + Ah.Bl + Al.Bh
          (split-bf16 entries; `split_model`) or ref itself (exact-f32 entries).
BETA is 4 x the largest ratio r_ref = max |chain32 - model| / ((sqrt(K) + 2) 2^-24 S) that a plain fp32 reference accumulation (`chain32`:
one k at a time, al*bh, ah*bl, ah*bh -- or the one product a*b -- added to an fp32 accumulator, nothing from the library) shows over
the rows of the tables below; the factor 4 is for the kernels' different, equally legitimate summation order (16-k MFMA blocks, three
interleaved chains, slices, atomics).  test_emu_contractions.py::test_beta_is_what_the_reference_chain_gives recomputes it.

Measured (seeded operands of the tables; the largest r_ref are those of the K = 20 and K = 52 rows):
  reference chain  r_ref max = 0.579  ->  BETA = 2.4
  largest kernel ratio |C - target| / ((sqrt(K) + 2) 2^-24 S), tables + caller-shaped rows:
                    split-bf16 MFMA   exact-f32 MFMA (vector loads)   exact-f32 scalar fall-back
    CPU emulator         0.69                   0.77                           0.50
    MI355X               0.29                   0.71                           0.50
(the kernels sit beside the reference chain, as they should; a ratio above BETA is a finding to run down -- a wrong tile edge is a few
elements far out, MFMA-internal rounding all elements slightly out -- not a reason to raise BETA).
"""
import math

import torch

from desed_task_amd import _lib

U24 = 2.0 ** -24
C_SPLIT = 3 * 2.0 ** -16
BETA = 2.4
CANARY = -12345.6787109375            # exactly representable in fp32
CANARY_BITS = int(torch.tensor([CANARY], dtype=torch.float32).view(torch.int32).item())
SED_ERR_ARG, SED_ERR_UNSUPPORTED = -1, -3
STATS = {}                            # largest tier-B ratio seen per (device, kernel), for the figures in the docstring / DESIGN.md


def rc(name, *args):
    """The entry's return code (lib.call raises on a non-zero one)."""
    return getattr(_lib.get()._dll, name)(*args)


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def stream(dev):
    return 0 if dev == "cpu" else torch.cuda.current_stream().cuda_stream


# ---- framed operands -------------------------------------------------------------------------------------------------------------
class Frame:
    """rows x ld floats inside a canary-filled buffer; `windows` = [(first column, columns)] are the operands that live in it (two for
    the interleaved operands of the BiGRU callers: dgi (B T, 2, 3H) holds both directions side by side)."""

    def __init__(self, dev, rows, ld, windows=None, misalign=0, guard=None):
        windows = [(0, ld)] if windows is None else list(windows)
        assert all(c0 >= 0 and c > 0 and c0 + c <= ld for c0, c in windows), (ld, windows)
        self.rows, self.ld, self.windows = rows, ld, windows
        guard = ld + 8 if guard is None else guard
        pre = (guard + 3) // 4 * 4
        n = pre + misalign + rows * ld + guard
        self.buf = torch.full((n,), CANARY, device=dev, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.start = pre + misalign
        self.mask = torch.zeros(n, dtype=torch.bool)
        body = self.mask[self.start:self.start + rows * ld].view(rows, ld)
        for c0, c in windows:
            body[:, c0:c0 + c] = True

    def ptr(self, w=0, row=0, col=0):
        return self.buf.data_ptr() + 4 * (self.start + row * self.ld + self.windows[w][0] + col)

    def view(self, w=0):
        c0, c = self.windows[w]
        return self.buf.as_strided((self.rows, c), (self.ld, 1), self.start + c0)

    def put(self, t, w=0):
        self.view(w).copy_(t.to(self.buf.device))
        return self

    def fill(self, value, w=0):
        self.view(w).fill_(value)
        return self

    def get(self, w=0):
        return self.view(w).cpu().clone()

    def bits(self):
        return self.buf.cpu().view(torch.int32).clone()

    def assert_frame(self, what):
        bad = (self.buf.cpu().view(torch.int32) != CANARY_BITS) & ~self.mask
        if bad.any():
            idx = bad.nonzero().flatten()
            rel = idx - self.start
            raise AssertionError("%s: %d canaries overwritten; first at (row %d, col %d) of a %d x %s window set with ld %d" % (
                what, idx.numel(), int(rel[0]) // max(self.ld, 1) if rel[0] >= 0 else -1, int(rel[0]) % max(self.ld, 1), self.rows,
                self.windows, self.ld))


def vec_frame(dev, n, misalign=0):
    """n floats (one row) with up to 4 104 canaries on either side."""
    return Frame(dev, 1, n, [(0, n)], misalign, guard=min(n, 4096) + 8) if n > 0 else Frame(dev, 0, 4)


# ---- references ------------------------------------------------------------------------------------------------------------------
def bf16_parts(x):
    """hi = bf16_rne(x), lo = bf16_rne(x - hi) (sed_common.h: bf16_split), both as fp32."""
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi, lo


def split_model(a, b):
    """float64 value of what the split-bf16 kernels are meant to compute for a (M,K) . b (K,N): Ah.Bh + Ah.Bl + Al.Bh."""
    ah, al = bf16_parts(a)
    bh, bl = bf16_parts(b)
    return ah.double() @ bh.double() + ah.double() @ bl.double() + al.double() @ bh.double()


def chain32(a, b, split):
    """The reference accumulation in fp32: one k at a time; split: al*bh, ah*bl, ah*bh in that order, else the one product a*b."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)               # thousands of small element-wise operations: a thread pool only gets in the way
    try:
        _chain32(acc, a, b, split)
    finally:
        torch.set_num_threads(threads)
    return acc


def _chain32(acc, a, b, split):
    if split:
        ah, al = bf16_parts(a)
        bh, bl = bf16_parts(b)
        for k in range(a.shape[1]):
            acc += al[:, k:k + 1] * bh[k:k + 1, :]
            acc += ah[:, k:k + 1] * bl[k:k + 1, :]
            acc += ah[:, k:k + 1] * bh[k:k + 1, :]
    else:
        for k in range(a.shape[1]):
            acc += a[:, k:k + 1] * b[k:k + 1, :]


def tier_b_unit(K, S):
    return (math.sqrt(K) + 2.0) * U24 * S


# ---- dispatch mirror ---------------------------------------------------------------------------------------------------------------
def slices_of(K, split):
    split = max(1, split)
    kps = ((K + split - 1) // split + 31) // 32 * 32
    return kps, (K + kps - 1) // kps


def mirror(entry, M, N, K, lda, ldb, ta, tb, split, acc, aligned=True):
    """Restates the tile / slice choice of gemmb_dispatch (sed_gemm_bf16.hip) and gemm_dispatch (sed_gru.hip).  Used ONLY to assert that
    a table row reaches the branch it was written for: if a threshold moves, the row fails with "choose a new shape"."""
    nb = 2 if "pair" in entry else 1
    part = "splitk" in entry
    kcat = "kcat" in entry
    kps, sl = slices_of(K, split)
    ok = aligned and lda % 4 == 0 and ldb % 4 == 0 and (M if ta else K) % 4 == 0 and (K if tb else N) % 4 == 0 and not (ta and tb)
    tiles = ((N + 127) // 128) * ((M + 127) // 128) * sl
    out = dict(kps=kps, slices=sl, reduce_y=nb if part else 0)
    if entry.endswith("bf16x3") and ok:
        ntn = 4 if N > 64 else 2
        if ntn == 4 and tiles * nb < 400:
            ntn = 2
        if ntn == 4 and not ta and tb and N % 96 == 0:
            rows, z = (M + 127) // 128, sl * nb
            t4, t3 = rows * ((N + 127) // 128) * z, rows * (N // 96) * z
            if t4 > 768 and t3 / (-(-t3 // 768) * 768) > t4 / (-(-t4 // 768) * 768) + 0.1:
                ntn = 3
        out.update(kernel="bf16x3", ntn=ntn, atomic=(not part) and (sl > 1 or bool(acc)))
        return out
    if entry.endswith("bf16x3") and (part or kcat):
        out.update(kernel="unsupported", ntn=0, atomic=False)
        return out
    if ta and tb:
        out.update(kernel="unsupported", ntn=0, atomic=False)
        return out
    if not ok:
        nb = 1                       # the scalar fall-back of a pair is two plain launches
    ntn = 4 if N > 64 else 2
    if ntn == 4 and tiles * nb < 200:
        ntn = 2
    out.update(kernel="vec" if ok else ("unsupported" if kcat else "scalar"), ntn=ntn, atomic=sl > 1 or bool(acc))
    return out


# ---- one GEMM problem (or two) in framed buffers ----------------------------------------------------------------------------------
def G(entry, M, N, K, ta, tb, split=1, acc=0, bias=True, pad=(0, 0, 0), inter=False, mixed=False, mis=(0, 0), ksplit=0, want=None):
    """A table row.  pad: extra floats of lda / ldb / ldc; inter: the two problems of a pair interleaved in ONE buffer (ld = 2 cols + pad,
    the second base cols floats further -- what the BiGRU callers pass); mis: A / B base moved by that many floats."""
    nb = 2 if "pair" in entry else 1
    ac, bc = (M if ta else K), (K if tb else N)
    il = inter and nb == 2
    return dict(entry=entry, M=M, N=N, K=K, ta=ta, tb=tb, split=split, acc=acc, bias=bias, mixed=mixed, mis=mis, ksplit=ksplit,
                lda=(2 * ac if il else ac) + pad[0], a1=ac if il else None, ldb=(2 * bc if il else bc) + pad[1], b1=bc if il else None,
                ldc=(2 * N if il else N) + pad[2], c1=N if il else None, want=want)


class Problem:
    def __init__(self, dev, row, seed):
        self.dev, self.row = dev, row
        r = row
        M, N, K, ta, tb = r["M"], r["N"], r["K"], r["ta"], r["tb"]
        self.nb = nb = 2 if "pair" in r["entry"] else 1
        self.kcat = "kcat" in r["entry"]
        g = torch.Generator().manual_seed(1000 + seed)
        ashape, bshape = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))

        def operand(shape, scaled_dim):
            t = torch.randn(shape, generator=g)
            if r["mixed"]:             # rows of opA / columns of opB scaled by 10^(-4 .. +2): what gradients look like
                s = 10.0 ** (torch.rand(shape[scaled_dim], generator=g) * 6.0 - 4.0)
                t = t * (s[:, None] if scaled_dim == 0 else s[None, :])
            return t
        self.A = [operand(ashape, 1 if ta else 0)]
        if nb == 2:
            self.A.append(self.A[0] if r["a1"] == 0 else operand(ashape, 1 if ta else 0))
        self.B = [operand(bshape, 0 if tb else 1)]
        if nb == 2:
            self.B.append(self.B[0] if r["b1"] == 0 else operand(bshape, 0 if tb else 1))
        self.bias = [torch.randn(N, generator=g) for _ in range(nb)] if r["bias"] else [None] * nb
        self.Cin = [torch.randn(M, N, generator=g) for _ in range(nb)]
        misa, misb = r["mis"]

        def frames(ts, shape, ld, off, mis, kcat_rows=None):
            """-> [(frame, window)] per problem"""
            rows, cols = shape
            if kcat_rows is not None:        # B0 / B1 of the K-concatenated form: two separate buffers
                f0 = Frame(dev, kcat_rows, ld, [(0, cols)], mis).put(ts[0][:kcat_rows])
                f1 = Frame(dev, rows - kcat_rows, ld, [(0, cols)], mis).put(ts[0][kcat_rows:])
                return [(f0, 0), (f1, 0)]
            if len(ts) == 1 or off is None:
                return [(Frame(dev, rows, ld, [(0, cols)], mis).put(t), 0) for t in ts]
            if off == 0:
                f = Frame(dev, rows, ld, [(0, cols)], mis).put(ts[0])
                return [(f, 0), (f, 0)]
            f = Frame(dev, rows, ld, [(0, cols), (off, cols)], mis).put(ts[0], 0).put(ts[1], 1)
            return [(f, 0), (f, 1)]
        self.fA = frames(self.A, ashape, r["lda"], r["a1"], misa)
        self.fB = frames(self.B, bshape, r["ldb"], r["b1"], misb, kcat_rows=r["ksplit"] if self.kcat else None)
        self.fbias = [vec_frame(dev, N).put(b[None, :]) if b is not None else None for b in self.bias]
        self.new_outputs()
        self.inputs = {id(f): f for f, _ in self.fA + self.fB}
        self.inputs.update({id(f): f for f in self.fbias if f is not None})
        self.snap = {k: f.bits() for k, f in self.inputs.items()}

    def new_outputs(self):
        r = self.row
        if self.nb == 1 or r["c1"] is None:
            self.fC = [(Frame(self.dev, r["M"], r["ldc"], [(0, r["N"])]), 0) for _ in range(self.nb)]
        else:
            f = Frame(self.dev, r["M"], r["ldc"], [(0, r["N"]), (r["c1"], r["N"])])
            self.fC = [(f, 0), (f, 1)]

    def fill_c(self, mode):
        for i, (f, w) in enumerate(self.fC):
            if mode == "rand":
                f.put(self.Cin[i], w)
            else:
                f.fill(CANARY if mode == "canary" else 0.0, w)

    def p(self, fw):
        return fw[0].ptr(fw[1])

    def ptrs(self):
        d = dict(A0=self.p(self.fA[0]), B0=self.p(self.fB[0]), C0=self.p(self.fC[0]),
                 bias0=self.fbias[0].ptr() if self.fbias[0] is not None else None)
        if self.nb == 2:
            d.update(A1=self.p(self.fA[1]), B1=self.p(self.fB[1]), C1=self.p(self.fC[1]),
                     bias1=self.fbias[1].ptr() if self.fbias[1] is not None else None)
        if self.kcat:
            d["B1"] = self.p(self.fB[1])
        return d

    def aligned(self):
        d = self.ptrs()
        keys = ["A0", "B0"] + (["A1", "B1"] if self.nb == 2 else [])
        return all(d[k] % 16 == 0 for k in keys)

    def out(self, i):
        f, w = self.fC[i]
        return f.get(w)

    def op(self, i):
        """opA(A), opB(B) of problem i as (M,K), (K,N) fp32 on the host"""
        r = self.row
        a = self.A[i].t() if r["ta"] else self.A[i]
        b = self.B[0 if self.kcat else i]
        return a, (b.t() if r["tb"] else b)

    def assert_clean(self, what, scratch=None):
        for f in {id(f): f for f, _ in self.fC}.values():
            f.assert_frame(what + ": C")
        if scratch is not None:
            scratch.assert_frame(what + ": scratch")
        for k, f in self.inputs.items():
            assert torch.equal(f.bits(), self.snap[k]), what + ": an input buffer changed"


def call_args(row, P, st, scratch=None):
    """The C-ABI argument tuple of a row; P: pointers (or symbolic stand-ins) A0, A1, B0, B1, bias0, bias1, C0, C1."""
    r, e = row, row["entry"]
    dims = (r["M"], r["N"], r["K"])
    lds = (r["lda"], r["ldb"], r["ldc"])
    if e in ("sed_gemm", "sed_gemm_bf16x3"):
        return (P["A0"], P["B0"], P.get("bias0"), P["C0"]) + dims + lds + (r["ta"], r["tb"], r["split"], r["acc"], st)
    if e in ("sed_gemm_pair", "sed_gemm_pair_bf16x3"):
        return (P["A0"], P["A1"], P["B0"], P["B1"], P.get("bias0"), P.get("bias1"), P["C0"], P["C1"]) + dims + lds + (
            r["ta"], r["tb"], r["split"], r["acc"], st)
    if e == "sed_gemm_pair_splitk_bf16x3":
        return (P["A0"], P["A1"], P["B0"], P["B1"], P["C0"], P["C1"]) + dims + lds + (r["ta"], r["tb"], r["split"], scratch, st)
    if e == "sed_gemm_splitk_bf16x3":
        return (P["A0"], P["B0"], P["C0"]) + dims + lds + (r["ta"], r["tb"], r["split"], scratch, st)
    if e == "sed_gemm_kcat_splitk_bf16x3":
        return (P["A0"], P["B0"], P["B1"], P["C0"]) + dims + (r["ksplit"],) + lds + (r["split"], scratch, st)
    if e in ("sed_gemm_kcat", "sed_gemm_kcat_bf16x3"):
        return (P["A0"], P["B0"], P["B1"], P["C0"]) + dims + (r["ksplit"],) + lds + (st,)
    raise KeyError(e)


def check_want(row, mir):
    want = row.get("want")
    if want:
        got = {k: mir[k] for k in want}
        assert got == want, "row %s reaches %s, was written for %s: choose a new shape" % (
            {k: row[k] for k in ("entry", "M", "N", "K", "ta", "tb", "split")}, got, want)


def check_bounds(dev, row, prob, mir, what):
    """Tier A and tier B for every problem of the row; -> largest tier-B ratio."""
    r, K = row, row["K"]
    worst = 0.0
    for i in range(prob.nb):
        a, b = prob.op(i)
        extra = torch.zeros(r["M"], r["N"], dtype=torch.float64)
        mag = torch.zeros_like(extra)
        if prob.bias[i] is not None:
            extra += prob.bias[i].double()[None, :]
            mag += prob.bias[i].double().abs()[None, :]
        if r["acc"]:
            extra += prob.Cin[i].double()
            mag += prob.Cin[i].double().abs()
        ref = a.double() @ b.double() + extra
        S = a.abs().double() @ b.abs().double() + mag
        C = prob.out(i).double()
        assert torch.isfinite(C).all(), what + ": non-finite output"
        split = mir["kernel"] == "bf16x3"
        bound_a = ((C_SPLIT if split else 0.0) + (K + mir["slices"] + 2) * U24) * S
        over = (C - ref).abs() > bound_a
        assert not over.any(), "%s problem %d: tier A: %d elements out, worst |err| / bound = %.3f" % (
            what, i, int(over.sum()), float(((C - ref).abs() / bound_a.clamp_min(1e-300)).max()))
        target = split_model(a, b) + extra if split else ref
        ratio = (C - target).abs() / tier_b_unit(K, S).clamp_min(1e-300)
        rmax = float(ratio.max())
        print("[contraction] %s %s problem %d: tier-B ratio %.3f (BETA %.2f)" % (dev, what, i, rmax, BETA))
        assert rmax <= BETA, "%s problem %d: tier B: %d of %d elements above BETA, largest ratio %.3f, median %.3f" % (
            what, i, int((ratio > BETA).sum()), ratio.numel(), rmax, float(ratio.median()))
        worst = max(worst, rmax)
    key = (dev, mir["kernel"])
    STATS[key] = max(STATS.get(key, 0.0), worst)
    return worst


def describe(row):
    return "%s M=%d N=%d K=%d t%d%d split=%d acc=%d" % (row["entry"], row["M"], row["N"], row["K"], row["ta"], row["tb"], row["split"],
                                                       row["acc"])


def run_plain(dev, row, seed=0):
    """sed_gemm / sed_gemm_bf16x3 / the two pair entries / the kcat forms without scratch."""
    lib = _lib.get()
    prob = Problem(dev, row, seed)
    mir = mirror(row["entry"], row["M"], row["N"], row["K"], row["lda"], row["ldb"], row["ta"], row["tb"], row["split"], row["acc"],
                 prob.aligned())
    check_want(row, mir)
    what = describe(row)
    prob.fill_c("rand" if row["acc"] else ("zero" if mir["atomic"] else "canary"))
    lib.call(row["entry"], *call_args(row, prob.ptrs(), stream(dev)))
    sync(dev)
    prob.assert_clean(what)
    check_bounds(dev, row, prob, mir, what)
    outs = [prob.out(i) for i in range(prob.nb)]
    if prob.nb == 2 and not mir["atomic"]:
        # each problem through the single-problem entry on the same operands: the same bits (same k order per element)
        single = row["entry"].replace("_pair", "")
        P = prob.ptrs()
        for i in range(2):
            fc = Frame(dev, row["M"], row["ldc"], [(0, row["N"])])
            r1 = dict(row, entry=single)
            lib.call(single, *call_args(r1, dict(A0=P["A%d" % i], B0=P["B%d" % i], bias0=P.get("bias%d" % i), C0=fc.ptr()), stream(dev)))
            sync(dev)
            fc.assert_frame(what + ": single-problem twin")
            assert torch.equal(fc.get().view(torch.int32), outs[i].view(torch.int32)), what + ": pair != single entry, problem %d" % i
    return prob, mir, outs


def run_splitk(dev, row, seed=0):
    """The deterministic split-K entries: bounds, frames, scratch extent, independence of previous contents, run-to-run bits, and
    the reduce order (= the fp32 sum, in slice order, of the one-slice products over the K ranges the mirror predicts)."""
    lib = _lib.get()
    r = row
    M, N, K = r["M"], r["N"], r["K"]
    prob = Problem(dev, row, seed)
    mir = mirror(r["entry"], M, N, K, r["lda"], r["ldb"], r["ta"], r["tb"], r["split"], 0, prob.aligned())
    check_want(row, mir)
    what = describe(row)
    nfl = int(lib.value("sed_gemm_splitk_scratch_floats", M, N, K, r["split"]))
    assert nfl == 2 * mir["slices"] * M * N, (what, nfl)
    touched = prob.nb * mir["slices"] * M * N              # the single-problem forms use the first half
    st = stream(dev)
    runs = []
    for fill_c, fill_s in (("canary", CANARY), ("rand", 3.25)):
        prob.new_outputs()
        prob.fill_c(fill_c)
        scr = vec_frame(dev, nfl)
        scr.fill(fill_s)
        lib.call(r["entry"], *call_args(row, prob.ptrs(), st, scr.ptr()))
        sync(dev)
        prob.assert_clean(what, scr)
        s = scr.get().flatten()
        assert torch.equal(s[touched:], torch.full((nfl - touched,), fill_s)), what + ": scratch written past the slices in use"
        if fill_s == CANARY:
            assert (s[:touched] != CANARY).all(), what + ": scratch_floats covers more than the launch writes"
        runs.append([prob.out(i) for i in range(prob.nb)])
    for i in range(prob.nb):
        assert torch.equal(runs[0][i].view(torch.int32), runs[1][i].view(torch.int32)), \
            "%s: two runs differ / the result depends on the previous contents of C or scratch (problem %d)" % (what, i)
    check_bounds(dev, row, prob, mir, what)
    # the reduce order
    P, kps = prob.ptrs(), mir["kps"]
    for i in range(prob.nb):
        acc = torch.zeros(M, N)
        for z in range(mir["slices"]):
            k0, k1 = z * kps, min(K, (z + 1) * kps)
            pa = P["A%d" % i] + 4 * (k0 * r["lda"] if r["ta"] else k0)
            tmp = Frame(dev, M, N)
            if prob.kcat and k0 < r["ksplit"] < k1:
                lib.call("sed_gemm_kcat_bf16x3", pa, P["B0"] + 4 * k0 * r["ldb"], P["B1"], tmp.ptr(), M, N, k1 - k0, r["ksplit"] - k0,
                         r["lda"], r["ldb"], N, st)
            else:
                if prob.kcat:
                    pb = P["B0"] + 4 * k0 * r["ldb"] if k1 <= r["ksplit"] else P["B1"] + 4 * (k0 - r["ksplit"]) * r["ldb"]
                else:
                    pb = P["B%d" % i] + 4 * (k0 if r["tb"] else k0 * r["ldb"])
                m1 = mirror("sed_gemm_bf16x3", M, N, k1 - k0, r["lda"], r["ldb"], r["ta"], r["tb"], 1, 0, pa % 16 == 0 and pb % 16 == 0)
                assert m1["kernel"] == "bf16x3" and m1["slices"] == 1, (what, m1)
                lib.call("sed_gemm_bf16x3", pa, pb, None, tmp.ptr(), M, N, k1 - k0, r["lda"], r["ldb"], N, r["ta"], r["tb"], 1, 0, st)
            sync(dev)
            tmp.assert_frame(what + ": one-slice product")
            acc = acc + tmp.get()
        assert torch.equal(acc.view(torch.int32), runs[0][i].view(torch.int32)), \
            "%s: not the slice-order fp32 sum of the one-slice products (problem %d, %d elements differ)" % (
                what, i, int((acc != runs[0][i]).sum()))
    return prob, mir, runs[0]


def run_row(dev, row, seed=0):
    return (run_splitk if "splitk" in row["entry"] else run_plain)(dev, row, seed)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ((0, 0), (0, 1), (1, 0))


def table_plain():
    """(a): plain and pair entries, both precisions, three layouts, both tile widths."""
    rows = []
    for bf in (True, False):
        sfx = "_bf16x3" if bf else ""
        kern = "bf16x3" if bf else "vec"
        for ta, tb in LAYOUTS:
            # single problem, ragged M, N against the tile, K % 32 != 0, padded leading dimensions, bias, plain store onto canaries
            rows.append(G("sed_gemm" + sfx, 132, 72, 52, ta, tb, pad=(4, 8, 12), want=dict(kernel=kern, ntn=2, slices=1, atomic=False)))
            # pair, interleaved bases, four slices of 96 with a last slice of 12, null biases, atomics onto zeros
            rows.append(G("sed_gemm_pair" + sfx, 260, 200, 300, ta, tb, split=4, bias=False, inter=True, pad=(4, 4, 4),
                          want=dict(kernel=kern, ntn=2, slices=4, kps=96, atomic=True)))
            # pair, K below one tile, N <= 64, accumulate onto a non-zero C
            rows.append(G("sed_gemm_pair" + sfx, 36, 40, 20, ta, tb, acc=1, pad=(8, 4, 4), want=dict(kernel=kern, ntn=2, slices=1, atomic=True)))
            # pair, distinct operands in separate buffers, plain store, bias: compared bit for bit with the single-problem entry
            rows.append(G("sed_gemm_pair" + sfx, 196, 136, 100, ta, tb, pad=(4, 0, 4), want=dict(kernel=kern, ntn=2, slices=1, atomic=False)))
            # the 128-column tile through the dispatch: 6 x 5 tiles x 2 problems x 8 (4) slices = 480 (240) workgroups; accumulate = 1
            rows.append(G("sed_gemm_pair" + sfx, 644, 612, 256 if bf else 128, ta, tb, split=8 if bf else 4, acc=1, inter=True,
                          want=dict(kernel=kern, ntn=4, slices=8 if bf else 4, atomic=True)))
            # operands of mixed magnitude
            rows.append(G("sed_gemm" + sfx, 132, 72, 1000, ta, tb, mixed=True, want=dict(kernel=kern, ntn=2, slices=1, atomic=False)))
    # the 128-column tile of the exact-f32 kernel with a plain store (one slice): 11 x 10 tiles x 2 problems = 220 workgroups
    rows.append(G("sed_gemm_pair", 1300, 1180, 36, 0, 1, want=dict(kernel="vec", ntn=4, slices=1, atomic=False)))
    return rows


def table_scalar():
    """sed_gemm on operands that break the 16-byte conditions one at a time (the scalar kernel), and the same arguments to
    sed_gemm_bf16x3, which must give the f32 fall-back's bits."""
    want = dict(kernel="scalar", ntn=2, slices=1)
    return [G("sed_gemm", 130, 72, 48, 0, 0, pad=(1, 0, 0), want=want),             # odd lda
            G("sed_gemm", 130, 72, 48, 0, 1, mis=(1, 0), want=want),                # A base + 4 bytes
            G("sed_gemm", 132, 72, 48, 1, 0, mis=(0, 1), want=want),                # B base + 4 bytes
            G("sed_gemm", 130, 70, 45, 0, 1, want=want),                            # K % 4 != 0
            G("sed_gemm", 96, 40, 300, 1, 0, split=4, bias=False, pad=(0, 3, 0), want=dict(kernel="scalar", ntn=2, slices=4, atomic=True))]


def table_splitk():
    """(b): the deterministic split-K entries: 1, 2, 3, 29, 32 slices, a request larger than K / 32, ragged shapes, padded lds."""
    pk, sk, kc = "sed_gemm_pair_splitk_bf16x3", "sed_gemm_splitk_bf16x3", "sed_gemm_kcat_splitk_bf16x3"
    w = lambda sl, ntn=2, y=1: dict(kernel="bf16x3", ntn=ntn, slices=sl, atomic=False, reduce_y=y)      # noqa: E731
    rows = [
        G(pk, 132, 72, 100, 1, 0, split=1, bias=False, inter=True, pad=(4, 4, 4), want=w(1, y=2)),
        G(pk, 132, 72, 100, 1, 0, split=2, bias=False, inter=True, pad=(4, 4, 4), want=w(2, y=2)),          # 64 + 36
        G(pk, 36, 40, 928, 1, 0, split=29, bias=False, pad=(4, 0, 8), want=w(29, y=2)),
        G(pk, 36, 40, 1000, 0, 1, split=32, bias=False, pad=(0, 4, 4), want=w(32, y=2)),                    # last slice: 8
        G(pk, 132, 72, 100, 0, 0, split=7, bias=False, want=w(4, y=2)),                                     # request > K / 32
        G(pk, 132, 72, 7488, 1, 0, split=29, bias=False, inter=True, mixed=True, want=w(26, y=2)),          # K and slices of the BiGRU dW at B = 48
        G(pk, 644, 612, 256, 1, 0, split=8, bias=False, inter=True, want=w(8, ntn=4, y=2)),                 # 128-column tile, plain stores
        G(pk, 644, 612, 256, 0, 0, split=8, bias=False, want=w(8, ntn=4, y=2)),
        G(pk, 644, 612, 256, 0, 1, split=8, bias=False, want=w(8, ntn=4, y=2)),
        G(sk, 132, 72, 96, 1, 0, split=3, bias=False, pad=(4, 4, 4), want=w(3)),
        G(sk, 260, 200, 300, 0, 1, split=2, bias=False, pad=(4, 8, 4), mixed=True, want=w(2)),              # 160 + 140
        G(sk, 36, 40, 928, 0, 0, split=29, bias=False, want=w(29)),
        G(kc, 132, 128, 768, 0, 0, split=2, ksplit=384, bias=False, pad=(4, 4, 4), want=w(2)),              # switch on a slice boundary
        G(kc, 132, 128, 768, 0, 0, split=5, ksplit=384, bias=False, want=w(5)),                             # 160-wide slices: one straddles it
        G(kc, 280, 72, 96, 0, 0, split=3, ksplit=64, bias=False, pad=(0, 4, 4), mixed=True, want=w(3)),
        G(kc, 36, 40, 1000, 0, 0, split=32, ksplit=512, bias=False, want=w(32)),
        G(kc, 132, 72, 100, 0, 0, split=1, ksplit=32, bias=False, want=w(1)),
    ]
    return rows


def bigru_rows(B, T, I, H, prec="bf16x3", dw_atomic=False, dx_splitk=True):
    """(c): the GEMM calls of ops.BiGRULayerFn (forward, backward, _weight_grads) as table rows; `sym` names the tensors behind the
    pointers (name, byte offset).  tests/test_emu_contractions.py::test_caller_rows_are_what_ops_issues pins it to ops.py."""
    BT = B * T
    bf = prec == "bf16x3"
    pair = "sed_gemm_pair_bf16x3" if bf else "sed_gemm_pair"
    split = max(1, min(32, BT // 256))
    base = dict(mixed=False, mis=(0, 0), ksplit=0, want=None, bias=False, acc=0)
    rows = [dict(base, tag="gi", entry=pair, M=BT, N=3 * H, K=I, ta=0, tb=1, split=1, bias=True, lda=I, a1=0, ldb=I, b1=None, ldc=6 * H,
                 c1=3 * H, sym=dict(A0=("x", 0), A1=("x", 0), B0=("w_ih0", 0), B1=("w_ih1", 0), bias0=("b_ih0", 0), bias1=("b_ih1", 0),
                                    C0=("gi", 0), C1=("gi", 12 * H)))]
    nsl = min(max(1, round(700.0 / (((I + 63) // 64) * ((BT + 127) // 128)))), max(1, (6 * H) // 128)) if dx_splitk else 1
    dxe = ("sed_gemm_kcat_splitk_bf16x3" if nsl > 1 and I % 4 == 0 else "sed_gemm_kcat_bf16x3") if bf else "sed_gemm_kcat"
    rows.append(dict(base, tag="dx", entry=dxe, M=BT, N=I, K=6 * H, ta=0, tb=0, split=nsl if "splitk" in dxe else 1, ksplit=3 * H,
                     lda=6 * H, a1=None, ldb=I, b1=None, ldc=I, c1=None,
                     sym=dict(A0=("dgi", 0), B0=("w_ih0", 0), B1=("w_ih1", 0), C0=("dx", 0))))
    dwe = "sed_gemm_pair_splitk_bf16x3" if bf and not dw_atomic else pair
    rows.append(dict(base, tag="dwi", entry=dwe, M=3 * H, N=I, K=BT, ta=1, tb=0, split=split, lda=6 * H, a1=3 * H, ldb=I, b1=0, ldc=I,
                     c1=None, sym=dict(A0=("dgi", 0), A1=("dgi", 12 * H), B0=("x", 0), B1=("x", 0), C0=("dwi0", 0), C1=("dwi1", 0))))
    rows.append(dict(base, tag="dwh", entry=dwe, M=3 * H, N=H, K=BT, ta=1, tb=0, split=split, lda=6 * H, a1=3 * H, ldb=2 * H, b1=H, ldc=H,
                     c1=None, sym=dict(A0=("dgh", 0), A1=("dgh", 12 * H), B0=("hprev", 0), B1=("hprev", 4 * H), C0=("dwh0", 0),
                                       C1=("dwh1", 0))))
    return rows


def embcat_rows(B, T, C=256, E=768):
    """(c): the GEMM calls of ops.EmbCatFn (forward, backward) on the default split-bf16 path."""
    M, W = B * T, C + E
    split = max(1, min(32, M // 256))
    base = dict(mixed=False, mis=(0, 0), ksplit=0, want=None, bias=False, acc=0, a1=None, b1=None, c1=None)
    return [dict(base, tag="y", entry="sed_gemm_bf16x3", M=M, N=C, K=W, ta=0, tb=1, split=1, bias=True, lda=W, ldb=W, ldc=C),
            dict(base, tag="dzx", entry="sed_gemm_bf16x3", M=M, N=C, K=C, ta=0, tb=0, split=1, lda=C, ldb=W, ldc=C),   # dy . W[:, :C]
            dict(base, tag="dw", entry="sed_gemm_splitk_bf16x3", M=C, N=W, K=M, ta=1, tb=0, split=split, lda=C, ldb=W, ldc=W)]


def case_table(dev, rows, first_seed=0):
    for i, row in enumerate(rows):
        run_row(dev, row, first_seed + i)


def case_scalar_paths(dev):
    lib = _lib.get()
    for i, row in enumerate(table_scalar()):
        prob, mir, outs = run_plain(dev, row, 300 + i)
        # the same arguments through sed_gemm_bf16x3: the operands miss its 16-byte requirements -> the f32 fall-back's bits
        r2 = dict(row, entry="sed_gemm_bf16x3")
        m2 = mirror(r2["entry"], row["M"], row["N"], row["K"], row["lda"], row["ldb"], row["ta"], row["tb"], row["split"], row["acc"],
                    prob.aligned())
        assert m2["kernel"] == "scalar", m2
        if mir["atomic"]:
            continue                      # (float atomics: no bit comparison)
        prob.new_outputs()
        prob.fill_c("canary")
        lib.call("sed_gemm_bf16x3", *call_args(r2, prob.ptrs(), stream(dev)))
        sync(dev)
        prob.assert_clean(describe(r2))
        assert torch.equal(prob.out(0).view(torch.int32), outs[0].view(torch.int32)), describe(r2) + ": not the f32 fall-back's bits"


def case_caller_rows(dev, bts, his, embcat=(), variants=("default", "dw_atomic", "f32")):
    """(c) numerically: every caller-shaped argument tuple on framed random operands.  variants: the default split-bf16 path with the
    deterministic split-K, its atomic weight-gradient fall-back (gru_dw_atomic), the exact-f32 path (SED_GEMM_PRECISION=f32).
    embcat: (B, T, C, E) of EmbCatFn."""
    seed = 500
    for (B, T) in bts:
        for (H, I) in his:
            sets = []
            if "default" in variants:
                sets.append(bigru_rows(B, T, I, H))
            if "dw_atomic" in variants:
                sets.append([r for r in bigru_rows(B, T, I, H, dw_atomic=True) if r["tag"].startswith("dw")])
            if "f32" in variants:
                sets.append(bigru_rows(B, T, I, H, prec="f32"))
            for rows in sets:
                for row in rows:
                    seed += 1
                    run_row(dev, row, seed)
    for (B, T, C, E) in embcat:
        for row in embcat_rows(B, T, C, E):
            seed += 1
            run_row(dev, row, seed)
        case_colsum(dev, shapes=((B * T, C, C, C, False),))


def required_instantiations():
    need = set()
    for ta, tb in LAYOUTS:
        for ntn in (2, 4):
            need.add(("bf16x3", ta, tb, ntn))
            need.add(("vec", ta, tb, ntn))
    return need


def case_tables_reach_every_instantiation():
    """Static: through the mirror, the rows' `want` cover gemm_bf16x3_kernel<ta,tb,{2,4}> and gemm_vec_kernel<ta,tb,{2,4}> for the three
    layouts, the scalar gemm_kernel, and splitk_reduce_kernel with gridDim.y 1 and 2.  (run_row asserts each `want` against the mirror.)"""
    seen, reduce_y, scalar = set(), set(), False
    for row in table_plain() + table_scalar() + table_splitk():
        w = row["want"]
        seen.add((w["kernel"], row["ta"], row["tb"], w["ntn"]))
        scalar = scalar or w["kernel"] == "scalar"
        if "reduce_y" in w:
            reduce_y.add(w["reduce_y"])
    missing = required_instantiations() - seen
    assert not missing, missing
    assert scalar and reduce_y == {1, 2}, (scalar, reduce_y)


# ---- BETA and the discrimination condition (no kernel involved) --------------------------------------------------------------------
def _host_problem(row, seed, max_rows=96):
    """opA(A), opB(B) of the row's first problem; the first 96 rows of the output (16 for K > 300: those rows never hold the largest
    r_ref, and the k-at-a-time chain is what costs time)."""
    prob = Problem("cpu", row, seed)
    a, b = prob.op(0)
    return a[:(max_rows if row["K"] <= 300 else 16)].contiguous(), b.contiguous()


def measure_r_ref(rows, max_rows=96):
    """-> largest r_ref = max |chain32 - model| / u over the rows (the first max_rows rows of each output)."""
    worst, per = 0.0, []
    for i, row in enumerate(rows):
        a, b = _host_problem(row, i, max_rows)
        split = row["entry"].endswith("bf16x3")
        S = a.abs().double() @ b.abs().double()
        target = split_model(a, b) if split else a.double() @ b.double()
        r = float(((chain32(a, b, split).double() - target).abs() / tier_b_unit(row["K"], S)).max())
        per.append((row["K"], split, r))
        worst = max(worst, r)
    return worst, per


def case_discrimination(rows, min_fraction=0.25):
    """For every split-bf16 row three mutants of the model -- lo*hi dropped, hi*lo dropped, the last 32-wide K tile of one slice
    dropped -- must exceed the tier-B bound in at least 25 % of the elements."""
    for i, row in enumerate(rows):
        if not row["entry"].endswith("bf16x3"):
            continue
        a, b = _host_problem(row, i)
        K = row["K"]
        S = a.abs().double() @ b.abs().double()
        bound = BETA * tier_b_unit(K, S)
        ah, al = bf16_parts(a)
        bh, bl = bf16_parts(b)
        kps, _ = slices_of(K, row["split"])
        k1 = min(K, kps)
        k0 = (k1 - 1) // 32 * 32                        # last K tile of slice 0
        tile = split_model(a[:, k0:k1], b[k0:k1])
        mutants = {"lo*hi dropped": al.double() @ bh.double(), "hi*lo dropped": ah.double() @ bl.double(), "a K tile dropped": tile}
        for name, delta in mutants.items():
            frac = float((delta.abs() > bound).double().mean())
            assert frac >= min_fraction, "%s: mutant '%s' is outside the tier-B bound in only %.0f %% of the elements" % (
                describe(row), name, 100 * frac)


# ---- (d) sed_colsum ----------------------------------------------------------------------------------------------------------------
COLSUM_SHAPES = ((0, 20, 24, 20, False), (1, 20, 24, 0, True), (63, 37, 40, 16, True), (64, 16, 16, 16, False), (65, 50, 64, 50, True),
                 (7488, 70, 76, 33, True), (7488, 768, 1152, 384, True))


def case_colsum(dev, shapes=COLSUM_SHAPES):
    """out[n] = sum_m X[m][n] (n < nsplit), out1[n - nsplit] (the rest) vs float64; |err| <= (M + 2) 2^-24 sum|x| (any order of M fp32
    additions); two runs bit-equal; frames intact."""
    lib = _lib.get()
    g = torch.Generator().manual_seed(77)
    for (M, N, ld, nsplit, with_out1) in shapes:
        X = torch.randn(M, N, generator=g) * 10.0 ** (torch.rand(N, generator=g) * 4 - 2)[None, :]
        fx = Frame(dev, M, ld, [(0, N)]).put(X) if M > 0 else Frame(dev, 0, ld, [(0, N)])
        snap = fx.bits()
        got = []
        for _ in range(2):
            o0 = vec_frame(dev, nsplit)
            o1 = vec_frame(dev, N - nsplit) if (with_out1 and N > nsplit) else None
            assert with_out1 or nsplit == N
            lib.call("sed_colsum", fx.ptr(), o0.ptr() if nsplit > 0 else None, o1.ptr() if o1 is not None else None, nsplit, M, N, ld,
                     stream(dev))
            sync(dev)
            o0.assert_frame("colsum out")
            if o1 is not None:
                o1.assert_frame("colsum out1")
            parts = [o0.get().flatten()[:nsplit]] + ([o1.get().flatten()] if o1 is not None else [])
            got.append(torch.cat(parts))
        assert torch.equal(fx.bits(), snap), "colsum changed its input"
        assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), ("colsum: two runs differ", M, N)
        ref = X.double().sum(0)
        bound = (M + 2) * U24 * X.double().abs().sum(0)
        assert ((got[0].double() - ref).abs() <= bound).all(), ("colsum", M, N, float((got[0].double() - ref).abs().max()))


# ---- (e) arena kernels -------------------------------------------------------------------------------------------------------------
ARENA_SIZES = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1112420, 2048 * 256 + 3)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def case_adam(dev, sizes=ARENA_SIZES, steps=3, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """sed_adam_step vs a float64 restatement of torch.optim.Adam (no weight decay / amsgrad) that takes the scalars as the entry
    receives them (fp32 values; 1 - b is exact in fp32 for b >= 0.5).
    Bound, from adam_kernel's operations with u = 2^-24 (each fp32 operation: relative error u):
      g s: 1 u;  m' = m b1 + (1 - b1) g: 3 u of Mm = |m| b1 + (1 - b1)|g| per step  ->  |dm| <= 3 t u Mm after t steps (Mm carried the same way);
      v' = v b2 + (1 - b2) g g: 4 u per step                                        ->  |dv| <= 4 t u v;
      denom = sqrt(v') ibc + eps: half of v's error + sqrt, product, sum            ->  (2 t + 3) u denom;
      p' = p - step (m' / denom): quotient 1 u, product 1 u, difference u |p'|      ->  per step u |p| + step (5 t + 6) u Mm / denom,
    summed over the steps; asserted with a factor 2 for the grad_scale product, the second-order terms and for evaluating the bound at
    the float64 trajectory."""
    lib = _lib.get()
    b1, b2, e32 = f32(betas[0]), f32(betas[1]), f32(eps)
    for n in sizes:
        for gscale in (1.0, 0.5):
            if n > 300 and gscale != 1.0 and n != 2048 * 256 + 3:
                continue
            g = torch.Generator().manual_seed(n % 1000 + int(gscale * 10))
            p0 = torch.randn(n, generator=g)
            grads = []
            for s in range(steps):
                gr = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 6 - 4)
                gr[::5] = 0.0                                   # exact zeros: v = 0 on those elements at step 1 (the eps path)
                grads.append(gr)
            results = []
            for device_hyper in (False, True):
                fp, fm, fv = vec_frame(dev, n).put(p0[None]), vec_frame(dev, n).fill(0.0), vec_frame(dev, n).fill(0.0)
                hyper = torch.zeros(2, device=dev)
                for s in range(steps):
                    fg = vec_frame(dev, n).put(grads[s][None])
                    gsnap = fg.bits()
                    step_size, ibc = lr / (1.0 - betas[0] ** (s + 1)), 1.0 / math.sqrt(1.0 - betas[1] ** (s + 1))
                    if device_hyper:
                        hyper.copy_(torch.tensor([step_size, ibc], dtype=torch.float32))
                        lib.call("sed_adam_step", fp.ptr(), fg.ptr(), fm.ptr(), fv.ptr(), n, b1, b2, e32, 123.0, 456.0, gscale,
                                 hyper.data_ptr(), stream(dev))
                    else:
                        lib.call("sed_adam_step", fp.ptr(), fg.ptr(), fm.ptr(), fv.ptr(), n, b1, b2, e32, step_size, ibc, gscale, None,
                                 stream(dev))
                    sync(dev)
                    assert torch.equal(fg.bits(), gsnap), "adam changed the gradient"
                for f, nm in ((fp, "p"), (fm, "m"), (fv, "v")):
                    f.assert_frame("adam n=%d %s" % (n, nm))
                results.append([f.get().flatten() for f in (fp, fm, fv)])
            for a, b in zip(*results):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("adam: by-value and device-resident hyper-parameters differ", n)
            # float64 restatement + the bound
            p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            Mm, bound = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            for s in range(steps):
                t = s + 1
                step_size, ibc = f32(lr / (1.0 - betas[0] ** t)), f32(1.0 / math.sqrt(1.0 - betas[1] ** t))
                gi = grads[s].double() * gscale
                m = m * b1 + (1.0 - b1) * gi
                Mm = Mm * b1 + (1.0 - b1) * gi.abs()
                v = v * b2 + (1.0 - b2) * gi * gi
                denom = v.sqrt() * ibc + e32
                bound += U24 * p.abs() + step_size * (5 * t + 6) * U24 * Mm / denom
                p = p - step_size * (m / denom)
            gp, gm, gv = [x.double() for x in results[0]]
            assert ((gp - p).abs() <= 2 * bound + 1e-300).all(), ("adam p", n, gscale, float(((gp - p).abs() / (2 * bound + 1e-300)).max()))
            assert ((gm - m).abs() <= 2 * 3 * steps * U24 * Mm + 1e-300).all(), ("adam m", n, gscale)
            assert ((gv - v).abs() <= 2 * 4 * steps * U24 * v + 1e-300).all(), ("adam v", n, gscale)
            assert (gv[::5] == 0).all() and (gp[::5] == p0[::5].double()).all(), "zero gradients must leave p alone (v = 0: the eps path)"


def case_ema(dev, sizes=ARENA_SIZES, steps=3, alpha=0.999):
    """sed_ema_update vs float64 on the fp32 scalars the entry receives.  t' = t a + (1 - a) s is two products and a sum: per step
    |dt'| <= a |dt| + 2 u (a |t| + (1 - a) |s|) (asserted with 1 % slack for the second-order terms)."""
    lib = _lib.get()
    for n in sizes:
        g = torch.Generator().manual_seed(n % 997)
        t0 = torch.randn(n, generator=g)
        results = []
        for device_alpha in (False, True):
            ft = vec_frame(dev, n).put(t0[None])
            g2 = torch.Generator().manual_seed(5)
            ref, bound = t0.double(), torch.zeros(n, dtype=torch.float64)
            for s in range(steps):
                a = 1.0 - 1.0 / (s + 2) if s < steps - 1 else alpha            # the warm-up values of update_ema, then the plateau
                a32, o32 = f32(a), f32(1.0 - a)
                sv = torch.randn(n, generator=g2) * 10.0 ** (torch.rand(n, generator=g2) * 4 - 2)
                fs = vec_frame(dev, n).put(sv[None])
                ssnap = fs.bits()
                if device_alpha:
                    ad = torch.tensor([a32, o32], dtype=torch.float32).to(dev)
                    lib.call("sed_ema_update", ft.ptr(), fs.ptr(), n, 9.0, -9.0, ad.data_ptr(), stream(dev))
                else:
                    lib.call("sed_ema_update", ft.ptr(), fs.ptr(), n, a32, o32, None, stream(dev))
                sync(dev)
                assert torch.equal(fs.bits(), ssnap), "ema changed the student"
                bound = a32 * bound + 2 * U24 * (a32 * ref.abs() + abs(o32) * sv.double().abs())
                ref = ref * a32 + o32 * sv.double()
            ft.assert_frame("ema n=%d teacher" % n)
            got = ft.get().flatten()
            assert ((got.double() - ref).abs() <= 1.01 * bound + 1e-300).all(), ("ema", n, float((got.double() - ref).abs().max()))
            results.append(got)
        assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32)), ("ema: by-value and device-resident alpha differ", n)


def case_zero_buffers(dev):
    lib = _lib.get()
    lens = (1, 255, 700, 257)
    fs = [vec_frame(dev, n).fill(5.0) for n in lens]
    lib.call("sed_zero_buffers", fs[0].ptr(), lens[0], fs[1].ptr(), lens[1], fs[2].ptr(), lens[2], fs[3].ptr(), lens[3], stream(dev))
    sync(dev)
    for f in fs:
        f.assert_frame("zero_buffers")
        assert (f.get() == 0).all()
    # a prefix only; null and zero-length entries are skipped
    fa, fb = vec_frame(dev, 600).fill(5.0), vec_frame(dev, 9).fill(5.0)
    lib.call("sed_zero_buffers", None, 0, fa.ptr(), 300, None, 40, fb.ptr(), 0, stream(dev))
    sync(dev)
    fa.assert_frame("zero_buffers")
    fb.assert_frame("zero_buffers")
    assert (fa.get().flatten()[:300] == 0).all() and (fa.get().flatten()[300:] == 5.0).all() and (fb.get() == 5.0).all()
    # a count that does not fit the kernel's int index: rejected before any launch (it used to turn negative: nothing was zeroed, rc 0)
    fc = vec_frame(dev, 4).fill(5.0)
    for pos in range(4):
        args = [None, 0] * 4
        args[2 * pos], args[2 * pos + 1] = fc.ptr(), 2 ** 31
        assert rc("sed_zero_buffers", *args, stream(dev)) == SED_ERR_UNSUPPORTED
    sync(dev)
    assert (fc.get() == 5.0).all()
    fc.assert_frame("zero_buffers")


def case_ema_alignment_contract(dev):
    """n >= 4 on a buffer that is not 16-byte aligned: SED_ERR_ARG (float4 accesses), nothing written; n < 4: legal at any alignment."""
    ft, fs = vec_frame(dev, 8, misalign=1).fill(1.0), vec_frame(dev, 8).fill(3.0)
    fa = vec_frame(dev, 8).fill(1.0)
    assert rc("sed_ema_update", ft.ptr(), fs.ptr(), 8, 0.5, 0.5, None, stream(dev)) == SED_ERR_ARG
    assert rc("sed_ema_update", fa.ptr(), ft.ptr(), 4, 0.5, 0.5, None, stream(dev)) == SED_ERR_ARG
    sync(dev)
    assert (ft.get() == 1.0).all() and (fa.get() == 1.0).all()
    for n in (1, 2, 3):
        ft = vec_frame(dev, 8, misalign=1).fill(1.0)
        assert rc("sed_ema_update", ft.ptr(), fs.ptr(), n, 0.5, 0.5, None, stream(dev)) == 0
        sync(dev)
        ft.assert_frame("ema tail-only")
        assert (ft.get().flatten()[:n] == 2.0).all() and (ft.get().flatten()[n:] == 1.0).all()


def _adam64(params, lr, betas, eps):
    return torch.optim.Adam([torch.nn.Parameter(p.detach().double().cpu().clone()) for p in params], lr=lr, betas=betas, eps=eps)


def case_fused_adam_host(dev, steps=14, lr=1e-3):
    """arena.FusedAdam vs float64 torch.optim.Adam over 14 steps: flat (one launch) -> per-tensor -> state_dict() / load_state_dict()
    -> flat again; step, exp_avg, exp_avg_sq and the parameters compared at the end.
    Tolerances: the kernel takes b2 as fp32 (0.999f: 1 - b2 is 1.3e-5 off in relative terms), so exp_avg_sq may differ by 2e-5 relative
    and an update (|m / (sqrt(v) + eps)| <= (1 - b1) / sqrt(1 - b2) < 3.2) by 3.2 lr 1e-5 per step; exp_avg: b1 as fp32 (3e-8) + 3 u per step."""
    from desed_task_amd.arena import FusedAdam, ParamArena
    g = torch.Generator().manual_seed(3)
    shapes = ((5, 3), (7,), (3,), (16, 16), (1,), (2, 3, 4))
    params = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    arena = ParamArena(params)
    opt = FusedAdam(params, lr=lr, arena=arena)
    ref = _adam64(params, lr, (0.9, 0.999), 1e-8)
    rparams = ref.param_groups[0]["params"]
    launches = []
    lib = _lib.get()
    orig = lib.call

    def spy(name, *a):
        if name == "sed_adam_step":
            launches.append(a[4])
        return orig(name, *a)
    lib.call = spy
    try:
        for s in range(steps):
            mode = "flat" if s < 4 or s >= 10 else "tensor"
            if s == 8:                                   # round trip through torch.optim.Adam's state-dict layout
                sd = opt.state_dict()
                assert all(float(st["step"]) == s for st in sd["state"].values())
                opt = FusedAdam(params, lr=lr, arena=arena)
                opt.load_state_dict(sd)
            before = len(launches)
            for p, rp in zip(params, rparams):
                gr = torch.randn(p.shape, generator=g) * 10.0 ** float(torch.rand((), generator=g) * 4 - 3)
                rp.grad = gr.double()
                if mode == "flat":
                    p.grad = None
                    p.grad = arena.grad_view_for(p)
                    p.grad.copy_(gr)
                else:
                    p.grad = gr.to(dev)
            assert arena.grads_are_flat() == (mode == "flat")
            opt.step()
            ref.step()
            sync(dev)
            assert len(launches) - before == (1 if mode == "flat" else len(params)), (s, mode, launches[before:])
    finally:
        lib.call = orig
    sd = opt.state_dict()
    for i, (p, rp) in enumerate(zip(params, rparams)):
        st, rst = sd["state"][i], ref.state[rp]
        assert float(st["step"]) == float(rst["step"]) == steps
        m, v = st["exp_avg"].cpu().double(), st["exp_avg_sq"].cpu().double()
        assert ((m - rst["exp_avg"]).abs() <= 1e-6 * rst["exp_avg"].abs() + 1e-6 * float(rst["exp_avg"].abs().max())).all(), i
        assert ((v - rst["exp_avg_sq"]).abs() <= 2e-5 * rst["exp_avg_sq"]).all(), i
        tol = steps * (3.2 * lr * 1e-5 + 4 * U24 * rp.detach().abs())
        assert ((p.detach().cpu().double() - rp.detach()).abs() <= tol).all(), (i, float((p.detach().cpu().double() - rp.detach()).abs().max()))


def case_ema_host(dev):
    """arena.ema_update_ through the one-launch arena route and the per-tensor route (incl. a 3-element tensor at an address that is not
    16-byte aligned: the tail-only form), vs float64; a longer unaligned tensor is a RuntimeError."""
    from desed_task_amd.arena import ParamArena, ema_update_
    g = torch.Generator().manual_seed(9)
    shapes = ((5, 3), (7,), (3,), (16, 16), (1,))
    mk = lambda: [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]      # noqa: E731
    alpha = 0.99
    a32, o32 = f32(alpha), f32(1.0 - alpha)
    for route in ("arena", "tensor"):
        teacher, student = mk(), mk()
        want = [t.detach().cpu().double() * a32 + o32 * s.detach().cpu().double() for t, s in zip(teacher, student)]
        if route == "arena":
            ta, sa = ParamArena(teacher), ParamArena(student)
            assert ema_update_(teacher, student, alpha, ta, sa) == 1
        else:
            store = torch.zeros(8, device=dev)
            odd = torch.nn.Parameter(store[1:4])
            store2 = torch.ones(8, device=dev)
            odd_s = torch.nn.Parameter(store2[1:4])
            assert odd.data_ptr() % 16 == 4
            teacher.append(odd)
            student.append(odd_s)
            want.append(torch.full((3,), float(o32), dtype=torch.float64))
            assert ema_update_(teacher, student, alpha) == len(teacher)
            sync(dev)
            assert store[0] == 0 and (store[4:] == 0).all()
        sync(dev)
        for t, w in zip(teacher, want):
            assert ((t.detach().cpu().double() - w).abs() <= 3 * U24 * (w.abs() + 1e-30) + 2 * U24 * 1.0).all(), route
    store = torch.zeros(12, device=dev)
    long_t, long_s = torch.nn.Parameter(store[1:6]), torch.nn.Parameter(torch.ones(12, device=dev)[1:6])
    try:
        ema_update_([long_t], [long_s], alpha)
    except RuntimeError as e:
        assert "unaligned" in str(e)
    else:
        raise AssertionError("ema_update_ accepted a 5-element tensor that is not 16-byte aligned")


# ---- (f) error contract -------------------------------------------------------------------------------------------------------------
def case_error_contract(dev):
    """Every documented rejection of these entries returns its code before any launch and leaves all canaries intact."""
    st = stream(dev)
    pk, sk, kc = "sed_gemm_pair_splitk_bf16x3", "sed_gemm_splitk_bf16x3", "sed_gemm_kcat_splitk_bf16x3"

    def attempt(row, want_rc, what, mutate=None, scratch=True, seed=900):
        prob = Problem(dev, row, seed)
        prob.fill_c("canary")
        scr = vec_frame(dev, 4096) if "splitk" in row["entry"] else None
        P = prob.ptrs()
        r2 = dict(row)
        if mutate:
            mutate(P, r2)
        got = rc(row["entry"], *call_args(r2, P, st, scr.ptr() if (scr is not None and scratch) else None))
        sync(dev)
        assert got == want_rc, (what, row["entry"], got, want_rc)
        for f in {id(f): f for f, _ in prob.fC}.values():
            assert (f.bits() == CANARY_BITS).all(), what + ": C written"
        if scr is not None:
            assert (scr.bits() == CANARY_BITS).all(), what + ": scratch written"
        for k, f in prob.inputs.items():
            assert torch.equal(f.bits(), prob.snap[k]), what

    def bump(key, by):
        def f(P, r):
            P[key] += by
        return f

    def setrow(**kw):
        def f(P, r):
            r.update(kw)
        return f
    for e in (pk, sk, kc):
        ks = dict(ksplit=32) if e == kc else {}
        ta = 0 if e == kc else 1
        ok = G(e, 36, 8, 64, ta, 0, split=2, bias=False, pad=(0, 0, 4), **ks)
        attempt(G(e, 36, 6, 64, ta, 0, split=2, bias=False, pad=(0, 0, 2), **ks), SED_ERR_ARG, "N % 4")
        attempt(G(e, 36, 8, 64, ta, 0, split=2, bias=False, pad=(0, 0, 1), **ks), SED_ERR_ARG, "ldc % 4")
        attempt(ok, SED_ERR_UNSUPPORTED, "misaligned C", bump("C0", 4))
        attempt(ok, SED_ERR_ARG, "null scratch", scratch=False)
        attempt(ok, SED_ERR_UNSUPPORTED, "unaligned A with dense partials", bump("A0", 4))
        attempt(ok, SED_ERR_UNSUPPORTED, "unaligned B with dense partials", bump("B0", 4))
        attempt(ok, SED_ERR_UNSUPPORTED, "odd lda with dense partials", setrow(lda=ok["lda"] + 1))
        if e == pk:
            attempt(ok, SED_ERR_UNSUPPORTED, "misaligned C1", bump("C1", 8))
            attempt(ok, SED_ERR_UNSUPPORTED, "unaligned A1", bump("A1", 4))
        if e != kc:
            attempt(ok, SED_ERR_ARG, "K = 0", setrow(K=0))
            attempt(ok, SED_ERR_UNSUPPORTED, "transA = transB = 1", setrow(ta=1, tb=1))
    for e in (kc, "sed_gemm_kcat_bf16x3", "sed_gemm_kcat"):
        ok = G(e, 36, 8, 64, 0, 0, split=2, bias=False, ksplit=32)
        attempt(ok, SED_ERR_ARG, "ksplit % 32", setrow(ksplit=16))
        attempt(ok, SED_ERR_ARG, "ksplit = 0", setrow(ksplit=0))
        attempt(ok, SED_ERR_ARG, "ksplit = K", setrow(ksplit=64))
        attempt(ok, SED_ERR_ARG, "ksplit > K", setrow(ksplit=96))
        if e != kc:
            attempt(ok, SED_ERR_UNSUPPORTED, "unaligned A with a K-concatenated B", bump("A0", 4))
    for e in ("sed_gemm", "sed_gemm_bf16x3", "sed_gemm_pair", "sed_gemm_pair_bf16x3"):
        attempt(G(e, 36, 8, 64, 0, 0), SED_ERR_UNSUPPORTED, "transA = transB = 1", setrow(ta=1, tb=1))
    # sed_colsum
    fx, o0 = Frame(dev, 8, 12, [(0, 12)]).fill(1.0), vec_frame(dev, 12)
    assert rc("sed_colsum", fx.ptr(), o0.ptr(), None, 13, 8, 12, 12, st) == SED_ERR_ARG          # nsplit > N
    assert rc("sed_colsum", fx.ptr(), o0.ptr(), None, 5, 8, 12, 12, st) == SED_ERR_ARG           # columns for out1, out1 null
    sync(dev)
    assert (o0.bits() == CANARY_BITS).all()
