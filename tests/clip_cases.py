"""Cases for gradient-norm clipping inside the fused optimizer step (csrc/sed_optim.hip: sed_grad_sqnorm, sed_adam_step_clipped;
arena.FusedAdam(max_grad_norm=...); the `training.gradient_clip` key through launcher.StepDriver, graph.GraphedStepDriver and
SEDTask4.configure_gradient_clipping).  Device-agnostic like contraction_cases.py / parity_cases.py: dev = "cpu" on the fiber
emulator (tests/test_emu_clip.py), "cuda" on the MI355X (tests/test_gpu_step_clip.py).

Semantics under test: torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) as Lightning 1.9 applies `gradient_clip_val`,
    total = || grad_scale g ||_2,  coef = min(1, max_norm / (total + 1e-6)),  Adam consumes g grad_scale coef.

Adam is almost blind to a uniform scale of its gradient (m / sqrt(v)): a forgotten coef moves the parameters by next to nothing.  Every
comparison here therefore includes exp_avg (linear in coef) and exp_avg_sq (quadratic), never the parameters alone.

The error model (u = 2^-24), from the addition order include/sed_hip.h documents for sed_grad_sqnorm and the constants it exports:
a sum of non-negative terms through an addition chain of depth d has relative error <= (d + 1) u (one rounding per addition, one for
the square -- the kernel fuses square and addition into one FMA, which only removes roundings), with
    d_partial(n) = 4 ceil(n4 / (G T)) + n % 4  +  6  +  (T / 64 - 1)          lane's serial adds, butterfly levels, LDS combine
    d(n)         = d_partial(n)  +  6  +  (P / 64 - 1)                        ... + the consumer's combine over the P partials
n4 = n // 4, T = SED_SQNORM_THREADS, P = SED_SQNORM_MAX_PARTIALS, G = min(P, max(1, ceil(n4 / T))) workgroups.
total = gscale sqrt(sum): half the sum's error + 1 (gscale is a power of two in these cases: exact);
coef = max_norm / (total + 1e-6): + the sum with 1e-6 and the quotient  ->  e_coef = ((d + 1) / 2 + 3) u.
As in contraction_cases.case_adam every bound is asserted with a factor 2 (second-order terms, the bound evaluated at the float64
trajectory).
"""
import math

import torch

from desed_task_amd import _lib
from tests.contraction_cases import ARENA_SIZES, U24, f32, stream, sync, vec_frame


def consts():
    c = _lib.header_constants()
    return c["SED_SQNORM_THREADS"], c["SED_SQNORM_MAX_PARTIALS"]


def sqnorm_grid(n):
    T, P = consts()
    return min(P, max(1, -(-(n // 4) // T)))


def depth_partial(n):
    T, P = consts()
    G = sqnorm_grid(n)
    return 4 * -(-(n // 4) // (G * T)) + n % 4 + 6 + (T // 64 - 1)


def depth(n):
    T, P = consts()
    return depth_partial(n) + 6 + (P // 64 - 1)


def e_coef(n):
    """Relative error of the kernel's clip coefficient (module docstring)."""
    return ((depth(n) + 1) / 2 + 3) * U24


def spread_grad(n, gen):
    """case_adam's gradients: magnitudes over 10^(-4 .. 2), every fifth element an exact zero (from element 2 on, so that the
    shortest vectors keep a non-zero norm for the thresholds to be taken from)."""
    gr = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 6 - 4)
    gr[2::5] = 0.0
    return gr


def partial_refs(gr):
    """float64 sum of squares of the elements each workgroup owns (the order sed_hip.h documents)."""
    T, P = consts()
    n = gr.numel()
    n4, G = n // 4, sqnorm_grid(n)
    sq = gr.double() ** 2
    ref = torch.zeros(P, dtype=torch.float64)
    if n4:
        owner = (torch.arange(n4) // T) % G
        ref.index_add_(0, owner, sq[:4 * n4].view(n4, 4).sum(1))
    ref[0] += sq[4 * n4:].sum()
    return ref


# ---- 1: the norm kernel ----------------------------------------------------------------------------------------------------------
def case_sqnorm(dev, sizes=ARENA_SIZES):
    """sed_grad_sqnorm on canary-framed operands vs float64.  Per workgroup: |partial - ref| <= 2 (d_partial + 1) u ref; slots beyond the
    grid are exact zeros; the float64 sum of the partials is within 2 (d_partial + 1) u of the float64 sum of squares (the consumer's
    combine, d - d_partial more levels, is checked through clip_out in case_adam_clipped).  Two calls give equal bits, the canaries
    survive, the gradient is only read.  Misaligned gradient with n >= 4: SED_ERR_ARG and nothing written; n < 4: legal."""
    lib = _lib.get()
    T, P = consts()
    for n in sizes:
        gen = torch.Generator().manual_seed(n % 1000 + 17)
        gr = spread_grad(n, gen)
        fg = vec_frame(dev, n).put(gr[None])
        gsnap = fg.bits()
        outs = []
        for rep in range(2):
            fp = vec_frame(dev, P).fill(7.0)          # (stale contents: every slot must be overwritten)
            lib.call("sed_grad_sqnorm", fg.ptr(), n, fp.ptr(), stream(dev))
            sync(dev)
            fp.assert_frame("sqnorm n=%d partials" % n)
            outs.append(fp.get().flatten())
        fg.assert_frame("sqnorm n=%d gradient" % n)
        assert torch.equal(fg.bits(), gsnap), "sqnorm changed the gradient"
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), ("sqnorm: two calls differ", n)
        got, ref = outs[0].double(), partial_refs(gr)
        G = sqnorm_grid(n)
        assert (outs[0][G:] == 0).all() and (outs[0][G:].view(torch.int32) == 0).all(), ("slots beyond the grid", n, G)
        rel = 2 * (depth_partial(n) + 1) * U24
        worst = float(((got - ref).abs() / (rel * ref + 1e-300)).max())
        print("sqnorm n=%d G=%d d_partial=%d d=%d  worst |err| / bound = %.3f" % (n, G, depth_partial(n), depth(n), worst))
        assert ((got - ref).abs() <= rel * ref + 1e-300).all(), ("sqnorm partial", n, worst)
        assert abs(float(got.sum()) - float((gr.double() ** 2).sum())) <= rel * float((gr.double() ** 2).sum()), ("sqnorm total", n)
    # alignment contract (sed_ema_update's)
    fm, fp = vec_frame(dev, 8, misalign=1).fill(2.0), vec_frame(dev, P).fill(7.0)
    rc = getattr(lib._dll, "sed_grad_sqnorm")
    assert rc(fm.ptr(), 8, fp.ptr(), stream(dev)) == -1
    sync(dev)
    assert (fp.get() == 7.0).all()
    for n in (1, 2, 3):
        assert rc(fm.ptr(), n, fp.ptr(), stream(dev)) == 0
        sync(dev)
        got = fp.get().flatten()
        assert got[0] == 4.0 * n and (got[1:] == 0).all(), (n, got[:4])
    fp.assert_frame("sqnorm tail-only")


# ---- 2: the clipped Adam kernel ----------------------------------------------------------------------------------------------------
def _norm64(gr, gscale):
    return abs(gscale) * math.sqrt(float((gr.double() ** 2).sum()))


def _run_kernel(dev, n, p0, grads, gscale, max_norms, lr, betas, eps, device_hyper, clipped=True):
    """`steps` launches of sed_grad_sqnorm + sed_adam_step_clipped (or of sed_adam_step) from zero moments -> (p, m, v, [clip_out per step])."""
    lib = _lib.get()
    T, P = consts()
    b1, b2, e32 = f32(betas[0]), f32(betas[1]), f32(eps)
    fp, fm, fv = vec_frame(dev, n).put(p0[None]), vec_frame(dev, n).fill(0.0), vec_frame(dev, n).fill(0.0)
    fpart, fclip = vec_frame(dev, P).fill(7.0), vec_frame(dev, 2).fill(7.0)
    hyper = torch.zeros(2, device=dev)
    clips = []
    for s, gr in enumerate(grads):
        fg = vec_frame(dev, n).put(gr[None])
        gsnap = fg.bits()
        step_size, ibc = lr / (1.0 - betas[0] ** (s + 1)), 1.0 / math.sqrt(1.0 - betas[1] ** (s + 1))
        by_value = (123.0, 456.0) if device_hyper else (step_size, ibc)
        if device_hyper:
            hyper.copy_(torch.tensor([step_size, ibc], dtype=torch.float32))
        hptr = hyper.data_ptr() if device_hyper else None
        if clipped:
            lib.call("sed_grad_sqnorm", fg.ptr(), n, fpart.ptr(), stream(dev))
            lib.call("sed_adam_step_clipped", fp.ptr(), fg.ptr(), fm.ptr(), fv.ptr(), n, b1, b2, e32, by_value[0], by_value[1], gscale,
                     hptr, fpart.ptr(), f32(max_norms[s]), fclip.ptr(), stream(dev))
        else:
            lib.call("sed_adam_step", fp.ptr(), fg.ptr(), fm.ptr(), fv.ptr(), n, b1, b2, e32, by_value[0], by_value[1], gscale, hptr,
                     stream(dev))
        sync(dev)
        assert torch.equal(fg.bits(), gsnap), "the step changed the gradient"
        fg.assert_frame("clipped adam n=%d gradient" % n)
        clips.append(fclip.get().flatten().clone())
    for f, nm in ((fp, "p"), (fm, "m"), (fv, "v"), (fpart, "partials"), (fclip, "clip_out")):
        f.assert_frame("clipped adam n=%d %s" % (n, nm))
    return [f.get().flatten() for f in (fp, fm, fv)], clips


def case_adam_clipped(dev, sizes=ARENA_SIZES, steps=3, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """sed_grad_sqnorm + sed_adam_step_clipped vs contraction_cases.case_adam's float64 restatement of torch.optim.Adam with the gradient
    scale gscale coef64, coef64 = min(1, max_norm / (gscale ||g||_2 + 1e-6)) in float64 (1e-6 and max_norm as fp32 values).
    Bounds: case_adam's, with the gradient's relative error raised by e = e_coef(n) (module docstring):
      m' = m b1 + (1 - b1) g:      |dm| <= t (3 u + e) Mm
      v' = v b2 + (1 - b2) g g:    |dv| <= t (4 u + 2 e) v
      denom: half of v's + 3 u;  p' = p - step m' / denom:  per step u |p| + step ((5 t + 6) u + 2 t e) Mm / denom
    each asserted with case_adam's factor 2.  clip_out: |total - total64| <= 2 ((d + 1) / 2 + 1) u total64, |coef - coef64| <= 2 e coef64.
    Thresholds from the float64 norm of each step's gradient, so the branch is certain: 0.5 x (clips: coef ~ 0.5) and 2 x (never clips:
    coef == 1.0f exactly and p, m, v BIT-IDENTICAL to sed_adam_step with the same grad_scale).  By-value and device-resident
    hyper-parameters give equal bits.  grad_scale 0.5: the norm is that of the scaled gradient."""
    b1, b2, e32 = f32(betas[0]), f32(betas[1]), f32(eps)
    eps_n = f32(1e-6)
    for n in sizes:
        for gscale in (1.0, 0.5):
            if n > 300 and gscale != 1.0 and n != 2048 * 256 + 3:
                continue
            gen = torch.Generator().manual_seed(n % 1000 + int(gscale * 10) + 3)
            p0 = torch.randn(n, generator=gen)
            grads = [spread_grad(n, gen) for _ in range(steps)]
            norms = [_norm64(gr, gscale) for gr in grads]
            e = e_coef(n)
            for factor in (0.5, 2.0):
                max_norms = [f32(factor * t) for t in norms]
                results = [_run_kernel(dev, n, p0, grads, gscale, max_norms, lr, betas, eps, dh) for dh in (False, True)]
                for a, b in zip(results[0][0], results[1][0]):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("clipped adam: by-value / device hyper differ", n)
                (gp, gm, gv), clips = results[0]
                if factor > 1:
                    plain, _ = _run_kernel(dev, n, p0, grads, gscale, max_norms, lr, betas, eps, False, clipped=False)
                    for a, b, nm in zip((gp, gm, gv), plain, "pmv"):
                        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("inactive clip must equal sed_adam_step", n, gscale, nm)
                    assert all(float(c[1]) == 1.0 for c in clips), clips
                p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
                Mm, bound = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
                for s in range(steps):
                    t = s + 1
                    coef64 = min(1.0, max_norms[s] / (norms[s] + eps_n))
                    tot_b, coef_b = 2 * ((depth(n) + 1) / 2 + 1) * U24 * norms[s], 2 * e * coef64
                    print("clipped adam n=%d gscale=%g factor=%g step %d: total %.9g (f64 %.9g, err/bound %.3f)  coef %.9g (f64 %.9g, err/bound %.3f)"
                          % (n, gscale, factor, t, float(clips[s][0]), norms[s], abs(float(clips[s][0]) - norms[s]) / tot_b,
                             float(clips[s][1]), coef64, abs(float(clips[s][1]) - coef64) / coef_b))
                    assert abs(float(clips[s][0]) - norms[s]) <= tot_b, ("clip_out total", n, gscale, s)
                    assert abs(float(clips[s][1]) - coef64) <= coef_b, ("clip_out coef", n, gscale, s)
                    assert (float(clips[s][1]) < 1.0) == (factor < 1), ("branch", n, factor, clips[s])
                    step_size, ibc = f32(lr / (1.0 - betas[0] ** t)), f32(1.0 / math.sqrt(1.0 - betas[1] ** t))
                    gi = grads[s].double() * (gscale * coef64)
                    m = m * b1 + (1.0 - b1) * gi
                    Mm = Mm * b1 + (1.0 - b1) * gi.abs()
                    v = v * b2 + (1.0 - b2) * gi * gi
                    denom = v.sqrt() * ibc + e32
                    bound += U24 * p.abs() + step_size * ((5 * t + 6) * U24 + 2 * t * e) * Mm / denom
                    p = p - step_size * (m / denom)
                gp, gm, gv = gp.double(), gm.double(), gv.double()
                assert ((gp - p).abs() <= 2 * bound + 1e-300).all(), ("clipped adam p", n, gscale, factor, float(((gp - p).abs() / (2 * bound + 1e-300)).max()))
                assert ((gm - m).abs() <= 2 * steps * (3 * U24 + e) * Mm + 1e-300).all(), ("clipped adam m", n, gscale, factor,
                                                                                          float(((gm - m).abs() / (2 * steps * (3 * U24 + e) * Mm + 1e-300)).max()))
                assert ((gv - v).abs() <= 2 * steps * (4 * U24 + 2 * e) * v + 1e-300).all(), ("clipped adam v", n, gscale, factor)
                assert (gv[2::5] == 0).all() and (gp[2::5] == p0[2::5].double()).all(), "zero gradients must leave p alone"


def case_adam_clipped_nonfinite(dev, n=1029, lr=1e-3):
    """A gradient holding one inf (total = inf, coef = 0: inf * 0 = NaN at that element, zero gradient elsewhere) and one holding a NaN
    (total = coef = NaN: everything NaN): p, exp_avg and exp_avg_sq are non-finite exactly where CPU clip_grad_norm_ +
    torch.optim.Adam make them so.  The value is planted in an ordinary buffer; nothing here faults."""
    for bad in (float("inf"), float("nan")):
        gen = torch.Generator().manual_seed(11)
        p0 = torch.randn(n, generator=gen)
        g0, g1 = spread_grad(n, gen), spread_grad(n, gen)
        g1[517] = bad
        ref_p = torch.nn.Parameter(p0.clone())
        ref = torch.optim.Adam([ref_p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
        for gr in (g0, g1):
            ref_p.grad = gr.clone()
            torch.nn.utils.clip_grad_norm_([ref_p], 0.5)
            ref.step()
        (gp, gm, gv), clips = _run_kernel(dev, n, p0, [g0, g1], 1.0, [0.5, 0.5], lr, (0.9, 0.999), 1e-8, False)
        st = ref.state[ref_p]
        for got, want, nm in ((gp, ref_p.detach(), "p"), (gm, st["exp_avg"], "exp_avg"), (gv, st["exp_avg_sq"], "exp_avg_sq")):
            assert torch.equal(torch.isfinite(got), torch.isfinite(want)), (bad, nm, int((~torch.isfinite(got)).sum()), int((~torch.isfinite(want)).sum()))
        nonfinite = int((~torch.isfinite(gm)).sum())
        assert nonfinite == (1 if math.isinf(bad) else n), (bad, nonfinite)
        tot, coef = float(clips[1][0]), float(clips[1][1])
        assert (math.isinf(tot) and coef == 0.0) if math.isinf(bad) else (math.isnan(tot) and math.isnan(coef)), (bad, tot, coef)


# ---- 3: arena.FusedAdam(max_grad_norm=...) -----------------------------------------------------------------------------------------
def case_fused_adam_clip_host(dev, steps=14, lr=1e-3):
    """FusedAdam(max_grad_norm=c) vs float64 clip_grad_norm_ + torch.optim.Adam on a fixed gradient sequence, through the round trip of
    contraction_cases.case_fused_adam_host: flat (norm launch + clipped launch) -> per-tensor (gradients outside the intact arena:
    gathered, ONE norm launch, one clipped launch per tensor) -> state_dict() / load_state_dict() -> flat again.  c = the geometric
    mean of the two middle norms of the sequence: about half the steps clip, and no norm lies within 1 % of c (asserted).
    `last_clip` vs the float64 norm / coef of every step within case_adam_clipped's clip_out bounds.
    Tolerances: case_fused_adam_host's (b1, b2 taken as fp32 by the kernel), each widened by 2 e -- the gradient's relative error from
    the coefficient, e = e_coef(arena floats), factor 2 as everywhere: exp_avg 1e-6 + 2 e (linear in coef), exp_avg_sq 2e-5 + 4 e
    (quadratic), an update 3.2 lr (1e-5 + 4 e) per step (m's error + half of v's).
    Then a FusedAdam without any arena (torch's arithmetic on the parameter list, per-tensor launches): same reference, 3 steps."""
    from desed_task_amd.arena import FusedAdam, ParamArena
    from tests.contraction_cases import _adam64
    gen = torch.Generator().manual_seed(3)
    shapes = ((5, 3), (7,), (3,), (16, 16), (1,), (2, 3, 4))
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
    grads = [[torch.randn(s, generator=gen) * 10.0 ** float(torch.rand((), generator=gen) * 4 - 3) for s in shapes] for _ in range(steps)]
    norms = [math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs)) for gs in grads]
    srt = sorted(norms)
    c = math.sqrt(srt[steps // 2 - 1] * srt[steps // 2])
    assert all(abs(t / c - 1) > 0.01 for t in norms), (c, norms)
    arena = ParamArena(params)
    opt = FusedAdam(params, lr=lr, arena=arena, max_grad_norm=c)
    assert opt.last_clip is None
    ref = _adam64(params, lr, (0.9, 0.999), 1e-8)
    rparams = ref.param_groups[0]["params"]
    e = e_coef(arena.numel)
    launches = []
    lib = _lib.get()
    orig = lib.call

    def spy(name, *a):
        if name in ("sed_adam_step", "sed_adam_step_clipped", "sed_grad_sqnorm"):
            launches.append(name)
        return orig(name, *a)
    lib.call = spy
    clip_ptr = None
    try:
        for s in range(steps):
            mode = "flat" if s < 4 or s >= 10 else "tensor"
            if s == 8:
                sd = opt.state_dict()
                opt = FusedAdam(params, lr=lr, arena=arena, max_grad_norm=c)
                opt.load_state_dict(sd)
            if s == 12:                                     # in place: the clip buffer (a captured graph holds its address) survives
                opt.load_state_dict(opt.state_dict())
                assert opt._clip_buf.data_ptr() == clip_ptr
            before = len(launches)
            for p, rp, gr in zip(params, rparams, grads[s]):
                rp.grad = gr.double()
                if mode == "flat":
                    p.grad = None
                    p.grad = arena.grad_view_for(p)
                    p.grad.copy_(gr)
                else:
                    p.grad = gr.to(dev)
            snap = [p.grad.detach().cpu().clone() for p in params]
            opt.step()
            torch.nn.utils.clip_grad_norm_(rparams, c)
            ref.step()
            sync(dev)
            clip_ptr = opt._clip_buf.data_ptr()
            for p, g0 in zip(params, snap):
                assert torch.equal(p.grad.detach().cpu(), g0), "FusedAdam must not rewrite p.grad"
            want = ["sed_grad_sqnorm"] + ["sed_adam_step_clipped"] * (1 if mode == "flat" else len(params))
            assert launches[before:] == want, (s, mode, launches[before:])
            tot, coef = [float(x) for x in opt.last_clip.cpu()]
            coef64 = min(1.0, c / (norms[s] + f32(1e-6)))
            assert abs(tot - norms[s]) <= 2 * ((depth(arena.numel) + 1) / 2 + 1) * U24 * norms[s], (s, tot, norms[s])
            assert abs(coef - coef64) <= 2 * e * coef64 + 2 * U24 * coef64, (s, coef, coef64)     # (+ max_norm taken as fp32)
            assert (coef < 1.0) == (norms[s] > c), (s, coef, norms[s], c)
    finally:
        lib.call = orig
    assert 4 <= sum(t > c for t in norms) <= steps - 4
    _compare_with_adam64(opt, params, ref, rparams, steps, lr, e)
    # pad lanes of the gradient arena never enter the norm: they are zeros
    assert_pad_lanes_zero(arena)
    # no arena at all
    params2 = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
    opt2 = FusedAdam(params2, lr=lr, max_grad_norm=c)
    ref2 = _adam64(params2, lr, (0.9, 0.999), 1e-8)
    for s in range(3):
        for p, rp, gr in zip(params2, ref2.param_groups[0]["params"], grads[steps // 2 + s]):
            rp.grad = gr.double()
            p.grad = gr.to(dev)
        opt2.step()
        torch.nn.utils.clip_grad_norm_(ref2.param_groups[0]["params"], c)
        ref2.step()
        sync(dev)
        tot, coef = [float(x) for x in opt2.last_clip.cpu()]
        assert abs(tot - norms[steps // 2 + s]) <= 1e-6 * tot and (coef < 1.0) == (norms[steps // 2 + s] > c)
    _compare_with_adam64(opt2, params2, ref2, ref2.param_groups[0]["params"], 3, lr, e)
    # adopt() leaves clipping off
    plain = torch.optim.Adam(params2, lr=lr)

    class Holder:
        pass
    h = Holder()
    h.arena, h.parameters = None, lambda: iter(params2)
    assert FusedAdam.adopt(plain, h) and plain.max_grad_norm is None and plain.last_clip is None


def _compare_with_adam64(opt, params, ref, rparams, steps, lr, e):
    sd = opt.state_dict()
    for i, (p, rp) in enumerate(zip(params, rparams)):
        st, rst = sd["state"][i], ref.state[rp]
        assert float(st["step"]) == float(rst["step"]) == steps
        m, v = st["exp_avg"].cpu().double(), st["exp_avg_sq"].cpu().double()
        rm, rv = rst["exp_avg"], rst["exp_avg_sq"]
        assert ((m - rm).abs() <= (1e-6 + 2 * e) * (rm.abs() + float(rm.abs().max()))).all(), ("exp_avg", i)
        assert ((v - rv).abs() <= (2e-5 + 4 * e) * rv).all(), ("exp_avg_sq", i)
        tol = steps * (3.2 * lr * (1e-5 + 4 * e) + 4 * U24 * rp.detach().abs())
        assert ((p.detach().cpu().double() - rp.detach()).abs() <= tol).all(), ("param", i)


# ---- 8: pad lanes --------------------------------------------------------------------------------------------------------------------
def pad_lane_mask(arena):
    mask = torch.ones(arena.numel, dtype=torch.bool)
    for p, o in zip(arena.params, arena.offsets):
        mask[o:o + p.numel()] = False
    return mask


def assert_pad_lanes_zero(arena):
    """Each slot of the arena is rounded up to 4 floats; the norm runs over the whole flat_grad, so the pad lanes must hold exact zeros."""
    pads = arena.flat_grad.detach().cpu()[pad_lane_mask(arena)]
    assert (pads.view(torch.int32) == 0).all(), ("pad lanes of flat_grad are not zero", pads)
    return pads.numel()


# ---- 4: the recipe key through the drivers and Lightning's hook order ----------------------------------------------------------------
ACTIVE = {False: 0.25, True: 0.05}      # [recipe2024]: the steps' norms are 0.88 - 0.93 (2023 task) / 0.17 - 0.19 (2024 task) at the seeds
INACTIVE = 5.0                          # below: a factor >= 3.5 on either side (5.0 is the 2024 recipe's own value)


def _surface_run(dev, mode, clip, recipe2024=False, epochs=2, per_epoch=3, n_samp=16000 + 1024, warmup=1, max_steps=None):
    """One run of parity_cases.case_lightning_surface's workload with hparams["training"]["gradient_clip"] = clip.
    mode: "driver" (the step driver by hand), "whole" / "hooks" (tests/lightning_order.Trainer with whole_step on / off; the trainer's
    on_before_optimizer_step slot calls model.configure_gradient_clipping(opt, 0, clip, "norm"), Lightning's order), "torch" (hooks
    order, the fused clip never armed: the hook calls torch.nn.utils.clip_grad_norm_ on the parameters itself).
    -> dict(losses, state, logged, clips = [last_clip per step], numel, live = mask of the arena floats that are no pad lanes, lr)."""
    import gc
    import random
    # A run leaves reference cycles (task <-> trainer, the hook's closure) that may own a captured graph; torch's CUDAGraph destructor
    # must not run while a later run's capture is open, so they are collected here, where no capture is
    gc.collect()
    import numpy as np
    from desed_task_amd import graph as G
    from desed_task_amd import ops as _ops
    from desed_task_amd.launcher import StepDriver
    from desed_task_amd.lookahead import BatchList
    from tests import parity_cases as P
    from tests.lightning_order import Trainer
    O = P.O
    bs = (2, 1, 1, 2, 2) if recipe2024 else (1, 1, 2)
    B = sum(bs)
    n_out = (1 + n_samp // 256) // 4
    audios = [P.to(dev, O.synth_audio(B, n_samp, seed=700 + 7 * i)) for i in range(per_epoch)]
    if recipe2024:
        ns = bs[0] + bs[1] + bs[2]
        labelss = []
        for i in range(per_epoch):
            lab = (O.lcg_fill((B, 27, n_out), 50 + i, 0.5, 0.5) < 0.1).float()
            lab[ns:ns + bs[3], :, 1:] = 0.0
            lab[ns + bs[3]:] = 0.0
            labelss.append(P.to(dev, lab))
        valid = torch.zeros(B, 27, dtype=torch.bool)
        valid[:bs[0], 10:] = True
        valid[bs[0]:, :10] = True
        valid = P.to(dev, valid)
        embs = [P.to(dev, torch.randn(B, 768, 31, generator=torch.Generator().manual_seed(5 + i))) for i in range(per_epoch)]
    else:
        labelss = [P.to(dev, O.synth_labels(bs, 10, n_out, seed=80 + i)) for i in range(per_epoch)]

    class Clips(BatchList):
        def __getitem__(self, i):
            if recipe2024:
                return (audios[i], labelss[i].clone(), [1.0] * B, embs[i].clone(), valid)
            return (audios[i], labelss[i].clone(), [1.0] * B)

    kw = dict(torch_adam=mode != "driver", whole_step=mode == "whole", train_data=Clips([None] * per_epoch))
    if recipe2024:
        task = P.build_task_2024(dev, bs, 27, **kw)
    else:
        task = P.build_task(dev, bs, O.make_state_dict(seed=7), dropout=0.5, specaug=True, rampup=5, **kw)
    task.hparams["training"]["gradient_clip"] = clip
    task.whole_step_warmup = warmup
    assert task._whole_step_blockers() is None
    random.seed(41); np.random.seed(101); torch.manual_seed(101)
    if dev != "cpu":
        torch.cuda.manual_seed(101)
    _ops.reseed_dropout()
    losses, clips = [], []

    def note_clip():
        lc = task.opt.last_clip
        clips.append(None if lc is None else lc.detach().cpu().clone())

    if mode == "driver":
        driver = (G.GraphedStepDriver(task, world_size=1, warmup=warmup, prefetch="teacher") if dev != "cpu"
                  else StepDriver(task, world_size=1, prefetch="teacher"))
        data = Clips([None] * per_epoch)
        for epoch in range(epochs):
            batches = list(torch.utils.data.DataLoader(data, batch_size=None))
            for i in range(per_epoch):
                if max_steps is not None and len(losses) >= max_steps:
                    break
                nxt = batches[i + 1] if i + 1 < per_epoch else None
                losses.append(float(driver.run_step(batches[i], i, next_batch=nxt).detach()))
                note_clip()
    else:
        if mode == "torch":
            def hook(opt, idx):
                torch.nn.utils.clip_grad_norm_(list(task.sed_student.parameters()), clip)
        else:
            def hook(opt, idx):
                task.configure_gradient_clipping(opt, idx, clip, "norm")
        if clip:
            task.on_before_optimizer_step = hook
        tr = Trainer(max_epochs=epochs if max_steps is None else 1, limit_train_batches=1.0 if max_steps is None else max_steps,
                     on_step=lambda tr_, model, i: note_clip())
        tr.fit(task)
        losses = [float(l) for l in tr.losses]
        if mode == "whole":
            drv = task._driver
            assert drv is not None and not task._served and task.opt.served is False
            if dev != "cpu":
                assert drv.graph is not None
        else:
            assert task._driver is None
    sync(dev)
    arena = task.sed_student.arena
    state = [arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone()]
    for model in (task.sed_student, task.sed_teacher):
        for i in range(7):
            bn = getattr(model.cnn.cnn, "batchnorm%d" % i)
            state += [bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone()]
    osd = task.opt.state_dict()
    state += [torch.cat([osd["state"][i]["exp_avg"].reshape(-1).cpu() for i in sorted(osd["state"])]),
              torch.cat([osd["state"][i]["exp_avg_sq"].reshape(-1).cpu() for i in sorted(osd["state"])]),
              torch.tensor([float(osd["state"][0]["step"]), float(task.scheduler["scheduler"].step_num)])]
    logged = {k: float(v) for k, v in task.logged.items()}
    assert len(logged) == (9 if recipe2024 else 11), sorted(logged)         # no new logged key
    pads = assert_pad_lanes_zero(arena)
    assert pads == (2 if recipe2024 else 4), pads
    out = dict(losses=losses, state=state, logged=logged, clips=clips, numel=arena.numel, live=~pad_lane_mask(arena),
               lr=max(float(g["lr"]) for g in task.opt.param_groups))
    task.__dict__.pop("on_before_optimizer_step", None)
    task.trainer = None
    del task, arena
    gc.collect()
    return out


def _same(a, b, what):
    assert a["losses"] == b["losses"], (what, a["losses"], b["losses"])
    for i, (x, y) in enumerate(zip(a["state"], b["state"])):
        assert torch.equal(x, y), "%s: state tensor %d differs (max %.3e)" % (what, i, float((x.double() - y.double()).abs().max()))
    assert a["logged"] == b["logged"], (what, a["logged"], b["logged"])


def case_lightning_surface_clip(dev, recipe2024=False, epochs=2, per_epoch=3, n_samp=16000 + 1024):
    """parity_cases.case_lightning_surface's three modes with `gradient_clip` configured: the driver by hand, the whole step behind
    Lightning's hook order, and the hooks one by one (configure_gradient_clipping arming the adopted FusedAdam) agree BIT FOR BIT --
    losses, both arenas, BatchNorm buffers, exp_avg, exp_avg_sq, step counts, the logged keys (still 11 / 9) and every step's
    last_clip -- at the ACTIVE threshold (coef < 1 after every step) and at the INACTIVE one (coef == 1 after every step); the inactive
    run equals, bit for bit, the same run with gradient_clip = 0.  No whole-step blocker; on the GPU the whole
    mode ends with a captured graph.  The pad lanes of flat_grad are zero after every run.
    Semantic anchor ("torch"): hooks order, the fused clip never armed, the hook calling torch.nn.utils.clip_grad_norm_ itself (it
    scales the arena's gradient views in place), compared with the fused hooks run after ONE step from identical state (later steps feed
    rounding differences through the training dynamics).  Both sides run adam_kernel's arithmetic on gradients that differ by
    e_g = ((d + 1) / 2 + 5) u relative (the kernel's coefficient e_coef + torch's in-place product and its own quotient), so with
    case_adam's t = 1 bounds on each side:  |dm| <= (6 u + e_g) Mm,  |dv| <= (8 u + 2 e_g) v,
    |dp| <= 2 u |p| + step (22 u + 2 e_g) Mm / denom, each asserted with case_adam's factor 2 and evaluated at the anchor's values."""
    kw = dict(recipe2024=recipe2024, epochs=epochs, per_epoch=per_epoch, n_samp=n_samp)
    active, inactive = ACTIVE[recipe2024], INACTIVE
    for clip in (active, inactive):
        runs = {mode: _surface_run(dev, mode, clip, **kw) for mode in ("driver", "whole", "hooks")}
        for mode in ("driver", "whole", "hooks"):
            cl = runs[mode]["clips"]
            assert len(cl) == epochs * per_epoch and all(c is not None for c in cl), (mode, cl)
            print("clip %g %s mode: norms %s coefs %s" % (clip, mode, [round(float(c[0]), 6) for c in cl], [round(float(c[1]), 6) for c in cl]))
            if clip == active:
                assert all(float(c[1]) < 1.0 for c in cl), (mode, cl)
                assert all(active * 3.5 <= float(c[0]) for c in cl), ("the norms drifted towards the active threshold", cl)
            else:
                assert all(float(c[1]) == 1.0 for c in cl), (mode, cl)
                assert all(float(c[0]) * 3.5 <= inactive for c in cl), ("the norms drifted towards the inactive threshold", cl)
        for mode in ("whole", "hooks"):
            _same(runs[mode], runs["driver"], "gradient_clip %g, %s vs driver" % (clip, mode))
            for a, b in zip(runs[mode]["clips"], runs["driver"]["clips"]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (mode, a, b)
        if clip == inactive:
            off = _surface_run(dev, "driver", 0.0, **kw)         # (the three modes are bit-equal to each other: one of them suffices)
            assert all(c is None for c in off["clips"]), "gradient_clip 0 must not touch the clipping path"
            _same(off, runs["driver"], "gradient_clip 0 vs the inactive threshold")
    # the semantic anchor, one step
    fused = _surface_run(dev, "hooks", active, max_steps=1, **kw)
    anchor = _surface_run(dev, "torch", active, max_steps=1, **kw)
    assert anchor["clips"] == [None] and float(fused["clips"][0][1]) < 1.0
    assert fused["losses"] == anchor["losses"]
    n = fused["numel"]
    e_g = ((depth(n) + 1) / 2 + 5) * U24
    p_f, m_f, v_f = [fused["state"][i].double() for i in (0, -3, -2)]
    p_a, m_a, v_a = [anchor["state"][i].double() for i in (0, -3, -2)]
    b1, b2 = 0.9, 0.999
    live = anchor["live"]              # pad lanes sit in the arena but not in the per-parameter state
    p_f, p_a = p_f[live], p_a[live]
    assert p_f.numel() == m_f.numel() == m_a.numel()
    Mm, denom = m_a.abs(), (v_a.sqrt() / math.sqrt(1 - f32(b2)) + 1e-8)
    assert ((m_f - m_a).abs() <= 2 * (6 * U24 + e_g) * Mm + 1e-300).all(), ("anchor exp_avg", float(((m_f - m_a).abs() / ((6 * U24 + e_g) * Mm + 1e-300)).max()))
    assert ((v_f - v_a).abs() <= 2 * (8 * U24 + 2 * e_g) * v_a + 1e-300).all(), ("anchor exp_avg_sq", float(((v_f - v_a).abs() / ((8 * U24 + 2 * e_g) * v_a + 1e-300)).max()))
    step_size = anchor["lr"] / (1 - b1)              # (an upper bound: read after the scheduler's step, and the warm-up lr only grows)
    assert ((p_f - p_a).abs() <= 2 * (2 * U24 * p_a.abs() + step_size * (22 * U24 + 2 * e_g) * Mm / denom) + 1e-300).all(), "anchor parameters"
    # ... and the bounds discriminate: the unclipped moments are a factor 1 / coef away
    coef = float(fused["clips"][0][1])
    unclipped = _surface_run(dev, "hooks", 0.0, max_steps=1, **kw)
    m_u = unclipped["state"][-3].double()
    assert ((m_u - m_a).abs() > 2 * (6 * U24 + e_g) * Mm).double().mean() > 0.5, "the anchor bound would not notice a forgotten coefficient"
    assert abs(float(m_a.abs().sum() / m_u.abs().sum()) / coef - 1) < 1e-4


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def case_step_bit_reproducible_clip(dev, steps=3, n_samp=16000 + 1024, clip=0.25):
    """parity_cases.case_step_bit_reproducible with clipping active: the same seeded steps give the SAME BITS run twice eagerly and
    (GPU) once more through the hipGraph driver -- eager warm-up, capture, replays -- loss, student, teacher, gradient, exp_avg,
    exp_avg_sq and last_clip."""
    import random
    import numpy as np
    from desed_task_amd import graph as G
    from desed_task_amd import ops
    from desed_task_amd.launcher import StepDriver
    from tests import parity_cases as P
    O = P.O
    bs = (1, 1, 2)
    B = sum(bs)
    sd = O.make_state_dict(seed=7)
    audio = P.to(dev, O.synth_audio(B, n_samp, seed=77))
    labels = P.to(dev, O.synth_labels(bs, 10, (1 + n_samp // 256) // 4, seed=5))
    finals = []
    for mode in ("eager", "eager") + (("graph",) if dev != "cpu" else ()):
        task = P.build_task(dev, bs, sd, dropout=0.5, specaug=True, rampup=5)
        task.hparams["training"]["gradient_clip"] = clip
        driver = StepDriver(task, world_size=1) if mode == "eager" else G.GraphedStepDriver(task, world_size=1, warmup=1)
        assert task.opt.max_grad_norm == clip
        for step in range(steps):
            random.seed(40 + step); np.random.seed(100 + step); torch.manual_seed(100 + step)
            ops.reseed_dropout()
            loss = driver.run_step((audio, labels.clone(), None, None), step)
        sync(dev)
        if mode == "graph":
            assert driver.graph is not None
        st = task.opt._flat_state
        assert float(task.opt.last_clip[1]) < 1.0
        finals.append((float(loss.detach()), task.sed_student.arena.flat.detach().cpu().clone(), task.sed_teacher.arena.flat.detach().cpu().clone(),
                       task.sed_student.arena.flat_grad.detach().cpu().clone(), st["m"].cpu().clone(), st["v"].cpu().clone(),
                       task.opt.last_clip.cpu().clone()))
    for name, other in zip(("second eager run", "hipGraph replay"), finals[1:]):
        assert finals[0][0] == other[0], (name, finals[0][0], other[0])
        for what, a, b_ in zip(("student", "teacher", "gradient", "exp_avg", "exp_avg_sq", "last_clip"), finals[0][1:], other[1:]):
            assert torch.equal(a, b_), "%s: %s differs (max %.3e)" % (name, what, (a - b_).abs().max().item())


def case_pad_lanes(dev, n_samp=16000 + 1024):
    """After clipped steps of either task (driver by hand, two steps) every pad lane of the student's flat_grad is exactly 0 -- the
    norm streams over the whole arena and relies on it (asserted inside _surface_run: 4 pad lanes in the 2023 task, 2 in the 2024 one)."""
    for recipe2024 in (False, True):
        out = _surface_run(dev, "driver", ACTIVE[recipe2024], recipe2024=recipe2024, epochs=1, per_epoch=2, n_samp=n_samp)
        assert int((~out["live"]).sum()) == (2 if recipe2024 else 4) and len(out["clips"]) == 2
