"""Per-kernel timing of the single-product "bf16" entries beside their three-product twins ("Mixed-precision mode";
profiles/bf16_mode.md): the six production convolutions of blocks 1-6 at B = 48, T = 156 -- forward, data gradient (BN-folded) and weight
gradient -- and the BiGRU GEMM launches.  Both modes run in ONE process, interleaved (x1, x3, x1, x3, ...), HIP-event time per launch,
median over the repetitions.

    python tools/bf16_mode_microbench.py [--reps 31] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from desed_task_amd import _lib  # noqa: E402
from desed_task_amd.ops import pack_conv_weights  # noqa: E402

LAYERS = ((16, 32, 64), (32, 64, 32), (64, 128, 16), (128, 128, 8), (128, 128, 4), (128, 128, 2))      # (CIN, COUT, F) of blocks 1-6
B, T = 48, 156


def timed(fns, reps):
    """fns: {mode: callable}; -> {mode: median us}, the modes alternating launch by launch."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ev = {m: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for m in fns}
    for r in range(reps):
        for m, f in fns.items():
            ev[m][r][0].record()
            f()
            ev[m][r][1].record()
    torch.cuda.synchronize()
    return {m: statistics.median(a.elapsed_time(b) for a, b in ev[m]) * 1e3 for m in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _lib.get()
    st = torch.cuda.current_stream().cuda_stream
    dev = "cuda"
    rows = []
    sfx = {"bf16": "_bf16x1", "bf16x3": "_bf16x3"}
    for CIN, COUT, F in LAYERS:
        x = torch.randn(B, T, F, CIN, device=dev)
        w = torch.randn(COUT, CIN, 3, 3, device=dev) * 0.03
        bias = torch.zeros(COUT, device=dev)
        y = torch.empty(B, T, F, COUT, device=dev)
        dz, dy, dx = torch.randn_like(y), torch.empty_like(y), torch.empty_like(x)
        stats = torch.cat((torch.zeros(COUT, device=dev), torch.ones(COUT, device=dev)))
        gam, dg, db, dbias = (torch.ones(COUT, device=dev), torch.randn(COUT, device=dev), torch.randn(COUT, device=dev),
                              torch.empty(COUT, device=dev))
        nblk = lib.value("sed_conv_fwd_blocks_bf16", B, T, F, CIN, COUT)
        partial = torch.empty(nblk * 2 * COUT, device=dev)
        scratch = torch.empty(int(lib.value("sed_conv_wgrad_scratch_floats", B, T, F, CIN, COUT)), device=dev)
        dw = torch.empty_like(w)
        packs = {m: pack_conv_weights([w], True, m)[0] for m in sfx}
        fwd = {m: (lambda m=m: lib.call("sed_conv3x3" + sfx[m], x.data_ptr(), packs[m][0].data_ptr(), bias.data_ptr(), y.data_ptr(),
                                        partial.data_ptr(), B, T, F, CIN, COUT, st)) for m in sfx}
        dgr = {m: (lambda m=m: lib.call("sed_conv3x3%s_bnbwd" % sfx[m], dz.data_ptr(), y.data_ptr(), stats.data_ptr(), gam.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), packs[m][1].data_ptr(), dx.data_ptr(), dy.data_ptr(), dbias.data_ptr(),
                                        B, T, F, COUT, CIN, st)) for m in sfx}
        wgr = {m: (lambda m=m: lib.call("sed_conv_wgrad" + sfx[m], x.data_ptr(), dy.data_ptr(), scratch.data_ptr(), dw.data_ptr(),
                                        B, T, F, CIN, COUT, st)) for m in sfx}
        for what, fns in (("forward", fwd), ("data gradient (BN-folded)", dgr), ("weight gradient", wgr)):
            t = timed(fns, args.reps)
            rows.append(dict(kernel="conv %d->%d F=%d %s" % (CIN, COUT, F, what), bf16_us=t["bf16"], bf16x3_us=t["bf16x3"]))
            print("%-52s bf16 %7.1f us   bf16x3 %7.1f us   x%.2f" % (rows[-1]["kernel"], t["bf16"], t["bf16x3"], t["bf16x3"] / t["bf16"]), flush=True)
    # BiGRU GEMMs at B T = 7488: layer 0 (I = 128) and layer 1 (I = 256), H = 128 -- the argument tuples of ops.BiGRULayerFn
    BT, H = B * T, 128
    for I in (128, 256):
        xg = torch.randn(BT, I, device=dev)
        wih = [torch.randn(3 * H, I, device=dev) * 0.05 for _ in range(2)]
        bih = [torch.zeros(3 * H, device=dev) for _ in range(2)]
        gi = torch.empty(BT, 2, 3 * H, device=dev)
        dgi = torch.randn(BT, 2, 3 * H, device=dev)
        dxg = torch.empty(BT, I, device=dev)
        dwi = [torch.empty(3 * H, I, device=dev) for _ in range(2)]
        split = max(1, min(32, BT // 256))
        nsl = min(max(1, round(700.0 / (((I + 63) // 64) * ((BT + 127) // 128)))), max(1, (6 * H) // 128))
        scr = torch.empty(int(lib.value("sed_gemm_splitk_scratch_floats", 3 * H, max(I, H), BT, split)) +
                          int(lib.value("sed_gemm_splitk_scratch_floats", BT, I, 6 * H, nsl)), device=dev)
        off = 3 * H * 4
        proj = {m: (lambda m=m: lib.call("sed_gemm_pair" + sfx[m], xg.data_ptr(), xg.data_ptr(), wih[0].data_ptr(), wih[1].data_ptr(),
                                         bih[0].data_ptr(), bih[1].data_ptr(), gi.data_ptr(), gi.data_ptr() + off, BT, 3 * H, I, I, I, 6 * H,
                                         0, 1, 1, 0, st)) for m in sfx}
        dxp = {m: (lambda m=m: lib.call("sed_gemm_kcat_splitk" + sfx[m], dgi.data_ptr(), wih[0].data_ptr(), wih[1].data_ptr(), dxg.data_ptr(),
                                        BT, I, 6 * H, 3 * H, 6 * H, I, I, nsl, scr.data_ptr(), st)) for m in sfx}
        dwp = {m: (lambda m=m: lib.call("sed_gemm_pair_splitk" + sfx[m], dgi.data_ptr(), dgi.data_ptr() + off, xg.data_ptr(), xg.data_ptr(),
                                        dwi[0].data_ptr(), dwi[1].data_ptr(), 3 * H, I, BT, 6 * H, I, I, 1, 0, split, scr.data_ptr(), st))
               for m in sfx}
        for what, fns in (("input projection (pair)", proj), ("dX (kcat, split-K)", dxp), ("dW_ih (pair, split-K)", dwp)):
            t = timed(fns, args.reps)
            rows.append(dict(kernel="BiGRU I=%d %s" % (I, what), bf16_us=t["bf16"], bf16x3_us=t["bf16x3"]))
            print("%-52s bf16 %7.1f us   bf16x3 %7.1f us   x%.2f" % (rows[-1]["kernel"], t["bf16"], t["bf16x3"], t["bf16x3"] / t["bf16"]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
