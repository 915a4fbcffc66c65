"""CPU (fiber-emulator) runs of the direct GEMM / colsum / arena-kernel cases (tests/contraction_cases.py), plus the checks that need
no kernel: BETA from the reference accumulation, the discrimination condition, and "the caller-shaped table is what ops.py issues"."""
import pytest
import torch

from tests import contraction_cases as C
from tests.emu_support import emu  # noqa: F401


def all_rows():
    return C.table_plain() + C.table_scalar() + C.table_splitk()


def test_tables_reach_every_instantiation():
    C.case_tables_reach_every_instantiation()


def test_beta_is_what_the_reference_chain_gives():
    """BETA = 4 x the largest r_ref of the plain fp32 reference accumulation over the tables (no kernel involved)."""
    worst, per = C.measure_r_ref(all_rows())
    print("r_ref per row (K, split, r):", [(k, s, round(r, 3)) for k, s, r in per])
    assert 4 * worst <= C.BETA <= 4 * worst + 0.2, "BETA %.2f, 4 x r_ref max = %.3f" % (C.BETA, 4 * worst)


def test_discrimination():
    C.case_discrimination(all_rows())


def test_plain_and_pair_entries(emu):
    C.case_table("cpu", C.table_plain())


def test_scalar_paths_and_f32_fallback_bits(emu):
    C.case_scalar_paths("cpu")


def test_deterministic_splitk(emu):
    C.case_table("cpu", C.table_splitk(), first_seed=100)


def test_caller_shaped_rows(emu):
    # B T = 19: every (H, I) of the two recipes, every variant; 300 (one slice) and 624 (two slices): one layer each
    C.case_caller_rows("cpu", bts=((1, 19),), his=((128, 128), (128, 256), (192, 128), (192, 384)), embcat=((1, 19, 256, 768),))
    C.case_caller_rows("cpu", bts=((2, 150),), his=((128, 128),), variants=("default", "f32"), embcat=((2, 150, 256, 256),))
    C.case_caller_rows("cpu", bts=((4, 156),), his=((128, 128),), embcat=((4, 156, 64, 128),))
    assert C.bigru_rows(4, 156, 128, 128)[2]["split"] == 2 and C.bigru_rows(2, 150, 128, 128)[2]["split"] == 1


def test_largest_kernel_ratios_are_reported(emu):
    """Prints the largest tier-B ratio per kernel family seen by the tests above (the emulator figure in contraction_cases' docstring)."""
    print("largest tier-B ratios:", {k: round(v, 3) for k, v in C.STATS.items()}, "BETA", C.BETA)
    assert all(v <= C.BETA for v in C.STATS.values())


@pytest.mark.parametrize("prec,dw_atomic", [("bf16x3", False), ("bf16x3", True), ("f32", False)])
def test_caller_rows_are_what_ops_issues(emu, prec, dw_atomic):
    """A real BiGRULayerFn forward + backward at B = 4, T = 156 with lib.call recorded issues exactly the argument tuples of
    contraction_cases.bigru_rows -- the table cannot drift from the caller."""
    from desed_task_amd import ops
    from desed_task_amd import _lib
    B, T, I, H = 4, 156, 128, 128
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, I, generator=g).requires_grad_(True)
    ws = []
    for d in range(2):
        ws += [torch.randn(3 * H, I, generator=g) / 11, torch.randn(3 * H, H, generator=g) / 11, torch.randn(3 * H, generator=g) / 11,
               torch.randn(3 * H, generator=g) / 11]
    ws = [w.requires_grad_(True) for w in ws]
    lib = _lib.get()
    calls, orig = [], lib.call

    def spy(name, *a):
        calls.append((name, a))
        return orig(name, *a)
    lib.call = spy
    try:
        out = ops.BiGRULayerFn.apply(x, *ws, dict(gemm_precision=prec, gru_dw_atomic=dw_atomic))
        out.backward(torch.randn(B, T, 2 * H, generator=g))
    finally:
        lib.call = orig
    fwd = [a for n, a in calls if n == "sed_gru_fwd"][0]
    bwd = [a for n, a in calls if n == "sed_gru_bwd"][0]
    base = {"x": x.data_ptr(), "w_ih0": ws[0].data_ptr(), "w_ih1": ws[4].data_ptr(), "b_ih0": ws[2].data_ptr(), "b_ih1": ws[6].data_ptr(),
            "dgi": bwd[5], "dgh": bwd[6], "hprev": bwd[7]}
    del base["dgi"], base["dgh"], base["hprev"]
    fwd_base = dict(base, gi=fwd[0])          # gi lives only during the forward: its memory is handed out again in the backward
    base = dict(base, dgi=bwd[5], dgh=bwd[6], hprev=bwd[7])
    extent = {"x": x.numel(), "w_ih0": ws[0].numel(), "w_ih1": ws[4].numel(), "b_ih0": 3 * H, "b_ih1": 3 * H, "gi": B * T * 6 * H,
              "dgi": B * T * 6 * H, "dgh": B * T * 6 * H, "hprev": B * T * 2 * H}

    def symbol(p, base):
        if not isinstance(p, int) or p < 4096:
            return p
        for k, b in base.items():
            if b <= p < b + 4 * extent[k]:
                return (k, p - b)
        return "out"
    names = [n for n, _ in calls]
    gemm_calls = [(n, tuple(symbol(v, fwd_base if i < names.index("sed_gru_fwd") else base) for v in a))
                  for i, (n, a) in enumerate(calls) if n.startswith("sed_gemm")]
    rows = C.bigru_rows(B, T, I, H, prec=prec, dw_atomic=dw_atomic)
    assert [n for n, _ in gemm_calls] == [r["entry"] for r in rows], [n for n, _ in gemm_calls]
    for (name, got), row in zip(gemm_calls, rows):
        sym = {k: (v if v[0] in fwd_base or v[0] in base else "out") for k, v in row["sym"].items()}
        want = C.call_args(row, sym, 0, scratch="out")
        assert got == want, (row["tag"], got, want)
    # the atomic form zero-fills its four outputs first
    assert ("sed_zero_buffers" in [n for n, _ in calls]) == (dw_atomic or prec == "f32")


def test_colsum(emu):
    C.case_colsum("cpu")


def test_adam_kernel(emu):
    C.case_adam("cpu")


def test_ema_kernel(emu):
    C.case_ema("cpu")


def test_zero_buffers_and_count_contract(emu):
    C.case_zero_buffers("cpu")


def test_ema_alignment_contract(emu):
    C.case_ema_alignment_contract("cpu")


def test_fused_adam_vs_float64_torch_adam(emu):
    C.case_fused_adam_host("cpu")


def test_ema_update_routes(emu):
    C.case_ema_host("cpu")


def test_error_contract(emu):
    C.case_error_contract("cpu")
