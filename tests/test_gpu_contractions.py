"""GPU runs (`pytest -m gpu`) of the direct GEMM / colsum / arena-kernel cases (tests/contraction_cases.py) through the real library."""
import pytest
import torch

from tests import contraction_cases as C
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


def test_tables_reach_every_instantiation():
    C.case_tables_reach_every_instantiation()


def test_plain_and_pair_entries():
    C.case_table("cuda", C.table_plain())


def test_scalar_paths_and_f32_fallback_bits():
    C.case_scalar_paths("cuda")


def test_deterministic_splitk():
    C.case_table("cuda", C.table_splitk(), first_seed=100)


@pytest.mark.parametrize("B", [1, 4, 48])
def test_caller_shaped_rows(B):
    """The exact argument tuples of BiGRULayerFn / EmbCatFn at T = 156 (B = 48: 29 requested, 26 actual slices of 288)."""
    C.case_caller_rows("cuda", bts=((B, 156),), his=((128, 128), (128, 256), (192, 128), (192, 384)), embcat=((B, 156, 256, 768),))


def test_largest_kernel_ratios_are_reported():
    """Not a check of its own: prints the largest tier-B ratio per kernel family seen by the tests above (the figure DESIGN.md quotes)."""
    print("largest tier-B ratios:", {k: round(v, 3) for k, v in C.STATS.items()}, "BETA", C.BETA)
    assert all(v <= C.BETA for v in C.STATS.values())


def test_colsum():
    C.case_colsum("cuda")


def test_adam_kernel():
    C.case_adam("cuda")


def test_ema_kernel():
    C.case_ema("cuda")


def test_zero_buffers_and_count_contract():
    C.case_zero_buffers("cuda")


def test_ema_alignment_contract():
    C.case_ema_alignment_contract("cuda")


def test_fused_adam_vs_float64_torch_adam():
    C.case_fused_adam_host("cuda")


def test_ema_update_routes():
    C.case_ema_host("cuda")


def test_error_contract():
    C.case_error_contract("cuda")
