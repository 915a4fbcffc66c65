"""GPU runs (`pytest -m gpu`) of the single-product "bf16" mode cases (tests/bf16_mode_cases.py) through the real library."""
import pytest
import torch

from tests import bf16_mode_cases as M
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


def test_mode_exists(hip):
    M.case_mode_exists(hip.path)


def test_gemm_entries_vs_float64_on_rounded_operands():
    M.case_gemm_entries("cuda")


def test_gemm_entries_equal_three_product_twins_on_bf16_operands():
    M.case_gemm_bit_equal("cuda")


@pytest.mark.parametrize("shape", M.CONV_SHAPES)
def test_conv_entries_vs_float64_on_rounded_operands(shape):
    M.case_conv_entries("cuda", shape)


def test_conv_walks_several_tiles():
    M.case_conv_walks("cuda")


@pytest.mark.parametrize("shape", M.CONV_SHAPES)
def test_conv_entries_equal_three_product_twins_on_bf16_operands(shape):
    M.case_conv_bit_equal("cuda", shape)


def test_prologue_and_packs():
    M.case_prologue_packs("cuda")


def test_module_step_vs_oracle_and_vs_rounded_three_product_kernels():
    M.case_module_vs_oracle("cuda")


@pytest.mark.parametrize("year", [2023, 2024])
def test_step_in_bf16_mode_captured_pipelined_reproducible(year):
    M.case_step_bf16("cuda", year)


@pytest.mark.parametrize("year", [2023, 2024])
def test_precision_16_warns_and_equals_32(year):
    M.case_precision_16_warns_and_changes_nothing("cuda", year)


@pytest.mark.parametrize("year", [2023, 2024])
def test_default_untouched(year):
    M.case_default_untouched("cuda", year)


@pytest.mark.parametrize("year", [2023, 2024])
def test_validation_step_runs_in_the_mode(year):
    M.case_validation_bf16("cuda", year)
