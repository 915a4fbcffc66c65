"""CPU (fiber-emulator) runs of the single-product "bf16" mode cases (tests/bf16_mode_cases.py), plus the checks that need no kernel."""
import pytest

from tests import bf16_mode_cases as M
from tests.emu_support import emu, emu_sequential  # noqa: F401


def test_mode_exists(emu):
    M.case_mode_exists(emu.path)


def test_precision_key_values():
    M.case_precision_key()


def test_gemm_discrimination():
    M.case_gemm_discrimination()


def test_conv_discrimination():
    M.case_conv_discrimination()


def test_gemm_entries_vs_float64_on_rounded_operands(emu):
    M.case_gemm_entries("cpu")


def test_gemm_entries_equal_three_product_twins_on_bf16_operands(emu):
    M.case_gemm_bit_equal("cpu")


@pytest.mark.parametrize("shape", M.CONV_SHAPES)
def test_conv_entries_vs_float64_on_rounded_operands(emu, shape):
    M.case_conv_entries("cpu", shape)


def test_conv_walks_several_tiles(emu):
    M.case_conv_walks("cpu")


@pytest.mark.parametrize("shape", M.CONV_SHAPES)
def test_conv_entries_equal_three_product_twins_on_bf16_operands(emu, shape):
    M.case_conv_bit_equal("cpu", shape)


def test_prologue_and_packs(emu):
    M.case_prologue_packs("cpu")


def test_module_step_vs_oracle_and_vs_rounded_three_product_kernels(emu_sequential):
    M.case_module_vs_oracle("cpu")


@pytest.mark.parametrize("year", [2023, 2024])
def test_step_in_bf16_mode_captured_pipelined_reproducible(emu_sequential, year):
    M.case_step_bf16("cpu", year)


@pytest.mark.parametrize("year", [2023, 2024])
def test_precision_16_warns_and_equals_32(emu_sequential, year):
    M.case_precision_16_warns_and_changes_nothing("cpu", year)


@pytest.mark.parametrize("year", [2023, 2024])
def test_default_untouched(emu_sequential, year):
    M.case_default_untouched("cpu", year)


@pytest.mark.parametrize("year", [2023, 2024])
def test_validation_step_runs_in_the_mode(emu, year):
    M.case_validation_bf16("cpu", year)
