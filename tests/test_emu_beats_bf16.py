"""CPU (fiber-emulator) runs of the extractor's single-product "bf16" mode cases (tests/beats_bf16_cases.py), plus the checks that need no
kernel.  GPU-only: the reproducibility screen at production depth (case 10: it is about the hardware's stage ordering) and the 12-layer,
496-token extractor case (three extractor passes of 50 s each on the emulator; the 2-layer case runs the same code paths here)."""
import pytest

from tests import beats_bf16_cases as M
from tests.emu_support import emu, emu_sequential  # noqa: F401


def test_mode_exists(emu):
    M.case_mode_exists(emu.path)


def test_split_tiles_image(emu):
    M.case_split_tiles("cpu")


def test_layernorm_tiles_image_and_y(emu):
    M.case_layernorm_tiles("cpu")


@pytest.mark.parametrize("row", M.LINEAR_SHAPES)
def test_linear_entries_vs_float64_on_rounded_operands(emu, row):
    M.case_linear_entries("cpu", row)


def test_linear_refusals(emu):
    M.case_linear_refusals("cpu")


@pytest.mark.parametrize("row", M.LINEAR_SHAPES)
def test_linear_output_image(emu, row):
    M.case_linear_out_image("cpu", row)


@pytest.mark.parametrize("row", M.LINEAR_SHAPES)
def test_linear_entries_equal_three_product_twins_on_bf16_operands(emu, row):
    M.case_linear_bit_equal("cpu", row)


def test_linear_discrimination():
    M.case_linear_discrimination()


def test_plain_fp32_product_is_inside_the_bounds():
    M.case_linear_plain_fp32_chain_is_inside()


def test_posconv_vs_float64_on_rounded_operands(emu):
    M.case_posconv("cpu")


def test_posconv_equals_three_product_twin_on_bf16_operands(emu):
    M.case_posconv_bit_equal("cpu")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", M.ATTN_SHAPES)
def test_attention_vs_float64_on_rounded_operands(emu, shape, bias):
    M.case_attention("cpu", *shape, bias)


@pytest.mark.parametrize("which", [2])
def test_extractor_vs_reference_fixture_and_back_to_default(emu, which):
    M.case_extractor("cpu", which)
