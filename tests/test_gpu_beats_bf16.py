"""GPU runs (`pytest -m gpu`) of the extractor's single-product "bf16" mode cases (tests/beats_bf16_cases.py) through the real library."""
import pytest
import torch

from tests import beats_bf16_cases as M
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


def test_split_tiles_image():
    M.case_split_tiles("cuda")


def test_layernorm_tiles_image_and_y():
    M.case_layernorm_tiles("cuda")


@pytest.mark.parametrize("row", M.LINEAR_SHAPES)
def test_linear_entries_vs_float64_on_rounded_operands(row):
    M.case_linear_entries("cuda", row)


def test_linear_refusals():
    M.case_linear_refusals("cuda")


@pytest.mark.parametrize("row", M.LINEAR_SHAPES)
def test_linear_output_image(row):
    M.case_linear_out_image("cuda", row)


@pytest.mark.parametrize("row", M.LINEAR_SHAPES)
def test_linear_entries_equal_three_product_twins_on_bf16_operands(row):
    M.case_linear_bit_equal("cuda", row)


def test_posconv_vs_float64_on_rounded_operands():
    M.case_posconv("cuda")


def test_posconv_equals_three_product_twin_on_bf16_operands():
    M.case_posconv_bit_equal("cuda")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", M.ATTN_SHAPES)
def test_attention_vs_float64_on_rounded_operands(shape, bias):
    M.case_attention("cuda", *shape, bias)


@pytest.mark.parametrize("which", [2, 12])
def test_extractor_vs_reference_fixture_and_back_to_default(which):
    M.case_extractor("cuda", which)


def test_linear_tiles_reproducible_at_production_depth():
    M.case_linear_tiles_reproducible("cuda")
