"""GPU runs (`pytest -m gpu`) of the direct BatchNorm / GLU / first-block cases (tests/block_cases.py) through the real library."""
import pytest
import torch

from tests import block_cases as K
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


@pytest.fixture(scope="module", autouse=True)
def ratios_printed_at_the_end():
    """Not a test: after the module's tests, prints the largest |err| / bound per family that check() recorded (-s shows it)."""
    yield
    K.report_ratios("cuda")


def test_rows_reach_every_kernel():
    K.case_rows_reach_every_kernel()


def test_glu_every_kernel():
    K.case_glu("cuda")


def test_glu16_grid_stride_loops():
    """8 200 pooled rows: the forward's 2 048 and the backward's 1 024 workgroups take a second (and third), unequal loop iteration."""
    K.case_glu("cuda", gpu_only=True)


def test_glu_seed_in_device_memory():
    K.case_glu_seed_dev("cuda")


def test_bn_finalize():
    K.case_finalize("cuda")


def test_bn_bwd_apply():
    """Includes, per C, npix just above 4 096 workgroups' worth: the grid-stride loop runs twice for some workgroups only."""
    K.case_apply("cuda", gpu=True)


def test_bn_bwd_apply_equals_folded_entry():
    K.case_apply_equals_folded_entry("cuda")


def test_conv0_fwd():
    K.case_conv0_fwd("cuda")


def test_conv0_wgrad():
    K.case_conv0_wgrad("cuda")


def test_block0():
    K.case_block0("cuda")


def test_block0_full_length_with_and_without_centring():
    """B = 2, T = 626, F = 128 on the offset input: asserted with centring on; block0_nocenter = 1 only prints its ratio."""
    K.case_block0("cuda", gpu_only=True)


def test_block0_chain_eval_and_seed_dev():
    K.case_block0_chain_and_eval("cuda")


@pytest.mark.parametrize("shape", M.CONV_SHAPES)
def test_conv_f32_twins(shape):
    K.case_conv_f32("cuda", shape)


def test_error_contract():
    K.case_error_contract("cuda")
