"""CPU (fiber-emulator) runs of the direct BatchNorm / GLU / first-block cases (tests/block_cases.py), plus the checks that need no
kernel: the bound constants from the fp32 restatement, the discrimination condition, and "the rows reach every kernel"."""
import pytest

from tests import block_cases as K
from tests import bf16_mode_cases as M
from tests.emu_support import emu  # noqa: F401


@pytest.fixture(scope="module", autouse=True)
def ratios_printed_at_the_end():
    """Not a test: after the module's tests, prints the largest |err| / bound per family that check() recorded (-s shows it)."""
    yield
    K.report_ratios("cpu")


def test_rows_reach_every_kernel():
    K.case_rows_reach_every_kernel()


def test_constants_follow_from_the_fp32_restatement():
    K.case_constants()


def test_discrimination():
    K.case_discrimination()


def test_glu_every_kernel(emu):
    K.case_glu("cpu")


def test_glu_seed_in_device_memory(emu):
    K.case_glu_seed_dev("cpu")


def test_bn_finalize(emu):
    K.case_finalize("cpu")


def test_bn_bwd_apply(emu):
    K.case_apply("cpu")


def test_bn_bwd_apply_equals_folded_entry(emu):
    K.case_apply_equals_folded_entry("cpu")


def test_conv0_fwd(emu):
    K.case_conv0_fwd("cpu")


def test_conv0_wgrad(emu):
    K.case_conv0_wgrad("cpu")


def test_block0(emu):
    K.case_block0("cpu")


def test_block0_chain_eval_and_seed_dev(emu):
    K.case_block0_chain_and_eval("cpu")


@pytest.mark.parametrize("shape", M.CONV_SHAPES)
def test_conv_f32_twins(emu, shape):
    K.case_conv_f32("cpu", shape)


def test_error_contract(emu):
    K.case_error_contract("cpu")
