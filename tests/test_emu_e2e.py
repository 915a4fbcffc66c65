"""CPU (fiber-emulator) runs of the `pretrained.e2e` cases (tests/e2e_cases.py): the token-major fusion kernel, the dispatch, and the
2023 `pretrained` step with the frozen BEATs extractor inside it (eager and pipelined; the captured step is GPU-only), at the
same shapes and step counts as the GPU runner (768 extractor rows: the tile-image Linears run).  The trainer cases take about
nine minutes together on eight emulator threads; the kernel cases a few seconds."""
import pytest

from tests import e2e_cases as M
from tests.emu_support import emu, emu_sequential  # noqa: F401


@pytest.mark.parametrize("shape", M.KERNEL_SHAPES)
def test_tokens_kernel_equals_twin_bit_for_bit(emu, shape):
    M.case_kernel_equals_twin("cpu", shape)


@pytest.mark.parametrize("shape", M.KERNEL_SHAPES)
def test_tokens_kernel_vs_float64_pooling(emu, shape):
    M.case_kernel_vs_float64("cpu", shape)


def test_tokens_kernel_refusals(emu):
    M.case_kernel_refusals("cpu")


def test_embcat_dispatch_on_layout(emu):
    M.case_dispatch("cpu")


def test_e2e_step_equals_precomputed_step(emu):
    M.case_e2e_equals_precomputed("cpu")


def test_e2e_step_vs_oracle(emu):
    M.case_e2e_vs_oracle("cpu")


def test_e2e_step_vs_reference_golden(emu):
    M.case_e2e_vs_reference_golden("cpu")


def test_e2e_validation_and_test_steps(emu):
    M.case_validation_and_test("cpu")


def test_e2e_pipelined_equals_unpipelined(emu):
    M.case_pipelined("cpu")


def test_e2e_refusals_and_surface(emu):
    M.case_refusals_and_surface("cpu")
