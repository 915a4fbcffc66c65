"""GPU runs (`pytest -m gpu`) of the `pretrained.e2e` cases (tests/e2e_cases.py) through the real library, the captured whole step
included."""
import pytest
import torch

from tests import e2e_cases as M
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("shape", M.KERNEL_SHAPES)
def test_tokens_kernel_equals_twin_bit_for_bit(shape):
    M.case_kernel_equals_twin("cuda", shape)


@pytest.mark.parametrize("shape", M.KERNEL_SHAPES)
def test_tokens_kernel_vs_float64_pooling(shape):
    M.case_kernel_vs_float64("cuda", shape)


def test_tokens_kernel_refusals():
    M.case_kernel_refusals("cuda")


def test_embcat_dispatch_on_layout():
    M.case_dispatch("cuda")


def test_e2e_step_equals_precomputed_step():
    M.case_e2e_equals_precomputed("cuda")


def test_e2e_step_vs_oracle():
    print(M.case_e2e_vs_oracle("cuda"))


def test_e2e_step_vs_reference_golden():
    print(M.case_e2e_vs_reference_golden("cuda"))


def test_e2e_validation_and_test_steps():
    M.case_validation_and_test("cuda")


def test_e2e_pipelined_equals_unpipelined():
    M.case_pipelined("cuda")


def test_e2e_pipelined_and_captured():
    M.case_pipelined("cuda", graph=True, steps=7, epoch_end=4)


def test_e2e_refusals_and_surface():
    M.case_refusals_and_surface("cuda")
