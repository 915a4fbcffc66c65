"""GPU runs (`pytest -m gpu`) of the resident-data cases (tests/resident_cases.py) through the real library, the captured whole step
included."""
import pytest
import torch

from tests import resident_cases as M
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("length", M.ROW_LENGTHS)
def test_gather_kernel_every_kind(length):
    M.case_kernel_one_stream("cuda", length)


def test_gather_kernel_four_streams_in_one_launch():
    M.case_kernel_four_streams("cuda")


def test_pool_building():
    M.case_pool_building("cuda")


def test_index_guard_launches_nothing():
    M.case_index_guard("cuda")


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "embeddings_and_mask"])
def test_same_batches_as_a_dataloader(extras):
    M.case_same_batches_as_dataloader("cuda", extras)


def test_ring_keeps_held_batches():
    M.case_ring("cuda")


@pytest.mark.parametrize("pretrained", [False, True], ids=["2023", "pretrained"])
def test_step_over_resident_set_equals_plain_loader(pretrained):
    M.case_through_the_step("cuda", pretrained=pretrained)


def test_eval_set_and_validation_step():
    M.case_eval_set("cuda")
