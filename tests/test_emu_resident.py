"""CPU (fiber-emulator) runs of the resident-data cases (tests/resident_cases.py): the gather kernel at every kind, row length and row
count, pool building, the index guard, batch-for-batch equality with a DataLoader, the ring, and the 2023 / pretrained steps and the
validation step over a resident set against the plain loader, all bit for bit."""
import pytest

from tests import resident_cases as M
from tests.emu_support import emu  # noqa: F401


@pytest.mark.parametrize("length", M.ROW_LENGTHS)
def test_gather_kernel_every_kind(emu, length):
    M.case_kernel_one_stream("cpu", length)


def test_gather_kernel_four_streams_in_one_launch(emu):
    M.case_kernel_four_streams("cpu")


def test_pool_building(emu):
    M.case_pool_building("cpu")


def test_index_guard_launches_nothing(emu):
    M.case_index_guard("cpu")


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "embeddings_and_mask"])
def test_same_batches_as_a_dataloader(emu, extras):
    M.case_same_batches_as_dataloader("cpu", extras)


def test_ring_keeps_held_batches(emu):
    M.case_ring("cpu")


@pytest.mark.parametrize("pretrained", [False, True], ids=["2023", "pretrained"])
def test_step_over_resident_set_equals_plain_loader(emu, pretrained):
    M.case_through_the_step("cpu", pretrained=pretrained)


def test_eval_set_and_validation_step(emu):
    M.case_eval_set("cpu")
