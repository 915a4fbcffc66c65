"""GPU runs (`pytest -m gpu`) of the device-PSDS cases (tests/psds_device_cases.py) through the real library, two validation batches
(48 clips) included."""
import pytest
import torch

from tests import psds_device_cases as M
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("setting", sorted(M.SETTINGS))
@pytest.mark.parametrize("name", M.GPU_CASES)
def test_kernel_steps_equal_the_host_steps(name, setting):
    M.case_kernel("cuda", name, setting)


@pytest.mark.parametrize("setting", sorted(M.SETTINGS))
@pytest.mark.parametrize("name", M.GPU_CASES)
def test_psds_from_score_buffer_equals_psds_from_scores(name, setting):
    M.case_end_to_end("cuda", name, setting)


def test_class_subset():
    M.case_class_subset("cuda")


def test_tables_and_written_files(tmp_path):
    M.case_tables("cuda", str(tmp_path))


def test_errors():
    M.case_errors("cuda")


def test_hooks_2023_flag_on_equals_flag_off(tmp_path):
    M.case_hooks_2023("cuda", str(tmp_path))


def test_hooks_2024_flag_on_equals_flag_off(tmp_path):
    M.case_hooks_2024("cuda", str(tmp_path))
