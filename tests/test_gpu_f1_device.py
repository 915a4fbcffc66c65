"""GPU runs (`pytest -m gpu`) of the device-F1 cases (tests/f1_device_cases.py) through the real library, two validation batches
(48 clips) included."""
import pytest
import torch

from tests import f1_device_cases as M
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("name", M.GPU_CASES)
def test_kernel_fields_equal_the_host_fields(name):
    M.case_kernel("cuda", name)


@pytest.mark.parametrize("name", M.GPU_CASES)
def test_to_dataframe_equals_batched_decode_preds(name):
    M.case_dataframe("cuda", name)


@pytest.mark.parametrize("name", M.GPU_CASES)
def test_f1_scores_equal_the_host_functions(name, tmp_path):
    M.case_end_to_end("cuda", name, str(tmp_path))


def test_written_reports(tmp_path):
    M.case_written_reports("cuda", str(tmp_path))


def test_class_and_clip_subset(tmp_path):
    M.case_class_subset("cuda", str(tmp_path))


def test_errors():
    M.case_errors("cuda")


@pytest.mark.parametrize("obj_type", [None, "event", "intersection"])
def test_hooks_2023_flag_on_equals_flag_off(tmp_path, obj_type):
    M.case_hooks_2023("cuda", str(tmp_path), obj_type)


def test_hooks_2024_flag_on_equals_flag_off(tmp_path):
    M.case_hooks_2024("cuda", str(tmp_path))
