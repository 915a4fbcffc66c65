"""CPU (fiber-emulator) runs of the device-F1 cases (tests/f1_device_cases.py): the `sed_f1_counts` kernel against the host classes for
every (threshold, clip, class), `DecodedScores.to_dataframe()` against `batched_decode_preds`, the two public functions against their
host paths, the errors, the host-only discrimination of lazy variants, and the 2023 / 2024 trainer hooks with `training.device_f1`
on and off."""
import pytest

from tests import f1_device_cases as M
from tests.emu_support import emu  # noqa: F401


@pytest.mark.parametrize("name", M.CPU_CASES)
def test_kernel_fields_equal_the_host_fields(emu, name):
    M.case_kernel("cpu", name)


@pytest.mark.parametrize("name", M.CPU_CASES)
def test_to_dataframe_equals_batched_decode_preds(emu, name):
    M.case_dataframe("cpu", name)


@pytest.mark.parametrize("name", M.CPU_CASES)
def test_f1_scores_equal_the_host_functions(emu, name, tmp_path):
    M.case_end_to_end("cpu", name, str(tmp_path))


def test_written_reports(emu, tmp_path):
    M.case_written_reports("cpu", str(tmp_path))


def test_class_and_clip_subset(emu, tmp_path):
    M.case_class_subset("cpu", str(tmp_path))


def test_errors(emu):
    M.case_errors("cpu")


def test_lazy_variants_change_a_field():
    M.case_discrimination()


@pytest.mark.parametrize("obj_type", [None, "event", "intersection"])
def test_hooks_2023_flag_on_equals_flag_off(emu, tmp_path, obj_type):
    M.case_hooks_2023("cpu", str(tmp_path), obj_type)


def test_hooks_2024_flag_on_equals_flag_off(emu, tmp_path):
    M.case_hooks_2024("cpu", str(tmp_path))
