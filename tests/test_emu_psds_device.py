"""CPU (fiber-emulator) runs of the device-PSDS cases (tests/psds_device_cases.py): the `sed_psds_steps` kernel against
`_clip_class_steps` for every (clip, class), `psds_from_score_buffer` against `psds_from_scores`, the score tables, the errors, and the
2023 / 2024 trainer hooks with `training.device_psds` on and off."""
import pytest

from tests import psds_device_cases as M
from tests.emu_support import emu  # noqa: F401


@pytest.mark.parametrize("setting", sorted(M.SETTINGS))
@pytest.mark.parametrize("name", M.CPU_CASES)
def test_kernel_steps_equal_the_host_steps(emu, name, setting):
    M.case_kernel("cpu", name, setting)


@pytest.mark.parametrize("setting", sorted(M.SETTINGS))
@pytest.mark.parametrize("name", M.CPU_CASES)
def test_psds_from_score_buffer_equals_psds_from_scores(emu, name, setting):
    M.case_end_to_end("cpu", name, setting)


def test_class_subset(emu):
    M.case_class_subset("cpu")


def test_tables_and_written_files(emu, tmp_path):
    M.case_tables("cpu", str(tmp_path))


def test_errors(emu):
    M.case_errors("cpu")


def test_hooks_2023_flag_on_equals_flag_off(emu, tmp_path):
    M.case_hooks_2023("cpu", str(tmp_path))


def test_hooks_2024_flag_on_equals_flag_off(emu, tmp_path):
    M.case_hooks_2024("cpu", str(tmp_path))
