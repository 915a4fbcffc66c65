"""n_RNN_cell = 256 on the CPU emulator build of the kernels (tests/rnn256_cases.py)."""
import pytest

from tests import contraction_cases as C
from tests import rnn256_cases as R
from tests.emu_support import emu, emu_sequential  # noqa: F401


@pytest.fixture(scope="module", autouse=True)
def wide_recurrence():
    with R.wide_recurrence():
        yield


@pytest.mark.parametrize("B,T,I", R.EMU_BIGRU_SHAPES)
def test_bigru_layer_vs_torch(emu, B, T, I):
    R.case_bigru("cpu", B, T, I)


@pytest.mark.parametrize("NC,p", ((27, 0.5), (10, 0.5), (27, 0.0)))
def test_head_vs_torch(emu, NC, p):
    R.case_head("cpu", NC, p)


def test_head_masks_vs_torch(emu):
    R.case_head_masked("cpu")


def test_backward_entries_whole_and_split(emu_sequential):
    R.case_backward_entries_whole_and_split("cpu")


def test_gemm_calls_of_the_layer(emu):
    """The GEMM calls ops.BiGRULayerFn issues at H = 256 (K / N = 768, the dX split-K over K = 1536; I = 128 and 512) as rows of
    tests/contraction_cases.py's caller table."""
    C.case_caller_rows("cpu", bts=((1, 19),), his=((256, 128), (256, 512)))


def test_oracle_vs_reference_golden():
    R.case_oracle_vs_reference_golden(R.golden())


def test_crnn_vs_reference_golden(emu):
    R.case_crnn_vs_reference_golden("cpu", R.golden())


@pytest.mark.timeout(900)
def test_step_2024_plain_equals_pipelined(emu):
    R.case_step_2024_three_drivers("cpu", graph=False)


@pytest.mark.timeout(900)
def test_training_step_2023_two_layers_vs_oracle(emu):
    R.case_training_step_2023_vs_oracle("cpu")


def test_other_widths_are_refused(emu):
    R.case_refusals("cpu")
