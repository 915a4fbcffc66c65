"""GPU runs (`pytest -m gpu`) of the n_RNN_cell = 256 cases (tests/rnn256_cases.py) through the real library.
(The file name sorts behind the other GPU test files on purpose: they run in one process, and the streams, graphs and memory pools
these cases create should not shift the state the older tests have always run in.)"""
import pytest
import torch

from tests import contraction_cases as C
from tests import rnn256_cases as R
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def wide_recurrence():
    with R.wide_recurrence():
        yield


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("B,T,I", R.EMU_BIGRU_SHAPES[:1] + R.GPU_BIGRU_SHAPES)
def test_bigru_layer_vs_torch(B, T, I):
    R.case_bigru("cuda", B, T, I)


@pytest.mark.parametrize("NC,p,B,T", ((27, 0.5, 2, 70), (10, 0.5, 2, 70), (27, 0.0, 2, 70), (27, 0.5, 3, 156), (10, 0.5, 3, 156)))
def test_head_vs_torch(NC, p, B, T):
    R.case_head("cuda", NC, p, B=B, T=T)


def test_head_masks_vs_torch():
    R.case_head_masked("cuda")


def test_backward_entries_whole_and_split():
    R.case_backward_entries_whole_and_split("cuda")


def test_gemm_calls_of_the_layer():
    C.case_caller_rows("cuda", bts=((4, 156),), his=((256, 128), (256, 512)), variants=("default",))


def test_crnn_vs_reference_golden():
    R.case_crnn_vs_reference_golden("cuda", R.golden())


@pytest.mark.timeout(600)
def test_step_2024_plain_equals_pipelined_eager_and_graph_and_two_eager_runs_bit_identical():
    R.case_step_2024_three_drivers("cuda", graph=True, repeat_plain=True)


@pytest.mark.timeout(600)
def test_step_two_eager_runs_and_graph_replay_bit_identical():
    R.case_step_eager_equals_graph("cuda")


@pytest.mark.timeout(600)
def test_step_2024_eager_equals_graph_replay():
    R.case_step_2024_eager_equals_graph("cuda")


@pytest.mark.timeout(600)
def test_training_step_2023_two_layers_vs_oracle():
    R.case_training_step_2023_vs_oracle("cuda")


def test_other_widths_are_refused():
    R.case_refusals("cuda")
