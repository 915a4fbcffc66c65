"""GPU runs (`pytest -m gpu`) of the gradient-clipping cases (tests/clip_cases.py) through the real library.
(The file name sorts behind the other GPU test files on purpose: they run in one process, and the streams, graphs and memory pools
these cases create should not shift the state the older tests have always run in.)"""
import pytest
import torch

from tests import clip_cases as C
from desed_task_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


def test_sqnorm_kernel():
    C.case_sqnorm("cuda")


def test_adam_clipped_kernel():
    C.case_adam_clipped("cuda")


def test_adam_clipped_inf_and_nan():
    C.case_adam_clipped_nonfinite("cuda")


def test_fused_adam_clip_vs_float64_torch():
    C.case_fused_adam_clip_host("cuda")


@pytest.mark.timeout(600)
def test_lightning_surface_clip_2023_task():
    C.case_lightning_surface_clip("cuda")


@pytest.mark.timeout(600)
def test_lightning_surface_clip_2024_task():
    C.case_lightning_surface_clip("cuda", recipe2024=True)


def test_step_bit_reproducible_clip():
    """Two eager runs and the captured step (warm-up, capture, replay) of the clipped step agree bit for bit."""
    C.case_step_bit_reproducible_clip("cuda")


def test_pad_lanes_of_the_gradient_arena_stay_zero():
    C.case_pad_lanes("cuda")
