"""CPU (fiber-emulator) runs of the gradient-clipping cases (tests/clip_cases.py)."""
import pytest

from tests import clip_cases as C
from tests.emu_support import emu, emu_sequential  # noqa: F401


def test_sqnorm_kernel(emu):
    C.case_sqnorm("cpu")


def test_sqnorm_bits_in_sequential_mode(emu_sequential):
    """In-order workgroups give the bits the threaded run gives: no addition order depends on scheduling."""
    C.case_sqnorm("cpu", sizes=(257, 2048 * 256 + 3))


def test_adam_clipped_kernel(emu):
    C.case_adam_clipped("cpu")


def test_adam_clipped_inf_and_nan(emu):
    C.case_adam_clipped_nonfinite("cpu")


def test_fused_adam_clip_vs_float64_torch(emu):
    C.case_fused_adam_clip_host("cpu")


def test_lightning_surface_clip_2023_task(emu):
    """(Clips of the length the thresholds were measured at; four steps per run keep the emulator's time in minutes.)"""
    C.case_lightning_surface_clip("cpu", epochs=2, per_epoch=2)


def test_lightning_surface_clip_2024_task(emu):
    C.case_lightning_surface_clip("cpu", recipe2024=True, epochs=2, per_epoch=2)


def test_step_bit_reproducible_clip(emu_sequential):
    C.case_step_bit_reproducible_clip("cpu")


def test_pad_lanes_of_the_gradient_arena_stay_zero(emu):
    C.case_pad_lanes("cpu", n_samp=2048 + 1024)
