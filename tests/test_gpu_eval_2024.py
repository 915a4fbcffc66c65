"""GPU checks of the 2024 recipe's validation / test path on the MI355X: both post-processing kernels against the reference fixture
at the recipe's shape (batch_size_val 24 x 156 frames x 27 classes), windows up to 31 at B = 48 against the host filter, the
validation step at the recipe's sizes (10 s clips, 768 x 496 embeddings, valid_class_mask) against the oracle's eval-mode forward,
and one validation epoch and one test epoch end to end."""
import pytest
import torch

from tests import eval2024_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    from desed_task_amd import _lib
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _lib.use_library(None)
    lib = _lib.get()
    assert not lib.is_emulator
    return lib


def test_kernels_vs_reference_fixture_at_recipe_shape():
    C.case_kernels_vs_fixture("cuda", C.golden())


def test_classwise_filter_b48_windows_to_31_vs_host_filter():
    C.case_host_filter_equivalence("cuda", B=48, T=156, NC=27)


def test_validation_epoch_at_recipe_sizes(tmp_path):
    C.case_validation_2024("cuda", str(tmp_path), n_samp=160000, te=496, check_oracle=True)


def test_test_epoch_end_to_end(tmp_path):
    C.case_test_2024("cuda", tmp_path)
