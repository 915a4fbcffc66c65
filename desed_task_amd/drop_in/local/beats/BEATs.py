"""`from local.beats.BEATs import BEATsModel, BEATs, BEATsConfig` (train_pretrained.py, extract_embeddings.py) -> the frozen
extractor on the HIP kernels."""
from desed_task_amd.beats import BEATs, BEATsConfig, BEATsModel  # noqa: F401
