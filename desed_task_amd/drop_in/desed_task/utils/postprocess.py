"""desed_task.utils.postprocess -> ClassWiseMedianFilter of desed_task_amd.postprocess (run on the device by batched_decode_preds)."""
from desed_task_amd.postprocess import ClassWiseMedianFilter  # noqa: F401
