"""Bidirectional GRU container (state-dict layout of desed_task/nnet/RNN.py:7-30: `rnn.weight_ih_l{k}[_reverse]` ...).
nn.GRU is used as the parameter holder / initialiser only; the arithmetic is ops.BiGRULayerFn.
n_hidden: 128 (2023 recipe), 192 (2024 recipe) or 256 (the widest n_RNN_cell of the 2024 recipe's search; opt-in, ops.GRU_WIDE / SED_GRU_WIDE=1); other widths raise."""
import torch.nn as nn

from .. import ops as _ops
from ..ops import BiGRULayerFn


class BidirectionalGRU(nn.Module):
    def __init__(self, n_in, n_hidden, dropout=0, num_layers=1, gemm_precision=None):
        super().__init__()
        # arithmetic of the input projections and their gradients (ops.gemm_entry): None = SED_GEMM_PRECISION or "bf16x3"; the
        # recurrence and the gate math are fp32 in every mode
        if gemm_precision is not None and gemm_precision not in _ops.PRECISIONS:
            raise ValueError("gemm_precision must be 'bf16x3', 'bf16' or 'f32'")
        self.gemm_precision = gemm_precision
        if n_hidden == 256 and not _ops.GRU_WIDE:
            raise NotImplementedError("n_hidden = 256 runs on the streamed-weight GRU kernels and is opt-in: set SED_GRU_WIDE=1 (or "
                                      "desed_task_amd.ops.GRU_WIDE = True) before building the model; 128 and 192 need no switch")
        if n_hidden not in (128, 192, 256):
            raise NotImplementedError("HIP GRU kernels are built for n_hidden = 128, 192 and 256 (the 2023 / 2024 recipes' n_RNN_cell "
                                      "and the widest value of the 2024 recipe's search), not %d" % n_hidden)
        if dropout:
            raise NotImplementedError("inter-layer GRU dropout (dropout_recurrent) is not on the 2023 path")
        self.num_layers = num_layers
        self.rnn = nn.GRU(n_in, n_hidden, bidirectional=True, dropout=dropout, batch_first=True, num_layers=num_layers)

    def forward(self, input_feat, arena=None):
        x = input_feat
        cfg = dict(arena=arena, gemm_precision=self.gemm_precision)
        for k in range(self.num_layers):
            g = lambda n: getattr(self.rnn, "%s_l%d" % (n, k))          # noqa: E731
            r = lambda n: getattr(self.rnn, "%s_l%d_reverse" % (n, k))  # noqa: E731
            x = BiGRULayerFn.apply(x, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"),
                                   r("weight_ih"), r("weight_hh"), r("bias_ih"), r("bias_hh"), cfg)
        return x
