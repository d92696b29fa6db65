"""CPU ORACLE for the online-learning step.  TEST INFRASTRUCTURE ONLY (see gnn_oracle.py).

Restates graphnet/graph_score_online.py:9-15 and :62-77: the GNN parameters under torch.optim.Adam(lr, weight_decay),
loss = gnn_score - kw_score + improvement with gnn_score = torch.max(scores, 0) (first maximum) and kw_score the score of
the KW decision, loss.backward(), optimizer.step().  The forward is oracle_forward (gnn_oracle.py) with the parameters as
autograd leaves; the backward pass is torch.autograd's, as in the reference.

Parity pin: tests/golden/*_online.npz hold gradients and parameters produced by the REFERENCE's own
GraphChoice.online_learning (oracle/make_golden_online.py); tests/test_online.py checks this file against them.
"""
from collections import OrderedDict

import numpy as np
import torch
from torch.nn import functional as F

from . import gnn_oracle
from .gnn_oracle import oracle_forward


def split_blob(blob, like):
    """A flat parameter / gradient blob as its named tensors in checkpoint order (`like`: a state dict, for names and shapes)."""
    blob = np.asarray(blob)
    out, off = OrderedDict(), 0
    for k, v in like.items():
        shape = tuple(np.shape(v))
        n = int(np.prod(shape))
        out[k] = blob[off:off + n].reshape(shape)
        off += n
    assert off == blob.size, (off, blob.size)
    return out


class ReluTap:
    """Stands in for torch.nn.functional inside gnn_oracle while one step runs.  Every ReLU on the differentiated path is recorded
    (`calls`: pre-activation, output with its gradient kept), and written as z * gate so that chosen gates can be flipped
    (`flips`: {index of the ReLU call: flat entry indices}).  The GNN is piecewise linear: at a pre-activation within rounding of
    zero both one-sided derivatives are right, and which one an fp32 evaluation takes depends on its summation order."""

    def __init__(self, flips=None):
        self.flips = dict(flips or {})
        self.calls = []

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, x):
        if not x.requires_grad:
            return F.relu(x)
        gate = x.detach() > 0
        i = len(self.calls)
        if i in self.flips:
            gate.view(-1)[torch.as_tensor(self.flips[i], dtype=torch.long)] ^= True
        y = x * gate.to(x.dtype)
        y.retain_grad()
        self.calls.append((x.detach(), y))
        return y


class OnlineOracle:
    """dtype: parameters, forward and Adam in that precision.  torch.float32 is the reference's arithmetic (the goldens pin it);
    torch.float64 is the yardstick the per-tensor gradient tests measure both fp32 forms against."""

    def __init__(self, state, lr=1e-4, wd=1e-4, T=2, dtype=torch.float32):
        self.T = T
        self.dtype = dtype
        self.params = OrderedDict((k, torch.nn.Parameter(torch.as_tensor(np.asarray(v)).float().to(dtype).clone())) for k, v in state.items())
        self.opt = torch.optim.Adam(list(self.params.values()), lr=lr, weight_decay=wd)       # graph_score_online.py:15

    def blob(self):
        return np.concatenate([p.detach().numpy().reshape(-1) for p in self.params.values()])

    def grad_blob(self):
        return np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).numpy().reshape(-1) for p in self.params.values()])

    def step(self, forward_args, kw_flat, improvement, apply=True, relu_tap=None):
        """forward_args: the argument tuple of GraphNet.forward for B subproblems; kw_flat (B) flat ReLU indices;
        improvement (B).  Returns (loss per subproblem, ragged scores).  relu_tap: a ReluTap for this step's forward."""
        lbs, ubs, duals, prim, x_lp, layers, masks = forward_args
        if relu_tap is not None:
            gnn_oracle.F = relu_tap
        try:
            scores = oracle_forward(self.params, lbs, ubs, duals, prim, x_lp, layers, masks, T=self.T, dtype=self.dtype)
        finally:
            gnn_oracle.F = F
        losses = []
        for b, s in enumerate(scores):
            gnn_score, _ = torch.max(s, 0)                                                    # :41
            kw_index = len(masks[b][:int(kw_flat[b])].nonzero())                              # :69
            losses.append(gnn_score - s[kw_index] + float(improvement[b]))                    # :73
        self.opt.zero_grad()                                                                  # :72
        torch.stack(losses).sum().backward()                                                  # :74
        if apply:
            self.opt.step()                                                                   # :75
        return np.array([float(l.detach()) for l in losses], np.float32 if self.dtype == torch.float32 else np.float64), [s.detach() for s in scores]
