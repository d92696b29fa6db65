"""The imitation loss (include/gnnb.h gnnb_imitation_step_rows) restated with Python and numpy floats, and a twin
of the step for tests/test_imitation_cpu.py and tests/test_gpu_imitation.py.

``rule`` is the loss of ONE sample, written from the issue's statement and nothing else: candidates = the entries of the table row that
are not NaN; teacher = their arg-max on (value descending, flat index ascending); for every other candidate q
delta = float32(margin * (tau[t] - tau[q])) with the product in fp64, term = float32(float32(s[q] - s[t]) + delta), a violator iff
term > 0; loss = float32(fsum of the violators' terms); ds = +1 per violator, minus their number at the teacher.  ``math.fsum`` is the
exactly rounded sum, so the loss here is the correctly rounded one and the kernel's fixed-order fp64 sum is held to 1 fp32 ulp of it.

``ImitationOracle`` is oracle.online_oracle.OnlineOracle -- its parameters, ``oracle_forward`` and optimiser -- under this loss, in fp32
and fp64; its ``step`` takes the table where OnlineOracle's takes the KW indices and the margin where it takes the improvements, so it
can stand in for OnlineOracle inside tests.test_online_gradients.check_gradient's ReLU-kink re-examination."""
import math

import numpy as np
import torch
from torch.nn import functional as F

from oracle import gnn_oracle
from oracle.gnn_oracle import oracle_forward
from oracle.online_oracle import OnlineOracle

NAN = float("nan")
F32 = np.float32
REFUSED = ([-1, -1, 0, 0], NAN)


def rule(s, mask, tau, margin):
    """One sample.  s, mask: (R) fp32; tau: (R) fp64; margin: a float >= 0.  Returns (loss float32 or NaN, ds (R) float32, report
    [teacher, pick, n_cand, n_viol], regret float, status 0 or 8)."""
    s, mask, tau = np.asarray(s, F32), np.asarray(mask, F32), np.asarray(tau, np.float64)
    R = s.size
    ds = np.zeros(R, F32)
    C = [r for r in range(R) if not math.isnan(tau[r])]
    if any(mask[r] == 0 or math.isinf(tau[r]) for r in C):
        return F32(NAN), ds, list(REFUSED[0]), NAN, 8
    if not C:
        return F32(NAN), ds, list(REFUSED[0]), NAN, 0
    t = min(C, key=lambda r: (-tau[r], r))
    pick = min(C, key=lambda r: (-float(s[r]), r))
    terms = []
    for q in C:
        if q == t:
            continue
        delta = F32(float(margin) * (float(tau[t]) - float(tau[q])))        # fp64 product, rounded once
        term = F32(F32(s[q] - s[t]) + delta)
        if term > 0:
            terms.append(float(term))
            ds[q] += F32(1.0)
    if terms:
        ds[t] -= F32(len(terms))
    return F32(math.fsum(terms)), ds, [t, pick, len(C), len(terms)], float(tau[t]) - float(tau[pick]), 0


def rule_rows(s, mask, tau, margin):
    """``rule`` per row of (n, R) arrays: (loss (n) fp32, ds (n, R) fp32, report (n, 4) int32, regret (n) fp64, status)."""
    out = [rule(a, b, c, margin) for a, b, c in zip(s, mask, tau)]
    status = 0
    for o in out:
        status |= o[4]
    return (np.array([o[0] for o in out], F32), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.float64), status)


def ulp32(x):
    return float(np.spacing(np.abs(F32(x))))


def seeded_table(masks, M, seed):
    """(B, R) fp64: per sample M of its undecided nodes (None: all of them), seeded, with improvements uniform in [0, 1]; NaN elsewhere."""
    g = np.random.RandomState(seed)
    masks = np.asarray(masks)
    tab = np.full(masks.shape, NAN, np.float64)
    for b in range(masks.shape[0]):
        idx = np.flatnonzero(masks[b])
        if M is not None:
            idx = np.sort(g.choice(idx, size=min(M, idx.size), replace=False))
        tab[b, idx] = g.uniform(0.0, 1.0, idx.size)
    return tab


class ImitationOracle(OnlineOracle):
    """OnlineOracle under the imitation loss.  After ``step``: ``terms`` (per sample {flat index: term as a Python float} over the
    candidates but the teacher, in the oracle's dtype) and ``violators`` (per sample the sorted flat indices with term > 0)."""

    def step(self, forward_args, table, margin, apply=True, relu_tap=None):
        lbs, ubs, duals, prim, x_lp, layers, masks = forward_args
        if relu_tap is not None:
            gnn_oracle.F = relu_tap
        try:
            scores = oracle_forward(self.params, lbs, ubs, duals, prim, x_lp, layers, masks, T=self.T, dtype=self.dtype)
        finally:
            gnn_oracle.F = F
        table = np.asarray(table, np.float64).reshape(len(scores), -1)
        losses, self.terms, self.violators = [], [], []
        for b, s in enumerate(scores):
            flat = np.flatnonzero(np.asarray(masks[b]))                       # ragged position -> flat ReLU index
            pos = {int(f): i for i, f in enumerate(flat)}
            C = [r for r in range(table.shape[1]) if not math.isnan(table[b, r])]
            assert all(r in pos and not math.isinf(table[b, r]) for r in C), "the twin's tables name undecided nodes and finite improvements"
            terms, loss = {}, s.sum() * 0
            if C:
                t = min(C, key=lambda r: (-table[b, r], r))
                for q in C:
                    if q == t:
                        continue
                    delta = float(margin) * (table[b, t] - table[b, q])
                    if self.dtype == torch.float32:
                        delta = float(F32(delta))
                    term = (s[pos[q]] - s[pos[t]]) + delta
                    terms[q] = float(term.detach())
                    if terms[q] > 0:
                        loss = loss + term
            losses.append(loss)
            self.terms.append(terms)
            self.violators.append(sorted(q for q, v in terms.items() if v > 0))
        self.opt.zero_grad()
        torch.stack(losses).sum().backward()
        if apply:
            self.opt.step()
        return np.array([float(l.detach()) for l in losses], np.float32 if self.dtype == torch.float32 else np.float64), [s.detach() for s in scores]
