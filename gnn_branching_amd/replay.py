"""Offline training of the scorer from a replay buffer of strong-branching tables.

``frontier.ReplayBuffer`` holds labelled states on the device -- ``branch_and_bound_frontier(..., imitate=Replay(every=1, steps=0))``
collects them with a frozen scorer --, and ``train_epochs`` runs epochs of minibatch steps over it, every step a
``gnnb_replay_sample`` and a ``gnnb_imitation_step_rows`` on the device.  The reference ships no training script; the loss is the
imitation step's ranking hinge (section 7.12)."""
import math

import numpy as np


def summarise(loss, report, regret, table_best=None):
    """The means of an evaluation (``ReplayBuffer.evaluate``'s three tensors) over the rows that have a teacher: mean loss, mean
    regret, mean relative regret (regret / the teacher's improvement, over the rows where that is positive) and top-1 agreement (the
    share of rows whose pick is the teacher).  table_best: the teacher's improvement per row (None: no relative regret)."""
    loss, report, regret = np.asarray(loss, np.float64), np.asarray(report), np.asarray(regret, np.float64)
    ok = report[:, 0] >= 0 if len(report) else np.zeros(0, bool)
    n = int(ok.sum())
    out = {"rows": n, "loss": math.nan, "regret": math.nan, "relative_regret": math.nan, "top1": math.nan}
    if n == 0:
        return out
    out.update(loss=float(loss[ok].mean()), regret=float(regret[ok].mean()), top1=float((report[ok, 0] == report[ok, 1]).mean()))
    if table_best is not None:
        best = np.asarray(table_best, np.float64)[ok]
        pos = best > 0
        if pos.any():
            out["relative_regret"] = float((regret[ok][pos] / best[pos]).mean())
    return out


def evaluate(buffer, margin=1.0):
    """``summarise`` of ``buffer.evaluate(margin)`` with the teacher's improvement read from the buffer's table."""
    loss, report, regret = buffer.evaluate(margin)
    n = len(loss)
    best = None
    if n:
        tab = buffer.table[:n].cpu().numpy()
        teacher = report[:, 0].numpy().clip(min=0)
        best = tab[np.arange(n), teacher]
    return summarise(loss.numpy(), report.numpy(), regret.numpy(), best)


def train_epochs(choice, buffer, epochs, batch=8, margin=1.0, seed=0, holdout=None):
    """Train ``choice``'s scorer on ``buffer`` for ``epochs`` epochs.  choice: a ``graphnet.graph_score_online.GraphChoice`` (it owns
    the optimizer's lr / wd); buffer: a ``frontier.ReplayBuffer`` of the network the choice's engine is bound to.  An epoch is
    ceil(filled / batch) calls of ``buffer.step(min(batch, filled), margin, seed, draw)`` with consecutive ``draw`` values that run
    through all epochs.  After each epoch ``evaluate`` of the buffer ("train") and, if given, of ``holdout`` are recorded.  At the end
    ``choice.model`` receives the device's parameters once, as the frontier loops leave them.

    Returns the per-epoch records: [{"epoch", "steps", "train": {...}, "holdout": {...} or None}], epoch 0 being the state before
    training."""
    from .frontier import REPLAY_BATCH_MAX, ReplayBuffer
    from .graphnet.graph_score_online import GraphChoice
    if not isinstance(choice, GraphChoice):
        raise TypeError(f"train_epochs needs a graphnet.graph_score_online.GraphChoice (it owns the optimizer's lr / wd), not {type(choice).__name__}")
    for name, b in (("buffer", buffer), ("holdout", holdout)):
        if not isinstance(b, ReplayBuffer) and not (name == "holdout" and b is None):
            raise ValueError(f"train_epochs: {name} is no ReplayBuffer")
    for name, v, least in (("epochs", epochs, 0), ("batch", batch, 1)):
        if isinstance(v, bool) or not isinstance(v, int) or v < least:
            raise ValueError(f"train_epochs: {name} = {v!r} (an integer >= {least})")
    if batch > REPLAY_BATCH_MAX:
        raise ValueError(f"train_epochs: batch = {batch} > {REPLAY_BATCH_MAX}, the most one draw holds")
    eng = choice._eng()
    if eng.sizes is None or list(eng.sizes) != buffer.sizes:
        eng.bind(buffer.engine._net_keepalive, _input_shape(buffer.engine))
    for b in (buffer, holdout):
        if b is not None:
            if b.sizes != list(eng.sizes):
                raise ValueError(f"train_epochs: a buffer holds states of a network with layer sizes {b.sizes}, the scorer's engine is bound to {list(eng.sizes)}")
            b.engine = eng
    buffer.read_state()
    if buffer.filled < 1:
        raise ValueError("train_epochs: the buffer is empty")
    n = min(batch, buffer.filled)
    per_epoch = (buffer.filled + batch - 1) // batch

    def record(epoch, steps):
        return {"epoch": epoch, "steps": steps, "train": evaluate(buffer, margin), "holdout": None if holdout is None else evaluate(holdout, margin)}
    records, draw = [record(0, 0)], 0
    try:
        for e in range(1, epochs + 1):
            for _ in range(per_epoch):
                buffer.step(n, margin, seed, draw)
                draw += 1
            records.append(record(e, draw))
    finally:
        if draw:
            choice.model.load_blob(eng.get_weights())             # the nn.Module mirrors the device
    return records


def _input_shape(engine):
    """The input shape the engine's network was bound with."""
    return engine._net_key[2]
