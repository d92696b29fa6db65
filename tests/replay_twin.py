"""The replay buffer's rules restated in Python, for tests/test_replay_cpu.py and tests/test_gpu_replay.py:
the sampler's keys and selection on numpy uint64, the push rule of a listed row, and a ring of Python objects that follows both."""
import math

import numpy as np

U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)


def ns_mix(z):
    """The splitmix64 finaliser on a numpy uint64 scalar or array (arithmetic mod 2^64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U64)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def keys(filled, seed, draw):
    """key_j for j = 0..filled - 1: base = ns_mix(seed ^ ns_mix(draw + 1)), key_j = ns_mix(base + GOLDEN (j + 1))."""
    with np.errstate(over="ignore"):
        base = ns_mix(U64(seed) ^ ns_mix(U64(draw) + U64(1)))
        j = np.arange(filled, dtype=U64)
        return ns_mix(base + GOLDEN * (j + U64(1)))


def sample(filled, n, seed, draw):
    """The n entries gnnb_replay_sample writes: the min(n, filled) slots with the smallest (key_j, j), ascending; -1 beyond."""
    k = keys(filled, seed, draw)
    order = np.lexsort((np.arange(filled), k))[:n]          # (the last key is the primary one: key, then j)
    return [int(j) for j in order] + [-1] * (n - len(order))


def row_class(tau, mask):
    """A table row against its mask row: "stored", "silent" (0 or 1 candidates) or "refused" (a candidate at a decided node or +-inf)."""
    cand = [i for i, v in enumerate(tau) if not math.isnan(v)]
    if any(mask[i] == 0 or math.isinf(tau[i]) for i in cand):
        return "refused"
    return "stored" if len(cand) >= 2 else "silent"


def push(table, mask, rows, K, C, state):
    """gnnb_replay_push's ranking of the listed rows: (slot per listed row or -1, the new state word, the status word)."""
    head, filled = state[0], state[1]
    slots, stored, status = [], 0, 0
    for r in rows:
        c = "refused" if not 0 <= r < K else row_class(list(table[r]), list(mask[r]))
        status |= 8 if c == "refused" else 0
        if c == "stored":
            slots.append((head + stored) % C)
            stored += 1
        else:
            slots.append(-1)
    return slots, [(head + stored) % C, min(C, filled + stored), stored, len(rows) - stored], status


class Ring:
    """A replay buffer of Python objects under the same two rules: ``push`` stores (item, table row) pairs, ``draw`` lists the pairs
    of a draw."""

    def __init__(self, capacity):
        self.capacity, self.state, self.slots = capacity, [0, 0, 0, 0], [None] * capacity

    def push(self, items, table, mask):
        rows = list(range(len(items)))
        slots, self.state, status = push(table, mask, rows, len(items), self.capacity, self.state)
        for i, s in enumerate(slots):
            if s >= 0:
                self.slots[s] = (items[i], np.array(table[i], dtype=np.float64))
        return status

    @property
    def filled(self):
        return self.state[1]

    def draw(self, n, seed, draw):
        idx = sample(self.filled, n, seed, draw)
        return idx, [self.slots[j] for j in idx]
