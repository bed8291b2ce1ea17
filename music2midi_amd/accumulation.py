"""Gradient accumulation windows — what pytorch-lightning 2.1.0's automatic optimisation does with
``Trainer(accumulate_grad_batches=N)`` (ref: train.py:40 passes ``config.trainer`` to ``pl.Trainer``), as plain bookkeeping that
the CPU tests drive:

* every micro-batch's backward sees ``loss / N`` — also in an incomplete last window (Lightning divides by N there too);
* the first micro-batch of a window overwrites the gradients, the others add to them;
* the optimizer (and the scheduler) steps after N micro-batches, and after the last micro-batch of the iterable when that
  window is incomplete; ``global_step`` counts those steps;
* under data parallelism the gradients are all-reduced once per window, on its last micro-batch (Lightning's ``no_sync``
  on the others).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Iterator, Tuple


def check_accumulate_grad_batches(value) -> int:
    """N as Lightning accepts it: an int >= 1 (a bool, float or string is refused)."""
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"accumulate_grad_batches must be an int >= 1, got {value!r}")
    return value


@dataclass(frozen=True)
class MicroStep:
    """What one micro-batch does: its position in the window, the factor of its loss in the backward pass, whether its gradients
    add to the buffer, and whether the gradient all-reduce and the optimizer step follow it."""
    position: int
    grad_scale: float
    accumulate: bool
    step: bool

    @property
    def sync(self) -> bool:            # the all-reduce happens exactly where the optimizer steps
        return self.step


def micro_step(n: int, position: int, last: bool = False) -> MicroStep:
    """The micro-batch at `position` (0-based) of a window of `n`; `last`: it ends the iterable."""
    n = check_accumulate_grad_batches(n)
    if not 0 <= position < n:
        raise ValueError(f"position {position} outside a window of {n}")
    return MicroStep(position, 1.0 / n, position > 0, last or position == n - 1)


def windows(batches: Iterable, n: int) -> Iterator[Tuple[object, MicroStep]]:
    """(batch, MicroStep) over an iterable of unknown length: one batch of look-ahead finds the last one."""
    n = check_accumulate_grad_batches(n)
    it = iter(batches)
    try:
        cur = next(it)
    except StopIteration:
        return
    pos = 0
    while True:
        try:
            nxt = next(it)
        except StopIteration:
            yield cur, micro_step(n, pos, last=True)
            return
        ms = micro_step(n, pos)
        yield cur, ms
        pos = 0 if ms.step else pos + 1
        cur = nxt
