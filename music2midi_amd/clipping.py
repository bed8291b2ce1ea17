"""Gradient clipping — what pytorch-lightning 2.1.0 does with ``Trainer(gradient_clip_val=, gradient_clip_algorithm=)`` (ref:
train.py:40 passes ``config.trainer`` to ``pl.Trainer``), restated as plain rules the CPU tests drive.  The device side is
csrc/grad_clip.hip (the global norm) and the ``CLIP`` forms of the Adafactor passes (csrc/adafactor.hip).

Lightning 2.1 (``lightning.pytorch.plugins.precision.Precision.clip_gradients(optimizer, clip_val, gradient_clip_algorithm)``):

* ``clip_val <= 0`` returns at once: no clipping;
* ``"value"`` calls ``torch.nn.utils.clip_grad_value_(params, clip_val)``;
* ``"norm"`` calls ``torch.nn.utils.clip_grad_norm_(params, clip_val)`` — norm type 2.

The Trainer's defaults and validation (``Trainer.__init__`` of 2.1), as this project applies them:

* ``gradient_clip_val=None`` means off;
* ``gradient_clip_algorithm=None`` means ``"norm"``; the name is compared lower-cased;
* a ``gradient_clip_val`` that is not an int or a float (a bool, a str) is a ``TypeError``;
* any other algorithm name is a ``ValueError``.

``torch.nn.utils.clip_grad_norm_(params, max_norm)``:

* ``total = || (||g_1||_2, ..., ||g_n||_2) ||_2`` over the parameters as ``module.parameters()`` lists them (the shared embedding
  counts once) — the norm of the stack of per-tensor norms, not one flat sum;
* ``coef = min(1, max_norm / (total + 1e-6))`` (``torch.clamp(..., max=1.0)``: a NaN stays a NaN);
* every gradient is multiplied by ``coef``, also when ``coef`` is 1;
* nothing is special-cased: ``total = inf`` gives ``coef = 0`` and ``0 * inf = NaN``.

``torch.nn.utils.clip_grad_value_(params, v)``: ``g.clamp_(-v, v)``; a NaN stays a NaN.

When: clipping runs where the optimizer steps — once per accumulation window, on the summed gradient, and under data parallelism
after the gradient all-reduce (``Music2MIDI._fit_windows`` has this order: all-reduce, then ``optimizer.step()``).

One difference from Lightning, on purpose: the device step reads the clipped gradient on the fly and never writes it back, so
``.grad`` keeps the UNCLIPPED gradient after ``optimizer.step()`` (Lightning's is clipped in place).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

OFF, NORM, VALUE = "off", "norm", "value"
MODE_CODES = {OFF: 0, NORM: 1, VALUE: 2}          # the `algorithm` argument of m2m_trainer_set_grad_clip


def check_gradient_clip(val, algorithm) -> Tuple[str, float]:
    """(mode, value) of ``Trainer(gradient_clip_val=val, gradient_clip_algorithm=algorithm)``: mode is "off" (value 0.0), "norm" or
    "value".  TypeError for a clip value that is not an int or float, ValueError for an unknown algorithm."""
    if val is not None and (isinstance(val, bool) or not isinstance(val, (int, float))):
        raise TypeError(f"gradient_clip_val should be an int or a float, got {val!r}")
    if algorithm is None:
        algorithm = NORM
    if not isinstance(algorithm, str) or algorithm.lower() not in (NORM, VALUE):
        raise ValueError(f"gradient_clip_algorithm {algorithm!r} is invalid: allowed algorithms are 'norm' and 'value'")
    if val is None or not val > 0:          # None: off;  <= 0: Precision.clip_gradients returns at once  (a NaN clips nothing either)
        return OFF, 0.0
    return algorithm.lower(), float(val)


def clip_reference(grads: Sequence, mode: str, value: float):
    """The definition: torch's own clipping, in place, on a list of tensors (in the order given).  Returns the total norm
    (a 0-dim tensor) in norm mode, else None."""
    import torch
    if mode == OFF:
        return None
    params = []
    for g in grads:
        p = torch.nn.Parameter(torch.empty_like(g), requires_grad=True)
        p.grad = g
        params.append(p)
    if mode == NORM:
        return torch.nn.utils.clip_grad_norm_(params, value)
    if mode == VALUE:
        torch.nn.utils.clip_grad_value_(params, value)
        return None
    raise ValueError(f"unknown clipping mode {mode!r}")
