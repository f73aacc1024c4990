"""Float64 numpy restatement of the three gradient-clipping modes the device step implements (torch 2.10
``torch.nn.utils.clip_grad_norm_`` with ``error_if_nonfinite=False`` and ``clip_grad_value_``), composed with tests/optim_rules64.py:
tests/test_grad_clip_host.py pins the composition to the reference's recorded steps (tests/golden/g18_clip_*.npz), the GPU tests judge
the device against it.  ``clip`` is a dict: ``max_norm`` + ``norm_type`` (2.0 or inf), or ``value``.  The clipped quantity is the
gradient of the loss (regulariser term included); weight decay is added afterwards, inside the optimizer's rule."""
import numpy as np


def total_norm(grads, norm_type=2.0):
    """the global norm over a list of arrays: sqrt of the sum of squares, or the largest magnitude (NaN-propagating, as torch's)"""
    gs = [np.asarray(g, np.float64).ravel() for g in grads]
    if norm_type == float("inf"):
        m = 0.0
        for g in gs:
            if g.size:
                m = np.maximum(m, np.max(np.abs(g)))      # (np.max / np.maximum propagate NaN)
        return float(m)
    if norm_type != 2.0:
        raise KeyError(norm_type)
    return float(np.sqrt(sum(float(np.sum(g * g)) for g in gs)))


def coefficient(total, max_norm):
    """``clamp(max_norm / (total + 1e-6), max=1)``: a NaN stays a NaN"""
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(total) + 1e-6)
    return float(c) if not c > 1.0 else 1.0


def clip_norm(grads, max_norm, norm_type=2.0):
    """``(clipped gradients, total norm, coefficient)``: every gradient times the coefficient, always (also when it is 1)"""
    total = total_norm(grads, norm_type)
    c = coefficient(total, max_norm)
    with np.errstate(all="ignore"):
        return [np.asarray(g, np.float64) * c for g in grads], total, c


def clip_value(grads, value):
    """element-wise clamp to [-value, +value]; a NaN stays a NaN"""
    out = []
    for g in grads:
        g = np.asarray(g, np.float64)
        out.append(np.where(g < -value, -value, np.where(g > value, value, g)))
    return out


def clipped(grads, clip):
    """``(clipped gradients, total norm or None, coefficient or None)`` for a clip dict (None / empty: unclipped)"""
    if not clip:
        return [np.asarray(g, np.float64) for g in grads], None, None
    if "value" in clip:
        return clip_value(grads, clip["value"]), None, None
    return clip_norm(grads, clip["max_norm"], clip.get("norm_type", 2.0))
