"""Float64 numpy restatement of the update rules the device step implements (torch 2.10 ``torch.optim``, single-tensor form), for
the optimizer tests: tests/test_optimizers_host.py pins it to the reference's recorded steps (tests/golden/g17_optim_*.npz), the GPU
tests judge the device against it.  ``t`` is the 1-based step; ``state`` holds float64 arrays under torch's own key names and is
updated in place (an absent ``momentum_buffer`` is SGD's first step: the buffer becomes the gradient, without dampening)."""
import numpy as np

STATE_KEYS = {"Adam": ("exp_avg", "exp_avg_sq"), "AdamW": ("exp_avg", "exp_avg_sq"), "SGD": ("momentum_buffer",),
              "Adagrad": ("sum",), "RMSprop": ("square_avg", "momentum_buffer")}


def state_keys(cls, kw):
    """the state tensors torch keeps for a configuration, in the order (m slot, v slot) of the kernel"""
    if cls == "SGD":
        return ("momentum_buffer",) if kw.get("momentum", 0) != 0 else ()
    if cls == "RMSprop":
        return ("momentum_buffer", "square_avg") if kw.get("momentum", 0) != 0 else ("square_avg",)
    return STATE_KEYS[cls]


def init_state(cls, kw, p):
    """what exists before the first update (Adagrad's ``sum`` is made at construction; SGD's buffer is absent)"""
    if cls == "Adagrad":
        return {"sum": np.full_like(p, kw.get("initial_accumulator_value", 0.0), dtype=np.float64)}
    if cls == "SGD":
        return {}
    return {k: np.zeros_like(p, dtype=np.float64) for k in state_keys(cls, kw)}


def update(cls, kw, t, p, g, state):
    """one update of parameter ``p`` (float64 array) with gradient ``g`` (of the loss, regulariser included); returns the new p"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    lr, wd = kw["lr"], kw.get("weight_decay", 0.01 if cls == "AdamW" else 0.0)
    decoupled = cls == "AdamW" or kw.get("decoupled_weight_decay", False)
    if wd != 0 and not decoupled:
        g = g + wd * p
    if cls in ("Adam", "AdamW"):
        b1, b2 = kw.get("betas", (0.9, 0.999))
        eps = kw.get("eps", 1e-8)
        if decoupled:
            p = p * (1 - lr * wd)
        m = state["exp_avg"] = state["exp_avg"] + (g - state["exp_avg"]) * (1 - b1)
        v = state["exp_avg_sq"] = b2 * state["exp_avg_sq"] + (1 - b2) * g * g
        return p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    if cls == "SGD":
        mom = kw.get("momentum", 0.0)
        d = g
        if mom != 0:
            if state.get("momentum_buffer") is None:
                buf = g.copy()
            else:
                buf = mom * state["momentum_buffer"] + (1 - kw.get("dampening", 0.0)) * g
            state["momentum_buffer"] = buf
            d = g + mom * buf if kw.get("nesterov", False) else buf
        return p - lr * d
    if cls == "Adagrad":
        clr = lr / (1 + (t - 1) * kw.get("lr_decay", 0.0))
        s = state["sum"] = state["sum"] + g * g
        return p - clr * g / (np.sqrt(s) + kw.get("eps", 1e-10))
    if cls == "RMSprop":
        alpha, mom = kw.get("alpha", 0.99), kw.get("momentum", 0.0)
        sq = state["square_avg"] = alpha * state["square_avg"] + (1 - alpha) * g * g
        q = g / (np.sqrt(sq) + kw.get("eps", 1e-8))
        if mom != 0:
            buf = state["momentum_buffer"] = mom * state["momentum_buffer"] + q
            return p - lr * buf
        return p - lr * q
    raise KeyError(cls)
