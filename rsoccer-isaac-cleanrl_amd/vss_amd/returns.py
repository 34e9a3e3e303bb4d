"""A rollout's advantages and returns in one launch: vss_gae (csrc/vss_returns.hip, include/vss.h).

gae() computes what ppo_continuous_action_isaacgym.compute_gae computes, bit for bit, on a GPU: the reversed
scan over the T steps runs inside one kernel, one lane per learner row, instead of nine torch kernels per
step.  With term_values / v_last (form B) it also does TerminalValues.next_values' merge in the kernel."""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _native as N


def kernel_selected(device) -> bool:
    """Whether the train loop computes advantages and returns with vss_gae on `device`: on a GPU, unless
    VSS_GAE=torch asks for compute_gae there (the two are bit-identical).  Read when called --
    train() calls it -- not at import."""
    mode = os.environ.get("VSS_GAE", "")
    if mode not in ("", "torch"):
        raise ValueError(f"VSS_GAE={mode!r}: expected 'torch' (compute_gae on the GPU) or nothing (vss_gae)")
    return torch.device(device).type == "cuda" and mode != "torch"


def gamma_lambda(gamma: float, lam: float) -> float:
    """The recurrence's constant as torch multiplies by it: Python's double product gamma * lam, rounded once
    to float32 -- not float32(gamma) * float32(lam), which is another number for some settings (0.997, 0.9)."""
    return ctypes.c_float(float(gamma) * float(lam)).value


def _extent(t: torch.Tensor):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _check(name: str, t, shape, device) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"gae: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"gae: {name} must be float32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"gae: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if t.device != device:
        raise ValueError(f"gae: {name} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"gae: {name} must be contiguous")


@torch.no_grad()
def gae(rewards, values, next_dones, next_timeouts, gamma, lam, *, next_values=None, term_values=None, v_last=None,
        out=None):
    """(advantages, returns) of compute_gae for (T, E) float32 rollout storage on one GPU.

    Form A: next_values (T, E), as compute_gae takes it.  Form B: term_values (T, E) and v_last (E,) --
    next_values[t] = where(next_dones[t] != 0, term_values[t], values[t + 1]) with v_last above the last step,
    selected in the kernel (rows of term_values that did not reset are never read into a sum).  Exactly one
    form.  out = (advantages, returns): (T, E) buffers written in place (they must not overlap an input or each
    other); allocated when None."""
    if not isinstance(rewards, torch.Tensor) or rewards.dim() != 2:
        raise ValueError("gae: rewards must be a (T, E) tensor")
    device = N.require_device(rewards.device)
    T, E = rewards.shape
    if (term_values is None) != (v_last is None):
        raise ValueError("gae: term_values and v_last come together (form B)")
    if (next_values is None) == (term_values is None):
        raise ValueError("gae: give either next_values (form A) or term_values and v_last (form B)")
    inputs = {"rewards": rewards, "values": values, "next_dones": next_dones, "next_timeouts": next_timeouts}
    if next_values is not None:
        inputs["next_values"] = next_values
    else:
        inputs["term_values"] = term_values
    for name, t in inputs.items():
        _check(name, t, (T, E), device)
    if v_last is not None:
        _check("v_last", v_last, (E,), device)
        inputs["v_last"] = v_last
    gamma = float(gamma)
    gl = gamma_lambda(gamma, lam)
    if not (math.isfinite(gamma) and math.isfinite(gl)):
        raise ValueError(f"gae: gamma {gamma} and gamma * lambda {gl} must be finite")
    if out is None:
        advantages, returns = torch.empty_like(rewards), torch.empty_like(rewards)
    else:
        advantages, returns = out
        _check("out[0] (advantages)", advantages, (T, E), device)
        _check("out[1] (returns)", returns, (T, E), device)
        spans = [("out[0]", _extent(advantages)), ("out[1]", _extent(returns))]
        for oname, (lo, hi) in spans:
            for name, t in inputs.items():
                ilo, ihi = _extent(t)
                if lo < ihi and ilo < hi:
                    raise ValueError(f"gae: {oname} overlaps {name}")
        if T * E and spans[0][1][0] < spans[1][1][1] and spans[1][1][0] < spans[0][1][1]:
            raise ValueError("gae: out[0] overlaps out[1]")
    if T == 0 or E == 0:  # nothing to do (an empty tensor has no address to pass)
        return advantages, returns
    N.check(N.load().vss_gae(N.stream_of(device), T, E, rewards.data_ptr(), values.data_ptr(), N.ptr(next_values),
                             N.ptr(term_values), N.ptr(v_last), next_dones.data_ptr(), next_timeouts.data_ptr(),
                             gamma, gl, advantages.data_ptr(), returns.data_ptr()), "vss_gae")
    return advantages, returns
