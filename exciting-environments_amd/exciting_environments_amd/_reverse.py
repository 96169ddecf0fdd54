"""What the reverse-mode mixins (_vjp.py, _step_vjp.py, _reward_vjp.py, _linearize.py) share on the way to a launch."""
from __future__ import annotations

import ctypes

import torch

from . import _native


def _leaf_list(x, fields):
    """State / PhysicalState pytree or a sequence -> list of leaves (None where absent)."""
    if x is None:
        return None
    x = getattr(x, "physical_state", x)
    if isinstance(x, (list, tuple)):
        assert len(x) == len(fields), f"expected {len(fields)} state leaves"
        return list(x)
    return [getattr(x, n, None) for n in fields]


def unsupported(env, saturated="the saturated PMSM has no reverse mode"):
    """The reason this environment's properties have no reverse mode, or None. Touches no device."""
    if getattr(env.env_properties, "saturated", False):
        return saturated
    if env._props_for(env.env_properties, env.batch_size)[1]:
        return "per-environment property arrays have no reverse mode (broadcast properties only)"
    return None


def cotangent(g, device, dtype, shape, strides=None, align=True):
    """g on the device in the working dtype as a 16-byte aligned tensor of `shape`: with `strides` (lane-major memory) itself when
    it is laid out so, else a copy; without, any tensor of as many elements whose first dimension is shape[0], made contiguous
    (align=False: wherever it starts, for arrays read one element per lane)."""
    g = g.detach()
    if g.device != device or g.dtype != dtype:
        g = g.to(device=device, dtype=dtype)
    if strides is None:
        assert g.numel() == shape[0] * (shape[1] if len(shape) > 1 else 1) and g.shape[0] == shape[0], \
            f"cotangent of shape {tuple(g.shape)}, expected {shape}"
        g = g.reshape(shape).contiguous()
        return g.clone() if align and g.data_ptr() % 16 else g
    assert tuple(g.shape) == shape, f"cotangent of shape {tuple(g.shape)}, expected {shape}"
    if tuple(g.stride()) == strides and g.data_ptr() % 16 == 0:
        return g
    buf = torch.empty_strided(shape, strides, dtype=dtype, device=device)
    buf.copy_(g)
    return buf


def opt_ptrs(tensors):
    """void*[n] of optional tensors (NULL where None); None for no list at all"""
    return None if tensors is None else (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def count_control(env):
    """excenv_control_t that carries only n_control (the calls that read no reference), None without controlled fields"""
    if not env.control_state:
        return None
    control = _native.Control()
    control.n_control = len(env.control_state)
    return control
