"""Guard bands around every buffer of excenv_policy_param_grad (helpers_guard): the C entry straight through ctypes, every buffer of
the call carved from one pattern-filled allocation, the workspace of exactly the reported bytes included. B = 1 and 326, K = 0, 1 and
7, the networks N2 / N1 / N0, both element types: the guards are untouched (the workspace's bands too), params / obs_traj / grad_raw
are unchanged, every element of grad_params is written, the outputs equal those of the same call on ordinary tensors bit for bit, and
a workspace filled with NaN beforehand gives the same bits (nothing is read before it is written)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers_policy as hp
import helpers_policy_param_grad as hg
from exciting_environments_amd import _native
from helpers_guard import Carved, Plain, arena_bytes

pytestmark = pytest.mark.gpu
NETS = ("N2", "N1", "N0")
SUB = 3


def _raw_call(case, activation, dtype, alloc, B, K, max_groups, ws_fill=None):
    """excenv_policy_param_grad on buffers from `alloc` (helpers_guard.Plain / Carved) -> grad_params"""
    widths = case["widths"]
    OW, A, P = widths[0], widths[-1], hg.param_count(widths)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    lane = lambda v, perm: np.ascontiguousarray(np.asarray(v).transpose(*perm)).astype(npdt)
    alloc("params", (P,), dtype, "params", fill=hg.hv.flat_params(case["W"], case["b"]).astype(npdt))
    alloc("obs_traj", (K * SUB + 1, OW, B), dtype, "obs", fill=lane(case["obs"], (1, 2, 0)))
    if K > 0:
        alloc("grad_raw", (K, A, B), dtype, "graw", fill=lane(case["graw"], (1, 2, 0)))
    need = hg.workspace_bytes(B, K, widths, max_groups)
    # (a scratch view: written and read by the launches, its guards checked like every other view's; K == 0 needs no byte of it)
    ws = alloc("workspace", (need // 8,), torch.float64, "workspace", role="scratch")
    if ws_fill is not None and ws.numel():
        ws.fill_(ws_fill)
    out = alloc("grad_params", (P,), dtype, "out")
    alloc.ready()
    w = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*widths)
    pol = _native.Policy(alloc.addr("params"), len(widths) - 1, _native.ACTIVATIONS[activation], w, None, 0.0, 0.0)
    rec = _native.PolicyParamGrad(pol, alloc.addr("obs_traj"), alloc.addr("grad_raw") if K > 0 else None, alloc.addr("grad_params"),
                                  alloc.addr("workspace"), need, max_groups)
    lib = _native.lib()
    assert lib.excenv_policy_param_grad_workspace_bytes(_native.dtype_id(dtype), B, K, ctypes.byref(pol), max_groups) == need
    dev = torch.device("cuda", torch.cuda.current_device())
    rc = lib.excenv_policy_param_grad(_native.dtype_id(dtype), B, K, SUB, ctypes.byref(rec), _native._raw_stream(dev))
    assert rc == 0, lib.excenv_last_error()
    assert _native.last_launch() == "policy_param_grad_kernel"
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B", [hp.B_MAIN, 1])
def test_the_launches_write_grad_params_and_nothing_else(B, dtype):
    elem = 4 if dtype == torch.float32 else 8
    n = 0
    for K in (0, 1, hp.K_MAIN):
        for v, net in enumerate(NETS):
            activation = hp.ACTIVATIONS[(v + K) % 2]
            widths = ((3, 8, 16)[v],) + tuple(hg.NETS[net]) + ((1, 2)[(v + K) % 2],)
            case = hg.random_case(widths, activation, B, K, SUB, 2, "float32" if elem == 4 else "float64")
            for mg in (0, 3):
                plain = Plain()
                ref = _raw_call(case, activation, dtype, plain, B, K, mg)
                place = ({}, {"out": elem, "workspace": 8}, {"params": elem, "obs": 16, "graw": elem})[(v + n) % 3]
                carved = Carved(arena_bytes(plain.sizes), place)
                got = _raw_call(case, activation, dtype, carved, B, K, mg)
                carved.arena.check(zero_filled=("grad_params",) if K == 0 else ())
                assert torch.equal(ref, got), (net, B, K, mg)
                # nothing of the workspace is read before it is written: NaN in it beforehand, the same bits
                again = _raw_call(case, activation, dtype, Plain(), B, K, mg, ws_fill=float("nan"))
                assert torch.equal(ref, again) and bool(torch.isfinite(again).all()), (net, B, K, mg)
                n += 1
    print(f"guard policy_param_grad {dtype} B={B}: {n} cases, guards untouched, inputs unchanged, grad_params written, NaN workspace the same bits")
