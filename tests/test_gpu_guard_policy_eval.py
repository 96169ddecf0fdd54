"""Guard bands around every buffer of excenv_policy_eval and excenv_gae (helpers_guard): the C entries straight through ctypes, every
buffer of a call carved from one pattern-filled allocation. B = 1 and 326, R or K = 1 and 7, the networks N2 / N1 / N0, both element
types, the flag bytes at offsets 4, 2 and 1, with and without each optional pointer: the guards are untouched, the inputs are
unchanged, every element of the outputs is written, the outputs equal those of the same call on ordinary tensors bit for bit, and
outputs filled with NaN beforehand give the same bits (nothing is read before it is written)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers_gae as hgae
import helpers_policy as hp
import helpers_policy_param_grad as hg
from exciting_environments_amd import _native
from helpers_guard import Carved, Plain, arena_bytes

pytestmark = pytest.mark.gpu
NETS = ("N2", "N1", "N0")
STRIDE = 3


def _raw_eval(case, activation, dtype, alloc, B, R, out_fill=None):
    """excenv_policy_eval on buffers from `alloc` (helpers_guard.Plain / Carved) -> out [R, A, B]"""
    widths = case["widths"]
    OW, A, P = widths[0], widths[-1], hg.param_count(widths)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    alloc("params", (P,), dtype, "params", fill=hg.hv.flat_params(case["W"], case["b"]).astype(npdt))
    # exactly the rows the call may read: (R - 1) * row_stride + 1
    rows = (R - 1) * STRIDE + 1
    alloc("obs_traj", (rows, OW, B), dtype, "obs", fill=np.ascontiguousarray(case["obs"][:, :rows].transpose(1, 2, 0)).astype(npdt))
    out = alloc("out", (R, A, B), dtype, "out")
    if out_fill is not None:
        out.fill_(out_fill)
    alloc.ready()
    w = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*widths)
    pol = _native.Policy(alloc.addr("params"), len(widths) - 1, _native.ACTIVATIONS[activation], w, None, 0.0, 0.0)
    rec = _native.PolicyEval(pol, alloc.addr("obs_traj"), alloc.addr("out"))
    lib = _native.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    rc = lib.excenv_policy_eval(_native.dtype_id(dtype), B, R, STRIDE, ctypes.byref(rec), _native._raw_stream(dev))
    assert rc == 0, lib.excenv_last_error()
    assert _native.last_launch() == "policy_eval_kernel"
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B", [hp.B_MAIN, 1])
def test_policy_eval_writes_out_and_nothing_else(B, dtype):
    elem = 4 if dtype == torch.float32 else 8
    n = 0
    for R in (1, hp.K_MAIN):
        for v, net in enumerate(NETS):
            activation = hp.ACTIVATIONS[(v + R) % 2]
            widths = ((3, 8, 16)[v],) + tuple(hg.NETS[net]) + ((1, 2)[(v + R) % 2],)
            case = hg.random_case(widths, activation, B, R, STRIDE, 2, "float32" if elem == 4 else "float64")
            plain = Plain()
            ref = _raw_eval(case, activation, dtype, plain, B, R)
            for place in ({}, {"out": elem}, {"params": elem, "obs": 16}, {"obs": elem, "out": 16}):
                carved = Carved(arena_bytes(plain.sizes), place)
                got = _raw_eval(case, activation, dtype, carved, B, R)
                carved.arena.check()
                assert torch.equal(ref, got), (net, B, R, place)
                n += 1
            # nothing of `out` is read: NaN in it beforehand, the same bits
            again = _raw_eval(case, activation, dtype, Plain(), B, R, out_fill=float("nan"))
            assert torch.equal(ref, again) and bool(torch.isfinite(again).all()), (net, B, R)
    print(f"guard policy_eval {dtype} B={B}: {n} carved cases, guards untouched, inputs unchanged, out written, NaN out the same bits")


def _raw_gae(case, dtype, alloc, B, K, gamma, lam, with_term, with_reset, with_ret, out_fill=None):
    """excenv_gae on buffers from `alloc` -> (advantage [K, B], returns [K, B] or None)"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    lane = lambda x, t: np.ascontiguousarray(np.asarray(x).T).astype(t)
    alloc("reward", (K, B), dtype, "reward", fill=lane(case["reward"], npdt))
    alloc("value", (K + 1, B), dtype, "value", fill=lane(case["value"], npdt))
    if with_term:
        alloc("terminated", (K, B), torch.uint8, "terminated", fill=lane(case["terminated"], np.uint8))
    if with_reset:
        alloc("reset", (K, B), torch.uint8, "reset", fill=lane(case["reset"], np.uint8))
    adv = alloc("advantage", (K, B), dtype, "advantage")
    ret = alloc("returns", (K, B), dtype, "returns") if with_ret else None
    if out_fill is not None:
        adv.fill_(out_fill)
        if ret is not None:
            ret.fill_(out_fill)
    alloc.ready()
    hgae.raw_gae(dtype, B, K, alloc.addr("reward"), alloc.addr("value"), alloc.addr("terminated") if with_term else None,
                 alloc.addr("reset") if with_reset else None, gamma, lam, alloc.addr("advantage"), alloc.addr("returns") if with_ret else None)
    torch.cuda.synchronize()
    return adv, ret


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B", [hp.B_MAIN, 1])
def test_gae_writes_its_outputs_and_nothing_else(B, dtype):
    elem = 4 if dtype == torch.float32 else 8
    npdt = np.float32 if elem == 4 else np.float64
    n = 0
    for K in (1, hp.K_MAIN):
        case = hgae.gae_case(B, K, np.dtype(npdt).name)
        for v, (with_term, with_reset, with_ret) in enumerate(((True, True, True), (False, True, True), (True, False, True), (True, True, False),
                                                               (False, False, False))):
            gamma, lam = hgae.DISCOUNTS[v % 3]
            plain = Plain()
            ref_a, ref_r = _raw_gae(case, dtype, plain, B, K, gamma, lam, with_term, with_reset, with_ret)
            want_a, want_r = hgae.gae_twin(case["reward"], case["value"], gamma, lam, case["terminated"] if with_term else None,
                                           case["reset"] if with_reset else None, npdt)
            assert hgae.same_bits(ref_a.t().cpu().numpy(), want_a) and (ref_r is None or hgae.same_bits(ref_r.t().cpu().numpy(), want_r))
            places = ({}, {"terminated": 4, "reset": 2}, {"terminated": 2, "reset": 1}, {"terminated": 1, "reset": 4},
                      {"reward": elem, "value": 16, "advantage": elem, "returns": 16})
            for place in places:
                carved = Carved(arena_bytes(plain.sizes), place)
                got_a, got_r = _raw_gae(case, dtype, carved, B, K, gamma, lam, with_term, with_reset, with_ret)
                carved.arena.check()
                assert torch.equal(ref_a, got_a) and (ref_r is None or torch.equal(ref_r, got_r)), (B, K, v, place)
                n += 1
            again_a, again_r = _raw_gae(case, dtype, Plain(), B, K, gamma, lam, with_term, with_reset, with_ret, out_fill=float("nan"))
            assert torch.equal(ref_a, again_a) and (ref_r is None or torch.equal(ref_r, again_r)) and bool(torch.isfinite(again_a).all())
    print(f"guard gae {dtype} B={B}: {n} carved cases, guards untouched, inputs unchanged, outputs written, NaN outputs the same bits")
