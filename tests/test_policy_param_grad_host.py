"""Host side of the policy's parameter gradient (no GPU):
- the header and its `_native` mirror, the exports, ABI 7; excenv_policy_param_grad refuses by code and whole message, before any
  launch, what it does not do; the empty batch; the workspace function is the formula, a function of (B, K, policy, max_groups) only;
- the sample tiles: the restated tile ranges cover every tile once;
- the two kernels exist for both element types without scratch memory; the LDS formula stays within the CU's 160 KB;
- the Python methods refuse by name what they do not do, and the setter;
- the ReLU inputs of the GPU test keep their margin."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import helpers_policy as hp
import helpers_policy_param_grad as hg
from exciting_environments_amd import EnvironmentRegistry, MLPPolicy, _native
from helpers_budget import budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32 = ctypes.c_int64, ctypes.c_int32
EINVAL, ENULL = -1, -2
FN = "excenv_policy_param_grad"


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_policy_param_grad\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_policy_param_grad_workspace_bytes\s*\(", hdr)
    assert re.search(r"\}\s*excenv_policy_param_grad_t\s*;", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # additions: a binder probes for the symbols
    assert re.search(r"#define\s+EXCENV_POLICY_MAX_INPUT\s+16\b", hdr) and _native.POLICY_MAX_INPUT == 8 + _native.MAX_CONTROL
    assert re.search(r"#define\s+EXCENV_PARAM_GRAD_CHAIN\s+4096\b", hdr) and _native.PARAM_GRAD_CHAIN == 4096 <= 4096
    assert _native.PARAM_GRAD_CHAIN % hg.TILE == 0 and _native.PARAM_GRAD_AUTO_GROUPS == hg.AUTO_GROUPS
    lib = ctypes.CDLL(_native.library_path())
    assert all(hasattr(lib, n) for n in (FN, FN + "_workspace_bytes")) and _native.lib().excenv_abi_version() == 7
    assert len(_native.PROTOTYPES[FN][1]) == 6 and len(_native.PROTOTYPES[FN + "_workspace_bytes"][1]) == 5
    assert _native.STRUCTS[_native.PolicyParamGrad] == "excenv_policy_param_grad_t"
    names = [n for n, _ in _native.PolicyParamGrad._fields_]
    assert names == ["policy", "obs_traj", "grad_raw", "grad_params", "workspace", "workspace_bytes", "max_groups"]
    assert _native.PolicyParamGrad.policy.size == ctypes.sizeof(_native.Policy) and _native.PolicyParamGrad.policy.offset == 0


def test_kernels_exist_without_scratch_and_the_lds_formula():
    res, spans = budget("policy_param_grad")
    for t in "fd":
        for key in (f"policy_param_grad_kernelI{t}E", f"policy_param_grad_reduce_kernelI{t}E"):
            hit = [k for k in res if key in k]
            assert len(hit) == 1, (key, hit)
            print(key, res[hit[0]], spans[hit[0]])
    assert len(res) == 4, sorted(res)
    over = {k: v for k, v in res.items() if v["scratch"] != 0 or v["lds"] != 0 or v["vgpr"] > 512}
    assert not over, over
    # policy.hpp policy_param_grad_lds_bytes: x^0, the hidden layers, d^L and the ones row, 66 elements a row; both limits in fp64
    widest = (16, 64, 64, 64, 2)
    assert hg.lds_bytes(widest, 8) == 211 * 66 * 8 <= 160 * 1024 and hg.lds_bytes(widest, 4) == 211 * 66 * 4
    assert hg.lds_bytes((1, 1), 8) == 3 * 66 * 8 and hg.lds_bytes((8,) + hp.NETS["N2"] + (2,), 8) <= 160 * 1024


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _record(widths=(2, 5, 1), **kw):
    w = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*widths)
    pol = _native.Policy(64, len(widths) - 1, _native.ACT_TANH, w, None, -1.0, 1.0)
    for k in [k for k in kw if k.startswith("policy_")]:
        setattr(pol, k[len("policy_"):], kw.pop(k))
    r = _native.PolicyParamGrad(pol, 64, 64, 64, 64, 1 << 40, 0)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(dtype=0, B=4, K=3, sub=1, rec=None, no_rec=False):
    lib = _native.lib()
    r = rec if rec is not None else _record()
    rc = lib.excenv_policy_param_grad(dtype, i64(B), i64(K), i32(sub), None if no_rec else ctypes.byref(r), None)
    return rc, lib.excenv_last_error().decode()


def test_refusals_come_back_by_code_and_whole_message_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    assert _call(no_rec=True) == (ENULL, f"{FN}: call is NULL")
    table = [
        (dict(policy_params=None), ENULL, "call->policy.params is NULL"),
        (dict(obs_traj=None), ENULL, "call->obs_traj is NULL"),
        (dict(grad_raw=None), ENULL, "call->grad_raw is NULL"),
        (dict(grad_params=None), ENULL, "call->grad_params is NULL"),
        (dict(workspace=None), ENULL, "call->workspace is NULL"),
        (dict(policy_n_layers=0), EINVAL, "policy.n_layers must be 1 .. 4 (got 0)"),
        (dict(policy_n_layers=5), EINVAL, "policy.n_layers must be 1 .. 4 (got 5)"),
        (dict(widths=(2, 65, 1)), EINVAL, "policy.widths[1] must be 1 .. 64 (got 65)"),
        (dict(widths=(2, 5, 0, 1)), EINVAL, "policy.widths[2] must be 1 .. 64 (got 0)"),
        (dict(widths=(17, 5, 1)), EINVAL, "policy.widths[0] must be 1 .. 16 (the widest observation row; got 17)"),
        (dict(widths=(0, 5, 1)), EINVAL, "policy.widths[0] must be 1 .. 16 (the widest observation row; got 0)"),
        (dict(widths=(2, 5, 3)), EINVAL, "policy.widths[2] must be 1 .. 2 (the action width; got 3)"),
        (dict(widths=(2, 0)), EINVAL, "policy.widths[1] must be 1 .. 2 (the action width; got 0)"),
        (dict(policy_activation=2), EINVAL, "policy.activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got 2)"),
        (dict(max_groups=-1), EINVAL, "call->max_groups must not be negative (got -1; 0: auto)"),
    ]
    for kw, code, text in table:
        assert _call(rec=_record(**kw)) == (code, f"{FN}: {text}"), kw
    assert _call(dtype=2) == (EINVAL, f"{FN}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(B=-1) == (EINVAL, f"{FN}: bad B=-1, K=3 or substeps=1")
    assert _call(K=-1) == (EINVAL, f"{FN}: bad B=4, K=-1 or substeps=1")
    assert _call(sub=0) == (EINVAL, f"{FN}: bad B=4, K=3 or substeps=0")
    assert _call(K=2 ** 30, sub=2) == (EINVAL, f"{FN}: K * substeps = 1073741824 * 2 rows exceed one launch")
    # the workspace: B = 4, K = 3 are three tiles and three workgroups of 21 parameters
    need = 3 * 21 * 8
    why = f"{FN}: needs an 8-byte aligned workspace of {need} bytes (excenv_policy_param_grad_workspace_bytes)"
    assert _call(rec=_record(workspace_bytes=need - 1)) == (EINVAL, why)
    assert _call(rec=_record(workspace=68)) == (EINVAL, why)
    assert _call(rec=_record(workspace_bytes=21 * 8 - 1, max_groups=1))[1] == why.replace(str(need), str(21 * 8))
    # K == 0 needs no grad_raw (row 0 of obs_traj exists all the same); B == 0 ends every valid call without a launch
    assert _call(B=0, K=0, rec=_record(grad_raw=None, workspace_bytes=0))[0] == 0
    assert _call(B=0)[0] == 0 and _call(B=0, dtype=1, sub=3)[0] == 0 and _call(B=0, K=2 ** 30 - 1, sub=2)[0] == 0
    assert _call(B=0, K=0, rec=_record(obs_traj=None))[0] == ENULL
    assert _call(B=0, rec=_record(widths=(16, 64, 64, 64, 2)))[0] == 0


def test_workspace_function_is_the_formula():
    lib = _native.lib()
    for widths in [(2, 5, 1), (8,) + hp.NETS["N2"] + (2,), (16, 64, 64, 64, 2), (3, 1)]:
        w = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*widths)
        # (params, noise and the clip bounds are not read: another record of the same shape, the same size)
        for pol in (_native.Policy(64, len(widths) - 1, 0, w, None, -1.0, 1.0), _native.Policy(None, len(widths) - 1, 1, w, 64, 0.0, 0.0)):
            for dtype in (0, 1):
                for B in (0, 1, 63, 64, 65, 326, 2 ** 15):
                    for K in (0, 1, 7, 1000):
                        for mg in (0, 1, 3, 1000):
                            got = lib.excenv_policy_param_grad_workspace_bytes(dtype, i64(B), i64(K), ctypes.byref(pol), mg)
                            assert got == hg.workspace_bytes(B, K, widths, mg), (widths, dtype, B, K, mg)
    pol = _native.Policy(64, 2, 0, (ctypes.c_int32 * 5)(2, 5, 1), None, 0.0, 0.0)
    bad = [(2, 4, 3, ctypes.byref(pol), 0), (0, -1, 3, ctypes.byref(pol), 0), (0, 4, -1, ctypes.byref(pol), 0), (0, 4, 3, None, 0),
           (0, 4, 3, ctypes.byref(pol), -1)]
    assert all(lib.excenv_policy_param_grad_workspace_bytes(a, i64(b), i64(c), d, e) == -1 for a, b, c, d, e in bad)
    assert hg.param_count((2, 5, 1)) == 21 and hg.param_count((16, 64, 64, 64, 2)) == 64 * 17 + 2 * 64 * 65 + 2 * 65


@pytest.mark.parametrize("max_groups", [0, 1, 3])
def test_tile_ranges_cover_every_tile_once(max_groups):
    for B in (1, 63, 64, 65, 326):
        for K in (0, 1, 7, 40):
            T, G = hg.tiles(B, K), hg.groups(B, K, max_groups)
            assert T == K * -(-B // 64) and G == min(T, max_groups or 512)
            ranges = hg.tile_ranges(B, K, max_groups)
            assert len(ranges) == G
            covered = [t for lo, hi in ranges for t in range(lo, hi)]
            assert covered == list(range(T)), (B, K, max_groups)
            assert all(hi > lo for lo, hi in ranges)  # no workgroup without a tile: each writes its whole slot of the workspace
            assert not ranges or max(hi - lo for lo, hi in ranges) - min(hi - lo for lo, hi in ranges) <= 1


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def _policy(widths=(2, 5, 1), activation="tanh", dtype=torch.float32, seed=3):
    g = torch.Generator().manual_seed(seed)
    W = [torch.randn(d, n, generator=g, dtype=dtype) for n, d in zip(widths[:-1], widths[1:])]
    b = [torch.randn(d, generator=g, dtype=dtype) for d in widths[1:]]
    return MLPPolicy(W, b, activation)


def test_python_refuses_by_name_and_the_setter():
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    policy = _policy()
    assert env.policy_param_grads == "torch"
    for bad in ("Fused", "", None, True, 1):
        with pytest.raises(ValueError, match="policy_param_grads needs to be 'torch' or 'fused'"):
            env.policy_param_grads = bad
    assert env.policy_param_grads == "torch"
    env.policy_param_grads = "fused"
    assert env.policy_param_grads == "fused" and EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu").policy_param_grads == "torch"
    env.policy_param_grads = "torch"
    acts = torch.zeros(4, 3, 1)
    for bad in ("sum", "Fused", None, 1, 0):
        with pytest.raises(ValueError, match=r"vmap_sim_ahead_policy_vjp: param_grads needs to be one of True, 'torch', False or 'fused', but .* is given"):
            env.vmap_sim_ahead_policy_vjp(policy, None, None, acts, env.tau, env.tau, param_grads=bad)
    for good in (True, "torch", False, "fused"):  # accepted: the next refusal speaks
        with pytest.raises(ValueError, match="vmap_sim_ahead_policy_vjp: `states` is None"):
            env.vmap_sim_ahead_policy_vjp(policy, None, None, acts, env.tau, env.tau, param_grads=good)
    obs, graw = torch.zeros(4, 4, 2), torch.zeros(4, 3, 1)
    for mg in (-1, 1.5, "1"):
        with pytest.raises(ValueError, match="vmap_policy_param_grads: max_groups needs to be a non-negative integer"):
            env.vmap_policy_param_grads(policy, obs, graw, env.tau, env.tau, max_groups=mg)
    with pytest.raises(ValueError, match=r"vmap_policy_param_grads: grad_raw needs to be of shape \(batch_size, n_actions, 1\)"):
        env.vmap_policy_param_grads(policy, obs, torch.zeros(4, 3, 2), env.tau, env.tau)
    with pytest.raises(ValueError, match=r"vmap_policy_param_grads: observations need to be of shape \(4, 4, 2\)"):
        env.vmap_policy_param_grads(policy, torch.zeros(4, 10, 2), graw, env.tau, env.tau)
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):  # there is no CPU fallback
        env.vmap_policy_param_grads(policy, obs, graw, env.tau, env.tau)
    empty = EnvironmentRegistry.PENDULUM.make(batch_size=0, device="cpu")
    got = empty.vmap_policy_param_grads(policy, torch.zeros(0, 4, 2), torch.zeros(0, 3, 1), env.tau, env.tau)
    assert got.shape == policy.params.shape and float(got.abs().max()) == 0.0


def test_relu_inputs_of_the_gpu_test_keep_their_margin():
    seen = 0
    for net, activation, OW, A, B, K in hg.ENTRY_CASES:
        if activation != "relu":
            continue
        case = hg.entry_case(net, activation, OW, A, B, K)
        low = float(hg.relu_min(case["W"], case["b"], case["rows"]).min())
        print(f"{net} OW={OW} A={A} B={B} K={K}: smallest |pre-activation| {low:.3e}")
        assert low >= hg.RELU_MARGIN_FP64
        seen += 1
    assert seen >= 6
    # the two restatements of the helper agree where they overlap: the magnitudes bound the gradient
    case = hg.entry_case("N1", "tanh", 8, 2, 65, 7)
    g = hg.restatement(case["W"], case["b"], "tanh", case["rows"], case["g"])
    assert np.all(np.abs(g) <= hg.term_magnitudes(case["W"], case["b"], "tanh", case["rows"], case["g"]) * (1 + 1e-12) + 1e-300)
