"""Host side of the network on stored rows (excenv_policy_eval, `vmap_policy_eval`; no GPU):
- the header and its `_native` mirror, the exports, ABI 7;
- excenv_policy_eval refuses by code and whole message, before any launch, what it does not do; B == 0 and R == 0 return OK;
- the sample tiles: the restated tile ranges cover every tile once, a function of (B, R) only;
- the kernel exists for both element types without scratch memory and without static LDS; the LDS formula;
- the Python method refuses by name what it does not do."""
import ctypes
import os
import re

import pytest
import torch

import helpers_policy as hp
import helpers_policy_param_grad as hg
from exciting_environments_amd import EnvironmentRegistry, MLPPolicy, _native
from helpers_budget import budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64 = ctypes.c_int64
EINVAL, ENULL = -1, -2
FN = "excenv_policy_eval"
MAX_GROUPS = 2048  # policy.hpp POLICY_EVAL_MAX_GROUPS, stated in include/excenv.h


def tiles(B, R):
    return R * -(-B // hg.TILE)


def tile_ranges(B, R):
    """[(first tile, one past the last tile)] per workgroup (include/excenv.h)"""
    T = tiles(B, R)
    G = min(T, MAX_GROUPS)
    return [(hg.first_tile(T, G, g), hg.first_tile(T, G, g + 1)) for g in range(G)]


def lds_rows(widths):
    """policy.hpp policy_eval_lds_rows: x^0 twice, x^1 / x^3 in one buffer, x^2 in the other"""
    hidden = list(widths[1:-1]) + [0, 0, 0]
    return 2 * widths[0] + max(hidden[0], hidden[2]) + hidden[1]


def test_header_declares_and_library_exports_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_policy_eval\s*\(", hdr)
    assert re.search(r"\}\s*excenv_policy_eval_t\s*;", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # an addition: a binder probes for the symbol
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, FN) and _native.lib().excenv_abi_version() == 7 and _native.ABI_VERSION == 7
    assert len(_native.PROTOTYPES[FN][1]) == 6
    assert _native.STRUCTS[_native.PolicyEval] == "excenv_policy_eval_t"
    assert [n for n, _ in _native.PolicyEval._fields_] == ["policy", "obs_traj", "out"]
    assert _native.PolicyEval.policy.size == ctypes.sizeof(_native.Policy) and _native.PolicyEval.policy.offset == 0


def test_kernel_exists_without_scratch_and_the_lds_formula():
    res, spans = budget("policy_eval")
    for t in "fd":
        hit = [k for k in res if f"policy_eval_kernelI{t}E" in k]
        assert len(hit) == 1, (t, hit)
        print(hit[0], res[hit[0]], spans[hit[0]])
    assert len(res) == 2, sorted(res)
    over = {k: v for k, v in res.items() if v["scratch"] != 0 or v["lds"] != 0 or v["vgpr"] > 256}
    assert not over, over
    widest = (16, 64, 64, 64, 2)
    assert lds_rows(widest) == 160 and 160 * 66 * 8 <= 160 * 1024
    assert lds_rows((3, 1)) == 6 and lds_rows((8, 11, 5, 2)) == 16 + 11 + 5 and lds_rows((8, 64, 64, 3, 2)) == 16 + 64 + 64


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _record(widths=(2, 5, 1), **kw):
    w = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*widths)
    pol = _native.Policy(64, len(widths) - 1, _native.ACT_TANH, w, None, -1.0, 1.0)
    for k in [k for k in kw if k.startswith("policy_")]:
        setattr(pol, k[len("policy_"):], kw.pop(k))
    r = _native.PolicyEval(pol, 64, 64)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(dtype=0, B=4, R=3, stride=1, rec=None, no_rec=False):
    lib = _native.lib()
    r = rec if rec is not None else _record()
    rc = lib.excenv_policy_eval(dtype, i64(B), i64(R), i64(stride), None if no_rec else ctypes.byref(r), None)
    return rc, lib.excenv_last_error().decode()


def test_refusals_come_back_by_code_and_whole_message_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    assert _call(no_rec=True) == (ENULL, f"{FN}: call is NULL")
    table = [
        (dict(policy_params=None), ENULL, "call->policy.params is NULL"),
        (dict(obs_traj=None), ENULL, "call->obs_traj is NULL"),
        (dict(out=None), ENULL, "call->out is NULL"),
        (dict(policy_n_layers=0), EINVAL, "policy.n_layers must be 1 .. 4 (got 0)"),
        (dict(policy_n_layers=5), EINVAL, "policy.n_layers must be 1 .. 4 (got 5)"),
        (dict(widths=(2, 65, 1)), EINVAL, "policy.widths[1] must be 1 .. 64 (got 65)"),
        (dict(widths=(2, 5, 0, 1)), EINVAL, "policy.widths[2] must be 1 .. 64 (got 0)"),
        (dict(widths=(17, 5, 1)), EINVAL, "policy.widths[0] must be 1 .. 16 (the widest observation row; got 17)"),
        (dict(widths=(0, 5, 1)), EINVAL, "policy.widths[0] must be 1 .. 16 (the widest observation row; got 0)"),
        (dict(widths=(2, 5, 3)), EINVAL, "policy.widths[2] must be 1 .. 2 (the action width; got 3)"),
        (dict(widths=(2, 0)), EINVAL, "policy.widths[1] must be 1 .. 2 (the action width; got 0)"),
        (dict(policy_activation=2), EINVAL, "policy.activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got 2)"),
    ]
    for kw, code, text in table:
        assert _call(rec=_record(**kw)) == (code, f"{FN}: {text}"), kw
    assert _call(dtype=2) == (EINVAL, f"{FN}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(B=-1) == (EINVAL, f"{FN}: bad B=-1, R=3 or row_stride=1")
    assert _call(R=-1) == (EINVAL, f"{FN}: bad B=4, R=-1 or row_stride=1")
    assert _call(stride=0) == (EINVAL, f"{FN}: bad B=4, R=3 or row_stride=0")
    assert _call(R=2 ** 30 + 1, stride=2) == (EINVAL, f"{FN}: (R - 1) * row_stride = 1073741824 * 2 rows exceed one launch")
    assert _call(R=2, stride=2 ** 31) == (EINVAL, f"{FN}: (R - 1) * row_stride = 1 * 2147483648 rows exceed one launch")
    # NULL pointers come first, whatever the values
    assert _call(dtype=2, rec=_record(out=None)) == (ENULL, f"{FN}: call->out is NULL")
    # B == 0 and R == 0 end every valid call without a launch, the largest strides included
    assert _call(B=0)[0] == 0 and _call(R=0)[0] == 0 and _call(B=0, R=0, dtype=1, stride=3)[0] == 0
    assert _call(B=0, R=2 ** 30, stride=2)[0] == 0 and _call(B=0, R=1, stride=2 ** 40)[0] == 0 and _call(B=0, R=2, stride=2 ** 31 - 1)[0] == 0
    assert _call(B=0, rec=_record(widths=(16, 64, 64, 64, 2)))[0] == 0
    assert _call(B=0, R=0, rec=_record(obs_traj=None))[0] == ENULL


def test_tile_ranges_cover_every_tile_once():
    for B in (1, 63, 64, 65, 326, 2 ** 15):
        for R in (0, 1, 8, 40, 1001):
            T = tiles(B, R)
            ranges = tile_ranges(B, R)
            assert len(ranges) == min(T, MAX_GROUPS)
            at = 0  # consecutive, non-empty ranges from 0 to T: every tile once
            for lo, hi in ranges:
                assert lo == at and hi > lo, (B, R, lo, hi)
                at = hi
            assert at == T
            assert not ranges or max(hi - lo for lo, hi in ranges) - min(hi - lo for lo, hi in ranges) <= 1


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def _policy(widths=(2, 5, 1), activation="tanh", dtype=torch.float32, seed=3):
    g = torch.Generator().manual_seed(seed)
    W = [torch.randn(d, n, generator=g, dtype=dtype) for n, d in zip(widths[:-1], widths[1:])]
    b = [torch.randn(d, generator=g, dtype=dtype) for d in widths[1:]]
    return MLPPolicy(W, b, activation)


def test_python_refuses_by_name():
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    policy = _policy()
    obs = torch.zeros(4, 7, 2)
    for bad in (0, -1, 1.5, "1", None):
        with pytest.raises(ValueError, match="vmap_policy_eval: row_stride needs to be a positive integer"):
            env.vmap_policy_eval(policy, obs, row_stride=bad)
    for shape in ((4, 7, 3), (3, 7, 2), (4, 0, 2), (4, 7), (4, 7, 2, 1)):
        with pytest.raises(ValueError, match=r"vmap_policy_eval: observations need to be of shape \(batch_size, n_rows, 2\)"):
            env.vmap_policy_eval(policy, torch.zeros(*shape))
    for stride, bad in ((1, 8), (3, 4), (1, -1), (1, 2.0)):
        with pytest.raises(ValueError, match=r"vmap_policy_eval: n_rows needs to be an integer from 0 to \d+ \(7 rows"):
            env.vmap_policy_eval(policy, obs, row_stride=stride, n_rows=bad)
    with pytest.raises(ValueError, match="vmap_policy_eval: observations require grad"):
        env.vmap_policy_eval(policy, obs.clone().requires_grad_())
    with torch.no_grad():  # values alone: the next refusal speaks
        with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
            env.vmap_policy_eval(policy, obs.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):  # there is no CPU fallback
        env.vmap_policy_eval(policy, obs)
    with pytest.raises(AssertionError, match="policy needs to be an MLPPolicy"):
        env.vmap_policy_eval(torch.nn.Linear(2, 1), obs)
    wide = _policy((2, 5, 3))
    with pytest.raises(ValueError, match="vmap_policy_eval: the policy needs at most 16 inputs and 2 outputs"):
        env.vmap_policy_eval(wide, obs)
    # no rows and no environments need no launch
    assert tuple(env.vmap_policy_eval(policy, obs, n_rows=0).shape) == (4, 0, 1)
    empty = EnvironmentRegistry.PENDULUM.make(batch_size=0, device="cpu")
    assert tuple(empty.vmap_policy_eval(policy, torch.zeros(0, 7, 2), row_stride=3).shape) == (0, 3, 1)
    assert hp.NETS["N2"] == (64, 64, 3)
