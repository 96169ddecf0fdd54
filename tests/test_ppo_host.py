"""Host side of the PPO objective (excenv_gaussian_logp, excenv_ppo_loss, excenv_ppo_loss_grad; `vmap_gaussian_logp`, `vmap_ppo_loss`;
no GPU):
- the header with the contract block and its `_native` mirrors, the exports, ABI 7;
- every refusal by code and whole message, before any launch; B == 0 and K == 0 return OK;
- the kernels exist for both element types and both action widths without scratch memory;
- the Python methods check shapes and arguments by name;
- the numpy twin of the contract block (helpers_ppo.ppo_twin) agrees with its long-double form within the bounds of the GPU test, and
  the input conditions of the GPU test hold for every shape it uses;
- the workspace and partition functions against a Python restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_ppo as hpp
from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64 = ctypes.c_int64
EINVAL, ENULL = -1, -2
LOGP, LOSS, GRAD = "excenv_gaussian_logp", "excenv_ppo_loss", "excenv_ppo_loss_grad"


def test_header_declares_the_contract_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)
    for fn in (LOGP, LOSS, GRAD, LOSS + "_workspace_bytes"):
        assert re.search(rf"\b{fn}\s*\(", hdr), fn
    assert re.search(r"\}\s*excenv_gaussian_logp_t\s*;", hdr) and re.search(r"\}\s*excenv_ppo_loss_t\s*;", hdr)
    for line in ("z[q]  = (sample[q] - mean[q]) * inv_std[q]", "logp  = logp_const;  for q = 0 .. A-1:  logp = fma(-0.5 * z[q], z[q], logp)",
                 "d     = logp - logp_old;   r = exp(d)", "a     = adv_norm ? (advantage - adv_norm[0]) * adv_norm[1] : advantage",
                 "s1    = r * a;   s2 = min(max(r, lo), hi) * a;   surr = min(s1, s2);   active = !(s2 < s1)", "valid = !reset[n]",
                 "gl            = active ? -(r * a) * w : 0", "grad_mean[q]  = valid ? gl * z[q] * inv_std[q] : 0",
                 "grad_value    = valid ? wv * (value - returns) : 0", "stats[3] = S_kl = sum ((r - 1) - d)",
                 "stats[5 + q] = S_gls[q] = sum (active ? -(r * a) : 0) * (z[q] * z[q] - 1)",
                 "first(g) = g * (Tn / G) + min(g, Tn mod G)", "inv_std[q] = exp(-log_std[q]),  logp_const = -sum_q log_std[q] - A/2 * log(2 pi)"):
        assert line in hdr, line
    lib = ctypes.CDLL(_native.library_path())
    for fn in (LOGP, LOSS, GRAD, LOSS + "_workspace_bytes"):
        assert hasattr(lib, fn) and fn in _native.PROTOTYPES, fn
    assert _native.lib().excenv_abi_version() == 7
    assert all(len(_native.PROTOTYPES[fn][1]) == 5 for fn in (LOGP, LOSS, GRAD)) and len(_native.PROTOTYPES[LOSS + "_workspace_bytes"][1]) == 3
    assert _native.STRUCTS[_native.GaussianLogp] == "excenv_gaussian_logp_t" and _native.STRUCTS[_native.PpoLoss] == "excenv_ppo_loss_t"
    assert [n for n, _ in _native.GaussianLogp._fields_] == ["mean", "sample", "inv_std", "logp_const", "n_actions", "logp"]
    assert [n for n, _ in _native.PpoLoss._fields_] == ["mean", "sample", "inv_std", "logp_const", "logp_old", "advantage", "value", "returns",
                                                       "reset", "adv_norm", "n_actions", "max_groups", "clip_eps", "stats", "workspace",
                                                       "workspace_bytes", "grad_scale", "grad_mean", "grad_value"]
    assert (_native.PPO_STATS, _native.PPO_TILE, _native.PPO_AUTO_GROUPS) == (hpp.N_STATS, hpp.TILE, hpp.AUTO_GROUPS) == (5, 1024, 2048)
    assert excenvs.PpoLoss._fields == ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "n")
    assert "PpoLoss" in excenvs.__all__
    for method in ("vmap_gaussian_logp", "vmap_ppo_loss"):
        assert callable(getattr(excenvs.CoreEnvironment, method))


@pytest.mark.parametrize("name", ["gaussian_logp_kernel", "ppo_loss_kernel", "ppo_loss_grad_kernel"])
def test_kernels_exist_for_both_types_and_widths_without_scratch(name):
    res, spans = budget(name)
    for t in "fd":
        for A in (1, 2):
            hit = [k for k in res if f"{name}I{t}Li{A}EE" in k]
            assert len(hit) == 1, (t, A, hit)
            print(hit[0], res[hit[0]], spans.get(hit[0]))
    assert len(res) == 4, sorted(res)
    over = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr"] > 256}
    assert not over, over
    # the streams hold no LDS; the forward holds the four wave sums of its tree
    assert all(v["lds"] == (32 if name == "ppo_loss_kernel" else 0) for v in res.values()), res
    red, _ = budget("ppo_loss_reduce_kernel")
    assert len(red) == 1 and all(v["scratch"] == 0 for v in red.values())


def _logp_record(**kw):
    r = _native.GaussianLogp(64, 64, 64, 64, 2, 64)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _loss_record(**kw):
    r = _native.PpoLoss(64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 2, 0, 0.2, 64, 64, 1 << 20, 64, 64, 64)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(fn, rec, dtype=0, B=4, K=3, no_rec=False):
    lib = _native.lib()
    rc = getattr(lib, fn)(dtype, i64(B), i64(K), None if no_rec else ctypes.byref(rec), None)
    return rc, lib.excenv_last_error().decode()


def test_gaussian_logp_refusals_by_code_and_whole_message():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    fn = LOGP
    assert _call(fn, None, no_rec=True) == (ENULL, f"{fn}: call is NULL")
    for field in ("mean", "sample", "inv_std", "logp_const", "logp"):
        assert _call(fn, _logp_record(**{field: None})) == (ENULL, f"{fn}: call->{field} is NULL")
    for A in (0, 3, -1):
        assert _call(fn, _logp_record(n_actions=A)) == (EINVAL, f"{fn}: call->n_actions must be 1 .. 2 (got {A})")
    assert _call(fn, _logp_record(), dtype=2) == (EINVAL, f"{fn}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(fn, _logp_record(), B=-1) == (EINVAL, f"{fn}: bad B=-1 or K=3")
    assert _call(fn, _logp_record(), K=-2) == (EINVAL, f"{fn}: bad B=4 or K=-2")
    assert _call(fn, _logp_record(), K=1 << 30) == (EINVAL, f"{fn}: K * n_actions = {1 << 30} * 2 rows exceed one launch")
    assert _call(fn, _logp_record(mean=None), dtype=2) == (ENULL, f"{fn}: call->mean is NULL")  # NULL pointers come first
    for rec in (_logp_record(), _logp_record(n_actions=1)):
        assert _call(fn, rec, B=0)[0] == 0 and _call(fn, rec, K=0)[0] == 0 and _call(fn, rec, B=0, K=0, dtype=1)[0] == 0
    assert _call(fn, _logp_record(logp=None), B=0)[0] == ENULL


@pytest.mark.parametrize("fn", [LOSS, GRAD])
def test_loss_refusals_by_code_and_whole_message(fn):
    grad = fn == GRAD
    assert _call(fn, None, no_rec=True) == (ENULL, f"{fn}: call is NULL")
    own = ("grad_scale",) if grad else ("stats", "workspace")
    for field in ("mean", "sample", "inv_std", "logp_const", "logp_old", "advantage") + own:
        assert _call(fn, _loss_record(**{field: None})) == (ENULL, f"{fn}: call->{field} is NULL")
    if grad:
        assert _call(fn, _loss_record(grad_mean=None, grad_value=None)) == (ENULL, f"{fn}: call->grad_mean and call->grad_value is NULL")
        assert _call(fn, _loss_record(grad_mean=None), B=0)[0] == 0 and _call(fn, _loss_record(grad_value=None), B=0)[0] == 0
        assert _call(fn, _loss_record(value=None, returns=None)) == (EINVAL, f"{fn}: call->grad_value needs call->value and call->returns")
        # what the forward alone reads is not looked at
        assert _call(fn, _loss_record(stats=None, workspace=None, workspace_bytes=0, max_groups=-1), B=0)[0] == 0
    else:
        assert _call(fn, _loss_record(grad_scale=None, grad_mean=None, grad_value=None), B=0)[0] == 0
    for miss in ("value", "returns"):
        assert _call(fn, _loss_record(**{miss: None})) == (EINVAL, f"{fn}: call->value and call->returns must be given both or neither")
    for A in (0, 3):
        assert _call(fn, _loss_record(n_actions=A)) == (EINVAL, f"{fn}: call->n_actions must be 1 .. 2 (got {A})")
    assert _call(fn, _loss_record(), dtype=2) == (EINVAL, f"{fn}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(fn, _loss_record(), dtype=-1)[0] == EINVAL
    assert _call(fn, _loss_record(), B=-1) == (EINVAL, f"{fn}: bad B=-1 or K=3")
    assert _call(fn, _loss_record(), K=-2) == (EINVAL, f"{fn}: bad B=4 or K=-2")
    for eps, shown in ((0.0, "0"), (1.0, "1"), (-0.2, "-0.2"), (1.5, "1.5")):
        assert _call(fn, _loss_record(clip_eps=eps)) == (EINVAL, f"{fn}: call->clip_eps must lie in (0, 1) (got {shown})")
    rc, msg = _call(fn, _loss_record(clip_eps=float("nan")))
    assert rc == EINVAL and msg.startswith(f"{fn}: call->clip_eps must lie in (0, 1) (got ") and "nan" in msg.lower()
    if not grad:
        assert _call(fn, _loss_record(max_groups=-1)) == (EINVAL, f"{fn}: call->max_groups must not be negative (got -1; 0: auto)")
        for B, K, mg in ((4, 3, 0), (1028, 9, 0), (1028, 9, 3), (1 << 15, 1000, 0)):
            need = hpp.workspace_bytes(B, K, mg)
            msg = f"{fn}: needs an 8-byte aligned workspace of {need} bytes (excenv_ppo_loss_workspace_bytes)"
            assert _call(fn, _loss_record(max_groups=mg, workspace_bytes=need - 1), B=B, K=K) == (EINVAL, msg)
            assert _call(fn, _loss_record(max_groups=mg, workspace_bytes=need, workspace=68), B=B, K=K) == (EINVAL, msg)
    assert _call(fn, _loss_record(), K=1 << 30) == (EINVAL, f"{fn}: K * n_actions = {1 << 30} * 2 rows exceed one launch")
    assert _call(fn, _loss_record(n_actions=1), K=0x7fffffff, B=0)[0] == 0
    # NULL pointers come first; the optional ones are optional
    assert _call(fn, _loss_record(mean=None, clip_eps=2.0), dtype=2) == (ENULL, f"{fn}: call->mean is NULL")
    for rec in (_loss_record(), _loss_record(reset=None, adv_norm=None), _loss_record(value=None, returns=None, grad_value=None), _loss_record(n_actions=1)):
        assert _call(fn, rec, B=0)[0] == 0 and _call(fn, rec, K=0)[0] == 0 and _call(fn, rec, B=0, K=0, dtype=1)[0] == 0
    assert _call(fn, _loss_record(advantage=None), B=0)[0] == ENULL


def test_workspace_and_partition_against_the_restatement():
    lib = _native.lib()
    for B in hpp.B_SIZES + (0, 1024, 1025, 1 << 15, (1 << 22) + 1):
        for K in hpp.K_SIZES + (0, 1000):
            for mg in hpp.MAX_GROUPS + (2048, 5000):
                assert lib.excenv_ppo_loss_workspace_bytes(B, K, mg) == hpp.workspace_bytes(B, K, mg), (B, K, mg)
    assert lib.excenv_ppo_loss_workspace_bytes(-1, 1, 0) == lib.excenv_ppo_loss_workspace_bytes(1, -1, 0) == lib.excenv_ppo_loss_workspace_bytes(1, 1, -1) == -1
    assert hpp.groups_of(1028, 9, 0) == (18, 18) and hpp.groups_of(1028, 9, 3) == (18, 3) and hpp.groups_of(1 << 15, 1000, 0) == (32000, 2048)
    for tiles, groups in ((18, 3), (18, 18), (32000, 2048), (7, 3)):  # contiguous runs that cover every tile once, sizes differ by at most one
        first = [hpp.first_tile(tiles, groups, g) for g in range(groups + 1)]
        sizes = np.diff(first)
        assert first[0] == 0 and first[-1] == tiles and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1 and np.all(np.diff(sizes) <= 0)


def test_python_checks_shapes_and_arguments_by_name():
    env = EnvironmentRegistry.PMSM.make(batch_size=4, device="cpu")
    B, K, A = 4, 3, 2
    mean, sample, ls = torch.zeros(B, K, A), torch.zeros(B, K, A), torch.zeros(A)
    lp, adv = torch.zeros(B, K), torch.zeros(B, K)
    for fn, call in (("vmap_gaussian_logp", lambda m, s, l: env.vmap_gaussian_logp(m, s, l)),
                     ("vmap_ppo_loss", lambda m, s, l: env.vmap_ppo_loss(m, s, l, lp, adv))):
        for shape in ((3, K, A), (B, K), (B, K, 3), (B, K, 0)):
            with pytest.raises(ValueError, match=rf"{fn}: mean needs to be of shape \(batch_size, n_steps, action_dim\) with action_dim from 1 to 2"):
                call(torch.zeros(*shape), sample, ls)
        with pytest.raises(ValueError, match=rf"{fn}: sample needs to be of the shape of mean which is \(4, 3, 2\)"):
            call(mean, torch.zeros(B, K + 1, A), ls)
        for bad in (torch.zeros(1), torch.zeros(3), torch.zeros(2, 1), torch.tensor(0.0)):
            with pytest.raises(ValueError, match=rf"{fn}: log_std needs to be of shape \(action_dim,\) which is \(2,\)"):
                call(mean, sample, bad)
        with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):  # there is no CPU fallback
            call(mean, sample, ls)
    with pytest.raises(ValueError, match="vmap_gaussian_logp: mean requires grad.*vmap_ppo_loss"):
        env.vmap_gaussian_logp(mean.clone().requires_grad_(), sample, ls)
    with torch.no_grad():  # under no_grad the values are read
        with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
            env.vmap_gaussian_logp(mean.clone().requires_grad_(), sample, ls)
    f = "vmap_ppo_loss"
    for name in ("logp_old", "advantage", "value", "returns", "reset"):
        kw = dict(logp_old=lp, advantage=adv, value=lp, returns=lp, reset=torch.zeros(B, K, dtype=torch.bool))
        kw[name] = torch.zeros(B, K + 1, dtype=kw[name].dtype)
        with pytest.raises(ValueError, match=rf"{f}: {name} needs to be of shape \(batch_size, n_steps\) which is \(4, 3\)"):
            env.vmap_ppo_loss(mean, sample, ls, **kw)
    for kw in (dict(value=lp), dict(returns=lp)):
        with pytest.raises(ValueError, match=f"{f}: value and returns need to be given both or neither"):
            env.vmap_ppo_loss(mean, sample, ls, lp, adv, **kw)
    for bad in (0.0, 1.0, -0.1, float("nan"), None, "0.2", True):
        with pytest.raises(ValueError, match=rf"{f}: clip_eps needs to be a number in \(0, 1\)"):
            env.vmap_ppo_loss(mean, sample, ls, lp, adv, clip_eps=bad)
    for name in ("vf_coef", "ent_coef"):
        for bad in (float("nan"), float("inf"), None, "1", False):
            with pytest.raises(ValueError, match=f"{f}: {name} needs to be a finite number"):
                env.vmap_ppo_loss(mean, sample, ls, lp, adv, **{name: bad})
    for bad in (-1, 1.0, None, True):
        with pytest.raises(ValueError, match=f"{f}: max_groups needs to be a non-negative integer"):
            env.vmap_ppo_loss(mean, sample, ls, lp, adv, max_groups=bad)
    for bad in (1.0, (1.0,), (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match=rf"{f}: adv_norm needs to be None or a \(shift, scale\) pair"):
            env.vmap_ppo_loss(mean, sample, ls, lp, adv, adv_norm=bad)
    # no step or no environment: no launch, every mean 0, the entropy term alone, and log_std still gets its gradient
    ent = float(ls.sum()) + 0.5 * A * (1.0 + np.log(2.0 * np.pi))
    for e, m in ((env, torch.zeros(B, 0, A)), (EnvironmentRegistry.PMSM.make(batch_size=0, device="cpu"), torch.zeros(0, K, A))):
        flat = torch.zeros(m.shape[:2])
        assert tuple(e.vmap_gaussian_logp(m, m, ls).shape) == tuple(flat.shape)
        out = e.vmap_ppo_loss(m, m, ls, flat, flat, value=flat, returns=flat, ent_coef=0.25)
        assert isinstance(out, excenvs.PpoLoss) and all(t.ndim == 0 and t.dtype == torch.float64 and t.grad_fn is None for t in out)
        assert float(out.n) == 0 and float(out.policy_loss) == 0 and float(out.value_loss) == 0 and float(out.approx_kl) == 0
        assert float(out.entropy) == pytest.approx(ent, abs=1e-15) and float(out.loss) == -0.25 * float(out.entropy)
        l2 = ls.clone().requires_grad_()
        out = e.vmap_ppo_loss(m, m, l2, flat, flat, ent_coef=0.25)
        assert out.loss.grad_fn is not None and all(t.grad_fn is None for t in out[1:])
        out.loss.backward()
        assert torch.equal(l2.grad, torch.full((A,), -0.25))


@pytest.mark.parametrize("dtype", hpp.DTYPES)
@pytest.mark.parametrize("A", hpp.A_SIZES)
def test_twin_agrees_with_the_reference_and_the_input_conditions_hold(A, dtype):
    """For every shape of the GPU test: the twin in T (numpy's exp standing for the device's) against the long-double reference,
    within the bounds the GPU test uses; the shares of clipped and inactive samples where the case is large enough for a share to
    mean something (helpers_ppo.MIN_SAMPLES); the share of flipped decisions everywhere."""
    worst = 0.0
    for B in hpp.B_SIZES:
        for K in hpp.K_SIZES:
            case = hpp.ppo_case(B, K, A, dtype)
            inv_std, c = hpp.consts(case["log_std"], dtype)
            twin, ref = hpp.changed(case, grad_scale=(0.37, 0.11), adv_norm=(0.05, 1.3))
            clipped, inactive, flips, n = hpp.input_conditions(twin, ref)
            print(f"B={B} K={K} A={A} {dtype}: valid {n}, clipped {clipped:.3f}, inactive {inactive:.3f}, flips {flips:.4f}, "
                  f"reset share {float(case['reset'].mean()):.3f}")
            assert flips <= 0.01
            if n >= hpp.MIN_SAMPLES:
                assert 0.05 <= clipped <= 0.6 and inactive >= 0.02
                assert 0.1 <= float(case["reset"][case["n_fixed"]:].mean()) <= 0.3
            if case["n_fixed"]:
                assert np.array_equal(case["reset"][:hpp.N_PATTERN], hpp.pattern_reset(K)) and not twin["valid"][3].any()
            assert np.all(twin["grad_mean"][~twin["valid"]] == 0) and np.all(twin["grad_value"][~twin["valid"]] == 0)
            same = twin["valid"] & (twin["active"] == ref["active"])
            rel = hpp.rel_bound(dtype, A, c, ref["logp"], ref["logp_old"])
            for q in range(A):
                err = np.abs(twin["grad_mean"][..., q].astype(np.float64) - np.asarray(ref["grad_mean"][..., q], np.float64))
                lim = rel * np.abs(np.asarray(ref["grad_mean"][..., q], np.float64))
                if same.any() and lim[same].max() > 0:
                    worst = max(worst, float(np.max(err[same] / np.maximum(lim[same], 1e-300))))
                assert np.all(err[same] <= lim[same])
            bounds = hpp.term_bounds(ref, rel, dtype, A)
            agree = twin["valid"] & (twin["active"] == ref["active"]) & (twin["clipped"] == ref["clipped"])
            for name, tt, tr, bd in zip(("n", "surr", "vsq", "kl", "clip") + ("gls",) * A, hpp.stat_terms(twin["terms"], A), hpp.stat_terms(ref["terms"], A), bounds):
                assert np.all(np.abs(tt - tr)[agree] <= bd[agree]), (name, B, K)
    print(f"A={A} {dtype}: largest |grad_mean - reference| / bound of the twin {worst:.3f}")
    assert worst <= 1.0
