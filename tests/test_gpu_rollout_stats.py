"""The rollout statistics on the GPU (excenv_row_moments, excenv_episode_stats: row_moments_kernel, episode_stats_kernel,
rollout_stats_reduce_kernel; `vmap_row_moments`, `vmap_advantage_norm`, `vmap_episode_stats`). B in {1, 63, 64, 65, 326, 1028} (the
batch tail, one wave, one past it, a B that is no multiple of four, an aligned B, more tiles than workgroups), N or K in {1, 2, 9}, C in
{1, 2, 5}, fp32 and fp64, max_groups in {0, 1, 3}; pattern lanes with the first row masked, the last row masked, a run of resets and an
all-masked lane; an all-masked batch:
1. moments: n exact, every sum within N 2^-53 sum |term| of math.fsum over the twin's terms, mean and var within that bound propagated
   through the composition (helpers_rollout_stats.composed_bounds); a column whose mean is 100 deviations away, with and without shift;
2. `vmap_advantage_norm` against numpy's masked mean and std, and into `vmap_ppo_loss` with the bits of the same two numbers as floats;
3. episodes: completed, the carries, the count, min and max equal the twin exactly, SR and SRR within the summation bound, SL exactly;
   a call split at row 4 of 9 with the carries passed on;
4. the same call twice gives the same bits; copied inputs and views offset by one element give the bits of the aligned call;
5. NaNs in every excluded sample and every dropped reward change no bit; one NaN in a valid sample reaches what the contracts name;
6. case E2 of helpers_episodes: the returned step counter is the rollout's own; one PPO iteration with the kernel's advantage
   normalisation against float64 torch on the CPU.
Every case prints its figures."""
import functools
import math

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_episodes as he
import helpers_gae as hgae
import helpers_ppo as hpp
import helpers_rollout_stats as hrs
import test_gpu_policy_eval as pe
import test_gpu_ppo_loss as tpl
from exciting_environments_amd import _native
from helpers import make_env
from helpers_vjp import rel_dist

pytestmark = pytest.mark.gpu
TORCH = {"float32": torch.float32, "float64": torch.float64}
dtypes = pytest.mark.parametrize("dtype", hrs.DTYPES)


@functools.lru_cache(maxsize=None)
def _env(B, dtype):
    return make_env("pendulum", B, TORCH[dtype])[0]


def _lane(env, x, dtype=None, offset=0):
    """The values of x [B, N] or [B, N, C] as a view over lane-major memory that starts `offset` elements into its allocation"""
    x = torch.as_tensor(np.asarray(x), dtype=dtype or env.dtype, device=env.device)
    B = x.shape[0]
    tail = tuple(x.shape[1:])
    buf = torch.empty(offset + x.numel(), dtype=x.dtype, device=env.device)[offset:].view(tail + (B,))
    view = buf.permute(2, 0, 1) if x.ndim == 3 else buf.t()
    view.copy_(x)
    return view


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """Two results of the same method: every field the same bits (a NaN standing for any NaN)"""
    bits = lambda x, y: np.array_equal(x, y) and x.dtype == y.dtype if x.dtype.kind in "iub" else hpp.same_bits(x, y)
    return all((x is None and y is None) or bits(_np(x), _np(y)) for x, y in zip(a, b))


def _check_moments(m, twin, shift, ddof, label):
    """n exact, the sums within the summation bound, mean and var within the propagated bound -> largest error-to-bound ratio of the sums"""
    C = len(twin["t1"])
    assert float(m.n) == twin["n"], label
    worst = 0.0
    for c in range(C):
        for got, terms in ((float(m.sum[c]), twin["t1"][c]), (float(m.sumsq[c]), twin["t2"][c])):
            want, room = hrs.sum_bound(terms)
            err = abs(got - want)
            assert err <= room, f"{label}: column {c} sum {got!r}, fsum {want!r}, bound {room:.3e}"
            worst = max(worst, err / room if room > 0 else 0.0)
        mean, mean_room, var, var_room = hrs.composed_bounds(twin["n"], twin["t1"][c], twin["t2"][c], 0.0 if shift is None else float(shift[c]), ddof)
        assert abs(float(m.mean[c]) - mean) <= mean_room, f"{label}: column {c} mean {float(m.mean[c])!r}, reference {mean!r}, bound {mean_room:.3e}"
        assert abs(float(m.var[c]) - var) <= var_room, f"{label}: column {c} var {float(m.var[c])!r}, reference {var!r}, bound {var_room:.3e}"
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1, 4
@dtypes
def test_moments_within_the_derived_bounds_every_shape(dtype):
    top = 0.0
    for B in hrs.B_SIZES:
        env = _env(B, dtype)
        for N in hrs.N_SIZES:
            for C in hrs.C_SIZES:
                case = hrs.moments_case(B, N, C, dtype)
                x = _lane(env, case["x"]) if C > 1 else _lane(env, case["x"][:, :, 0])  # C == 1: the two-dimensional form
                mask = _lane(env, case["mask"], torch.bool)
                twins = {True: hrs.moments_twin(case["x"], case["mask"], case["shift"]), False: hrs.moments_twin(case["x"], case["mask"], None)}
                worst = 0.0
                for v, mg in enumerate(hrs.MAX_GROUPS):
                    shifted, ddof = v != 1, v % 2
                    shift = case["shift"] if shifted else None
                    m = env.vmap_row_moments(x, mask=mask, shift=shift, ddof=ddof, max_groups=mg)
                    assert _native.last_launch() == "row_moments_kernel"
                    assert all(t.dtype == torch.float64 and t.device == env.device and t.grad_fn is None for t in m)
                    assert m.n.ndim == 0 and all(tuple(t.shape) == (C,) for t in m[1:])
                    worst = max(worst, _check_moments(m, twins[shifted], shift, ddof, f"B={B} N={N} C={C} mg={mg}"))
                    assert _same(m, env.vmap_row_moments(x, mask=mask, shift=shift, ddof=ddof, max_groups=mg)), (B, N, C, mg)  # 4
                # no mask: every sample counts
                m = env.vmap_row_moments(x)
                _check_moments(m, hrs.moments_twin(case["x"]), None, 0, f"B={B} N={N} C={C} no mask")
                top = max(top, worst)
        print(f"moments {dtype} B={B}: n exact, sums, mean and var within their bounds; largest |sum - fsum| / bound so far {top:.3e}")
    print(f"moments {dtype}: largest error-to-bound ratio of the sums over all shapes {top:.3e}")


@dtypes
def test_a_column_a_hundred_deviations_from_zero(dtype):
    B, N = 326, 9
    env = _env(B, dtype)
    case = hrs.far_case(B, N, dtype)
    x, mask = _lane(env, case["x"]), _lane(env, case["mask"], torch.bool)
    first = [float(case["x"][0, 0, c]) for c in range(2)]  # (masked or not: any value near the mean serves)
    for shift in (first, None):
        twin = hrs.moments_twin(case["x"], case["mask"], shift)
        m = env.vmap_row_moments(x, mask=mask, shift=shift, ddof=1)
        _check_moments(m, twin, shift, 1, f"far column {dtype} shift={shift}")
        _, _, var, room = hrs.composed_bounds(twin["n"], twin["t1"][1], twin["t2"][1], 0.0 if shift is None else shift[1], 1)
        print(f"far column {dtype} shift={'first element' if shift else 'None'}: var {float(m.var[1]):.15e}, reference {var:.15e}, "
              f"distance {abs(float(m.var[1]) - var):.3e}, bound {room:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 2
@dtypes
def test_advantage_norm_against_numpy_and_into_the_ppo_loss(dtype):
    B, K, A = 326, 9, 1
    env = _env(B, dtype)
    case = hpp.ppo_case(B, K, A, dtype)
    adv, reset = _lane(env, case["advantage"]), _lane(env, case["reset"], torch.bool)
    eps = 1e-8
    shift, scale = env.vmap_advantage_norm(adv, reset)
    assert _native.last_launch() == "row_moments_kernel"
    assert all(t.ndim == 0 and t.dtype == torch.float64 and t.device == env.device for t in (shift, scale))
    m = env.vmap_row_moments(adv, mask=reset, ddof=1)
    assert torch.equal(shift, m.mean[0]) and torch.equal(scale, 1.0 / (torch.sqrt(m.var[0]) + eps))
    a = case["advantage"][~case["reset"]]
    twin = hrs.moments_twin(case["advantage"][:, :, None], case["reset"])
    _, mean_room, _, var_room = hrs.composed_bounds(twin["n"], twin["t1"][0], twin["t2"][0], 0.0, 1)
    assert abs(float(shift) - a.mean()) <= mean_room and abs(float(m.var[0]) - a.var(ddof=1)) <= var_room
    # scale = 1 / (std + eps): |sqrt(v) - sqrt(v*)| = |v - v*| / (sqrt(v) + sqrt(v*)) <= |v - v*| / sqrt(v*), and a few roundings of size std
    std = a.std(ddof=1)
    assert abs(1.0 / float(scale) - eps - std) <= var_room / std + 8 * hrs.U * std
    # into the objective: tensors or the same two numbers as floats
    dev = lambda v: torch.as_tensor(np.asarray(v), dtype=env.dtype, device=env.device)
    ls = torch.as_tensor(case["log_std"], dtype=torch.float64, device=env.device)
    with torch.no_grad():
        sample = _lane(env, case["sample"])
        logp_old = env.vmap_gaussian_logp(_lane(env, case["mean_old"]), sample, ls)
        run = lambda norm: env.vmap_ppo_loss(_lane(env, case["mean"]), sample, ls, logp_old, adv, value=dev(case["value"]),
                                             returns=dev(case["returns"]), reset=reset, adv_norm=norm)
        with_tensors, with_floats, without = run((shift, scale)), run((float(shift), float(scale))), run(None)
    assert all(torch.equal(p, q) for p, q in zip(with_tensors, with_floats))
    assert not torch.equal(with_tensors.policy_loss, without.policy_loss)
    # the all-masked batch
    every = torch.ones(B, K, dtype=torch.bool, device=env.device)
    m0 = env.vmap_row_moments(adv, mask=every, ddof=1)
    s0, c0 = env.vmap_advantage_norm(adv, every, eps=eps)
    assert float(m0.n) == 0 and float(m0.mean[0]) == 0 and float(m0.var[0]) == 0 and float(s0) == 0 and float(c0) == 1.0 / eps and math.isfinite(float(c0))
    print(f"advantage norm {dtype}: shift {float(shift):.6e} (numpy {a.mean():.6e}, bound {mean_room:.2e}), scale {float(scale):.6e} (numpy "
          f"{1.0 / (std + eps):.6e}); policy_loss {float(with_tensors.policy_loss):.6e} with tensors and with floats, {float(without.policy_loss):.6e} "
          "without; the all-masked batch gives n = 0, shift 0, scale 1 / eps")


# ---------------------------------------------------------------------------------------------------------------- 4, 5
@dtypes
def test_moments_layouts_and_nans(dtype):
    for B, N, C in ((1028, 2, 5), (64, 9, 2), (326, 9, 5)):
        env = _env(B, dtype)
        case = hrs.moments_case(B, N, C, dtype)
        x, mask, shift = _lane(env, case["x"]), _lane(env, case["mask"], torch.bool), case["shift"]
        assert x.data_ptr() % 16 == 0 and mask.data_ptr() % 4 == 0
        base = env.vmap_row_moments(x, mask=mask, shift=shift, max_groups=3)
        run = lambda xx, mm: env.vmap_row_moments(xx, mask=mm, shift=torch.as_tensor(shift), max_groups=3)
        row_major = torch.as_tensor(case["x"], dtype=env.dtype, device=env.device)
        assert row_major.is_contiguous() and _same(base, run(row_major, torch.as_tensor(case["mask"]))), "row-major (copied) inputs"
        off_x, off_m = _lane(env, case["x"], offset=1), _lane(env, case["mask"], torch.bool, offset=1)
        assert off_x.data_ptr() % 16 != 0 and off_m.data_ptr() % 4 == 1 and tuple(off_x.stride()) == tuple(x.stride())
        assert _same(base, run(off_x, mask)) and _same(base, run(x, off_m)) and _same(base, run(off_x, off_m)), "views offset by one element"
        assert _same(base, run(x.double(), mask)), "another dtype (copied)"
        # NaN in every excluded sample: no bit changes
        planted = case["x"].copy()
        planted[case["mask"]] = np.nan
        assert _same(base, run(_lane(env, planted), mask)) and _same(base, run(_lane(env, planted, offset=1), off_m)), "NaN behind the mask"
        # one NaN in a valid sample: the sums of its own column, nothing else
        b, n = (int(i[0]) for i in np.nonzero(~case["mask"] & (np.arange(B)[:, None] >= B // 2)))
        c = C - 1
        spot = case["x"].copy()
        spot[b, n, c] = np.nan
        got = run(_lane(env, spot), mask)
        others = [q for q in range(C) if q != c]
        assert torch.equal(got.n, base.n) and all(bool(torch.isnan(f[c])) for f in got[1:])
        assert all(hpp.same_bits(_np(f)[others], _np(g)[others]) for f, g in zip(got[1:], base[1:]))
        print(f"moments layouts {dtype} B={B} N={N} C={C}: copied and offset inputs give the aligned call's bits; NaN behind {int(case['mask'].sum())} "
              f"masked samples reaches nothing; a NaN at ({b}, {n}, {c}) reaches column {c} only")


# ---------------------------------------------------------------------------------------------------------------- 3, 4
def _raw_stats(env, case, carried=True):
    """The six numbers of excenv_episode_stats straight from the C entry -> float64 numpy [6]"""
    B, K = case["B"], case["K"]
    dev = env.device
    reward, reset = _lane(env, case["reward"]), _lane(env, case["reset"], torch.bool)
    ri = torch.as_tensor(case["return_in"], dtype=torch.float64, device=dev) if carried else None
    si = torch.as_tensor(case["steps_in"], dtype=torch.int32, device=dev) if carried else None
    stats = torch.empty(hrs.EPISODE_STATS, dtype=torch.float64, device=dev)
    nbytes = hrs.episode_workspace_bytes(B)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    hrs.raw_episodes(env.dtype, B, K, reward.data_ptr(), reset.data_ptr(), _native._ptr(ri), _native._ptr(si), None, None, None, stats.data_ptr(),
                     work.data_ptr(), nbytes)
    torch.cuda.synchronize()
    return _np(stats)


def _check_episodes(e, twin, label):
    """The exact fields of an EpisodeStats against the twin"""
    st = twin["stats"]
    if e.completed is not None:
        assert hpp.same_bits(_np(e.completed), twin["completed"]), label
    assert hpp.same_bits(_np(e.episode_return), twin["ret"]) and np.array_equal(_np(e.episode_steps), twin["steps"]), label
    assert e.episode_steps.dtype == torch.int32 and e.episode_return.dtype == torch.float64
    assert float(e.n_episodes) == st[0] and float(e.min_return) == st[4] and float(e.max_return) == st[5], label
    n1 = max(st[0], 1.0)
    assert float(e.mean_length) == math.fsum(twin["L"]) / n1, label  # SL is exact: integers below 2^53


@dtypes
def test_episode_stats_equal_the_twin_every_shape(dtype):
    top = 0.0
    for B in hrs.B_SIZES:
        env = _env(B, dtype)
        dev = env.device
        for K in hrs.N_SIZES:
            case = hrs.episode_case(B, K, dtype)
            reward, reset = _lane(env, case["reward"]), _lane(env, case["reset"], torch.bool)
            ri, si = torch.as_tensor(case["return_in"], device=dev), torch.as_tensor(case["steps_in"], device=dev)
            for carried in (True, False):
                twin = hrs.episode_twin(case["reward"], case["reset"], *((case["return_in"], case["steps_in"]) if carried else (None, None)))
                args = dict(episode_return=ri, episode_steps=si) if carried else {}
                e = env.vmap_episode_stats(reward, reset, per_row=carried, **args)
                assert _native.last_launch() == "episode_stats_kernel"
                assert (e.completed is not None) == carried and all(t.ndim == 0 and t.dtype == torch.float64 for t in e[:6])
                _check_episodes(e, twin, f"B={B} K={K} carried={carried}")
                assert _same(e, env.vmap_episode_stats(reward, reset, per_row=carried, **args)), (B, K, carried)  # 4
                raw = _raw_stats(env, case, carried)
                assert raw[0] == twin["stats"][0] and raw[3] == math.fsum(twin["L"]) and raw[4] == twin["stats"][4] and raw[5] == twin["stats"][5]
                for i, terms in ((1, twin["R"]), (2, twin["R"] * twin["R"])):
                    want, room = hrs.sum_bound(terms)
                    err = abs(raw[i] - want)
                    assert err <= room, f"B={B} K={K}: stats[{i}] = {raw[i]!r}, fsum {want!r}, bound {room:.3e}"
                    top = max(top, err / room if room > 0 else 0.0)
                n1 = max(raw[0], 1.0)
                assert float(e.mean_return) == raw[1] / n1 and float(e.mean_length) == raw[3] / n1
                assert float(e.std_return) == pytest.approx(math.sqrt(max((raw[2] - raw[1] * raw[1] / n1) / n1, 0.0)), rel=1e-15, abs=0.0)
            if K == 9:  # split at row 4: the carries continue the running episodes
                whole = env.vmap_episode_stats(reward, reset, episode_return=ri, episode_steps=si, per_row=True)
                head = env.vmap_episode_stats(reward[:, :4], reset[:, :4], episode_return=ri, episode_steps=si, per_row=True)
                tail = env.vmap_episode_stats(reward[:, 4:], reset[:, 4:], episode_return=head.episode_return, episode_steps=head.episode_steps,
                                              per_row=True)
                assert torch.equal(torch.cat((head.completed, tail.completed), dim=1), whole.completed)
                assert torch.equal(tail.episode_return, whole.episode_return) and torch.equal(tail.episode_steps, whole.episode_steps)
                assert float(head.n_episodes) + float(tail.n_episodes) == float(whole.n_episodes)
                assert min(float(head.min_return), float(tail.min_return)) == float(whole.min_return)
                assert max(float(head.max_return), float(tail.max_return)) == float(whole.max_return)
        print(f"episodes {dtype} B={B}: completed, carries, count, min and max equal the twin; SR, SRR within the bound (largest ratio so far "
              f"{top:.3e}); the split call continues the episodes")
    print(f"episodes {dtype}: largest error-to-bound ratio of SR and SRR over all shapes {top:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 4, 5
@dtypes
def test_episode_layouts_and_nans(dtype):
    for B, K in ((326, 9), (1028, 9), (64, 2)):
        env = _env(B, dtype)
        dev = env.device
        case = hrs.episode_case(B, K, dtype)
        reward, reset = _lane(env, case["reward"]), _lane(env, case["reset"], torch.bool)
        ri, si = torch.as_tensor(case["return_in"], device=dev), torch.as_tensor(case["steps_in"], device=dev)
        run = lambda rw, rs: env.vmap_episode_stats(rw, rs, episode_return=ri, episode_steps=si, per_row=True)
        base = run(reward, reset)
        row_major = torch.as_tensor(case["reward"], dtype=env.dtype, device=dev)
        assert _same(base, run(row_major, torch.as_tensor(case["reset"]))), "row-major (copied) inputs"
        assert _same(base, run(row_major.cpu().double(), case["reset"])), "host inputs of another dtype"
        off_r, off_f = _lane(env, case["reward"], offset=1), _lane(env, case["reset"], torch.bool, offset=1)
        assert off_r.data_ptr() % 16 != 0 and off_f.data_ptr() % 4 == 1
        assert _same(base, run(off_r, off_f)) and _same(base, run(off_r, reset)), "views offset by one element"
        assert _same(base, env.vmap_episode_stats(reward, reset, episode_return=ri.cpu(), episode_steps=si.long(), per_row=True)), "carries from elsewhere"
        # NaN in every dropped reward: no bit changes
        planted = case["reward"].copy()
        planted[case["reset"]] = np.nan
        assert _same(base, run(_lane(env, planted), reset)), "NaN in the dropped rewards"
        # one NaN in a counted reward of an episode that ends inside the rows
        clean = hrs.episode_twin(case["reward"], case["reset"], case["return_in"], case["steps_in"])
        ends = np.argwhere((clean["completed"] != 0) & (np.arange(K)[None, :] >= 1) & ~np.roll(case["reset"], 1, axis=1))
        if len(ends):
            b, end = (int(v) for v in ends[len(ends) // 2])
            spot = case["reward"].copy()
            spot[b, end - 1] = np.nan
            got = run(_lane(env, spot), reset)
            want = hrs.episode_twin(spot, case["reset"], case["return_in"], case["steps_in"])
            _check_episodes(got, want, f"NaN at ({b}, {end - 1})")
            assert bool(torch.isnan(got.completed[b, end])) and int(torch.isnan(got.completed).sum()) == 1
            assert bool(torch.isnan(got.mean_return)) and bool(torch.isnan(got.std_return))
            assert torch.equal(got.n_episodes, base.n_episodes) and torch.equal(got.mean_length, base.mean_length)
            assert torch.equal(got.episode_return, base.episode_return) and torch.equal(got.episode_steps, base.episode_steps)
            assert math.isfinite(float(got.min_return)) and math.isfinite(float(got.max_return))
        print(f"episode layouts {dtype} B={B} K={K}: copied and offset inputs give the aligned call's bits; NaN in {int(case['reset'].sum())} dropped "
              f"rewards reaches nothing; a NaN in a counted reward reaches its episode's return, SR and SRR only ({len(ends)} candidate episodes)")


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("dtype", pe.DTYPES, ids=["fp32", "fp64"])
def test_step_counter_equals_the_rollouts_own(dtype):
    env, _, inp, _, ro = pe._episodes(dtype)
    steps_in = torch.as_tensor(inp["steps_in"], dtype=torch.int32, device=env.device)
    e = env.vmap_episode_stats(ro.reward, ro.reset, episode_steps=steps_in, per_row=True)
    assert _native.last_launch() == "episode_stats_kernel"
    assert e.episode_steps.dtype == ro.episode_steps.dtype and torch.equal(e.episode_steps, ro.episode_steps)
    twin = hrs.episode_twin(_np(ro.reward).astype(np.float64), _np(ro.reset), None, inp["steps_in"])
    _check_episodes(e, twin, "E2")
    assert float(e.n_episodes) > 0 and 0.0 < float(ro.reset.double().mean()) < 1.0
    print(f"E2 {dtype}: episode_steps equals the rollout's counter on {he.B} environments; {int(e.n_episodes)} episodes, mean return "
          f"{float(e.mean_return):.6e}, mean length {float(e.mean_length):.3f}")


def test_one_ppo_iteration_with_the_kernels_advantage_normalisation_equals_float64_torch_on_the_cpu():
    """tests/test_gpu_ppo_loss.py's iteration with adv_norm=env.vmap_advantage_norm(adv, ro.reset), under that test's bounds with the
    normalised advantage in the place of the advantage"""
    dtype = torch.float64
    VF, ENT = tpl.VF, tpl.ENT
    env, actor, inp, noise, ro = pe._episodes(dtype)
    B, K, OW, A = he.B, he.K, env._obs_dim(), env.action_dim
    rng = np.random.default_rng(78)
    cw = (OW, 11, 1)
    critic = excenvs.MLPPolicy([rng.normal(0.0, 1.0 / np.sqrt(n), (d, n)) for n, d in zip(cw[:-1], cw[1:])],
                               [rng.uniform(-0.1, 0.1, d) for d in cw[1:]], "tanh", device=env.device, dtype=dtype)
    log_std = torch.full((A,), math.log(pe.SIGMA), dtype=dtype, device=env.device, requires_grad=True)
    with torch.no_grad():
        mean_old = env.vmap_policy_eval(actor, ro.observations, n_rows=K)
        sample = noise + mean_old
        logp_old = env.vmap_gaussian_logp(mean_old, sample, log_std)
    actor.params.requires_grad_()
    critic.params.requires_grad_()
    values = env.vmap_policy_eval(critic, ro.observations)[..., 0]
    adv, ret = env.vmap_gae(ro.reward, values, pe.GAMMA, pe.LAM, terminated=ro.terminated, reset=ro.reset)
    norm = env.vmap_advantage_norm(adv, ro.reset)
    assert _native.last_launch() == "row_moments_kernel" and all(t.grad_fn is None for t in norm)
    with torch.no_grad():
        actor.params.add_(torch.as_tensor(rng.normal(0.0, 0.02, actor.params.numel()), dtype=dtype, device=env.device).reshape(actor.params.shape))
    mean = env.vmap_policy_eval(actor, ro.observations, n_rows=K)
    out = env.vmap_ppo_loss(mean, sample, log_std, logp_old, adv, value=values[:, :K], returns=ret, reset=ro.reset, clip_eps=pe.CLIP_EPS,
                            vf_coef=VF, ent_coef=ENT, adv_norm=norm)
    out.loss.backward()
    torch.cuda.synchronize()
    # the same iteration on the CPU
    cpu = lambda t: t.detach().cpu()
    obs = cpu(ro.observations).contiguous()
    pa, pc = cpu(actor.params).clone().requires_grad_(), cpu(critic.params).clone().requires_grad_()
    ls_c = cpu(log_std).clone().requires_grad_()
    mean_c = actor.torch_forward(obs[:, :K], pa)
    values_c = critic.torch_forward(obs, pc)[..., 0]
    adv_c, ret_c = hgae.gae_direct(cpu(ro.reward).numpy(), values_c.detach().numpy(), pe.GAMMA, pe.LAM, cpu(ro.terminated).numpy(), cpu(ro.reset).numpy())
    valid = ~cpu(ro.reset)
    mask = valid.to(dtype)
    adv_t = torch.as_tensor(adv_c)
    a_c = (adv_t - adv_t[valid].mean()) / (adv_t[valid].std() + 1e-8)
    a_gpu = (cpu(adv) - cpu(norm[0])) * cpu(norm[1])
    loss_c, ratio = tpl._ppo_loss_cpu(mean_c, cpu(mean_old), cpu(sample), ls_c, values_c[:, :K], a_c, torch.as_tensor(ret_c), mask)
    loss_c.backward()
    da, dc = rel_dist(pe._np(actor.params.grad), pa.grad.numpy()), rel_dist(pe._np(critic.params.grad), pc.grad.numpy())
    n = float(mask.sum())
    rel = float(hpp.rel_bound("float64", A, float(-ls_c.detach().sum() - 0.5 * A * math.log(2 * math.pi)), cpu(logp_old).numpy(), cpu(logp_old).numpy()).max())
    z2 = (((cpu(sample) - mean_c.detach()) * torch.exp(-ls_c.detach())) ** 2)
    size = ((ratio.detach() * a_c.abs()).unsqueeze(-1) * (1.0 + z2) * mask.unsqueeze(-1)).sum() / n
    room = 4.0 * rel * (float(size) + float((0.5 * (values_c[:, :K].detach() - torch.as_tensor(ret_c)) ** 2 * mask).sum() / n) + 1.0)
    d_in = max(float((cpu(mean) - mean_c.detach()).abs().max()), float((cpu(values) - values_c.detach()).abs().max()),
               float(((a_gpu - a_c).abs() * mask).max()), float((cpu(ret) - torch.as_tensor(ret_c)).abs().max()))
    steep = float(((1.0 + (ratio.detach() * a_c.abs()).unsqueeze(-1) * (1.0 + z2)) * torch.exp(-ls_c.detach())).max())
    room += 4.0 * steep * (1.0 + float((values_c.detach()[:, :K] - torch.as_tensor(ret_c)).abs().max())) * d_in
    d_loss = abs(float(out.loss.detach()) - float(loss_c.detach()))
    d_ls = float((cpu(log_std.grad) - ls_c.grad).abs().max())
    print(f"PPO iteration fp64 with the kernel's advantage moments: shift {float(norm[0]):.6e} (CPU {float(adv_t[valid].mean()):.6e}), scale "
          f"{float(norm[1]):.6e} (CPU {1.0 / (float(adv_t[valid].std()) + 1e-8):.6e}); loss {float(out.loss.detach()):.6e} (CPU "
          f"{float(loss_c.detach()):.6e}, distance {d_loss:.3e}, bound {room:.3e}); actor grad {da:.3e}, critic grad {dc:.3e} (bound {pe.TOL:.0e}); "
          f"log_std.grad distance {d_ls:.3e}; n {int(out.n)}")
    assert float(pa.grad.abs().max()) > 0 and float(pc.grad.abs().max()) > 0 and float(out.n) == n and float(out.approx_kl) > 0
    assert da <= pe.TOL and dc <= pe.TOL
    assert d_loss <= room and d_ls <= room
