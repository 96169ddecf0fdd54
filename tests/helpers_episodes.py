"""Inputs and references of the episode-rollout tests (tests/test_episodes_host.py, tests/test_gpu_episodes.py,
tests/test_gpu_guard_episodes.py): the two input cases E1 / E2 of `vmap_rollout_episodes` (include/excenv.h excenv_episode_t), a numpy
restatement of its reset rule, and the float64 oracle episode loop (oracle.gym_step, the numpy policy of helpers_policy, np.where)."""
import functools

import numpy as np

import oracle
import helpers_policy as hp
from helpers import ANGLE_STATES, random_state
from helpers_vjp import CASES, SOLVERS, case_spec  # noqa: F401  (what the tests parametrise over)

B, K = 326, 9
NET = "N1"
R = 2
RESET_SEEDS = (500, 501)
STEPS_SEED = 4242
CONTROL = {"pendulum": ["theta"], "mass_spring_damper": ["deflection"], "cartpole": ["theta", "deflection"],
           "acrobot": ["theta_1", "theta_2"], "fluid_tank": ["height"], "pmsm": ["i_d", "i_q"]}
# scale: the factor of every non-angle state field in normalised coordinates. episode_steps_in ~ integers[0, max_episode_steps) in both
# cases: the counter of a running episode is below its budget (E1: 0 .. 11, E2: 0 or 1). A counter at or past the budget would end
# the episode on row 0 whatever the state, and under E2 a PMSM without dead time that leaves its current circle one step after such
# a reset then takes a fourth reset within the 9 rows (16 - 25 of 326 environments with counters from 0 .. 11).
EPISODE_CASES = {"E1": dict(scale=1.4, max_episode_steps=12), "E2": dict(scale=1.0, max_episode_steps=2)}
END_BOTH = ("terminated", "truncated")


def scaled(env_name, spec, st, factor):
    """The states with every non-angle field multiplied by `factor` in normalised coordinates"""
    out = []
    for j, name in enumerate(oracle.STATE_FIELDS[env_name]):
        v = np.asarray(st[j], np.float64)
        if factor != 1.0 and j not in ANGLE_STATES.get(env_name, []):
            lo, hi = (np.asarray(x, np.float64) for x in spec["phys_norm"][name])
            v = (factor * (2.0 * (v - lo) / (hi - lo) - 1.0) + 1.0) / 2.0 * (hi - lo) + lo
        out.append(v)
    return out


def episode_inputs(env_name, spec, case, hidden=None, B=B, K=K, n_rows=R, control="default"):
    """float64 inputs of one case: helpers_policy.policy_inputs' (states, network, noise, references) with the initial states scaled,
    + reset ([n_rows] lists of S arrays [B], from helpers.random_state seeds 500, 501, ..), steps_in [B] int32, max_episode_steps"""
    cfg = EPISODE_CASES[case]
    control = CONTROL[env_name] if control == "default" else control
    inp = dict(hp.policy_inputs(env_name, spec, hp.NETS[NET] if hidden is None else hidden, B, K, control=control))
    inp["st"] = scaled(env_name, spec, inp["st"], cfg["scale"])
    inp["reset"] = [scaled(env_name, spec, random_state(env_name, B, np.float64, spec, RESET_SEEDS[0] + r), cfg["scale"]) for r in range(n_rows)]
    inp["steps_in"] = np.random.default_rng(STEPS_SEED).integers(0, cfg["max_episode_steps"], B).astype(np.int32)
    inp["max_episode_steps"] = cfg["max_episode_steps"]
    inp["control"] = control
    return inp


def reset_rule_np(term_rows, trunc_rows, steps_in, max_episode_steps, end_on):
    """The reset rule of the contract from the per-row verdicts: term_rows / trunc_rows [B, K] bool, the flags of rows 0 .. K-1
    (trunc_rows: any flag of the row) -> (reset [B, K] bool, n_resets [B], episode_steps_out [B], time_only [B, K]: resets no flag
    asked for)"""
    term_rows, trunc_rows = np.asarray(term_rows, bool), np.asarray(trunc_rows, bool)
    Bn, Kn = term_rows.shape
    t = np.asarray(steps_in, np.int64).copy()
    reset = np.zeros((Bn, Kn), bool)
    time_only = np.zeros((Bn, Kn), bool)
    for n in range(Kn):
        flag = np.zeros(Bn, bool)
        if "terminated" in end_on:
            flag |= term_rows[:, n]
        if "truncated" in end_on:
            flag |= trunc_rows[:, n]
        timed = (t >= max_episode_steps) if max_episode_steps > 0 else np.zeros(Bn, bool)
        reset[:, n] = flag | timed
        time_only[:, n] = timed & ~flag
        t = np.where(reset[:, n], 0, t + 1)
    return reset, reset.sum(axis=1).astype(np.int32), t.astype(np.int32), time_only


def _ctl(inp):
    return [(n, inp["refs"][n]) for n in inp["control"]] if inp["control"] else None


def row_outputs(env_name, st, props, ctl):
    """(reward [B], terminated [B], truncated [B, TW]) of the states `st`: generate_reward / _terminated / _truncated of one row"""
    two = [np.stack([np.asarray(v, np.float64)] * 2, axis=1) for v in st]
    rew, trunc, term = oracle.rew_trunc_term_ahead(env_name, two, props, control=ctl)
    return rew[:, 0, 0], term[:, 0, 0].astype(bool), trunc[:, 0].astype(bool)


def oracle_episode_loop(env_name, solver, props, inp, tau, activation, end_on=END_BOTH, K=K, noise=True, clip=hp.CLIP):
    """The contract of vmap_rollout_episodes in float64 on the oracle alone: oracle.gym_step for the step and the gym outputs of the
    stepped state, the numpy policy, np.where for the reset -> dict(obs [B, K+1, OW], states (S x [B, K+1]), last, actions [B, K, A],
    reward [B, K], terminated [B, K], truncated [B, K+1, TW], reset [B, K], flag_reset / time_only [B, K], n_resets, steps_out,
    term0: terminated of row 0)"""
    st = [np.asarray(v, np.float64) for v in inp["st"]]
    Bn = st[0].shape[0]
    A = hp.action_dim(env_name)
    ctl = _ctl(inp)
    observe = lambda s: oracle.sim_ahead(env_name, solver, s, np.zeros((Bn, 0, A)), props, tau, control=ctl)[0][:, 0]
    rew, term, trunc = row_outputs(env_name, st, props, ctl)
    term0 = term
    ob = observe(st)
    t = inp["steps_in"].astype(np.int64).copy()
    e = np.zeros(Bn, np.int64)
    n_rows = len(inp["reset"])
    rows_o, rows_s, acts, rews, terms, truncs, resets, flagged, timed_only = [ob], [st], [], [], [], [trunc], [], [], []
    for n in range(K):
        a, _, _ = hp.mlp_np(ob, inp["W"], inp["b"], activation, inp["noise"][:, n] if noise else None, clip)
        flag = np.zeros(Bn, bool)
        if "terminated" in end_on:
            flag |= term
        if "truncated" in end_on:
            flag |= trunc.any(axis=1)
        timed = (t >= inp["max_episode_steps"]) if inp["max_episode_steps"] > 0 else np.zeros(Bn, bool)
        end = flag | timed
        ob_s, st_s, rew_s, term_s, trunc_s = oracle.gym_step(env_name, solver, st, a, props, tau, control=ctl)
        pick = e % n_rows
        st_r = [np.choose(pick, [inp["reset"][r][j] for r in range(n_rows)]) for j in range(len(st))]
        st = [np.where(end, r, s) for r, s in zip(st_r, st_s)]
        rew_r, term_r, trunc_r = row_outputs(env_name, st, props, ctl)
        rew = np.where(end, rew_r, rew_s[:, 0])
        term = np.where(end, term_r, term_s[:, 0].astype(bool))
        trunc = np.where(end[:, None], trunc_r, trunc_s.astype(bool))
        ob = np.where(end[:, None], observe(st), ob_s)
        e += end
        t = np.where(end, 0, t + 1)
        acts.append(a)
        resets.append(end)
        flagged.append(flag)
        timed_only.append(timed & ~flag)
        rows_o.append(ob)
        rows_s.append(st)
        rews.append(rew)
        terms.append(term)
        truncs.append(trunc)
    S = len(st)
    stack = lambda rows, empty: np.stack(rows, axis=1) if rows else empty
    return dict(obs=np.stack(rows_o, axis=1), states=[np.stack([r[j] for r in rows_s], axis=1) for j in range(S)], last=st,
                actions=stack(acts, np.zeros((Bn, 0, A))), reward=stack(rews, np.zeros((Bn, 0))), terminated=stack(terms, np.zeros((Bn, 0), bool)),
                truncated=np.stack(truncs, axis=1), reset=stack(resets, np.zeros((Bn, 0), bool)), flag_reset=stack(flagged, np.zeros((Bn, 0), bool)),
                time_only=stack(timed_only, np.zeros((Bn, 0), bool)), n_resets=e.astype(np.int32), steps_out=t.astype(np.int32), term0=term0)


@functools.lru_cache(maxsize=None)
def main_case(env_name, deadtime, case):
    """(spec, inputs) of a main case, float64, computed once per process"""
    spec = case_spec(env_name, deadtime)
    return spec, episode_inputs(env_name, spec, case)


@functools.lru_cache(maxsize=None)
def oracle_case(env_name, deadtime, solver, case, activation):
    """The float64 oracle episode loop of a main case, once per process (the CPU input condition and GPU test 5 share it)"""
    spec, inp = main_case(env_name, deadtime, case)
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    return oracle_episode_loop(env_name, solver, props, inp, spec["tau"], activation)
