"""The draws of the randomised closed-loop tests (tests/test_gpu_fuzz_closed_loop.py on the GPU, tests/test_fuzz_closed_loop_host.py for
their input conditions on the CPU). Nothing here needs a GPU.

One draw function per launch family — `vmap_sim_ahead_feedback` (draw_feedback), its reverse mode `vmap_sim_ahead_feedback_vjp`
(draw_vjp) and `vmap_sim_ahead_policy` (draw_policy). A draw crosses what the fixed suites vary one axis at a time: model, solver,
number format, batch sizes around the block sizes (64, 256) and the slices of the batch sum, K, substeps, PMSM dead time, up to
EXCENV_MAX_CONTROL control columns, per-environment properties (forward families), the policy's forms. A draw is a pair (cfg, spec):
cfg a plain dict that a failing test prints in full, spec the model's specification with the drawn per-environment arrays (None for
the saturated PMSM, whose specification comes from helpers_feedback.saturated_env). The inputs of a draw are
helpers_feedback.feedback_inputs' and helpers_policy.policy_inputs' under the draw's seed: no new distribution.

Seed bases. Draw `i` of a family uses default_rng(BASE[family] + i). The bases 21000 / 22349 / 23065 are the first ones, searched
upwards from 21000 / 22000 / 23000 with tests/test_fuzz_closed_loop_host.py's own checks, whose 24 draws meet the input conditions of that
file: every batch size, model, solver and gain form occurs, a draw with >= 4 control columns, a broadcast-gain reverse draw with
A * OW > 2 * EXCENV_MAX_STATIC, a policy whose widest hidden layer is not the first, the clamp and ReLU shares, and (fp32 reverse
draws) the share of environments within KINK_MARGIN of a kink at most KINK_CAP."""
import os

import numpy as np

import oracle
import helpers_feedback as hf
import helpers_policy as hp
from conftest import ENV_NAMES
from helpers import spec_of

BASE = {"feedback": 21000, "vjp": 22349, "policy": 23065}
DEFAULT_SEEDS = 24
SATURATED = "pmsm_saturated"  # the seventh model of the forward families
B_LIST = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1031]
K_LIST = [0, 1, 2, 5, 7]
SOLVERS = ["euler", "rk4", "tsit5"]
DTYPES = ["float32", "float64"]
CLIPS = [(-1.0, 1.0), (-0.25, 0.5), None]
GAIN_FORMS = ["broadcast", "per_env", "mixed"]  # mixed: a broadcast gain next to a per-environment integral gain
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 33, 63, 64]
MAX_CONTROL, MAX_STATIC = 8, 9  # include/excenv.h EXCENV_MAX_CONTROL, EXCENV_MAX_STATIC
COTANGENTS = ("obs", "states", "last", "actions", "z")


def n_seeds():
    return int(os.environ.get("EXCENV_FUZZ_SEEDS", str(DEFAULT_SEEDS)))


def model_of(cfg):
    """The model's name for the oracle, the twin and the input helpers"""
    return "pmsm" if cfg["env_name"] == SATURATED else cfg["env_name"]


def _choice(rng, options):
    return options[int(rng.integers(len(options)))]


def _common(rng, family, seed):
    """The axes every family shares -> (cfg, spec)"""
    forward = family != "vjp"
    names = ENV_NAMES + ([SATURATED] if forward else [])
    env_name = _choice(rng, names)
    model = "pmsm" if env_name == SATURATED else env_name
    cfg = dict(family=family, seed=int(seed), env_name=env_name, solver=_choice(rng, SOLVERS), dtype=_choice(rng, DTYPES),
               B=int(_choice(rng, B_LIST)), K=int(_choice(rng, K_LIST)), substeps=1 if model == "pmsm" else int(_choice(rng, [1, 2, 3])),
               deadtime=int(rng.integers(2)) if env_name == "pmsm" else None)
    spec = None
    if env_name != SATURATED:
        spec = spec_of(model)
        if cfg["deadtime"] is not None:
            spec["params"]["deadtime"] = cfg["deadtime"]
    # control columns: none, one, two, or every state field (at most EXCENV_MAX_CONTROL), in a random order
    fields = oracle.STATE_FIELDS[model]
    n_ctl = min(_choice(rng, [0, 1, 2, min(len(fields), MAX_CONTROL)]), len(fields))
    cfg["control"] = [fields[int(i)] for i in rng.choice(len(fields), size=n_ctl, replace=False)]
    # per-environment property arrays as tests/test_gpu_fuzz.py draws them (forward families; the reverse entry refuses them, and the
    # saturated PMSM takes no parameter overrides)
    batched = []
    if forward and spec is not None:
        B = cfg["B"]
        for group, keys in (("params", list(spec["params"])), ("phys_norm", list(spec["phys_norm"])), ("act_norm", list(spec["act_norm"]))):
            for k in keys:
                if rng.random() < 0.15 and not (model == "pmsm" and k == "deadtime"):
                    if group == "params":
                        v = float(spec["params"][k])
                        spec["params"][k] = v * rng.uniform(0.8, 1.2, B) if v != 0 else rng.uniform(0.0, 1e-3, B)
                    else:
                        lo, hi = spec[group][k]
                        spec[group][k] = (lo - abs(hi - lo) * rng.uniform(0, 0.1, B), hi)
                    batched.append(f"{group}.{k}")
    cfg["batched"] = batched
    if forward:
        cfg["store_states"] = bool(rng.integers(2))
    return cfg, spec


def _policy_form(rng, cfg):
    """The affine policy's forms, shared by the forward and the reverse family"""
    cfg["gain_form"] = _choice(rng, GAIN_FORMS)
    cfg["integral"] = _choice(rng, ["none", "zeros", "z0"])  # absent; present from zeros; present with an initial integrator state
    if cfg["gain_form"] == "mixed" and cfg["integral"] == "none":
        cfg["integral"] = _choice(rng, ["zeros", "z0"])
    cfg["clip"] = _choice(rng, CLIPS)


def draw_feedback(rng, seed=0):
    cfg, spec = _common(rng, "feedback", seed)
    _policy_form(rng, cfg)
    cfg["feedforward"] = _choice(rng, ["none", "lane_major", "plain"])
    return cfg, spec


def draw_vjp(rng, seed=0):
    cfg, spec = _common(rng, "vjp", seed)
    _policy_form(rng, cfg)
    cfg["feedforward"] = _choice(rng, ["none", "plain"])
    S = len(oracle.STATE_FIELDS[cfg["env_name"]])
    picked = [c for c in COTANGENTS if rng.random() < 0.5]
    cfg["cotangents"] = picked
    # individual state leaves may be absent: the leaves of `states` / `last` that do get a cotangent (never none of them)
    for name in ("states", "last"):
        leaves = [j for j in range(S) if rng.random() < 0.7]
        cfg[f"{name}_leaves"] = leaves or [int(rng.integers(S))]
    cfg["cotangents"] = effective_cotangents(cfg)
    # one draw in four asks the entry for what it refuses by name; nothing is launched there
    cfg["refusal"] = _choice(rng, ["per_env", "saturated"]) if rng.random() < 0.25 else None
    return cfg, spec


def effective_cotangents(cfg):
    """The drawn subset without what the call cannot take (actions without action rows, z without an integrator); never empty"""
    out = [c for c in cfg["cotangents"] if not (c == "actions" and cfg["K"] == 0) and not (c == "z" and cfg["integral"] == "none")]
    return out or ["obs"]


def draw_policy(rng, seed=0):
    cfg, spec = _common(rng, "policy", seed)
    L = int(rng.integers(1, 5))
    hidden = [int(_choice(rng, WIDTHS)) for _ in range(L - 1)]
    # the dynamic LDS is sized by the widest hidden layer wherever it stands: in three draws of four with two or more hidden layers
    # the widest one is moved off the first place
    if len(hidden) >= 2 and rng.random() < 0.75 and max(hidden[1:]) <= hidden[0]:
        j = int(rng.integers(1, len(hidden)))
        hidden[0], hidden[j] = hidden[j], hidden[0]
        if hidden[0] == hidden[j]:  # a tie: the first one steps down the list of widths (from 1: the later one steps up)
            i = WIDTHS.index(hidden[0])
            if i > 0:
                hidden[0] = WIDTHS[i - 1]
            else:
                hidden[j] = WIDTHS[1]
    cfg["hidden"] = tuple(hidden)
    cfg["activation"] = _choice(rng, list(hp.ACTIVATIONS))
    cfg["noise"] = bool(rng.integers(2))
    cfg["clip"] = _choice(rng, CLIPS)
    return cfg, spec


DRAW = {"feedback": draw_feedback, "vjp": draw_vjp, "policy": draw_policy}


def draw(family, i):
    """Draw `i` of a family -> (cfg, spec)"""
    seed = BASE[family] + i
    return DRAW[family](np.random.default_rng(seed), seed)


def widest_not_first(hidden):
    return len(hidden) >= 2 and max(hidden[1:]) > hidden[0]


def describe(cfg):
    return ", ".join(f"{k}={v}" for k, v in cfg.items())


# ---- the inputs of a draw ----------------------------------------------------------------------------------------------------------
def feedback_case(cfg, spec):
    """helpers_feedback.feedback_inputs of a feedback / vjp draw in its gain form, float64"""
    model = model_of(cfg)
    integral = cfg["integral"] != "none"
    inp = dict(hf.feedback_inputs(model, spec, cfg["B"], cfg["K"], seed=cfg["seed"], control=cfg["control"] or None,
                                  per_env_gains=cfg["gain_form"] != "broadcast", integral=integral, feedforward=cfg["feedforward"] != "none"))
    if cfg["gain_form"] == "mixed":
        inp["gain"] = inp["gain"][0].copy()  # [A, OW] next to a [B, A, OW] integral gain
    if cfg["integral"] == "zeros":
        inp["z0"] = None
    return inp


def policy_case(cfg, spec):
    """helpers_policy.policy_inputs of a policy draw, float64"""
    return hp.policy_inputs(model_of(cfg), spec, cfg["hidden"], cfg["B"], cfg["K"], control=cfg["control"] or None, seed=cfg["seed"])


def host_props(cfg, spec):
    """-> (spec, float64 oracle properties) of a forward draw without a GPU (the saturated PMSM: from a CPU environment)"""
    if cfg["env_name"] == SATURATED:
        import torch

        _, props, keep, spec = hf.saturated_env(cfg["B"], torch.float64, cfg["solver"], "cpu")
        return spec, (props, keep)
    return spec, oracle.make_props(model_of(cfg), spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, cfg["B"])


def vjp_cotangents(cfg, rows, OW, S, A, dtype=None):
    """The cotangent group of a reverse draw: helpers_feedback_vjp.cotangent_groups' full group under the draw's seed, cut down to the
    drawn subset and leaves; rounded to `dtype` where given"""
    import helpers_feedback_vjp as hv

    full = hv.cotangent_groups(np.random.default_rng(cfg["seed"] + 9000), cfg["B"], rows, OW, S, cfg["K"], A, integral=cfg["integral"] != "none")[0]
    r = (lambda a: a) if dtype is None else (lambda a: a.astype(dtype).astype(np.float64))
    group = {}
    for name in cfg["cotangents"]:
        if name in ("states", "last"):
            group[name] = [r(g) if j in cfg[f"{name}_leaves"] else None for j, g in enumerate(full[name])]
        else:
            group[name] = r(full[name])
    return group


def round_to(inp, dtype):
    """The inputs of feedback_case as a kernel of that number format sees them: rounded to it, as float64"""
    r = lambda v: None if v is None else np.asarray(v).astype(dtype).astype(np.float64)
    out = {k: r(inp[k]) for k in ("gain", "igain", "ff", "z0")}
    out["st"] = [r(v) for v in inp["st"]]
    out["refs"] = None if inp.get("refs") is None else {n: r(v) for n, v in inp["refs"].items()}
    return out


# ---- what the CPU references say about a draw (tests/test_fuzz_closed_loop_host.py) -------------------------------------------------
def host_figures(family, i):
    """The input conditions of draw `i` from the oracle or the twin alone -> dict(cfg, clamped: share of action entries the clamp
    changed, negative: share of negative hidden pre-activations (policy), excluded: share of environments within KINK_MARGIN of a
    kink (reverse draws, on the inputs of the draw's number format)); None figures where nothing runs (refusal draws)"""
    cfg, spec = draw(family, i)
    out = dict(cfg=cfg, clamped=None, negative=None, excluded=None)
    model, K, sub, control = model_of(cfg), cfg["K"], cfg["substeps"], cfg["control"] or None
    if family == "vjp":
        import helpers_feedback_vjp as hv
        from helpers_vjp import KINK_MARGIN

        if cfg["refusal"]:
            return out
        inp = feedback_case(cfg, spec)
        if cfg["dtype"] == "float32":
            inp = round_to(inp, np.float32)
        twin, _, res = hv.twin_run(model, spec, cfg["solver"], inp, K, sub, clip=cfg["clip"], control=control)
        kd = twin.kink_distance()
        out["clamped"] = res["clamped"]
        out["excluded"] = 0.0 if kd is None else 1.0 - float(np.mean(kd.numpy() >= KINK_MARGIN))
        return out
    spec, (props, _keep) = host_props(cfg, spec)
    if family == "feedback":
        res = hf.oracle_closed_loop(model, cfg["solver"], props, feedback_case(cfg, spec), spec["tau"], K=K, sub=sub, clip=cfg["clip"],
                                    control=control)
    else:
        res = hp.oracle_policy_loop(model, cfg["solver"], props, policy_case(cfg, spec), spec["tau"], cfg["activation"], K=K, sub=sub,
                                    clip=cfg["clip"], control=control, noise=cfg["noise"])
        out["negative"] = res["negative"]
    out["clamped"] = res["clamped"]
    return out
