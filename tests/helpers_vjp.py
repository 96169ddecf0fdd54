"""A float64 torch restatement ("twin") of the six vector fields, the three fixed-step solvers and both trajectory semantics,
written from the reference's Python sources (exciting_environments/*/..._env.py) and the CPU oracle's definitions
(oracle/oracle_body.inc). Its gradients come from torch.autograd on the CPU and are what the reverse-mode kernel is compared with
(tests/test_gpu_vjp.py); its forward is validated against the oracle first (tests/test_vjp_twin.py).

Subgradient conventions (the kernel's): a clamp / clip has derivative 0 on its boundary, sign() has derivative 0,
the tank's sqrt term has derivative 0 where h <= 0. torch.where with strict comparisons states them explicitly.

Everything is vectorised over the batch: state leaves [B], actions [B, K, A]."""
import math

import numpy as np
import torch

import oracle

DT = torch.float64
PI = math.pi
SEM = {"step": oracle.SEM_STEP, "ahead": oracle.SEM_AHEAD}

# Butcher tableaux (Euler: diffrax.Euler; RK4 classic; Tsit5: the first six stages, b7 = 0)
TABLEAU = {
    "rk4": dict(a=[[], [0.5], [0.0, 0.5], [0.0, 0.0, 1.0]], b=[1 / 6, 1 / 3, 1 / 3, 1 / 6], c1=[3]),
    "tsit5": dict(
        a=[[], [0.161], [-0.008480655492356989, 0.335480655492357],
           [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
           [5.325864828439257, -11.74888356406283, 7.4955393428898365, -0.09249506636175525],
           [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383]],
        b=[0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774], c1=[5]),
}


def normalize(x, lo, hi):
    return 2 * (x - lo) / (hi - lo) - 1


def denormalize(x, lo, hi):
    return (x + 1) / 2 * (hi - lo) + lo


def wrap(th):
    return torch.remainder(th + PI, 2 * PI) - PI


def clamp0(x, lo, hi):
    """clip with derivative 0 on and outside the bounds"""
    inside = (x > lo) & (x < hi)
    return torch.where(inside, x, torch.clamp(x.detach(), lo, hi))


class Twin:
    """One environment type with broadcast properties (spec: tests/helpers.spec_of)."""

    def __init__(self, env_name, spec, solver, semantics, tau=None):
        self.env, self.solver, self.sem = env_name, solver, semantics
        self.P = {k: float(v) for k, v in spec["params"].items()}
        self.fields = oracle.STATE_FIELDS[env_name]
        self.smin = [float(spec["phys_norm"][n][0]) for n in self.fields]
        self.smax = [float(spec["phys_norm"][n][1]) for n in self.fields]
        self.amin = [float(spec["act_norm"][n][0]) for n in oracle.ACTION_FIELDS[env_name]]
        self.amax = [float(spec["act_norm"][n][1]) for n in oracle.ACTION_FIELDS[env_name]]
        self.tau = float(spec["tau"] if tau is None else tau)
        self.kinks = []  # per evaluation: relative distances to the nearest kink, [B] tensors (kink mask)
        self.clips = []  # PMSM, per evaluation of the action path: [B] bool, the hexagon clip changed the voltage
        self.levels = []  # tank, per evaluation of f and of the clamp: [B] the level as read (before max(h, 0)), see near_dry()

    # ---- vector fields: y list of [B], u list of [B]; returns list of [B] ----------------------------------------------
    def f(self, y, u, omega_el=None):
        P = self.P
        e = self.env
        if e == "pendulum":
            return [y[1], (u[0] + P["l"] * P["m"] * P["g"] * torch.sin(y[0])) / (P["m"] * (P["l"] * P["l"]))]
        if e == "mass_spring_damper":
            return [y[1], (u[0] - P["d"] * y[1] - P["k"] * y[0]) / P["m"]]
        if e == "cartpole":
            mu_p, mu_c, l, m_p, m_c, g = (P[k] for k in ("mu_p", "mu_c", "l", "m_p", "m_c", "g"))
            vel, th, om = y[1], y[2], y[3]
            s, co = torch.sin(th), torch.cos(th)
            sg = torch.sign(vel.detach())
            self.kinks.append(vel.detach().abs() / (self.smax[1] - self.smin[1]))
            d_om = (g * s + co * ((-u[0] - m_p * l * (om * om) * s + mu_c * sg) / (m_c + m_p)) - mu_p * om / (m_p * l)) / (
                l * (4.0 / 3.0 - m_p * (co * co) / (m_c + m_p)))
            d_vel = (u[0] + m_p * l * ((om * om) * s - d_om * co) - mu_c * sg) / (m_c + m_p)
            return [vel, d_vel, om, d_om]
        if e == "acrobot":
            g, l_1, m_1, m_2, l_c1, l_c2, I_1, I_2 = (P[k] for k in ("g", "l_1", "m_1", "m_2", "l_c1", "l_c2", "I_1", "I_2"))
            th1, th2, om1, om2 = y
            s2, c2 = torch.sin(th2), torch.cos(th2)
            d_11 = m_1 * (l_c1 * l_c1) + m_2 * (l_1 * l_1 + l_c2 * l_c2 + 2 * l_1 * l_c2 * c2) + I_1 + I_2
            d_12 = m_2 * (l_c2 * l_c2 + l_1 * l_c2 * c2) + I_2
            d_22 = m_2 * (l_c2 * l_c2) + I_2
            h_1 = -m_2 * l_1 * l_c2 * s2 * (om2 * om2) - 2 * m_2 * l_1 * l_c2 * s2 * om1 * om2
            h_2 = m_2 * l_1 * l_c2 * s2 * (om1 * om1)
            cA, cB = torch.cos(th1 + PI / 2), torch.cos(th1 + th2 + PI / 2)
            phi_1 = (m_1 * l_c1 + m_2 * l_1) * g * cA + m_2 * l_c2 * g * cB
            phi_2 = m_2 * l_c2 * g * cB
            d_om1 = 1 / (d_12 - d_22 / d_12 * d_11) * (u[0] + d_22 / d_12 * (h_1 + phi_1) - h_2 - phi_2)
            d_om2 = (-d_11 * d_om1 - h_1 - phi_1) / d_12
            return [om1, om2, d_om1, d_om2]
        if e == "fluid_tank":
            wet = y[0] > 0
            self.levels.append(y[0].detach())
            self.kinks.append(y[0].detach().abs() / (self.smax[0] - self.smin[0]))
            h = torch.where(wet, y[0], torch.ones_like(y[0]))
            root = torch.where(wet, torch.sqrt(2 * P["g"] * h), torch.zeros_like(h))
            return [u[0] / P["base_area"] - P["c_d"] * P["orifice_area"] / P["base_area"] * root]
        if e == "pmsm":  # y = (i_d, i_q, eps)
            r_s, l_d, l_q, psi_p = P["r_s"], P["l_d"], P["l_q"], P["psi_p"]
            return [(u[0] + omega_el * l_q * y[1] - r_s * y[0]) / l_d,
                    (u[1] - omega_el * (l_d * y[0] + psi_p) - r_s * y[1]) / l_q, omega_el + 0 * y[0]]
        raise KeyError(e)

    def rk_step(self, y, u, u1, dt, omega_el=None):
        if self.solver == "euler":
            dy = self.f(y, u, omega_el)
            return [a + b * dt for a, b in zip(y, dy)]
        tb = TABLEAU[self.solver]
        ks = []
        for s, row in enumerate(tb["a"]):
            yi = list(y)
            if s > 0:
                for j in range(len(y)):
                    acc = 0.0
                    for q, a in enumerate(row):
                        if a != 0.0:
                            acc = a * ks[q][j] + acc
                    yi[j] = y[j] + acc
            dy = self.f(yi, u1 if s in tb["c1"] else u, omega_el)
            ks.append([d * dt for d in dy])
        out = []
        for j in range(len(y)):
            acc = 0.0
            for q, b in enumerate(tb["b"]):
                acc = b * ks[q][j] + acc
            out.append(y[j] + acc)
        return out

    # ---- post-processing of a state (list of S leaves) and the observation ---------------------------------------------
    def post(self, st):
        e = self.env
        st = list(st)
        if e == "pendulum":
            st[0] = wrap(st[0])
        elif e == "cartpole":
            st[2] = wrap(st[2])
        elif e == "acrobot":
            st[0], st[1] = wrap(st[0]), wrap(st[1])
        elif e == "fluid_tank":
            self.levels.append(st[0].detach())
            self.kinks.append(st[0].detach().abs() / (self.smax[0] - self.smin[0]))
            st[0] = torch.where(st[0] > 0, st[0], torch.zeros_like(st[0]))
        elif e == "pmsm":
            st[2] = wrap(st[2])
            st[5] = self.torque(st[3], st[4])
        return st

    def torque(self, i_d, i_q):
        P = self.P
        return 1.5 * P["p"] * (P["psi_p"] + (P["l_d"] - P["l_q"]) * i_d) * i_q

    def observe(self, st):
        n = lambda j: normalize(st[j], self.smin[j], self.smax[j])
        if self.env == "pmsm":
            return torch.stack([n(3), n(4), n(6), n(5), torch.cos(st[2]), torch.sin(st[2]), n(0), n(1)], dim=-1)
        return torch.stack([n(j) for j in range(len(st))], dim=-1)

    # ---- PMSM action path: rotation -> hexagon clip -> rotation back (pmsm_env.py:92-102, 594-616) ------------------------
    def constraint(self, a, eps, omega_el, deadtime):
        P = self.P
        half_dc = P["u_dc"] / 2
        n_d = denormalize(a[0], self.amin[0], self.amax[0]) / half_dc
        n_q = denormalize(a[1], self.amin[1], self.amax[1]) / half_dc
        adv = eps + (deadtime + 0.5) * self.tau * omega_el
        adv = torch.remainder(adv, 2 * PI)
        adv = torch.where(adv > PI, adv - 2 * PI, adv)
        sn, cs = torch.sin(adv), torch.cos(adv)
        re = cs * n_d - sn * n_q
        im = sn * n_d + cs * n_q
        # sector of (re, im): the rotation that maps it to the sector around the real axis's upper neighbour
        red, imd = re.detach(), im.detach()
        t = 1.7320508075688772 * red
        i0, i1, i2 = (imd >= 0).double(), ((-imd - t) >= 0).double(), ((t - imd) >= 0).double()
        q = float(np.float32(0.8660254037844386))
        d = i2 - i1
        ri = q * d
        neg = (1 - i0) * torch.maximum(i1, i2)
        rr = (1 - 0.5 * d.abs()) * (1 - 2 * neg)
        tr = re * rr - im * ri
        ti = re * ri + im * rr
        lim_re, lim_im = 2.0 / 3.0, 2.0 / 3.0 * math.sqrt(3.0)
        # kinks: the clip's faces and the sector seams, relative to the hexagon's size
        seam = torch.minimum(torch.minimum(imd.abs(), (-imd - t).abs()), (t - imd).abs())
        face = torch.minimum(torch.minimum((tr.detach() - lim_re).abs(), (tr.detach() + lim_re).abs()),
                             torch.minimum(ti.detach().abs(), (ti.detach() - lim_im).abs()))
        # a seam only matters where the clip is active (inside the hexagon the clip is the identity in every sector)
        active = (tr.detach().abs() >= lim_re) | (ti.detach() <= 0) | (ti.detach() >= lim_im)
        self.kinks.append(torch.minimum(face, torch.where(active, seam, torch.full_like(seam, 1e9))))
        self.clips.append(active)
        tr = clamp0(tr, -lim_re, lim_re)
        ti = clamp0(ti, 0.0, lim_im)
        al = tr * rr + ti * ri
        be = ti * rr - tr * ri
        return [(cs * al + sn * be) * half_dc, (cs * be - sn * al) * half_dc]

    # ---- trajectories ----------------------------------------------------------------------------------------------------
    def sim_ahead(self, state, actions, obs_stepsize, substeps=1):
        """state: list of S [B] tensors, actions [B, K, A] -> (observations [B, N+1, O], states list of [B, N+1], last list of [B])"""
        self.kinks, self.clips, self.levels = [], [], []
        e = self.env
        K = actions.shape[1]
        N = K * substeps
        dt = float(obs_stepsize)
        pmsm = e == "pmsm"
        st = list(state)
        rows = []
        if pmsm:
            deadtime = self.P["deadtime"]
            dead = deadtime > 0
        if self.sem == "step":
            for n in range(N + 1):
                rows.append(list(st))
                if n == N:
                    break
                k = n // substeps
                a = [actions[:, k, j] for j in range(actions.shape[2])]
                if pmsm:
                    uc = self.constraint(a, st[2], st[6], deadtime)
                    if dead:
                        u = [st[0], st[1]]
                        st[0], st[1] = uc
                    else:
                        u = uc
                    y = self.rk_step([st[3], st[4], st[2]], u, u, dt, st[6])
                    st[3], st[4], st[2] = y
                else:
                    u = [denormalize(a[0], self.amin[0], self.amax[0])]
                    st = self.rk_step(st, u, u, dt)
                st = self.post(st)
        else:
            if pmsm:
                eps0, om = st[2], st[6]
                prev = [st[0], st[1]]
                lin_stop = self.tau * (K - 1)
                t_of = lambda k: lin_stop if k == K - 1 else lin_stop * (k / (K - 1))
            for n in range(N + 1):
                sv = self.post(st)
                if pmsm:
                    sv[0], sv[1] = (prev[0], prev[1]) if dead else (torch.zeros_like(st[0]), torch.zeros_like(st[1]))
                rows.append(sv)
                if n == N:
                    break
                k = n // substeps
                k1 = min((n + 1) // substeps, K - 1)
                a = [actions[:, k, j] for j in range(actions.shape[2])]
                a1 = [actions[:, k1, j] for j in range(actions.shape[2])]
                if pmsm:
                    uc = self.constraint(a, eps0 + t_of(k) * om, om, deadtime)
                    if dead:
                        u = prev
                        u1 = u if k1 == k else uc
                    else:
                        u = uc
                        u1 = self.constraint(a1, eps0 + t_of(k1) * om, om, deadtime) if self.solver != "euler" else u
                    y = self.rk_step([st[3], st[4], st[2]], u, u1, dt, om)
                    st = list(st)
                    st[3], st[4], st[2] = y
                    prev = uc
                else:
                    u = [denormalize(a[0], self.amin[0], self.amax[0])]
                    u1 = [denormalize(a1[0], self.amin[0], self.amax[0])]
                    st = self.rk_step(st, u, u1, dt)
        obs = torch.stack([self.observe(r) for r in rows], dim=1)
        states = [torch.stack([r[j] for r in rows], dim=1) for j in range(len(st))]
        # state clamps: the normalisation box is not a clamp of these models (observations may leave [-1, 1]); nothing to mark
        return obs, states, rows[-1]

    def clip_share(self):
        """PMSM: the share of action-path evaluations of the last sim_ahead in which the hexagon clip was active"""
        return float(torch.stack(self.clips, dim=0).double().mean()) if self.clips else 0.0

    def near_dry(self, margin):
        """Tank, [B] bool: some evaluation of the last sim_ahead read a NONZERO level within `margin` of the range from 0. A level
        that is exactly 0 (the clamp's own output, read again by the next step) is robust — every fp64 evaluation of the same
        trajectory takes the same branch there —, a nonzero one below the margin is not: rounding decides its sign."""
        lv = torch.stack(self.levels, dim=0)
        return ((lv != 0) & (lv.abs() / (self.smax[0] - self.smin[0]) < margin)).any(dim=0)

    def kink_distance(self):
        """[B]: the smallest relative distance to a kink any evaluation of the last sim_ahead came to"""
        if not self.kinks:
            return None
        return torch.stack(self.kinks, dim=0).min(dim=0).values


def leaves(st_np, requires_grad=False):
    return [torch.tensor(np.asarray(v, dtype=np.float64), dtype=DT, requires_grad=requires_grad) for v in st_np]


def vjp(twin, st_np, actions_np, obs_stepsize, substeps, g_obs=None, g_states=None, g_last=None):
    """Gradients of <cotangents, outputs> w.r.t. actions [B, K, A] and every initial state leaf ([B] each), float64 numpy.
    Also returns the kink distance [B] of the forward."""
    st = leaves(st_np, True)
    act = torch.tensor(np.asarray(actions_np, dtype=np.float64), dtype=DT, requires_grad=True)
    obs, states, last = twin.sim_ahead(st, act, obs_stepsize, substeps)
    loss = torch.zeros((), dtype=DT)
    if g_obs is not None:
        loss = loss + (obs * torch.as_tensor(g_obs, dtype=DT)).sum()
    if g_states is not None:
        for s, g in zip(states, g_states):
            if g is not None:
                loss = loss + (s * torch.as_tensor(g, dtype=DT)).sum()
    if g_last is not None:
        for s, g in zip(last, g_last):
            if g is not None:
                loss = loss + (s * torch.as_tensor(g, dtype=DT)).sum()
    grads = torch.autograd.grad(loss, [act] + st, allow_unused=True)
    z = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()
    kd = twin.kink_distance()
    return z(grads[0], act), [z(g, s) for g, s in zip(grads[1:], st)], (None if kd is None else kd.numpy())


# ---- the inputs of the GPU tests (and of the CPU test that checks the kink cap on them) ------------------------------------------
KINK_MARGIN = 1e-4   # relative distance to a kink below which an environment is excluded from the fp32 comparison: ~1000 x the
                     # fp32 unit roundoff (6e-8), i.e. well above what an fp32 run deviates by in the clip's own inputs
KINK_CAP = 0.02      # at most this share of the environments may be excluded


def vjp_inputs(env_name, spec, B, K, seed, np_dtype=np.float64):
    """Seeded initial states and actions for the reverse-mode tests: tank levels away from empty, PMSM actions scaled so that some
    but not most rows clip."""
    from helpers import random_state

    rng = np.random.default_rng(seed + 1000)
    st = random_state(env_name, B, np.float64, spec, seed)
    if env_name == "fluid_tank":
        lo, hi = spec["phys_norm"]["height"]
        st[0] = rng.uniform(0.3, 0.9, B) * (hi - lo) + lo
        acts = rng.uniform(-0.2, 1.0, (B, K, 1))
    elif env_name == "pmsm":
        acts = rng.uniform(-0.75, 0.75, (B, K, 2))
    else:
        acts = rng.uniform(-1, 1, (B, K, 1))
    return [np.asarray(v, dtype=np_dtype) for v in st], acts.astype(np_dtype)


# ---- off-default, asymmetric models ------------------------------------------------------------------------------------------------
# One factor per static parameter: pairwise distinct within a model, none 1, so that no two parameters that are equal at the
# defaults stay equal and none stays at 1 (a transposed Jacobian that swaps two of them, or multiplies where it should divide, gives
# the default results bit for bit). PMSM's pole-pair number is an integer: 3 -> 4.
SKEW = {
    "pendulum": {"g": 1.12, "l": 0.85, "m": 1.3},
    "mass_spring_damper": {"k": 1.2, "d": 0.8, "m": 1.25},
    "cartpole": {"mu_p": 1.3, "mu_c": 0.75, "l": 1.15, "m_p": 0.85, "m_c": 1.25, "g": 1.1},
    "acrobot": {"g": 1.1, "l_1": 0.8, "l_2": 1.2, "m_1": 1.3, "m_2": 0.85, "l_c1": 0.9, "l_c2": 1.15, "I_1": 0.75, "I_2": 1.25},
    "fluid_tank": {"base_area": 1.2, "orifice_area": 0.8, "c_d": 1.3, "g": 0.9},
    "pmsm": {"r_s": 1.3, "l_d": 1.15, "l_q": 0.85, "psi_p": 1.2, "u_dc": 0.9},
}
SKEW_ACTION = {"u_q": (1.3, 0.7)}  # (factor of the lower bound, of the upper bound); every other action field:
SKEW_ACTION_DEFAULT = (0.65, 1.35)
SKEW_PHYSICAL = (1.2, 0.85)        # non-angle state fields; a bound that is 0 moves outwards by 5 % of the range instead


def skewed_spec(env_name, deadtime=None):
    """spec_of(env_name) with every static parameter off its default, asymmetric action ranges (the tank's lower bound nonzero)
    and asymmetric ranges of the non-angle state fields (angles keep +-pi). Broadcast values only. The package takes PMSM's action
    bounds as given (they are not derived from u_dc), so u_dc and the bounds are skewed independently."""
    from helpers import ANGLE_STATES, spec_of

    spec = spec_of(env_name)
    for name, factor in SKEW[env_name].items():
        spec["params"][name] = spec["params"][name] * factor
    if env_name == "pmsm":
        spec["params"]["p"] = 4
        if deadtime is not None:
            spec["params"]["deadtime"] = deadtime
    assert all(v != 1 for k, v in spec["params"].items() if k != "deadtime")
    for name, (lo, hi) in spec["act_norm"].items():
        flo, fhi = SKEW_ACTION.get(name, SKEW_ACTION_DEFAULT)
        spec["act_norm"][name] = (flo * lo if lo != 0 else 0.1 * hi, fhi * hi)
    angles = [oracle.STATE_FIELDS[env_name][j] for j in ANGLE_STATES.get(env_name, [])]
    for name, (lo, hi) in spec["phys_norm"].items():
        if name in angles:
            continue
        span = hi - lo
        spec["phys_norm"][name] = (SKEW_PHYSICAL[0] * lo if lo != 0 else -0.05 * span, SKEW_PHYSICAL[1] * hi if hi != 0 else 0.05 * span)
    return spec


# ---- the dry tank --------------------------------------------------------------------------------------------------------------------
DRY_MARGIN = 1e-9        # a nonzero level within this share of the range from 0: rounding may decide its sign (Twin.near_dry)
DRY_STEP_FACTOR = 1e4    # the step of the dry-tank cases in units of tau (1 s at tau = 1e-4 s): the level moves


def dry_tank_inputs(B=256, K=24):
    """Initial levels of at most 2 cm and mostly no inflow: the tank runs dry within the trajectory and stays dry for rows on end
    (normalised action -1 is the range's lower bound, an inflow of exactly 0 at the default range)."""
    rng = np.random.default_rng(77)
    level = rng.uniform(0.0, 0.02, B)
    closed = rng.uniform(0.0, 1.0, (B, K, 1)) < 0.7
    other = rng.uniform(-1.0, -0.8, (B, K, 1))
    return [level], np.where(closed, -1.0, other)


# ---- one GPU run and what the GPU tests compare it with (tests/test_gpu_vjp.py, tests/test_gpu_vjp_edges.py) -----------------------------
CASES = [(e, None) for e in oracle.STATE_FIELDS if e != "pmsm"] + [("pmsm", 0), ("pmsm", 1)]
SOLVERS = ["euler", "rk4", "tsit5"]


def case_spec(env_name, deadtime):
    from helpers import spec_of

    spec = spec_of(env_name)
    if deadtime is not None:
        spec["params"]["deadtime"] = deadtime
    return spec


def dev(x, env):
    if isinstance(x, torch.Tensor):  # a device tensor as the caller laid it out
        return x
    return torch.as_tensor(np.asarray(x), dtype=env.dtype, device=env.device)


class GpuRun:
    """One forward launch on the GPU and the reverse launches over its state trajectory."""

    def __init__(self, env_name, spec, dtype, solver, semantics, st_np, acts_np, sub=1, control_state=None, envs_per_lane=0,
                 lane_major_actions=True, reference=None, step=None):
        from exciting_environments_amd import _native
        from helpers import make_env, to_state

        self.env, _, _, _ = make_env(env_name, st_np[0].shape[0], dtype, solver, spec=spec, control_state=control_state)
        env = self.env
        env.sim_ahead_semantics = semantics
        if envs_per_lane:
            env.launch_opts = _native.launch_opts(envs_per_lane=envs_per_lane)
        self.tau, self.sub = (spec["tau"] if step is None else step), sub  # the solver's step (obs_stepsize)
        K = acts_np.shape[1]
        if lane_major_actions:
            self.actions = env.new_actions_buffer(K)
            self.actions.copy_(dev(acts_np, env))
        else:
            self.actions = dev(acts_np, env).contiguous()
        self.state = to_state(env, st_np, reference=reference)
        self.obs, self.states, self.last = env.vmap_sim_ahead(self.state, self.actions, self.tau, self.tau * sub)

    def vjp(self, g_obs=None, g_states=None, g_last=None):
        from exciting_environments_amd import _native

        env = self.env
        ga, gs = env.vmap_sim_ahead_vjp(
            self.states, self.actions, self.tau, self.tau * self.sub,
            None if g_obs is None else dev(g_obs, env),
            None if g_states is None else [None if g is None else dev(g, env) for g in g_states],
            None if g_last is None else [None if g is None else dev(g, env) for g in g_last])
        self.launch = _native.last_launch()
        torch.cuda.synchronize()
        return ga.cpu().numpy().astype(np.float64), [getattr(gs, n).cpu().numpy().astype(np.float64) for n in env.STATE_FIELDS]


def cotangents(rng, B, rows, OW, S):
    return rng.normal(size=(B, rows, OW)), [rng.normal(size=(B, rows)) for _ in range(S)], [rng.normal(size=B) for _ in range(S)]


def twin_grads(twin, st_np, acts_np, tau, sub, groups, O):
    """Twin gradients for several cotangent groups over one forward graph -> list of (grad_actions, [grad leaves]), kink distance,
    forward observations. Within a group a leaf's cotangent may be None."""
    st = leaves(st_np, True)
    act = torch.tensor(np.asarray(acts_np, dtype=np.float64), requires_grad=True)
    obs, states, last = twin.sim_ahead(st, act, tau, sub)
    out = []
    for g_obs, g_states, g_last in groups:
        loss = torch.zeros((), dtype=torch.float64)
        if g_obs is not None:
            loss = loss + (obs * torch.as_tensor(g_obs[..., :O])).sum()
        if g_states is not None:
            loss = loss + sum((s * torch.as_tensor(g)).sum() for s, g in zip(states, g_states) if g is not None)
        if g_last is not None:
            loss = loss + sum((s * torch.as_tensor(g)).sum() for s, g in zip(last, g_last) if g is not None)
        gr = torch.autograd.grad(loss, [act] + st, allow_unused=True, retain_graph=True)
        z = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy()
        out.append((z(gr[0], act), [z(g, s) for g, s in zip(gr[1:], st)]))
    return out, twin.kink_distance(), obs.detach().numpy()


def rel_dist(got, want, keep=None):
    """max |got - want| over the kept environments, relative to the tensor's largest magnitude"""
    if keep is not None:
        got, want = got[keep], want[keep]
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    return float(np.max(np.abs(got - want))) / scale if scale > 0 else float(np.max(np.abs(got), initial=0.0))


def obs_floor(got, want, env_name, keep=None):
    """Relative distance of forward observations (the fp32 floor): over the kept environments only, normalised wrapped angles
    compared on the circle of period 2 (an fp32 / fp64 wrap flip at +-pi is no distance)"""
    from helpers import ANGLE_OBS

    got, want = np.array(got, dtype=np.float64), np.array(want, dtype=np.float64)
    if keep is not None:
        got, want = got[keep], want[keep]
    d = np.abs(got - want)
    for c in ANGLE_OBS.get(env_name, []):
        d[..., c] = np.minimum(d[..., c], np.abs(2.0 - d[..., c]))
    return float(d.max()) / float(np.max(np.abs(want)))


# ---- the wide forms (csrc/vjp.hpp vjp_wide_ok, restated) ------------------------------------------------------------------------------
def vjp_wide_ok(env_name, elem, solver):
    """16 bytes per lane exist for every solver of the three small models, the Euler kernels of cart-pole, and of acrobot and
    PMSM with 4-byte elements"""
    if env_name in ("pendulum", "mass_spring_damper", "fluid_tank"):
        return True
    if solver != "euler":
        return False
    return env_name == "cartpole" or elem == 4


WIDE_CASES = [(e, elem, s, sem) for e in oracle.STATE_FIELDS for elem in (4, 8) for s in SOLVERS for sem in ("ahead", "step")
              if vjp_wide_ok(e, elem, s)]
WIDE_LANES, WIDE_K = 326, 7  # lanes: one full workgroup (256), one full wavefront (64) and 6 lanes of a third


def wide_inputs(env_name, elem, spec):
    """The inputs of a wide case: B = V * 326 environments (B % V == 0, B % 64 != 0), K = 7, in the kernel's own number format;
    substeps 3 where the model allows substeps (all but PMSM)"""
    V = 16 // elem
    st, acts = vjp_inputs(env_name, spec, V * WIDE_LANES, WIDE_K, seed=72, np_dtype=np.float32 if elem == 4 else np.float64)
    return V, (1 if env_name == "pmsm" else 3), st, acts
