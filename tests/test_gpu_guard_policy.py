"""Guard-band tests of the policy-rollout kernel (``-m gpu``): an excenv_sim_policy launch writes its outputs and nothing else.

Shaped like the excenv_sim_feedback block of tests/test_gpu_guard_reverse.py: the cases call the C ABI with nothing but addresses —
plain, on ordinary torch tensors, and carved, every array a view of one 0xFF-filled arena (tests/helpers_guard.py) with 64 KiB of
untouched pattern on either side, one argument group at a time at the offsets 16, 48, 64 and the element size modulo 256. Per case:
two plain runs are bit-equal; per carved run the guards are untouched, the inputs (the parameter array included) unchanged, every
output element written and equal to the plain run's. Every model, with and without state trajectory / actions_out / noise, B = 1 and
B = 326 (a tail inside a wavefront), K = 0, 1, 7, the widest network (N2: the largest LDS footprint) next to N1 and N0."""
import ctypes
import time

import numpy as np
import pytest
import torch

from helpers import make_env
from helpers_guard import FLOAT_OFFSETS, Carved, Plain, arena_bytes
from helpers_vjp import CASES

pytestmark = pytest.mark.gpu

EHIP = -3
TORCH = {4: torch.float32, 8: torch.float64}
NP = {4: np.float32, 8: np.float64}
POLICY_CASES = [(e, d, elem) for (e, d) in CASES + [("pmsm_sat", None)] for elem in (4, 8)]  # pmsm_sat: the saturated PMSM


class Refused(Exception):
    def __init__(self, rc):
        from exciting_environments_amd import _native

        self.rc, self.message = rc, _native.lib().excenv_last_error().decode("utf-8", "replace")
        super().__init__(f"excenv_sim_policy: rc={rc}: {self.message}")


def _ptrs(alloc, names):
    arr = (ctypes.c_void_p * len(names))()
    for j, name in enumerate(names):
        arr[j] = alloc.addr(name)
    return arr


def two_runs(where, setup, groups, elem):
    """setup(alloc) -> {name: output tensor}; raises Refused. -> problems"""
    from exciting_environments_amd import _native

    problems = []
    plain = Plain()
    ref = setup(plain)
    ref1 = setup(Plain())
    torch.cuda.synchronize()
    if any(not torch.equal(ref[n], ref1[n]) for n in ref):
        problems.append(f"{where}: two plain runs differ in {[n for n in ref if not torch.equal(ref[n], ref1[n])]}")
    size = arena_bytes(plain.sizes)
    for place in [{}] + [{g: o} for g in groups for o in FLOAT_OFFSETS + (elem,)]:
        at = f"{where} @ {place or 'offset 0'}"
        carved = Carved(size, place)
        try:
            got = setup(carved)
        except Refused as e:
            torch.cuda.synchronize()
            if e.rc == EHIP:
                pytest.exit(f"guard {at}: the GPU reported a fault, nothing more is launched: {e}", returncode=3)
            problems.append(f"{at}: refused: {e}")  # (the entry point asks no alignment beyond the element's)
            continue
        torch.cuda.synchronize()
        if _native.last_launch() != "sim_policy_kernel":
            problems.append(f"{at}: launched {_native.last_launch()!r}")
        problems += [f"{at}: {p}" for p in carved.arena.problems()]
        bad = [n for n in ref if not torch.equal(got[n], ref[n])]
        if bad:
            problems.append(f"{at}: {bad} differ from the plain run")
    for p in problems:
        print("guard problem:", p)
    return problems


@pytest.mark.parametrize("env_name,deadtime,elem", POLICY_CASES, ids=lambda v: str(v))
def test_sim_policy(env_name, deadtime, elem):
    from exciting_environments_amd import _native
    from helpers_feedback import saturated_env
    from helpers_policy import CLIP, NETS, policy_inputs, substeps_of
    from helpers_vjp import skewed_spec

    t0 = time.perf_counter()
    dt, npdt = TORCH[elem], NP[elem]
    saturated = env_name == "pmsm_sat"
    env_name = "pmsm" if saturated else env_name
    spec = None if saturated else skewed_spec(env_name, deadtime)
    sub = substeps_of(env_name)
    lib = _native.lib()
    problems = []
    # (B, K, network, activation, state trajectory, actions_out, noise)
    shapes = [(326, 7, "N2", 1, True, True, True), (326, 7, "N1", 0, False, False, False), (326, 1, "N0", 0, True, False, True),
              (1, 7, "N1", 1, False, True, True), (1, 1, "N2", 0, True, True, False), (326, 0, "N1", 1, True, True, True),
              (1, 0, "N0", 1, False, False, False)]
    for B, K, net, activation, states, with_actions, with_noise in shapes:
        if saturated:
            env, _, _, spec = saturated_env(B, dt, "euler", "cuda")
        else:
            env, _, _, _ = make_env(env_name, B, dt, "rk4" if elem == 8 else "euler", spec=spec)
        props, keep = env._props_for(env.env_properties, B)
        S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
        inp = policy_inputs(env_name, spec, NETS[net], B, K)
        flat = np.concatenate([v.reshape(-1) for pair in zip(inp["W"], inp["b"]) for v in pair]).astype(npdt)
        rows = K * sub + 1
        widths = (ctypes.c_int32 * 5)(*(inp["widths"] + (0,) * (5 - len(inp["widths"]))))

        def setup(alloc):
            sin = [f"state_in[{j}]" for j in range(S)]
            for j, n in enumerate(sin):
                alloc(n, (B,), dt, "state_io", fill=np.asarray(inp["st"][j], dtype=npdt))
            alloc("params", (flat.size,), dt, "params", fill=flat)
            if with_noise:
                alloc("noise", (K, A, B), dt, "noise", fill=np.ascontiguousarray(inp["noise"].transpose(1, 2, 0)).astype(npdt))
            out = {"obs": alloc("obs_traj", (rows, OW, B), dt, "obs")}
            tn = [f"state_traj[{j}]" for j in range(S)] if states else None
            for n in tn or []:
                out[n] = alloc(n, (rows, B), dt, "straj")
            ln = [f"last_state[{j}]" for j in range(S)]
            for n in ln:
                out[n] = alloc(n, (B,), dt, "state_io")
            if with_actions:
                out["actions_out"] = alloc("actions_out", (K, A, B), dt, "actions_out")
            alloc.ready()
            pol = _native.Policy(alloc.addr("params"), len(inp["widths"]) - 1, activation, widths,
                                 alloc.addr("noise") if with_noise else None, CLIP[0], CLIP[1])
            with _native._on_device(env.device):
                rc = lib.excenv_sim_policy(env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, K, sub, ctypes.byref(props), None,
                                           float(env.tau), float(env.tau), _ptrs(alloc, sin), ctypes.byref(pol), alloc.addr("obs_traj"),
                                           _ptrs(alloc, tn) if tn else None, _ptrs(alloc, ln),
                                           alloc.addr("actions_out") if with_actions else None, None, _native._raw_stream(env.device))
            if rc:
                raise Refused(rc)
            return out

        groups = ["state_io", "params", "obs"] + (["noise"] if with_noise else []) + (["actions_out"] if with_actions else []) \
            + (["straj"] if states else [])
        where = (f"excenv_sim_policy({env_name}{' saturated' if saturated else ''}, dead={deadtime}, elem={elem}, B={B}, K={K}, net={net}, activation={activation}, "
                 f"states={states}, actions_out={with_actions}, noise={with_noise})")
        try:
            problems += two_runs(where, setup, groups, elem)
        except RuntimeError as e:  # a fault the device reports at a synchronisation ends the run: nothing more is launched after it
            pytest.exit(f"guard policy: {e}", returncode=3)
    print(f"guard policy: {time.perf_counter() - t0:.1f} s")
    assert not problems, "\n".join(problems[:30]) + (f"\n... {len(problems) - 30} more" if len(problems) > 30 else "")
