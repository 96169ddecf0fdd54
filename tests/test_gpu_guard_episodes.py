"""Guard-band tests of the episode-rollout kernel (``-m gpu``): an excenv_sim_policy_episodes launch writes its outputs and nothing else.

Shaped like tests/test_gpu_guard_policy.py: the cases call the C ABI with nothing but addresses — plain, on ordinary torch tensors, and
carved, every array a view of one 0xFF-filled arena (tests/helpers_guard.py) with 64 KiB of untouched pattern on either side, one
argument group at a time at the offsets 16, 48, 64 and the element size modulo 256, the byte outputs also at 4, 2 and 1 (a
`truncated` array that is not 4-byte aligned leaves byte by byte). Per case: two plain runs are bit-equal; per carved run the guards
are untouched, the inputs (the parameter array, the reset rows and the step counters included) unchanged, every output element written
and equal to the plain run's. Every model, with and without each optional output, B = 1 and B = 326 (a tail inside a wavefront),
K = 0, 1, 9."""
import ctypes
import time

import numpy as np
import pytest
import torch

from helpers import make_env
from helpers_guard import BYTE_OFFSETS, FLOAT_OFFSETS, Carved, Plain, arena_bytes
from helpers_vjp import CASES
from test_gpu_guard_policy import EHIP, NP, TORCH, Refused, _ptrs

pytestmark = pytest.mark.gpu

EPISODE_CASES = [(e, d, elem) for (e, d) in CASES + [("pmsm_sat", None)] for elem in (4, 8)]  # pmsm_sat: the saturated PMSM
BYTE_GROUPS = ("terminated", "truncated", "reset")
OPTIONAL = ("reward", "terminated", "truncated", "reset", "n_resets", "steps_out", "steps_in", "actions_out", "straj")


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
    places = [{}] + [{g: o} for g in groups for o in (BYTE_OFFSETS if g in BYTE_GROUPS else FLOAT_OFFSETS + (elem,))]
    for place in places:
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
        if _native.last_launch() != "sim_episodes_kernel":
            problems.append(f"{at}: launched {_native.last_launch()!r}")
        problems += [f"{at}: {p}" for p in carved.arena.problems()]
        bad = [n for n in ref if not torch.equal(got[n], ref[n])]
        if bad:
            problems.append(f"{at}: {bad} differ from the plain run")
    for p in problems:
        print("guard problem:", p)
    return problems


@pytest.mark.parametrize("env_name,deadtime,elem", EPISODE_CASES, ids=lambda v: str(v))
def test_sim_policy_episodes(env_name, deadtime, elem):
    from exciting_environments_amd import _native
    from helpers_episodes import CONTROL, EPISODE_CASES as INPUT_CASES, episode_inputs
    from helpers_feedback import saturated_env
    from helpers_policy import CLIP
    from helpers_vjp import case_spec

    t0 = time.perf_counter()
    dt, npdt = TORCH[elem], NP[elem]
    saturated = env_name == "pmsm_sat"
    env_name = "pmsm" if saturated else env_name
    lib = _native.lib()
    problems = []
    everything = set(OPTIONAL)
    # (B, K, the optional arguments that are there, control columns, end mask)
    shapes = [(326, 9, everything, True, 3), (326, 9, set(), False, 2), (326, 1, everything - {"reward", "reset"}, True, 1),
              (1, 9, everything - {"terminated", "n_resets", "straj"}, True, 3), (1, 1, everything - {"truncated", "steps_out", "steps_in"}, False, 3),
              (326, 0, everything, True, 3), (1, 0, {"truncated"}, False, 0)]
    for B, K, have, controlled, mask in shapes:
        control = CONTROL[env_name] if controlled else None
        if saturated:
            env, _, _, spec = saturated_env(B, dt, "euler", "cuda", control_state=control)
        else:
            spec = case_spec(env_name, deadtime)
            env, _, _, _ = make_env(env_name, B, dt, "rk4" if elem == 8 else "euler", spec=spec, control_state=control)
        props, keep = env._props_for(env.env_properties, B)
        S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
        TW = _native.truncated_width(env.ENV_ID, len(env.control_state))
        inp = episode_inputs(env_name, spec, "E2", B=B, K=K, control=control)
        R = len(inp["reset"])
        flat = np.concatenate([v.reshape(-1) for pair in zip(inp["W"], inp["b"]) for v in pair]).astype(npdt)
        widths = (ctypes.c_int32 * 5)(*(inp["widths"] + (0,) * (5 - len(inp["widths"]))))
        idx = [env.STATE_FIELDS.index(n) for n in control] if control else []

        def setup(alloc):
            sin = [f"state_in[{j}]" for j in range(S)]
            for j, n in enumerate(sin):
                alloc(n, (B,), dt, "state_io", fill=np.asarray(inp["st"][j], dtype=npdt))
            rsn = [f"reset_states[{j}]" for j in range(S)]
            for j, n in enumerate(rsn):
                alloc(n, (R, B), dt, "reset_rows", fill=np.stack([inp["reset"][r][j] for r in range(R)]).astype(npdt))
            rfn = [f"reference[{j}]" for j in range(len(idx))]
            for n, name in zip(rfn, control or []):
                alloc(n, (B,), dt, "reference", fill=np.asarray(inp["refs"][name], dtype=npdt))
            alloc("params", (flat.size,), dt, "params", fill=flat)
            alloc("noise", (K, A, B), dt, "noise", fill=np.ascontiguousarray(inp["noise"].transpose(1, 2, 0)).astype(npdt))
            if "steps_in" in have:
                alloc("steps_in", (B,), torch.int32, "steps_in", fill=inp["steps_in"])
            out = {"obs": alloc("obs_traj", (K + 1, OW, B), dt, "obs")}
            tn = [f"state_traj[{j}]" for j in range(S)] if "straj" in have else None
            for n in tn or []:
                out[n] = alloc(n, (K + 1, B), dt, "straj")
            ln = [f"last_state[{j}]" for j in range(S)]
            for n in ln:
                out[n] = alloc(n, (B,), dt, "state_io")
            if "actions_out" in have:
                out["actions_out"] = alloc("actions_out", (K, A, B), dt, "actions_out")
            if "reward" in have:
                out["reward"] = alloc("reward", (K, B), dt, "reward")
            for n, shape in (("terminated", (K, B)), ("truncated", (K + 1, B, TW)), ("reset", (K, B))):
                if n in have:
                    out[n] = alloc(n, shape, torch.uint8, n)
            for n in ("n_resets", "steps_out"):
                if n in have:
                    out[n] = alloc(n, (B,), torch.int32, "counters")
            alloc.ready()
            pol = _native.Policy(alloc.addr("params"), len(inp["widths"]) - 1, 1, widths, alloc.addr("noise") if K > 0 else None, CLIP[0], CLIP[1])
            ctl = None
            if control:
                ctl = _native.Control(len(idx), (ctypes.c_int32 * 8)(*(idx + [0] * (8 - len(idx)))),
                                      (ctypes.c_void_p * 8)(*([alloc.addr(n) for n in rfn] + [None] * (8 - len(idx)))), (ctypes.c_void_p * 8)())
            rows = _ptrs(alloc, rsn)
            addr = lambda n: alloc.addr(n) if n in have else None
            ep = _native.Episode(ctypes.addressof(rows), R, mask, 2, addr("steps_in"), addr("reward"), addr("terminated"), addr("truncated"),
                                 addr("reset"), addr("n_resets"), addr("steps_out"))
            with _native._on_device(env.device):
                rc = lib.excenv_sim_policy_episodes(env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, K, 1, ctypes.byref(props),
                                                    None if ctl is None else ctypes.byref(ctl), float(env.tau), float(env.tau),
                                                    _ptrs(alloc, sin), ctypes.byref(pol), alloc.addr("obs_traj"),
                                                    _ptrs(alloc, tn) if tn else None, _ptrs(alloc, ln), addr("actions_out"),
                                                    ctypes.byref(ep), None, _native._raw_stream(env.device))
            if rc:
                raise Refused(rc)
            return out

        groups = ["state_io", "reset_rows", "params", "obs", "noise"] + (["reference"] if control else []) \
            + [g for g in ("steps_in", "actions_out", "straj", "reward", "terminated", "truncated", "reset") if g in have] \
            + (["counters"] if have & {"n_resets", "steps_out"} else [])
        where = (f"excenv_sim_policy_episodes({env_name}{' saturated' if saturated else ''}, dead={deadtime}, elem={elem}, B={B}, K={K}, "
                 f"with={sorted(have)}, control={control}, end_mask={mask})")
        try:
            problems += two_runs(where, setup, groups, elem)
        except RuntimeError as e:  # a fault the device reports at a synchronisation ends the run: nothing more is launched after it
            pytest.exit(f"guard episodes: {e}", returncode=3)
    print(f"guard episodes: {time.perf_counter() - t0:.1f} s")
    assert not problems, "\n".join(problems[:30]) + (f"\n... {len(problems) - 30} more" if len(problems) > 30 else "")
