"""Guard-band arena: one allocation filled with 0xFF from which a test carves every buffer a launch reads or writes, so that a
stray store of a correct call lands in memory the test owns and turns into a failure instead of silent corruption.

    arena = Arena(nbytes, device)
    x = arena.carve((B,), torch.float32, offset=16, role="in", name="state_in[0]"); x.copy_(...)
    y = arena.carve((rows, OW, B), torch.float32, role="out", name="obs", permute=(2, 0, 1))   # [B, rows, OW] over lane-major memory
    arena.seal()                      # snapshots the "in" views
    launch(...); torch.cuda.synchronize()
    arena.check()                     # guards untouched, inputs unchanged, every output element written

All-ones is NaN in fp32 and fp64, -1 in the int64 key and hold arrays and 255 in a flag byte: a correct launch on finite inputs
stores none of them, so an output element that still holds the pattern was not written.

Every view has GUARD bytes of pattern in front of it and GUARD bytes behind it that belong to no other view (neighbours do not
share guards). GUARD is 64 KiB: the most one workgroup stores for one row is row_lds <= 64 << 10 (sim_plan.hpp, row_sync == 2); a
1024-thread workgroup of 16-byte stores is 16 KiB.

The limit: a stray store more than GUARD bytes away from every view lands outside the arena, or inside another view where only the
snapshot of an "in" view would notice it, and is not seen. The arena finds the stores of tail lanes, packed flag stores, ring flushes,
transposition tiles and workspaces used beyond their reported size; it does not find a wild pointer.

Works on any device (tests/test_guard_arena_host.py drives it on the CPU)."""
import math

import numpy as np
import torch

GUARD = 64 << 10
PATTERN = 0xFF
ROLES = ("in", "out", "scratch")
_WORD = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def nbytes_of(shape, dtype):
    return int(math.prod(shape)) * torch.empty((), dtype=dtype).element_size()


def arena_bytes(sizes):
    """Bytes an arena needs for views of these byte sizes, whatever their offsets"""
    return sum(int(s) + 2 * GUARD + 256 for s in sizes) + 512


class GuardError(AssertionError):
    pass


class _View:
    __slots__ = ("name", "role", "start", "nbytes", "tensor", "block", "snapshot")


class Arena:
    def __init__(self, nbytes, device="cuda"):
        self.device = torch.device(device)
        self.buf = torch.full((int(nbytes) + 256,), PATTERN, dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = (-self.base) % 256  # arena offsets are counted from a 256-byte boundary
        self.origin = self.cursor
        self.views = []
        self.sealed = False

    # ------------------------------------------------------------------ carving
    def carve(self, shape, dtype, offset=0, role="out", name=None, permute=None):
        """A contiguous view of `shape` whose data_ptr() % 256 == offset, GUARD bytes of pattern on either side. permute: return
        view.permute(*permute) instead (the strided variant: memory [rows][OW][B] seen as [B, rows, OW] is permute=(2, 0, 1)); the
        bytes the result addresses are exactly the block's."""
        assert role in ROLES, role
        assert not self.sealed, "carve every view before seal()"
        isz = torch.empty((), dtype=dtype).element_size()
        assert 0 <= offset < 256 and offset % isz == 0, f"offset {offset} is no multiple of the element size {isz}"
        shape = tuple(int(s) for s in shape)
        n = nbytes_of(shape, dtype)
        start = self.cursor + GUARD
        start += (offset - (self.base + start)) % 256
        end = start + n
        if end + GUARD > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is too small for view {name!r} ({n} bytes at {start})")
        block = self.buf[start:end].view(dtype).view(shape)
        assert name not in [w.name for w in self.views], f"two views named {name!r}"
        v = _View()
        v.name, v.role, v.start, v.nbytes = name or f"view{len(self.views)}", role, start, n
        v.block, v.tensor, v.snapshot = block, (block if permute is None else block.permute(*permute)), None
        self.views.append(v)
        self.cursor = end + GUARD  # the next view's leading guard starts here: guards are not shared
        assert block.data_ptr() % 256 == offset or n == 0
        return v.tensor

    def guard_ranges(self):
        """[(first byte, end byte, name of the view in front or None, name of the view behind or None)] of the pattern regions"""
        out, at, prev = [], 0, None
        for v in self.views:
            out.append((at, v.start, prev, v.name))
            at, prev = v.start + v.nbytes, v.name
        out.append((at, self.buf.numel(), prev, None))
        return out

    def seal(self):
        """Snapshot the "in" views (the caller has filled them) and freeze the arena's map"""
        for v in self.views:
            if v.role == "in":
                v.snapshot = self._bytes(v).clone()
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.device)
        for v in self.views:
            mask[v.start:v.start + v.nbytes] = False
        self.guard_mask = mask
        self.sealed = True

    def _bytes(self, v):
        return self.buf[v.start:v.start + v.nbytes]

    def _neighbours(self, at):
        for a, b, before, after in self.guard_ranges():
            if a <= at < b:
                return before, after
        return None, None

    # ------------------------------------------------------------------ checking
    def problems(self, wrote=True, zero_filled=()):
        """-> list of messages, empty when (1) every guard byte is still 0xFF, (2) every "in" view equals its snapshot bit for bit,
        (3) wrote=True: no element of an "out" view, as a raw integer word, still holds the all-ones pattern (zero_filled: names of
        "out" views that must hold zeros instead); wrote=False: every "out" byte still is 0xFF (a call the library refused)."""
        assert self.sealed, "seal() the arena before the launch"
        out = []
        damaged = ((self.buf != PATTERN) & self.guard_mask).nonzero()
        if damaged.numel():
            first, last = int(damaged[0]), int(damaged[-1])
            fb, fa = self._neighbours(first)
            lb, la = self._neighbours(last)
            out.append(f"guard damaged: {damaged.numel()} bytes, first at arena offset {first - self.origin} (between {fb!r} and {fa!r}"
                       + (f", {first - self._end_of(fb)} bytes behind {fb!r}" if fb else "")
                       + (f", {self._start_of(fa) - first} bytes in front of {fa!r}" if fa else "")
                       + f"), last at {last - self.origin} (between {lb!r} and {la!r})")
        for v in self.views:
            raw = self._bytes(v)
            if v.role == "in":
                if not torch.equal(raw, v.snapshot):
                    bad = (raw != v.snapshot).nonzero()
                    out.append(f"input {v.name!r} changed: {bad.numel()} bytes, first at byte {int(bad[0])}, last at byte {int(bad[-1])}")
            elif v.role == "out" and v.nbytes:
                isz = v.block.element_size()
                words = v.block.reshape(-1).view(_WORD[isz])
                if not wrote:
                    if bool((raw != PATTERN).any()):
                        bad = (raw != PATTERN).nonzero()
                        out.append(f"output {v.name!r} written by a refused call: {bad.numel()} bytes, first at byte {int(bad[0])}")
                elif v.name in zero_filled:
                    if bool((raw != 0).any()):
                        bad = (raw != 0).nonzero()
                        out.append(f"output {v.name!r} not zero-filled: {bad.numel()} bytes, first at byte {int(bad[0])}")
                else:
                    ones = 255 if isz == 1 else -1
                    unwritten = (words == ones).nonzero()
                    if unwritten.numel():
                        out.append(f"output {v.name!r} not written: {unwritten.numel()} of {words.numel()} elements, first at element "
                                   f"{int(unwritten[0])}, last at element {int(unwritten[-1])}")
        return out

    def _start_of(self, name):
        return next(v.start for v in self.views if v.name == name)

    def _end_of(self, name):
        return next(v.start + v.nbytes for v in self.views if v.name == name)

    def check(self, wrote=True, zero_filled=()):
        """Call after torch.cuda.synchronize(). Raises GuardError (an AssertionError) naming every problem."""
        found = self.problems(wrote, zero_filled)
        if found:
            raise GuardError("; ".join(found))

    def reset_outputs(self):
        """Back to the pattern in every "out" and "scratch" view (a second launch into the same arena)"""
        for v in self.views:
            if v.role != "in":
                self._bytes(v).fill_(PATTERN)


# ---------------------------------------------------------------------- the two providers of a two-run case
class Plain:
    """Ordinary torch tensors with the interface of Carved: the run every carved run is compared with. Records the byte size of
    every buffer it hands out (sizes), from which the arena of the carved runs is sized."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.sizes = []
        self.arena = None
        self._addr, self._keep = {}, []

    def __call__(self, name, shape, dtype, group=None, role=None, fill=None, permute=None):
        shape = tuple(int(s) for s in shape)
        self.sizes.append(nbytes_of(shape, dtype))
        if fill is not None:
            t = torch.tensor(np.asarray(fill), dtype=dtype).reshape(shape).contiguous().to(self.device)  # a copy: the inputs stay as they are
        else:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
        self._keep.append(t)  # the caller may hold the address only
        if t.numel() == 0:  # an empty array still has an address (torch reports 0 for it)
            self._keep.append(torch.zeros(16, dtype=torch.uint8, device=self.device))
            self._addr[name] = self._keep[-1].data_ptr()
        else:
            self._addr[name] = t.data_ptr()
        return t if permute is None else t.permute(*permute)

    def ready(self):
        pass

    def addr(self, name):
        """Device address of the buffer of that name"""
        return self._addr[name]


class Carved:
    """Every buffer a view of one Arena. placement: {argument group: offset in bytes modulo 256}; a group that is not named lies at
    offset 0."""

    def __init__(self, nbytes, placement=None, device="cuda"):
        self.arena = Arena(nbytes, device)
        self.placement = dict(placement or {})
        self.device = self.arena.device

    def __call__(self, name, shape, dtype, group=None, role=None, fill=None, permute=None):
        """role: "in" with a fill and "out" without one unless given ("scratch" with a fill: a buffer updated in place)"""
        role = role or ("in" if fill is not None else "out")
        t = self.arena.carve(shape, dtype, self.placement.get(group, 0), role, name, permute)
        if fill is not None:
            block = self.arena.views[-1].block
            block.copy_(torch.tensor(np.asarray(fill), dtype=dtype).reshape(block.shape))
        return t

    def ready(self):
        self.arena.seal()

    def addr(self, name):
        return self.arena.base + self.arena._start_of(name)


# ====================================================================== the forward cases (tests/test_gpu_guard_forward.py)
# Shared with tests/test_guard_arena_host.py, which proves the condition behind "everything was written": the CPU oracle's outputs on
# every case's inputs are finite and its flags are 0 or 1. Nothing below needs a GPU.
FLOAT_OFFSETS = (16, 48, 64)       # inside a 64-byte sector (16, 48); 16-byte aligned but not 128-byte aligned (64); + the element size
BYTE_OFFSETS = (16, 48, 64, 4, 2, 1)
BYTE_GROUPS = ("terminated", "truncated")
ACTION_RANGE = 1.1                 # normalised actions reach past the clip
VMAX = {"float32": 4, "float64": 2}
ELEM = {"float32": 4, "float64": 8}
HOLD_MIN, HOLD_MAX = 10, 1000      # GymWrapper's default ref_params


def control_names(env_name, controls):
    """controls: 0, 1, 2 or "max" (every state field) -> the controlled field names"""
    import oracle

    fields = oracle.STATE_FIELDS[env_name]
    n = len(fields) if controls == "max" else min(int(controls), len(fields))
    return tuple(fields[:n])


def guard_spec(model, B, per_env=False):
    """helpers_forms.linear_spec (off-default, asymmetric); per_env: one static parameter, one state range and one action range
    become [B] arrays (what sends a call to the general kernels)"""
    from helpers_forms import linear_spec

    spec = linear_spec(model)
    if per_env:
        rng = np.random.default_rng(41)
        name = next(k for k in spec["params"] if k not in ("p", "deadtime"))
        spec["params"][name] = float(spec["params"][name]) * rng.uniform(0.9, 1.1, B)
        f = next(iter(spec["phys_norm"]))
        lo, hi = spec["phys_norm"][f]
        spec["phys_norm"][f] = (lo - abs(hi - lo) * rng.uniform(0.0, 0.1, B), hi)
        a = next(iter(spec["act_norm"]))
        lo, hi = spec["act_norm"][a]
        spec["act_norm"][a] = (lo, hi + abs(hi - lo) * rng.uniform(0.0, 0.1, B))
    return spec


def saturated_host_spec(model):
    """The saturated PMSM's specification and prepared tables without a GPU (helpers_lut.make_saturated's, from a CPU environment)"""
    import torch as _torch

    from exciting_environments_amd import EnvironmentRegistry, MotorVariant, prepare_pmsm_lut
    from helpers_forms import saturated_tables

    lut = saturated_tables(model)
    env = EnvironmentRegistry.PMSM.make(batch_size=1, saturated=True, motor_variant=MotorVariant.BRUSA, pmsm_lut=lut, dtype=_torch.float64,
                                        device="cpu")
    ep = env.env_properties
    params = {n: getattr(ep.static_params, n) for n in env.PARAM_FIELDS}
    pn = {n: (getattr(ep.physical_normalizations, n).min, getattr(ep.physical_normalizations, n).max) for n in env.STATE_FIELDS}
    an = {n: (getattr(ep.action_normalizations, n).min, getattr(ep.action_normalizations, n).max) for n in env.ACTION_FIELDS}
    return dict(params=params, phys_norm=pn, act_norm=an, tau=env.tau), prepare_pmsm_lut(lut)


def guard_inputs(env_name, spec, dtype, B, K, names, rows=0, seed=7):
    """Seeded inputs of one case, in the kernel's own number format: states inside the normalisation box, K action rows in
    [-1.1, 1.1], one reference per controlled field, normalised observations, keys and hold counters of the reference generator,
    and (rows > 0) stored state leaves [B, rows] up to 1.2 times the box with references that vary along the rows."""
    import oracle
    from helpers import random_state

    npdt = np.dtype(dtype).type
    rng = np.random.default_rng(seed + 1)
    A = len(oracle.ACTION_FIELDS[env_name])
    O = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][2]
    box = {n: (np.broadcast_to(np.asarray(lo, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (B,)))
           for n, (lo, hi) in spec["phys_norm"].items()}
    out = dict(st=random_state(env_name, B, npdt, spec, seed), acts=rng.uniform(-ACTION_RANGE, ACTION_RANGE, (B, K, A)).astype(npdt))
    out["refs"] = [((rng.uniform(-0.9, 0.9, B) + 1) / 2 * (box[n][1] - box[n][0]) + box[n][0]).astype(npdt) for n in names]
    out["obs"] = rng.uniform(-1.0, 1.0, (B, O + len(names))).astype(npdt)
    out["keys"] = oracle.split(oracle.prng_key(seed), B).astype(np.int64)
    out["hold"] = rng.choice([0, 0, 1, 5], B).astype(np.int64)
    if rows:
        fields = oracle.STATE_FIELDS[env_name]
        out["leaves"] = [((rng.uniform(-1.2, 1.2, (B, rows)) + 1) / 2 * (box[n][1] - box[n][0])[:, None] + box[n][0][:, None]).astype(npdt)
                         for n in fields]
        out["row_refs"] = [((rng.uniform(-1.0, 1.0, (B, rows)) + 1) / 2 * (box[n][1] - box[n][0])[:, None] + box[n][0][:, None]).astype(npdt)
                           for n in names]
    return out


def emr_period(env_name, dtype, K, ahead):
    """sim_plan.hpp emr_rows / emr_period restated: environments between the lanes of a register-ring wave"""
    import math as _m

    import oracle

    S = len(oracle.STATE_FIELDS[env_name])
    pmsm = env_name == "pmsm"
    ring = S - (1 if pmsm else 0) - (1 if (pmsm and ahead) else 0)
    elem = ELEM[dtype]
    W = (128 if ring * 32 <= 128 // (elem // 4) else 64) // elem
    return W // _m.gcd(W, (K + 1) % W) if (K + 1) % W else 1


def groups_of(c):
    """The argument groups of a case that a placement can move"""
    kind = c["kind"]
    if kind in ("sim", "step"):
        g = ["obs", "state_io"]
        if kind == "step" or c["K"] > 0:
            g.insert(0, "actions")
        if kind == "sim" and c["states"]:
            g.append("straj")
        if c["controls"]:
            g.append("refs")
        if c["gym"]:
            g += ["reward", "terminated", "truncated"]
        if kind == "sim" and c["ws"]:
            g.append("workspace")
        return g
    if kind == "rew":
        return ["straj", "reward", "terminated", "truncated"] + (["refs"] if c["controls"] else [])
    if kind == "transpose":
        return ["in", "out"]
    refs = ["refs"] if c["controls"] else []
    return {"observe": ["state_io", "obs"] + refs, "from_obs": ["obs", "state_io"] + refs, "random_state": ["keys", "state_io"],
            "update_ref_to": refs + ["keys"], "update_ref": refs + ["keys"]}[kind]


def placements(c, sweep="full", extra=()):
    """[{group: offset}]: everything at offset 0 first, then one group at a time. sweep: "full" (every offset), "one" (16 and the
    element size only: the large batches), "none". extra: further offsets for the float groups."""
    out = [{}]
    if sweep == "none":
        return out
    elem = ELEM[c["dtype"]]
    for g in c.get("groups") or groups_of(c):
        if g in BYTE_GROUPS:
            offs = BYTE_OFFSETS if sweep == "full" else (16, 1)
        elif g == "keys":
            offs = (16, 48, 64, 8) if sweep == "full" else (8,)
        else:
            offs = (FLOAT_OFFSETS + (elem,) + tuple(extra)) if sweep == "full" else (16, elem)
        out += [{g: o} for o in offs]
    return out


def _case(kind, **kw):
    base = dict(kind=kind, solver="euler", K=0, sub=1, sem="step", controls=0, per_env=False, gym=False, a="lane", t="lane", states=True,
                epl=0, emm=0, flags=0, ws=False, expect=None, sweep="full", extra=(), keep_twice=False)
    base.update(kw)
    return base


SHAPES = [(0, 1), (1, 1), (2, 3), (7, 1)]  # (K, substeps): no row, one, two with substeps, seven; PMSM runs the substeps as 1


def _env(model):
    from helpers_forms import MODEL_CASES

    return MODEL_CASES[model][0]


SIX = ["pendulum", "mass_spring_damper", "cartpole", "acrobot", "fluid_tank", "pmsm_deadtime1"]
DTYPES = ["float32", "float64"]


def _sub(model, sub):
    return 1 if _env(model) == "pmsm" else sub


def fallen_width(V, B):
    """The lane width a request for V environments per lane runs at batch size B: halved until it divides B"""
    while V > 1 and B % V:
        V //= 2
    return V


def _lean_name(V, sem="step", wide=False):
    w = ", 1024 threads" if wide else ""
    return f"sim_ahead_kernel (V={V}{w}, accumulated t)" if sem == "ahead_accumulated_t" else f"sim_ahead_kernel (V={V}{w})"


def forward_rows():
    """{row name: [case]}: the table of the issue, row by row. A case is a dict (see _case): what is launched, how it is forced, the
    form it must report at offset 0 (expect; None where the table names no single form) and how far its placements are swept."""
    rows = {}
    # -- step_kernel / gym step
    r = rows["step"] = []
    for m in SIX:
        for d in DTYPES:
            for B in (1, 63, 65, 257):
                for controls, gym in ((0, False), (2, False), (0, True), (2, True)):
                    r.append(_case("step", model=m, dtype=d, B=B, controls=controls, gym=gym,
                                   expect="step_kernel (general)" if (controls or gym) else "step_kernel (V=1)",
                                   solver="rk4" if (m == "pendulum" and B == 65) else "euler"))
            for V in (1, 2, 4):
                if V <= VMAX[d]:
                    r.append(_case("step", model=m, dtype=d, B=1304, epl=V, expect=f"step_kernel (V={V})"))
            for B in (1302, 1301):  # the widest request steps down to two and to one per lane
                r.append(_case("step", model=m, dtype=d, B=B, epl=VMAX[d], expect=f"step_kernel (V={fallen_width(VMAX[d], B)})", sweep="one"))
            r.append(_case("step", model=m, dtype=d, B=257, per_env=True, expect="step_kernel (general)", sweep="one"))
    # -- sim_ahead_kernel general: per-environment properties, control columns and gym outputs together
    r = rows["general"] = []
    for m in ("pendulum", "cartpole", "fluid_tank", "pmsm_deadtime1"):
        for d in DTYPES:
            for B in (1, 65, 257):
                for K, sub in SHAPES:
                    r.append(_case("sim", model=m, dtype=d, B=B, K=K, sub=_sub(m, sub), per_env=True, controls=2, gym=True,
                                   sem="ahead" if K == 2 else "step", solver="rk4" if (m == "pendulum" and K == 7) else "euler",
                                   expect="sim_ahead_kernel (general)", sweep="full" if B == 65 else "one"))
            r.append(_case("sim", model=m, dtype=d, B=65, K=7, sub=_sub(m, 3), per_env=True, sem="ahead_accumulated_t",
                           expect="sim_ahead_kernel (general, accumulated t)", sweep="one"))
    # -- sim_ahead_kernel lean V = 1, 2, 4
    r = rows["lean"] = []
    for m, solver in (("pendulum", "euler"), ("pmsm_deadtime1", "euler"), ("acrobot", "rk4"), ("mass_spring_damper", "euler")):
        for d in DTYPES:
            for V in (1, 2, 4):
                if V > VMAX[d]:
                    continue
                for B, K, sub, sem, states in ((1304, 7, 1, "step", True), (1304, 2, 3, "ahead", False), (1304, 7, 3, "ahead_accumulated_t", True),
                                               (1304, 0, 1, "step", True), (1304, 1, 1, "ahead", True), (1300, 7, 1, "step", True),
                                               (1302, 7, 1, "step", True), (1301, 7, 1, "step", False), (1302, 2, 1, "ahead_accumulated_t", True),
                                               (1304, 2, 1, "ahead_accumulated_t", False)):
                    # 1300 divides by four; 1302 only by two and 1301 by neither: the forced width steps down (plan_lane_major)
                    runs = fallen_width(V, B)
                    r.append(_case("sim", model=m, solver=solver, dtype=d, B=B, K=K, sub=_sub(m, sub), sem=sem, states=states, epl=V,
                                   expect=_lean_name(runs, sem), sweep="full" if K == 7 and sem == "step" else "one"))
                if _env(m) == "pmsm":  # the constant columns stay as the first launch into the same buffers left them
                    r.append(_case("sim", model=m, solver=solver, dtype=d, B=1304, K=7, epl=V, flags=2, keep_twice=True,
                                   expect=_lean_name(V), sweep="one"))
    # -- lean gym outputs: every model with no, one and its largest control set at the widest lane
    r = rows["lean_gym"] = []
    for m in SIX:
        for d in DTYPES:
            # V * TW bytes of flags per lane and row (store_flag_bytes): fp32 8 / 12 / 16 (pendulum, mass-spring-damper with 0 / 1 / 2
            # controls), 16 / 20 / 28 / 32 (cart-pole, acrobot with 0 / 1 / 3 / 4), 4 (tank, PMSM); fp64 half of each (14 = 12 + 2 with
            # three controls, 6 and 10 on the 2-byte aligned path)
            for controls in (0, 1, 3, "max") if m in ("cartpole", "acrobot") else (0, 1, "max"):
                Ks = (0, 1, 2, 7) if (m == "pendulum" and controls == "max") else (7,)
                for K in Ks:
                    r.append(_case("sim", model=m, dtype=d, B=1304, K=K, sub=_sub(m, 3 if K == 2 else 1), controls=controls, gym=True,
                                   epl=VMAX[d], sem="ahead" if K == 1 else "step", expect="sim_ahead_kernel (lean, gym outputs)",
                                   sweep="full" if K == 7 else "one"))
    # -- control columns filled behind the lean kernel
    r = rows["control_fill"] = []
    for m in ("pendulum", "pmsm_deadtime0"):
        for d in DTYPES:
            for V in (1, VMAX[d]):
                r.append(_case("sim", model=m, dtype=d, B=1304, K=7, controls=2, epl=V, sem="ahead", expect=_lean_name(V)))
    # -- row-major actions read by the lean kernel
    r = rows["aem"] = []
    for m in ("pendulum", "cartpole", "pmsm_deadtime1"):
        for d in DTYPES:
            for K in (4, 8):
                for controls in (0, 2):
                    r.append(_case("sim", model=m, dtype=d, B=768 if d == "float32" else 384, K=K, a="env", controls=controls,
                                   epl=VMAX[d], sem="ahead" if K == 8 else "step", expect="sim_ahead_kernel (row-major actions fused)",
                                   extra=(32,)))
    # -- the LDS-ring env-major kernel and its general variant
    r = rows["em"] = []
    for m in ("pendulum", "acrobot", "pmsm_deadtime1"):
        for d in DTYPES:
            for B in (1, 65, 130):
                for K in (1, 7, 9):
                    A = 2 if _env(m) == "pmsm" else 1
                    fused = (B * K * A * ELEM[d]) % 16 == 0
                    r.append(_case("sim", model=m, dtype=d, B=B, K=K, a="env", t="env", emm=2, sem="ahead" if K == 9 else "step",
                                   solver="rk4" if K == 7 and m == "pendulum" else "euler",
                                   expect="sim_ahead_em_kernel" if fused else None, sweep="full" if (B == 130 and K == 9) else "one"))
                    if K != 7:
                        r.append(_case("sim", model=m, dtype=d, B=B, K=K, a="env", t="env", emm=2, controls=2, per_env=(K == 9),
                                       expect="sim_ahead_em_kernel (general)" if fused else None,
                                       sweep="full" if (B == 130 and K == 9) else "one"))
    # -- the register-ring env-major kernel
    r = rows["emr"] = []
    for m in ("pendulum", "cartpole", "pmsm_deadtime1"):
        for d in DTYPES:
            A = 2 if _env(m) == "pmsm" else 1
            for K in (16 // (A * ELEM[d]), 2 * 16 // (A * ELEM[d])):
                for sem in ("step", "ahead"):
                    P = emr_period(_env(m), d, K, sem != "step")
                    for tail in (1, 63):
                        r.append(_case("sim", model=m, dtype=d, B=64 * P * 2 + tail, K=K, a="env", t="env", emm=3, sem=sem,
                                       expect="sim_ahead_emr_kernel", extra=(128,), groups=["obs", "straj", "actions"],
                                       sweep="full" if tail == 63 else "one"))
    # -- env-major buffers through a workspace of exactly the reported bytes
    r = rows["workspace"] = []
    for m in ("pendulum", "pmsm_deadtime1"):
        for d in DTYPES:
            for B in (65, 4099):
                r.append(_case("sim", model=m, dtype=d, B=B, K=7, sub=_sub(m, 3), a="env", t="env", emm=1, ws=True,
                               expect="transposition workspace + sim_ahead_kernel", sweep="full" if B == 65 else "one"))
                r.append(_case("sim", model=m, dtype=d, B=B, K=7, a="env", t="env", emm=1, ws=True, sem="ahead_accumulated_t", controls=2,
                               expect="transposition workspace + sim_ahead_kernel (accumulated t)", sweep="one"))
                r.append(_case("sim", model=m, dtype=d, B=B, K=7, a="env", t="lane", flags=1, ws=True, states=False,
                               expect="transposition workspace + sim_ahead_kernel", sweep="one"))
    # -- one environment per lane, rows stored together (LDS rows at whole workgroups, barrier rows else)
    r = rows["row_sync"] = []
    for m, d in (("pendulum", "float32"), ("pendulum", "float64"), ("pmsm_deadtime1", "float32")):
        for B in ((1 << 17) + 256, (1 << 17) + 1):
            r.append(_case("sim", model=m, dtype=d, B=B, K=2, epl=1, expect=_lean_name(1), sweep="one", groups=["obs", "straj"]))
    # -- 1024-thread lean form and its gym variant
    r = rows["wide"] = []
    for m in ("pendulum", "mass_spring_damper"):
        for d in DTYPES:
            B = (1 << 20) + 260 if d == "float32" else (1 << 19) + 130
            V = VMAX[d]
            r.append(_case("sim", model=m, dtype=d, B=B, K=2, epl=V, expect=_lean_name(V, wide=True), sweep="one", groups=["obs"]))
            r.append(_case("sim", model=m, dtype=d, B=B, K=2, epl=V, sem="ahead_accumulated_t", states=False,
                           expect=_lean_name(V, "ahead_accumulated_t", wide=True), sweep="none"))
            if not (m == "pendulum" and d == "float64"):  # sim_wide_gym_ok: the fp64 pendulum keeps 256 threads with the gym outputs
                r.append(_case("sim", model=m, dtype=d, B=B, K=2, epl=V, gym=True, controls=1,
                               expect="sim_ahead_kernel (lean, gym outputs, 1024 threads)", sweep="one", groups=["truncated"]))
    # -- saturated PMSM, tables in LDS and in global memory
    r = rows["saturated"] = []
    for m in ("pmsm_saturated_lds", "pmsm_saturated_global"):
        for d in DTYPES:
            for solver in ("euler", "rk4"):
                r.append(_case("sim", model=m, solver=solver, dtype=d, B=257, K=2, expect=_lean_name(1), sweep="one"))
            r.append(_case("step", model=m, dtype=d, B=257, expect="step_kernel (V=1)", sweep="one"))
    # -- rew_trunc_term
    r = rows["rew"] = []
    for m in SIX:
        for d in DTYPES:
            for B in (1, 65, 1304):
                for nrows in (1, 2, 8):
                    for out_lane, in_lane, vary in ((True, True, False), (False, False, True), (True, False, False), (False, True, True)):
                        r.append(_case("rew", model=m, dtype=d, B=B, rows=nrows, controls=2, out_lane=out_lane, in_lane=in_lane, vary=vary,
                                       sweep="full" if (B == 65 and nrows == 8) else "one"))
    # -- the small entry points
    r = rows["small"] = []
    for kind in ("observe", "from_obs", "random_state", "update_ref_to", "update_ref"):
        for m in SIX:
            for d in DTYPES:
                for B in (1, 65, 257):
                    for controls in (0, 2):
                        if kind == "random_state" and controls:
                            continue
                        r.append(_case(kind, model=m, dtype=d, B=B, controls=controls, sweep="full" if B == 65 else "one"))
    r = rows["transpose"] = []
    for d in DTYPES:
        for M, N in ((1, 1), (63, 65), (4099, 12), (12, 4099)):
            r.append(_case("transpose", model=None, dtype=d, M=M, N=N, B=M))
    return rows


def case_id(c):
    keys = ("model", "solver", "dtype", "B", "K", "sub", "sem", "controls", "per_env", "gym", "a", "t", "states", "epl", "emm", "flags", "ws")
    extra = {k: c[k] for k in ("rows", "out_lane", "in_lane", "vary", "M", "N") if k in c}
    return c["kind"] + "(" + ", ".join(f"{k}={c[k]}" for k in keys if c[k] != _case("x").get(k, None) or k in ("model", "dtype", "B")) + \
        ("".join(f", {k}={v}" for k, v in extra.items())) + ")"


# Every string plan_name() (sim_plan.hpp) can return, and the four step_kernel names: what the forward file must reach
FORWARD_FORMS = [
    "sim_ahead_kernel (general)", "sim_ahead_kernel (general, accumulated t)",
    "sim_ahead_kernel (V=1)", "sim_ahead_kernel (V=2)", "sim_ahead_kernel (V=4)",
    "sim_ahead_kernel (V=2, 1024 threads)", "sim_ahead_kernel (V=4, 1024 threads)",
    "sim_ahead_kernel (V=1, accumulated t)", "sim_ahead_kernel (V=2, accumulated t)", "sim_ahead_kernel (V=4, accumulated t)",
    "sim_ahead_kernel (V=2, 1024 threads, accumulated t)", "sim_ahead_kernel (V=4, 1024 threads, accumulated t)",
    "sim_ahead_kernel (lean, gym outputs)", "sim_ahead_kernel (lean, gym outputs, 1024 threads)",
    "sim_ahead_kernel (row-major actions fused)", "sim_ahead_em_kernel", "sim_ahead_em_kernel (general)", "sim_ahead_emr_kernel",
    "transposition workspace + sim_ahead_kernel", "transposition workspace + sim_ahead_kernel (accumulated t)",
    "step_kernel (V=1)", "step_kernel (V=2)", "step_kernel (V=4)", "step_kernel (general)",
]


# ====================================================================== the reverse cases (tests/test_gpu_guard_reverse.py)
# Inputs are those of the existing helpers: helpers_vjp.vjp_inputs / wide_inputs on skewed_spec, helpers_step_vjp.step_inputs,
# helpers_reward_vjp.reward_inputs, helpers_feedback.feedback_inputs.
REV_SEED = 72
REV_K = 7


def rev_sim_cases(pgrad=False):
    """[dict]: excenv_sim_ahead_vjp (pgrad: excenv_sim_ahead_vjp_params). V = 1 at B = 1 and 257 for every model; every wide form
    at B = V * 326, K = 7 (helpers_vjp.WIDE_CASES / helpers_vjp_params.PGRAD_WIDE_CASES); env-major actions with a workspace of
    exactly the reported bytes; the tank under "ahead" with an RK solver, whose workspace also holds the raw levels
    (excenv_sim_ahead_vjp_workspace_bytes_for); one cotangent group at a time."""
    from helpers_vjp import CASES, WIDE_CASES
    from helpers_vjp_params import PGRAD_WIDE_CASES

    out = []
    for i, (env_name, deadtime) in enumerate(CASES):
        for elem in (4, 8):
            for B in (1, 257):
                solver = ("euler", "rk4", "tsit5")[(i + elem // 4) % 3]
                out.append(dict(env=env_name, deadtime=deadtime, elem=elem, solver=solver, sem="ahead" if B == 257 else "step", B=B, K=REV_K,
                                sub=1 if env_name == "pmsm" else 3, V=1, a="lane", groups=("obs", "states", "last"), wide=False))
            out.append(dict(env=env_name, deadtime=deadtime, elem=elem, solver="euler", sem="step", B=257, K=REV_K, sub=1, V=1, a="env",
                            groups=("obs", "states", "last"), wide=False))
    for solver in ("rk4", "tsit5"):  # the raw levels in the workspace, lane-major and env-major actions
        for a in ("lane", "env"):
            out.append(dict(env="fluid_tank", deadtime=None, elem=4 if a == "lane" else 8, solver=solver, sem="ahead", B=257, K=REV_K, sub=3,
                            V=1, a=a, groups=("obs", "states", "last"), wide=False))
    for groups in (("obs",), ("states",), ("last",)):
        out.append(dict(env="cartpole", deadtime=None, elem=4, solver="rk4", sem="ahead", B=257, K=REV_K, sub=3, V=1, a="lane", groups=groups,
                        wide=False))
        out.append(dict(env="pmsm", deadtime=1, elem=8, solver="euler", sem="step", B=257, K=REV_K, sub=1, V=1, a="lane", groups=groups,
                        wide=False))
    for env_name, elem, solver, sem in (PGRAD_WIDE_CASES if pgrad else WIDE_CASES):
        V = 16 // elem
        out.append(dict(env=env_name, deadtime=None, elem=elem, solver=solver, sem=sem, B=V * 326, K=REV_K, sub=1 if env_name == "pmsm" else 3,
                        V=V, a="lane", groups=("obs", "states", "last"), wide=True))
    return out


def rev_sim_inputs(c):
    """-> spec, states, actions, (g_obs [B, rows, OW], g_states, g_last) of a reverse trajectory case, in the kernel's number format"""
    import oracle
    from helpers_vjp import cotangents, skewed_spec, vjp_inputs, wide_inputs

    spec = skewed_spec(c["env"], c["deadtime"])
    npdt = np.float32 if c["elem"] == 4 else np.float64
    if c["wide"]:
        V, sub, st, acts = wide_inputs(c["env"], c["elem"], spec)
        assert (V, sub) == (c["V"], c["sub"]) and acts.shape[:2] == (c["B"], c["K"])
    else:
        st, acts = vjp_inputs(c["env"], spec, c["B"], c["K"], seed=REV_SEED, np_dtype=npdt)
    S, A, O, _ = oracle.ENV_DIMS[oracle.ENV_IDS[c["env"]]]
    g = cotangents(np.random.default_rng(REV_SEED + 1), c["B"], c["K"] * c["sub"] + 1, O, S)
    return spec, st, acts, (g[0].astype(npdt), [x.astype(npdt) for x in g[1]], [x.astype(npdt) for x in g[2]])


def rev_id(c):
    return ", ".join(f"{k}={v}" for k, v in c.items() if k not in ("wide",))
