"""Guard bands around every buffer of excenv_lqr_backward (helpers_guard): the C entry straight through ctypes, every buffer of a call
carved from one pattern-filled allocation. B = 1 and 326, N = 1 and 7, both element types, the four shapes spread over the variants,
both store_all values, the dense and the time-invariant Jacobian, with and without each optional pointer (Qf, q, r, ff, P0, p0, dV,
n_bad), the buffers at offsets off the 16-byte and the 128-byte boundaries: the guards are untouched, the inputs are unchanged, every
element of the outputs is written, the outputs equal those of the same call on ordinary tensors bit for bit and the twin's, and outputs
filled with NaN beforehand give the same bits (nothing is read before it is written). B == 0 writes nothing; N == 0 writes P0, p0, dV
and n_bad and no gain row."""
import numpy as np
import pytest
import torch

import helpers_lqr as hl
import helpers_policy as hp
from helpers_guard import Carved, Plain, arena_bytes

pytestmark = pytest.mark.gpu
NAN = float("nan")
OPTIONAL = ("Qf", "q", "r", "ff", "P0", "p0", "dV", "n_bad")
# (S, A), store_all, time-invariant, the optional pointers left out
VARIANTS = (((7, 2), 1, False, ()), ((4, 1), 0, False, ("Qf", "q")), ((2, 1), 1, True, ("r", "ff", "dV")), ((1, 1), 0, True, ("P0", "p0", "n_bad")),
            ((7, 2), 0, True, ("q", "r")), ((4, 1), 1, False, OPTIONAL))


def _lane(x, t):
    return np.ascontiguousarray(np.moveaxis(np.asarray(x), 0, -1)).astype(t)


def _raw(case, dtype, alloc, S, A, B, N, store_all, invariant, without, out_fill=None, launch=(None, None)):
    """excenv_lqr_backward on buffers from `alloc` (helpers_guard.Plain / Carved) -> dict of the outputs that were asked for. launch:
    the (B, N) the entry is called with, where it is not the buffers'"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    have = lambda name: name not in without
    F, G = (case["F"][:, -1:], case["G"][:, -1:]) if invariant else (case["F"], case["G"])
    alloc("jac", (F.shape[1], S, S + A, B), dtype, "jac", fill=_lane(np.concatenate([F, G], axis=-1), npdt))
    alloc("Q", (S, S), dtype, "Q", fill=case["Q"].astype(npdt))
    alloc("R", (A, A), dtype, "R", fill=case["R"].astype(npdt))
    if have("Qf"):
        alloc("Qf", (S, S), dtype, "Qf", fill=case["Qf"].astype(npdt))
    if have("q"):
        alloc("q", (N + 1, S, B), dtype, "q", fill=_lane(case["q"], npdt))
    if have("r"):
        alloc("r", (N, A, B), dtype, "r", fill=_lane(case["r"], npdt))
    rows = N if store_all else 1
    shapes = dict(gain=(rows, A, S, B), ff=(rows, A, B), P0=(S, S, B), p0=(S, B), dV=(2, B))
    out = {k: alloc(k, shape, dtype, k) for k, shape in shapes.items() if k == "gain" or have(k)}
    if have("n_bad"):
        out["n_bad"] = alloc("n_bad", (B,), torch.int32, "n_bad")
    if out_fill is not None:
        for k, t in out.items():
            t.fill_(-7 if k == "n_bad" else out_fill)
    alloc.ready()
    addr = lambda name: alloc.addr(name) if (name in ("jac", "Q", "R", "gain") or have(name)) else None
    Bc, Nc = (B if launch[0] is None else launch[0]), (N if launch[1] is None else launch[1])
    hl.raw_lqr(dtype, Bc, Nc, S, A, addr("jac"), 0 if invariant else S * (S + A) * B, addr("Q"), addr("Qf"), addr("R"), addr("q"), addr("r"), 0.125,
               store_all, addr("gain"), addr("ff"), addr("P0"), addr("p0"), addr("dV"), addr("n_bad"))
    torch.cuda.synchronize()
    return out


def _guarded(B, dtype):
    elem = 4 if dtype == torch.float32 else 8
    name = "float32" if elem == 4 else "float64"
    same = lambda a, b: a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    n = 0
    for N in (1, hp.K_MAIN):
        for v, ((S, A), store_all, invariant, without) in enumerate(VARIANTS):
            case = hl.rounded(hl.random_problem(S, A, B, N, seed=40 + v), name)
            plain = Plain()
            ref = _raw(case, dtype, plain, S, A, B, N, store_all, invariant, without)
            have = lambda k: k not in without
            tw = hl.lqr_twin(case["F"][:, -1] if invariant else case["F"], case["G"][:, -1] if invariant else case["G"], case["Q"], case["R"],
                             Qf=case["Qf"] if have("Qf") else None, q=case["q"] if have("q") else None, r=case["r"] if have("r") else None,
                             reg=0.125, dtype=name, n_iter=N if invariant else None).at(N, store_all)
            for k, t in ref.items():
                got = t.cpu().numpy() if k == "n_bad" else np.moveaxis(t.cpu().numpy(), -1, 0)
                assert hl.same_bits(got, tw[k]), (B, N, v, k)
            places = ({}, {"jac": 16, "q": 48, "gain": 16}, {"jac": elem, "q": elem, "r": elem, "gain": elem, "ff": elem, "P0": elem, "p0": elem, "dV": elem},
                      {"Q": elem, "Qf": 64 + elem, "R": 16, "n_bad": 4, "gain": 64}, {"jac": 48, "r": 64, "P0": 48, "p0": 16, "dV": 64, "ff": 48})
            for place in places:
                carved = Carved(arena_bytes(plain.sizes), place)
                got = _raw(case, dtype, carved, S, A, B, N, store_all, invariant, without)
                carved.arena.check()
                assert same(ref, got), (B, N, v, place)
                n += 1
            # nothing of the outputs is read: NaN in them beforehand, the same bits
            again = _raw(case, dtype, Plain(), S, A, B, N, store_all, invariant, without, out_fill=NAN)
            assert same(ref, again), (B, N, v)
        # B == 0: EXCENV_OK, nothing written
        (S, A), case = (4, 1), hl.rounded(hl.random_problem(4, 1, B, N, seed=50), name)
        plain = Plain()
        _raw(case, dtype, plain, S, A, B, N, 1, False, ())
        carved = Carved(arena_bytes(plain.sizes), {"jac": elem})
        _raw(case, dtype, carved, S, A, B, N, 1, False, (), launch=(0, None))
        carved.arena.check(wrote=False)
        # N == 0: P0 = Qf, p0 = q[0], dV = 0, n_bad = 0 are written, gain and ff keep the pattern
        carved = Carved(arena_bytes(plain.sizes), {"q": elem})
        got = _raw(case, dtype, carved, S, A, B, N, 1, False, (), launch=(None, 0))
        problems = carved.arena.problems()
        assert len(problems) == 2 and all("not written" in p and (("'gain'" in p) or ("'ff'" in p)) for p in problems), problems
        assert all(f"{B * N * w} of {B * N * w} elements" in p for p, w in zip(sorted(problems), (1, 4))), problems  # ff: A, gain: A S
        npdt = np.float32 if elem == 4 else np.float64
        sym = np.triu(case["Qf"]) + np.triu(case["Qf"], 1).T
        assert hl.same_bits(np.moveaxis(got["P0"].cpu().numpy(), -1, 0), np.broadcast_to(sym.astype(npdt), (B, S, S)))
        assert hl.same_bits(np.moveaxis(got["p0"].cpu().numpy(), -1, 0), case["q"][:, 0].astype(npdt))
        assert not got["dV"].any() and not got["n_bad"].any()
        n += 2
    print(f"guard lqr_backward {dtype} B={B}: {n} carved cases, guards untouched, inputs unchanged, outputs written, NaN outputs the same bits, "
          "B == 0 writes nothing, N == 0 writes no gain row")


def test_lqr_backward_writes_its_outputs_and_nothing_else():
    for B in (hp.B_MAIN, 1):
        for dtype in (torch.float32, torch.float64):
            _guarded(B, dtype)
