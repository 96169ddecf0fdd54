"""Guard bands around every buffer of excenv_row_moments and excenv_episode_stats (helpers_guard): the C entries straight through ctypes,
every buffer of a call carved from one pattern-filled allocation. B = 1 and 326, N or K = 1 and 7, both element types, the byte arrays
at offsets 4, 2 and 1, with and without each optional pointer: the guards are untouched, the inputs are unchanged, every element of the
outputs is written, the outputs equal those of the same call on ordinary tensors bit for bit (and the twin where it is exact), and
outputs filled with NaN beforehand give the same bits (nothing is read before it is written). B == 0 and N == 0 write nothing."""
import numpy as np
import pytest
import torch

import helpers_policy as hp
import helpers_rollout_stats as hrs
from helpers_guard import Carved, Plain, arena_bytes

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _lane(x, t):
    """[B, N(, C)] -> [N(, C), B] contiguous"""
    x = np.asarray(x)
    return np.ascontiguousarray(np.moveaxis(x, 0, -1)).astype(t)


def _raw_moments(case, dtype, alloc, B, N, C, with_mask, with_shift, max_groups, out_fill=None, launch=(None, None)):
    """excenv_row_moments on buffers from `alloc` (helpers_guard.Plain / Carved) -> stats [1 + 2 C]. launch: the (B, N) the entry is
    called with, where it is not the buffers' (a call that must write nothing)"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    alloc("x", (N, C, B), dtype, "x", fill=_lane(case["x"], npdt))
    if with_mask:
        alloc("mask", (N, B), torch.uint8, "mask", fill=_lane(case["mask"], np.uint8))
    if with_shift:
        alloc("shift", (C,), torch.float64, "shift", fill=np.asarray(case["shift"], np.float64))
    stats = alloc("stats", (1 + 2 * C,), torch.float64, "stats")
    nbytes = hrs.moments_workspace_bytes(B, N, C, max_groups)
    work = alloc("workspace", (nbytes // 8,), torch.float64, "workspace", role="scratch")
    if out_fill is not None:
        stats.fill_(out_fill)
        work.fill_(out_fill)
    alloc.ready()
    Bc, Nc = (B if launch[0] is None else launch[0]), (N if launch[1] is None else launch[1])
    hrs.raw_moments(dtype, Bc, Nc, C, alloc.addr("x"), alloc.addr("mask") if with_mask else None, alloc.addr("shift") if with_shift else None,
                    max_groups, alloc.addr("stats"), alloc.addr("workspace"), nbytes)
    torch.cuda.synchronize()
    return stats


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B", [hp.B_MAIN, 1])
def test_row_moments_writes_its_sums_and_nothing_else(B, dtype):
    elem = 4 if dtype == torch.float32 else 8
    name = "float32" if elem == 4 else "float64"
    n = 0
    for N in (1, hp.K_MAIN):
        for v, (C, with_mask, with_shift, mg) in enumerate(((5, True, True, 0), (1, False, True, 1), (2, True, False, 3), (16, False, False, 0))):
            case = hrs.moments_case(B, N, C, name)
            plain = Plain()
            ref = _raw_moments(case, dtype, plain, B, N, C, with_mask, with_shift, mg)
            twin = hrs.moments_twin(case["x"], case["mask"] if with_mask else None, case["shift"] if with_shift else None)
            assert float(ref[0]) == twin["n"] and bool(torch.isfinite(ref).all())
            for place in ({}, {"mask": 4, "x": 16}, {"mask": 2, "x": elem}, {"mask": 1, "stats": 8, "workspace": 8}, {"shift": 8, "x": 48}):
                carved = Carved(arena_bytes(plain.sizes), place)
                got = _raw_moments(case, dtype, carved, B, N, C, with_mask, with_shift, mg)
                carved.arena.check()
                assert torch.equal(ref, got), (B, N, v, place)
                n += 1
            # nothing of the outputs is read: NaN in them beforehand, the same bits
            again = _raw_moments(case, dtype, Plain(), B, N, C, with_mask, with_shift, mg, out_fill=NAN)
            assert torch.equal(ref, again), (B, N, v)
        # B == 0 and N == 0: EXCENV_OK, nothing written
        case = hrs.moments_case(B, N, 2, name)
        plain = Plain()
        _raw_moments(case, dtype, plain, B, N, 2, True, True, 0)
        for launch in ((0, None), (None, 0)):
            carved = Carved(arena_bytes(plain.sizes), {"mask": 1})
            _raw_moments(case, dtype, carved, B, N, 2, True, True, 0, launch=launch)
            carved.arena.check(wrote=False)
            n += 1
    print(f"guard row_moments {dtype} B={B}: {n} carved cases, guards untouched, inputs unchanged, stats written, NaN outputs the same bits, "
          "empty calls write nothing")


def _raw_episodes(case, dtype, alloc, B, K, with_carries, with_completed, with_outs, out_fill=None, launch=(None, None)):
    """excenv_episode_stats on buffers from `alloc` -> (stats [6], completed [K, B] or None, return_out [B] or None, steps_out [B] or None)"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    alloc("reward", (K, B), dtype, "reward", fill=_lane(case["reward"], npdt))
    alloc("reset", (K, B), torch.uint8, "reset", fill=_lane(case["reset"], np.uint8))
    if with_carries:
        alloc("return_in", (B,), torch.float64, "return_in", fill=np.asarray(case["return_in"], np.float64))
        alloc("steps_in", (B,), torch.int32, "steps_in", fill=np.asarray(case["steps_in"], np.int32))
    stats = alloc("stats", (hrs.EPISODE_STATS,), torch.float64, "stats")
    completed = alloc("completed", (K, B), torch.float64, "completed") if with_completed else None
    ret = alloc("return_out", (B,), torch.float64, "return_out") if with_outs else None
    steps = alloc("steps_out", (B,), torch.int32, "steps_out") if with_outs else None
    nbytes = hrs.episode_workspace_bytes(B)
    work = alloc("workspace", (nbytes // 8,), torch.float64, "workspace", role="scratch")
    if out_fill is not None:
        for t in (stats, completed, ret, work):
            if t is not None:
                t.fill_(out_fill)
        if steps is not None:
            steps.fill_(-7)
    alloc.ready()
    addr = lambda name, have=True: alloc.addr(name) if have else None
    Bc, Kc = (B if launch[0] is None else launch[0]), (K if launch[1] is None else launch[1])
    hrs.raw_episodes(dtype, Bc, Kc, addr("reward"), addr("reset"), addr("return_in", with_carries), addr("steps_in", with_carries),
                     addr("completed", with_completed), addr("return_out", with_outs), addr("steps_out", with_outs), addr("stats"),
                     addr("workspace"), nbytes)
    torch.cuda.synchronize()
    return stats, completed, ret, steps


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B", [hp.B_MAIN, 1])
def test_episode_stats_writes_its_outputs_and_nothing_else(B, dtype):
    elem = 4 if dtype == torch.float32 else 8
    name = "float32" if elem == 4 else "float64"
    same = lambda a, b: all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))
    n = 0
    for K in (1, hp.K_MAIN):
        case = hrs.episode_case(B, K, name)
        for v, (with_carries, with_completed, with_outs) in enumerate(((True, True, True), (False, True, True), (True, False, True), (True, True, False),
                                                                       (False, False, False))):
            plain = Plain()
            ref = _raw_episodes(case, dtype, plain, B, K, with_carries, with_completed, with_outs)
            twin = hrs.episode_twin(case["reward"], case["reset"], *((case["return_in"], case["steps_in"]) if with_carries else (None, None)))
            st = ref[0].cpu().numpy()
            assert st[0] == twin["stats"][0] and st[4] == twin["stats"][4] and st[5] == twin["stats"][5]
            if with_completed:
                assert hrs.same_bits(ref[1].t().cpu().numpy(), twin["completed"])
            if with_outs:
                assert hrs.same_bits(ref[2].cpu().numpy(), twin["ret"]) and np.array_equal(ref[3].cpu().numpy(), twin["steps"])
            places = ({}, {"reset": 4, "reward": 16}, {"reset": 2, "reward": elem}, {"reset": 1, "completed": 8, "return_out": 8, "steps_out": 4},
                      {"return_in": 8, "steps_in": 4, "stats": 8, "workspace": 8})
            for place in places:
                carved = Carved(arena_bytes(plain.sizes), place)
                got = _raw_episodes(case, dtype, carved, B, K, with_carries, with_completed, with_outs)
                carved.arena.check()
                assert same(ref, got), (B, K, v, place)
                n += 1
            again = _raw_episodes(case, dtype, Plain(), B, K, with_carries, with_completed, with_outs, out_fill=NAN)
            assert same(ref, again), (B, K, v)
        plain = Plain()
        _raw_episodes(case, dtype, plain, B, K, True, True, True)
        for launch in ((0, None), (None, 0)):
            carved = Carved(arena_bytes(plain.sizes), {"reset": 1})
            _raw_episodes(case, dtype, carved, B, K, True, True, True, launch=launch)
            carved.arena.check(wrote=False)
            n += 1
    print(f"guard episode_stats {dtype} B={B}: {n} carved cases, guards untouched, inputs unchanged, outputs written, NaN outputs the same bits, "
          "empty calls write nothing")
