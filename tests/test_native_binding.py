"""Host-only checks that the Python binding (_native.py) says what include/excenv.h says — prototypes, constants, structure
layouts — and that the host logic in front of every trajectory launch (_trajectory.py: `_route`) decides what it always has.
No kernel is launched here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from exciting_environments_amd import EnvironmentRegistry, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "excenv.h")
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")


def _header_without_comments():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_every_declared_function_has_a_prototype_of_the_declared_length():
    hdr = _header_without_comments()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(excenv_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert {"excenv_step", "excenv_sim_ahead_ws", "excenv_last_error", "excenv_env_dims", "excenv_stream_pattern"} <= set(declared)
    assert set(declared) == set(_native.PROTOTYPES)
    for name, args in declared.items():
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert len(_native.PROTOTYPES[name][1]) == n, name
    lib = _native.lib()
    for name, (restype, argtypes) in _native.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_pointer_arguments_take_full_width_addresses():
    """What the prototypes are for: a bare Python int in a pointer position is a 64-bit address (without argtypes ctypes passes it
    as a C int, and an address whose low 32 bits are zero arrives as NULL). Nothing is gathered for a count of 0: the call returns
    after its argument checks."""
    lib = _native.lib()
    assert lib.excenv_allgather(1 << 40, 0, None, None, 0, None) == 0
    assert lib.excenv_allgather(0, 0, None, None, 0, None) == -2 and b"NULL" in lib.excenv_last_error()
    with pytest.raises(ctypes.ArgumentError):
        lib.excenv_step_bytes(0.5, 0)


def test_mirrored_constants_equal_the_header():
    hdr = _header_without_comments()
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+EXCENV_([A-Z_0-9]+)\s+\(?(-?\d+)\)?", hdr)}
    values.update({m.group(1): int(m.group(2)) for m in re.finditer(r"\bEXCENV_([A-Z_0-9]+)\s*=\s*(-?\d+)", hdr)})
    mirrored = {k: v for k, v in vars(_native).items() if k.isupper() and not k.startswith("_") and type(v) is int}
    assert {"MAX_STATE", "MAX_ACTION", "MAX_STATIC", "MAX_CONTROL", "TILE", "LAYOUT_ENV_MAJOR", "LAYOUT_LANE_MAJOR", "LAYOUT_TILED",
            "SEM_STEP", "SEM_AHEAD", "SEM_AHEAD_ACCUMULATED_T", "F32", "F64", "OPT_NO_FUSED_ACTIONS", "ABI_VERSION"} <= set(mirrored)
    for name, value in mirrored.items():
        assert name in values, f"_native.{name} mirrors nothing in include/excenv.h"
        assert values[name] == value, name
    assert sorted(_native.SEMANTICS.values()) == sorted(v for k, v in values.items() if k.startswith("SEM_"))


def test_structure_layouts_equal_the_host_compilers(tmp_path):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    probes = []
    for cls, ctype in _native.STRUCTS.items():
        probes.append(f'  std::printf("{ctype} %zu\\n", sizeof({ctype}));')
        probes += [f'  std::printf("{ctype}.{f[0]} %zu\\n", offsetof({ctype}, {f[0]}));' for f in cls._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "excenv.h"\nint main() {\n' + "\n".join(probes) + "\n  return 0;\n}\n")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    hdr = _header_without_comments()
    assert set(re.findall(r"\}\s*(excenv_[a-z_]+_t)\s*;", hdr)) - set(re.findall(r"typedef enum.*?\}\s*(excenv_[a-z_]+_t)\s*;", hdr, flags=re.S)) \
        == set(_native.STRUCTS.values())
    for cls, ctype in _native.STRUCTS.items():
        assert ctypes.sizeof(cls) == compiled[ctype], ctype
        for f in cls._fields_:
            assert getattr(cls, f[0]).offset == compiled[f"{ctype}.{f[0]}"], f"{ctype}.{f[0]}"
        # every member of the C structure is mirrored: the fields fill the structure up to its alignment padding
        end = max(getattr(cls, f[0]).offset + getattr(cls, f[0]).size for f in cls._fields_)
        assert compiled[ctype] - end < ctypes.alignment(cls), ctype


# ---- the routing table of _trajectory.py -------------------------------------------------------------------------------------
# Call shape -> (output provider, effective launch options (envs_per_lane, env_major_mode, lds_pad_bytes, flags) or None, workspace
# requested). Pendulum, fp32 (S = 2, OW = 2, A = 1), B > 0 on a HIP device. The expected values were RECORDED from the code before
# `_run_sim_ahead` became one function: its three launch paths were driven over these shapes with the library call
# (`_native.sim_ahead` / `sim_ahead_raw`) and `TrajectoryPlacement.acquire` replaced by recorders (and the device by one that says
# "cuda"), and what they were handed is pasted here. Sizes straddle the shared-allocation limit (32 MiB: 136 bytes per environment at K = 7 with states) and the
# placement limit (1 GiB: 128 bytes per environment for a row-major set). An exception's name stands for the provider of a call
# that is refused.
# spec: (B, K, substeps, trajectory layout, action layout, gym outputs, out=, env_major_fused, env_major_workspace, launch_opts,
#        store_state_trajectory, semantics)
ROUTES = [
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 0, 1, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 1, 0, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 0, 0, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('shared', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('shared', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('shared', None, True)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 0, 1, None, 1, 'ahead'), ('shared', (0, 1, 0, 1), True)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 1, 0, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 0, 0, None, 1, 'ahead'), ('shared', (0, 1, 0, 1), False)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('shared', (2, 0, 0, 0), True)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('shared', (2, 1, 0, 1), True)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 3, 64, 1), True)),
    ((4096, 7, 1, 'lane', 'env', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 1, 64, 1), True)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 1, 1, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 0, 1, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 1, 0, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 0, 0, None, 1, 'ahead'), ('shared', None, False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('shared', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('shared', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'lane', 'tiled', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 0, 1, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), True)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 1, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 0, 0, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), False)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), True)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 1, 0, 0), True)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), True)),
    ((4096, 7, 1, 'env', 'lane', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 1, 64, 0), True)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 0, 1, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), True)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 1, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 0, 0, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), False)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), True)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 1, 0, 0), True)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), True)),
    ((4096, 7, 1, 'env', 'env', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 1, 64, 0), True)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 0, 1, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), True)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 1, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 0, 0, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), False)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), True)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 1, 0, 0), True)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), True)),
    ((4096, 7, 1, 'env', 'tiled', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 1, 64, 0), True)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 0, 1, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 1, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 0, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 0, 1, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), True)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 1, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 0, 0, None, 1, 'ahead'), ('plain', (0, 1, 0, 0), False)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), True)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 1, 0, 0), True)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), True)),
    ((4096, 7, 1, 'tiled', 'env', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 1, 64, 0), True)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 0, 1, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 1, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 0, 0, None, 1, 'ahead'), ('plain', None, False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 1, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 0, 1, (2, 0, 0, 0), 1, 'ahead'), ('plain', (2, 0, 0, 0), False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'tiled', 'tiled', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 3, 64, 1), False)),
    ((246720, 7, 1, 'lane', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('shared', None, False)),
    ((246724, 7, 1, 'lane', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, False)),
    ((8388604, 7, 1, 'lane', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, False)),
    ((8388608, 7, 1, 'lane', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, False)),
    ((8388608, 7, 1, 'lane', 'lane', 0, 0, 1, 1, None, 0, 'ahead'), ('placed', None, False)),
    ((8388608, 7, 1, 'lane', 'lane', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 3, 64, 1), False)),
    ((246720, 7, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((246724, 7, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((8388604, 7, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((8388608, 7, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((8388608, 7, 1, 'lane', 'env', 0, 0, 1, 1, None, 0, 'ahead'), ('placed', None, True)),
    ((8388608, 7, 1, 'lane', 'env', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 1, 64, 1), True)),
    ((246720, 7, 1, 'env', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((246724, 7, 1, 'env', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((8388604, 7, 1, 'env', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((8388608, 7, 1, 'env', 'lane', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((8388608, 7, 1, 'env', 'lane', 0, 0, 1, 1, None, 0, 'ahead'), ('plain', None, True)),
    ((8388608, 7, 1, 'env', 'lane', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 1, 64, 0), True)),
    ((246720, 7, 1, 'env', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((246724, 7, 1, 'env', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((8388604, 7, 1, 'env', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((8388608, 7, 1, 'env', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((8388608, 7, 1, 'env', 'env', 0, 0, 1, 1, None, 0, 'ahead'), ('plain', None, True)),
    ((8388608, 7, 1, 'env', 'env', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 1, 64, 0), True)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, False)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 1, 1, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 3, 64, 1), True)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 0, 1, None, 1, 'ahead'), ('placed', (0, 1, 0, 1), True)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 1, 64, 1), True)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 1, 0, None, 1, 'ahead'), ('placed', None, False)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 1, 0, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 3, 64, 1), False)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 0, 0, None, 1, 'ahead'), ('placed', (0, 1, 0, 1), False)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 0, 0, (0, 3, 64, 1), 1, 'ahead'), ('placed', (0, 1, 64, 1), False)),
    ((1048576, 8, 1, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead_accumulated_t'), ('placed', None, True)),
    ((1048576, 8, 1, 'lane', 'env', 1, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((1048576, 8, 2, 'lane', 'env', 0, 0, 1, 1, None, 1, 'ahead'), ('placed', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 1, 0, 1, 1, None, 1, 'ahead'), ('shared', None, False)),
    ((8388608, 7, 1, 'lane', 'lane', 1, 0, 1, 1, None, 1, 'ahead'), ('placed', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 1, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 3, 64, 1), False)),
    ((4096, 7, 1, 'lane', 'env', 1, 0, 1, 1, None, 1, 'ahead'), ('shared', None, True)),
    ((8388608, 7, 1, 'lane', 'env', 1, 0, 1, 1, None, 1, 'ahead'), ('placed', None, True)),
    ((4096, 7, 1, 'lane', 'env', 1, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('shared', (0, 1, 64, 1), True)),
    ((4096, 7, 1, 'env', 'lane', 1, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((8388608, 7, 1, 'env', 'lane', 1, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((4096, 7, 1, 'env', 'lane', 1, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 1, 64, 0), True)),
    ((4096, 7, 1, 'env', 'env', 1, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((8388608, 7, 1, 'env', 'env', 1, 0, 1, 1, None, 1, 'ahead'), ('plain', None, True)),
    ((4096, 7, 1, 'env', 'env', 1, 0, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('plain', (0, 1, 64, 0), True)),
    ((246720, 7, 1, 'lane', 'lane', 0, 1, 1, 1, None, 1, 'ahead'), ('out', None, False)),
    ((246724, 7, 1, 'lane', 'lane', 0, 1, 1, 1, None, 1, 'ahead'), ('out', None, False)),
    ((4096, 7, 1, 'lane', 'lane', 0, 1, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('out', (0, 3, 64, 1), False)),
    ((246720, 7, 1, 'lane', 'env', 0, 1, 1, 1, None, 1, 'ahead'), ('out', None, True)),
    ((246724, 7, 1, 'lane', 'env', 0, 1, 1, 1, None, 1, 'ahead'), ('out', None, True)),
    ((4096, 7, 1, 'lane', 'env', 0, 1, 0, 1, (0, 3, 64, 1), 1, 'ahead'), ('out', (0, 1, 64, 1), True)),
    ((4096, 7, 1, 'env', 'lane', 0, 1, 1, 1, None, 1, 'ahead'), ('ValueError', None, None)),
    ((4096, 7, 1, 'tiled', 'lane', 0, 1, 1, 1, None, 1, 'ahead'), ('ValueError', None, None)),
    ((4096, 7, 1, 'lane', 'lane', 1, 1, 1, 1, None, 1, 'ahead'), ('ValueError', None, None)),
]
_LAYOUT_NAME = {"lane": "lane_major", "env": "env_major", "tiled": "tiled"}
_LAYOUT_ID = {"lane": _native.LAYOUT_LANE_MAJOR, "env": _native.LAYOUT_ENV_MAJOR, "tiled": _native.LAYOUT_TILED}


@pytest.mark.parametrize("spec, want", ROUTES, ids=[" ".join(map(str, s)).replace(" ", "-") for s, _ in ROUTES])
def test_trajectory_routing_is_what_the_three_former_paths_did(spec, want):
    B, K, sub, traj, act, gym, out, fused, ws, opts, states, sem = spec
    env = EnvironmentRegistry.PENDULUM.make(batch_size=B, device="cpu")
    env.traj_layout, env.env_major_fused, env.env_major_workspace = _LAYOUT_NAME[traj], bool(fused), bool(ws)
    env.store_state_trajectory, env.sim_ahead_semantics = bool(states), sem
    env.launch_opts = None if opts is None else _native.launch_opts(*opts)
    props, _keep = env._props_for(env.env_properties, B)
    aligned = [torch.zeros(16) for _ in range(3)]  # read for their addresses only
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    try:
        t_layout, want_states, o, ws_bytes, provider = env._route(B, K, sub, _LAYOUT_ID[act], bool(gym), bool(out), True, props,
                                                                  aligned[0], aligned[1:])
    except (ValueError, AssertionError) as e:
        assert (type(e).__name__, None, None) == want
        return
    assert t_layout == _LAYOUT_ID[traj] and want_states == bool(states)
    got = (provider, None if o is None else (o.envs_per_lane, o.env_major_mode, o.lds_pad_bytes, o.flags), ws_bytes > 0)
    assert got == want


def test_routing_off_the_gpu_is_one_plain_allocation_per_array():
    """B == 0 or a CPU device: nothing is pooled, shared or placed, out= is refused, and an overridden call carries no flags."""
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4096, device="cpu")
    env.env_major_fused = False
    env.launch_opts = _native.launch_opts(0, 0, 64, _native.OPT_NO_FUSED_ACTIONS)
    props, _keep = env._props_for(env.env_properties, 4096)
    a = [torch.zeros(16) for _ in range(3)]
    for traj in ("lane_major", "env_major", "tiled"):
        env.traj_layout = traj
        _, _, o, _, provider = env._route(4096, 7, 1, _native.LAYOUT_ENV_MAJOR, False, False, False, props, a[0], a[1:])
        assert provider == "plain" and (o.envs_per_lane, o.env_major_mode, o.lds_pad_bytes, o.flags) == (0, 1, 64, 0)
        with pytest.raises(ValueError, match="out="):
            env._route(4096, 7, 1, _native.LAYOUT_ENV_MAJOR, False, True, False, props, a[0], a[1:])
    env.traj_layout = "sideways"
    with pytest.raises(ValueError, match="traj_layout must be"):
        env._route(4096, 7, 1, _native.LAYOUT_ENV_MAJOR, False, False, False, props, a[0], a[1:])
