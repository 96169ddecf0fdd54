"""The register / scratch / loop budget of the built kernels for the host tests: tools/loop_code_size.py loaded once, and each of its
two passes over the library's code objects made once, whatever number of tests asks."""
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("loop_code_size", os.path.join(ROOT, "tools", "loop_code_size.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _all_spans():
    return tool().loop_spans(match="")


@functools.lru_cache(maxsize=None)
def _all_resources():
    return tool().kernel_resources()


def spans(match):
    """tool().loop_spans(match=match)"""
    if not os.path.exists(tool().OBJDUMP):
        pytest.skip("llvm-objdump not available")
    return {k: v for k, v in _all_spans().items() if match in k}


def budget(match):
    """-> (resources, spans) of the kernels whose symbol contains `match`: tool().kernel_resources() and tool().loop_spans()"""
    if not (os.path.exists(tool().OBJDUMP) and os.path.exists(tool().READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    return {k: v for k, v in _all_resources().items() if match in k}, spans(match)


def check_budget(res, spans):
    """No scratch memory, at most 256 vector registers, a span for every kernel and the largest loop under 60 KB (the bound of the
    headline test). -> the (symbol, (loop bytes, kernel bytes)) of the largest loop"""
    over = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr"] > 256}
    for k, v in sorted(over.items()):
        print(v, k)
    assert not over, f"{len(over)} of {len(res)} instantiations over budget"
    assert len(spans) == len(res)
    worst = max(spans.items(), key=lambda kv: kv[1][0])
    print("largest loop:", worst, "largest kernel:", max(v[1] for v in spans.values()), "most registers:", max(v["vgpr"] for v in res.values()))
    assert worst[1][0] < 60 * 1024
    return worst
