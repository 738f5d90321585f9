"""CPU: the surface of the 16-bit streamed paths (csrc/stream_h16.hip) that needs no GPU -- the three entry points are
declared, bound and exported, and the Python wrappers refuse what they must with the right error."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H16_SYMBOLS = ("creid_stream_poslist_h16", "creid_stream_count_h16", "creid_stream_topk_collect_h16")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    import centroids_reid_amd._lib as L
    assert os.path.exists(L.LIB_PATH)
    return L


def _header_params(name):
    txt = open(os.path.join(ROOT, "include", "creid.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, txt, flags=re.S)
    assert m, f"{name} is not declared in include/creid.h"
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", H16_SYMBOLS)
def test_h16_stream_symbols_declared_bound_and_exported(built_lib, name):
    """Declared in the header as the fp32 entry point's arguments with `const void* q, g` and an `int dtype` after D; the
    ctypes table has the same arity with pointers in the pointer slots; the library exports the symbol."""
    params = _header_params(name)
    base = _header_params(name[:-len("_h16")])
    assert len(params) == len(base) + 1
    assert params[0] == "const void* q" and params[1] == "const void* g"
    d = next(i for i, p in enumerate(params) if re.search(r"\bD$", p))
    assert params[d + 1] == "int dtype"
    assert [re.sub(r"^const float\* (q|g)$", r"const void* \1", p) for p in base] == params[:d + 1] + params[d + 2:]
    restype, argtypes = built_lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params)
    for a, p in zip(argtypes, params):
        assert (a is ctypes.c_void_p) == ("*" in p), (name, p, a)
        if "*" not in p and "int64_t" in p:
            assert ctypes.sizeof(a) == 8, (name, p, a)
    assert hasattr(ctypes.CDLL(built_lib.LIB_PATH), name)
    assert built_lib.lib().creid_abi_version() == 1


def test_topk_stream_h16_on_cpu_tensors_needs_gpu(built_lib):
    """16-bit CPU tensors are refused for being on the CPU (the message of the fp32 call), not for their dtype."""
    from centroids_reid_amd import reid_metric as rm
    with pytest.raises(built_lib.CreidError) as e32:
        rm.topk_stream(torch.zeros(4, 8), torch.zeros(16, 8), 2)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(built_lib.CreidError) as e16:
            rm.topk_stream(torch.zeros(4, 8, dtype=dt), torch.zeros(16, 8, dtype=dt), 2)
        assert str(e16.value) == str(e32.value) and "CPU" in str(e16.value)


def test_get_similar_refuses_other_compute_dtypes(built_lib):
    from centroids_reid_amd import inference as inf
    q, g = torch.zeros(2, 8).numpy(), torch.zeros(5, 8).numpy()
    for bad in (torch.int8, torch.float64, "bf16"):
        with pytest.raises(built_lib.CreidError, match="compute_dtype"):
            inf.get_similar(q, ["a", "b"], g, list("cdefg"), topk=2, compute_dtype=bad)


def test_topk_stream_refuses_mixed_dtypes(built_lib):
    """q and g of different dtypes: CreidError naming both, whatever device they are on."""
    from centroids_reid_amd import reid_metric as rm
    for qd, gd in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.float16, torch.float32)):
        with pytest.raises(built_lib.CreidError, match="one dtype"):
            rm.topk_stream(torch.zeros(4, 8, dtype=qd), torch.zeros(16, 8, dtype=gd), 2)
