"""mcx_debug_fill_allocations and mcx_debug_fill_scratch (include/mcx.h; DESIGN.md "Scratch and its history"): the two test
hooks behind tests/test_gpu_scratch_history.py, as far as they go without a GPU.  Both are declared and exported, the ABI
version stays, every refusal is MCX_ERR_INVALID with a message before a device is touched (this machine has none: a call that
went on to one would come back with another status), and the setter hands back its count and goes back to off."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # include/mcx.h MCX_ERR_INVALID
HOOKS = ("mcx_debug_fill_allocations", "mcx_debug_fill_scratch")


@pytest.fixture(autouse=True)
def allocation_fill_off():
    from mcpar_amd import engine as E
    yield
    E.debug_fill_allocations(-1)


def test_declared_exported_and_the_abi_version_stays():
    import mcpar_amd
    lib = mcpar_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", src))
    for name in HOOKS:
        assert name in declared and hasattr(lib, name), name
    assert lib.mcx_abi_version() == 5
    assert re.search(r"#define MCX_ABI_VERSION 5\b", src)
    assert re.search(r"int mcx_debug_fill_allocations\(int byte, unsigned long long \*nfilled\);", src)
    assert re.search(r"int mcx_debug_fill_scratch\(mcx_engine \*e, mcx_store \*s, int byte, size_t bytes\[3\]\);", src)


def last_error():
    import mcpar_amd
    return mcpar_amd.load().mcx_last_error().decode()


# any non-NULL pointer: a refusal reads neither the engine nor the store
FAKE = C.c_void_p(0x1000)


@pytest.mark.parametrize("e, s, byte, word", [
    (None, None, 0, "neither"), (FAKE, FAKE, 0, "both"),
    (FAKE, None, -1, "byte = -1"), (None, FAKE, -1, "byte = -1"), (FAKE, None, 256, "byte = 256"), (None, FAKE, 256, "byte = 256"),
    (None, None, 256, "neither"),  # the owners are looked at first
])
def test_fill_scratch_refusals_touch_no_device(e, s, byte, word):
    import mcpar_amd
    out = (C.c_size_t * 3)(7, 7, 7)
    assert mcpar_amd.load().mcx_debug_fill_scratch(e, s, byte, out) == INVALID
    assert word in last_error(), last_error()
    assert list(out) == [7, 7, 7]  # nothing was reported, because nothing was filled
    assert mcpar_amd.load().mcx_debug_fill_scratch(e, s, byte, None) == INVALID


@pytest.mark.parametrize("byte", [-2, 256, 1 << 20, -(1 << 20)])
def test_fill_allocations_refuses_and_keeps_its_setting(byte):
    import mcpar_amd
    from mcpar_amd import engine as E
    lib = mcpar_amd.load()
    assert E.debug_fill_allocations(0x3C) == 0
    n = C.c_ulonglong(99)
    assert lib.mcx_debug_fill_allocations(byte, C.byref(n)) == INVALID and n.value == 99
    assert "byte = %d" % byte in last_error()
    assert lib.mcx_debug_fill_allocations(byte, None) == INVALID
    with pytest.raises(mcpar_amd.McxError) as ei:
        E.debug_fill_allocations(byte)
    assert ei.value.code == INVALID


def test_setter_returns_the_count_and_goes_back_to_off():
    import mcpar_amd
    from mcpar_amd import engine as E
    lib = mcpar_amd.load()
    before = E.debug_live_resources()
    for byte in (0, 0xFF, 0x3C, -1, 255, -1):  # every value that is taken, NULL and not NULL for the count
        assert lib.mcx_debug_fill_allocations(byte, None) == 0
        assert E.debug_fill_allocations(byte) == 0  # no allocation was made, so none was filled
    assert E.debug_fill_allocations() == 0          # the default argument is off
    assert E.debug_live_resources() == before       # a setting is not a resource
