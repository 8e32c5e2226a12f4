"""Derived columns and bootstrap draws (include/mcx.h): what needs no GPU.  The new entry points are
declared and exported and the header is still C99; the index of a draw is the stated function of (seed, i, N), restated
here with step_ref.philox4x32 and Python integers; the example derive texts build for gfx950 at the edges of the shape
range and a text that does not build comes back with its own line numbers; and every refusal that needs no device names
the argument it refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import step_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "mcpar_amd", "examples")
NEW = ("mcx_samples_derive", "mcx_rows_derive", "mcx_store_destroy", "mcx_store_shape", "mcx_store_copy", "mcx_store_summary",
       "mcx_store_rank_summary", "mcx_store_covariance", "mcx_debug_derive_compile", "mcx_samples_draw", "mcx_store_draw",
       "mcx_debug_draw_indices")
ST_DRAW = 5


def test_new_symbols_are_declared_and_exported():
    import mcpar_amd
    lib = mcpar_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "MCX_DERIVE_LINEAR = 1" in src and "MCX_DERIVE_SOURCE = 2" in src
    assert lib.mcx_abi_version() == 5


def test_header_with_the_additions_is_plain_c99(tmp_path):
    src = tmp_path / "derive_cabi.c"
    src.write_text('#include "mcx.h"\nint main(void){ mcx_derive f = {MCX_DERIVE_LINEAR, 1, 0, 0, 0}; mcx_store *s = 0; int64_t ix[2];\n'
                   ' if (mcx_rows_derive(0, 4, 1, 1, &f, &s) != MCX_ERR_INVALID) return 2;\n'
                   ' if (mcx_debug_draw_indices(1u, 1u, 0u, 2, ix) != MCX_OK || ix[0] != 0 || ix[1] != 0) return 3;\n'
                   ' return mcx_store_destroy(s) == MCX_OK ? 0 : 1; }\n')
    exe = tmp_path / "derive_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def ref_indices(seed, N, first, n):
    out = []
    for i in range(first, first + n):
        w = S.philox4x32(i & 0xffffffff, i >> 32, 0, 0, seed, ST_DRAW)
        r = (int(w[0]) << 32) | int(w[1])
        out.append((r * N) >> 64)
    return np.array(out, np.int64)


@pytest.mark.parametrize("seed, N, first, n", [
    (8675309, 1, 0, 64),                 # one row: every index is 0
    (8675309, 65, 0, 300),
    (8675309, 65536000, 0, 300),         # the rows of the C3 store
    (8675309, 1 << 40, 0, 300),          # a 32-bit high product gets these wrong
    (8675309, 65, (1 << 32) - 2, 4),     # the counter's high word takes part
    (8675309, 1 << 40, (1 << 32) - 2, 4),
    (1, 65536000, 0, 300),               # another seed
])
def test_draw_indices_are_the_stated_rule(seed, N, first, n):
    import mcpar_amd as M
    got = M.debug_draw_indices(seed, N, first, n)
    want = ref_indices(seed, N, first, n)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got[:8], want[:8])
    assert got.min() >= 0 and got.max() < N
    if N == 1:
        assert not got.any()
    if N == 1 << 40:
        assert got.max() >= 1 << 32


def test_two_seeds_and_the_counter_words_differ():
    import mcpar_amd as M
    a, b = M.debug_draw_indices(8675309, 65536000, 0, 300), M.debug_draw_indices(1, 65536000, 0, 300)
    assert not np.array_equal(a, b)
    lo, hi = M.debug_draw_indices(7, 1 << 40, 0, 2), M.debug_draw_indices(7, 1 << 40, 1 << 32, 2)
    assert not np.array_equal(lo, hi)  # draw 2^32 is not draw 0 again
    # first + k is one sequence: the window over 2^32 is the tail of one and the head of the other
    w = M.debug_draw_indices(7, 1 << 40, (1 << 32) - 2, 4)
    assert np.array_equal(w[2:], hi)


def example(name):
    return open(os.path.join(EXAMPLES, name)).read()


@pytest.mark.parametrize("name", ["derive_linear.hip", "derive_contrast.hip"])
@pytest.mark.parametrize("np_, nout", [(2, 1), (16, 3), (40, 17), (256, 256)])
def test_example_texts_build(name, np_, nout):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    assert E.user_source_available(), M.load().mcx_last_error()  # hiprtc cross-compiles: a build machine has it
    assert M.debug_derive_compile(example(name), np_, nout) > 0


def test_a_text_that_does_not_build_reports_its_own_lines():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    assert E.user_source_available(), M.load().mcx_last_error()  # hiprtc cross-compiles: a build machine has it
    text = ("__device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout) "
            "{ out[0] = no_such_thing(); }\n")
    with pytest.raises(M.McxError) as ei:
        M.debug_derive_compile(text, 3, 1)
    assert ei.value.code == 7 and "no_such_thing" in str(ei.value) and "mcx_user_derive:1" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("text, np_, nout, word", [("", 3, 1, "source"), ("x", 3, 0, "nout"), ("x", 3, 257, "nout")])
def test_compile_refusals(text, np_, nout, word):
    import mcpar_amd as M
    with pytest.raises(M.McxError) as ei:
        M.debug_derive_compile(text, np_, nout)
    assert ei.value.code == 1 and word in str(ei.value), str(ei.value)


def test_spec_refusals_need_no_device():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    rows = np.zeros((8, 4), np.float32)  # nsteps = 4, nc = 2, np = 3
    good = M.derive_linear(np.ones((2, 3)), np.zeros(2))
    short = M.derive_linear(np.ones((2, 2)), np.zeros(2))       # npar = 6, nout * (np + 1) = 8
    unknown = E.DeriveSpec(3, 1, np.zeros(4))
    nopar = E.DeriveSpec(E.DERIVE_LINEAR, 2, np.zeros(8))
    nopar.c.par = None
    notext = E.DeriveSpec(E.DERIVE_SOURCE, 2)
    wide = E.DeriveSpec(E.DERIVE_LINEAR, 257, np.zeros(257 * 4))
    for spec, word in ((None, "spec"), (unknown, "kind"), (short, "npar"), (nopar, "par is NULL"), (notext, "source"),
                       (wide, "nout")):
        with pytest.raises(M.McxError) as ei:
            M.derive_rows(rows, 4, 2, spec)
        assert ei.value.code == 1 and word in str(ei.value), (word, str(ei.value))
    with pytest.raises(M.McxError) as ei:  # the range comes after the spec, before the device
        M.derive_rows(rows, 0, 2, good)
    assert ei.value.code == 1 and "nsteps" in str(ei.value)
    h = C.c_void_p()
    assert M.load().mcx_rows_derive(rows.ctypes.data_as(C.POINTER(C.c_float)), 4, 2, 3, C.byref(good.c), None) == 1
    assert b"out" in M.load().mcx_last_error()
    assert M.load().mcx_store_shape(h, None, None, None) == 1 and b"store" in M.load().mcx_last_error()
    assert M.load().mcx_store_destroy(None) == 0
    with pytest.raises(M.McxError) as ei:
        M.debug_draw_indices(1, 0, 0, 1)
    assert ei.value.code == 1
