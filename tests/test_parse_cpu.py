"""One token -> one float: `mcpar_amd/csrc/parse_g.hpp` (the GPU's parse sweep and the host's fallback use the same routine) must
give, for every token of its exact domain, the bits of glibc's strtof in the "C" locale.  Sampled here; `parse_check all`
(every bit pattern through fmt_g6's text and through %.9g, eleven minutes on eight cores) was run when the file was written:
4 294 967 296 values, 0 differences, and 0 floats x -- denormals included -- with fmt(parse(fmt(x))) != fmt(x)."""
import os
import subprocess

import pytest

import parse_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_equals_the_c_library(tmp_path):
    """plain g++, no HIP: the header alone against strtof"""
    exe = str(tmp_path / "parse_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "parse_check.cc")])
    r = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 differences")


def test_the_reference_tokeniser_knows_the_specials():
    for t, b in R.SPECIAL_BITS.items():
        assert R.token_bits(t) == b, t
    assert all(R.status(t) == R.BAD for t in R.REFUSED)
    assert all(R.status(t) == R.NEEDS_HOST for t in R.FOR_HOST)
    assert all(R.status(t) == R.OK for t in R.SPECIALS)


@pytest.mark.parametrize("tokens", [R.SPECIALS, R.REFUSED, R.FOR_HOST, R.random_tokens(20000)],
                         ids=["specials", "refused", "for_host", "random"])
def test_library_tokens_equal_the_reference(tokens):
    """the library's copy of the header, through mcx_debug_parse_token"""
    for t in tokens:
        bits, st = E.debug_parse_token(t)
        assert st == R.status(t), t
        if st != R.BAD:
            assert R.same_bits_but_nan([bits], [R.strtof_bits(t)]), (t, hex(bits))


def test_library_gives_floats_back_from_nine_digits():
    for b in R.float_patterns(20000):
        t = b"%.9g" % float(b.view("float32"))
        bits, st = E.debug_parse_token(t)
        assert st == R.OK and R.same_bits_but_nan([bits], [b]), t


@pytest.mark.parametrize("kw", [dict(ncol=1), dict(ncol=258), dict(ncol=-1), dict(nc=0), dict(skip_lines=-1), dict(piece_bytes=63)])
def test_bad_specs_are_refused_before_a_device_is_asked_for(kw):
    args = dict(nc=1, ncol=2)
    args.update(kw)
    with pytest.raises(McxError) as e:
        E.store_from_text(b"1 2\n", **args)
    assert e.value.code == 1
