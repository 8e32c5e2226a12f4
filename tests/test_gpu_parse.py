"""Sample text read back on the GPU against tests/parse_ref.py: the plain-Python tokeniser whose values
are libc's strtof.  Everything is compared bit for bit (a NaN stands for any NaN); the texts are written by format_rows (what
MCout::output prints) and at %.9g, which must give the source bits back.  Inputs of at most nine digits must never reach the
host: nfallback == 0 is asserted with every such text, so no case passes by sending its tokens to strtof."""
import ctypes as C
import gc

import numpy as np
import pytest

import parse_ref as R
import mcpar_amd as M
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import TextReport, TextSpec, load

pytestmark = pytest.mark.gpu


def bits_of(rows):
    return np.ascontiguousarray(rows, np.float32).view(np.uint32)


def nine_text(bits, sep=b"  ", eol=b"\n", final=True, blank_every=0):
    """the rows at %.9g: `sep` between fields, `eol` behind a row, a line of blanks every blank_every rows"""
    out = []
    for r, row in enumerate(bits.view(np.float32)):
        if blank_every and r % blank_every == 0:
            out.append(b" \t" + eol)
        out.append(sep.join(b"%.9g" % float(v) for v in row) + eol)
    text = b"".join(out)
    return text if final else text[:len(text) - len(eol)]


def check_text(text, nc, ncol, want_bits=None, **kw):
    """parse_text against parse_ref (and against the source bits); -> (rows, report)"""
    rows, rep = E.parse_text(text, nc, ncol, **kw)
    ref, ref_ncol, ref_fb = R.parse(text, ncol, nc, kw.get("skip_lines", 0), kw.get("max_rows", -1))
    assert rows.shape == ref.shape and rep["ncol"] == ref_ncol and rep["nrows"] == ref.shape[0]
    assert rep["ntokens"] == ref.size and rep["nfallback"] == ref_fb
    assert R.same_bits_but_nan(bits_of(rows), ref)
    if want_bits is not None:
        assert R.same_bits_but_nan(bits_of(rows), want_bits)
    return rows, rep


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("ncol", [2, 3, 17, 257])
@pytest.mark.parametrize("nc", [1, 3, 64])
def test_shapes(nc, ncol, T):
    src = R.float_patterns(T * nc * ncol, seed=[nc, ncol, T]).reshape(T * nc, ncol)
    text = E.format_rows(src.view(np.float32))
    rows, rep = check_text(text, nc, ncol)
    assert rep["nfallback"] == 0 and rep["npieces"] == 1 and rep["nlines"] == T * nc
    assert E.format_rows(rows) == text  # byte for byte
    rows0, rep0 = check_text(text, nc, 0)  # the columns of the first line
    assert rep0["ncol"] == ncol and rows0.tobytes() == rows.tobytes()
    # nine digits give the floats back, whatever separates them
    t9 = nine_text(src, sep=b"\t", eol=b"\r\n", final=False, blank_every=3)
    _, rep9 = check_text(t9, nc, ncol, want_bits=src)
    assert rep9["nfallback"] == 0
    _, rep9 = check_text(nine_text(src, sep=b" "), nc, ncol, want_bits=src)
    assert rep9["nfallback"] == 0


def test_many_rows_same_bytes_and_pieces():
    """70 000 rows of 3: more token starts than a workgroup's tile holds, more workgroups than the scan's 1024 lanes (the wide
    text: 20 blanks between fields), the default piece and many small ones"""
    n = 70000
    src = R.float_patterns(n * 3, seed=70000).reshape(n, 3)
    text = E.format_rows(src.view(np.float32))
    rows, rep = check_text(text, 1, 3)
    assert rep["nfallback"] == 0 and rep["npieces"] == 1 and E.format_rows(rows) == text
    again, _ = E.parse_text(text, 1, 3)
    assert again.tobytes() == rows.tobytes()  # the same text, the same bytes
    small, reps = E.parse_text(text, 1, 3, piece_bytes=65537)
    assert small.tobytes() == rows.tobytes() and reps["npieces"] == R.npieces(text, 65537) > 20
    wide = nine_text(src, sep=b" " * 20)
    assert len(wide) > 1024 * 4096
    wrows, wrep = E.parse_text(wide, 1, 3)
    assert wrep["nfallback"] == 0 and wrep["nrows"] == n and R.same_bits_but_nan(bits_of(wrows), src)


def test_piece_boundaries():
    """pieces that end behind every position of a line: the same bytes as one piece, and as many pieces as the rule says"""
    src = R.float_patterns(40 * 3, seed=40).reshape(40, 3)
    text = E.format_rows(src.view(np.float32))
    longest = max(len(ln) for ln in text.split(b"\n")) + 1
    assert longest <= 64
    one, rep = check_text(text, 2, 3)
    assert rep["npieces"] == 1
    for text_k, final in ((text, True), (text[:-1], False)):
        for pb in range(64, 64 + longest + 3):
            rows, rep = E.parse_text(text_k, 2, 3, piece_bytes=pb)
            assert rows.tobytes() == one.tobytes(), pb
            assert rep["npieces"] == R.npieces(text_k, pb) and rep["nlines"] == 40 and rep["nfallback"] == 0, pb


@pytest.mark.parametrize("nlong", [0, 1, E.TEXT_FALLBACK_CAPACITY + 1])
def test_fallback_counts_and_values(nlong):
    """tokens of 25 digits go to strtof on the host, one by one or -- more than the list holds -- with their whole piece"""
    rng = np.random.default_rng(nlong)
    n = 1100
    toks = [[b"%.6g" % v for v in row] for row in rng.normal(0, 100, (n, 2))]
    for i in rng.permutation(n * 2)[:nlong]:
        toks[i // 2][i % 2] = b"".join(b"%d" % d for d in rng.integers(1, 10, 25)) + b"e-%d" % rng.integers(0, 40)
    text = b"".join(b"  ".join(r) + b"  \n" for r in toks)
    _, rep = check_text(text, 1, 2)
    assert rep["nfallback"] == nlong and rep["npieces"] == 1
    if nlong:
        _, rep = check_text(text, 1, 2, piece_bytes=4096)
        assert rep["nfallback"] == nlong and rep["npieces"] > 1


def test_long_tokens_of_other_kinds():
    text = b"1.5 " + b"0" * 40 + b"2\n-0." + b"0" * 45 + b"3 12345678901234567890\n"
    rows, rep = check_text(text, 1, 2)
    assert rep["nfallback"] == 3 and rows[0, 1] == 2.0


def test_header_trailer_and_file(tmp_path):
    """the reference's drivers: a line before the rows, lines behind them; and the same from a file read in pieces"""
    src = R.float_patterns(30 * 4, seed=30).reshape(30, 4)
    body = E.format_rows(src.view(np.float32))
    text = b"nsamp = 30  nburn = 10\n" + body + b"max likelihood value: -3.2\n1  2  \n"
    rows, rep = check_text(text, 3, 4, skip_lines=1, max_rows=30)
    assert E.format_rows(rows) == body and rep["nfallback"] == 0
    rows0, _ = check_text(text, 3, 0, skip_lines=1, max_rows=30)
    assert rows0.tobytes() == rows.tobytes()
    path = tmp_path / "dump.txt"
    path.write_bytes(text)
    for pb in (0, 64, 101, 1000):
        store, frep = E.store_from_file(path, 3, 4, skip_lines=1, max_rows=30, piece_bytes=pb)
        assert store.shape == (10, 3, 4) and store.rows().tobytes() == rows.tobytes(), pb
        assert frep["nrows"] == 30 and frep["nfallback"] == 0
        store.close()
    with pytest.raises(McxError) as e:
        E.store_from_file(tmp_path / "none.txt", 3)
    assert e.value.code == 1


def refused(text, nc, ncol, **kw):
    """mcx_text_store refuses: -> the message; *out stays NULL, nothing stays allocated"""
    gc.collect()
    before = E.debug_live_resources()
    text = bytes(text)
    spec = TextSpec(ncol, nc, kw.get("skip_lines", 0), kw.get("max_rows", -1), kw.get("piece_bytes", 0))
    h, rep = C.c_void_p(), TextReport()
    rc = load().mcx_text_store(text, len(text), C.byref(spec), C.byref(h), C.byref(rep))
    msg = load().mcx_last_error().decode()
    assert rc == 1 and not h.value, msg
    assert E.debug_live_resources() == before
    return msg


GOOD = [b"1  2  3  ", b"4  5  6  ", b"7  8  9  ", b"10  11  12  "]


def lines(*ls):
    return b"".join(ln + b"\n" for ln in ls)


@pytest.mark.parametrize("name, text, kw", [
    ("short_first", lines(b"1  2  ", *GOOD), {}),
    ("long_first", lines(b"1  2  3  4  ", *GOOD), {}),
    ("short_last", lines(*GOOD, b"1  2  "), {}),
    ("long_last", lines(*GOOD, b"1  2  3  4")[:-1], {}),
    ("two_wrong", lines(GOOD[0], b"1  2  3  4  ", GOOD[1], b"5  ", GOOD[2]), {}),
    ("short_then_long_same_total", lines(b"1  2  ", b"3  4  5  6  ", *GOOD), {}),
    ("wrong_in_a_later_piece", lines(*GOOD * 6, b"1  2  ", *GOOD), dict(piece_bytes=64)),
    ("wrong_behind_skipped_and_empty", lines(b"header", b"", *GOOD, b"  ", b"1 2 3 4", *GOOD), dict(skip_lines=1)),
    ("bad_token", lines(*GOOD, b"1  0x10  3  ", *GOOD), {}),
    ("bad_token_NA", lines(b"1  2  NA"), {}),
    ("bad_before_wrong", lines(GOOD[0], b"1  e5  3  ", b"1  2  "), {}),
    ("wrong_count_before_bad_on_one_line", lines(GOOD[0], b"1  1e  "), {}),
    ("bad_long_token", lines(GOOD[0], b"1  2  12345678901234567890123x  "), {}),
])
def test_errors_name_the_line(name, text, kw):
    with pytest.raises(R.ParseError) as e:
        R.parse(text, 3, 1, kw.get("skip_lines", 0))
    msg = refused(text, 1, 3, **kw)
    assert str(e.value) in msg, (msg, str(e.value))
    assert e.value.line is not None


def test_other_refusals():
    text = lines(*GOOD)
    assert "multiple of nc" in refused(text, 3, 3)
    assert "no rows" in refused(b" \n\n", 1, 3)
    assert "no rows" in refused(b"", 1, 3)
    assert "longer than a piece" in refused(lines(GOOD[0], b" ".join(b"%d" % i for i in range(40)), GOOD[1]), 1, 0, piece_bytes=64)
    assert "first line has 1 fields" in refused(b"1\n2\n", 1, 0)
    with pytest.raises(McxError):
        E.parse_text(text, 1, 3, max_rows=0)
    # capacity_rows too small
    spec, rep = TextSpec(3, 1, 0, -1, 0), TextReport()
    buf = np.zeros((2, 3), np.float32)
    assert load().mcx_text_rows(text, len(text), C.byref(spec), buf.ctypes.data_as(C.POINTER(C.c_float)), 2, C.byref(rep)) == 1
    assert load().mcx_text_rows(text, len(text), C.byref(spec), None, 0, C.byref(rep)) == 0 and rep.nrows == 4


def same(a, b):
    """dicts of arrays, equal with NaN where NaN"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype.kind == "f":
            n = np.isnan(y)
            assert np.array_equal(np.isnan(x), n) and x[~n].tobytes() == y[~n].tobytes(), k
        else:
            assert x.tobytes() == y.tobytes(), k
    return True


def test_store_of_an_engines_text():
    """the analyses of the store read from an engine's own text are those of the rows parse_ref reads from it"""
    d, nc, T = 3, 64, 40
    M.load().mcx_set_device(0)
    pinit = (0.5 * np.sin(0.37 * np.arange(nc * d))).astype(np.float32).reshape(nc, d)
    vl, _keep = M.make_vlfunc(M.VL_GAUSSIAN, d)
    eng = M.Engine(d, nc, pl=1.0)
    eng.run(T, 60, pinit, vl)
    text = eng.samples_text(0, T)
    eng.close()
    ref, ncol, _ = R.parse(text, 0, nc)
    rows = ref.view(np.float32)
    assert ncol == d + 1 and rows.shape == (T * nc, d + 1)
    store, rep = E.store_from_text(text, nc)
    assert store.shape == (T, nc, d + 1) and rep["nfallback"] == 0 and rep["nrows"] == T * nc
    assert store.rows().tobytes() == rows.tobytes()
    assert same(store.summary(), E.rows_summary(rows, T, nc))
    assert same(store.covariance(), E.rows_covariance(rows, T, nc))
    assert same(store.chain_table(), E.rows_chain_table(rows, T, nc))
    assert same(store.step_table(), E.rows_step_table(rows, T, nc))
    store.close()
