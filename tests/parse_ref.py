"""Sample text read back, restated in plain Python: the tokeniser and the rules of include/mcx.h's
mcx_text_store.  A token's value is libc's strtof through ctypes (restype c_float), never np.float32(float(t)), which rounds
twice.  The tests of the library's parser compare with this."""
import ctypes
import re

import numpy as np

_libc = ctypes.CDLL(None)
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]

NUMBER = re.compile(rb"[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?|[nN][aA][nN])")
TOKEN = re.compile(rb"[^ \t\r\n]+")
OK, BAD, NEEDS_HOST = 0, 1, 2
MAX_BYTES, MAX_DIGITS = 40, 19


class ParseError(ValueError):
    """line counts from 1 in the whole text; field (from 1) is None for a line with the wrong number of fields"""

    def __init__(self, msg, line=None, field=None, nfields=None):
        super().__init__(msg)
        self.line, self.field, self.nfields = line, field, nfields


def strtof_bits(tok):
    """the float32 bit pattern of libc's strtof (the interpreter's LC_NUMERIC is "C")"""
    return int(np.float32(_libc.strtof(bytes(tok), None)).view(np.uint32))


def status(tok):
    """OK / BAD / NEEDS_HOST of one token: the grammar, then the exact domain of parse_g.hpp"""
    tok = bytes(tok)
    if not NUMBER.fullmatch(tok):
        return BAD
    mant = re.split(rb"[eE]", tok.lstrip(b"+-"))[0]
    if mant[:1] in b"iInN":
        return OK
    digits = mant.replace(b".", b"").lstrip(b"0")
    return NEEDS_HOST if len(digits) > MAX_DIGITS or len(tok) > MAX_BYTES else OK


def token_bits(tok):
    """the bits of a token of the grammar, None for any other"""
    return strtof_bits(tok) if status(tok) != BAD else None


def lines_of(text):
    """the text's lines without their \\n; a last line without one counts when it holds a byte"""
    lines = bytes(text).split(b"\n")
    return lines[:-1] if lines[-1] == b"" else lines


def parse(text, ncol=0, nc=1, skip_lines=0, max_rows=-1):
    """-> (rows [nrows, ncol] float32 as uint32 bit patterns, ncol, nfallback); ParseError as mcx_text_store refuses"""
    rows, nfallback, lineno = [], 0, skip_lines
    for line in lines_of(text)[skip_lines:]:
        if max_rows >= 0 and len(rows) >= max_rows:
            break
        lineno += 1
        toks = TOKEN.findall(line)
        if not toks:
            continue
        if ncol == 0:
            ncol = len(toks)
            if not 2 <= ncol <= 257:
                raise ParseError("ncol")
        if len(toks) != ncol:
            raise ParseError("line %d: %d fields, expected %d" % (lineno, len(toks), ncol), lineno, None, len(toks))
        bits = []
        for f, t in enumerate(toks):
            s = status(t)
            if s == BAD:
                raise ParseError("line %d, field %d" % (lineno, f + 1), lineno, f + 1)
            nfallback += s == NEEDS_HOST
            bits.append(strtof_bits(t))
        rows.append(bits)
    if not rows or len(rows) % nc:
        raise ParseError("%d rows, nc = %d" % (len(rows), nc))
    return np.array(rows, np.uint32), ncol, nfallback


def npieces(text, piece_bytes, skip_lines=0):
    """the pieces mcx_text_store cuts: each ends behind the last \\n among its first piece_bytes bytes; what is left, once it
    fits, is the last piece.  None when a line does not fit."""
    text = bytes(text)
    o = 0
    for _ in range(skip_lines):
        o = text.index(b"\n", o) + 1
    n = 0
    while o < len(text):
        n += 1
        if len(text) - o <= piece_bytes:
            break
        cut = text.rfind(b"\n", o, o + piece_bytes)
        if cut < 0:
            return None
        o = cut + 1
    return n


def same_bits_but_nan(a, b):
    """uint32 bit patterns equal, a NaN standing for any NaN"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    if a.shape != b.shape:
        return False
    na, nb = (a & 0x7fffffff) > 0x7f800000, (b & 0x7fffffff) > 0x7f800000
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


# ---- token lists the CPU and GPU tests share
SPECIALS = [b"9.99999e+07", b"7.00649e-46", b"7.0065e-46", b"3.40282e+38", b"3.40283e+38", b"1e39", b"-1e39", b"-0", b"0", b".5",
            b"5.", b"+1e+2", b"16777217", b"16777219", b"inf", b"-inf", b"+INF", b"Infinity", b"-iNfInItY", b"nan", b"-NaN", b"+nan",
            b"0e999", b"-0.000e-999", b"1e-99999", b"1e99999", b"1.17549435e-38", b"1.17549e-38", b"1.4013e-45", b"1E0",
            b"0.0000000000000000000000000000000001", b"1234567890123456789", b"0001234567890123456789"]
SPECIAL_BITS = {b"9.99999e+07": 0x4cbebc14, b"7.00649e-46": 0, b"7.0065e-46": 1, b"3.40283e+38": 0x7f800000, b"1e39": 0x7f800000,
                b"-0": 0x80000000, b".5": 0x3f000000, b"5.": 0x40a00000, b"+1e+2": 0x42c80000, b"16777217": 0x4b800000}
REFUSED = [b"0x10", b"1e", b"NA", b"1.2.3", b"--1", b"e5", b"nan(1)", b"+", b"-", b".", b"1e+", b"1e-", b"e", b"1f", b"infinit",
           b"in", b"na", b"+-1", b"1e5.0", b"0x1p3", b"1d5", b"-.e1", b"12345678901234567890x", b"1,5"]
FOR_HOST = [b"12345678901234567890", b"1.2345678901234567890e5", b"00000000000000000000000000000000000000001",
            b"0.000000000000000000000000000000000000001", b"1234567890123456789012345", b"-9.9999999999999999999999999e-30"]


def random_tokens(n, seed=1):
    """tokens of 1-19 digits: a point anywhere, exponents -70 .. 45, both signs, e / E, + exponents, leading zeros"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nd = int(rng.integers(1, 20))
        d = "".join(str(int(c)) for c in rng.integers(0, 10, nd))
        q = int(rng.integers(-70, 46))
        s = ["", "+", "-", "-"][int(rng.integers(0, 4))] + "0" * int(rng.integers(0, 3))
        pt = int(rng.integers(0, nd + 2))
        if pt <= nd:
            s += d[:pt] + "." + d[pt:]
            if nd == pt == 0:
                s += "0"
            q += nd - pt
        else:
            s += d
        if q or rng.integers(0, 2):
            s += "eE"[int(rng.integers(0, 2))] + ("-" if q < 0 else "+" if rng.integers(0, 2) else "") + str(abs(q))
        out.append(s.encode())
    return out


def float_patterns(n, seed=2):
    """n bit patterns over all exponents, denormals, +-0, +-inf and NaN among them"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,
                     0x7fc00000, 0x4cbebc14, 0x3f800000, 0x00000fff, 0x80000fff, 0x4b800000], np.uint32)
    k = min(n, edge.size)
    b[rng.permutation(n)[:k]] = edge[:k]
    return b
