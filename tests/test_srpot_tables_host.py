"""CPU tests (no GPU) of the constants the pair kernels evaluate erfc and exp from: the tables and polynomial coefficients are
parsed out of ``csrc/srpot.h`` / ``csrc/rows_body.h`` and evaluated by Horner's rule with the index and argument arithmetic of
the device code (``erfc_from_table``, ``erfc_from_exp``, ``exp_neg_table2`` -- its constants parsed too, its expressions asserted as
text), float64 for the double forms and float32
arithmetic for the fp32 polynomial, against ``tests/golden/sr_pointwise.npz`` (mpmath, ``make_sr_pointwise_golden.py``).  The
bounds are the figures the comments in ``srpot.h`` state."""

import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-pme_amd", "csrc")
NUM = r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?"


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _macro(src, name):
    """Numbers of a multi-line ``#define name ...`` (continuation lines end in a backslash)."""
    m = re.search(r"#define\s+" + name + r"\b((?:.*\\\n)*.*)\n", src)
    assert m, name
    return np.array([float(t) for t in re.findall(NUM, m.group(1).replace("\\\n", " "))])


def _constant(src, name):
    m = re.search(r"\b" + name + r"\s*=\s*(" + NUM + ")", src)
    assert m, name
    return float(m.group(1))


def _fp32_coefficients(src, func):
    """The nine Horner coefficients in the body of `func` (first ``p = c`` / ``p = c * t + c``, then eight ``p = p * t + c``)."""
    body = src[src.index(func):]
    body = body[: body.index("return") if "return" in body[:1500] else 1500]
    first = re.search(r"p = (" + NUM + r")f(?: \* t \+ (" + NUM + r")f)?;", body)
    assert first, func
    coeff = [g for g in first.groups() if g is not None]
    coeff += re.findall(r"p = p \* t \+ (" + NUM + r")f;", body[first.end():])
    return coeff


def _body(src, signature, length=2500):
    """Text of the function that starts at `signature`."""
    return src[src.index(signature):][:length]


def _fit_constants(src, signature):
    """tlo and the 0.4 of t = 1 / (1 + 0.4 y) as written in the device function at `signature`, and xs, x0 from the expressions it
    states for them."""
    body = _body(src, signature)
    tlo = _constant(body, "tlo")
    assert "xs = 2.0 / (1.0 - tlo), x0 = -(1.0 + tlo) / (1.0 - tlo);" in body
    assert "__builtin_fma(xs, t, x0)" in body
    m = re.search(r"rcp_newton\(1\.0 \+ (" + NUM + r") \* y\)", body)
    assert m, signature
    return tlo, float(m.group(1)), 2.0 / (1.0 - tlo), -(1.0 + tlo) / (1.0 - tlo)


@pytest.fixture(scope="module")
def srpot():
    return _read("srpot.h")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sr_pointwise.npz"))


def test_erfcx_table_layout(srpot):
    """52 rows of 9 coefficients + a zero pad, covering [0, kErfcxEnd) exactly: the row index int(8 y) of the last table point
    is the last row, and the whole-range fit takes over where the table ends."""
    tab = _macro(srpot, "MIPME_ERFCX_TAB")
    n, terms, row = (int(_constant(srpot, k)) for k in ("kErfcxIntervals", "kErfcxTerms", "kErfcxRow"))
    assert (n, terms, row) == (52, 9, 10) and tab.shape == (n * row,)
    assert np.all(tab.reshape(n, row)[:, terms:] == 0.0)
    winv, w, end = (_constant(srpot, k) for k in ("kErfcxWidthInv", "kErfcxWidth", "kErfcxEnd"))
    assert winv * w == 1.0 and n * w == end == 6.5
    assert len(_macro(srpot, "MIPME_ERFC_CHEB")) == int(_constant(srpot, "kErfcChebTerms")) == 21
    assert len(_macro(srpot, "MIPME_EXP2_TAB")) == int(_constant(srpot, "kExp2Tab")) == 64


def test_erfcx_table_against_mpmath(srpot, golden):
    """erfc_from_table's polynomial part: j = int(8 y), u = y - centre_j, Horner in float64: 2.22e-15 relative (the comment above
    the table), at ~2000 points of (0, 6.5) and at every row boundary with its two neighbours."""
    tab = _macro(srpot, "MIPME_ERFCX_TAB").reshape(52, 10)
    y, ref = golden["y"], golden["erfcx"]
    sel = y < _constant(srpot, "kErfcxEnd")
    y, ref = y[sel], ref[sel]
    assert len(y) > 2100
    winv, w, n = _constant(srpot, "kErfcxWidthInv"), _constant(srpot, "kErfcxWidth"), int(_constant(srpot, "kErfcxIntervals"))
    body = _body(srpot, "double erfc_from_table(double y, double e")
    assert "int j = int(y * kErfcxWidthInv);" in body and "j = j < kErfcxIntervals ? j : kErfcxIntervals - 1;" in body
    assert "__builtin_fma(double(j), -kErfcxWidth, y - 0.5 * kErfcxWidth)" in body
    j = np.minimum((y * winv).astype(np.int64), n - 1)
    assert set(j) == set(range(52))
    u = (y - 0.5 * w) - j * w  # fma(j, -w, y - w/2): j w is exact, so this is the same two roundings
    p = tab[j, 8]
    for k in range(7, -1, -1):
        p = p * u + tab[j, k]
    err = np.abs(p - ref) / ref
    print(f"erfcx table: max relative error {err.max():.3e} at y = {y[err.argmax()]!r}")
    for row in range(52):
        assert err[j == row].max() <= 2.22e-15, (row, err[j == row].max())


def _whole_range_fit(c, y, consts):
    tlo, c04, xs, x0 = consts
    t = 1.0 / (1.0 + c04 * y)
    x = xs * t + x0
    p = np.full_like(y, c[-1])
    for k in range(len(c) - 2, -1, -1):
        p = p * x + c[k]
    return t * p


def test_whole_range_fit_against_mpmath(srpot, golden):
    """erfc_from_exp(double): t P20(x) against erfcx on [0, 27]: 2e-15 relative (the comment above MIPME_ERFC_CHEB)."""
    c = _macro(srpot, "MIPME_ERFC_CHEB")
    y, ref = golden["y"], golden["erfcx"]
    assert y.max() == 27.0 and (y > 6.5).sum() >= 90
    consts = _fit_constants(srpot, "double erfc_from_exp(double y, double e, const double* __restrict__ c)")
    # erfc_from_table carries its own copy of the same argument arithmetic for y >= kErfcxEnd
    assert _fit_constants(srpot, "double erfc_from_table(double y, double e") == consts
    err = np.abs(_whole_range_fit(c, y, consts) - ref) / ref
    print(f"whole-range fit: max relative error {err.max():.3e} at y = {y[err.argmax()]!r}")
    assert err.max() <= 2e-15


def test_fp32_polynomial_against_mpmath(srpot, golden):
    """erfc_from_exp(float) in float32 arithmetic: 3.7e-7 relative on [0, 6.5], 2e-5 beyond (evaluated up to y = 9.3, where
    erfc leaves the float32 range).  The reference is moved to the float32 input by erfcx' = 2 y erfcx - 2 / sqrt(pi)."""
    c = [np.float32(t) for t in _fp32_coefficients(srpot, "float erfc_from_exp(float y, float e)")]
    assert len(c) == 9
    y64, ref = golden["y"], golden["erfcx"]
    sel = y64 <= 9.3
    y64, ref = y64[sel], ref[sel]
    y = y64.astype(np.float32)
    ref = ref + (2.0 * y64 * ref - 2.0 / np.sqrt(np.pi)) * (y.astype(np.float64) - y64)
    m = re.search(r"1\.0f / \(1\.0f \+ (" + NUM + r")f \* y\)", _body(srpot, "float erfc_from_exp(float y, float e)", 300))
    assert m
    one, c04 = np.float32(1.0), np.float32(m.group(1))
    t = one / (one + c04 * y)
    p = np.full_like(t, c[0])
    for k in c[1:]:
        p = p * t + k
    got = (t * p).astype(np.float64)
    assert got.dtype == np.float64 and p.dtype == np.float32
    err = np.abs(got - ref) / ref
    lo = y64 <= 6.5
    print(f"fp32 polynomial: max relative error {err[lo].max():.3e} on [0, 6.5], {err[~lo].max():.3e} on (6.5, 9.3]")
    assert err[lo].max() <= 3.7e-7
    assert err[~lo].max() <= 2e-5


def test_exp2_table(srpot):
    """T[j] = 2^(j/64): the correctly rounded double (which is within the ulp the kernel's error budget counts on)."""
    tab = _macro(srpot, "MIPME_EXP2_TAB")
    j = np.arange(64)
    ref = np.exp2(j.astype(np.longdouble) / 64)
    assert np.finfo(np.longdouble).eps < 1e-18
    assert np.all(np.abs(tab.astype(np.longdouble) - ref) <= np.spacing(tab))
    assert np.array_equal(tab, ref.astype(np.float64))


def test_exp_table_reduction(srpot, golden):
    """exp_neg_table2 with its own arithmetic (n = rint(-64 x / ln 2), two-step remainder, T[n & 63], degree-5 Taylor, 2^(n >> 6))
    in float64 against exp(-x) on the golden grid: the 4e-16 its comment states."""
    tab = _macro(srpot, "MIPME_EXP2_TAB")
    x, ref = golden["exp_x"], golden["exp_ref"]
    x, ref = x[x <= 700.0], ref[x <= 700.0]
    body = _body(srpot, "void exp_neg_table2(")
    scale = float(re.search(r"__builtin_rint\(-x \* (" + NUM + r")\)", body).group(1))
    hi = float(re.search(r"__builtin_fma\(nf\[u\], (" + NUM + r"), -x\)", body).group(1))
    lo = float(re.search(r"__builtin_fma\(nf\[u\], (" + NUM + r"), r\[u\]\)", body).group(1))
    assert abs(scale * np.log(2.0) / 64 - 1) < 1e-15 and hi < 0 and lo < 0
    assert "tab[n[u] & (kExp2Tab - 1)]" in body and "n[u] >> 6" in body
    # the Taylor coefficients, in the order the source applies them: q = 1/120, then q = fma(q, r, c)
    taylor = re.findall(r"__builtin_fma\(q\[u\], r\[u\], ([0-9. /]+)\)", body)
    assert re.search(r"q\[u\] = 1\.0 / 120\.0;", body) and taylor == ["1.0 / 24.0", "1.0 / 6.0", "0.5", "1.0", "1.0"], taylor
    n = np.rint(-x * scale)
    r = (n * hi - x) + n * lo
    q = np.full_like(x, 1.0 / 120.0)
    for c in taylor:
        q = q * r + eval(c)  # noqa: S307 (one of the five strings asserted above)
    ni = n.astype(np.int64)
    got = np.ldexp(tab[ni & 63] * q, ni >> 6)
    err = np.abs(got - ref) / ref
    print(f"exp table form: max relative error {err.max():.3e}")
    assert np.abs(r).max() <= np.log(2.0) / 128 * (1 + 1e-9)
    assert len(x) > 700 and err.max() <= 4e-16


def test_fp32_coefficient_copies_are_the_same_text(srpot):
    """The packed fp32 body (fast_rs_eval_pk) and erfc_from_exp_fast carry their own copies of the nine coefficients of
    erfc_from_exp(float): the same digits, character for character."""
    want = _fp32_coefficients(srpot, "float erfc_from_exp(float y, float e)")
    assert len(want) == 9 and len(set(want)) == 9
    assert _fp32_coefficients(srpot, "float erfc_from_exp_fast(float y, float e)") == want
    assert _fp32_coefficients(_read("rows_body.h"), "void fast_rs_eval_pk(") == want
