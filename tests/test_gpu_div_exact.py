"""The short division of the device code (include/fh_elementary.h: fhe_div, fhe_div_nofix) against IEEE division, bit for bit (-m gpu).

numpy's float32 division on the host is the reference.  Every pair lies inside the operand ranges the converted sites claim -- read from the sources, so a new site or
a wider claim widens what is tested: |a| in {0} u [2^ALO, 2^AHI], |b| in [2^BLO, 2^BHI] (fredholm_amd/csrc/fh_vec.h: div_r, div_r_nofix, normalize_r).  Pairs outside every
claim are not part of the claim and are not asserted.  No mismatch is allowed.
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from fredholm_amd import native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _claims():
    """(ALO, AHI, BLO, BHI, nofix) of every converted site, from the sources"""
    out = []
    for f in sorted(glob.glob(os.path.join(ROOT, "fredholm_amd", "csrc", "*"))):
        if not f.endswith((".h", ".hip", ".inc")):
            continue
        text = open(f).read()
        for m in re.finditer(r"\bdiv_r(_nofix)?<\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*>", text):
            out.append((int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), bool(m.group(1))))
        for m in re.finditer(r"\bnormalize_r<\s*(-?\d+)\s*,\s*(-?\d+)\s*>\s*\(", text):  # 1 / length
            out.append((0, 0, int(m.group(1)), int(m.group(2)), False))
    return sorted(set(out))


CLAIMS = _claims()
# the box that holds every claim; it satisfies fhe_div's conditions as a whole (asserted below), so every pair in it is inside the theorem, and every site's claim inside it
ALO, AHI = min(c[0] for c in CLAIMS), max(c[1] for c in CLAIMS)
BLO, BHI = min(c[2] for c in CLAIMS), max(c[3] for c in CLAIMS)


def _div(renderer, a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and a.ndim == 1
    fix, nofix = np.empty_like(a), np.empty_like(a)
    N.check(renderer._ctx, N.lib().fh_kat_div(renderer._ctx, C.c_uint32(a.size), N.ptr(a), N.ptr(b), N.ptr(fix), N.ptr(nofix)), "fh_kat_div")
    return fix, nofix


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _mismatches(got, want):
    return np.flatnonzero(~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))


def _report(name, a, b, got, want):
    bad = _mismatches(got, want)
    msg = f"{name}: {bad.size} of {a.size} differ from IEEE"
    for i in bad[:8]:
        msg += f"\n  a = {float(a[i]).hex()} b = {float(b[i]).hex()}: got {float(got[i]).hex()}, IEEE {float(want[i]).hex()}"
    print(f"{name}: {a.size} pairs, {bad.size} mismatches")
    return bad.size, msg


def _pow2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e, np.int32)).astype(np.float32)


def _random_in_box(rng, n, elo, ehi, mant=None):
    """floats of random sign with exponents uniform in [elo, ehi) and random mantissas (the value 2^ehi itself is an edge case, below)"""
    e = rng.integers(elo + 127, ehi + 127, size=n, dtype=np.uint32)
    m = rng.integers(0, 1 << 23, size=n, dtype=np.uint32) if mant is None else mant.astype(np.uint32)
    s = rng.integers(0, 2, size=n, dtype=np.uint32)
    return ((s << 31) | (e << 23) | m).view(np.float32)


def test_the_claims_are_read_and_their_box_is_inside_the_conditions():
    assert len(CLAIMS) >= 8, CLAIMS
    assert any(c[4] for c in CLAIMS) and any(not c[4] for c in CLAIMS)
    # include/fh_elementary.h: 2^-126 <= |b| <= 2^126, |a| >= 2^-100, 2^-125 <= |a / b| < 2^127
    assert BLO >= -126 and BHI <= 126 and ALO >= -100 and ALO - BHI >= -125 and AHI - BLO <= 126, (ALO, AHI, BLO, BHI)


def test_random_pairs_across_the_widest_claimed_range(renderer):
    rng = np.random.default_rng(11)
    n = 1 << 24
    a = _random_in_box(rng, n, ALO, AHI)
    b = _random_in_box(rng, n, BLO, BHI)
    fix, nofix = _div(renderer, a, b)
    want = a / b
    n1, m1 = _report("fhe_div, random pairs", a, b, fix, want)
    n2, m2 = _report("fhe_div_nofix, random pairs", a, b, nofix, want)
    assert n1 == 0 and n2 == 0, m1 + "\n" + m2


def test_quotients_next_to_rounding_midpoints(renderer):
    """For 2^16 divisors -- random mantissas, all ones, all zeros, 0x7fffff - 1, 0x000000 + 1 and their neighbours -- and 16 quotients each: the numerators b x m rounded
    down and up, m the midpoint above a float q (with q's mantissa random, all ones or all zeros).  a / b then lies within a fraction of an ulp either side of m: the pairs
    a wrong final correction rounds the wrong way.  b x m has 24 + 25 bits: exact in float64."""
    rng = np.random.default_rng(12)
    nb, nq = 1 << 16, 16
    mant = rng.integers(0, 1 << 23, size=nb, dtype=np.uint32)
    special = np.array([0x7fffff, 0x000000, 0x7ffffe, 0x000001, 0x7ffffd, 0x000002, 0x400000, 0x3fffff, 0x400001], np.uint32)
    mant[: nb // 2] = special[np.arange(nb // 2) % special.size]
    b = np.repeat(_random_in_box(rng, nb, BLO, BHI, mant), nq)
    qm = rng.integers(0, 1 << 23, size=nb * nq, dtype=np.uint32)
    qm[0::4] = 0x7fffff
    qm[1::4] = 0
    # the quotient's exponent keeps the numerator inside [2^ALO, 2^AHI): eq + eb + 2 <= AHI, eq + eb >= ALO
    eb = np.frexp(np.abs(b))[1].astype(np.int64) - 1
    lo, hi = np.maximum(ALO - eb, -120), np.minimum(AHI - 2 - eb, 120)
    assert (lo <= hi).all()
    eq = (lo + (rng.integers(0, 1 << 30, size=b.size) % (hi - lo + 1))).astype(np.int64)
    q = (((eq + 127).astype(np.uint32) << 23) | qm).view(np.float32)
    mid = q.astype(np.float64) + np.ldexp(1.0, (eq - 24).astype(np.int32))  # q + half an ulp
    prod = mid * np.abs(b).astype(np.float64)                               # exact
    near = prod.astype(np.float32)
    down = np.where(near.astype(np.float64) > prod, np.nextafter(near, np.float32(0)), near)
    up = np.nextafter(down, np.float32(np.inf))
    a = np.concatenate([down, up, np.nextafter(down, np.float32(0)), np.nextafter(up, np.float32(np.inf))]).astype(np.float32)
    bb = np.concatenate([b, b, b, b])
    a = np.where(rng.integers(0, 2, size=a.size) == 1, -a, a).astype(np.float32)
    inside = (np.abs(a) >= _pow2(ALO)) & (np.abs(a) <= _pow2(AHI))
    a, bb = a[inside], bb[inside]
    assert a.size > 3 * nb * nq
    fix, nofix = _div(renderer, a, bb)
    want = a / bb
    n1, m1 = _report("fhe_div, next to midpoints", a, bb, fix, want)
    n2, m2 = _report("fhe_div_nofix, next to midpoints", a, bb, nofix, want)
    assert n1 == 0 and n2 == 0, m1 + "\n" + m2


def test_powers_of_two_and_the_edges_of_every_claim(renderer):
    av, bv = [], []
    # every pair of powers of two in the box
    ea, eb = np.meshgrid(np.arange(ALO, AHI + 1), np.arange(BLO, BHI + 1), indexing="ij")
    av.append(_pow2(ea.ravel())); bv.append(_pow2(eb.ravel()))
    one_in = lambda x, towards: np.nextafter(np.float32(x), np.float32(towards))
    for alo, ahi, blo, bhi, _ in CLAIMS:
        a_edge = [_pow2(alo), one_in(_pow2(alo), np.inf), _pow2(ahi), one_in(_pow2(ahi), 0)]
        b_edge = [_pow2(blo), one_in(_pow2(blo), np.inf), _pow2(bhi), one_in(_pow2(bhi), 0)]
        mid_a, mid_b = np.float32(1.5) * _pow2((alo + ahi) // 2), np.float32(1.25) * _pow2((blo + bhi) // 2)
        for x in a_edge + [mid_a]:
            for y in b_edge + [mid_b]:
                for sx in (1, -1):
                    for sy in (1, -1):
                        av.append(np.array([sx * x], np.float32)); bv.append(np.array([sy * y], np.float32))
    a, b = np.concatenate(av).astype(np.float32), np.concatenate(bv).astype(np.float32)
    fix, nofix = _div(renderer, a, b)
    want = a / b
    n1, m1 = _report("fhe_div, powers of two and edges", a, b, fix, want)
    n2, m2 = _report("fhe_div_nofix, powers of two and edges", a, b, nofix, want)
    assert n1 == 0 and n2 == 0, m1 + "\n" + m2


def test_zeros_infinities_and_nan(renderer):
    """Ending (a): the fix-up answers what is not a finite non-zero number as IEEE does, a numerator of -0 included.  Ending (b) claims +0 over a divisor in range only."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    special = [np.float32(0.0), np.float32(-0.0), inf, -inf, nan]
    ordinary = [np.float32(1.0), np.float32(-3.0), _pow2(ALO), -_pow2(AHI), _pow2(BLO), -_pow2(BHI), np.float32(0.1), np.float32(-1e-20)]
    pairs = [(x, y) for x in special for y in special + ordinary] + [(x, y) for x in ordinary for y in special]
    a = np.array([p[0] for p in pairs], np.float32)
    b = np.array([p[1] for p in pairs], np.float32)
    fix, _ = _div(renderer, a, b)
    with np.errstate(all="ignore"):
        want = a / b
    n1, m1 = _report("fhe_div, special operands", a, b, fix, want)
    assert n1 == 0, m1
    bz = np.concatenate([_random_in_box(np.random.default_rng(13), 4096, BLO, BHI), _pow2([BLO, BHI]), -_pow2([BLO, BHI])]).astype(np.float32)
    az = np.zeros_like(bz)
    fix, nofix = _div(renderer, az, bz)
    n2, m2 = _report("fhe_div_nofix, +0 numerator", az, bz, nofix, az / bz)
    n3, m3 = _report("fhe_div, +0 numerator", az, bz, fix, az / bz)
    assert n2 == 0 and n3 == 0, m2 + "\n" + m3
