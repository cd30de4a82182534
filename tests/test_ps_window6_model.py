"""Integer model of two changes to the one-lane CRT decrypt (csrc/hensel_ps_bal.hpp, csrc/hensel_ps.hpp; CPU test, no GPU),
on top of the model of tests/test_ps_balanced_model.py:

  * the pair squaring on a DOUBLED operand: a2 = 2a is formed once, the symmetric product takes a2[i] * a[j] (i < j) straight
    into the column accumulator -- no separate cross sum, no shift -- and the second product is a2 * b instead of a * (2b);
  * the HALF-SQUARED window table, entry 2k = (entry k)^2, entry 2k+1 = entry 2k (x) base, and with it 6-bit windows for the
    1024-bit exponents of the 2048-bit class.

Checked: the doubled squaring is bit-identical (result limbs, digits, carry) with the present one on random operands, on
operands at the main loop's 0.54 p bound and on all-(+-2^28) limbs; the two column bounds of the doubled form; the half-squared
table holds the same residues as the chained one for w = 3, 5, 6; the whole exponentiation at w = 6 is pow(c, p-1, p^2), also
where the top window is partial: 1024 bits leave 4; the 2037-bit fixture key (tests/golden/primes_uneven.json) has primes of 1013
and 1024 bits, which leave 5 and 4; and a key of a 1018- and a 1019-bit prime, made here, leaves 4 and 5."""
import math
import random

import pytest

from test_ps_balanced_model import (HALF, K, KEYS, LB, R, ColumnLog, Side, decrypt_side, entry, exit_mp, is_prime, key_setup,
                                    limbs, montmul_limbs, num, pair_row, sext)

UNIT = 1 << 56                                        # |limb product| <= 2^28 * 2^28


class BoundLog(ColumnLog):
    """every partial column sum below `units` * 2^56 (and inside int64: ColumnLog)"""

    def __init__(self, units):
        super().__init__()
        self.limit = units * UNIT

    def see(self, acc):
        super().see(acc)
        assert abs(acc) < self.limit, "column sum beyond its bound"


def double(a):
    a2 = [2 * v for v in a]
    assert all(-(1 << 31) <= v < (1 << 31) for v in a2), "2a must fit int32_t"
    assert all(abs(v) <= 1 << LB for v in a2)
    return a2


def montsqr_doubled_limbs(a2, a, n, n0inv, log=None):
    """psb_montmul<..., SYM, DBL>: the q*n chain, then a2[i] * a[col-i] for i < col-i onto the SAME accumulator, then the
    diagonal a[col/2]^2; the digits are recorded (QMODE 1)"""
    log = log or ColumnLog()
    q, r, acc = [], [], 0
    for col in range(2 * K):
        lo, hi = (0, col) if col < K else (col - K + 1, K)
        for i in range(lo, hi):
            acc += q[i] * n[col - i]
            log.see(acc)
        for i in range(0 if col < K else col - K + 1, (col + 1) // 2):
            acc += a2[i] * a[col - i]
            log.see(acc)
        if col % 2 == 0:
            acc += a[col // 2] * a[col // 2]
            log.see(acc)
        if col < K:
            d = sext((acc & 0xFFFFFFFF) * n0inv)
            q.append(d)
            acc += d * n[0]
            log.see(acc)
            assert acc % (1 << LB) == 0
            acc >>= LB
        else:
            r.append(sext(acc))
            acc = (acc + HALF) >> LB
    return r, q, acc


def pairsqr_present(a, b, n, n0inv, log=None):
    """psb_pairsqr without the doubled operand: t = a*a with its digits, b = a * (2b) + q"""
    t, q, c1 = montmul_limbs(a, a, n, n0inv, log=log)
    w, _, c2 = montmul_limbs(a, [2 * v for v in b], n, n0inv, qin=q, log=log)
    return t, w, q, c1, c2


def pairsqr_doubled(a, b, n, n0inv, log_sym=None, log_ab=None):
    """... with it: a2 = 2a once, t = sym(a2, a) with its digits, b = a2 * b + q"""
    a2 = double(a)
    t, q, c1 = montsqr_doubled_limbs(a2, a, n, n0inv, log=log_sym)
    w, _, c2 = montmul_limbs(a2, b, n, n0inv, qin=q, log=log_ab)
    return t, w, q, c1, c2


def _side(name):
    p, q = KEYS[name]
    return Side(min(p, q), max(p, q), (p * q).bit_length())


def test_doubled_squaring_is_bit_identical_on_random_and_bound_operands():
    rng = random.Random(6)
    for name in ("iso", "worst1040", "2037"):
        S = _side(name)
        p = S.p
        edge = 54 * p // 100
        vals = [(rng.randrange(-p // 2, p // 2), rng.randrange(-p // 2, p // 2)) for _ in range(6)]
        vals += [(sa * edge, sb * edge) for sa in (1, -1) for sb in (1, -1)]          # the main loop's largest values
        vals += [(0, 0), (1, 0), (-1, 1), (edge, 0), (0, -edge)]
        for a, b in vals:
            la, lb_ = limbs(a), limbs(b)
            want = pairsqr_present(la, lb_, S.nl, S.n0inv)
            got = pairsqr_doubled(la, lb_, S.nl, S.n0inv)
            assert got == want
            assert (num(got[0]), num(got[1]), got[3], got[4]) == S.pmul((a, b), (a, b)) + (0, 0)
        # limbs drawn directly (values that need not fit: the carries out of the top column are compared as well)
        for _ in range(6):
            la = [rng.randrange(-HALF, HALF) for _ in range(K)]
            lb_ = [rng.randrange(-HALF, HALF) for _ in range(K)]
            assert pairsqr_doubled(la, lb_, S.nl, S.n0inv) == pairsqr_present(la, lb_, S.nl, S.n0inv)


def test_doubled_squaring_on_extreme_limbs_and_its_column_bounds():
    """all limbs +-2^28 (so a2 = +-2^29), the largest modulus limbs, digits as they fall.  In units of 2^56: a symmetric column is
    at most 18 cross products of 2^57 (or 17 and the square) and 36 q*n terms, below 73; an a2 * b column 36 products of 2^57 and
    36 q*n terms, 108 -- what the a * (2b) form sums today -- plus the carry and the recorded digit (PsbFits: + 2^(LB+6))"""
    assert 18 * 2 + 1 + 36 <= 73 and 36 * 2 + 36 == 108 and 108 * UNIT + (1 << (LB + 6)) < 1 << 63
    nl = [HALF if i else (HALF - 1) for i in range(K)]
    n0 = (-pow(nl[0], -1, 1 << LB)) % (1 << LB)
    sym, ab = BoundLog(73), BoundLog(109)
    for sa in (1, -1):
        for sb in (1, -1):
            for alt_a in (False, True):
                for alt_b in (False, True):
                    a = [sa * HALF * (-1 if alt_a and i & 1 else 1) for i in range(K)]
                    b = [sb * HALF * (-1 if alt_b and i & 1 else 1) for i in range(K)]
                    got = pairsqr_doubled(a, b, nl, n0, log_sym=sym, log_ab=ab)
                    assert got == pairsqr_present(a, b, nl, n0)
    # (the operand parts alone reach 36 and 72 units on these inputs; whatever sign the q*n chain has, half of that shows)
    assert 18 * UNIT <= sym.top < 73 * UNIT
    assert 36 * UNIT <= ab.top < 108 * UNIT + (1 << (LB + 6))
    # a worst-case modulus of the class with real digits
    S = _side("worst1040")
    for sa in (1, -1):
        a = [sa * HALF] * K
        assert pairsqr_doubled(a, a, S.nl, S.n0inv, log_sym=sym, log_ab=ab) == pairsqr_present(a, a, S.nl, S.n0inv)


def chained_table(S, base, w):
    tbl = [S.one, base]
    for _ in range(2, 1 << w):
        tbl.append(S.pmul(tbl[-1], base))
    return tbl


def half_squared_table(S, base, w):
    """entry 2k = (entry k)^2, entry 2k+1 = entry 2k (x) base: 2^(w-1) - 1 squarings and as many products"""
    tbl = [S.one, base] + [None] * ((1 << w) - 2)
    for k in range(1, 1 << (w - 1)):
        tbl[2 * k] = S.pmul(tbl[k], tbl[k])
        tbl[2 * k + 1] = S.pmul(tbl[2 * k], base)
    return tbl


def window_counts(bits, w):
    """(pair squarings, pair products) of one exponentiation: half-squared table, top digit loaded directly"""
    nwin = (bits + w - 1) // w
    build = (1 << (w - 1)) - 1
    return (nwin - 1) * w + build, (nwin - 1) + build


def test_window_counts_of_the_issue():
    assert window_counts(1024, 6) == (1051, 201) and window_counts(1024, 5) == (1035, 219)
    SQR, MUL = 5260, 7278                                  # profiles/ps_balanced.txt: the loops of hensel_decrypt_psb_kernel
    cost = {w: s * SQR + m * MUL for w in range(1, 8) for s, m in [window_counts(1024, w)]}
    assert min(cost, key=cost.get) == 6
    cost512 = {w: s * SQR + m * MUL for w in range(1, 8) for s, m in [window_counts(512, w)]}
    assert min(cost512, key=cost512.get) == 5


def exponentiate(S, row, chunking, w, exp_bits=None, seen=None):
    """decrypt_side of the parent model with the half-squared table; exp_bits: the launch's window count (the kernel takes
    it from the key, the same for both sides: leading zero windows multiply by entry 0 = one)"""
    pair_l2, pchunks, pchunk_limbs = chunking
    base = entry(S, row, pair_l2, pchunks, pchunk_limbs, S.consts)
    tbl = half_squared_table(S, base, w)
    e = S.p - 1
    bits = exp_bits or e.bit_length()
    assert bits >= e.bit_length()
    nwin = (bits + w - 1) // w
    x = tbl[(e >> (w * (nwin - 1))) & ((1 << w) - 1)]
    for i in range(nwin - 2, -1, -1):
        for _ in range(w):
            x = S.pmul(x, x)
        x = S.pmul(x, tbl[(e >> (w * i)) & ((1 << w) - 1)])
    assert 100 * max(abs(x[0]), abs(x[1])) < 56 * S.p
    return base, x, exit_mp(S, x, S.hp, seen)


@pytest.mark.parametrize("name", ["iso", "2037", "2051"])
def test_half_squared_table_equals_the_chained_one(name):
    p, q = sorted(KEYS[name])
    n = p * q
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    rng = random.Random(len(name))
    for c in (n * n - 1, pow(rng.randrange(2, n), n, n * n)):
        row = pair_row(c, n, Pn, Rn)
        for S in sides:
            base = entry(S, row, *chunking, S.consts)
            for w in (3, 5, 6):
                half, chain = half_squared_table(S, base, w), chained_table(S, base, w)
                assert len(half) == 1 << w and None not in half
                assert [S.val(t) for t in half] == [S.val(t) for t in chain]
                assert [S.val(t) for t in half] == [pow(c, e, S.psq) * R % S.psq for e in range(1 << w)]
            # the squared entries start from the entry's wide values (a < 2.1 p, b < 4.2 p): still far inside K balanced limbs
            assert S.top < 4.5


def _prime_below(bits):
    v = (1 << bits) - 1
    while not is_prime(v):
        v -= 2
    return v


TOP_BITS = {"iso": [1024, 1024], "2037": [1013, 1024], "p1018_1019": [1018, 1019]}


@pytest.mark.parametrize("name", sorted(TOP_BITS))
def test_exponentiation_at_six_bits_with_a_partial_top_window(name):
    p, q = sorted(KEYS[name]) if name in KEYS else (_prime_below(1018), _prime_below(1019))
    n = p * q
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    bits = [(S.p - 1).bit_length() for S in sides]
    assert bits == TOP_BITS[name] and n.bit_length() == (2048 if name == "iso" else 2037)
    assert all(b % 6 in (4, 5) for b in bits)                                  # what is left for the top window
    shared = max(bits)                                                         # the launch's exponent length
    rng = random.Random(p % 977)
    seen = set()
    for c in (1, n + 1, n * n - 1, rng.randrange(n * n), pow(rng.randrange(2, n), n, n * n) * (1 + n * 12345) % (n * n)):
        row = pair_row(c, n, Pn, Rn)
        for S in sides:
            u = pow(c % S.psq, S.p - 1, S.psq)
            outs = []
            for exp_bits in (None, shared, 1024):
                base, x, mp = exponentiate(S, row, chunking, 6, exp_bits, seen)
                assert S.val(x) == u * R % S.psq
                outs.append(mp)
            assert outs == [decrypt_side(S, row, chunking, w=5)[2]] * 3        # the 5-bit chained flow of the parent model
            if math.gcd(c, S.p) == 1:
                assert outs[0] == (u - 1) // S.p * S.hp_canon % S.p
    assert seen <= {-1, 0}
