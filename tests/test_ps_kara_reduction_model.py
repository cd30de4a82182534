"""Integer model of the folded reduction of psb_montmul (csrc/hensel_ps_bal.hpp, KRED / PGPU_PSB_KARA_RED; CPU test, no GPU).
From column K on every quotient digit is known, so the q * n terms of columns K .. 2K-2 are the upper part of a plain product
of q = q0 + q1 B^H and n = n0 + n1 B^H: the cross terms of index k = H .. 2H-2 (column k + H) are L'_k + H'_k + M'_k with
    L' = q0 n0,   H' = q1 n1,   M' = (q0 - q1)(n1 - n0),
L'_k the q0 n0 terms the digit-serial column k takes anyway, H'_k the q1 n1 terms column k + 2H takes anyway: 1143 q * n
products instead of 1296.  The kernel folds the reductions whose operand product is in the Karatsuba form (a2 * b of a pair
squaring, a * c of a pair product): L'_k rides in the chain of L_k, H'_k in the chain of Hh_k, the joins deliver both.  That
form is modelled column by column with EVERY accumulator reduced modulo 2^64, and digits, limbs and every finished column are
compared with the schoolbook model of tests/test_ps_balanced_model.py, with the M and M' products before and after the join.
A chain that waits holds at most 17 operand products of 2^57 and 17 q * n terms of 2^56; the M' products are 17 of at most
2^58 = 2^62.1, and beside the 17 operand products dx dy of up to 2^59 a partial sum really does leave the 64-bit range where
they land before the join (asserted); the wraps cancel and the finished column is the schoolbook column, whose bound (PsbFits)
is unchanged.  Where the join lands first (the order of the source) nothing wraps.  The symmetric product of a pair squaring
keeps the schoolbook reduction (the model's pairsqr takes it from the schoolbook model)."""
import random

import pytest

from test_ps_balanced_model import HALF, K, KEYS, LB, ColumnLog, R, Side, bal, is_prime, limbs, montmul_limbs, num, sext
from test_ps_karatsuba_model import M64, Wraps, s64, schoolbook_columns

H = K // 2
FITS = 3 * K * (1 << (2 * (LB - 1))) + (1 << (LB + 6))      # PsbFits: what a finished column may reach
assert FITS < 1 << 63


def folded_montmul(x, y, n, n0inv, qin=None, wraps=None, m_first=False):
    """psb_montmul<K, LB, 1, false, QMODE, false, true, true> column by column, every register 64 bits wide:
    (r limbs, digits q, carry out, the column values as the signed 64-bit numbers the kernel holds).
    m_first: the M and M' products land on the accumulator before the join does"""
    wraps = wraps or Wraps()
    dn = [n[H + j] - n[j] for j in range(H)]
    dx = [x[j] - x[H + j] for j in range(H)]
    dy = [y[H + j] - y[j] for j in range(H)]
    assert all(-(1 << 31) <= v < (1 << 31) for v in dn + dx + dy)                 # int32_t
    lo, hi = {}, {}
    q, dq, r, cols = [], None, [], []
    acc = true = 0                                                    # acc: the register; true: the same sum unreduced

    def add(v):
        nonlocal acc, true
        acc = (acc + v) & M64
        true += v
        wraps.see(true)

    def chain(terms):
        s = 0
        for a, b in terms:
            s = (s + a * b) & M64
        return s

    for col in range(2 * K):
        if col == K:
            dq = [q[j] - q[H + j] for j in range(H)]
            assert all(abs(v) <= 1 << LB for v in dq)
        # ---- q * n straight onto the accumulator
        if col < K:
            for i in range(col):
                if not (col >= H and i < H and col - i < H):
                    add(q[i] * n[col - i])
        elif col < K + H:
            m = col - K
            for i in range(m + 1):
                add(q[H + i] * n[H + m - i])
        # ---- the chains and the joins
        kr = range(max(0, col - H - H + 1), min(col - H, H - 1) + 1)           # i of index k = col - H
        if col <= 2 * H - 2:
            t = [(x[i], y[col - i]) for i in range(max(0, col - H + 1), min(col, H - 1) + 1)]
            if col >= H:
                t += [(q[i], n[col - i]) for i in range(col - H + 1, H)]
            lo[col] = chain(t)
            add(s64(lo[col]))
        if H <= col <= 3 * H - 2:
            k = col - H
            t = [(x[H + i], y[H + k - i]) for i in kr]
            if k >= H:
                t += [(q[H + i], n[H + k - i]) for i in kr]
            hi[k] = chain(t)
            u = s64((lo.pop(k) + hi[k]) & M64)
            if not m_first:
                add(u)
            for i in kr:
                add(dx[i] * dy[k - i])
            if k >= H:
                for i in kr:
                    add(dq[i] * dn[k - i])
            if m_first:
                add(u)
        if 2 * H <= col <= 4 * H - 2:
            add(s64(hi.pop(col - 2 * H)))
        assert len(lo) <= H + 1 and len(hi) <= H + 1
        assert s64(acc) == true, col                                  # the finished column never wraps ...
        v = s64(acc)
        if col < K:
            if qin is not None:
                v += qin[col]
            cols.append(v)
            d = sext((v & 0xFFFFFFFF) * n0inv)
            q.append(d)
            v += d * n[0]
            assert abs(v) <= FITS and v % (1 << LB) == 0               # ... nor leaves the PsbFits range
            v >>= LB
        else:
            assert abs(v) <= FITS
            cols.append(v)
            r.append(sext(v))
            v = (v + HALF) >> LB
        acc, true = v & M64, v
    assert not lo and not hi
    return r, q, s64(acc), cols


def check(x, y, n, n0inv, qin=None, wraps=None):
    """both orders against the schoolbook model; wraps = (join first, products first)"""
    r0, q0, c0 = montmul_limbs(x, y, n, n0inv, qin=qin, log=ColumnLog())
    want = schoolbook_columns(x, y, n, q0, qin=qin)
    for m_first in (False, True):
        r1, q1, c1, cols = folded_montmul(x, y, n, n0inv, qin=qin, wraps=wraps[m_first] if wraps else None, m_first=m_first)
        assert (r1, q1, c1) == (r0, q0, c0)
        assert cols == want
    return r1, q1


def dbl(a):
    return [2 * v for v in a]


P = KEYS["worst1040"][0]
S = Side(P, 0, 0)
N_MAX = [HALF if i else HALF - 1 for i in range(K)]


def n0inv_of(n):
    return (-pow(n[0], -1, 1 << LB)) % (1 << LB)


def wide_dn_modulus(sign):
    """an odd modulus whose halves stand at opposite ends: |dn| = 2^29 - 1, the largest two balanced limbs can differ by"""
    n = [-HALF] * H + [HALF - 1] * H if sign == 1 else [HALF - 1] * H + [-HALF] * H
    n[0] |= 1
    n[K - 1] = 1 << 24                                               # (a positive modulus of 1040 bits)
    return n


# the first primes above / below those moduli (found once by search; checked below)
WIDE_DN_PRIMES = [num(wide_dn_modulus(1)) + 2 * 571, num(wide_dn_modulus(-1)) - 2 * 468]
MODULI = [N_MAX, wide_dn_modulus(1), wide_dn_modulus(-1)] + [limbs(p) for p in WIDE_DN_PRIMES]


def test_counts_and_what_waits():
    """1296 -> 1143 products per reduction; a chain holds 17 + 17 products, the M' products are 17 of 2^58"""
    direct = sum(1 for col in range(K) for i in range(col) if not (col >= H and i < H and col - i < H))
    direct += sum(col - K + 1 for col in range(K, K + H))
    chains = 2 * sum(2 * H - 1 - k for k in range(H, 2 * H - 1))
    mprime = sum(2 * H - 1 - k for k in range(H, 2 * H - 1))
    assert mprime == 153 and direct + chains + mprime + K == 1143 == K * K - 153
    assert (H - 1) * (1 << (2 * LB - 1)) + (H - 1) * (1 << (2 * LB - 2)) < 1 << 63
    assert (H - 1) * (1 << (2 * LB)) < 1 << 63 < (H - 1) * ((1 << (2 * LB)) + (1 << (2 * LB + 1)))


def test_wide_dn_primes_are_primes():
    for p, sign in zip(WIDE_DN_PRIMES, (1, -1)):
        assert is_prime(p) and p.bit_length() <= LB * K - 4
        n = limbs(p)
        assert sum(abs(n[H + j] - n[j]) >= (1 << LB) - 2048 for j in range(H)) >= H - 2


@pytest.mark.parametrize("qmode", [1, 2])
def test_random_operands(qmode):
    rng = random.Random(31 + qmode)
    for n in [S.nl] + MODULI:
        inv = n0inv_of(n)
        for _ in range(3):
            # the limbs of numbers below p / 2 ...
            a, b = (rng.randrange(-P // 2, P // 2) for _ in range(2))
            al, bl = limbs(a), limbs(b)
            if qmode == 2:
                _, qd, _ = montmul_limbs(al, al, n, inv)
                r, _ = check(dbl(al), bl, n, inv, qin=qd)
                if n is S.nl:
                    assert num(r) == S.pmul((a, b), (a, b))[1]
            else:
                r, q = check(al, bl, n, inv)
                if n is S.nl:
                    assert (num(r), num(q)) == S.redc(a * b)
            # ... and random limbs over the whole range
            y = [rng.randrange(-HALF, HALF + 1) for _ in range(K)]
            x = [rng.randrange(-2 * HALF, 2 * HALF + 1) for _ in range(K)]
            qin = [rng.randrange(-HALF, HALF) for _ in range(K)] if qmode == 2 else None
            check(x, y, n, inv, qin=qin)


@pytest.mark.parametrize("name", ["iso", "2051", "worst1040", "c2048-tight", "c2048-heavy"])
def test_values_at_the_settled_size(name):
    """|value| near 0.54 p, both signs: where the window loop's values settle"""
    p = KEYS[name][0]
    side = Side(p, 0, 0)
    for sa in (1, -1):
        for sb in (1, -1):
            a, b = sa * (54 * p // 100), sb * (54 * p // 100 - 12345)
            al, bl = limbs(a), limbs(b)
            _, qd, _ = montmul_limbs(al, al, side.nl, side.n0inv)
            r, _ = check(dbl(al), bl, side.nl, side.n0inv, qin=qd)
            assert num(r) == side.pmul((a, b), (a, b))[1]
            r, q = check(al, bl, side.nl, side.n0inv)
            assert (num(r), num(q)) == side.redc(a * b)


def test_extreme_limbs_wrap_and_the_wraps_cancel():
    """all limbs at +-2^28 (x = 2a: +-2^29) in every sign pattern of the halves, flat and alternating, on the moduli of the
    largest limbs and of the largest |dn|.  Products before the join: a partial sum wraps; join first: none does.  The
    finished column is the schoolbook column throughout (check)"""
    wrapped = 0
    for n in MODULI[:3]:
        inv = n0inv_of(n)
        for s0 in (1, -1):
            for s1 in (1, -1):
                for alt in (False, True):
                    def half(s, mag):
                        return [s * mag * (-1 if alt and i & 1 else 1) for i in range(H)]
                    y = half(s0, HALF) + half(s1, HALF)
                    for t0 in (1, -1):
                        for t1 in (1, -1):
                            x = half(t0, 2 * HALF) + half(t1, 2 * HALF)
                            for qin in (None, [HALF - 1] * K, [-HALF] * K):
                                w = (Wraps(), Wraps())
                                check(x, y, n, inv, qin=qin, wraps=w)
                                assert w[0].count == 0 and w[0].top < 1 << 63
                                if t0 == -t1 and s0 == -s1 and not alt:
                                    assert w[1].count > 0 and w[1].top >= 1 << 63
                                    wrapped += 1
    assert wrapped == 3 * 4 * 3


@pytest.mark.parametrize("mod", range(len(MODULI)))
def test_digit_patterns_q0_equals_minus_q1(mod):
    """operands chosen so that the DIGITS come out as q0 = -q1 at the largest magnitudes (dq = 2 q0 = +-2^29): the single
    product x * 1 with x = -Q n modulo R"""
    n = MODULI[mod]
    inv, nn = n0inv_of(n), num(n)
    one = [1] + [0] * (K - 1)
    for sign in (1, -1):
        for alt in (False, True):
            v = [sign * (HALF - 1) * (-1 if alt and i & 1 else 1) for i in range(H)]
            Q = v + [-u for u in v]
            xl = limbs(bal(-num(Q) * nn))
            _, q = check(xl, one, n, inv)
            assert q == Q and all(abs(Q[j] - Q[H + j]) == (1 << LB) - 2 for j in range(H))
            for qin in ([HALF - 1] * K, [-HALF] * K):                 # QMODE 2: the digits handed in move the product's
                xq = limbs(bal(-num(Q) * nn - num(qin)))
                _, q = check(xq, one, n, inv, qin=qin)
                assert q == Q


def pairsqr(side, al, bl):
    """psb_pairsqr<K, LB, true, true, true>: t = sym(2a, a) with its digits (the same columns as a * a, schoolbook reduction),
    b = (2a * b + q) reduced in the Karatsuba form with the folded reduction, a = t"""
    t, qd, c = montmul_limbs(al, al, side.nl, side.n0inv)
    assert c == 0
    w, _, c, _ = folded_montmul(dbl(al), bl, side.nl, side.n0inv, qin=qd)
    assert c == 0
    return t, w


def pairmul(side, al, bl, cl, dl):
    """psb_pairmul<K, LB, true, true>: t = a * c in the Karatsuba form with the folded reduction and its digits,
    b = (a * d + b * c + q) reduced (two products, schoolbook)"""
    t, qd, c, _ = folded_montmul(al, cl, side.nl, side.n0inv)
    assert c == 0
    w, _, c = montmul_limbs(al, dl, side.nl, side.n0inv, x2=bl, y2=cl, qin=qd)
    assert c == 0
    return t, w


@pytest.mark.parametrize("name", ["iso", "2051", "worst1040"])
def test_pair_squarings_and_pair_product_against_pow(name):
    p = KEYS[name][0]
    side = Side(p, 0, 0)
    rinv = pow(R, -1, side.psq)
    rng = random.Random(name)
    for _ in range(2):
        u, v = rng.randrange(side.psq), rng.randrange(side.psq)
        x, y = (((a, b - p if b >= p // 2 else b)) for a, b in (side.pair(u * R), side.pair(v * R)))
        xl = (limbs(x[0]), limbs(x[1]))
        for _ in range(6):                                            # six squarings and a product, as a window runs them
            xl = pairsqr(side, *xl)
            x = side.pmul(x, x)
            assert (num(xl[0]), num(xl[1])) == x
        xl = pairmul(side, xl[0], xl[1], limbs(y[0]), limbs(y[1]))
        x = side.pmul(x, y)
        assert (num(xl[0]), num(xl[1])) == x
        assert side.val(x) * rinv % side.psq == pow(u, 64, side.psq) * v % side.psq
