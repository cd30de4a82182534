"""Integer model of the ODD-POWER window table of the one-lane CRT decrypt (csrc/hensel_ps_bal.hpp, csrc/hensel_ps.hpp; CPU
test, no GPU), on top of the models of tests/test_ps_balanced_model.py and tests/test_ps_window6_model.py:

  * the table holds entry 0 = one and entry j = base^(2j-1), j = 1 .. 2^(w-1): one pair squaring (base^2, the multiplier of
    the chain) and 2^(w-1) - 1 pair products, entry j+1 = entry j (x) base^2;
  * a window of digit d = 2^s * o (o odd) multiplies by entry (o+1)/2 after w - s of its squarings, a zero digit by entry 0
    after all of them; the top window is an ordinary window that starts from `one` and has the bits the exponent leaves it.

Checked: the schedule gives pow(c, e, p^2) for e = p - 1 of the fixture keys and of primes built here whose p - 1 spells the
digits 0, 1, 32, 63 and runs of equal digits, for random c, c = +-1 (mod p^2) and c = n^2 - 1; every window is w squarings and
one product whatever its digit; the values of the new chain (products by a SQUARE) and of products met after fewer than w
squarings stay inside K balanced limbs and their columns inside PsbFits, limb by limb on a sample and on whole integers
throughout; the unsigned forms keep their sixteen-fold headroom; the counts of the policy (csrc/policy.cpp)."""
import functools
import math
import random

import pytest

from test_ps_balanced_model import BIAS, KEYS, LB, R, entry, exit_mp, is_prime, key_setup, limbs, montmul_limbs, num, pair_row
from test_ps_window6_model import BoundLog, decrypt_side, exponentiate, pairsqr_doubled

W = 6
LOW_DIGITS = (32, 0, 0, 1, 63, 63, 63, 2, 48, 0, 31)       # digit 0 upwards of p - 1: s = 5, zeros, 1, a run of 63, s = 1, s = 4


def digits_of(e, bits, w):
    nwin = (bits + w - 1) // w
    return [(e >> (w * i)) & ((1 << w) - 1) for i in range(nwin)]


def schedule(e, bits, w):
    """the kernel's operation list, top window first: ("sqr",) and ("mul", table index); bits: the launch's exponent length"""
    assert e.bit_length() <= bits
    ds = digits_of(e, bits, w)
    ops = []
    for win in range(len(ds) - 1, -1, -1):
        d = ds[win]
        wl = bits - win * w if win == len(ds) - 1 else w       # the top window: what the exponent leaves
        s = (d & -d).bit_length() - 1 if d else 0
        pos, idx = wl - s, ((d >> s) + 1) >> 1
        assert 0 <= pos <= wl and (d == 0) == (idx == 0)
        for i in range(wl + 1):
            if i == pos:
                ops.append(("mul", idx))
            if i < wl:
                ops.append(("sqr",))
    return ops


def odd_table(pmul, one, base, w):
    """entry 0 = one, entry j = base^(2j-1): (the table, base^2)"""
    half = 1 << (w - 1)
    tbl = [one, base]
    sq = pmul(base, base) if half > 1 else None
    for j in range(1, half):
        tbl.append(pmul(tbl[j], sq))
    assert len(tbl) == half + 1
    return tbl, sq


def run_schedule(pmul, one, tbl, ops, watch=None):
    x = one
    for op in ops:
        if op[0] == "sqr":
            x = pmul(x, x)
        else:
            x = pmul(x, tbl[op[1]])
        if watch:
            watch(op, x)
    return x


def counts(bits, w):
    """(pair squarings, pair products) of one exponentiation in the odd-table form"""
    half = 1 << (w - 1)
    nwin = (bits + w - 1) // w
    return (1 if half > 1 else 0) + bits, (half - 1) + nwin


def test_counts_of_the_issue_and_of_the_policy():
    assert counts(1024, 6) == (1025, 202)
    SQR, MUL = 5145, 7278
    cost = {w: s * SQR + m * MUL for w in range(1, 8) for s, m in [counts(1024, w)]}
    assert min(cost, key=cost.get) == 6
    assert cost[6] - (1051 * SQR + 201 * MUL) == -26 * SQR + MUL == -126492
    # 512 and 1536 bits: the squarings do not depend on the width, so the products decide -- 118 / 117 at w = 5 / 6 for 512
    # bits (one product in 3.5 M instructions: the policy asks a wider table to save 0.5 % and stays at 5), 323 / 287 / 283 at
    # w = 5 / 6 / 7 for 1536 bits (6; the seventh bit would save 0.3 %)
    assert [counts(512, w)[1] for w in (5, 6)] == [118, 117]
    assert [counts(1536, w)[1] for w in (5, 6, 7)] == [323, 287, 283]
    assert all(counts(b, w)[0] == b + 1 for b in (512, 1024, 1536) for w in (2, 5, 6, 7))


@pytest.mark.parametrize("w", [1, 2, 3, 5, 6])
def test_every_window_is_w_squarings_and_one_product(w):
    for bits in (w, 6 * w, 6 * w + 1, 7 * w - 1):
        nwin = (bits + w - 1) // w
        top = bits - (nwin - 1) * w
        for d in range(1 << w):
            for dtop in sorted({0, 1, 2, (1 << top) - 1, 1 << (top - 1), (1 << (top - 1)) + 2} & set(range(1 << top))):
                e = (dtop << (w * (nwin - 1))) | (d << w if nwin > 2 else 0) | (d if nwin > 1 else 0)
                if nwin == 1:
                    e = dtop
                ops = schedule(e, bits, w)
                assert sum(o[0] == "sqr" for o in ops) == bits and sum(o[0] == "mul" for o in ops) == nwin
                # window by window: wl squarings and one product, wherever the product stands
                at = 0
                for win in range(nwin - 1, -1, -1):
                    wl = top if win == nwin - 1 else w
                    part = ops[at:at + wl + 1]
                    at += wl + 1
                    assert sum(o[0] == "sqr" for o in part) == wl and sum(o[0] == "mul" for o in part) == 1
                assert at == len(ops)
                # plain integers: the schedule spells the exponent
                tbl, _ = odd_table(lambda x, y: x + y, 0, 1, w)
                assert tbl == [0] + [2 * j - 1 for j in range(1, (1 << (w - 1)) + 1)]
                assert run_schedule(lambda x, y: x + y, 0, tbl, ops) == e


@functools.lru_cache(maxsize=None)
def crafted_prime(bits, seed, low=LOW_DIGITS, top=None, w=W):
    """a prime of `bits` bits, made from a seeded generator, whose p - 1 has the digits `low` at the bottom and, if given, the
    top digit `top` (of the bits the top window has)"""
    rng = random.Random(seed)
    lowv = sum(d << (w * i) for i, d in enumerate(low))
    lb_ = w * len(low)
    nwin = (bits + w - 1) // w
    tb = bits - (nwin - 1) * w
    while True:
        e = rng.getrandbits(bits) | (1 << (bits - 1))
        e = (e >> lb_ << lb_) | lowv
        if top is not None:
            assert top >> (tb - 1) == 1
            e = (e & ((1 << (w * (nwin - 1))) - 1)) | (top << (w * (nwin - 1)))
        if is_prime(e + 1):
            return e + 1


def test_crafted_primes_spell_the_digits_of_the_issue():
    p = crafted_prime(1024, "zero-digits")
    ds = digits_of(p - 1, 1024, W)
    assert tuple(ds[:len(LOW_DIGITS)]) == LOW_DIGITS and {0, 1, 32, 63} <= set(ds)
    assert any(ds[i] == ds[i + 1] == ds[i + 2] for i in range(len(ds) - 2))
    q = crafted_prime(1024, "even-top", low=(2,), top=8)
    assert digits_of(q - 1, 1024, W)[-1] == 8 and q.bit_length() == 1024


def _ciphertexts(n, rng):
    n2 = n * n
    return [1, n2 - 1, n + 1, rng.randrange(n2), pow(rng.randrange(2, n), n, n2) * (1 + n * 12345) % n2]


@pytest.mark.parametrize("name", ["iso", "2037", "2051", "crafted", "even-top", "worst1040", "c2048-tight", "c2048-heavy"])
def test_odd_table_exponentiation_is_pow_and_stays_inside_the_limbs(name):
    if name == "crafted":
        p, q = sorted((crafted_prime(1024, "zero-digits"), crafted_prime(1024, "zero-digits-q")))
    elif name == "even-top":
        p, q = sorted((crafted_prime(1024, "even-top", low=(2,), top=8), crafted_prime(1023, "even-top-q", low=(62, 62), top=0b100)))
    else:
        p, q = sorted(KEYS[name])
    n = p * q
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    shared = max((S.p - 1).bit_length() for S in sides)     # the launch's exponent length: both sides run its window count
    rng = random.Random(name)
    seen = set()
    for c in _ciphertexts(n, rng):
        row = pair_row(c, n, Pn, Rn)
        for S in sides:
            assert c % S.psq in (1, S.psq - 1) or c not in (1, n * n - 1)      # c = +-1 modulo p^2
            base = entry(S, row, *chunking, S.consts)
            tbl, sq = odd_table(S.pmul, S.one, base, W)                        # (S.pmul asserts the K-limb range of every value)
            assert [S.val(t) for t in tbl[1:]] == [pow(c, 2 * j - 1, S.psq) * R % S.psq for j in range(1, 33)]
            assert S.val(sq) == pow(c, 2, S.psq) * R % S.psq
            # base^2 and every product by it (entries 2 .. 32; entry 1 is the wide base itself) below 0.6 p
            assert all(10 * max(abs(v[0]), abs(v[1])) < 6 * S.p for v in [sq] + tbl[2:])
            u = pow(c % S.psq, S.p - 1, S.psq)
            outs = []
            for bits in sorted({(S.p - 1).bit_length(), shared}):
                ops = schedule(S.p - 1, bits, W)
                x = run_schedule(S.pmul, S.one, tbl, ops)
                assert S.val(x) == u * R % S.psq
                assert 100 * max(abs(x[0]), abs(x[1])) < 56 * S.p
                outs.append(exit_mp(S, x, S.hp, seen))
            assert outs == [exponentiate(S, row, chunking, 6, shared)[2]] * len(outs)     # the half-squared form
            assert outs[0] == decrypt_side(S, row, chunking, w=5)[2]                      # the chained 5-bit form
            if math.gcd(c, S.p) == 1:
                assert outs[0] == (u - 1) // S.p * S.hp_canon % S.p
    for S in sides:
        # the entry is the widest value (a below 2.1 p, b below 4.2 p); base^2 and every product by it are below 0.6 p
        assert S.top < 4.5 and BIAS // S.p >= 7, S.top
    assert seen <= {-1, 0}


def test_other_exponents_cover_every_digit_and_position():
    """the schedule is an exponentiation by ANY exponent: every digit value in every window position of a short exponent, and
    all-zero / all-63 / alternating runs of a long one"""
    p, q = sorted(KEYS["iso"])
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    S = sides[0]
    n = p * q
    c = pow(3, n, n * n)
    base = entry(S, pair_row(c, n, Pn, Rn), *chunking, S.consts)
    tbl, _ = odd_table(S.pmul, S.one, base, W)
    used = set()
    for d in range(64):
        for bits, e in ((16, (9 << 12) | (d << 6) | (63 - d)), (12, (d << 6) | d), (6, d), (3, d & 7)):
            used |= set(digits_of(e, bits, W))
            x = run_schedule(S.pmul, S.one, tbl, schedule(e, bits, W))
            assert S.val(x) == pow(c, e, S.psq) * R % S.psq
    assert used == set(range(64))
    for e in (0, (1 << 120) - 1, int("100000" * 20, 2), int("000001" * 20, 2), 1 << 119):
        x = run_schedule(S.pmul, S.one, tbl, schedule(e, 120, W))
        assert S.val(x) == pow(c, e, S.psq) * R % S.psq


class LimbPair:
    """the pair product and the pair squaring limb by limb (psb_pairmul, psb_pairsqr on the doubled operand), every column
    inside PsbFits: 3K products of 2^56 and 2^(LB+6), below 2^63; the results must equal the integer model's"""

    def __init__(self, S):
        self.S = S
        self.log = BoundLog(109)
        self.sym = BoundLog(73)

    def pmul(self, x, y):
        S = self.S
        if x is y or x == y:
            t, w, _, c1, c2 = pairsqr_doubled(limbs(x[0]), limbs(x[1]), S.nl, S.n0inv, log_sym=self.sym, log_ab=self.log)
        else:
            a, b, c, d = (limbs(v) for v in (*x, *y))
            t, qd, c1 = montmul_limbs(a, c, S.nl, S.n0inv, log=self.log)
            w, _, c2 = montmul_limbs(a, d, S.nl, S.n0inv, x2=b, y2=c, qin=qd, log=self.log)
        assert (c1, c2) == (0, 0)                           # nothing leaves the top column: the value fits K balanced limbs
        got = (num(t), num(w))
        assert got == S.pmul(x, y)
        return got


@pytest.mark.parametrize("name", ["worst1040", "iso"])
def test_columns_of_the_new_chain_and_of_an_early_product(name):
    """limb by limb: base^2 from the entry's wide base (a below 2.1 p, b below 4.2 p), the first and the last products of the
    chain -- whose multiplier is a SQUARE, not the base --, and windows whose product comes after 1, 2, ... w squarings (the
    first of them the top window's even digit, on squarings of `one`)"""
    p, q = sorted(KEYS[name])
    n = p * q
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    S = sides[1]                                            # the larger prime: the largest p / R
    L = LimbPair(S)
    for c in (n * n - 1, pow(5, n, n * n)):
        base = entry(S, pair_row(c, n, Pn, Rn), *chunking, S.consts)
        sq = L.pmul(base, base)
        tbl_fast, sq_fast = odd_table(S.pmul, S.one, base, W)
        assert sq == sq_fast
        assert L.pmul(base, sq) == tbl_fast[2] and L.pmul(tbl_fast[2], sq) == tbl_fast[3] and L.pmul(tbl_fast[31], sq) == tbl_fast[32]
        # digits 8 (top window of 4 bits: product first, s = 3), then s = 5 .. 0 and a zero digit
        e = int("1000" + "100000" + "010000" + "001000" + "110100" + "000010" + "111111" + "000000", 2)
        ops = schedule(e, 46, W)
        assert ops[:2] == [("sqr",), ("mul", 1)] and [o[0] for o in ops[-7:]] == ["sqr"] * 6 + ["mul"]
        x = run_schedule(L.pmul, S.one, tbl_fast, ops)
        assert S.val(x) == pow(c, e, S.psq) * R % S.psq
    assert L.log.top < 108 * (1 << 56) + (1 << (LB + 6)) < 1 << 63 and L.sym.top < 73 * (1 << 56)


@pytest.mark.parametrize("bits,Ku,LBu", [(512, 19, 29), (1024, 38, 28), (1536, 56, 28)])
def test_unsigned_forms_keep_their_headroom(bits, Ku, LBu):
    """hensel_decrypt_ps_kernel<38,28>, <56,28>, <19,29>: upper bounds as multiples of P with the worst headroom R = 16 P
    (tests/test_hensel_model.py: redc(T) < T/R + P), pushed through base^2, the chain of products by base^2, and a main loop in
    which the product by the worst entry follows ANY number of squarings.  Everything stays below R = 16 P."""
    F = lambda a, b=1: a / b * (1 + 1e-12)
    rho = 16.0
    assert LBu * Ku >= bits + LBu + 4
    pair_l2 = {512: 2 * 19, 1024: 4 * 18, 1536: 8 * 14}[bits]
    chunks = -(-pair_l2 // ((LBu * Ku - 2) // 29))

    def pairmul(x, y):
        (a, b), (c, d) = x, y
        return (F(a * c, rho) + 1, F(a * d + b * c, rho) + 1 + 1e-6)

    z = rho / 4
    a, b = pairmul((z, 0.0), (1.0, 1.0))
    b += F(z * 1.0, rho) + 1
    base = (chunks * a, chunks * b)
    assert max(base) < rho
    sq = pairmul(base, base)                                # the multiplier of the chain: below the base's own bound
    assert max(sq) < rho
    ent = worst = base
    for _ in range(64):
        ent = pairmul(ent, sq)
        worst = (max(worst[0], ent[0]), max(worst[1], ent[1]))
    assert max(worst) < rho
    one = (1.0, 1.0)                                        # the loop starts from `one`, constants below P
    top = worst
    for pos in range(W + 1):                                # the product after `pos` squarings of every window
        s = one
        for _ in range(60):
            for i in range(W + 1):
                if i == pos:
                    s = pairmul(s, worst)
                    top = (max(top[0], s[0]), max(top[1], s[1]))
                if i < W:
                    s = pairmul(s, s)
                    top = (max(top[0], s[0]), max(top[1], s[1]))
    assert max(top) < rho
    assert 3 * Ku * (1 << (2 * LBu)) < 1 << 64
