"""Integer model of the one-lane CRT decrypt on BALANCED limbs (csrc/hensel_ps_bal.hpp; CPU test, no GPU): a prime of the
2048-bit class in K = 36 signed limbs of LB = 29 bits, P = p itself, signed Montgomery digits.  The model follows the
kernel's flow -- entry from the chunks of a pair row, window table, window loop, exit under the prime -- twice: limb by limb
(every column sum checked against the 64-bit accumulator) and on whole integers (the same digits, fast enough for whole
exponentiations); the two are checked against each other.  The plaintext half it yields is compared with
L_p(c^(p-1) mod p^2) * h_p mod p of oracle/paillier_oracle.py (ipcl/pri_key.cpp:128-157)."""
import json
import os
import random

import pytest

from oracle import paillier_oracle as orc

K, LB, RB = 36, 29, 29
HALF = 1 << (LB - 1)
R = 1 << (LB * K)
BIAS = sum(HALF << (LB * i) for i in range(K))        # a value v has K balanced limbs  <=>  -BIAS <= v < R - BIAS
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIT_BITS = LB * K - 4                                 # capi_keys.inc: primes up to 1040 bits


def sext(v):
    v &= (1 << LB) - 1
    return v - (1 << LB) if v >= HALF else v


def limbs(v):
    """K balanced limbs in [-2^28, 2^28) of v (the kernel's result columns: r = sext(acc), carry = (acc + 2^28) >> 29)"""
    assert -BIAS <= v < R - BIAS, "value does not fit K balanced limbs"
    out = []
    for _ in range(K):
        r = sext(v)
        out.append(r)
        v = (v - r) >> LB
    assert v == 0
    return out


def num(ls):
    return sum(x << (LB * i) for i, x in enumerate(ls))


def bal(v):
    """the representative of v mod R that K balanced digits spell"""
    return (v + BIAS) % R - BIAS


class ColumnLog:
    def __init__(self):
        self.top = 0

    def see(self, acc):
        self.top = max(self.top, abs(acc))
        assert -(1 << 63) <= acc < (1 << 63), "column sum leaves the 64-bit accumulator"


def montmul_limbs(x1, y1, n, n0inv, x2=None, y2=None, qin=None, log=None):
    """psb_montmul column by column: (r limbs, digits q).  x2/y2: the second product (NP = 2); qin: QMODE 2"""
    log = log or ColumnLog()
    q, r, acc = [], [], 0
    for col in range(2 * K):
        lo, hi = (0, col) if col < K else (col - K + 1, K)
        for i in range(lo, hi):
            acc += q[i] * n[col - i]                  # i <= col - 1 for col < K; n_0 belongs to the digit step
            log.see(acc)
        lo, hi = (0, col + 1) if col < K else (col - K + 1, K)
        for i in range(lo, hi):
            acc += x1[i] * y1[col - i]
            log.see(acc)
            if x2 is not None:
                acc += x2[i] * y2[col - i]
                log.see(acc)
        if col < K:
            if qin is not None:
                acc += qin[col]
            d = sext((acc & 0xFFFFFFFF) * n0inv)
            q.append(d)
            acc += d * n[0]
            log.see(acc)
            assert acc % (1 << LB) == 0
            acc >>= LB
        else:
            r.append(sext(acc))
            acc = (acc + HALF) >> LB
    return r, q, acc                                  # acc: the carry out of the top column (0 when the result fits)


class Side:
    """one side of a key: the constants of capi_keys.inc (build_hensel_set, balanced variant) as integers"""

    def __init__(self, p, other, n_bits):
        assert p.bit_length() <= FIT_BITS
        self.p, self.psq = p, p * p
        self.n0inv = (-pow(p, -1, 1 << LB)) % (1 << LB)
        self.n0full = (-pow(p, -1, R)) % R
        self.nl = limbs(p)
        self.top = 0.0                                # largest |value| / p seen

    def rng_ok(self, v):
        assert -BIAS <= v < R - BIAS
        self.top = max(self.top, abs(v) * 1000 // self.p / 1000)
        return v

    def redc(self, T):
        """(T + Q p) / R with the digits the kernel finds: Q = the balanced representative of T * (-p^-1) mod R"""
        Q = bal(T * self.n0full)
        assert (T + Q * self.p) % R == 0
        return self.rng_ok((T + Q * self.p) // R), Q

    def pair(self, z):
        """z mod p^2 as (a, b), z == a - p b, both in [0, p) (put_pair of capi_keys.inc: the sign convention and the values
        of the unsigned sets; only the LIMBS of a constant are balanced.  The a of a pair counts exactly, not modulo p)"""
        z %= self.psq
        a, f = z % self.p, z // self.p
        b = (self.p - f) % self.p
        assert (a - self.p * b - z) % self.psq == 0
        return a, b

    def val(self, x):
        return (x[0] - self.p * x[1]) % self.psq

    def pmul(self, x, y):
        (a, b), (c, d) = x, y
        t, q = self.redc(a * c)
        w, _ = self.redc(a * d + b * c + q)
        return t, w

    def mul(self, x, y):
        return self.redc(x * y)[0]


def entry(S, c_r_pair_row, pair_l2, pchunks, pchunk_limbs, hp_consts):
    """ps_entry_from_pair_row: per chunk a single product for its b half and a pair product for its a half, summed"""
    pconv, pcb = hp_consts
    acc_a = acc_b = 0
    for i in range(pchunks):
        za = c_r_pair_row[0] >> (RB * pchunk_limbs * i) & ((1 << (RB * pchunk_limbs)) - 1)
        zb = c_r_pair_row[1] >> (RB * pchunk_limbs * i) & ((1 << (RB * pchunk_limbs)) - 1)
        tb = S.mul(S.rng_ok(zb), pcb[i])
        a, b = S.pmul((S.rng_ok(za), 0), pconv[i])
        acc_a, acc_b = S.rng_ok(acc_a + a), S.rng_ok(acc_b + b + tb)
    return acc_a, acc_b


def exit_flag(t, p):
    """j with t = h + j p for the canonical h = t mod p: [t >= p] - [t < 0] for |t| < 2p"""
    return (1 if t >= p else 0) - (1 if t < 0 else 0)


def exit_mp(S, x, hp, seen=None):
    """(a, b) (x) (hp, 0) under the prime; mp = (j - b') mod p with a' = hp + j p"""
    t, w = S.pmul(x, (hp, 0))
    j = exit_flag(t, S.p)
    assert t - j * S.p == hp
    if seen is not None:
        seen.add(j)
    d = j - w
    assert -S.p < d < S.p                            # one conditional + p canonicalises it
    return d + S.p if d < 0 else d


def key_setup(p, q):
    """(side objects, chunking, per-side constants) as build_hensel_set builds them for the balanced set"""
    n = p * q
    # limbs per half of the key's pair rows (policy.hpp: pair_form_for_bits): (4,18) up to 2051 bits of n, then (8,14) -- the
    # kernel takes either, in chunks of at most 35 row limbs
    pair_l2 = 72 if n.bit_length() <= 2051 else 112
    fit = (K * LB - 2) // RB
    pchunks = -(-pair_l2 // fit)
    pchunk_limbs = -(-pair_l2 // pchunks)
    kn = (-pow(n, -1, 1 << RB)) % (1 << RB)
    Pn, Rn = n * kn, 1 << (RB * pair_l2)
    sides = []
    for pr, other in ((p, q), (q, p)):
        S = Side(pr, other, n.bit_length())
        R2n = R * R * pow(Rn, -1, S.psq) % S.psq
        kappa = other * kn % pr                       # k = 1: P = p
        r2n_p = R * R * pow(Rn, -1, pr) % pr
        pconv, pcb = [], []
        for i in range(pchunks):
            sh = 1 << (RB * pchunk_limbs * i)
            pconv.append(S.pair(R2n * sh))
            pcb.append(kappa * sh * r2n_p % pr)
        hp = orc.PrivateKey(n, p, q)._hfun(pr, pr * pr)
        S.consts = (pconv, pcb)
        S.hp = S.hp_canon = hp                        # (hp, 0) is a pair: hp - p would be another residue modulo p^2
        S.one = S.pair(R)
        sides.append(S)
    return sides, (pair_l2, pchunks, pchunk_limbs), (Pn, Rn)


def pair_row(c, n, Pn, Rn):
    """the pair row every other kernel writes for ciphertext c: c Rn mod Pn^2 as (a, b), c Rn == a - Pn b, unsigned"""
    z = c * Rn % (Pn * Pn)
    a, f = z % Pn, z // Pn
    return a, (Pn - f) % Pn


def decrypt_side(S, row, chunking, w=5, seen=None):
    pair_l2, pchunks, pchunk_limbs = chunking
    base = entry(S, row, pair_l2, pchunks, pchunk_limbs, S.consts)
    tbl = [S.one, base]
    for _ in range(2, 1 << w):
        tbl.append(S.pmul(tbl[-1], base))
    e = S.p - 1
    nwin = (e.bit_length() + w - 1) // w
    x = tbl[(e >> (w * (nwin - 1))) & ((1 << w) - 1)]
    for i in range(nwin - 2, -1, -1):
        for _ in range(w):
            x = S.pmul(x, x)
        x = S.pmul(x, tbl[(e >> (w * i)) & ((1 << w) - 1)])
    assert 100 * max(abs(x[0]), abs(x[1])) < 56 * S.p    # the main loop's values
    return base, x, exit_mp(S, x, S.hp, seen)


def is_prime(v):
    if any(v % s == 0 for s in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
        return False
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):            # Miller-Rabin, fixed bases
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(r - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def keys():
    out = {}
    for c in json.load(open(os.path.join(GOLD, "key_widths.json")))["cases"]:
        if c["bits"] in (2051, 2052):
            out[str(c["bits"])] = (int(c["p"], 16), int(c["q"], 16))
    k = json.load(open(os.path.join(GOLD, "primes_uneven.json")))
    assert k["bits"] == 2037
    out["2037"] = (int(k["p"], 16), int(k["q"], 16))
    for c in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"]:
        if c["bits"] == 2048 and "iso" not in out:
            out["iso"] = (int(c["p"], 16), int(c["q"], 16))
    # the widest primes the form takes: the two largest primes of 1040 bits (the largest p / R the bounds must hold for)
    found, v = [], (1 << FIT_BITS) - 1
    while len(found) < 2:
        if is_prime(v):
            found.append(v)
        v -= 2
    out["worst1040"] = (found[1], found[0])
    # the edges of the 2048-bit class (gen_ps_edge_primes.py): the narrowest and the widest primes the unsigned <38,28> kernel
    # serves beside this one, uneven pairs, and primes whose balanced limbs are nearly all zero / all of the largest magnitude
    for c in json.load(open(os.path.join(GOLD, "ps_edge_primes.json")))["cases"]:
        if c["name"].startswith("c2048-"):
            out[c["name"]] = (int(c["p"], 16), int(c["q"], 16))
    return out


KEYS = keys()


def test_key_fixture_covers_the_issue_list():
    assert sorted(KEYS) == ["2037", "2051", "2052", "c2048-heavy", "c2048-low", "c2048-tight", "c2048-uneven-low", "c2048-uneven-top",
                            "iso", "worst1040"]
    for name, (p, q) in KEYS.items():
        assert max(p.bit_length(), q.bit_length()) <= FIT_BITS, name
    assert KEYS["worst1040"][0].bit_length() == FIT_BITS
    widths = {name: tuple(sorted(v.bit_length() for v in KEYS[name])) for name in KEYS if name.startswith("c2048-")}
    assert widths == {"c2048-low": (1005, 1005), "c2048-tight": (1032, 1032), "c2048-uneven-top": (1018, 1032),
                      "c2048-uneven-low": (980, 1005), "c2048-heavy": (1024, 1024)}
    for v in KEYS["c2048-tight"]:                           # 2^1032 - j 2^28 + 1: balanced limbs nearly all zero
        assert sum(1 for x in limbs(v) if x == 0) >= 30
    for v in KEYS["c2048-heavy"]:                           # ... and limbs 0 .. 34 all of the largest magnitude
        assert all(abs(x) >= HALF - (1 << 16) for x in limbs(v)[:35])
    assert limbs(min(KEYS["c2048-uneven-low"]))[34:] == [0, 0]            # zero top limbs on one side


@pytest.mark.parametrize("name", sorted(KEYS))
def test_flow_gives_the_reference_plaintext_half(name):
    p, q = KEYS[name]
    if q < p:
        p, q = q, p
    n = p * q
    import math
    assert math.gcd(p, q) == 1 and math.gcd((p - 1) * q % p, p) == 1
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    rng = random.Random(len(name) + p % 1000)
    seen = set()
    cts = [1, n + 1, n * n - 1, rng.randrange(n * n), (1 + n * (n - 1)) * pow(rng.randrange(2, n), n, n * n) % (n * n),
           pow(rng.randrange(2, n), n, n * n)]
    for c in cts:
        row = pair_row(c, n, Pn, Rn)
        for S in sides:
            base, x, mp = decrypt_side(S, row, chunking, seen=seen)
            assert S.val(base) == c * R % S.psq                       # the entry: c R as a pair
            u = pow(c % S.psq, S.p - 1, S.psq)
            assert S.val(x) == u * R % S.psq
            if math.gcd(c, S.p) == 1:
                assert mp == (u - 1) // S.p * S.hp_canon % S.p        # pri_key.cpp:142, 154-157
    for S in sides:
        # the entry sums three or four chunk products of constants below p (a below 2.1 p, b below 4.2 p); from there on
        # |value| <= p (1/2 + (p / R) |x| |y| / p^2) settles near 0.54 p.  K balanced limbs hold +-BIAS >= +-7.9 p
        assert S.top < 4.5 and BIAS // S.p >= 7, S.top
    assert seen <= {-1, 0}


def test_exit_flag_cases_are_all_reached():
    """a' of both signs, and beyond the prime (which the flow never produces: |a'| < 0.56 p): the flag generalises
    [a' >= p] to {-1, 0, 1}; mp is the same residue in every case"""
    p, q = KEYS["iso"]
    if q < p:
        p, q = q, p
    S = Side(p, q, (p * q).bit_length())
    rng = random.Random(5)
    hp = rng.randrange(1, p)
    seen = set()
    for _ in range(40):
        L = rng.randrange(p)                                          # the value the exit must return: u = 1 + p L, times hp
        target = (hp + p * (L * hp % p)) % S.psq                      # the pair (a', b') represents this modulo p^2
        for j in (-1, 0, 1):
            a1 = hp + j * p                                           # a' < 0, in [0, p), >= p
            b1 = ((a1 - target) // p) % p
            assert (a1 - p * b1 - target) % S.psq == 0
            for b_rep in (b1, b1 - p):                                # b' of both signs
                f = exit_flag(a1, p)
                seen.add((f, b_rep < 0))
                d = f - b_rep
                assert (d % p) == L * hp % p
    assert seen == {(j, s) for j in (-1, 0, 1) for s in (False, True)}
    # the flow itself reaches a' of both signs
    sides, chunking, (Pn, Rn) = key_setup(p, q)
    n = p * q
    flow = set()
    for i in range(12):
        c = pow(rng.randrange(2, n), n, n * n) * (1 + n * i) % (n * n)
        decrypt_side(sides[i & 1], pair_row(c, n, Pn, Rn), chunking, w=5, seen=flow)
        if flow == {-1, 0}:
            break
    assert flow == {-1, 0}


def test_columns_stay_inside_the_accumulator_on_adversarial_operands():
    """all limbs +-2^28 (the doubled operand of a squaring +-2^29), digits as they fall: every partial column sum inside
    int64, and the analytic bound 3K 2^56 + 2^(LB+6) < 2^63 of the static_assert"""
    assert 3 * K * (1 << (2 * (LB - 1))) + (1 << (LB + 6)) < 1 << 63
    p = KEYS["worst1040"][0]
    S = Side(p, 0, 0)
    log = ColumnLog()
    for sa in (1, -1):
        for sb in (1, -1):
            for alt in (False, True):
                a = [sa * HALF * (-1 if alt and i & 1 else 1) for i in range(K)]
                b2 = [2 * sb * HALF * (-1 if alt and i & 1 else 1) for i in range(K)]
                nl = [HALF if i else (HALF - 1) for i in range(K)]    # the largest modulus limbs (odd n_0)
                n0 = (-pow(nl[0], -1, 1 << LB)) % (1 << LB)
                _, q, _ = montmul_limbs(a, a, nl, n0, log=log)
                montmul_limbs(a, b2, nl, n0, qin=q, log=log)          # the squaring's second product
                b1 = [v // 2 for v in b2]
                montmul_limbs(a, b1, nl, n0, x2=b1, y2=a, qin=q, log=log)     # the pair product's a d + b c + q
    assert log.top < 1 << 63
    # ... and with a real modulus the limb model and the integer model are the same arithmetic
    rng = random.Random(11)
    for _ in range(6):
        a, b, c, d = (rng.randrange(-p // 2, p // 2) for _ in range(4))
        r, q, carry = montmul_limbs(limbs(a), limbs(c), S.nl, S.n0inv, log=log)
        t, Q = S.redc(a * c)
        assert (num(r), num(q), carry) == (t, Q, 0)
        r2, _, carry = montmul_limbs(limbs(a), limbs(d), S.nl, S.n0inv, x2=limbs(b), y2=limbs(c), qin=q, log=log)
        assert (num(r2), carry) == (S.pmul((a, b), (c, d))[1], 0)
        dbl = [2 * v for v in limbs(b)]
        r3, _, carry = montmul_limbs(limbs(a), dbl, S.nl, S.n0inv, qin=montmul_limbs(limbs(a), limbs(a), S.nl, S.n0inv)[1], log=log)
        assert (num(r3), carry) == (S.pmul((a, b), (a, b))[1], 0)
