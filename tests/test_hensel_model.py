"""Integer model of the split-form arithmetic of csrc/hensel.hpp (CPU test, no GPU): residues modulo P^2 as pairs
x == a - P*b, the pair Montgomery product built from two half-width reductions, the chunked entry of a
ciphertext, the fixed-window exponentiation, and the exit under the true prime that yields
mp = L_p(c^(p-1) mod p^2) * hp mod p (ipcl/pri_key.cpp:136-157) without a division.  The lazy bounds the kernel
relies on (every component below 2P) are asserted on the way."""
import json
import os
import random

import pytest

LB = 29
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def setup(p, K):
    k = (-pow(p, -1, 1 << LB)) % (1 << LB)
    P = k * p
    assert P % (1 << LB) == (1 << LB) - 1            # unit quotient digits
    R = 1 << (LB * 2 * K)
    assert R >= 256 * P
    return k, P, R


def to_pair(z, P):
    z %= P * P
    a, f = z % P, z // P
    return (a, (P - f) % P)


def val(pr, P):
    return (pr[0] - P * pr[1]) % (P * P)


def redc(T, P, R):
    q = (T * (-pow(P, -1, R))) % R
    return (T + q * P) // R, q


def pmul(x, y, P, R):
    (a, b), (c, d) = x, y
    t, q = redc(a * c, P, R)
    w, _ = redc(a * d + b * c + q, P, R)
    assert t < 2 * P and w < 2 * P
    return (t, w)


def cases():
    out = []
    for case in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"]:
        if case["bits"] in (1024, 2048):
            out.append((int(case["p"], 16), int(case["q"], 16)))
    return out[:2]


@pytest.mark.parametrize("side", [0, 1])
def test_pair_exponentiation_matches_reference_formula(side):
    rng = random.Random(3 + side)
    for p, q in cases():
        if side:
            p, q = q, p
        bits = p.bit_length()
        K = (bits + 37 + 2 * LB - 1) // (2 * LB)
        k, P, R = setup(p, K)
        n = p * q
        cw = min((bits + 63) // 64, bits // 64)
        nch = (2 * ((n.bit_length() + 63) // 64) + cw - 1) // cw
        conv = [to_pair((1 << (64 * cw * i)) * R * R, P) for i in range(nch)]
        hp = pow(((pow(n + 1, p - 1, p * p) - 1) // p), -1, p)        # computeHfun, pri_key.cpp:159-167
        for c in (1, n + 1, n * n - 1, rng.randrange(n * n), rng.randrange(n * n)):
            acc = (0, 0)
            for i in range(nch):
                z = (c >> (64 * cw * i)) & ((1 << (64 * cw)) - 1)
                assert z < 2 * P
                t = pmul((z, 0), conv[i], P, R)
                acc = (acc[0] + t[0], acc[1] + t[1])
            assert val(acc, P) == c * R % (P * P)
            w = 5
            tbl = [to_pair(R, P), acc]
            for _ in range(2, 1 << w):
                tbl.append(pmul(tbl[-1], acc, P, R))
            e = p - 1
            nwin = (e.bit_length() + w - 1) // w
            x = tbl[(e >> (w * (nwin - 1))) & 31]
            for i in range(nwin - 2, -1, -1):
                for _ in range(w):
                    x = pmul(x, x, P, R)
                x = pmul(x, tbl[(e >> (w * i)) & 31], P, R)
            u = pow(c, p - 1, p * p)
            assert val(x, P) % (p * p) == u * R % (p * p)
            # exit: (a, k*b mod p) is a pair modulo p^2; product with (hp, 0) under the true prime
            a, B = x[0], redc(x[1] * (k * R % p), p, R)[0]            # k*b mod p (lazy) by a half-width product
            assert B < 2 * p and (B - k * x[1]) % p == 0
            n0 = (-pow(p, -1, R)) % R
            q1 = a * hp * n0 % R
            t = (a * hp + q1 * p) // R
            q2 = (B * hp + q1) * n0 % R
            w2 = (B * hp + q1 + q2 * p) // R
            assert t < 2 * p and w2 < 2 * p and t % p == hp
            j = 1 if t >= p else 0
            assert (j - w2) % p == ((u - 1) // p) * hp % p          # pri_key.cpp:142, 154-157


# the edges of the classes, with the pair rows their keys have (tests/golden/ps_edge_primes.json): 1032-bit primes beside a
# 1018-bit one on (4,18) rows, beside another of their width on (8,14) rows
@pytest.mark.parametrize("bits,K,LBp,pair_l2", [pytest.param(512, 19, 29, 38, id="512-19-29"), pytest.param(1024, 38, 28, 72, id="1024-38-28"),
                                                pytest.param(1536, 56, 28, 112, id="1536-56-28"),
                                                (490, 19, 29, 38), (518, 19, 29, 38), (1005, 38, 28, 72), (1032, 38, 28, 72),
                                                (1032, 38, 28, 112), (1509, 56, 28, 112)])
def test_product_scanning_form_bounds_with_sixteen_fold_headroom(bits, K, LBp, pair_l2):
    """csrc/hensel_ps.hpp keeps a residue in K limbs of LB bits with R = 2^(LB K) >= 16 P only (capi_keys.inc: build_hensel;
    the multi-lane forms keep 256).  Upper bounds, as multiples of P, pushed through the kernel's flow with the WORST
    headroom R = 16 P: the chunked entry (a chunk below R/4, at most 4 chunks summed), the window-table recurrence, the main
    loop (squarings, products by any table entry), and the column sums of the widest product.  Everything must stay below
    R (the limbs hold it) and a column below 2^64 (one 64-bit accumulator holds it).  Lazy Montgomery product:
    redc(T) < T/R + P."""
    F = lambda a, b=1: a / b * (1 + 1e-12)      # upper bounds in floating point, rounded up a little at every step
    assert LBp * K >= bits + LBp + 4 and LBp * (K - 1) < bits + LBp + 4          # the K build_hensel picks
    rho = 16.0                                                                   # R / P, worst case
    assert pair_l2 in (2 * 19, 4 * 18, 8 * 14)                                   # 29-bit limbs per half of an n^2 pair row
    chunks = -(-pair_l2 // ((LBp * K - 2) // 29))                                # (build_hensel_set: pchunks)
    assert chunks <= 4

    def mul(c1, c2):                       # one lazy product of values below c1 P and c2 P
        return F(c1 * c2, rho) + 1

    def pairmul(x, y):                     # (a, b) (x) (c, d): t = a c, w = a d + b c + q (q < R: + 1 P at most, counted in the +1)
        (a, b), (c, d) = x, y
        return (mul(a, c), F(a * d + b * c, rho) + 1 + 1e-6)

    # entry: chunk values below R/4 = rho/4 P, conversion constants below P
    z = rho / 4
    a, b = pairmul((z, 0.0), (1.0, 1.0))
    b += mul(z, 1.0)                      # ps_add(b, tb)
    base = (chunks * a, chunks * b)        # ps_add(acc, .) over the chunks
    assert max(base) < rho
    # window table: entry e = entry e-1 (x) base; the bounds are monotone in the inputs, so their running maximum covers all
    entry = base
    worst = base
    for _ in range(64):
        entry = pairmul(entry, base)
        worst = (max(worst[0], entry[0]), max(worst[1], entry[1]))
    assert max(worst) < rho
    # main loop from any entry: squarings and products by the worst entry, to a fixed point
    s = worst
    top = s
    for _ in range(200):
        for _ in range(5):
            s = pairmul(s, s)
            top = (max(top[0], s[0]), max(top[1], s[1]))
        s = pairmul(s, worst)
        top = (max(top[0], s[0]), max(top[1], s[1]))
    assert max(top) < rho and max(s) < 3
    # columns: canonical limbs below 2^LB, the doubled operand of a squaring below 2^(LB+1): at most 3K products of 2^(2 LB) each
    assert 3 * K * (1 << (2 * LBp)) < 1 << 64


# ---- csrc/hensel_wave.hpp, lane for lane ----------------------------------------------------------------------------
def _edge_prime(name, side):
    """the primes at the edges of the one-lane / one-wavefront forms: tests/golden/ps_edge_primes.json, and the tight
    3072-bit key of primes_worst_headroom.json"""
    if name == "worst-headroom":
        k = json.load(open(os.path.join(GOLD, "primes_worst_headroom.json")))
    else:
        k = {c["name"]: c for c in json.load(open(os.path.join(GOLD, "ps_edge_primes.json")))["cases"]}[name]
    return int(k["pq"[side]], 16)


class WaveLanes:
    """one wavefront of hensel_decrypt_wave_kernel<K, LB, WIDEQ> with Python integers: lane l holds limb l, lane K is the
    zero lane above them; every 32-bit register and 64-bit accumulator of the kernel is checked for its width"""

    def __init__(self, K, LBk, wide, p):
        self.K, self.LB, self.wide, self.p = K, LBk, wide, p
        self.M = (1 << LBk) - 1
        self.k = (-pow(p, -1, 1 << LBk)) % (1 << LBk)
        self.P = p * self.k
        self.R = 1 << (LBk * K)
        self.nl = [(self.P >> (LBk * l)) & self.M for l in range(K)] + [0]
        self.worst = 0

    def lanes(self, v):                             # canonical limbs
        assert 0 <= v < self.R
        return [(v >> (self.LB * l)) & self.M for l in range(self.K)] + [0]

    def num(self, ls):
        return sum(v << (self.LB * l) for l, v in enumerate(ls))

    def slide(self, acc):
        K, M, LBk = self.K, self.M, self.LB
        return [(acc[l + 1] & M if l + 1 <= K else 0) + (acc[l] >> LBk) for l in range(K + 1)]

    def digit(self, acc):
        return acc[0] & (0xFFFFFFFF if self.wide else self.M)

    def finish(self, acc):                          # wv_finish: own low limb plus the carry of the lane below
        return [(acc[l] & self.M) + ((acc[l - 1] >> self.LB) if l else 0) for l in range(self.K + 1)]

    def pairop(self, a, b, c, d, sqr):
        """wv_pairsqr (c = a, d = b, the b operand doubled IN 32 BITS) / wv_pairmul, lock-step"""
        K, M, nl = self.K, self.M, self.nl
        assert max(a + b + c + d) < 1 << 32
        acc1, acc2 = [0] * (K + 1), [0] * (K + 1)
        mul2 = [2 * v for v in b] if sqr else d
        assert max(mul2) < 1 << 32, "the doubled operand of a squaring leaves its 32-bit register"
        for i in range(K):
            acc1 = [acc1[l] + a[i] * c[l] for l in range(K + 1)]
            q1 = self.digit(acc1)
            acc2 = [acc2[l] + a[i] * mul2[l] for l in range(K + 1)]
            if not sqr:
                acc2 = [acc2[l] + b[i] * c[l] for l in range(K + 1)]
            acc1 = [acc1[l] + q1 * nl[l] for l in range(K + 1)]
            acc2[0] += q1
            q2 = self.digit(acc2)
            self.worst = max(self.worst, max(acc1), max(acc2) + q2 * M)
            assert acc1[0] & M == 0
            acc1 = self.slide(acc1)
            acc2 = [acc2[l] + q2 * nl[l] for l in range(K + 1)]
            assert acc2[0] & M == 0
            acc2 = self.slide(acc2)
        t, w = self.finish(acc1), self.finish(acc2)
        assert t[K] == 0 and w[K] == 0
        return t, w

    def check(self, t, w, x, y):
        """(t, w) is the pair product of hensel.hpp of the pairs x and y (limb lists)"""
        P, R, num = self.P, self.R, self.num
        vx, vy = num(x[0]) - P * num(x[1]), num(y[0]) - P * num(y[1])
        assert (num(t) - P * num(w)) % (P * P) == vx * vy * pow(R, -1, P * P) % (P * P)


# (K, LB, wide, key, side): the six (K, wide) combinations a key can get, at the tight primes (k = 2^LB - 1: R / P at its least,
# 16 with LB-bit digits and 2^10 with 32-bit ones) and at the narrowest primes of each class.  No key of the fixture has tight
# 1026-bit primes: "tight-1026" is 2^1026 - 2^28 + 1 (any odd modulus serves the algebra)
WAVE_EDGES = [(19, 29, False, "c1024-tight", 0), (19, 29, False, "c1024-tight", 1), (19, 29, True, "c1024-tight-wide", 1),
              (19, 29, True, "c1024-low", 0), (38, 28, False, "c2048-tight", 0), (38, 28, False, "c2048-tight", 1),
              (38, 28, False, "c2048-uneven-top", 0), (38, 28, True, "tight-1026", 0), (38, 28, True, "c2048-low", 0),
              (38, 28, True, "c2048-heavy", 1), (56, 28, False, "worst-headroom", 0), (56, 28, False, "worst-headroom", 1),
              (56, 28, True, "c3072-tight-wide", 1), (56, 28, True, "c3072-low", 0)]
# the bit length of the larger prime of each key: it picks K and the digit form for both sides (capi.cpp: decrypt_on)
WAVE_EDGE_BITS = {"c1024-tight": 518, "c1024-tight-wide": 512, "c1024-low": 490, "c2048-tight": 1032, "c2048-uneven-top": 1032,
                  "tight-1026": 1026, "c2048-low": 1005, "c2048-heavy": 1024, "worst-headroom": 1536, "c3072-tight-wide": 1530,
                  "c3072-low": 1509}


@pytest.mark.parametrize("pbits,K,LBk,wide,modulus",
                         [pytest.param(1024, 38, 28, False, None, id="1024-38-28-False"), pytest.param(1024, 38, 28, True, None, id="1024-38-28-True"),
                          pytest.param(512, 19, 29, True, None, id="512-19-29-True"), pytest.param(1536, 56, 28, False, None, id="1536-56-28-False")]
                         + [pytest.param(WAVE_EDGE_BITS[name], K, LBk, wide, (name, side), id="%s-%d-%d-%d-%s" % (name, side, K, LBk, wide))
                            for K, LBk, wide, name, side in WAVE_EDGES])
def test_wavefront_wide_form_lane_model(pbits, K, LBk, wide, modulus):
    """csrc/hensel_wave.hpp lane for lane with Python integers: one limb per lane, operand scan with the accumulators sliding
    down the lanes, the two scans of a pair product in lock-step, relaxed limbs, and -- `wide` -- whole-word (32-bit) quotient
    digits where R >= 2^10 P.  Every product must be the pair product of hensel.hpp, every accumulator stay below 2^64 and every
    limb (the doubled b operand of a squaring included) in its 32-bit register.

    Without a modulus: a random one, squarings and products from values of 4 P (17 P / 9 P with wide digits); they settle below
    2 P (17 P / 9 P) and fit the K limbs.

    With one of the edge primes (WAVE_EDGES) the kernel's OWN flow is followed from the values the code hands in:
      - the entry (hensel_ps_entry_kernel): a chunk of the pair row has at most (LB K - 2) / 29 limbs of 29 bits, so it is below
        R / 4 (capi_keys.inc: build_hensel_set, `fit`); its products by constants below P are lazy products of the one-lane
        code with LB-bit digits: below (R / 4) P / R + P = 1.25 P, in canonical limbs.  A row has up to pchunks chunks (3, 4 and
        3 for K = 19, 38, 56: 38 and 112 row limbs per half), each with a pair product for its a half and a single product for
        its b half: the wave kernel sums pchunks partial values into a (below 5 P) and 2 pchunks into b (below 10 P), limb by
        limb -- limbs of up to 2 pchunks 2^LB.  One carry step (wv_finish) makes them relaxed limbs before anything is
        multiplied: doubled for a squaring, the summed limbs of <19,29> leave 32 bits, and the main loop starts from entry 1 =
        base where the exponent's top window holds a lone bit;
      - the table recurrence entry e = entry e-1 (x) base over the 32 entries of the widest table;
      - the main loop from entry 1, entry 2 (the largest) and the last entry: w squarings and a product by an entry, three
        windows each -- by then the values have settled.
    WHAT THE EXIT NEEDS of the pair it picks up (hensel_ps_exit_kernel, ps_exit_words in hensel_ps.hpp): that a and b FIT THE K
    LIMBS, a, b < R = 2^(LB K), nothing tighter -- ps_relimb<K, LB, K, LB> carries relaxed limbs into canonical ones ("the value
    must fit"), and the products under the true prime p divide by R >= 16 p k: k b = b kr / R + p < 2 p for b < R, kr < p;
    a' = a hp / R + p < 2 p for a < R; b' = (kb hp + q) / R + p < 2 p.  The one conditional subtraction of each then holds.  The
    2 P (17 P / 9 P) of the random-modulus cases is what the digits GUARANTEE once the values have settled, not what the exit
    requires: with LB-bit digits at R = 16 P the flow passes (5 P, 10 P) -> (2.6 P, 7.3 P) -> ... and every value is below R."""
    if modulus is None:
        rng = random.Random(pbits + K + wide)
        while True:                                     # a prime-like odd modulus is enough for the algebra: any odd p works
            p = rng.getrandbits(pbits) | (1 << (pbits - 1)) | 1
            if p % 3 and p % 5:
                break
    elif modulus[0] == "tight-1026":
        p = (1 << 1026) - (1 << 28) + 1
    else:
        p = _edge_prime(*modulus)
    W = WaveLanes(K, LBk, wide, p)
    M, P, R, lanes, num, pairop = W.M, W.P, W.R, W.lanes, W.num, W.pairop
    assert P % (1 << LBk) == M and R >= 16 * P and (not wide or LBk * K - (pbits + LBk) >= 10)      # capi.cpp: decrypt_on
    assert LBk * K >= pbits + LBk + 4 > LBk * (K - 1)                                               # capi_keys.inc: build_hensel
    assert modulus is None or wide == (LBk * K - (pbits + LBk) >= 10)                               # (PGPU_WAVE_WIDEQ=0 aside)
    bound = ((1 << (32 - LBk)) + 1) * P if wide else 2 * P
    if modulus is None:
        start = 4 * P - 1 if not wide else bound - 1              # the largest values the flow can hand in
        a, b = lanes(start), lanes(start - 12345)
        c, d = lanes(start - 99), lanes(start - 7)
        for rounds in range(3):
            t, w = pairop(a, b, c, d, False)
            W.check(t, w, (a, b), (c, d))
            assert num(t) < bound and num(w) < bound and max(t + w) < (1 << LBk) + (1 << 9)
            a, b = t, w
            t, w = pairop(a, b, a, b, True)
            W.check(t, w, (a, b), (a, b))
            assert num(t) < bound and num(w) < bound
            a, b = t, w
        assert W.worst < 1 << 64
        return
    # ---- the fixture's property this case is there for ----
    name = modulus[0]
    if "tight" in name or name == "worst-headroom":
        assert W.k == M and p.bit_length() == pbits
        least = 1 << 10 if wide else 16
        assert least * P <= R < least * (P + (P >> 20))               # R / P at the least the digit form is taken with
    elif name.endswith("-low"):
        assert p.bit_length() == pbits and LBk * (K - 1) == pbits - 1 + LBk + 4        # one bit less takes K - 1 limbs
    # ---- the base as the code hands it in ----
    fit = (LBk * K - 2) // 29
    pchunks = {19: 3, 38: 4, 56: 3}[K]
    assert pchunks == -(-{19: 38, 38: 112, 56: 112}[K] // fit) <= 4 and 1 << (29 * fit) <= R // 4
    part = (R // 4 * P) // R + P                                   # a lazy product of a chunk by a constant: below this
    assert part <= 5 * P // 4 + 1
    parts = [lanes(part - 1 - 1000003 * r) for r in range(2 * pchunks)]
    raw_a = [sum(parts[2 * r][l] for r in range(pchunks)) for l in range(K + 1)]
    raw_b = [sum(parts[r][l] for r in range(2 * pchunks)) for l in range(K + 1)]
    assert max(raw_a + raw_b) < 1 << 32 and num(raw_a) < 5 * P + 4 and num(raw_b) < 10 * P + 8
    # doubled as they are, the summed limbs fit 32 bits at <38,28> and <56,28> only (8 * 2^28 * 2, 6 * 2^28 * 2; 6 * 2^29 * 2)
    assert (2 * 2 * pchunks * M < 1 << 32) == (K != 19)
    if K == 19 and name != "c1024-low":
        assert 2 * max(raw_b) >= 1 << 32
    base = (W.finish(raw_a), W.finish(raw_b))                      # the carry step: nothing leaves limb K - 1
    assert base[0][K] == 0 and base[1][K] == 0 and (num(base[0]), num(base[1])) == (num(raw_a), num(raw_b))
    assert max(base[0] + base[1]) < (1 << LBk) + 2 * pchunks
    # as a MULTIPLIER the summed limbs are harmless (the accumulators hold them): the same product either way
    t, w = pairop(base[0], base[1], raw_a, raw_b, False)
    assert W.worst < 1 << 64
    W.check(t, w, base, base)
    # ---- window table: entry e = entry e-1 (x) base, 32 entries (w = 5, the widest the LDS table takes) ----
    table = [None, base]
    for e in range(2, 32):
        t, w = pairop(table[-1][0], table[-1][1], base[0], base[1], False)
        W.check(t, w, table[-1], base)
        assert num(t) < R and num(w) < R
        table.append((t, w))
    top = max(max(num(x[0]), num(x[1])) for x in table[2:])        # (of the products: the base itself is below 10 P)
    # ---- main loop: from entry 1 (squared at once: the lone top bit), the largest entry and the last ----
    digit_p = (1 << (32 - LBk)) if wide else 1                     # a lazy product is below T / R + digit_p P
    for first in (1, 2, 31):
        a, b = table[first]
        for win, e in enumerate((2, 31, 1)):
            for _ in range(5):
                t, w = pairop(a, b, a, b, True)
                W.check(t, w, (a, b), (a, b))
                a, b = t, w
                assert num(a) < R and num(b) < R                   # what the exit needs, at every step
                top = max(top, num(a), num(b))
            t, w = pairop(a, b, table[e][0], table[e][1], False)
            W.check(t, w, (a, b), table[e])
            a, b = t, w
            assert num(a) < R and num(b) < R
            top = max(top, num(a), num(b))
        # settled: what the digits guarantee from values of that size -- and relaxed limbs ps_relimb's 32-bit carries take
        assert num(a) < (digit_p + 1) * P and num(b) < (digit_p + 2) * P and max(a + b) < (1 << LBk) + (1 << 9)
    assert top < R and W.worst < 1 << 64
    if not wide and R < 17 * P:
        assert top > 2 * P                                          # ... and the flow does pass values beyond 2 P on its way
