"""Integer model of the unit-factor fixed-base table and of the DJN encrypt that runs on it (csrc/hensel.hpp:
hensel_fb_build_kernel / hensel_fb_unit_factor_kernel / hensel_fb_encrypt_kernel, csrc/hensel_seq.hpp: hensel_fb_encrypt_seq_kernel,
csrc/hensel_wave_n2.hpp: hensel_fb_encrypt_wave_kernel).  CPU test, no GPU.

A table entry is a pair g*R == a - P*b (mod P^2) under the scaled modulus P = n*k == -1 (mod 2^29).  Modulo n^2
        a - P*b == a * (1 + n*beta),     beta = (-k * b * a^-1) mod n        (a^-1 under the TRUE modulus n)
and the table stores (a, beta).  The encrypt multiplies the pairs (a_i, 0) -- two half-width products instead of three --,
adds the beta_i and lets the sum S ride on the plaintext:  c = (prod a_i) * (1 + n*(m + S)).

The model follows the kernels step by step: lazy pair products (components below 2P, a parts mostly far ABOVE n), the
simultaneous inversion (running products under n, one total per row or per segment of a row inverted on the host, the walk
back with two half-width products per entry), canonical betas, the lazy limb sum of S with a carry round every second step, no reduction of S (the Montgomery
product by gm takes m + S < R / 4 down below 2n), and the exit  b += M(M(m + S, gm), a).  Ciphertexts are compared with
oracle/paillier_oracle.py."""
import json
import os
import random

import pytest

from oracle import paillier_oracle as orc

LB = 29
MASK = (1 << LB) - 1
GOLD = os.path.join(os.path.dirname(__file__), "golden")
# (lanes per half, limbs per lane) of the sequential-halves form per key size (capi_keys.inc: build_hensel_pub picks the
# smallest compiled form with 29*L2 >= bits + 29 + 8)
FORMS = {1024: (2, 19), 2048: (4, 18), 3072: (8, 14)}


def keys():
    out = {}
    for case in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"]:
        if case["djn"] and case["bits"] in (1024, 3072) and case["bits"] not in out:
            out[case["bits"]] = (int(case["p"], 16) * int(case["q"], 16), int(case["hs"], 16))
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    out[2048] = (int(k["p"], 16) * int(k["q"], 16), int(k["bench_hs"], 16))
    return out


class Ctx:
    def __init__(self, n, bits):
        self.n, self.bits = n, bits
        self.G, self.K = FORMS[bits]
        self.L2 = self.G * self.K
        assert LB * self.L2 >= bits + LB + 8
        self.k = (-pow(n, -1, 1 << LB)) % (1 << LB)
        self.P = self.k * n
        assert self.P % (1 << LB) == MASK
        self.R = 1 << (LB * self.L2)
        assert self.R >= (1 << 37) * n                     # the headroom the lazy sum relies on
        self.n0 = (-pow(n, -1, self.R)) % self.R
        self.P0 = (-pow(self.P, -1, self.R)) % self.R
        self.gm = (-pow(self.k, -1, n)) * self.R * self.R % n      # HenselPubDev::gm

    def M(self, x, y):
        """lazy half-width Montgomery product under the TRUE modulus n: below x*y/R + n"""
        t = x * y
        return (t + (t * self.n0 % self.R) * self.n) // self.R

    def redcP(self, T):
        q = T * self.P0 % self.R
        return (T + q * self.P) // self.R, q

    def pmul(self, x, y, dz=False):
        """(a, b) (x) (c, d); dz: d is zero and its product is not formed"""
        (a, b), (c, d) = x, y
        t, q = self.redcP(a * c)
        w, _ = self.redcP((0 if dz else a * d) + b * c + q)
        assert t < 2 * self.P and w < 2 * self.P
        return (t, w)

    def to_pair(self, z):
        z %= self.P * self.P
        return (z % self.P, (self.P - z // self.P) % self.P)

    def val(self, pr):
        return (pr[0] - self.P * pr[1]) % (self.P * self.P)

    # ---- limbs: lane x of the G lanes holds limbs [x*K, x*K + K) ----
    def limbs(self, v):
        assert v < self.R
        return [(v >> (LB * i)) & MASK for i in range(self.L2)]

    def num(self, ls):
        return sum(v << (LB * i) for i, v in enumerate(ls))

    def add_normalise(self, a, k):
        """kernels.hpp: add_normalise -- a += k, a carry pass inside every lane, the lane's carry-out rippled through the next
        lane, what that leaves added to the limb 0 after it"""
        G, K = self.G, self.K
        out, carry = [], []
        for x in range(G):
            c = 0
            for j in range(K):
                u = a[x * K + j] + k[x * K + j] + c
                assert u < 1 << 32
                out.append(u & MASK)
                c = u >> LB
            carry.append(c)
        cc2 = []
        for x in range(G):
            cc = carry[x - 1] if x else 0
            for j in range(K):
                u = out[x * K + j] + cc
                out[x * K + j] = u & MASK
                cc = u >> LB
            cc2.append(cc)
        assert carry[G - 1] == 0 and cc2[G - 1] == 0        # the value stays below R
        for x in range(1, G):
            out[x * K] += cc2[x - 1]
        return out


def build_table(C, hs, w, nwin, seg_len=None):
    """hensel_fb_build_kernel, hensel_fb_unit_factor_kernel and the host step between them; returns [row][d] = (alpha, beta).  seg_len: entries
    per inversion segment (the library: 1024 for longer rows) -- every segment has its own running products and total"""
    n, R = C.n, C.R
    T = 1 << w
    base = C.to_pair(hs * R)
    table = []
    above_n = 0
    scale = (R % n) * ((n - C.k % n) % n) % n              # R * (-k) mod n
    for i in range(nwin):
        if i:
            for _ in range(w):
                base = C.pmul(base, base)
        ent = [C.to_pair(R), base]
        for d in range(2, T):
            ent.append(C.pmul(ent[-1], base))
        assert all(C.val(e) == pow(hs, d << (w * i), C.P * C.P) * R % (C.P * C.P) for d, e in list(enumerate(ent))[:3])
        above_n += sum(1 for a, _ in ent if a >= n)
        # hensel_fb_build_kernel: running products of the a parts, restarted at every segment
        sl = seg_len or T
        assert sl >= 2 and T % sl == 0
        pre = []
        for d in range(T):
            pre.append(ent[d][0] if d % sl == 0 else C.M(pre[-1], ent[d][0]))
            # a parts are below 2P = 2kn, far above n: the first products of a segment are large (a * a' / R), then every
            # step contracts by 2P / R <= 2^-7 -- always below R / 4, below 2n from the fourth on
            assert pre[-1] < R // 4 and (d % sl < 4 or pre[-1] < 2 * n)
        # hensel_fb_unit_factor_kernel: the walk back, segment by segment; the host inverts ONE total per segment
        row = [None] * T
        for d in range(T - 1, -1, -1):
            if d % sl == sl - 1:
                tot = pre[d] % n
                assert tot
                u = pow(tot, -1, n) * scale % n
            first = d % sl == 0
            a, b = ent[d]
            r = u if first else C.M(u, pre[d - 1])                             # half B: ia = a_d^-1 * R * (-k)
            un = u if first else C.M(u, a)                                     # half A: u_(d-1)
            be = C.M(b, r)
            assert be < 2 * n and un < 2 * n
            be %= n                                                            # full_normalise + cond_sub_limbs
            if d < 3 or d == T - 1:
                assert be == (-C.k * b * pow(a, -1, n)) % n
            assert a * (1 + n * be) % (n * n) == C.val(ent[d]) % (n * n)       # the identity, modulo n^2
            row[d] = (a, be)
            u = un
        table.append(row)
    assert above_n > nwin * T // 2                         # relaxed a parts: most of them are larger than n (P = n*k)
    return table


def lazy_sum(C, betas, m):
    """the S of the paired and the sequential-halves kernel: beta_0, then per step a plain limb-wise addition (odd steps) or
    add_normalise (even steps); at the exit add_normalise(m, S).  Returns the limbs of m + S.  Every bound the kernels rely on
    is asserted on the way: 32-bit limb arithmetic, limbs below 3 * 2^29 between carry rounds, no carry out of the top lane."""
    S = C.limbs(betas[0])
    s_val = betas[0]
    for i in range(1, len(betas)):
        bl = C.limbs(betas[i])
        if i & 1:
            S = [s + t for s, t in zip(S, bl)]
            assert max(S) < 3 << LB                        # below 2^31
        else:
            S = C.add_normalise(S, bl)
            assert max(S) <= (1 << LB) + 1
        s_val += betas[i]
        assert C.num(S) == s_val
    mv = C.add_normalise(C.limbs(m), S)
    assert max(mv) <= (1 << LB) + 1 and C.num(mv) == m + s_val
    return mv


def wave_sum(C, betas, m):
    """the S of the wavefront-wide kernel (hensel_wave_n2.hpp: sum_beta): add, then ONE carry round, every step and for m"""
    S = [0] * C.L2
    total = 0
    for y in list(betas) + [m]:
        t = [s + v for s, v in zip(S, C.limbs(y))]
        assert max(t) < 1 << 32
        assert t[-1] >> LB == 0                            # nothing leaves the top limb
        S = [(t[i] & MASK) + ((t[i - 1] >> LB) if i else 0) for i in range(C.L2)]
        assert max(S) <= (1 << LB) + 2
        total += y
        assert C.num(S) == total
    return S


def encrypt(C, table, w, nwin, r, m):
    """the encrypt kernels on a unit-factor table; returns the ciphertext as a residue modulo n^2"""
    n, R = C.n, C.R
    dig = lambda i: (r >> (w * i)) & ((1 << w) - 1)
    acc = (table[0][dig(0)][0], 0)
    for i in range(1, nwin):
        acc = C.pmul(acc, (table[i][dig(i)][0], 0), dz=True)
    betas = [table[i][dig(i)][1] for i in range(nwin)]
    mv = lazy_sum(C, betas, m)
    assert C.num(wave_sum(C, betas, m)) == C.num(mv)
    assert C.num(mv) < (nwin + 2) * n and (nwin + 2) * n < R // 4
    u = C.M(C.num(mv), C.gm)
    v = C.M(u, acc[0])
    assert u < 2 * n and v < 2 * n
    out = (acc[0], acc[1] + v)
    return C.val(out) * pow(R, -1, n * n) % (n * n)


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_unit_factor_encrypt_matches_oracle(bits):
    n, hs = keys()[bits]
    C = Ctx(n, bits)
    rbits = bits // 2
    rng = random.Random(bits)
    opk = orc.PublicKey(n, bits)
    opk.set_djn(hs)
    for w, seg_len in (((4, None), (5, 8)) if bits == 2048 else ((5, None),)):
        nwin = (rbits + w - 1) // w
        table = build_table(C, hs, w, nwin, seg_len)
        ones = sum(1 << (w * i) for i in range(nwin)) & ((1 << rbits) - 1)     # every window 0...01
        rs = [0, 1, (1 << rbits) - 1, ones, rng.getrandbits(rbits), rng.getrandbits(rbits)]
        ms = [0, n - 1, rng.randrange(n), 1, rng.getrandbits(64), rng.randrange(n)]
        for r, m in zip(rs, ms):
            c = encrypt(C, table, w, nwin, r, m)
            assert c == pow(hs, r, n * n) * (1 + n * m) % (n * n)
            assert c == opk.encrypt([m], [r])[0]


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_lazy_sum_bound_of_the_masked_product(bits):
    """The worst case pushed through the kernels' own summation (lazy_sum / wave_sum above, the code encrypt() runs): 2048
    steps -- more than the masked product ever walks (w = 1 and a 2048-bit r) --, every beta with ALL-ONES limbs over the
    whole width of n (2^bits - 1: above any canonical beta), m = n - 1.  The limbs must stay inside 32 bits and below
    3 * 2^29 between carry rounds, nothing may leave the top lane, m + S must stay below R / 4, and the Montgomery product by
    gm must bring it below 2n -- with the key's real R, and with the smallest headroom a split form may have (R = 2^37 n:
    the limbs the sum occupies are the same, only the bound on the value moves)."""
    n, _ = keys()[bits]
    C = Ctx(n, bits)
    steps = 2048
    worst = (1 << bits) - 1
    assert worst >= n - 1 and all(v == MASK for v in C.limbs(worst)[:bits // LB])
    for count in (steps, steps - 1):                       # the last step a carry round, or a plain addition
        betas = [worst] * count
        for mv in (lazy_sum(C, betas, n - 1), wave_sum(C, betas, n - 1)):
            total = C.num(mv)
            assert total == count * worst + n - 1
            assert 4 * total < C.R and 4 * total < (1 << 37) * n
            u = C.M(total, C.gm)
            assert u < 2 * n
            assert total * n // ((1 << 37) * n) + n < 2 * n        # the same product under R = 2^37 n
            assert C.M(u, 2 * C.P - 1) < 2 * n                     # and the second one, by the largest a part
