"""The lazy bounds of the pair arithmetic at the TIGHT keys of tests/golden/key_widths.json (CPU test, no GPU; a sibling of
test_hensel_model.py, whose pair product it reuses).  At the upper edge of a pair-row class -- n of 1065, 2051, 3211 bits with
k = -n^-1 mod 2^29 = 2^29 - 1 -- the loop modulus P = n k is as close to R / 256 as a key can bring it, R = 2^(29 L2), so
whatever the kernels' comments promise "for R >= 2^8 P" is promised with nothing to spare.  Restated in Python integers:

  * the n^2-domain pair product (csrc/hensel.hpp: pairmul -- "lazy: inputs < 8P -> outputs < 2P") from worst-case operands;
  * the entry from words in chunks (hensel.hpp: pair_from_words; capi_keys.inc: make_pub_form -- cw, nchunks and the
    R^2 2^(64 cw i) ladder), from n^2 - 1 and from all-ones rows: every chunk below 2P, the sum below the 8P a product takes;
  * the column sums of a product on relaxed limbs (hensel.hpp: "a column of half B receives 3K products (+ relaxed limbs):
    must stay below 2^64"; mont_core.hpp: montmul_finish -- limb 0 of a lane below 2^30, limb 1 below 2^29 + 2^7);
  * the private side's entry from pair rows (hensel.hpp: hensel_decrypt_kernel, A.ct_pair; capi_keys.inc: build_hensel_set
    -- pchunks, pchunk_limbs, kappa, the R^2 Rn^-1 2^(29 pchunk_limbs i) ladder) for the forms such a key has."""
import json
import os

import pytest

from test_hensel_model import LB, pmul, redc, to_pair, val

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CLASS = {1065: (2, 19), 2051: (4, 18), 3211: (8, 14)}                    # (G, K) of the class whose upper edge the key sits on
TIGHT = [c for c in json.load(open(os.path.join(GOLD, "key_widths.json")))["cases"] if c["tight"]]
# the split forms of CRT decrypt (csrc/launch.hpp: hensel_has, default build)
HENSEL = {2: (10, 19), 4: (5, 10, 14), 8: (3, 5, 7)}


def key(case):
    p, q = int(case["p"], 16), int(case["q"], 16)
    return p, q, p * q


def pub(case):
    p, q, n = key(case)
    G, K = CLASS[case["bits"]]
    L2 = G * K
    k = (-pow(n, -1, 1 << LB)) % (1 << LB)
    P, R = n * k, 1 << (LB * L2)
    return n, k, P, R, L2, K


def test_fixture_has_the_three_tight_keys():
    assert sorted(c["bits"] for c in TIGHT) == [1065, 2051, 3211]
    for c in TIGHT:
        p, q, n = key(c)
        assert n.bit_length() == c["bits"] and p % (1 << 28) == 1 and q % (1 << 28) == 1
        n_, k, P, R, L2, K = pub(c)
        assert k == (1 << LB) - 1 and P % (1 << LB) == (1 << LB) - 1            # the largest multiplier; unit quotient digits
        assert 256 * P <= R < 257 * P                                           # R = 2^8 P and next to nothing more
        assert LB * L2 == c["bits"] + LB + 8                                    # one more bit of n and the class ends


@pytest.mark.parametrize("case", TIGHT, ids=lambda c: str(c["bits"]))
def test_pair_product_bounds_at_the_tight_keys(case):
    n, k, P, R, L2, K = pub(case)
    top, lazy = 8 * P - 1, 2 * P - 1
    worst = [(top, top), (top, 0), (0, top), (lazy, lazy), (lazy, 0), (0, lazy), (lazy, P), (P - 1, lazy), (1, 0), (0, 0)]
    for x in worst:
        for y in worst:
            t = pmul(x, y, P, R)                                                # (asserts t, w < 2P)
            assert val(t, P) == val(x, P) * val(y, P) * pow(R, -1, P * P) % (P * P)
    # a chain from the worst pair: squarings and products by it settle below 2P from the first product on
    x = (top, top)
    for _ in range(12):
        x = pmul(x, x, P, R)
        x = pmul(x, (top, top), P, R)
    # ciphertext values at the ends of the range, as pairs of c R
    for c in (n * n - 1, 1, n, n + 1, n * n - n):
        a = to_pair(c * R, P)
        assert a[0] < P and a[1] < P
        s = pmul(a, a, P, R)
        assert val(s, P) % (n * n) == c * c * R % (n * n)


@pytest.mark.parametrize("case", TIGHT, ids=lambda c: str(c["bits"]))
def test_entry_from_words_in_chunks_at_the_tight_keys(case):
    n, k, P, R, L2, K = pub(case)
    nw = (n.bit_length() + 63) // 64
    cw = min(nw, n.bit_length() // 64)                                          # make_pub_form
    nch = (2 * nw + cw - 1) // cw
    assert cw == nw - 1 and nch == 3                                            # n does not fill its words: a third chunk
    conv = [to_pair((R * R % (P * P)) * (1 << (64 * cw * i)), P) for i in range(nch)]
    for c in (n * n - 1, (1 << (128 * nw)) - 1, 1 << (64 * cw), (1 << (64 * cw)) - 1, 0):    # (a row may hold any words)
        acc = (0, 0)
        for i in range(nch):
            z = (c >> (64 * cw * i)) & ((1 << (64 * cw)) - 1)
            assert z < 2 * P                                                    # (z, 0) is a lazy pair
            t = pmul((z, 0), conv[i], P, R)
            acc = (acc[0] + t[0], acc[1] + t[1])
        assert acc[0] < 8 * P and acc[1] < 8 * P and 8 * P < R                   # what the next product takes, and the limbs hold
        assert val(acc, P) == c * R % (P * P)
        pmul(acc, acc, P, R)


@pytest.mark.parametrize("G,K", sorted(set(CLASS.values())) + [(8, 9)])
def test_column_sums_on_relaxed_limbs(G, K):
    """Upper bound of one 64-bit column accumulator of half B over its lifetime: K products of the lane's multiplicand
    limbs with rows of c, K with rows of a (a squaring: K with its own limbs doubled instead), K quotient digits times limbs
    of P, and the hand-over from the neighbouring lane.  Relaxed limbs: per lane limb 0 below 2^30, limb 1 below
    2^29 + 2^7, the others below 2^29; a row is a relaxed limb as well."""
    relaxed = [(1 << 30) - 1, (1 << 29) + (1 << 7) - 1] + [(1 << 29) - 1] * (K - 2)
    canon = (1 << 29) - 1

    def column(mult, rows):                 # the worst column c: limb j meets row (c - j) mod K -- in this block or the one before
        return max(sum(mult[j] * rows[(c - j) % K] for j in range(K)) for c in range(K))

    product = 2 * column(relaxed, relaxed)                                         # b c + d a
    squaring = column([2 * v for v in relaxed], relaxed)                            # 2 a b
    reduction = K * canon * canon                                                  # unit quotient digits below 2^29, P canonical
    handover = 1 << 36                                                             # (mont_core.hpp: a lane's carry-out)
    assert 3 * K + 6 < 64                                                          # the kernel's static_assert
    print(G, K, "worst column / 2^58:", (max(product, squaring) + reduction + handover) / 2.0 ** 58)
    assert max(product, squaring) + reduction + handover < 1 << 64


def private_forms(p, q):
    """(H, K) per lane count as capi_keys.inc: build_hensel picks them"""
    need = max(p.bit_length(), q.bit_length()) + LB + 8
    out = []
    for H in (8, 4, 2):
        for K in range(1, 20):
            if K in HENSEL[H] and LB * H * K >= need:
                out.append((H, K))
                break
    return out


@pytest.mark.parametrize("case", TIGHT, ids=lambda c: str(c["bits"]))
def test_private_entry_from_pair_rows_at_the_tight_keys(case):
    p, q, n = key(case)
    n_, kn, Pn, Rn, l2, _ = pub(case)
    forms = private_forms(p, q)
    if case["bits"] == 3211:
        assert forms == []                  # primes of 1606 bits: beyond (4,14) / (8,7); resident rows decrypt as words
        return
    assert forms
    for H, K in forms:
        L2 = H * K
        R = 1 << (LB * L2)
        pchunks = -(-l2 // L2)                                                   # build_hensel_set
        plimbs = -(-l2 // pchunks)
        assert pchunks * plimbs >= l2 and plimbs <= L2
        for pr, other in ((p, q), (q, p)):
            k = (-pow(pr, -1, 1 << LB)) % (1 << LB)
            assert k == (1 << LB) - 1
            P = pr * k
            assert R >= 256 * P
            kappa = other * kn * pow(k, -1, pr) % pr
            R2n = R * R * pow(Rn, -1, P * P) % (P * P)
            pconv = [to_pair(R2n * (1 << (LB * plimbs * i)), P) for i in range(pchunks)]
            pcb = [kappa * (1 << (LB * plimbs * i)) * R * R * pow(Rn, -1, pr) % pr for i in range(pchunks)]
            sat = (1 << (LB * l2)) - 1                                           # every limb of the row saturated
            for a, b in ((2 * Pn - 1, 2 * Pn - 1), (sat, sat), (Pn - 1, 0), (0, 2 * Pn - 1), to_pair((n * n - 1) * Rn, Pn), (0, 0)):
                acc = (0, 0)
                for i in range(pchunks):
                    za = (a >> (LB * plimbs * i)) & ((1 << (LB * plimbs)) - 1)
                    zb = (b >> (LB * plimbs * i)) & ((1 << (LB * plimbs)) - 1)
                    assert za < R and zb < R
                    t, q1 = redc(za * pconv[i][0], P, R)                          # (z, 0) (x) pconv[i]: the d a product and q
                    w, _ = redc(za * pconv[i][1] + q1, P, R)
                    tb, _ = redc(zb * pcb[i], P, R)                               # half-width, added to half B
                    assert t < 2 * P and w < 2 * P and tb < 2 * P
                    acc = (acc[0] + t, acc[1] + w + tb)
                assert acc[0] < 8 * P and acc[1] < 8 * P and 8 * P < R
                c_rn = (a - Pn * b) % (n * n)                                    # the row's value: c Rn mod n^2
                assert val(acc, P) % (pr * pr) == c_rn * pow(Rn, -1, pr * pr) * R % (pr * pr)
                pmul(acc, acc, P, R)
