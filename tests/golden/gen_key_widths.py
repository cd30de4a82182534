"""Generates tests/golden/key_widths.json: Paillier primes whose n = p q has a bit length OFF the standard key sizes -- in
the middle of a pair-row class, at its first width and at its last (csrc/policy.hpp: pair_form_for_bits).  Data only (the
inputs of tests/test_gpu_key_widths.py and tests/test_key_width_bounds.py; expected values come from Python integers and
the oracle at test time); deterministic.

The three keys at the upper edge of a class (1065, 2051, 3211 bits) are TIGHT: p, q == 1 (mod 2^29) -- so also 1 modulo
2^28 -- and n as close below 2^width as the search finds.  Then k = -n^-1 mod 2^29 = 2^29 - 1, the largest multiplier of
the split form, and the loop modulus P = n k sits just below 2^(width + 29): R = 2^(29 L2) is 2^8 P and no more, the least
headroom the pair rows of the class ever have (L2 = 38, 72, 112 limbs per half).  The same holds for each prime on the
private side (k = 2^29 - 1 for 29-bit limbs, 2^28 - 1 for 28-bit ones).  R / P is printed and kept in the `note` field.

The 2052-bit key is UNEVEN (a 1021- and a 1031-bit prime: a ciphertext enters the private split form in chunks of 15
words, not 17).  The mid-class widths 1088, 1536 and 2560 are whole words, where a private key refuses primes of different
width (q^2 must fit the words of n), so the uneven pair sits at the nearest width that has room.
usage: python tests/golden/gen_key_widths.py"""
import json
import os
import random

import gen_primes

LB = 29
# width -> (limbs per half of the class's pair rows or 0, tight, prime widths, purpose)
CASES = [
    (512, 38, False, (256, 256), "smallest (2,19) user, most zero top limbs"),
    (1065, 38, True, None, "upper edge of (2,19)"),
    (1088, 72, False, (544, 544), "between the (2,19) edge and the first width (4,10) cannot hold: (4,18) rows"),
    (1124, 72, False, (562, 562), "first width whose smallest 4-lane form is (4,18)"),
    (1536, 72, False, (768, 768), "mid (4,18)"),
    (2051, 72, True, None, "upper edge of (4,18)"),
    (2052, 112, False, (1021, 1031), "first (8,14) width; uneven primes"),
    (2560, 112, False, (1280, 1280), "mid (8,14)"),
    (3211, 112, True, None, "upper edge of (8,14); primes too wide for the private split forms of the default build"),
    (3212, 0, False, (1606, 1606), "first width without pair rows in the default build"),
]


def tight_pair(width, rng):
    """p just below 2^ceil(width/2), q the largest prime with p q < 2^width, both == 1 (mod 2^29)"""
    step = 1 << LB
    pb = (width + 1) // 2
    c = (1 << pb) - step + 1
    while not gen_primes.is_prime(c, rng):
        c -= step
    p = c
    c = ((1 << width) // p - 1) // step * step + 1
    while not gen_primes.is_prime(c, rng):
        c -= step
    return p, c


def main():
    out = []
    for width, l2, tight, pq_bits, purpose in CASES:
        rng = random.Random(width)
        if tight:
            p, q = tight_pair(width, rng)
        else:
            p, q = gen_primes.prime(pq_bits[0], rng), gen_primes.prime(pq_bits[1], rng)
        n = p * q
        assert n.bit_length() == width and p != q, (width, n.bit_length())
        note = purpose
        if tight:
            k = (-pow(n, -1, 1 << LB)) % (1 << LB)
            assert p % (1 << 28) == 1 and q % (1 << 28) == 1 and k == (1 << LB) - 1
            ratio = (1 << (LB * l2)) / (n * k)
            assert 256 <= ratio < 257
            note += "; p, q == 1 mod 2^29, k = 2^29 - 1, R / P = 2^(29*%d) / (n k) = %.9f" % (l2, ratio)
            print(width, "R/P =", "%.9f" % ratio, "2^width - n has", ((1 << width) - n).bit_length(), "bits")
        p, q = min(p, q), max(p, q)
        out.append({"bits": width, "tight": tight, "p_bits": p.bit_length(), "q_bits": q.bit_length(),
                    "p": hex(p)[2:], "q": hex(q)[2:], "note": note})
        print(width, p.bit_length(), q.bit_length())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "key_widths.json")
    json.dump({"generator": "gen_key_widths.py", "cases": out}, open(path, "w"), indent=1)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
