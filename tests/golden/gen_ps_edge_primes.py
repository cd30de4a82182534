"""Generates tests/golden/ps_edge_primes.json: Paillier primes at the EDGES of what the one-lane and one-wavefront CRT
decrypt kernels serve (csrc/hensel_ps.hpp, hensel_ps_bal.hpp, hensel_wave.hpp).  Which kernel a key gets, and with how
little headroom, follows from the bit length B of its larger prime and from k = -p^-1 mod 2^lb (capi_keys.inc:
build_hensel picks K with lb K >= B + lb + 4 > lb (K - 1); capi.cpp: decrypt_on takes 32-bit quotient digits in the
one-wavefront form where lb K - (B + lb) >= 10):

  class   form (K, lb)            serves B       R / P can fall to                 32-bit digits when
  1024    (19, 29)                490 .. 518     16 at B = 518,  k = 2^29 - 1      B <= 512
  2048    (38, 28), bal. (36, 29) 1005 .. 1032   16 at B = 1032, k = 2^28 - 1      B <= 1026
  3072    (56, 28)                1509 .. 1536   16 at B = 1536, k = 2^28 - 1      B <= 1530

TIGHT: p, q == 1 (mod 2^lb), the first two primes found stepping down by 2^lb from 2^B - 2^lb + 1.  Then k = 2^lb - 1 and
the loop modulus P = p k sits just below 2^(B + lb): the largest P, the least R / P, and limbs of P that are nearly all
ones.  LOW: the first two primes above 2^(B - 1) at the narrowest B of a class (zero top limbs).  HEAVY: two 1024-bit primes
whose balanced 29-bit limbs 0 .. 34 all have magnitude >= 2^28 - 2^16 (limbs +-(2^28 - 1) of alternating sign below a top limb
that makes the value 1024 bits long, the low limb stepped by 2 until the value is prime).  UNEVEN: primes of different widths;
a private key refuses a pair whose larger square does not fit the words of n (capi_keys.inc: pgpu_privkey_create), so the
narrow side of `c2048-uneven-low` is the narrowest the library takes beside its 1005-bit prime, searched from 973 bits up.
The tight 3072-bit key of B = 1536 is primes_worst_headroom.json (gen_worst_headroom.py).

Data only (inputs of tests/test_gpu_ps_edge_primes.py and of the CPU models; expected values come from Python integers and
the oracle at test time); deterministic.  usage: python tests/golden/gen_ps_edge_primes.py"""
import json
import os
import random

import gen_primes

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ps_edge_primes.json")


def form_for(B):
    """(K, lb) of the one-lane / one-wavefront set: build_hensel tries 28-bit limbs first; compiled (38,28), (56,28), (19,29)"""
    for lb in (28, 29):
        K = -(-(B + lb + 4) // lb)
        if (K, lb) in ((38, 28), (56, 28), (19, 29)):
            return K, lb
    raise AssertionError(B)


def tight(B, lb, rng):
    out, j = [], 1
    while len(out) < 2:
        c = (1 << B) - (j << lb) + 1
        j += 1
        if gen_primes.is_prime(c, rng):
            assert c.bit_length() == B and (-pow(c, -1, 1 << lb)) % (1 << lb) == (1 << lb) - 1
            out.append(c)
    return out[1], out[0]


def low(B, rng):
    out, c = [], (1 << (B - 1)) + 1
    while len(out) < 2:
        if gen_primes.is_prime(c, rng):
            assert c.bit_length() == B
            out.append(c)
        c += 2
    return out[0], out[1]


def ones_limbs(p, K, lb):
    """limbs of P = p k that are all ones"""
    P = p * ((-pow(p, -1, 1 << lb)) % (1 << lb))
    return sum(1 for j in range(K) if (P >> (lb * j)) & ((1 << lb) - 1) == (1 << lb) - 1)


def balanced_limbs(v, K=36, lb=29):
    out = []
    for _ in range(K):
        r = v & ((1 << lb) - 1)
        if r >= 1 << (lb - 1):
            r -= 1 << lb
        out.append(r)
        v = (v - r) >> lb
    assert v == 0
    return out


def heavy(sign, rng):
    """limbs j = 0 .. 34: sign (-1)^j (2^28 - 1); limb 35 = 2^8, one more where limb 34 is negative (1024 bits either way)"""
    s = [sign * (-1) ** j for j in range(35)]
    top = (1 << 8) + (1 if s[34] < 0 else 0)
    for step in range(1 << 15):
        l0 = s[0] * ((1 << 28) - 1 - 2 * step)
        v = l0 + sum(s[j] * ((1 << 28) - 1) << (29 * j) for j in range(1, 35)) + (top << (29 * 35))
        if gen_primes.is_prime(v, rng):
            bl = balanced_limbs(v)
            assert v.bit_length() == 1024 and all(abs(x) >= (1 << 28) - (1 << 16) for x in bl[:35]) and bl[35] == top
            return v
    raise AssertionError("no prime")


def accepted(p, q):
    """pgpu_privkey_create: p^2 and q^2 must fit the words of n"""
    nw = ((p * q).bit_length() + 63) // 64
    return max(p, q).bit_length() * 2 <= 64 * nw and (max(p, q) ** 2).bit_length() <= 64 * nw


def ratio_note(p, q):
    B = max(p.bit_length(), q.bit_length())
    K, lb = form_for(B)
    r = []
    for v in (p, q):
        P = v * ((-pow(v, -1, 1 << lb)) % (1 << lb))
        r.append(((1 << (lb * K)) << 40) // P / (1 << 40))
    return "R/P = %.8f, %.8f at (%d,%d)" % (r[0], r[1], K, lb)


def main():
    cases = []

    def add(name, p, q, what):
        assert p != q
        p, q = min(p, q), max(p, q)
        assert accepted(p, q), name
        cases.append({"name": name, "bits": (p * q).bit_length(), "p_bits": p.bit_length(), "q_bits": q.bit_length(),
                      "p": hex(p)[2:], "q": hex(q)[2:], "note": what + "; " + ratio_note(p, q)})
        print(name, cases[-1]["bits"], cases[-1]["p_bits"], cases[-1]["q_bits"], cases[-1]["note"])

    p, q = low(490, random.Random(490))
    assert form_for(490) == (19, 29) and 29 * 18 == 489 + 29 + 4      # (489 bits take 18 limbs)
    add("c1024-low", p, q, "narrowest (19,29); zero top limbs")

    p, q = tight(512, 29, random.Random(512))
    assert 29 * 19 - (512 + 29) == 10
    add("c1024-tight-wide", p, q, "wave<19,29,true> at its least R/P, 2^10")

    p, q = tight(518, 29, random.Random(518))
    assert form_for(518) == (19, 29) and 29 * 19 == 518 + 29 + 4
    assert ones_limbs(p, 19, 29) == ones_limbs(q, 19, 29) == 15
    add("c1024-tight", p, q, "one-lane (19,29) and wave<19,29,false> at the least R/P; 15 of 19 limbs of P all ones")

    p, q = low(1005, random.Random(1005))
    assert form_for(1005) == (38, 28) and 28 * 37 == 1004 + 28 + 4
    add("c2048-low", p, q, "narrowest (38,28) and balanced (36,29); (4,18) rows")

    p, q = tight(1032, 28, random.Random(1032))
    assert form_for(1032) == (38, 28) and 28 * 38 == 1032 + 28 + 4
    assert ones_limbs(p, 38, 28) == ones_limbs(q, 38, 28) == 34
    assert sum(1 for x in balanced_limbs(p) if x == 0) >= 30
    add("c2048-tight", p, q, "(38,28) and wave<38,28,false> at the least R/P; (8,14) rows; 34 of 38 limbs of P all ones, balanced limbs nearly all zero")

    rng = random.Random(1018)
    p, q = gen_primes.prime(1018, rng, top2=False), gen_primes.prime(1032, rng, top2=False)
    assert (p.bit_length(), q.bit_length()) == (1018, 1032) and (p * q).bit_length() <= 2051
    add("c2048-uneven-top", p, q, "widest prime on (4,18) rows; q^2 just fits the words of n")

    rng = random.Random(973)
    q = gen_primes.prime(1005, rng, top2=False)
    for pb in range(973, 1006):
        p = gen_primes.prime(pb, rng, top2=False)
        if accepted(p, q):
            break
    assert q.bit_length() == 1005 and p.bit_length() == pb < 1005
    add("c2048-uneven-low", p, q, "the narrowest prime the library takes beside a 1005-bit one (from 973 bits up: q^2 must fit the words of n); zero top limbs on one side")

    rng = random.Random(1024)
    p, q = heavy(1, rng), heavy(-1, rng)
    assert form_for(1024) == (38, 28)
    add("c2048-heavy", p, q, "balanced 29-bit limbs 0..34 of magnitude >= 2^28 - 2^16")

    p, q = low(1509, random.Random(1509))
    assert form_for(1509) == (56, 28) and 28 * 55 == 1508 + 28 + 4 and 28 * 56 - (1509 + 28) >= 10
    add("c3072-low", p, q, "narrowest (56,28); wave<56,28,true>")

    p, q = tight(1530, 28, random.Random(1530))
    assert form_for(1530) == (56, 28) and 28 * 56 - (1530 + 28) == 10
    add("c3072-tight-wide", p, q, "wave<56,28,true> at its least R/P, 2^10")

    with open(OUT, "w") as f:
        json.dump({"generator": "gen_ps_edge_primes.py", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
