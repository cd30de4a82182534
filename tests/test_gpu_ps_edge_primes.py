"""The CRT decrypt kernels that run one exponentiation per lane (csrc/hensel_ps.hpp: hensel_decrypt_ps_kernel<19,29>, <38,28>,
<56,28>; csrc/hensel_ps_bal.hpp: hensel_decrypt_psb_kernel<36,29>) and per wavefront (csrc/hensel_wave.hpp:
hensel_decrypt_wave_kernel<K,LB,WIDEQ>) at the EDGES of the prime widths they serve: tests/golden/ps_edge_primes.json
(gen_ps_edge_primes.py) and the tight 3072-bit key of primes_worst_headroom.json.  Which kernel a key gets follows from the bit
length B of its larger prime (capi_keys.inc: build_hensel; capi.cpp: decrypt_on):

  class   one-lane (K, LB)            serves B       R / P can fall to              one-wavefront form: 32-bit digits when
  1024    (19, 29)                    490 .. 518     16 at B = 518,  k = 2^29 - 1   B <= 512
  2048    (38, 28), balanced (36, 29) 1005 .. 1032   16 at B = 1032, k = 2^28 - 1   B <= 1026
  3072    (56, 28)                    1509 .. 1536   16 at B = 1536, k = 2^28 - 1   B <= 1530

The form every key must get is written out below (FORMS) and asserted before every launch: a fall-back to another kernel
fails the test.  Per key: the forced one-lane kernels (balanced and unsigned limbs x odd-power / half-squared / masked table),
the forced one-wavefront kernel with indexed and with masked table access -- the digit form it took read back from
pgpu_debug_last_wave_wide --, and the paired form as the answer of a kernel that shares none of this code.  Ciphertexts: uploaded
word rows (1, n + 1, n^2 - 1, two encryptions, random units) and the rows of every producer of resident rows: CT + CT, CT + PT,
CT x PT, the negation and the DJN encrypt.  Every result at every index against oracle/paillier_oracle.py (pow) or the known
plaintexts, and bit for bit among the forms: the two half-width exponentiations of PrivateKey::decryptCRT,
ipcl/pri_key.cpp:114-157.  The arithmetic at these primes is modelled in tests/test_hensel_model.py (lane model of the
one-wavefront form, bounds of the one-lane form), tests/test_ps_balanced_model.py, test_ps_karatsuba_model.py and
test_ps_odd_table_model.py."""
import functools
import json
import math
import os
import random

import pytest

from test_gpu_key_widths import _q3
from test_gpu_round4 import Res

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

# name -> (limbs of the one-lane kernel on unsigned limbs, on balanced limbs or None, limbs of the one-wavefront kernel, its
# digit form: True = 32-bit digits), from the table above and the bit length of the key's larger prime
FORMS = {
    "c1024-low": (19, None, 19, True),             # B = 490
    "c1024-tight-wide": (19, None, 19, True),      # B = 512: 29 * 19 - (512 + 29) = 10
    "c1024-tight": (19, None, 19, False),          # B = 518: wave<19,29,false>
    "c2048-low": (38, 36, 38, True),               # B = 1005
    "c2048-tight": (38, 36, 38, False),            # B = 1032
    "c2048-uneven-top": (38, 36, 38, False),       # B = 1032 beside 1018 bits
    "c2048-uneven-low": (38, 36, 38, True),        # B = 1005 beside 980 bits
    "c2048-heavy": (38, 36, 38, True),             # B = 1024
    "c3072-low": (56, None, 56, True),             # B = 1509: wave<56,28,true>
    "c3072-tight-wide": (56, None, 56, True),      # B = 1530: 28 * 56 - (1530 + 28) = 10
    "worst-headroom": (56, None, 56, False),       # B = 1536
}
# limbs per half of the key's pair rows (csrc/policy.hpp: pair_form_for_bits)
PAIR_L2 = {"c1024-low": 38, "c1024-tight-wide": 38, "c1024-tight": 38, "c2048-low": 72, "c2048-tight": 112, "c2048-uneven-top": 72,
           "c2048-uneven-low": 72, "c2048-heavy": 72, "c3072-low": 112, "c3072-tight-wide": 112, "worst-headroom": 112}
TABLES = ("odd", "half-squared", "masked")


def lane_counts(name):
    """a lone element, the clamped tail lanes of a second wavefront pair, a third pair (the 3072-bit class: two pairs)"""
    return (1, 65) if FORMS[name][0] == 56 else (1, 65, 130)


WAVE_COUNTS = (1, 37)


@functools.lru_cache(maxsize=None)
def _key(name):
    """(p, q, hs): hs = (-x^2)^n mod n^2 as pub_key.cpp:40-49 forms it, x seeded"""
    if name == "worst-headroom":
        k = json.load(open(os.path.join(GOLD, "primes_worst_headroom.json")))
    else:
        k = {c["name"]: c for c in json.load(open(os.path.join(GOLD, "ps_edge_primes.json")))["cases"]}[name]
    p, q = int(k["p"], 16), int(k["q"], 16)
    n = p * q
    x = random.Random("hs " + name).randrange(2, n)
    return p, q, pow(n * n - x * x % (n * n), n, n * n)


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """(ciphertexts, the oracle's plaintexts) for the largest count of the key, computed once: every count takes a prefix.
    1, n + 1 and n^2 - 1 come first, then two encryptions, then random values; every one a unit modulo n^2"""
    from oracle import paillier_oracle as orc
    p, q, _ = _key(name)
    n = p * q
    rng = random.Random("ct " + name)
    enc = [(1 + n * rng.randrange(n)) * pow(rng.randrange(2, n), n, n * n) % (n * n) for _ in range(2)]
    raw = [1, n + 1, n * n - 1] + enc + [rng.randrange(1, n * n) for _ in range(max(lane_counts(name) + WAVE_COUNTS) - 5)]
    assert all(math.gcd(c, n) == 1 for c in raw)
    return raw, orc.PrivateKey(n, p, q).decrypt(raw)


def _restore(L, odd):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_ps_odd_table(odd)
    L.pgpu_debug_set_hensel(1)
    L.pgpu_debug_set_seq_decrypt(4)
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_wave_decrypt(1)
    L.pgpu_debug_set_ps_balanced(1)
    _capi.check(L.pgpu_set_table_gather_policy(0))


def _sources(R, name, count, engine):
    """{source: (resident batch, the plaintexts it must decrypt to)} and the private key"""
    p, q, hs = _key(name)
    n = p * q
    bits = n.bit_length()
    nw, mw, rw = (bits + 63) // 64, bits // 64, ((bits + 1) // 2 + 63) // 64
    raw, want = (v[:count] for v in _vectors(name))
    sk = engine.PrivateKey(p, q)
    pk = engine.PublicKey(n, bits, hs=hs)
    L = R.L
    rng = random.Random(name + str(count))
    up = R.up(raw, 2 * nw)
    pm = ([n - 1, 0, 1] + [rng.randrange(n) for _ in range(count)])[:count]
    e = rng.getrandbits(40) | 1
    m = ([min(n - 1, (1 << (64 * mw)) - 1), 0, 1] + [rng.getrandbits(64 * mw) % n for _ in range(count)])[:count]
    r = [rng.getrandbits(64 * rw) for _ in range(count)]
    # D is a homomorphism of the units modulo n^2 into the integers modulo n: every row below is a unit
    src = {"words": (up, want),
           "pair rows": (R.op(L.pgpu_batch_ct_add, pk._h, up, R.up([1], 2 * nw)), want),
           "plus plain": (R.op(L.pgpu_batch_ct_add_plain, pk._h, up, R.up(pm, nw)), [(a + b) % n for a, b in zip(want, pm)]),
           "times plain": (R.op(L.pgpu_batch_ct_mul, pk._h, up, R.up([e], 1), 40), [a * e % n for a in want]),
           "negation": (R.op(L.pgpu_batch_ct_negate, pk._h, up), [-a % n for a in want]),
           "encrypt": (R.op(L.pgpu_batch_encrypt, pk._h, R.up(m, mw), R.up(r, rw), 64 * rw), m)}
    assert L.pgpu_batch_row_limbs(src["words"][0]) == 0
    for s in ("pair rows", "times plain", "encrypt"):
        assert L.pgpu_batch_row_limbs(src[s][0]) == 2 * PAIR_L2[name], s
    return sk, src


def _paired(R, sk, src, count):
    """every source through the paired form: a kernel that shares no code with the forms under test"""
    L = R.L
    L.pgpu_debug_set_hensel(1)
    L.pgpu_debug_set_seq_decrypt(0)
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_wave_decrypt(0)
    out = {}
    for s, (h, expect) in src.items():
        assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0)[0] == 1
        out[s] = R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, h))
        assert out[s] == expect, s
    L.pgpu_debug_set_seq_decrypt(4)
    return out


@pytest.mark.parametrize("name,count", [(name, count) for name in FORMS for count in lane_counts(name)])
def test_one_lane_kernels_at_the_edge_primes(engine, name, count):
    from pailliercryptolib_amd import _capi
    unsigned, balanced, _, _ = FORMS[name]
    R = Res()
    L = R.L
    was = L.pgpu_debug_set_ps_odd_table(1)
    try:
        sk, src = _sources(R, name, count, engine)
        ref = _paired(R, sk, src, count)
        L.pgpu_debug_set_ps_decrypt(2)
        for s, (h, expect) in src.items():
            for bal in ((1, 0) if balanced else (0,)):
                for table in TABLES:
                    L.pgpu_debug_set_ps_balanced(bal)
                    _capi.check(L.pgpu_set_table_gather_policy(1 if table == "masked" else 0))
                    L.pgpu_debug_set_ps_odd_table(0 if table == "half-squared" else 1)
                    assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0) == (4, 1, balanced if bal else unsigned), (s, bal, table)
                    got = R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, h))
                    assert got == expect, (s, bal, table)                    # the oracle / the plaintexts, every index
                    assert got == ref[s], (s, bal, table)                    # ... and the paired form, bit for bit
    finally:
        _restore(L, was)
        R.close()


@pytest.mark.parametrize("name,count", [(name, count) for name in FORMS for count in WAVE_COUNTS])
def test_one_wavefront_kernel_at_the_edge_primes(engine, name, count):
    from pailliercryptolib_amd import _capi
    _, _, limbs, wide = FORMS[name]
    R = Res()
    L = R.L
    was = L.pgpu_debug_set_ps_odd_table(1)
    try:
        sk, src = _sources(R, name, count, engine)
        ref = _paired(R, sk, src, count)
        L.pgpu_debug_set_wave_decrypt(2)
        for s, (h, expect) in src.items():
            for gather in (0, 1):
                _capi.check(L.pgpu_set_table_gather_policy(gather))
                assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0) == (5, 64, limbs), (s, gather)
                got = R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, h))
                assert L.pgpu_debug_last_wave_wide() == (1 if wide else 0), (s, gather)
                assert got == expect, (s, gather)
                assert got == ref[s], (s, gather)
    finally:
        _restore(L, was)
        R.close()
