"""The one-lane CRT decrypt on balanced limbs with the Karatsuba split of its single products (csrc/hensel_ps_bal.hpp,
PGPU_PSB_KARATSUBA: a2*b of every pair squaring and a*c of every pair product of hensel_decrypt_psb_kernel<36,29> in
3 * 18^2 limb products) against pow on the oracle, every plaintext, and bit for bit against the unsigned <38,28> kernel
(pgpu_debug_set_ps_balanced(0): code the split does not touch), the masked table policy and both table forms
(pgpu_debug_set_ps_odd_table(0/1)): the two half-width exponentiations of PrivateKey::decryptCRT, ipcl/pri_key.cpp:114-157.
The one-lane form is forced (pgpu_debug_set_ps_decrypt(2)).  Counts 1, 63, 65 and 130: a lone element, a wavefront short of
one lane, the clamped tail lanes of a second wavefront pair, and a third pair on the other side.  Keys: ISO 2048 bits, the two
made keys of tests/test_gpu_ps_odd_table.py (zero digits; even top digits) and the 2051-bit key (the last width of the
(4,18) pair rows, primes of unequal top limbs).  Ciphertexts: uploaded word rows and the rows written by every producer of
resident rows -- the ciphertext product, CT + PT, CT x PT, the negation and, where the key has hs, the DJN encrypt --, among
them the non-encryptions 1, n + 1 and n^2 - 1.  The arithmetic is modelled in tests/test_ps_karatsuba_model.py."""
import functools
import random

import pytest

from test_gpu_key_widths import KEYS, _q3, djn_hs
from test_gpu_ps_odd_table import _key as _made_key
from test_gpu_ps_odd_table import _vectors as _made_vectors
from test_gpu_round4 import Res

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 65, 130)
NAMES = ("iso", "zero-digit", "even-top", 2051)
FORMS = ("odd", "half-squared", "masked")


@functools.lru_cache(maxsize=None)
def _key(name):
    """(p, q, hs or None)"""
    if name == 2051:
        return KEYS[2051] + (djn_hs(2051),)
    return _made_key(name)


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """(ciphertexts, the oracle's plaintexts) for the largest count, computed once per key: every count takes a prefix.
    n^2 - 1, 1 and n + 1 come first, then two encryptions, then values that are no encryptions"""
    if name != 2051:
        return _made_vectors(name)
    from oracle import paillier_oracle as orc
    p, q, _ = _key(name)
    n = p * q
    rng = random.Random(str(name))
    enc = [(1 + n * rng.randrange(n)) * pow(rng.randrange(2, n), n, n * n) % (n * n) for _ in range(2)]
    raw = [n * n - 1, 1, n + 1] + enc + [rng.randrange(1, n * n) for _ in range(max(COUNTS) - 5)]
    return raw, orc.PrivateKey(n, p, q).decrypt(raw)


def _restore(L, odd):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_ps_odd_table(odd)
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_ps_balanced(1)
    _capi.check(L.pgpu_set_table_gather_policy(0))
    _capi.check(L.pgpu_set_batch_lane(0))


def _set_form(L, bal, form):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_ps_balanced(bal)
    _capi.check(L.pgpu_set_table_gather_policy(1 if form == "masked" else 0))
    L.pgpu_debug_set_ps_odd_table(0 if form == "half-squared" else 1)


@pytest.mark.parametrize("name,count", [(name, count) for name in NAMES for count in COUNTS])
def test_against_oracle_unsigned_kernel_table_forms_and_masked_policy(engine, name, count):
    p, q, hs = _key(name)
    n = p * q
    bits = n.bit_length()
    nw = (bits + 63) // 64
    raw, want = (v[:count] for v in _vectors(name))
    sk = engine.PrivateKey(p, q)
    pk = engine.PublicKey(n, bits, hs=hs)
    R = Res()
    L = R.L
    was = L.pgpu_debug_set_ps_odd_table(1)
    try:
        rng = random.Random(count)
        up = R.up(raw, 2 * nw)
        pm = [n - 1, 0, 1] + [rng.randrange(n) for _ in range(count)]
        pm = pm[:count]
        e = rng.getrandbits(40) | 1
        # D is a homomorphism of the units modulo n^2 into the integers modulo n: every row below is a unit
        sources = {"words": (up, want),
                   "product": (R.op(L.pgpu_batch_ct_add, pk._h, up, R.up([1], 2 * nw)), want),
                   "plus plain": (R.op(L.pgpu_batch_ct_add_plain, pk._h, up, R.up(pm, nw)), [(a + b) % n for a, b in zip(want, pm)]),
                   "times plain": (R.op(L.pgpu_batch_ct_mul, pk._h, up, R.up([e], 1), 40), [a * e % n for a in want]),
                   "negation": (R.op(L.pgpu_batch_ct_negate, pk._h, up), [-a % n for a in want])}
        if hs is not None:
            m = ([0, n - 1, 1] + [rng.randrange(n) for _ in range(count)])[:count]
            rw = ((bits + 1) // 2 + 63) // 64
            r = [rng.getrandbits(64 * rw) for _ in range(count)]
            sources["encrypt"] = (R.op(L.pgpu_batch_encrypt, pk._h, R.up(m, nw), R.up(r, rw), 64 * rw), m)
        L.pgpu_debug_set_ps_decrypt(2)
        for src, (h, expect) in sources.items():
            got = {}
            for bal in (1, 0):
                for form in FORMS:
                    _set_form(L, bal, form)
                    assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0) == (4, 1, 36 if bal else 38)
                    got[bal, form] = R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, h))
            for key, g in got.items():
                assert g == expect, (src, key)                               # every result against the oracle / the plaintexts
            first = got[0, "half-squared"]
            assert all(g == first for g in got.values()), src                # ... and bit-equal among the kernels and forms
    finally:
        _restore(L, was)
        R.close()


def test_two_lanes_at_once(engine):
    """two resident batches of 130 in flight on two batch lanes, three rounds (the first starts beside an idle neighbour):
    beside a busy lane a launch claims whole CUs and runs the build that owns the register file (<36,29,1>)"""
    from pailliercryptolib_amd import _capi
    p, q, hs = _key("iso")
    n, nw, count = p * q, 32, 130
    raw, want = _vectors("iso")
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    R = Res()
    L = R.L
    was = L.pgpu_debug_set_ps_odd_table(1)
    try:
        assert L.pgpu_batch_lanes() >= 2
        L.pgpu_debug_set_ps_decrypt(2)
        sets = []
        for ln in range(2):
            rng = random.Random(70 + ln)
            m = ([0, 1, n - 1] + [rng.randrange(n) for _ in range(count)])[:count]
            _capi.check(L.pgpu_set_batch_lane(ln))
            rows = raw if ln == 0 else raw[::-1]
            sets.append((m, R.up(m, nw), R.up([rng.getrandbits(1024) for _ in range(count)], nw // 2), R.up(rows, 2 * nw)))
        outs, raw_outs = [None] * 2, [None] * 2
        for _ in range(3):
            for ln in range(2):
                _capi.check(L.pgpu_set_batch_lane(ln))
                ct = R.op(L.pgpu_batch_encrypt, pk._h, sets[ln][1], sets[ln][2], 1024)
                outs[ln] = R.op(L.pgpu_batch_decrypt_crt, sk._h, ct)
                raw_outs[ln] = R.op(L.pgpu_batch_decrypt_crt, sk._h, sets[ln][3])
        _capi.check(L.pgpu_set_batch_lane(0))
        _capi.check(L.pgpu_synchronize())
        for ln in range(2):
            assert R.down(outs[ln]) == sets[ln][0], ln
            assert R.down(raw_outs[ln]) == (want if ln == 0 else want[::-1]), ln
    finally:
        _restore(L, was)
        R.close()
