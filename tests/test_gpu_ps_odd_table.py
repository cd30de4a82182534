"""The one-lane CRT decrypt on the ODD-POWER window table (csrc/hensel_ps_bal.hpp, csrc/hensel_ps.hpp: entry j = base^(2j-1),
the product of a window placed after w - ctz(digit) of its squarings, the top window an ordinary one from `one`) against
oracle/paillier_oracle, every plaintext -- the table form that ran read back from pgpu_debug_last_ps_table_entries (33
entries against 64 at 6 bits) --, and bit for bit against the half-squared form (pgpu_debug_set_ps_odd_table(0), what
PGPU_PS_ODD_TABLE=0 does for a whole process) and against the masked table policy, which keeps the full table and the fixed
order: the two half-width exponentiations of PrivateKey::decryptCRT, ipcl/pri_key.cpp:114-157.  The one-lane form is forced
(pgpu_debug_set_ps_decrypt(2)).  Counts 1, 63, 65 and 130: a lone element, a wavefront short of one lane, the clamped tail
lanes of a second wavefront pair, and a third pair, which is a second workgroup.  Keys: ISO 2048 bits (K = 36 balanced and
K = 38 unsigned limbs), the seeded 1024-bit (K = 19) and 3072-bit (K = 56) keys, and two keys made here from seeded
generators: one whose p - 1 spells the digits 32, 0, 0, 1, 63, 63, 63, ... and one whose top digits are even (8 of a 4-bit top
window; 4 under a shorter q).  Ciphertexts: uploaded word rows, pair rows written by the ciphertext product and by the DJN
encrypt; among them non-encryptions, 1, n + 1 and n^2 - 1.  The arithmetic is modelled in tests/test_ps_odd_table_model.py."""
import functools
import random

import pytest

from test_gpu_key_widths import _q3
from test_gpu_round4 import Res, key_case
from test_ps_odd_table_model import LOW_DIGITS, W, crafted_prime, digits_of

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 65, 130)
PS_LIMBS = {"iso": (36, 38), 1024: (19,), 3072: (56,), "zero-digit": (36, 38), "even-top": (36, 38)}
CASES = [(name, count) for name in ("iso", 1024, 3072) for count in COUNTS] + [("zero-digit", 65), ("even-top", 65)]


@functools.lru_cache(maxsize=None)
def _key(name):
    """(p, q, hs or None)"""
    if name == "iso":
        return key_case(2048)
    if name == "zero-digit":
        return crafted_prime(1024, "zero-digits"), crafted_prime(1024, "zero-digits-q"), None
    if name == "even-top":
        return crafted_prime(1024, "even-top", low=(2,), top=8), crafted_prime(1023, "even-top-q", low=(62, 62), top=0b100), None
    return key_case(name)


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """(ciphertexts, the oracle's plaintexts) for the largest count, computed once per key: every count takes a prefix"""
    from oracle import paillier_oracle as orc
    p, q, _ = _key(name)
    n = p * q
    rng = random.Random(str(name))
    enc = [(1 + n * rng.randrange(n)) * pow(rng.randrange(2, n), n, n * n) % (n * n) for _ in range(2)]
    raw = [n * n - 1, 1, n + 1] + enc + [rng.randrange(1, n * n) for _ in range(max(COUNTS) - 5)]
    return raw, orc.PrivateKey(n, p, q).decrypt(raw)


def test_the_made_keys_have_the_digits():
    p, q, _ = _key("zero-digit")
    ds = digits_of(p - 1, 1024, W)
    assert tuple(ds[:len(LOW_DIGITS)]) == LOW_DIGITS and ds.count(0) >= 3
    p, q, _ = _key("even-top")
    assert digits_of(p - 1, 1024, W)[-1] == 8 and digits_of(q - 1, 1024, W)[-1] == 4       # (the launch's length: 1024 bits)


def _restore(L, odd):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_ps_odd_table(odd)
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_ps_balanced(1)
    _capi.check(L.pgpu_set_table_gather_policy(0))


@pytest.mark.parametrize("name,count", CASES)
def test_odd_table_against_oracle_half_squared_form_and_masked_policy(engine, name, count):
    from pailliercryptolib_amd import _capi
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
        sources = {"words": (R.up(raw, 2 * nw), want),
                   "product": (R.op(L.pgpu_batch_ct_add, pk._h, R.up(raw, 2 * nw), R.up([1], 2 * nw)), want)}
        if hs is not None:
            m = [0, n - 1] + [rng.randrange(n) for _ in range(count)]
            m = m[:count]
            r = [rng.getrandbits(64) for _ in range(count)]
            rw = ((bits + 1) // 2 + 63) // 64
            sources["encrypt"] = (R.op(L.pgpu_batch_encrypt, pk._h, R.up(m, nw), R.up(r, rw), 64 * rw), m)
        L.pgpu_debug_set_ps_decrypt(2)
        for src, (h, expect) in sources.items():
            got = {}
            for bal in (1, 0) if len(PS_LIMBS[name]) == 2 else (1,):
                L.pgpu_debug_set_ps_balanced(bal)
                limbs = PS_LIMBS[name][0 if bal else 1]
                for form in ("odd", "half-squared", "masked"):
                    _capi.check(L.pgpu_set_table_gather_policy(1 if form == "masked" else 0))
                    L.pgpu_debug_set_ps_odd_table(0 if form == "half-squared" else 1)
                    assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0) == (4, 1, limbs)
                    got[bal, form] = R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, h))
                    # which table the launch built: `one` and the 2^(w-1) odd powers, the full table of the half-squared form,
                    # the 3-bit table of the masked policy (csrc/policy.cpp: 6-bit windows from 1005-bit exponents, 5 below)
                    w = 6 if max(p.bit_length(), q.bit_length()) > 1000 else 5
                    assert L.pgpu_debug_last_ps_table_entries() == {"odd": (1 << (w - 1)) + 1, "half-squared": 1 << w, "masked": 8}[form]
            for key, g in got.items():
                assert g == expect, (src, key)                               # every result against the oracle / the plaintexts
            first = next(iter(got.values()))
            assert all(g == first for g in got.values()), src                # ... and bit-equal among the forms
    finally:
        _restore(L, was)
        R.close()
