"""The one-lane CRT decrypt on balanced limbs with the folded reductions (csrc/hensel_ps_bal.hpp, PGPU_PSB_KARA_RED: the q * n
terms of columns K .. 2K-2 of the reductions of a2*b and of a*c in 1143 products instead of 1296, on the chains of the split
products, hensel_decrypt_psb_kernel<36,29>) against pow on the oracle, every plaintext, and bit for bit against the unsigned <38,28>
kernel (pgpu_debug_set_ps_balanced(0): code the fold does not touch), in the odd, the half-squared and the masked table forms.
The one-lane form is forced (pgpu_debug_set_ps_decrypt(2)).  Counts 1, 63, 65 and 130: a lone element, a wavefront short of one
lane, the clamped tail lanes of a second wavefront pair, and a third pair on the other side.  Keys: ISO 2048 bits, the two made
keys of tests/test_gpu_ps_odd_table.py and the 2051-bit key (primes of unequal top limbs: dn differs between the sides).
Ciphertexts: uploaded word rows and the rows written by the producers of resident rows of tests/test_gpu_ps_karatsuba.py, among
them the non-encryptions 1, n + 1 and n^2 - 1.  The arithmetic is modelled in tests/test_ps_kara_reduction_model.py."""
import random

import pytest

from test_gpu_key_widths import _q3
from test_gpu_ps_karatsuba import COUNTS, FORMS, NAMES, _key, _restore, _set_form, _vectors
from test_gpu_round4 import Res

pytestmark = pytest.mark.gpu
assert COUNTS == (1, 63, 65, 130) and NAMES == ("iso", "zero-digit", "even-top", 2051)
assert FORMS == ("odd", "half-squared", "masked")


@pytest.mark.parametrize("name,count", [(name, count) for name in NAMES for count in COUNTS])
def test_against_oracle_and_unsigned_kernel_in_every_table_form(engine, name, count):
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
        rng = random.Random(1000 + count)
        up = R.up(raw, 2 * nw)
        pm = ([0, n - 1, n // 2] + [rng.randrange(n) for _ in range(count)])[:count]
        e = rng.getrandbits(48) | 1
        # D is a homomorphism of the units modulo n^2 into the integers modulo n: every row below is a unit
        sources = {"words": (up, want),
                   "product": (R.op(L.pgpu_batch_ct_add, pk._h, up, R.up([n + 1], 2 * nw)), [(a + 1) % n for a in want]),
                   "plus plain": (R.op(L.pgpu_batch_ct_add_plain, pk._h, up, R.up(pm, nw)), [(a + b) % n for a, b in zip(want, pm)]),
                   "times plain": (R.op(L.pgpu_batch_ct_mul, pk._h, up, R.up([e], 1), 48), [a * e % n for a in want]),
                   "negation": (R.op(L.pgpu_batch_ct_negate, pk._h, up), [-a % n for a in want])}
        if hs is not None:
            m = ([n - 1, 0, 1] + [rng.randrange(n) for _ in range(count)])[:count]
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
    """two resident batches of 130 in flight on two batch lanes, three rounds: beside a busy lane a launch claims whole CUs and
    runs the build that owns the register file (<36,29,1>), the one the headline runs"""
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
            rng = random.Random(170 + ln)
            m = ([n - 1, 1, 0] + [rng.randrange(n) for _ in range(count)])[:count]
            _capi.check(L.pgpu_set_batch_lane(ln))
            rows = raw[::-1] if ln == 0 else raw
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
            assert R.down(raw_outs[ln]) == (want[::-1] if ln == 0 else want), ln
    finally:
        _restore(L, was)
        R.close()
