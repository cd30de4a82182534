"""The one-lane CRT decrypt on balanced limbs (csrc/hensel_ps_bal.hpp: hensel_decrypt_psb_kernel<36,29>, the 2048-bit class in 36
signed limbs of 29 bits instead of 38 unsigned ones of 28) against the oracle and against the unsigned kernel it replaces
(PGPU_PS_BALANCED=0 / pgpu_debug_set_ps_balanced(0)), bit for bit: the two half-width exponentiations of
PrivateKey::decryptCRT, ipcl/pri_key.cpp:114-157.  The one-lane form is forced (pgpu_debug_set_ps_decrypt(2)); counts 1, 63,
64, 65 and 130 are a lone element, a wavefront short of one lane, a full one, the clamped tail lanes of a second wavefront
pair and a third pair.  The arithmetic itself is modelled in tests/test_ps_balanced_model.py."""
import ctypes
import functools
import random

import numpy as np
import pytest

from test_gpu_key_widths import KEYS, Key, _q3
from test_gpu_round4 import Res, key_case

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65, 130)


def _restore(L):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_ps_balanced(1)
    _capi.check(L.pgpu_set_table_gather_policy(0))
    _capi.check(L.pgpu_set_batch_lane(0))


@functools.lru_cache(maxsize=None)
def _oracle(bits):
    from oracle import paillier_oracle as orc
    p, q = (key_case(2048)[:2] if bits == "iso" else KEYS[bits])
    return orc.PrivateKey(p * q, p, q)


def _ran_form(L, sk, count):
    """(split, lanes, limbs) of the kernel a lone decrypt of `count` runs"""
    return _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0)


@pytest.mark.parametrize("count", COUNTS)
def test_iso_key_every_producer_both_forms(engine, count):
    """DJN encrypt (pair rows), CT + CT, uploaded words (converted on entry) and the same values as pair rows, with the
    non-encryptions 1, n + 1 and n^2 - 1 and the plaintext edges 0, 1 and n - 1; indexed and masked table access"""
    from pailliercryptolib_amd import _capi
    p, q, hs = key_case(2048)
    n, nw = p * q, 32
    rng = random.Random(count)
    m = ([n - 1, 0, 1] + [rng.randrange(n) for _ in range(count)])[:count]
    m2 = ([1, n - 1, n - 1] + [rng.randrange(n) for _ in range(count)])[:count]
    r = [rng.getrandbits(1024) for _ in range(count)]
    raw = ([n * n - 1, 1, n + 1] + [rng.randrange(1, n * n) for _ in range(count)])[:count]
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    idx = sorted({0, 1, 2, count // 2, count - 1} & set(range(count)))
    oraw = _oracle("iso").decrypt([raw[i] for i in idx])
    R = Res()
    L = R.L
    try:
        c1 = R.op(L.pgpu_batch_encrypt, pk._h, R.up(m, nw), R.up(r, nw // 2), 1024)
        c2 = R.op(L.pgpu_batch_encrypt, pk._h, R.up(m2, nw), R.up(r[::-1], nw // 2), 1024)
        s = R.op(L.pgpu_batch_ct_add, pk._h, c1, c2)
        up = R.up(raw, 2 * nw)
        up_pair = R.op(L.pgpu_batch_ct_add, pk._h, up, R.up([1], 2 * nw))
        assert L.pgpu_batch_row_limbs(c1) == 144 and L.pgpu_batch_row_limbs(up_pair) == 144 and L.pgpu_batch_row_limbs(up) == 0
        srcs = (c1, s, up_pair, up)
        L.pgpu_debug_set_ps_decrypt(2)
        got = {}
        for gather in (0, 1):
            _capi.check(L.pgpu_set_table_gather_policy(gather))
            for bal in (1, 0):
                L.pgpu_debug_set_ps_balanced(bal)
                assert _ran_form(L, sk, count) == (4, 1, 36 if bal else 38)
                assert _q3(L.pgpu_decrypt_kernel_form, sk._h, count) == (4, 1, 38)          # the key's class, either way
                got[gather, bal] = [R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, x)) for x in srcs]
        for key, g in got.items():
            assert g[0] == m, key
            assert g[1] == [(a + b) % n for a, b in zip(m, m2)], key
            assert [g[2][i] for i in idx] == oraw and g[3] == g[2], key
        assert got[0, 1] == got[0, 0] == got[1, 1] == got[1, 0]                           # the two forms, bit for bit
    finally:
        _restore(L)
        R.close()


def test_iso_key_on_all_four_batch_lanes(engine):
    """four resident batches of 130 in flight, one per batch lane: beside busy neighbours a launch claims whole CUs and runs
    the build that owns the register file (<36,29,1>).  Every lane's round trip and its non-encryptions, several rounds"""
    from pailliercryptolib_amd import _capi
    p, q, hs = key_case(2048)
    n, nw, count = p * q, 32, 130
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    R = Res()
    L = R.L
    try:
        L.pgpu_debug_set_ps_decrypt(2)
        sets = []
        for ln in range(4):
            rng = random.Random(40 + ln)
            m = ([0, 1, n - 1] + [rng.randrange(n) for _ in range(count)])[:count]
            raw = ([1, n + 1, n * n - 1] + [rng.randrange(1, n * n) for _ in range(count)])[:count]
            _capi.check(L.pgpu_set_batch_lane(ln))
            sets.append((m, R.up(m, nw), R.up([rng.getrandbits(1024) for _ in range(count)], nw // 2), raw, R.up(raw, 2 * nw)))
        want_raw = []
        L.pgpu_debug_set_ps_balanced(0)
        for ln in range(4):                                # the unsigned kernel's answers first, lane by lane
            _capi.check(L.pgpu_set_batch_lane(ln))
            want_raw.append(R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, sets[ln][4])))
        assert want_raw[0][:3] == _oracle("iso").decrypt(sets[0][3][:3])
        L.pgpu_debug_set_ps_balanced(1)
        outs, raw_outs = [None] * 4, [None] * 4
        for _ in range(3):                                 # (the first round starts beside idle lanes)
            for ln in range(4):
                _capi.check(L.pgpu_set_batch_lane(ln))
                ct = R.op(L.pgpu_batch_encrypt, pk._h, sets[ln][1], sets[ln][2], 1024)
                outs[ln] = R.op(L.pgpu_batch_decrypt_crt, sk._h, ct)
                raw_outs[ln] = R.op(L.pgpu_batch_decrypt_crt, sk._h, sets[ln][4])
        _capi.check(L.pgpu_set_batch_lane(0))
        _capi.check(L.pgpu_synchronize())
        for ln in range(4):
            assert R.down(outs[ln]) == sets[ln][0], ln
            assert R.down(raw_outs[ln]) == want_raw[ln], ln
        # what the policy reports for the headline's launch: 8192 ciphertexts beside three busy lanes
        L.pgpu_debug_set_ps_decrypt(1)
        assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, 8192, 3) == (4, 1, 36)
        L.pgpu_debug_set_ps_balanced(0)
        assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, 8192, 3) == (4, 1, 38)
    finally:
        _restore(L)
        R.close()


@pytest.mark.parametrize("bits", [2037, 2051, 2052])
def test_keys_off_the_standard_width(engine, bits):
    """primes of unequal width (2037), the last width of the (4,18) pair rows (2051) and the first of the (8,14) rows (2052):
    other chunkings of the entry (3 x 24 and 4 x 28 row limbs) and other top limbs of the prime"""
    K = Key(engine, bits)
    L, R, n, nsq = K.L, K.R, K.n, K.nsq
    count = 65
    rng = random.Random(bits)
    try:
        c1, m = K.fresh(rng, count)
        raw = ([nsq - 1, 1, n + 1] + [rng.randrange(1, nsq) for _ in range(count)])[:count]
        up = R.up(raw, 2 * K.nw)
        idx = [0, 1, 2, count - 1]
        oraw = _oracle(bits).decrypt([raw[i] for i in idx])
        L.pgpu_debug_set_ps_decrypt(2)
        got = {}
        for bal in (1, 0):
            L.pgpu_debug_set_ps_balanced(bal)
            assert _ran_form(L, K.sk, count) == (4, 1, 36 if bal else 38)
            got[bal] = [K.decrypt(c1), K.decrypt(up)]
            assert got[bal][0] == m and [got[bal][1][i] for i in idx] == oraw, bal
        assert got[1] == got[0]
    finally:
        _restore(L)
        K.close()


def test_keys_that_do_not_fit_keep_their_path(engine):
    """2560 bits (primes of 1280 bits: beyond 29 * 36 - 4) has no one-lane form at all, 1024- and 3072-bit keys keep the
    unsigned kernels of 19 and 56 limbs: the switch changes neither the form nor the plaintexts"""
    count = 65
    K = Key(engine, 2560)
    L, R = K.L, K.R
    try:
        rng = random.Random(2560)
        c1, m = K.fresh(rng, count)
        L.pgpu_debug_set_ps_decrypt(2)
        forms = []
        for bal in (1, 0):
            L.pgpu_debug_set_ps_balanced(bal)
            forms.append(_ran_form(L, K.sk, count))
            assert K.decrypt(c1) == m
        assert forms[0] == forms[1] and forms[0][2] != 36
        for kbits, limbs in ((1024, 19), (3072, 56)):
            p, q, hs = key_case(kbits)
            n, nw = p * q, kbits // 64
            pk, sk = engine.PublicKey(n, kbits, hs=hs), engine.PrivateKey(p, q)
            mm = [0, 1, n - 1] + [rng.randrange(n) for _ in range(count - 3)]
            c = R.op(L.pgpu_batch_encrypt, pk._h, R.up(mm, nw), R.up([rng.getrandbits(kbits // 2) for _ in mm], nw // 2), kbits // 2)
            for bal in (1, 0):
                L.pgpu_debug_set_ps_balanced(bal)
                assert _ran_form(L, sk, count) == (4, 1, limbs)
                assert R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, c)) == mm
    finally:
        _restore(L)
        K.close()
