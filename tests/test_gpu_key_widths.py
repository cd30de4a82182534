"""Resident ciphertext operations at key widths OFF the standard classes (tests/golden/key_widths.json, and the uneven
2037-bit key of primes_uneven.json): the smallest user of a pair-row class, its first width, a width in its middle, and its
last -- where R = 2^(29 L2) is 2^8 P for the loop modulus P = n k and no more.  Every operation on resident ciphertexts
picks its kernel form and its host-side constants (the chunking of word rows cw / nchunks, the pair-row entry of CRT
decrypt pchunks / pchunk_limbs / kappa, the R^2 2^(64 cw i) ladders of capi_keys.inc) from the bit length of n; at 1024,
2048 and 3072 bits n fills its words, the primes are of one width and the limbs of the class match the key, so none of
that is exercised by the tests of the standard sizes.

Everything is compared bit for bit with Python integers (pow, %) and the Python oracle: encrypt (DJN and r^n), CT+CT,
CT x PT, CT+PT, CRT decrypt in every form a key has, matvec, segment_sum, segment_scan, pack, spmv, matmul (both layouts)
and the bucket matvec, with edge plaintexts, randomness, exponents, weights and ciphertext values, at batch sizes 1 and 37
(ragged for 16, 8 and 4 elements per wavefront).  Keys of the (4,18) class run their aggregation kernels in two forms,
(4,18) and (8,9) by the size of the launch: pack and segment_sum are run in both at four widths of that class, the bucket
reduction at its first and its last (the weighted sum has its own widths test in test_gpu_wsum.py).  One bit beyond the last class every
aggregation call and its plan query refuses.  The reference takes any key length that is a multiple of 4 (ipcl/keygen.cpp:101) and composes all of these from
PublicKey::encrypt (pub_key.cpp:82-129), CipherText::operator+ / operator* (ciphertext.cpp:35-106) and
PrivateKey::decrypt (pri_key.cpp:65-157)."""
import ctypes
import functools
import json
import os
import random

import numpy as np
import pytest

from test_gpu_pair_rows import Res

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NONE = 0xFFFFFFFF                                    # kSegsumNone
UNSUPPORTED = -3                                     # PGPU_ERR_UNSUPPORTED
REVERSE = 1                                          # PGPU_SCAN_REVERSE
MATMUL_TRANSPOSED = 1                                # PGPU_MATMUL_TRANSPOSED
COUNTS = (1, 37)


def _load():
    keys = {c["bits"]: (int(c["p"], 16), int(c["q"], 16)) for c in json.load(open(os.path.join(GOLD, "key_widths.json")))["cases"]}
    k = json.load(open(os.path.join(GOLD, "primes_uneven.json")))
    keys[k["bits"]] = (int(k["p"], 16), int(k["q"], 16))
    return keys


KEYS = _load()
WIDTHS = sorted(KEYS)
assert WIDTHS == [512, 1065, 1088, 1124, 1536, 2037, 2051, 2052, 2560, 3211, 3212]


# ---- the class table, written out (csrc/policy.hpp: pair_form_for_bits; csrc/launch.hpp) ----
def pair_form(bits, features=0):
    """(G, K) of the key's pair rows, or None: word rows"""
    if bits <= 1065:
        return (2, 19)                               # 38 limbs per half
    if bits <= 2051:
        return (4, 18)                               # 72 -- 1066 .. 1123 included
    if bits <= 3211:
        return (8, 14)                               # 112
    if bits <= 4139 and features & 1:
        return (8, 18)                               # 144, builds with the 4096-bit forms only
    return None


PAIR_WIDTHS = [b for b in WIDTHS if b <= 3211]       # ... with the aggregation kernels (launch.hpp: matvec_has)
WIDE_WIDTHS = [1124, 1536, 2037, 2051]               # (8,9) beside (4,18)
# the widest prime a private split form holds: (4,14) / (8,7), 29 * 56 = 1624 >= bits + 37 (launch.hpp: hensel_has)
PRIVATE_SPLIT_MAX_PRIME = 1587
# limbs of the one-lane / one-wavefront decrypt forms per width (launch.hpp: hensel_ps_has; capi_keys.inc: build_hensel --
# 28 K >= prime bits + 32 > 28 (K - 1)): primes of 1005 .. 1032 bits take K = 38; no other key here has such primes
PS_LIMBS = {2037: 38, 2051: 38, 2052: 38}
# (lanes, limbs) of the sequential-halves decrypt form, the key's private form of fewest lanes (launch.hpp: hensel_seq_has):
# primes up to 543 bits (2,10), up to 1065 (2,19), up to 1587 (4,14)
SEQ_FORM = {512: (2, 10), 1065: (2, 10), 1088: (2, 19), 1124: (2, 19), 1536: (2, 19), 2037: (2, 19), 2051: (2, 19), 2052: (2, 19),
            2560: (4, 14)}


@functools.lru_cache(maxsize=None)
def djn_hs(bits):
    """hs = (-x^2)^n mod n^2 as pub_key.cpp:40-49 forms it, x seeded (the one pow per DJN case)"""
    p, q = KEYS[bits]
    n = p * q
    x = random.Random(bits).randrange(2, n)
    return pow(n * n - x * x % (n * n), n, n * n)


class Key:
    def __init__(self, engine, bits, djn=True):
        self.bits, self.djn = bits, djn
        self.p, self.q = KEYS[bits]
        self.n = self.p * self.q
        assert self.n.bit_length() == bits
        self.nsq = self.n * self.n
        self.nw = (bits + 63) // 64                  # words of n
        self.mw = bits // 64                         # the widest plaintext rows that are no wider than n
        self.rw = ((bits + 1) // 2 + 63) // 64       # words of DJN randomness (bits / 2 random bits)
        self.hs = djn_hs(bits) if djn else None
        self.pk, self.sk = engine.PublicKey(self.n, bits, hs=self.hs), engine.PrivateKey(self.p, self.q)
        self.R = Res()
        self.L = self.R.L
        self.form = pair_form(bits, self.L.pgpu_build_features())
        self.l2 = self.form[0] * self.form[1] if self.form else 0
        self.split_private = max(self.p.bit_length(), self.q.bit_length()) <= PRIVATE_SPLIT_MAX_PRIME
        self._obf = {}
        self.pool = [random.Random(bits + 1).randrange(2, self.n) for _ in range(2)]     # r^n randomness: few values, one pow each

    def obf(self, r):
        if r not in self._obf:
            self._obf[r] = pow(self.hs, r, self.nsq) if self.djn else pow(r, self.n, self.nsq)
        return self._obf[r]

    def enc_expect(self, m, r):
        return [(1 + self.n * a) % self.nsq * self.obf(b) % self.nsq for a, b in zip(m, r)]

    def rand_r(self, rng, count, edges=True):
        """randomness rows: DJN of rw words, r^n of nw words; few distinct values (one Python pow each)"""
        if self.djn:
            head = [0, 1, (1 << (64 * self.rw)) - 1] if edges else []
            return (head + [rng.getrandbits(64) for _ in range(count)])[:count] if count > 1 else [(1 << (64 * self.rw)) - 1 if edges else rng.getrandbits(64)]
        pool = self.pool
        head = [1, (1 << (64 * self.nw)) - 1, 0, self.n - 1] if edges else []
        return (head + [pool[i % 2] for i in range(count)])[:count] if count > 1 else [(1 << (64 * self.nw)) - 1 if edges else pool[0]]

    def encrypt(self, m, r, m_words):
        rw = self.rw if self.djn else self.nw
        return self.R.op(self.L.pgpu_batch_encrypt, self.pk._h, self.R.up(m, m_words), self.R.up(r, rw), 64 * rw)

    def fresh(self, rng, count):
        """resident DJN ciphertexts of random plaintexts below 2^(64 mw): pair rows where the key has them"""
        m = [rng.getrandbits(64 * self.mw) % self.n for _ in range(count)]
        r = [rng.getrandbits(64) for _ in range(count)]
        x = self.encrypt(m, r, self.mw)
        assert self.L.pgpu_batch_row_limbs(x) == 2 * self.l2
        return x, m

    def decrypt(self, h):
        return self.R.down(self.R.op(self.L.pgpu_batch_decrypt_crt, self.sk._h, h))

    def close(self):
        self.R.close()


def _q3(fn, *args):
    from pailliercryptolib_amd import _capi
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _capi.check(fn(*args, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def _half_limbs(form):
    """limbs per half of a (split, lanes, limbs) answer: the paired forms put a half on lanes / 2 lanes"""
    split, lanes, limbs = form
    return {0: 0, 1: lanes // 2 * limbs, 2: lanes * limbs, 5: limbs}[split]


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    names = ("PGPU_MATVEC_SLICES", "PGPU_MATVEC_WINDOW", "PGPU_SEGSUM_CHUNK", "PGPU_SEGSCAN_CHUNK", "PGPU_PACK_WIDE",
             "PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK", "PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES",
             "PGPU_BUCKET_WINDOW", "PGPU_BUCKET_BLOCK")
    for name in names:
        monkeypatch.delenv(name, raising=False)

    def force(**kw):
        for name in names:
            v = kw.get(name[5:].lower())
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


def _restore(L):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_seq_decrypt(4)
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_wave_decrypt(1)
    L.pgpu_debug_set_hensel(1)
    _capi.check(L.pgpu_set_table_gather_policy(0))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", WIDTHS)
def test_forms_follow_the_class_table(engine, bits):
    """what the queries and the plan calls report, against the table above: 38, 72 or 112 limbs per half, or word rows"""
    K = Key(engine, bits)
    L, l2 = K.L, K.l2
    big = 1 << 20
    try:
        # rows of every producer
        rng = random.Random(bits)
        x, _ = K.fresh(rng, 3)
        assert L.pgpu_batch_row_limbs(x) == 2 * l2
        s = K.R.op(L.pgpu_batch_ct_add, K.pk._h, x, x)
        t = K.R.op(L.pgpu_batch_ct_mul, K.pk._h, x, K.R.up([3], 1), 2)
        u = K.R.op(L.pgpu_batch_ct_add_plain, K.pk._h, x, K.R.up([5], K.mw))
        up = K.R.op(L.pgpu_batch_ct_add, K.pk._h, K.R.up([K.nsq - 1] * 3, 2 * K.nw), x)       # uploaded words join
        assert [L.pgpu_batch_row_limbs(h) for h in (s, t, u, up)] == [2 * l2] * 4
        # plaintext rows wider than floor(bits / 64) words leave Montgomery-form words (capi_batches.inc: pgpu_batch_encrypt)
        full = K.encrypt([1, 2, 3], [1, 2, 3], K.nw)
        assert L.pgpu_batch_row_limbs(full) == (2 * l2 if bits % 64 == 0 else 0) and L.pgpu_batch_is_montgomery(full) == 1
        # DJN encrypt
        assert _half_limbs(_q3(L.pgpu_encrypt_kernel_form, K.pk._h, K.mw, big)) == l2
        if bits % 64:
            assert _q3(L.pgpu_encrypt_kernel_form, K.pk._h, K.nw, big)[0] == 0
        assert _half_limbs(_q3(L.pgpu_encrypt_kernel_form_ex, K.pk._h, K.mw, big, 3)) == l2
        L.pgpu_debug_set_wave_decrypt(2)
        room = K.form is not None and 29 * l2 - (bits + 29) >= 10 and l2 in (38, 72, 112)      # (32-bit quotient digits: R >= 2^10 P)
        f = _q3(L.pgpu_encrypt_kernel_form_ex, K.pk._h, K.mw, 37, -1)
        assert (f == (5, 64, l2)) == room
        f = _q3(L.pgpu_modexp_n2_kernel_form, K.pk._h, 37)
        assert (f == (5, 64, l2)) == room
        # CT x PT and CT + CT, sequential halves forced: the pair form itself
        L.pgpu_debug_set_wave_decrypt(0)
        L.pgpu_debug_set_seq_decrypt(2)
        if K.form and K.form != (8, 18):
            assert _q3(L.pgpu_modexp_n2_kernel_form, K.pk._h, big) == (2,) + K.form
            assert _q3(L.pgpu_ct_add_kernel_form, K.pk._h, big) == (2,) + K.form
        L.pgpu_debug_set_seq_decrypt(0)
        assert _half_limbs(_q3(L.pgpu_ct_add_kernel_form, K.pk._h, big)) == l2
        assert _half_limbs(_q3(L.pgpu_ct_add_kernel_form, K.pk._h, 37)) == l2
        if K.form:
            assert _half_limbs(_q3(L.pgpu_modexp_n2_kernel_form, K.pk._h, big)) == l2
        else:
            assert _q3(L.pgpu_modexp_n2_kernel_form, K.pk._h, big)[0] == 0
        # CRT decrypt: a split form of the private key, or the full-width kernels
        for args in ((37,), (big,)):
            assert (_q3(L.pgpu_decrypt_kernel_form, K.sk._h, *args)[0] != 0) == K.split_private
        assert (_q3(L.pgpu_decrypt_kernel_form_ex, K.sk._h, 8192, 3)[0] != 0) == K.split_private
        # the four plan calls
        agg = bits in PAIR_WIDTHS
        w, sl, tb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        rc = L.pgpu_ct_matvec_plan(bits, 5, 7, 32, ctypes.byref(w), ctypes.byref(sl), ctypes.byref(tb))
        assert rc == (0 if agg else UNSUPPORTED)
        if agg:
            assert tb.value == 7 * (1 << w.value) * 2 * l2 * 4
        a, b, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert L.pgpu_ct_segment_sum_plan(bits, 37, 6, 20, ctypes.byref(a), ctypes.byref(b)) == (0 if agg else UNSUPPORTED)
        assert L.pgpu_ct_segment_scan_plan(bits, 3, 9, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr)) == (0 if agg else UNSUPPORTED)
        for rows in (1, big):
            rc = L.pgpu_ct_pack_plan(bits, rows, 2, 3, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr))
            assert rc == (0 if agg else UNSUPPORTED)
            if agg:
                wide = rows == 1 and K.form == (4, 18)
                assert (a.value, b.value) == ((8, 9) if wide else K.form) and a.value * b.value == l2
    finally:
        _restore(L)
        K.close()


# ---------------------------------------------------------------------------------------------------------------------
def _chain(K, count, m_words, seed):
    """encrypt -> CT+CT -> CT x PT -> CT+PT -> CRT decrypt, as test_gpu_pair_rows.test_resident_chain_in_pair_rows; word
    ciphertexts mixed in, one-element operands, plaintext rows wider than n"""
    from oracle import paillier_oracle as orc
    L, R, n, nsq, nw, bits = K.L, K.R, K.n, K.nsq, K.nw, K.bits
    rng = random.Random(seed)
    top = (1 << (64 * m_words)) - 1
    edge_m = [0, 1, top] + ([n - 1, n] if m_words == nw else [])           # (n - 1 and n need all the words of n)
    edge_e = [0, 1, 2, (1 << 40) - 1, rng.getrandbits(bits) | (1 << (bits - 1))]   # ... and one full-width exponent
    if count == 1:
        m1, e = [edge_m[-1] if m_words == nw else top], [edge_e[-1]]
    else:
        m1 = (edge_m + [rng.getrandbits(64 * m_words) % n for _ in range(count)])[:count]
        e = (edge_e + [rng.getrandbits(40) for _ in range(count)])[:count]
    m2 = [rng.getrandbits(64 * m_words) % n for _ in range(count)]
    r1, r2 = K.rand_r(rng, count), K.rand_r(rng, count, edges=False)
    ew = (bits + 63) // 64
    pair = 2 * K.l2 if 64 * m_words <= bits else 0                          # rows of the encrypt's result
    bm1, bm2, be = R.up(m1, m_words), R.up(m2, m_words), R.up(e, ew)
    c1, c2 = K.encrypt(m1, r1, m_words), K.encrypt(m2, r2, m_words)
    oc1, oc2 = K.enc_expect(m1, r1), K.enc_expect(m2, r2)
    assert L.pgpu_batch_row_limbs(c1) == pair and L.pgpu_batch_is_montgomery(c1) == 1
    assert R.down(c1) == oc1 and R.down(c2) == oc2
    s = R.op(L.pgpu_batch_ct_add, K.pk._h, c1, c2)
    osum = [a * b % nsq for a, b in zip(oc1, oc2)]
    assert R.down(s) == osum
    t = R.op(L.pgpu_batch_ct_mul, K.pk._h, s, be, bits)
    omul = [pow(a, b, nsq) for a, b in zip(osum, e)]
    assert R.down(t) == omul
    u = R.op(L.pgpu_batch_ct_add_plain, K.pk._h, t, bm1)
    oadd = [a * ((1 + n * b) % nsq) % nsq for a, b in zip(omul, m1)]
    assert R.down(u) == oadd
    # results are pair rows whatever came in -- but CT + PT with plaintext rows wider than n runs full width, on plain words
    assert [L.pgpu_batch_row_limbs(h) for h in (s, t, u)] == [2 * K.l2, 2 * K.l2, 2 * K.l2 if 64 * m_words <= bits else 0]
    ok = [i for i in range(count) if oc1[i] % K.p and oc1[i] % K.q]            # (r = 0 under r^n: c = 0 decrypts to nothing)
    got = K.decrypt(u)
    assert [got[i] for i in ok] == [((m1[i] + m2[i]) * e[i] + m1[i]) % n for i in ok]
    got = K.decrypt(c1)
    assert [got[i] for i in ok] == [m1[i] % n for i in ok]
    assert K.decrypt(c2) == m2
    # uploaded (plain) ciphertext words join; the ends of the value range among them
    raw = ([1, nsq - 1, n, n + 1, nsq - n] + [rng.randrange(1, nsq) for _ in range(count)])[:count] if count > 1 else [nsq - 1]
    pr = R.up(raw, 2 * nw)
    want = [a * b % nsq for a, b in zip(oc1, raw)]
    assert R.down(R.op(L.pgpu_batch_ct_add, K.pk._h, c1, pr)) == want
    assert R.down(R.op(L.pgpu_batch_ct_add, K.pk._h, pr, c1)) == want
    assert R.down(R.op(L.pgpu_batch_ct_add, K.pk._h, pr, pr)) == [a * a % nsq for a in raw]
    assert R.down(R.op(L.pgpu_batch_ct_mul, K.pk._h, pr, be, bits)) == [pow(a, b, nsq) for a, b in zip(raw, e)]
    assert R.down(R.op(L.pgpu_batch_ct_add_plain, K.pk._h, pr, bm2)) == [a * ((1 + n * b) % nsq) % nsq for a, b in zip(raw, m2)]
    pc2 = R.up(oc2, 2 * nw)
    assert K.decrypt(pc2) == m2
    units = [i for i in range(count) if raw[i] % K.p and raw[i] % K.q][:3]     # (n and n^2 - n are no units)
    got = K.decrypt(pr)
    assert [got[i] for i in units] == orc.PrivateKey(n, K.p, K.q).decrypt([raw[i] for i in units])
    if count > 1:                                                              # one-element operands broadcast
        one = R.up([raw[1]], 2 * nw)
        assert R.down(R.op(L.pgpu_batch_ct_add, K.pk._h, c1, one)) == [a * raw[1] % nsq for a in oc1]
        e1 = R.up([e[3]], ew)
        assert R.down(R.op(L.pgpu_batch_ct_mul, K.pk._h, c2, e1, bits)) == [pow(a, e[3], nsq) for a in oc2]
        m0 = R.up([m1[2]], m_words)
        assert R.down(R.op(L.pgpu_batch_ct_add_plain, K.pk._h, c1, m0)) == [a * ((1 + n * m1[2]) % nsq) % nsq for a in oc1]
    # plaintext rows WIDER than n: the full-width kernels, and their results still mix with pair rows
    wide = [v + n * (i % 3) for i, v in enumerate(m2)]
    bw = R.up(wide, 2 * nw)
    cw = K.encrypt(wide, r2, 2 * nw)
    assert L.pgpu_batch_row_limbs(cw) == 0 and R.down(cw) == oc2
    assert R.down(R.op(L.pgpu_batch_ct_add, K.pk._h, c1, cw)) == osum
    assert R.down(R.op(L.pgpu_batch_ct_add_plain, K.pk._h, c1, bw)) == [a * ((1 + n * b) % nsq) % nsq for a, b in zip(oc1, wide)]


@pytest.mark.parametrize("djn", [True, False], ids=["djn", "rn"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_resident_chain(engine, bits, djn):
    K = Key(engine, bits, djn)
    try:
        for count in COUNTS:
            for m_words in sorted({K.mw, K.nw}):        # rows no wider than n (pair rows out), and the words of n
                _chain(K, count, m_words, bits * 31 + count * 7 + m_words)
                K.close()
    finally:
        K.close()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", WIDTHS)
def test_every_decrypt_form_the_key_has(engine, bits):
    """paired, sequential-halves, one-lane and one-wavefront CRT decrypt of rows from every producer and of host words,
    with indexed and with masked table access; a form the key lacks is reported as lacking and the forced setting still
    returns the plaintexts"""
    from oracle import paillier_oracle as orc
    from pailliercryptolib_amd import _capi
    K = Key(engine, bits)
    L, R, n, nsq = K.L, K.R, K.n, K.nsq
    count = 37
    rng = random.Random(bits + 3)
    try:
        c1, m = K.fresh(rng, count)
        c2, m2 = K.fresh(rng, count)
        e = ([0, 1, (1 << 33) - 1] + [rng.getrandbits(33) for _ in range(count)])[:count]
        s = R.op(L.pgpu_batch_ct_add, K.pk._h, c1, c2)
        t = R.op(L.pgpu_batch_ct_mul, K.pk._h, s, R.up(e, 1), 33)
        raw = ([nsq - 1, 1, nsq - 2, n + 1] + [rng.randrange(1, nsq) for _ in range(count)])[:count]
        up = R.up(raw, 2 * K.nw)                                                  # word rows
        up_pair = R.op(L.pgpu_batch_ct_add, K.pk._h, up, R.up([1], 2 * K.nw))     # the same values as pair rows
        assert L.pgpu_batch_row_limbs(up_pair) == 2 * K.l2 and L.pgpu_batch_row_limbs(up) == 0
        idx = [0, 1, 2, 3, count - 1]
        oraw = orc.PrivateKey(n, K.p, K.q).decrypt([raw[i] for i in idx])
        want = [m, [(a + b) % n for a, b in zip(m, m2)], [(a + b) * x % n for a, b, x in zip(m, m2, e)]]
        srcs = (c1, s, t, up_pair, up)
        host = np.ascontiguousarray(R.i2l(raw, 2 * K.nw))
        ps = PS_LIMBS.get(bits)
        # (name, PGPU_SEQ_DECRYPT, PGPU_PS_DECRYPT, PGPU_WAVE_FORMS, pgpu_debug_set_hensel: 2 = the private form of fewest
        # lanes whatever the batch size -- the only one with a sequential-halves kernel)
        settings = [("paired", 0, 1, 0, 1), ("sequential", 2, 1, 0, 2), ("one-lane", 4, 2, 0, 1), ("one-wavefront", 4, 1, 2, 1)]
        first = None
        for gather in (0, 1):
            _capi.check(L.pgpu_set_table_gather_policy(gather))
            for name, seq, pspol, wave, hmode in settings:
                L.pgpu_debug_set_hensel(hmode)
                L.pgpu_debug_set_seq_decrypt(seq)
                L.pgpu_debug_set_ps_decrypt(pspol)
                L.pgpu_debug_set_wave_decrypt(wave)
                f = _q3(L.pgpu_decrypt_kernel_form, K.sk._h, count)
                if not K.split_private:
                    assert f[0] == 0, (name, f)
                elif name == "paired":
                    assert f[0] == 1, f
                elif name == "sequential":
                    assert f == (2,) + SEQ_FORM[bits], f
                elif name == "one-lane":
                    assert f == ((4, 1, ps) if ps else f) and (f[0] == 4) == (ps is not None), f
                else:
                    assert f == ((5, 64, ps) if ps else f) and (f[0] == 5) == (ps is not None), f
                got = [K.decrypt(x) for x in srcs]
                assert got[:3] == want, (name, gather)
                assert got[3] == got[4] and [got[3][i] for i in idx] == oraw, (name, gather)
                out = np.zeros((count, K.nw), dtype=np.uint64)
                _capi.check(L.pgpu_paillier_decrypt_crt(K.sk._h, host.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), count))
                assert R.l2i(out) == got[3], (name, gather)
                if first is None:
                    first = got
                assert got == first, (name, gather)                            # every form, bit for bit
    finally:
        _restore(L)
        K.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_forced_forms_of_the_elementwise_kernels(engine, bits):
    """CT x PT, CT + CT and DJN encrypt in the paired, the sequential-halves and the one-wavefront forms (the forms of
    large and of small launches, forced at test size): the same ciphertexts as pow() in each"""
    K = Key(engine, bits)
    L, R, n, nsq = K.L, K.R, K.n, K.nsq
    count = 37
    rng = random.Random(bits + 4)
    top = (1 << (64 * K.mw)) - 1
    m = ([0, 1, top] + [rng.getrandbits(64 * K.mw) % n for _ in range(count)])[:count]
    m2 = [rng.getrandbits(64 * K.mw) % n for _ in range(count)]
    r, r2 = K.rand_r(rng, count), K.rand_r(rng, count, edges=False)
    e = ([0, 1, 2, (1 << 40) - 1] + [rng.getrandbits(40) for _ in range(count)])[:count]
    oc, oc2 = K.enc_expect(m, r), K.enc_expect(m2, r2)
    osum = [a * b % nsq for a, b in zip(oc, oc2)]
    omul = [pow(a, b, nsq) for a, b in zip(osum, e)]
    try:
        for seq, wave in ((0, 0), (2, 0), (0, 2), (2, 2)):
            L.pgpu_debug_set_seq_decrypt(seq)
            L.pgpu_debug_set_wave_decrypt(wave)
            be = R.up(e, 1)
            c, c2 = K.encrypt(m, r, K.mw), K.encrypt(m2, r2, K.mw)
            assert L.pgpu_batch_row_limbs(c) == 2 * K.l2
            assert R.down(c) == oc and R.down(c2) == oc2, (seq, wave)
            s = R.op(L.pgpu_batch_ct_add, K.pk._h, c, c2)
            assert R.down(s) == osum, (seq, wave)
            t = R.op(L.pgpu_batch_ct_mul, K.pk._h, s, be, 40)
            assert R.down(t) == omul, (seq, wave)
            t2 = R.op(L.pgpu_batch_ct_mul, K.pk._h, t, R.up([e[3]], 1), 40)      # its own rows, one exponent for the batch
            assert R.down(t2) == [pow(a, e[3], nsq) for a in omul], (seq, wave)
            assert K.decrypt(t) == [(a + b) * x % n for a, b, x in zip(m, m2, e)], (seq, wave)
            K.close()
    finally:
        _restore(L)
        K.close()


# ---------------------------------------------------------------------------------------------------------------------
def _matvec_expect(K, xs, wm):
    out = []
    for row in wm:
        acc = 1
        for x, w in zip(xs, row):
            acc = acc * pow(x, w, K.nsq) % K.nsq
        out.append(acc)
    return out


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_matvec(engine, knobs, bits):
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 5)
    rows, cols = 5, 7
    try:
        x, m = K.fresh(rng, cols)
        xs = R.down(x)
        wm = [[rng.getrandbits(32) for _ in range(cols)] for _ in range(rows)]
        wm[0][:3] = [0, 1, (1 << 32) - 1]
        wm[1] = [0] * cols
        wm[2] = [(1 << 32) - 1] * cols
        want = _matvec_expect(K, xs, wm)
        wb = R.up([v for row in wm for v in row], 1)
        for slices in (None, 3):
            knobs(matvec_slices=slices)
            y = R.op(L.pgpu_batch_ct_matvec, K.pk._h, x, wb, rows, 32)
            assert L.pgpu_batch_count(y) == rows and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, slices
            assert K.decrypt(y) == [sum(a * w for a, w in zip(m, row)) % K.n for row in wm], slices
        knobs()
        up = R.up(xs, 2 * K.nw)                                                   # word rows: converted on the way in
        assert R.down(R.op(L.pgpu_batch_ct_matvec, K.pk._h, up, wb, rows, 32)) == want
    finally:
        K.close()


def _segsum_expect(K, xs, ids, groups, n_segments):
    cols = len(xs)
    out = [1] * (groups * n_segments)
    for g in range(groups):
        for j in range(cols):
            s = ids[g * cols + j]
            if s != NONE:
                out[g * n_segments + s] = out[g * n_segments + s] * xs[j] % K.nsq
    return out


def _segsum(K, x, ids, groups, n_segments):
    a = np.array(ids, dtype=np.uint32)
    return K.R.op(K.L.pgpu_batch_ct_segment_sum, K.pk._h, x, a.ctypes.data_as(ctypes.c_void_p), groups, n_segments)


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_segment_sum(engine, knobs, bits):
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 6)
    cols, groups, bins = 37, 2, 3
    try:
        x, m = K.fresh(rng, cols)
        xs = R.down(x)
        ids = [rng.choice((0, 2)) for _ in range(cols)] + [rng.randrange(3) for _ in range(cols)]    # group 0: bin 1 stays empty
        ids[5] = NONE
        ids[cols + 11] = NONE
        want = _segsum_expect(K, xs, ids, groups, bins)
        assert want[1] == 1
        for chunk in (None, 2):
            knobs(segsum_chunk=chunk)
            y = _segsum(K, x, ids, groups, bins)
            assert L.pgpu_batch_count(y) == groups * bins and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, chunk
            dec = K.decrypt(y)
            assert dec == [sum(m[j] for j in range(cols) if ids[g * cols + j] == s) % K.n for g in range(groups) for s in range(bins)]
        knobs()
        edge = [1, K.nsq - 1, K.n + 1, K.nsq - K.n + 1] + xs[4:]                   # word rows with the ends of the range
        assert R.down(_segsum(K, R.up(edge, 2 * K.nw), ids, groups, bins)) == _segsum_expect(K, edge, ids, groups, bins)
    finally:
        K.close()


def _scan_expect(K, xs, seg_len, reverse):
    out = [None] * len(xs)
    for r in range(len(xs) // seg_len):
        acc = 1
        for t in (range(seg_len - 1, -1, -1) if reverse else range(seg_len)):
            acc = acc * xs[r * seg_len + t] % K.nsq
            out[r * seg_len + t] = acc
    return out


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_segment_scan(engine, knobs, bits):
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 7)
    rows, seg_len = 3, 9
    try:
        x, m = K.fresh(rng, rows * seg_len)
        xs = R.down(x)
        for chunk in (None, 2):
            knobs(segscan_chunk=chunk)
            for reverse in (False, True):
                y = R.op(L.pgpu_batch_ct_segment_scan, K.pk._h, x, seg_len, REVERSE if reverse else 0)
                assert L.pgpu_batch_count(y) == rows * seg_len and L.pgpu_batch_row_limbs(y) == 2 * K.l2
                assert R.down(y) == _scan_expect(K, xs, seg_len, reverse), (chunk, reverse)
        knobs()
        y = R.op(L.pgpu_batch_ct_segment_scan, K.pk._h, x, seg_len, 0)
        assert K.decrypt(y) == [sum(m[r * seg_len:r * seg_len + t + 1]) % K.n for r in range(rows) for t in range(seg_len)]
        edge = [K.nsq - 1, 1, K.n + 1] + xs[3:]
        got = R.down(R.op(L.pgpu_batch_ct_segment_scan, K.pk._h, R.up(edge, 2 * K.nw), seg_len, REVERSE))
        assert got == _scan_expect(K, edge, seg_len, True)
    finally:
        K.close()


def _pack_shape(bits):
    """(seg_len, slot_bits) with seg_len * slot_bits == bits - 1 exactly: the smallest factor from 3 up, else 2; a prime
    bits - 1 packs bits - 1 one-bit slots"""
    cap = bits - 1
    for f in list(range(3, 50)) + [2]:
        if cap % f == 0:
            return f, cap // f
    return cap, 1


def _pack_expect(K, xs, seg_len, slot_bits):
    out = []
    for r in range(len(xs) // seg_len):                      # Horner, as the kernel: slot_bits squarings and one product per slot
        acc = xs[r * seg_len + seg_len - 1]
        for t in range(seg_len - 2, -1, -1):
            acc = pow(acc, 1 << slot_bits, K.nsq) * xs[r * seg_len + t] % K.nsq
        out.append(acc)
    return out


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_pack_at_the_capacity_bound(engine, knobs, bits):
    """seg_len * slot_bits = bitlen(n) - 1 exactly; one more bit is refused host-side; decrypt and unpack_slots return the
    slots"""
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 8)
    seg_len, slot_bits = _pack_shape(bits)
    assert seg_len * slot_bits == bits - 1
    rows = 2 if seg_len < 100 else 1
    try:
        m = [rng.getrandbits(slot_bits) for _ in range(rows * seg_len)]
        m[0], m[seg_len - 1] = (1 << slot_bits) - 1, (1 << slot_bits) - 1           # the first and the last slot full
        r = [rng.getrandbits(64) for _ in m]
        x = K.encrypt(m, r, K.mw)
        assert L.pgpu_batch_row_limbs(x) == 2 * K.l2
        xs = R.down(x)
        y = R.op(L.pgpu_batch_ct_pack, K.pk._h, x, seg_len, slot_bits)
        assert L.pgpu_batch_count(y) == rows and L.pgpu_batch_row_limbs(y) == 2 * K.l2
        assert R.down(y) == _pack_expect(K, xs, seg_len, slot_bits)
        dec = K.decrypt(y)
        assert dec == [sum(m[i * seg_len + t] << (slot_bits * t) for t in range(seg_len)) for i in range(rows)]
        assert engine.unpack_slots(dec, seg_len, slot_bits, width_bits=bits - 1) == m
        # one more bit: refused before anything is launched
        out = ctypes.c_void_p()
        assert L.pgpu_set_timing(1) == 0
        try:
            kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
            assert seg_len > 1
            assert L.pgpu_batch_ct_pack(K.pk._h, x, seg_len, slot_bits + 1, ctypes.byref(out)) == -1
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0 and not out.value
        finally:
            L.pgpu_set_timing(0)
        a, b, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert L.pgpu_ct_pack_plan(bits, rows, seg_len, slot_bits + 1, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr)) == -1
        assert L.pgpu_ct_pack_plan(bits, rows, seg_len, slot_bits, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr)) == 0
        assert pr.value == rows * (seg_len - 1) * (slot_bits + 1)
    finally:
        K.close()


def _edge_matrix(rng, rows, cols):
    """32-bit weights with 0, 1 and 2^32 - 1, an all-zero and an all-ones row (rows >= 3, cols >= 3)"""
    wm = [[rng.getrandbits(32) for _ in range(cols)] for _ in range(rows)]
    wm[0][:3] = [0, 1, (1 << 32) - 1]
    wm[1] = [0] * cols
    wm[2] = [(1 << 32) - 1] * cols
    return wm


def _spmv(K, x, row_ptr, col_idx, wb, e_bits):
    rp, ci = np.array(row_ptr, dtype=np.uint64), np.array(col_idx, dtype=np.uint32)
    return K.R.op(K.L.pgpu_batch_ct_spmv, K.pk._h, x, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p),
                  wb, len(row_ptr) - 1, e_bits)


def _spmv_expect(K, xs, row_ptr, col_idx, weights):
    out = []
    for i in range(len(row_ptr) - 1):
        acc = 1
        for t in range(row_ptr[i], row_ptr[i + 1]):
            acc = acc * pow(xs[col_idx[t]], weights[t], K.nsq) % K.nsq
        out.append(acc)
    return out


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_spmv(engine, knobs, bits):
    """5 rows over 7 columns: a full row, an empty one, one of a single entry; with the default chunk and with chunk 2 (the
    rows of 7 and 4 entries are cut into chains and folded)"""
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 10)
    cols = 7
    try:
        x, m = K.fresh(rng, cols)
        xs = R.down(x)
        row_ptr, col_idx = [0], []
        for length in (3, 0, 1, 7, 4):
            col_idx += rng.sample(range(cols), length)                          # (unsorted within a row)
            row_ptr.append(len(col_idx))
        weights = [rng.getrandbits(32) for _ in col_idx]
        weights[:3] = [0, 1, (1 << 32) - 1]
        weights[3] = (1 << 32) - 1                                               # the row of one entry
        weights[4:6] = [(1 << 32) - 1, 0]
        want = _spmv_expect(K, xs, row_ptr, col_idx, weights)
        assert want[1] == 1
        plain = [sum(weights[t] * m[col_idx[t]] for t in range(row_ptr[i], row_ptr[i + 1])) % K.n for i in range(5)]
        wb = R.up(weights, 1)
        chunk, levels = ctypes.c_int(), ctypes.c_int()
        for forced in (None, 2):
            knobs(spmv_chunk=forced)
            assert L.pgpu_ct_spmv_plan(bits, 5, cols, len(col_idx), 7, 32, None, ctypes.byref(chunk), ctypes.byref(levels), None, None) == 0
            if forced:
                assert chunk.value == 2 and levels.value > 1                     # fold levels exist
            y = _spmv(K, x, row_ptr, col_idx, wb, 32)
            assert L.pgpu_batch_count(y) == 5 and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, forced
            assert K.decrypt(y) == plain, forced
            edge = [1, K.nsq - 1, K.n + 1] + xs[3:]                              # word rows with the ends of the range
            assert R.down(_spmv(K, R.up(edge, 2 * K.nw), row_ptr, col_idx, wb, 32)) == _spmv_expect(K, edge, row_ptr, col_idx, weights), forced
    finally:
        K.close()


def _transpose(flat, outer, inner):
    """[outer][inner] -> [inner][outer]"""
    return [flat[a * inner + b] for b in range(inner) for a in range(outer)]


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_matmul(engine, knobs, bits):
    """3 vectors of 7 under a 5 x 7 matrix, in both layouts: with the plan's knobs, and with tiles of 2 vectors (a last pass
    of one; the transposed layout staged) over 3 column slices (folded)"""
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 11)
    n_vec, rows, cols = 3, 5, 7
    try:
        x, m = K.fresh(rng, n_vec * cols)
        xs = R.down(x)
        xt = R.up(_transpose(xs, n_vec, cols), 2 * K.nw)                         # the same matrix of ciphertexts stored [cols][n_vec]
        wm = _edge_matrix(rng, rows, cols)
        want = [v for k in range(n_vec) for v in _matvec_expect(K, xs[k * cols:(k + 1) * cols], wm)]
        assert [want[k * rows + 1] for k in range(n_vec)] == [1] * n_vec
        plain = [sum(a * w for a, w in zip(m[k * cols:(k + 1) * cols], row)) % K.n for k in range(n_vec) for row in wm]
        wb = R.up([v for row in wm for v in row], 1)
        sl, tile = ctypes.c_int(), ctypes.c_size_t()
        for forced in (None, (3, 2)):
            knobs(matmul_slices=forced and forced[0], matmul_tile=forced and forced[1])
            assert L.pgpu_ct_matmul_plan(bits, n_vec, rows, cols, 32, None, ctypes.byref(sl), ctypes.byref(tile), None, None) == 0
            if forced:
                assert (sl.value, tile.value) == forced and tile.value < n_vec
            y = R.op(L.pgpu_batch_ct_matmul, K.pk._h, x, wb, n_vec, rows, 32, 0)
            assert L.pgpu_batch_count(y) == n_vec * rows and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, forced
            assert K.decrypt(y) == plain, forced
            yt = R.op(L.pgpu_batch_ct_matmul, K.pk._h, xt, wb, n_vec, rows, 32, MATMUL_TRANSPOSED)
            assert L.pgpu_batch_count(yt) == n_vec * rows and L.pgpu_batch_row_limbs(yt) == 2 * K.l2
            assert R.down(yt) == _transpose(want, n_vec, rows), forced
            assert K.decrypt(yt) == _transpose(plain, n_vec, rows), forced
    finally:
        K.close()


def _bucket(K, x, weights, rows, e_bits):
    ww = (e_bits + 63) // 64
    wa = K.R.i2l(weights, ww)
    return K.R.op(K.L.pgpu_batch_ct_matvec_bucket, K.pk._h, x, wa.ctypes.data_as(ctypes.c_void_p), ww, rows, e_bits)


@pytest.mark.parametrize("bits", PAIR_WIDTHS)
def test_matvec_bucket(engine, knobs, bits):
    """2 x 40 under forced (c, b): both reduction levels, level 2 alone, level 1 alone; 13-bit weights and 65-bit ones in two
    words.  x once as pair rows from a resident encrypt (and through CRT decrypt), once as uploaded words with the ends of
    the value range in the first columns; the dense matvec on the same x and weights gives the same rows"""
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 12)
    rows, cols = 2, 40
    c, b = ctypes.c_int(), ctypes.c_int()
    try:
        x, m = K.fresh(rng, cols)
        xs = R.down(x)
        edge = [1, K.nsq - 1, K.n + 1, K.nsq - K.n + 1] + xs[4:]
        xe = R.up(edge, 2 * K.nw)
        for e_bits in (13, 65):
            w = [rng.getrandbits(e_bits) for _ in range(rows * cols)]
            w[:3] = [0, 1, (1 << e_bits) - 1]
            wm = [w[i * cols:(i + 1) * cols] for i in range(rows)]
            tail = _matvec_expect(K, xs[4:], [r[4:] for r in wm])                # the columns both inputs share: once
            want = [a * b4 % K.nsq for a, b4 in zip(tail, _matvec_expect(K, xs[:4], [r[:4] for r in wm]))]
            want_e = [a * b4 % K.nsq for a, b4 in zip(tail, _matvec_expect(K, edge[:4], [r[:4] for r in wm]))]
            plain = [sum(a * v for a, v in zip(m, r)) % K.n for r in wm]
            wb = R.up(w, (e_bits + 63) // 64)
            assert R.down(R.op(L.pgpu_batch_ct_matvec, K.pk._h, x, wb, rows, e_bits)) == want
            assert R.down(R.op(L.pgpu_batch_ct_matvec, K.pk._h, xe, wb, rows, e_bits)) == want_e
            for cw, blk in ((4, 4), (3, 1), (3, 8)):
                knobs(bucket_window=cw, bucket_block=blk)
                assert L.pgpu_ct_matvec_bucket_plan(bits, rows, cols, e_bits, ctypes.byref(c), ctypes.byref(b), None, None, None) == 0
                assert (c.value, b.value) == (cw, blk)
                y = _bucket(K, x, w, rows, e_bits)
                assert L.pgpu_batch_count(y) == rows and L.pgpu_batch_row_limbs(y) == 2 * K.l2
                assert R.down(y) == want, (e_bits, cw, blk)
                assert K.decrypt(y) == plain, (e_bits, cw, blk)
                assert R.down(_bucket(K, xe, w, rows, e_bits)) == want_e, (e_bits, cw, blk)
            knobs()
    finally:
        K.close()


@pytest.mark.parametrize("bits", [WIDE_WIDTHS[0], WIDE_WIDTHS[-1]])
def test_bucket_reductions_in_both_forms(engine, knobs, bits):
    """the first and the last width of the (4,18) class -- at the last one R = 2^8 P and no more, and the bucket reduction is
    lazily reduced end to end --: shape 3 of test_gpu_bucket.BASE_SHAPES puts both reduction levels beyond 8192 chains, on
    bucket_reduce_kernel<4,18>; its first two rows alone are a small call, on <8,9> as in test_matvec_bucket, and give the
    same rows"""
    import test_gpu_bucket as tb
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 13)
    (cw, blk, e_bits, rows), _ = tb.BASE_SHAPES[3]
    try:
        knobs(bucket_window=cw, bucket_block=blk)
        xv = [1, K.nsq - 1, K.n + 1, K.nsq - K.n + 1] + [rng.randrange(1, K.nsq) for _ in range(tb.BASE_COLS - 4)]
        x = R.up(xv, 2 * K.nw)
        y, table, pick = tb.base_form_shape(L, R, K.pk._h, bits, K.nsq, x, xv, 3, rng)
        W, levels = tb.reduce_chains(2, e_bits, cw, blk)
        assert all(tb.wide_pays(L, bits, lv[0]) for lv in levels)
        small = _bucket(K, x, table[pick[0]] + table[pick[1]], 2, e_bits)
        assert R.down(small) == R.down(y)[:2]
    finally:
        K.close()


@pytest.mark.parametrize("bits", WIDE_WIDTHS)
def test_base_and_wide_forms_agree(engine, knobs, bits):
    """keys of the (4,18) class run small launches of segment_sum and pack on 8 lanes per half with 9 limbs each: both
    forms, forced and on both sides of the threshold, give the same rows"""
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 9)
    lanes, limbs = ctypes.c_int(), ctypes.c_int()

    def plan(rows, seg_len, slot_bits):
        assert L.pgpu_ct_pack_plan(bits, rows, seg_len, slot_bits, ctypes.byref(lanes), ctypes.byref(limbs), None) == 0
        return lanes.value, limbs.value
    try:
        # pack: 37 rows of 3 slots, PGPU_PACK_WIDE = 0 / 1
        xs = [1, K.nsq - 1, K.n + 1] + [rng.randrange(1, K.nsq) for _ in range(37 * 3 - 3)]
        x = R.op(L.pgpu_batch_ct_add, K.pk._h, R.up(xs, 2 * K.nw), R.up([1], 2 * K.nw))        # pair rows
        assert L.pgpu_batch_row_limbs(x) == 144
        want = _pack_expect(K, xs, 3, 11)
        got = {}
        for wide in (0, 1):
            knobs(pack_wide=wide)
            assert plan(37, 3, 11) == ((8, 9) if wide else (4, 18))
            got[wide] = R.down(R.op(L.pgpu_batch_ct_pack, K.pk._h, x, 3, 11))
        assert got[0] == got[1] == want
        knobs()
        assert plan(37, 3, 11) == (8, 9) and plan(8193, 3, 11) == (4, 18)
        R.close()
        # segment_sum on both sides of the wide-form threshold (8192 chains): 8320 segments of 3 elements, then chunk 2
        cols, n_segments, groups = 192, 64, 130
        xs = [rng.randrange(1, K.nsq) for _ in range(cols)]
        x = R.up(xs, 2 * K.nw)
        ids = [j % n_segments for _ in range(groups) for j in range(cols)]
        want = _segsum_expect(K, xs, ids, groups, n_segments)
        base = R.down(_segsum(K, x, ids, groups, n_segments))                     # one level of 8320 chains: (4,18)
        knobs(segsum_chunk=2)
        mixed = R.down(_segsum(K, x, ids, groups, n_segments))                    # 16640 chains, then 8320 ... the folds in (8,9)
        knobs()
        small = R.down(_segsum(K, x, ids[:cols], 1, n_segments))                  # 64 chains: (8,9)
        assert base == mixed == want and small == want[:n_segments]
    finally:
        K.close()


# ---------------------------------------------------------------------------------------------------------------------
def test_keys_without_a_pair_form_refuse_the_aggregations(engine, knobs):
    """3212 bits: one bit beyond (8,14).  The element-wise chain runs on word rows (test_resident_chain); matvec,
    segment_sum, segment_scan, pack, spmv, matmul and the bucket matvec return PGPU_ERR_UNSUPPORTED before anything is
    launched, and so do their plans"""
    K = Key(engine, 3212)
    L, R = K.L, K.R
    rng = random.Random(3212)
    try:
        xs = [rng.randrange(1, K.nsq) for _ in range(6)]
        x = R.up(xs, 2 * K.nw)
        w = R.up([1, 2, 3, 4, 5, 6], 1)
        ids = np.zeros(6, dtype=np.uint32)
        row_ptr, col_idx = np.array([0, 3, 6], dtype=np.uint64), np.arange(6, dtype=np.uint32)
        wh = R.i2l([1, 2, 3, 4, 5, 6], 1)                                        # host weights of the bucket matvec
        out = ctypes.c_void_p()
        assert L.pgpu_set_timing(1) == 0
        try:
            kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
            assert L.pgpu_batch_ct_matvec(K.pk._h, x, w, 1, 32, ctypes.byref(out)) == UNSUPPORTED
            assert L.pgpu_batch_ct_segment_sum(K.pk._h, x, ids.ctypes.data_as(ctypes.c_void_p), 1, 2, ctypes.byref(out)) == UNSUPPORTED
            assert L.pgpu_batch_ct_segment_scan(K.pk._h, x, 3, 0, ctypes.byref(out)) == UNSUPPORTED
            assert L.pgpu_batch_ct_pack(K.pk._h, x, 3, 5, ctypes.byref(out)) == UNSUPPORTED
            assert not out.value
            assert L.pgpu_batch_ct_spmv(K.pk._h, x, row_ptr.ctypes.data_as(ctypes.c_void_p), col_idx.ctypes.data_as(ctypes.c_void_p),
                                        w, 2, 32, ctypes.byref(out)) == UNSUPPORTED
            assert b"pair" in L.pgpu_last_error() and not out.value
            for flags in (0, MATMUL_TRANSPOSED):                                 # 2 vectors of 3 under a 2 x 3 matrix
                assert L.pgpu_batch_ct_matmul(K.pk._h, x, w, 2, 2, 32, flags, ctypes.byref(out)) == UNSUPPORTED
                assert b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_batch_ct_matvec_bucket(K.pk._h, x, wh.ctypes.data_as(ctypes.c_void_p), 1, 1, 32, ctypes.byref(out)) == UNSUPPORTED
            assert b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0 and not out.value
        finally:
            L.pgpu_set_timing(0)
        a, b, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert L.pgpu_ct_matvec_plan(3212, 1, 6, 32, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr)) == UNSUPPORTED
        assert L.pgpu_ct_segment_sum_plan(3212, 6, 2, 6, ctypes.byref(a), ctypes.byref(b)) == UNSUPPORTED
        assert L.pgpu_ct_segment_scan_plan(3212, 2, 3, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr)) == UNSUPPORTED
        assert L.pgpu_ct_pack_plan(3212, 2, 3, 5, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr)) == UNSUPPORTED
        lv, tile = ctypes.c_int(), ctypes.c_size_t()
        assert L.pgpu_ct_spmv_plan(3212, 2, 6, 6, 3, 32, ctypes.byref(a), ctypes.byref(b), ctypes.byref(lv), ctypes.byref(pr), None) == UNSUPPORTED
        assert L.pgpu_ct_matmul_plan(3212, 2, 2, 3, 32, ctypes.byref(a), ctypes.byref(b), ctypes.byref(tile), ctypes.byref(pr), None) == UNSUPPORTED
        assert L.pgpu_ct_matvec_bucket_plan(3212, 1, 6, 32, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pr), None, None) == UNSUPPORTED
        assert b"pair" in L.pgpu_last_error()
        # ... and the same values still add, multiply and decrypt on word rows
        s = R.op(L.pgpu_batch_ct_add, K.pk._h, x, x)
        assert L.pgpu_batch_row_limbs(s) == 2 * K.l2 and R.down(s) == [v * v % K.nsq for v in xs]
    finally:
        K.close()


def test_pair_rows_decrypt_through_a_private_key_without_a_split_form(engine, knobs):
    """3211 bits: public pair rows (8,14), primes of 1605 / 1606 bits -- beyond the 1587 bits the private split forms hold.
    Rows from encrypt, CT + CT and pack become plain words on the way into the full-width CRT kernels (capi_batches.inc:
    pgpu_batch_decrypt_crt) and decrypt exactly"""
    from oracle import paillier_oracle as orc
    K = Key(engine, 3211)
    L, R = K.L, K.R
    rng = random.Random(3211)
    try:
        assert not K.split_private and K.form == (8, 14)
        assert _q3(L.pgpu_decrypt_kernel_form, K.sk._h, 37)[0] == 0
        x, m = K.fresh(rng, 37)
        x2, m2 = K.fresh(rng, 37)
        assert L.pgpu_batch_row_limbs(x) == 224
        assert K.decrypt(x) == m
        s = R.op(L.pgpu_batch_ct_add, K.pk._h, x, x2)
        assert L.pgpu_batch_row_limbs(s) == 224 and K.decrypt(s) == [(a + b) % K.n for a, b in zip(m, m2)]
        small = [rng.getrandbits(100) for _ in range(36)]
        xp = K.encrypt(small, [rng.getrandbits(64) for _ in small], K.mw)
        y = R.op(L.pgpu_batch_ct_pack, K.pk._h, xp, 12, 100)
        assert L.pgpu_batch_row_limbs(y) == 224
        assert engine.unpack_slots(K.decrypt(y), 12, 100, width_bits=3210) == small
        raw = [1, K.nsq - 1, K.n + 1, rng.randrange(1, K.nsq)]                      # uploaded words, no encryptions
        assert K.decrypt(R.up(raw, 2 * K.nw)) == orc.PrivateKey(K.n, K.p, K.q).decrypt(raw)
    finally:
        K.close()
