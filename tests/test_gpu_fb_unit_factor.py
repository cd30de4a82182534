"""DJN encrypt on the UNIT-FACTOR fixed-base table (csrc/hensel.hpp: hensel_fb_build_kernel): a table entry is (alpha, beta)
with g == alpha * (1 + n*beta) mod n^2, the kernels multiply the pairs (alpha, 0) -- two half-width products per step instead of
three -- and add the betas, whose sum joins the plaintext in the closing 1 + n*m product.  Every encrypt form is forced --
paired halves (hensel_fb_encrypt_kernel, pair rows and words), sequential halves (hensel_fb_encrypt_seq_kernel),
wavefront-wide (hensel_fb_encrypt_wave_kernel), the quarter-chip launches beside busy lanes -- with indexed and masked table
access, for 1024-, 2048- and 3072-bit keys, at 1 / 63 / 65 / 300 / 4100 / 8192 elements, and held bit-identical with the oracle
(up to 300 elements: every row against oracle/paillier_oracle.py; above: every row against the C oracle, sample rows against
the Python one).  Randomness 0, 1, all ones and every-window-one patterns; plaintexts 0 and n - 1; results decrypt back.
tests/test_fb_unit_factor_model.py is the integer model of the same arithmetic."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SIZES = [1, 63, 65, 300, 4100, 8192]


def key_case(bits):
    if bits == 2048:
        k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
        return int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
    c = [c for c in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"] if c["bits"] == bits and c["djn"]][0]
    return int(c["p"], 16), int(c["q"], 16), int(c["hs"], 16)


def inputs(bits, count, n, seed):
    rb = bits // 2
    rng = random.Random(seed)
    every = lambda w: sum(1 << (w * i) for i in range((rb + w - 1) // w)) & ((1 << rb) - 1)     # every window of width w is 1
    edge_r = [0, 1, (1 << rb) - 1, every(4), every(5), every(8), every(12), every(13), 1 << (rb - 1)]
    edge_m = [0, n - 1, n - 1, 0, 1, n - 1, 0, n - 2, n - 1]
    r = (edge_r + [rng.getrandbits(rb) for _ in range(count)])[:count]
    m = (edge_m + [rng.randrange(n) for _ in range(count)])[:count]
    return m, r


class Want:
    """the oracle's ciphertexts of (m, r): all rows from the Python oracle up to 300 elements; above, all rows from the C oracle
    and the first rows (the edge cases) and a few others from the Python one"""

    def __init__(self, bits, n, p, q, hs, m, r):
        from oracle import paillier_oracle as orc
        from pailliercryptolib_amd.limbs import ints_to_limbs, limbs_to_ints
        opk = orc.PublicKey(n, bits)
        opk.set_djn(hs)
        nw = bits // 64
        if len(m) <= 300:
            self.rows = opk.encrypt(m, r)
        else:
            from oracle import c_oracle
            c_oracle.set_threads(min(c_oracle.lib().orc_max_threads(), c_oracle.usable_cpus()))
            be = c_oracle.ifma_modexp_batch if c_oracle.ifma_lib() is not None else (
                c_oracle.openssl_modexp_batch if c_oracle.openssl_lib() is not None else c_oracle.modexp_batch)
            c = c_oracle.paillier_encrypt_with(be, ints_to_limbs([n], nw)[0], ints_to_limbs([hs], 2 * nw)[0],
                                               ints_to_limbs(m, nw), ints_to_limbs(r, nw // 2))
            self.rows = limbs_to_ints(np.ascontiguousarray(c, dtype=np.uint64))
            pick = list(range(12)) + [len(m) // 2, len(m) - 1]
            assert [self.rows[i] for i in pick] == opk.encrypt([m[i] for i in pick], [r[i] for i in pick]), "the two oracles differ"


class Res:
    def __init__(self):
        from pailliercryptolib_amd import _capi
        from pailliercryptolib_amd.limbs import ints_to_limbs, limbs_to_ints
        self.L, self.check, self.i2l, self.l2i = _capi.lib(), _capi.check, ints_to_limbs, limbs_to_ints
        self.live = []

    def up(self, vals, words):
        h = ctypes.c_void_p()
        a = self.i2l(vals, words)
        self.check(self.L.pgpu_batch_upload(a.ctypes.data_as(ctypes.c_void_p), len(vals), words, words, ctypes.byref(h)))
        self.live.append(h)
        return h

    def down(self, h):
        out = np.empty((self.L.pgpu_batch_count(h), self.L.pgpu_batch_words(h)), dtype=np.uint64)
        self.check(self.L.pgpu_batch_download(h, out.ctypes.data_as(ctypes.c_void_p)))
        return self.l2i(out)

    def op(self, fn, *a):
        h = ctypes.c_void_p()
        self.check(fn(*a, ctypes.byref(h)))
        self.live.append(h)
        return h

    def close(self):
        for h in self.live:
            self.L.pgpu_batch_destroy(h)
        self.live = []


@pytest.mark.parametrize("count", SIZES)
@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_every_encrypt_form_matches_the_oracle(engine, bits, count):
    from pailliercryptolib_amd import _capi
    p, q, hs = key_case(bits)
    n = p * q
    nw, rb = bits // 64, bits // 2
    m, r = inputs(bits, count, n, 1000 * bits + count)
    want = Want(bits, n, p, q, hs, m, r).rows
    pk, sk = engine.PublicKey(n, bits, hs=hs), engine.PrivateKey(p, q)
    R = Res()
    L = R.L
    l2 = {1024: 38, 2048: 72, 3072: 112}[bits]

    def form():
        split, lanes, limbs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _capi.check(L.pgpu_encrypt_kernel_form_ex(pk._h, nw, count, -1, ctypes.byref(split), ctypes.byref(lanes), ctypes.byref(limbs)))
        return split.value

    def resident(what):
        c = R.op(L.pgpu_batch_encrypt, pk._h, hm, hr, rb)
        assert L.pgpu_batch_row_limbs(c) == 2 * l2, what + ": not a pair row"
        assert R.down(c) == want, what + ": differs from the oracle"
        return c
    try:
        hm, hr = R.up(m, nw), R.up(r, nw // 2)
        for masked in (0, 1):
            _capi.check(L.pgpu_set_table_gather_policy(masked))
            tag = " (masked)" if masked else " (indexed)"
            # words in, words out: the paired kernel's way back to a full-width residue
            L.pgpu_debug_set_wave_decrypt(0)
            L.pgpu_debug_set_seq_decrypt(0)
            assert pk.encrypt(m, r) == want, "paired halves, words" + tag
            # resident results: paired halves, sequential halves, wavefront-wide
            c = resident("paired halves" + tag)
            L.pgpu_debug_set_seq_decrypt(2)
            cs = resident("sequential halves" + tag)
            L.pgpu_debug_set_seq_decrypt(0)
            if count <= 1024:
                L.pgpu_debug_set_wave_decrypt(2)
                assert form() == 5
                c = resident("wavefront-wide" + tag)
                L.pgpu_debug_set_wave_decrypt(0)
            assert R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, c)) == m
            assert R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, cs)) == m
        # the default policy, whatever it picks at this size
        _capi.check(L.pgpu_set_table_gather_policy(0))
        L.pgpu_debug_set_wave_decrypt(1)
        L.pgpu_debug_set_seq_decrypt(4)
        resident("default policy")
        assert sk.decrypt(pk.encrypt(m[:300], r[:300])) == m[:300]
    finally:
        _capi.check(L.pgpu_set_table_gather_policy(0))
        L.pgpu_debug_set_wave_decrypt(1)
        L.pgpu_debug_set_seq_decrypt(4)
        R.close()


def window_worker(w):
    """body of test_wide_and_narrow_windows, in a process of its own started with PGPU_FB_WINDOW=w"""
    import pailliercryptolib_amd as pa
    from pailliercryptolib_amd import _capi
    pa.initialize()
    bits = 2048
    p, q, hs = key_case(bits)
    n = p * q
    nw, rb = bits // 64, bits // 2
    m, r = inputs(bits, 300, n, 77 + w)
    want = Want(bits, n, p, q, hs, m, r).rows
    R = Res()
    L = R.L
    try:
        pk, sk = pa.PublicKey(n, bits, hs=hs), pa.PrivateKey(p, q)
        hm, hr = R.up(m, nw), R.up(r, nw // 2)
        L.pgpu_debug_set_wave_decrypt(0)
        for seq in (0, 2):
            L.pgpu_debug_set_seq_decrypt(seq)
            c = R.op(L.pgpu_batch_encrypt, pk._h, hm, hr, rb)
            assert R.down(c) == want
            assert R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, c)) == m
        win, nbytes, ms = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_double()
        _capi.check(L.pgpu_pubkey_fixed_base_info(pk._h, 0, ctypes.byref(win), ctypes.byref(nbytes), ctypes.byref(ms)))
        assert win.value == w and nbytes.value == ((rb + w - 1) // w << w) * 2 * 72 * 4 and ms.value > 0
    finally:
        R.close()
        pa.terminate()
    print("window ok", w)


@pytest.mark.parametrize("w", [5, 12, 13])
def test_wide_and_narrow_windows(engine, w):
    """the table at the bench's window (13 bits: 79 rows of 8192 entries, inverted in 8 segments each), one below it (4
    segments), and a narrow one: 300 elements through the paired and the sequential-halves kernel.  An explicit window stays
    explicit for the life of a process (young keys then skip their 8-bit table), so the case runs in a process of its own,
    which takes the window from PGPU_FB_WINDOW."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PGPU_FB_WINDOW=str(w), PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(w)], capture_output=True, text=True, timeout=600,
                       env=env, cwd=root)
    assert r.returncode == 0 and "window ok %d" % w in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_four_lanes_in_flight(engine):
    """the headline's shape: four resident batches of 8192 in flight under the 2048-bit key -- beside three busy lanes every
    encrypt is a quarter-chip launch of hensel_fb_encrypt_seq_kernel<4,18> under its CU claim.  Every lane's ciphertexts
    against the C oracle, sample rows against the Python one, and the round trip."""
    from pailliercryptolib_amd import _capi
    bits, count = 2048, 8192
    p, q, hs = key_case(bits)
    n = p * q
    nw, rb = bits // 64, bits // 2
    pk, sk = engine.PublicKey(n, bits, hs=hs), engine.PrivateKey(p, q)
    R = Res()
    L = R.L
    try:
        sets = []
        for ln in range(4):
            m, r = inputs(bits, count, n, 4242 + ln)
            _capi.check(L.pgpu_set_batch_lane(ln))
            sets.append((m, Want(bits, n, p, q, hs, m, r).rows, R.up(m, nw), R.up(r, nw // 2)))
        cts, outs = [None] * 4, [None] * 4
        for _ in range(3):                      # (the first round starts beside idle lanes: the later ones run the quarter-chip forms)
            for ln in range(4):
                _capi.check(L.pgpu_set_batch_lane(ln))
                cts[ln] = R.op(L.pgpu_batch_encrypt, pk._h, sets[ln][2], sets[ln][3], rb)
                outs[ln] = R.op(L.pgpu_batch_decrypt_crt, sk._h, cts[ln])
        _capi.check(L.pgpu_set_batch_lane(0))
        _capi.check(L.pgpu_synchronize())
        for ln in range(4):
            assert R.down(cts[ln]) == sets[ln][1], "lane %d: ciphertexts differ from the oracle" % ln
            assert R.down(outs[ln]) == sets[ln][0], "lane %d: round trip failed" % ln
    finally:
        _capi.check(L.pgpu_set_batch_lane(0))
        R.close()


if __name__ == "__main__":
    import sys
    window_worker(int(sys.argv[1]))
