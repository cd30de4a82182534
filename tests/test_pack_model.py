"""The encrypted slot packing (pgpu_batch_ct_pack; csrc/hensel_pack.hpp: pack_kernel) on the CPU.

1. The kernel's schedule restated in plain integers: one Horner chain per row -- start as the LAST entry, then for
   t = seg_len - 2 ... 0 square slot_bits times and multiply by entry t -- held against prod_t x_t^(2^(b t)) mod n^2 from
   Python's pow, under a toy key, and through decrypt and unpack_slots back to the slot values.  (32, 64) needs a
   plaintext of more than 2048 bits: its schedule identity is checked under the toy key like the others (the identity
   is one of exponents, it holds modulo any n^2), its decrypt under the 3072-bit key of tests/golden.
2. unpack_slots, the pure host slicing of PublicKey.pack's way back.
3. pgpu_ct_pack_plan, the host-only query: the form, the product count and the refusals.
In the reference such a packed sum could only be composed from CipherText::operator* by plaintext powers of two and
CipherText::operator+ (ipcl/ciphertext.cpp), element by element."""
import ctypes
import json
import os
import random

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 5), (2, 1), (3, 7), (32, 64)]          # (seg_len, slot_bits)


class Key:
    """textbook Paillier with g = n + 1"""

    def __init__(self, p, q):
        self.p, self.q, self.n = p, q, p * q
        self.nsq = self.n * self.n
        self.lam = (p - 1) * (q - 1)
        self.mu = pow(self.lam, -1, self.n)

    def encrypt(self, m, rng):
        if not hasattr(self, "noise"):                            # r^n for a few r, multiplied up per call: still some r^n
            self.noise = [pow(rng.randrange(2, self.n), self.n, self.nsq) for _ in range(3)]
        return (1 + self.n * m) * rng.choice(self.noise) * rng.choice(self.noise) % self.nsq

    def decrypt(self, c):
        return (pow(c, self.lam, self.nsq) - 1) // self.n * self.mu % self.n


TOY = Key(4093, 4099)                                 # n of 24 bits: room for 3 slots of 7 bits


def big_key():
    c = [c for c in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"] if c["bits"] == 3072][0]
    return Key(int(c["p"], 16), int(c["q"], 16))


def pack_schedule(xs, rows, seg_len, slot_bits, nsq, ipw=16):
    """pack_kernel in integers: 64/G rows per wavefront, idle groups of the last wavefront clamp to the last row and store
    nothing; every chain of the launch has the same trip count"""
    out = [None] * rows
    stats = {"squarings": 0, "products": 0}
    for w0 in range(0, rows, ipw):
        for g in range(ipw):
            live = w0 + g < rows
            r = w0 + g if live else rows - 1
            row = xs[r * seg_len:(r + 1) * seg_len]
            acc = row[seg_len - 1]
            m = row[seg_len - 2 if seg_len > 1 else 0]            # the entry that travels under the squarings
            for t in range(seg_len - 2, -1, -1):
                for _ in range(slot_bits):
                    acc = acc * acc % nsq
                acc = acc * m % nsq
                m = row[t - 1 if t else 0]
                if live:
                    stats["squarings"] += slot_bits
                    stats["products"] += 1
            if live:
                assert out[r] is None
                out[r] = acc
    assert None not in out
    return out, stats


def direct(xs, rows, seg_len, slot_bits, nsq):
    out = []
    for r in range(rows):
        acc = 1
        for t in range(seg_len):
            acc = acc * pow(xs[r * seg_len + t], 1 << (slot_bits * t), nsq) % nsq
        out.append(acc)
    return out


@pytest.mark.parametrize("seg_len,slot_bits", SHAPES)
def test_schedule_equals_the_power_product(seg_len, slot_bits):
    from pailliercryptolib_amd import unpack_slots
    rng = random.Random(seg_len * 100 + slot_bits)
    fits_toy = seg_len * slot_bits <= TOY.n.bit_length() - 1
    for key in ([TOY] if fits_toy else [TOY, big_key()]):
        for rows in ((1, 3, 17) if key is TOY else (1, 3)):       # (the chains of the large key are 2015 products long)
            fits = seg_len * slot_bits <= key.n.bit_length() - 1
            ms = [rng.randrange(1 << slot_bits) for _ in range(rows * seg_len)]
            if fits:                                              # a slot at its largest value beside an empty one
                ms[0] = (1 << slot_bits) - 1
                if seg_len > 1:
                    ms[1] = 0
            xs = [key.encrypt(m, rng) for m in ms] if fits else [rng.randrange(1, key.nsq) for _ in ms]
            want = direct(xs, rows, seg_len, slot_bits, key.nsq)
            for ipw in (8, 16, 32):                               # 3072-, 2048- and 1024-bit key classes
                got, stats = pack_schedule(xs, rows, seg_len, slot_bits, key.nsq, ipw)
                assert got == want, (rows, ipw)
                assert stats["squarings"] + stats["products"] == rows * (seg_len - 1) * (slot_bits + 1)
            if seg_len == 1:
                assert want == xs                                 # a copy
            if fits:
                dec = [key.decrypt(c) for c in want]
                assert dec == [sum(ms[r * seg_len + t] << (slot_bits * t) for t in range(seg_len)) for r in range(rows)]
                assert unpack_slots(dec, seg_len, slot_bits, width_bits=key.n.bit_length() - 1) == ms
    assert fits_toy or seg_len * slot_bits <= big_key().n.bit_length() - 1      # every shape went through a decrypt


@pytest.mark.parametrize("b", [1, 7, 32, 64, 83])
def test_unpack_slots_slices_at_every_boundary(b):
    from pailliercryptolib_amd import unpack_slots
    rng = random.Random(b)
    ones = (1 << b) - 1
    for seg_len in (1, 2, 3, 24, 2047 // b):
        patterns = [[ones] * seg_len, [0] * seg_len, [ones if t % 2 else 0 for t in range(seg_len)],
                    [0 if t % 2 else ones for t in range(seg_len)], [rng.randrange(1 << b) for _ in range(seg_len)],
                    [1 << (b - 1)] * seg_len, [1] * seg_len]
        ms = [sum(v << (b * t) for t, v in enumerate(p)) for p in patterns]
        assert unpack_slots(ms, seg_len, b) == [v for p in patterns for v in p]
        assert unpack_slots(ms, seg_len, b, width_bits=seg_len * b) == [v for p in patterns for v in p]
        with pytest.raises(ValueError):
            unpack_slots(ms, seg_len, b, width_bits=seg_len * b - 1)      # more slot bits than the plaintext is wide
        with pytest.raises(ValueError):
            unpack_slots([1 << (seg_len * b)], seg_len, b)                 # a bit beyond the last slot
    assert unpack_slots([], 3, b) == []
    for seg_len, bits in ((0, b), (-1, b), (3, 0), (3, -b)):
        with pytest.raises(ValueError):
            unpack_slots([0], seg_len, bits)
    with pytest.raises(ValueError):
        unpack_slots([-1], 1, b)


def _plan(key_bits, rows, seg_len, slot_bits):
    from pailliercryptolib_amd import _capi
    L = _capi.lib()
    lanes, limbs, products = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = L.pgpu_ct_pack_plan(key_bits, rows, seg_len, slot_bits, ctypes.byref(lanes), ctypes.byref(limbs), ctypes.byref(products))
    return rc, lanes.value, limbs.value, products.value


def test_pack_plan_is_host_only(monkeypatch):
    from pailliercryptolib_amd import _capi
    monkeypatch.delenv("PGPU_PACK_WIDE", raising=False)
    L = _capi.lib()
    assert _plan(1024, 5, 15, 64) == (0, 2, 19, 5 * 14 * 65)
    assert _plan(2048, 32768, 31, 64) == (0, 4, 18, 32768 * 30 * 65)
    assert _plan(2048, 32768, 16, 32) == (0, 4, 18, 32768 * 15 * 33)
    assert _plan(3072, 7, 32, 64) == (0, 8, 14, 7 * 31 * 65)
    assert _plan(2048, 9, 1, 5) == (0, 8, 9, 0)                           # a copy: no product
    # 2048-bit keys: the same rows on 8 lanes per half while that leaves at most one wavefront per SIMD (8 rows each)
    assert _plan(2048, 64, 31, 64)[:3] == _plan(2048, 2048, 31, 64)[:3] == _plan(2048, 8192, 31, 64)[:3] == (0, 8, 9)
    assert _plan(2048, 8193, 31, 64)[:3] == (0, 4, 18)
    assert _plan(1024, 1, 15, 64)[:3] == (0, 2, 19) and _plan(3072, 1, 32, 64)[:3] == (0, 8, 14)   # no such form there
    for bits in (1024, 2048, 3072):
        # the capacity bound is key_bits - 1: a pack that wraps modulo n is never meant
        assert _plan(bits, 1, 1, bits)[0] == -1 and b"wrap" in L.pgpu_last_error()
        assert _plan(bits, 1, bits, 1)[0] == -1 and _plan(bits, 1, bits // 64, 64)[0] == -1
        assert _plan(bits, 1, 1, bits - 1)[0] == 0 and _plan(bits, 1, bits - 1, 1)[0] == 0
        assert _plan(bits, 3, 2, (bits - 1) // 2)[:1] == (0,) and _plan(bits, 3, 2, (bits - 1) // 2)[3] == 3 * ((bits - 1) // 2 + 1)
        assert _plan(bits, 1, 2, 0)[0] == -1 and _plan(bits, 1, 2, -3)[0] == -1
        assert _plan(bits, 1, 0, 8)[0] == -1 and _plan(bits, 0, 2, 8)[0] == -1
        # seg_len * slot_bits beyond 64 bits: 2^62 * 4 == 0 and (2^63 + 1) * 2 == 2 modulo 2^64 must not pass as small
        assert _plan(bits, 1, 1 << 62, 4)[0] == -1 and _plan(bits, 1, (1 << 63) + 1, 2)[0] == -1
        assert _plan(bits, 1, (1 << 64) - 1, (1 << 31) - 1)[0] == -1
    assert _plan(4096, 4, 8, 32)[0] == -3 and b"pair" in L.pgpu_last_error()   # PGPU_ERR_UNSUPPORTED: no pair rows
    assert _plan(0, 4, 8, 32)[0] == -1
    assert L.pgpu_ct_pack_plan(2048, 4, 8, 32, None, None, None) == 0          # every output is optional
    assert _plan(2048, (1 << 64) - 1, 16, 32)[0] == -1                         # the product count itself overflows


def test_binding_names_the_new_symbols():
    from pailliercryptolib_amd import _capi
    assert {"pgpu_batch_ct_pack", "pgpu_ct_pack_plan"} <= set(_capi.SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "pgpu.h")).read()
    assert "PGPU_KERNEL_PACK = 8" in hdr
