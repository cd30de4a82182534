"""The encrypted slot packing of resident ciphertexts (pgpu_batch_ct_pack; csrc/hensel_pack.hpp) on the GPU: x read as
[rows][seg_len],
    out[r] = prod_t x[r][t]^(2^(slot_bits t)) mod n^2        i.e. Dec(out[r]) = sum_t Dec(x[r][t]) 2^(slot_bits t) mod n
held bit-identical to Python integers for the 1024-, 2048- and 3072-bit key classes: every shape class (a single element,
the shortest chain, rows that do not fill a wavefront's groups, rows across the 8 / 16 / 32 chains of a wavefront of the
three geometries, a second workgroup, the workload's slot shape, the longest squaring run at the capacity bound), inputs
in every form a resident ciphertext batch can have, edge ciphertexts, the round trip through CRT decrypt and
unpack_slots, the agreement with the matrix-vector route, two lanes at once, the timing record and the refusals.

The workload's slot shape is 32 slots of 64 bits.  That is 2048 bits, which a 2048-bit n does not hold (the call refuses
seg_len * slot_bits > bitlen(n) - 1: such a pack wraps modulo n) -- so, as 15 slots stand for 16 under a 1024-bit key, 31
slots stand for 32 under a 2048-bit key, and test_refusals_are_host_side holds that 32 x 64 is refused there.

In the reference such a packed sum could only be composed from CipherText::operator* by plaintext powers of two and
CipherText::operator+ (ipcl/ciphertext.cpp), element by element."""
import ctypes
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_gpu_pair_rows import Res, key_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [1024, 2048, 3072]
KIND_PACK, FORM_SEQ = 8, 2            # PGPU_KERNEL_PACK, PGPU_FORM_SEQ (include/pgpu.h)
SLOTS = {1024: 15, 2048: 31, 3072: 32}                    # slots of 64 bits that fit below the bits of n


def shapes(bits):
    """(rows, seg_len, slot_bits)"""
    return [(1, 1, 1), (1, 2, 1), (3, 7, 5), (17, 3, 2), (33, 2, 7), (130, 2, 1), (2, SLOTS[bits], 64), (2, 2, (bits - 1) // 2)]


class Case:
    """a key, and helpers that keep everything resident"""

    def __init__(self, engine, bits):
        self.bits = bits
        self.p, self.q, self.hs = key_case(bits, True)
        self.n = self.p * self.q
        assert self.n.bit_length() == bits
        self.nsq = self.n * self.n
        self.nw = bits // 64
        self.pk, self.sk = engine.PublicKey(self.n, bits, hs=self.hs), engine.PrivateKey(self.p, self.q)
        self.R = Res()
        self.L = self.R.L

    def encrypt(self, m, rng):
        rw = self.bits // 128
        r = [rng.getrandbits(64 * rw) for _ in m]
        return self.R.op(self.L.pgpu_batch_encrypt, self.pk._h, self.R.up(m, self.nw), self.R.up(r, rw), 64 * rw)

    def pack(self, x, seg_len, slot_bits):
        return self.R.op(self.L.pgpu_batch_ct_pack, self.pk._h, x, seg_len, slot_bits)

    def expect(self, xs, seg_len, slot_bits):
        out = []
        for r in range(len(xs) // seg_len):
            acc = 1
            for t in range(seg_len):
                acc = acc * pow(xs[r * seg_len + t], 1 << (slot_bits * t), self.nsq) % self.nsq
            out.append(acc)
        return out

    def decrypt(self, y):
        return self.R.down(self.R.op(self.L.pgpu_batch_decrypt_crt, self.sk._h, y))


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.delenv("PGPU_PACK_WIDE", raising=False)

    def force(wide=None):
        if wide is None:
            monkeypatch.delenv("PGPU_PACK_WIDE", raising=False)
        else:
            monkeypatch.setenv("PGPU_PACK_WIDE", str(int(wide)))
    return force


def plan_form(bits, rows, seg_len, slot_bits):
    from pailliercryptolib_amd import _capi
    lanes, limbs = ctypes.c_int(), ctypes.c_int()
    assert _capi.lib().pgpu_ct_pack_plan(bits, rows, seg_len, slot_bits, ctypes.byref(lanes), ctypes.byref(limbs), None) == 0
    return lanes.value, limbs.value


@pytest.mark.parametrize("bits,wide", [(1024, None), (2048, None), (2048, 0), (3072, None)])
def test_pack_is_exact_at_every_shape(engine, knobs, bits, wide):
    """x from a resident DJN encrypt.  wide = 0 keeps 2048-bit keys in their (4,18) form, which the rule (policy.hpp:
    pack_wide_pays) leaves to launches of more than 8192 rows; the other key classes have one form"""
    knobs(wide)
    assert plan_form(bits, 1, 1, 1) == {1024: (2, 19), 2048: (4, 18) if wide == 0 else (8, 9), 3072: (8, 14)}[bits]
    c = Case(engine, bits)
    rng = random.Random(bits)
    L = c.L
    try:
        for rows, seg_len, slot_bits in shapes(bits):
            x = c.encrypt([rng.randrange(c.n) for _ in range(rows * seg_len)], rng)
            xs = c.R.down(x)
            y = c.pack(x, seg_len, slot_bits)
            assert L.pgpu_batch_count(y) == rows
            assert L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(x) > 0 and L.pgpu_batch_lane(y) == L.pgpu_batch_lane(x)
            assert c.R.down(y) == c.expect(xs, seg_len, slot_bits), (rows, seg_len, slot_bits)
            assert c.R.down(x) == xs                                # the input is left as it was
            c.R.close()
    finally:
        c.R.close()


def test_the_threshold_between_the_two_forms_of_2048_bit_keys(engine, knobs):
    """8192 rows still run on 8 lanes per half, 8193 on 4; and each form forced onto the other's side"""
    c = Case(engine, 2048)
    rng = random.Random(77)
    R = c.R
    try:
        pool = [rng.randrange(1, c.nsq) for _ in range(64)]
        xs = [pool[(i * 7 + i // 64) % 64] for i in range(2 * 8193)]
        want = c.expect(xs, 2, 3)
        for rows, form in ((8192, (8, 9)), (8193, (4, 18))):
            assert plan_form(2048, rows, 2, 3) == form
            x = R.up(xs[:2 * rows], 2 * c.nw)
            assert R.down(c.pack(x, 2, 3)) == want[:rows], rows
            knobs(form != (8, 9))                                # the other form on the same rows
            assert plan_form(2048, rows, 2, 3) != form
            assert R.down(c.pack(x, 2, 3)) == want[:rows], (rows, "forced")
            knobs(None)
            R.close()
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_inputs_in_every_form(engine, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    L, R = c.L, c.R
    try:
        rows, seg_len, slot_bits = 5, 6, 9
        x = c.encrypt([rng.randrange(c.n) for _ in range(rows * seg_len)], rng)   # resident DJN encrypt: pair rows
        xs = R.down(x)
        want = c.expect(xs, seg_len, slot_bits)
        assert R.down(c.pack(x, seg_len, slot_bits)) == want
        u = R.up(xs, 2 * c.nw)                                                    # uploaded plain ciphertext words
        assert L.pgpu_batch_row_limbs(u) == 0
        y = c.pack(u, seg_len, slot_bits)
        assert R.down(y) == want and L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(x) > 0
        assert R.down(u) == xs
        s = R.op(L.pgpu_batch_ct_segment_scan, c.pk._h, x, seg_len, 0)            # the output of segment_scan
        ss = R.down(s)
        assert R.down(c.pack(s, seg_len, slot_bits)) == c.expect(ss, seg_len, slot_bits)
        assert R.down(c.pack(s, 3, 17)) == c.expect(ss, 3, 17)
        # a packed batch is an ordinary resident batch: it feeds the other operations, and a pack of packs is a wider pack
        z = c.pack(y, rows, seg_len * slot_bits)
        assert L.pgpu_batch_count(z) == 1 and R.down(z) == c.expect(xs, rows * seg_len, slot_bits)
        both = R.op(L.pgpu_batch_ct_add, c.pk._h, y, y)
        assert R.down(both) == [v * v % c.nsq for v in want]
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_edge_values(engine, bits):
    """the edge ciphertexts of the segmented-sum tests: 1 and n^2 - 1 at the first slot, at the last slot, and in runs"""
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    R = c.R
    try:
        top, seg_len = c.nsq - 1, 6
        rnd = lambda k: [rng.randrange(1, c.nsq) for _ in range(k)]   # noqa: E731
        rows = [[1] + rnd(5), [top] + rnd(5), rnd(5) + [1], rnd(5) + [top], [1] * 6, [top] * 6, [1, 1, 1, top, top, top],
                [top, top, 1, 1] + rnd(2), [top, 1, top, 1, top, 1]]
        xs = [v for row in rows for v in row]
        x = R.up(xs, 2 * c.nw)
        for slot_bits in (1, 2, 11):
            assert R.down(c.pack(x, seg_len, slot_bits)) == c.expect(xs, seg_len, slot_bits), slot_bits
        for seg_len, slot_bits in ((1, 3), (2, 5), (3, 4), (len(xs), 2)):
            assert R.down(c.pack(x, seg_len, slot_bits)) == c.expect(xs, seg_len, slot_bits), (seg_len, slot_bits)
        assert R.down(c.pack(R.up([1] * 10, 2 * c.nw), 5, 8)) == [1, 1]
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_round_trip_through_decrypt_and_unpack(engine, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    try:
        for rows, seg_len, b in ((3, 7, 5), (2, SLOTS[bits], 64), (4, 2, 1), (33, 2, 7)):
            m = [rng.randrange(1 << b) for _ in range(rows * seg_len)]
            m[0], m[1] = (1 << b) - 1, 0                       # a slot at its largest value next to an empty one
            m[-2], m[-1] = 0, (1 << b) - 1
            y = c.pack(c.encrypt(m, rng), seg_len, b)
            d = c.decrypt(y)
            assert len(d) == rows
            assert d == [sum(m[r * seg_len + t] << (b * t) for t in range(seg_len)) for r in range(rows)]
            assert engine.unpack_slots(d, seg_len, b, width_bits=c.n.bit_length() - 1) == m, (rows, seg_len, b)
            c.R.close()
        # headroom is the caller's: 16-bit values in 20-bit slots, 16 packed rows added slot-wise stay apart
        rows, seg_len, b = 16, 5, 20
        m = [rng.randrange(1 << 16) for _ in range(rows * seg_len)]
        y = c.pack(c.encrypt(m, rng), seg_len, b)
        total = c.R.op(c.L.pgpu_batch_ct_segment_sum, c.pk._h, y, np.zeros(rows, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p), 1, 1)
        assert engine.unpack_slots(c.decrypt(total), seg_len, b) == [sum(m[r * seg_len + t] for r in range(rows)) for t in range(seg_len)]
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_agrees_with_the_matvec_route(engine, bits):
    """what a caller could do before: one matrix row with the weights 2^(8 t)"""
    c = Case(engine, bits)
    rng = random.Random(bits + 4)
    L, R = c.L, c.R
    try:
        m = [rng.randrange(256) for _ in range(4)]
        x = c.encrypt(m, rng)
        w = R.up([1 << (8 * t) for t in range(4)], 1)
        mv = R.op(L.pgpu_batch_ct_matvec, c.pk._h, x, w, 1, 25)
        y = c.pack(x, 4, 8)
        assert R.down(y) == R.down(mv)                          # both leave the device canonical: bit-identical
        assert c.decrypt(y) == c.decrypt(mv) == [sum(v << (8 * t) for t, v in enumerate(m))]
    finally:
        R.close()


def test_two_lanes_at_once(engine):
    """two threads on different batch lanes, each with its own inputs; one run"""
    c = Case(engine, 2048)
    L = c.L
    results, errors = {}, []

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            rng = random.Random(800 + lane)
            rows, seg_len, b = 18 + lane, 3 + lane, 30 + lane
            xs = [rng.randrange(1, c.nsq) for _ in range(rows * seg_len)]
            x = R.up(xs, 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for rep in range(2):
                y = R.op(L.pgpu_batch_ct_pack, c.pk._h, x, seg_len, b)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, rep)] = (R.down(y), xs, seg_len, b)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(results) == 4
    for got, xs, seg_len, b in results.values():
        assert got == c.expect(xs, seg_len, b)


def test_launch_carries_the_pack_kind(engine):
    c = Case(engine, 2048)
    rng = random.Random(12)
    L, R = c.L, c.R
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(40 * 3)], rng)    # pair rows already: no conversion launch
        xs = R.down(x)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            for seg_len, b in ((3, 12), (1, 4)):                           # (a copy is the same one launch)
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)             # drop what earlier calls left
                y = c.pack(x, seg_len, b)
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)         # (before the download, which may launch a conversion)
                assert n == 1 and kinds[0] == KIND_PACK and forms[0] == FORM_SEQ and ms[0] > 0
                assert R.down(y) == c.expect(xs, seg_len, b)
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_refusals_are_host_side(engine):
    """every refusal of the call but one: the refusal for pools of more than one GPU cannot be provoked on one GPU and is
    NOT covered here (nor is it for the sibling aggregation calls)"""
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(10)
    try:
        xs = [rng.randrange(1, c.nsq) for _ in range(6)]
        x = R.up(xs, 2 * c.nw)
        out = ctypes.c_void_p()

        def call(key, xb, seg_len, slot_bits):
            return L.pgpu_batch_ct_pack(key, xb, seg_len, slot_bits, ctypes.byref(out))
        assert call(c.pk._h, x, 0, 8) == -1 and b"seg_len" in L.pgpu_last_error()
        assert call(c.pk._h, x, 4, 8) == -1 and call(c.pk._h, x, 7, 8) == -1       # 6 % seg_len != 0
        assert call(c.pk._h, x, 3, 0) == -1 and b"slot_bits" in L.pgpu_last_error()
        assert call(c.pk._h, x, 3, -1) == -1 and call(c.pk._h, x, 1, -(1 << 31)) == -1
        # the capacity bound: seg_len * slot_bits <= bitlen(n) - 1 = 2047
        assert call(c.pk._h, x, 2, 1024) == -1 and b"wrap" in L.pgpu_last_error()
        assert call(c.pk._h, x, 1, 2048) == -1 and call(c.pk._h, x, 6, 342) == -1 and call(c.pk._h, x, 3, (1 << 31) - 1) == -1
        x64 = R.up([rng.randrange(1, c.nsq) for _ in range(64)], 2 * c.nw)
        assert call(c.pk._h, x64, 32, 64) == -1 and b"wrap" in L.pgpu_last_error()   # 32 slots of 64 bits: not under a 2048-bit n
        assert call(None, x, 3, 8) == -1 and call(c.pk._h, None, 3, 8) == -1
        assert L.pgpu_batch_ct_pack(c.pk._h, x, 3, 8, None) == -1
        assert call(c.pk._h, R.up([3, 5], c.nw), 2, 8) == -1 and b"width" in L.pgpu_last_error()
        # a batch of another key: pair rows of a 1024-bit key, and words of the wrong width
        c1 = Case(engine, 1024)
        try:
            x1 = c1.encrypt([1, 2, 3, 4, 5, 6], rng)
            assert call(c.pk._h, x1, 3, 8) == -1
            p3, q3, hs3 = key_case(3072, True)
            assert call(engine.PublicKey(p3 * q3, 3072, hs=hs3)._h, x, 3, 8) == -1
        finally:
            c1.R.close()
        assert not out.value                                   # (stale handles: test_stale_handles_are_refused, own process)
        assert R.down(c.pack(x, 1, 2047)) == xs and R.down(c.pack(x, 6, 341)) == c.expect(xs, 6, 341)   # at the bound: fine
        # the masked table-gather policy: refused, and the text says why; switched off again the call works
        assert L.pgpu_set_table_gather_policy(1) == 0
        try:
            assert call(c.pk._h, x, 3, 8) == -3
            assert b"masked" in L.pgpu_last_error() and not out.value
        finally:
            L.pgpu_set_table_gather_policy(0)
        assert R.down(c.pack(x, 3, 8)) == c.expect(xs, 3, 8)
        # a key class without pair rows
        p4, q4, _ = key_case(4096, False)
        pk4 = engine.PublicKey(p4 * q4, 4096)
        x4 = R.up([3, 5], 128)
        assert call(pk4._h, x4, 2, 8) == -3 and b"pair" in L.pgpu_last_error() and not out.value
    finally:
        R.close()


_NO_PAIR_ROWS = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
pk = pa.PublicKey(p * q, 2048, hs=hs)
R = Res()
x = R.up([3, 5, 7, 9], 64)
out = ctypes.c_void_p()
rc = R.L.pgpu_batch_ct_pack(pk._h, x, 2, 8, ctypes.byref(out))
print("rc", rc, R.L.pgpu_last_error().decode())
R.close()
sys.exit(0 if rc == -3 and not out.value else 1)
"""


_STALE = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
nsq = (p * q) ** 2
R = Res()
L = R.L
old_key = pa.PublicKey(p * q, 2048, hs=hs)
old_x = R.up([3, 5, 7, 9], 64)
L.pgpu_shutdown()                      # the pool the key and the batch were created under is gone
pa.initialize()
new_key = pa.PublicKey(p * q, 2048, hs=hs)
new_x = R.up([3, 5, 7, 9], 64)
out = ctypes.c_void_p()
ok = True
for key, x in ((old_key, new_x), (new_key, old_x), (old_key, old_x)):
    rc = L.pgpu_batch_ct_pack(key._h, x, 2, 3, ctypes.byref(out))
    print("rc", rc, L.pgpu_last_error().decode())
    ok = ok and rc == -1 and b"shut down" in L.pgpu_last_error() and not out.value
rc = L.pgpu_batch_ct_pack(new_key._h, new_x, 2, 3, ctypes.byref(out))
ok = ok and rc == 0 and bool(out.value)
if out.value:
    got = R.down(out)
    L.pgpu_batch_destroy(out)
    ok = ok and got == [3 * 5 ** 8 % nsq, 7 * 9 ** 8 % nsq]
    print("pack", got)
L.pgpu_batch_destroy(new_x)
sys.exit(0 if ok else 1)
"""


def test_stale_handles_are_refused(engine):
    """a key or a batch created under a device pool that has been shut down: PGPU_ERR_INVALID_PARAM, *out untouched (own
    process: the pool of the test session stays up)"""
    r = subprocess.run([sys.executable, "-c", _STALE, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


@pytest.mark.parametrize("switch", ["PGPU_PAIR_ROWS", "PGPU_HENSEL"])
def test_refused_without_pair_rows(engine, switch):
    """PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 keep resident ciphertexts as Montgomery-form words: no pair form,
    PGPU_ERR_UNSUPPORTED (own process: the switches are read once)"""
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, "-c", _NO_PAIR_ROWS, ROOT], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def test_python_pack(engine):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(5)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    m = [rng.randrange(1 << 40) for _ in range(12)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    packed = pk.pack(ct, 4, 48)
    assert len(packed) == 3
    assert engine.unpack_slots(sk.decrypt(packed), 4, 48) == m
    assert engine.unpack_slots(sk.decrypt(pk.pack(ct, 12, 40)), 12, 40, width_bits=2047) == m
    assert pk.pack(ct, 1, 7) == ct
    for seg_len, b in ((5, 8), (0, 8), (4, 0), (4, 512)):                     # 12 % 5, no slots, no bits, 2048 bits
        with pytest.raises(RuntimeError):
            pk.pack(ct, seg_len, b)
    with pytest.raises(RuntimeError):
        pk.pack([], 1, 8)
