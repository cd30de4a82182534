"""The one-lane CRT decrypt with 5-bit and with 6-bit windows on the half-squared window table (csrc/hensel_ps.hpp,
csrc/hensel_ps_bal.hpp: entry 2k = (entry k)^2, entry 2k+1 = entry 2k (x) base; the balanced form squares on a doubled operand)
against oracle/paillier_oracle, every plaintext, and against each other, bit for bit: the two half-width exponentiations of
PrivateKey::decryptCRT, ipcl/pri_key.cpp:114-157.  The one-lane form is forced (pgpu_debug_set_ps_decrypt(2)), the window by
pgpu_debug_set_fixed_window (what PGPU_FIXED_WINDOW does for a whole process); indexed and masked table access (the masked
policy keeps its 3-bit windows whatever is forced), the balanced and the unsigned kernel.  Counts 1, 63, 64, 65 and 129: a lone
element, a wavefront short of one lane, a full one, the clamped tail lanes of a second wavefront pair, and a third pair, which
is a second workgroup.  Keys: ISO 2048 bits (1024-bit exponents: 4 bits in the top window at w = 6), the uneven 2037-bit key
(primes of 1013 and 1024 bits) and the 2051-bit key.  The arithmetic is modelled in tests/test_ps_window6_model.py."""
import ctypes
import functools
import random

import pytest

from test_gpu_key_widths import KEYS, _q3
from test_gpu_round4 import Res, key_case

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65, 129)
NAMES = ("iso", 2037, 2051)


def _pq(name):
    return key_case(2048)[:2] if name == "iso" else KEYS[name]


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """(ciphertexts, the oracle's plaintexts) for the largest count, computed once per key: every count takes a prefix"""
    from oracle import paillier_oracle as orc
    p, q = _pq(name)
    n = p * q
    rng = random.Random(str(name))
    raw = [n * n - 1, 1, n + 1] + [rng.randrange(1, n * n) for _ in range(max(COUNTS) - 3)]
    return raw, orc.PrivateKey(n, p, q).decrypt(raw)


def _restore(L, window):
    from pailliercryptolib_amd import _capi
    L.pgpu_debug_set_fixed_window(window)
    L.pgpu_debug_set_ps_decrypt(1)
    L.pgpu_debug_set_ps_balanced(1)
    _capi.check(L.pgpu_set_table_gather_policy(0))


def test_window_policy_of_the_one_lane_forms(engine):
    """the weighted count picks 6 bits for 1024-bit exponents in the one-lane forms only; a forced width holds for every form"""
    L = Res().L
    L.pgpu_debug_decrypt_window.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int]
    entry = 2 * 8192 * 2 * 36 * 4                       # one table entry of every exponentiation of the headline's launch
    was = L.pgpu_debug_set_fixed_window(0)
    try:
        assert L.pgpu_debug_decrypt_window(1024, entry, 1) == 6 and L.pgpu_debug_decrypt_window(1024, entry, 0) == 5
        assert L.pgpu_debug_decrypt_window(512, entry, 1) == 5 and L.pgpu_debug_decrypt_window(1536, entry, 1) == 6
        assert L.pgpu_debug_decrypt_window(1024, (4 << 30) // 64 + 1, 1) == 5          # the table cap of 4 GiB
        for w in (5, 6, 3):
            assert L.pgpu_debug_set_fixed_window(w) in (0, 5, 6)
            assert L.pgpu_debug_decrypt_window(1024, entry, 1) == w == L.pgpu_debug_decrypt_window(1024, entry, 0)
    finally:
        L.pgpu_debug_set_fixed_window(was)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", NAMES)
def test_windows_5_and_6_both_forms_both_table_policies(engine, name, count):
    from pailliercryptolib_amd import _capi
    p, q = _pq(name)
    n = p * q
    nw = (n.bit_length() + 63) // 64
    raw, want = (v[:count] for v in _vectors(name))
    sk = engine.PrivateKey(p, q)
    R = Res()
    L = R.L
    was = L.pgpu_debug_set_fixed_window(0)
    try:
        up = R.up(raw, 2 * nw)
        L.pgpu_debug_set_ps_decrypt(2)
        got = {}
        for gather in (0, 1):
            _capi.check(L.pgpu_set_table_gather_policy(gather))
            for bal in (1, 0):
                L.pgpu_debug_set_ps_balanced(bal)
                for w in (5, 6):
                    L.pgpu_debug_set_fixed_window(w)
                    assert _q3(L.pgpu_decrypt_kernel_form_ex, sk._h, count, 0) == (4, 1, 36 if bal else 38)
                    got[gather, bal, w] = R.down(R.op(L.pgpu_batch_decrypt_crt, sk._h, up))
        for key, g in got.items():
            assert g == want, key                                            # every result against the oracle
        assert all(got[g, b, 5] == got[g, b, 6] for g in (0, 1) for b in (0, 1))
    finally:
        _restore(L, was)
        R.close()
