"""Generates tests/golden/aggregate_refusals.json: the return code and the full text of pgpu_last_error() of every refusal
the six aggregation calls on resident ciphertexts share (pgpu_batch_ct_matvec / _spmv / _weighted_sum / _segment_sum /
_segment_scan / _pack), plus one parameter refusal of each call's own, under a 1024- and a 2048-bit key.  Recorded results
only; needs a GPU.  Recorded at the commit BEFORE the six host drivers were folded into csrc/capi_aggregate.inc, so that
tests/test_gpu_aggregate_refusals.py -- which drives the same cases through collect() below -- holds the shared driver to
the messages, codes and order of the six separate ones.

Every case violates exactly one condition, so the fixture fixes no order between checks that the code does not intend.
Operands are 2-6 ciphertexts; nothing is exponentiated.  The "other key" of each width is a product of two seeded primes
(gen_primes.py), kept in the fixture as "other_n".  The cases:
  width       the ciphertext batch is one word wider than 2 * words(n)
  mont_other  a word batch in the Montgomery domain of another key (made with the split forms switched off)
  pair_other  a pair-row batch of another key of the same class
  masked      the masked table-gather policy switched on
  no_pair     a 4096-bit key, which has no pair form (recorded once per call, under "4096")
  own         matvec: e_bits 0; spmv: a column index not below count(x); weighted sum: w_words 0 with weights; segment
              sum: an id not below n_segments (checked AFTER the shared refusals: the sort finds it); segment scan: an
              unknown flag bit; pack: seg_len * slot_bits beyond bitlen(n) - 1
usage: python tests/golden/gen_aggregate_refusals.py [out.json]     (from the root of the tree whose library is recorded)"""
import ctypes
import json
import os
import sys

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
OPS = ("matvec", "spmv", "weighted_sum", "segment_sum", "segment_scan", "pack")
CASES = ("width", "mont_other", "pair_other", "masked", "own")


def modulus(bits):
    if bits == 2048:
        k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    elif bits == 4096:
        k = json.load(open(os.path.join(GOLD, "primes_4096.json")))
    else:
        k = [c for c in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"] if c["bits"] == bits][0]
    return int(k["p"], 16) * int(k["q"], 16)


def collect(pa, bits, other_n):
    """{op: {case: {"rc", "error", "out_null", "launches"}}} for the key of `bits`; other_n: another modulus of that width"""
    from pailliercryptolib_amd import _capi
    from pailliercryptolib_amd.limbs import ints_to_limbs
    L = _capi.lib()
    n = modulus(bits)
    W = 2 * ((n.bit_length() + 63) // 64)
    key, other, key4 = pa.PublicKey(n, bits), pa.PublicKey(other_n, bits), pa.PublicKey(modulus(4096), 4096)
    live, keep = [], []

    def ptr(a):
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)

    def up(vals, words):
        h = ctypes.c_void_p()
        _capi.check(L.pgpu_batch_upload(ptr(ints_to_limbs(vals, words)), len(vals), words, words, ctypes.byref(h)))
        live.append(h)
        return h

    def add(k):     # a product of two uploaded batches under key k: a resident batch in that key's own domain
        h = ctypes.c_void_p()
        _capi.check(L.pgpu_batch_ct_add(k._h, up([3, 5, 7, 9], W), up([2, 4, 6, 8], W), ctypes.byref(h)))
        live.append(h)
        return h

    good, good2 = up([3, 5, 7, 9], W), up([11, 13, 17, 19], W)
    x = {"width": up([3, 5, 7, 9], W + 1), "pair_other": add(other), "masked": good, "own": good,
         "no_pair": up([3, 5, 7, 9], 128)}
    L.pgpu_debug_set_hensel(0)
    try:
        x["mont_other"] = add(other)
    finally:
        L.pgpu_debug_set_hensel(1)
    assert L.pgpu_batch_row_limbs(x["mont_other"]) == 0 and L.pgpu_batch_is_montgomery(x["mont_other"]) == 1
    assert L.pgpu_batch_row_limbs(x["pair_other"]) > 0 and L.pgpu_batch_row_limbs(good) == 0
    w8, w3 = up([1, 2, 3, 4, 5, 6, 7, 5], 1), up([1, 2, 3], 1)
    row_ptr = np.array([0, 2, 3], dtype=np.uint64)
    weights = ints_to_limbs([3, 5], 1)

    def call(op, k, xb, case, out):
        o, own = ctypes.byref(out), case == "own"
        if op == "matvec":
            return L.pgpu_batch_ct_matvec(k, xb, w8, 2, 0 if own else 3, o)
        if op == "spmv":
            cols = np.array([0, 4 if own else 3, 1], dtype=np.uint32)
            return L.pgpu_batch_ct_spmv(k, xb, ptr(row_ptr), ptr(cols), w3, 2, 3, o)
        if op == "weighted_sum":
            arr = (ctypes.c_void_p * 2)(xb.value if case == "no_pair" else good2.value, xb.value)
            return L.pgpu_batch_ct_weighted_sum(k, arr, 2, ptr(weights), 0 if own else 1, o)
        if op == "segment_sum":
            ids = np.array([0, 1, 2 if own else 0, 1], dtype=np.uint32)
            return L.pgpu_batch_ct_segment_sum(k, xb, ptr(ids), 1, 2, o)
        if op == "segment_scan":
            return L.pgpu_batch_ct_segment_scan(k, xb, 2, 2 if own else 0, o)
        return L.pgpu_batch_ct_pack(k, xb, 2, n.bit_length() if own else 8, o)

    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    res = {}
    assert L.pgpu_set_timing(1) == 0
    try:
        for op in OPS:
            res[op] = {}
            for case in CASES + ("no_pair",):
                assert L.pgpu_synchronize() == 0
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                       # drop what the set-up left
                out = ctypes.c_void_p()
                if case == "masked":
                    assert L.pgpu_set_table_gather_policy(1) == 0
                try:
                    rc = call(op, key4._h if case == "no_pair" else key._h, x[case], case, out)
                    err = L.pgpu_last_error().decode()
                finally:
                    if case == "masked":
                        L.pgpu_set_table_gather_policy(0)
                assert L.pgpu_synchronize() == 0
                res[op][case] = {"rc": rc, "error": err, "out_null": not out.value,
                                 "launches": L.pgpu_timing_collect_ex(kinds, forms, ms, 64)}
                if out.value:
                    live.append(out)
    finally:
        L.pgpu_set_timing(0)
        for h in live:
            L.pgpu_batch_destroy(h)
    return res


def main():
    sys.path.insert(0, os.getcwd())
    import pailliercryptolib_amd as pa
    pa.initialize()
    import random
    import gen_primes
    fixture = {"generator": "tests/golden/gen_aggregate_refusals.py", "4096": {}, "other_n": {}}
    for bits in (1024, 2048):
        rng = random.Random(bits + 1)
        other_n = gen_primes.prime(bits // 2, rng) * gen_primes.prime(bits // 2, rng)
        assert other_n.bit_length() == bits and other_n != modulus(bits)
        fixture["other_n"][str(bits)] = hex(other_n)
        res = collect(pa, bits, other_n)
        for op in OPS:
            for case, r in res[op].items():
                assert r["rc"] != 0 and r["out_null"] and r["launches"] == 0, (bits, op, case, r)
                rec = [r["rc"], r["error"]]
                if case == "no_pair":
                    assert fixture["4096"].setdefault(op, rec) == rec
                else:
                    fixture.setdefault(str(bits), {}).setdefault(op, {})[case] = rec
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "aggregate_refusals.json")
    json.dump(fixture, open(out, "w"), indent=1, sort_keys=True)
    print("wrote", out)
    pa.terminate()


if __name__ == "__main__":
    main()
