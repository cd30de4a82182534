"""Encrypted slot packing: the pack launch against its yardsticks, on the same key and the same resident inputs, in the
same process (tools/, a measurement; bench.py is the headline).  2048-bit key, one GPU, HIP-event kernel time from the
timing record (pgpu_set_timing) and wall time (host clock around the call, ending in pgpu_synchronize).

  pack      pgpu_batch_ct_pack(x, seg_len, slot_bits): rows chains of (seg_len - 1) * (slot_bits + 1) pair products, in the
            form the policy picks and with either form forced (PGPU_PACK_WIDE=0: (4,18), =1: (8,9))
  ct_mul    the yardstick for the kernel, existing code: ONE pgpu_batch_ct_mul launch over `rows` resident elements with the
            single shared exponent 2^((seg_len - 1) * slot_bits) -- the same squarings plus its table build and its
            window products
  decrypt   the yardstick for the feature: pgpu_batch_decrypt_crt of all rows * seg_len ciphertexts, against pack plus
            pgpu_batch_decrypt_crt of the rows packed ones

Cases (rows, seg_len, slot_bits): 31 slots of 64 bits at 64, 2048 and 32768 rows, 16 slots of 32 bits at 32768 rows; with
--cases e,f also 31 x 64 at 8192 and 16384 rows, either side of the switch between the two forms of the key.  (32
slots of 64 bits are 2048 bits: more than the plaintext of a 2048-bit key holds, the call refuses them.)  Per case one
warm-up run, then --reps timed runs of every leg, the legs alternating; the median is reported and all runs printed.
Row 0 of every pack result is compared with Python integers.

usage: python tools/bench_pack.py [--reps 5] [--cases a,b,c,d,e,f] [--quick] [--out profiles/pack_bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi
from pailliercryptolib_amd.limbs import limbs_to_ints
from bench_segsum import Box, random_rows

GOLD = os.path.join(ROOT, "tests", "golden")
KIND_PACK = 8
BITS = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    os.environ.pop("PGPU_PACK_WIDE", None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_bench.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B = Box()
    L = B.L
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    p, q, hs = int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
    nsq = (p * q) ** 2
    pk, sk = pa.PublicKey(p * q, BITS, hs=hs), pa.PrivateKey(p, q)
    nw = BITS // 64
    rng = np.random.default_rng(2048)
    zero = B.up(np.zeros((1, 1), dtype=np.uint64))

    def resident(count, head=0):
        a = random_rows(rng, count, nw)
        t = B.up(a)
        h = B.op(L.pgpu_batch_ct_add_plain, pk._h, t, zero)      # uploaded words -> pair rows
        B.free(t)
        return (h, limbs_to_ints(a[:head])) if head else h

    shapes = {"a": (64, 31, 64), "b": (2048, 31, 64), "c": (32768, 31, 64), "d": (32768, 16, 32),
              "e": (8192, 31, 64), "f": (16384, 31, 64)}         # e, f: either side of the switch between the two forms
    if args.quick:
        shapes = {"a": (4, 31, 64), "b": (64, 31, 64), "c": (128, 31, 64), "d": (128, 16, 32), "e": (96, 31, 64), "f": (112, 31, 64)}
    say("# box: %s | key %d bits | reps %d | times: median of the runs in brackets, ms" % (L.pgpu_device_name().decode(), BITS, args.reps))
    ok = True
    for case in args.cases.split(","):
        rows, seg_len, b = shapes[case]
        count = rows * seg_len
        x, row0 = resident(count, seg_len)
        first = resident(rows)                                   # the operand of the ct_mul yardstick: `rows` resident elements
        e_bits = (seg_len - 1) * b + 1
        ew = np.zeros((1, (e_bits + 63) // 64), dtype=np.uint64)
        ew[0, (e_bits - 1) // 64] = np.uint64(1) << np.uint64((e_bits - 1) % 64)
        e = B.up(ew)
        lanes, limbs, products = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        _capi.check(L.pgpu_ct_pack_plan(BITS, rows, seg_len, b, ctypes.byref(lanes), ctypes.byref(limbs), ctypes.byref(products)))
        def forced(wide):                                        # the same call with the form forced (2048-bit keys have two)
            def fn():
                os.environ["PGPU_PACK_WIDE"] = str(wide)
                try:
                    return B.op(L.pgpu_batch_ct_pack, pk._h, x, seg_len, b)
                finally:
                    os.environ.pop("PGPU_PACK_WIDE", None)
            return fn

        legs = {
            "pack": (lambda: B.op(L.pgpu_batch_ct_pack, pk._h, x, seg_len, b), KIND_PACK),
            "pack_4_18": (forced(0), KIND_PACK),
            "pack_8_9": (forced(1), KIND_PACK),
            "ct_mul": (lambda: B.op(L.pgpu_batch_ct_mul, pk._h, first, e, e_bits), None),
            "decrypt_all": (lambda: B.op(L.pgpu_batch_decrypt_crt, sk._h, x), None),
        }
        res = {name: {"wall": [], "kern": [], "launches": 0} for name in list(legs) + ["decrypt_packed"]}
        _, _, packed = B.timed(legs["pack"][0])                  # warm-up of every leg; the packed batch feeds the last one
        legs["decrypt_packed"] = (lambda: B.op(L.pgpu_batch_decrypt_crt, sk._h, packed), None)
        got = limbs_to_ints(B.down(packed)[:1])[0]
        want = 1
        for t, v in enumerate(row0):
            want = want * pow(v, 1 << (b * t), nsq) % nsq
        same = got == want
        ok = ok and same
        for name in ("pack_4_18", "pack_8_9"):
            h = B.timed(legs[name][0])[2]
            same = same and limbs_to_ints(B.down(h)[:1])[0] == want
            B.free(h)
        ok = ok and same
        for name in ("ct_mul", "decrypt_all", "decrypt_packed"):
            B.free(B.timed(legs[name][0])[2])
        for _ in range(args.reps):                               # the legs alternate
            for name, (fn, kind) in legs.items():
                wall, rec, h = B.timed(fn)
                B.free(h)
                assert kind is None or (len(rec) == 1 and rec[0][0] == kind), rec
                res[name]["wall"].append(wall)
                res[name]["kern"].append(sum(ms for _, ms in rec))
                res[name]["launches"] = len(rec)
        B.free(packed, x, first, e)
        o = {"case": case, "rows": rows, "seg_len": seg_len, "slot_bits": b, "form": [lanes.value, limbs.value],
             "products": products.value, "row0_exact": same}
        for name, r in res.items():
            o[name] = {"kernel_ms": statistics.median(r["kern"]), "kernel_ms_all": [round(v, 3) for v in r["kern"]],
                       "wall_ms": statistics.median(r["wall"]), "launches": r["launches"]}
        pk_ms, mul_ms = o["pack"]["kernel_ms"], o["ct_mul"]["kernel_ms"]
        all_ms, few_ms = o["decrypt_all"]["kernel_ms"], o["decrypt_packed"]["kernel_ms"]
        say("(%s) %d rows x %d slots of %d bits | form (%d,%d), %d products | row 0 %s"
            % (case, rows, seg_len, b, lanes.value, limbs.value, products.value, "exact" if same else "DIFFERENT"))
        say("    pack    kernel %.3f ms %s wall %.3f | %.3f G products/s"
            % (pk_ms, o["pack"]["kernel_ms_all"], o["pack"]["wall_ms"], products.value / pk_ms / 1e6))
        say("    forced forms: (4,18) kernel %.3f ms %s | (8,9) kernel %.3f ms %s | (8,9) / (4,18) = %.3f"
            % (o["pack_4_18"]["kernel_ms"], o["pack_4_18"]["kernel_ms_all"], o["pack_8_9"]["kernel_ms"], o["pack_8_9"]["kernel_ms_all"],
               o["pack_8_9"]["kernel_ms"] / o["pack_4_18"]["kernel_ms"]))
        say("    ct_mul  of %d elements by 2^%d: kernel %.3f ms %s in %d launches, wall %.3f | pack / ct_mul = %.3f"
            % (rows, e_bits - 1, mul_ms, o["ct_mul"]["kernel_ms_all"], o["ct_mul"]["launches"], o["ct_mul"]["wall_ms"], pk_ms / mul_ms))
        say("    decrypt of all %d: kernel %.3f ms %s wall %.3f | pack + decrypt of %d: kernel %.3f + %.3f = %.3f ms %s wall %.3f + %.3f"
            " | %.2f x in kernel time, 1/%d of the bytes downloaded"
            % (count, all_ms, o["decrypt_all"]["kernel_ms_all"], o["decrypt_all"]["wall_ms"], rows, pk_ms, few_ms, pk_ms + few_ms,
               o["decrypt_packed"]["kernel_ms_all"], o["pack"]["wall_ms"], o["decrypt_packed"]["wall_ms"], all_ms / (pk_ms + few_ms), seg_len))
        say("JSON " + json.dumps(o))
    pa.terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
