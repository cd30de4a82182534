"""Ciphertext negation and subtraction: the two calls against their yardsticks, on the same key and the same resident
inputs, in the same process (tools/, a measurement; bench.py is the headline).  2048-bit key.

  negate    pgpu_batch_ct_negate(x)                     3 (count - 1) pair products, one host inversion
  sub       pgpu_batch_ct_sub(a, b)                     count more, multiplied in by the last walk
  (a)       ONE pgpu_batch_ct_add launch over the same count, times three (sub: times four): the ideal by product count --
            every product useful, rows read in order, one row stored per product
  (b)       pgpu_batch_ct_mul by the one-element exponent n - 1: the only route to Enc(-m) before these calls

Sizes: 2^20, 65536, 2048 and 64 elements.  Per size: HIP-event kernel time (pgpu_set_timing: the sum over the launches
of kind PGPU_KERNEL_INVERT, every launch listed -- forward passes first, then the walks back from the top level down --
and beside it the two row conversions around the host inversion), wall time (host clock around the call, which includes
the plan and the round trip of one row through the host, ending in pgpu_synchronize), the plan (chunk, levels, launches,
products).  The bar of the project: at 2^20 and 65536 elements negate's kernel time at most twice (a).  One warm-up, then
--reps timed runs; the median is reported and all runs printed.  --sweep repeats negate with PGPU_INVERT_CHUNK forced to
each of %(sweep)s and, at the default chunk, with PGPU_INVERT_WIDE forced both ways; every such result is compared bit for
bit with the default plan's.  Last, two existing calls from the same run, to be read beside the parent commit's figures:
pgpu_batch_ct_segment_scan on 512 rows x 32 (profiles/aggregate_refactor.txt) and the ct_add of 2^20 elements itself
(profiles/segsum_bench.txt).

usage: python tools/bench_negate.py [--reps 5] [--sweep] [--sizes 1048576,65536,2048,64] [--quick] [--out profiles/negate_bench.txt]
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
from pailliercryptolib_amd.limbs import ints_to_limbs
from bench_segsum import Box, random_rows

GOLD = os.path.join(ROOT, "tests", "golden")
KIND_INVERT, KIND_SEGSCAN = 14, 7
BITS = 2048
SWEEP = [2, 3, 4, 8, 16, 32, 64, 128, 256]
__doc__ = __doc__ % {"sweep": SWEEP}


def measure(B, fn, reps, kind):
    """Box.measure with the launches of `kind` summed as the kernel time and everything else (row conversions) beside it"""
    _, _, h = B.timed(fn)                              # warm-up; its result is the one compared
    out = B.down(h)
    B.free(h)
    walls, kerns, others, launches = [], [], [], []
    for _ in range(reps):
        wall, rec, h = B.timed(fn)
        B.free(h)
        walls.append(wall)
        kerns.append(sum(ms for k, ms in rec if kind is None or k == kind))
        others.append(sum(ms for k, ms in rec if kind is not None and k != kind))
        launches.append([round(ms, 3) for k, ms in rec if kind is None or k == kind])
    mid = len(launches) // 2
    return out, {"wall_ms": statistics.median(walls), "kernel_ms": statistics.median(kerns), "other_ms": statistics.median(others),
                 "kernel_ms_all": [round(v, 3) for v in kerns], "wall_ms_all": [round(v, 3) for v in walls], "launch_ms": launches[mid]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="repeat negate with every forced chunk of %s and both forms" % SWEEP)
    ap.add_argument("--sizes", default="1048576,65536,2048,64")
    ap.add_argument("--quick", action="store_true", help="tiny sizes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "negate_bench.txt"))
    args = ap.parse_args()
    for name in ("PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE", "PGPU_SEGSCAN_CHUNK"):
        os.environ.pop(name, None)
    sizes = [4096, 512, 64] if args.quick else [int(v) for v in args.sizes.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B = Box()
    L = B.L
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    p, q, hs = int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
    n = p * q
    pk = pa.PublicKey(n, BITS, hs=hs)
    nw = BITS // 64
    rng = np.random.default_rng(2048)
    zero = B.up(np.zeros((1, 1), dtype=np.uint64))
    n_minus_1 = B.up(ints_to_limbs([n - 1], nw))

    def resident(count):
        t = B.up(random_rows(rng, count, nw))          # (a random residue is a unit modulo n but for a chance of 2^-1000)
        h = B.op(L.pgpu_batch_ct_add_plain, pk._h, t, zero)      # uploaded words -> pair rows
        B.free(t)
        return h

    def plan(count):
        c, lv, la, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        _capi.check(L.pgpu_ct_negate_plan(BITS, count, ctypes.byref(c), ctypes.byref(lv), ctypes.byref(la), ctypes.byref(pr)))
        return c.value, lv.value, la.value, pr.value

    say("# box: %s | key %d bits | reps %d | times: median, ms" % (L.pgpu_device_name().decode(), BITS, args.reps))
    ok = True
    for count in sizes:
        x, a = resident(count), resident(count)

        def run(call, forced=None, wide=None):
            for name, v in (("PGPU_INVERT_CHUNK", forced), ("PGPU_INVERT_WIDE", wide)):
                if v is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = str(v)
            chunk, levels, launches, products = plan(count)
            out, t = measure(B, call, args.reps, KIND_INVERT)
            for name in ("PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE"):
                os.environ.pop(name, None)
            assert len(t["launch_ms"]) == launches, (launches, t["launch_ms"])
            nf = launches - levels
            t.update({"chunk": chunk, "levels": levels, "launches": launches, "products": products,
                      "forward_ms": t["launch_ms"][:nf], "walk_ms_top_first": t["launch_ms"][nf:]})
            return out, t

        _, add = measure(B, lambda: B.op(L.pgpu_batch_ct_add, pk._h, x, a), args.reps, None)
        neg_out, neg = run(lambda: B.op(L.pgpu_batch_ct_negate, pk._h, x))
        _, sub = run(lambda: B.op(L.pgpu_batch_ct_sub, pk._h, a, x))
        mul_reps = args.reps if count <= 65536 else min(args.reps, 2)
        _, mul = measure(B, lambda: B.op(L.pgpu_batch_ct_mul, pk._h, x, n_minus_1, BITS), mul_reps, None)   # (about 2400 products per element)
        o = {"count": count, "ct_add": add, "negate": neg, "sub": sub, "ct_mul_n_minus_1": mul}
        say("%d elements | chunk %d, levels %d, launches %d, products %d" % (count, neg["chunk"], neg["levels"], neg["launches"], neg["products"]))
        say("    (a) ct_add x 1: kernel %.3f ms %s, wall %.3f" % (add["kernel_ms"], add["kernel_ms_all"], add["wall_ms"]))
        for name, t, factor in (("negate", neg, 3), ("sub   ", sub, 4)):
            say("    %s: kernel %.3f ms %s (forward %s; walks back, top first %s) + row conversions %.3f | wall %.3f %s, host round trip "
                "and plan %.3f | %.2f x (a) x %d"
                % (name, t["kernel_ms"], t["kernel_ms_all"], t["forward_ms"], t["walk_ms_top_first"], t["other_ms"], t["wall_ms"],
                   t["wall_ms_all"], t["wall_ms"] - t["kernel_ms"] - t["other_ms"], t["kernel_ms"] / (factor * add["kernel_ms"]), factor))
        say("    (b) ct_mul by n - 1: kernel %.3f ms %s, wall %.3f | negate is %.0f x faster (kernel), %.0f x (wall)"
            % (mul["kernel_ms"], mul["kernel_ms_all"], mul["wall_ms"], mul["kernel_ms"] / neg["kernel_ms"], mul["wall_ms"] / neg["wall_ms"]))
        if args.sweep:
            o["sweep"] = []
            variants = [(c, None) for c in SWEEP] + [(None, 0), (None, 1)]
            for forced, wide in variants:
                so, st = run(lambda: B.op(L.pgpu_batch_ct_negate, pk._h, x), forced, wide)
                same = bool(np.array_equal(neg_out, so))
                ok = ok and same
                st["forced_chunk"], st["forced_wide"] = forced, wide
                o["sweep"].append(st)
                say("    %s: levels %d, launches %d, kernel %.3f ms %s (forward %s; walks %s), wall %.3f%s"
                    % ("chunk %3d" % forced if forced else "wide %d   " % wide, st["levels"], st["launches"], st["kernel_ms"],
                       st["kernel_ms_all"], st["forward_ms"], st["walk_ms_top_first"], st["wall_ms"], "" if same else "  DIFFERENT"))
        say("JSON " + json.dumps(o))
        B.free(x, a)
    # two existing calls, unchanged by this addition: to be read beside the parent commit's figures
    rows, seg_len = (16, 32) if args.quick else (512, 32)
    xs = resident(rows * seg_len)
    _, sc = measure(B, lambda: B.op(L.pgpu_batch_ct_segment_scan, pk._h, xs, seg_len, 0), args.reps, KIND_SEGSCAN)
    say("existing: pgpu_batch_ct_segment_scan %d rows x %d: kernel %.3f ms %s, wall %.3f" % (rows, seg_len, sc["kernel_ms"], sc["kernel_ms_all"], sc["wall_ms"]))
    big_n = 1 << (12 if args.quick else 20)
    big = resident(big_n)
    _, ad = measure(B, lambda: B.op(L.pgpu_batch_ct_add, pk._h, big, big), args.reps, None)
    say("existing: pgpu_batch_ct_add of %d elements: kernel %.3f ms %s = %.3f ns per product" % (big_n, ad["kernel_ms"], ad["kernel_ms_all"], ad["kernel_ms"] / big_n * 1e6))
    pa.terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
