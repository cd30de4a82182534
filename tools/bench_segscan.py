"""Encrypted segmented prefix sum: the fused call against its yardsticks, on the same key and the same resident inputs, in
the same process (tools/, a measurement; bench.py is the headline).  2048-bit key.

  fused     pgpu_batch_ct_segment_scan(x, seg_len, flags)
  ideal     ONE pgpu_batch_ct_add launch over as many elements as the call has products (pgpu_ct_segment_scan_plan):
            every product useful, rows read in order, one row stored per product -- measured on 2^20 elements and scaled
  matvec    what a caller could do before: one pgpu_batch_ct_matvec per row with the lower-triangular 0/1 matrix and
            e_bits = 1 (case c only)

Cases: (a) 32768 rows x 32 bins (one chain per row); (b) 1 row x 2^20 (multi-level); (c) 512 rows x 32 (small,
latency-bound); (d) 64 rows x 4096.  Per case: HIP-event kernel time (pgpu_set_timing: the sum over the launches, and
every launch: up-sweeps first, then the scans from the deepest level up) and wall time (host clock around the call, which
includes the host's plan, ending in pgpu_synchronize), the plan (chunk, levels, products) and the product rate as a
fraction of the ideal.  One warm-up, then --reps timed runs; the median is reported and all runs printed.  --sweep repeats
the cases with PGPU_SEGSCAN_CHUNK forced to each of 2 .. 512 (on (a) that switches the single-level rule off below 32);
every sweep result is compared bit for bit with the default plan's.

usage: python tools/bench_segscan.py [--reps 5] [--sweep] [--cases a,b,c,d] [--quick] [--reverse] [--out profiles/segscan_bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi
from bench_segsum import Box, random_rows

GOLD = os.path.join(ROOT, "tests", "golden")
KIND_SEGSCAN, KIND_MATVEC = 7, 5
BITS = 2048
SWEEP = [2, 4, 8, 16, 32, 64, 128, 256, 512]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="repeat cases a, b, d with every forced chunk of %s" % SWEEP)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--reverse", action="store_true", help="suffix instead of prefix products")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segscan_bench.txt"))
    args = ap.parse_args()
    os.environ.pop("PGPU_SEGSCAN_CHUNK", None)
    flags = _capi.SCAN_REVERSE if args.reverse else 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B = Box()
    L = B.L
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    p, q, hs = int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
    pk = pa.PublicKey(p * q, BITS, hs=hs)
    nw = BITS // 64
    rng = np.random.default_rng(2048)
    zero = B.up(np.zeros((1, 1), dtype=np.uint64))

    def resident(count):
        t = B.up(random_rows(rng, count, nw))
        h = B.op(L.pgpu_batch_ct_add_plain, pk._h, t, zero)      # uploaded words -> pair rows
        B.free(t)
        return h

    big_n = 1 << (12 if args.quick else 20)
    big = resident(big_n)
    say("# box: %s | key %d bits | reps %d | %s | times: median, ms"
        % (L.pgpu_device_name().decode(), BITS, args.reps, "reverse" if args.reverse else "forward"))
    _, ideal = B.measure(lambda: B.op(L.pgpu_batch_ct_add, pk._h, big, big), args.reps, None)
    ideal_per_product = ideal["kernel_ms"] / big_n
    say("ideal: pgpu_batch_ct_add of %d elements: kernel %.3f ms %s = %.3f ns per product"
        % (big_n, ideal["kernel_ms"], ideal["kernel_ms_all"], ideal_per_product * 1e6))
    shapes = {"a": (32768, 32), "b": (1, big_n), "c": (512, 32), "d": (64, 4096)}
    if args.quick:
        shapes = {"a": (128, 32), "b": (1, big_n), "c": (16, 32), "d": (4, 1024)}
    xs = {big_n: big}
    ok = True
    for case in args.cases.split(","):
        rows, seg_len = shapes[case]
        count = rows * seg_len
        if count not in xs:
            xs[count] = resident(count)
        x = xs[count]

        def fused():
            return B.op(L.pgpu_batch_ct_segment_scan, pk._h, x, seg_len, flags)

        def run_fused(forced=None):
            if forced is None:
                os.environ.pop("PGPU_SEGSCAN_CHUNK", None)
            else:
                os.environ["PGPU_SEGSCAN_CHUNK"] = str(forced)
            chunk, levels, products = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
            _capi.check(L.pgpu_ct_segment_scan_plan(BITS, rows, seg_len, ctypes.byref(chunk), ctypes.byref(levels), ctypes.byref(products)))
            out, t = B.measure(fused, args.reps, KIND_SEGSCAN)
            os.environ.pop("PGPU_SEGSCAN_CHUNK", None)
            assert len(t["launch_ms"]) == 2 * levels.value - 1, (levels.value, t["launch_ms"])
            nl = levels.value
            t.update({"chunk": chunk.value, "levels": nl, "products": products.value,
                      "up_ms": t["launch_ms"][:nl - 1], "scan_ms_deepest_first": t["launch_ms"][nl - 1:],
                      "frac_of_ideal": round(products.value * ideal_per_product / t["kernel_ms"], 3)})
            return out, t

        out, t = run_fused()
        o = {"case": case, "rows": rows, "seg_len": seg_len, "fused": t}
        say("(%s) %d rows x %d | chunk %d, levels %d, products %d (%.3f x count) | fused kernel %.3f ms %s (up-sweeps %s; scans, "
            "deepest first %s) wall %.3f | %.3f of the ideal over as many products"
            % (case, rows, seg_len, t["chunk"], t["levels"], t["products"], t["products"] / count, t["kernel_ms"], t["kernel_ms_all"],
               t["up_ms"], t["scan_ms_deepest_first"], t["wall_ms"], t["frac_of_ideal"]))
        if case == "c":
            # the route a caller had: one matvec per row, rows taken as batches of their own
            tri = np.triu if args.reverse else np.tril
            w = B.up(tri(np.ones((seg_len, seg_len), dtype=np.uint64)).reshape(-1, 1))
            xw = B.down(x)
            row_h = [B.up(xw[r * seg_len:(r + 1) * seg_len]) for r in range(rows)]
            row_p = [B.op(L.pgpu_batch_ct_add_plain, pk._h, h, zero) for h in row_h]
            B.free(*row_h)

            def route():
                return [B.op(L.pgpu_batch_ct_matvec, pk._h, h, w, seg_len, 1) for h in row_p]

            def timed_route():
                B.sync()
                L.pgpu_set_timing(1)
                t0 = time.perf_counter()
                hs_ = route()
                B.sync()
                wall = (time.perf_counter() - t0) * 1e3
                cap = 1 << 14
                kinds, ms = (ctypes.c_int * cap)(), (ctypes.c_double * cap)()
                n = L.pgpu_timing_collect(kinds, ms, cap)
                L.pgpu_set_timing(0)
                assert all(kinds[i] == KIND_MATVEC for i in range(n))
                return wall, sum(ms[i] for i in range(n)), n, hs_
            _, _, _, hs_ = timed_route()
            same = all(np.array_equal(B.down(hs_[r]), out[r * seg_len:(r + 1) * seg_len]) for r in (0, rows // 2, rows - 1))
            ok = ok and same
            B.free(*hs_)
            walls, kerns = [], []
            for _ in range(args.reps):
                wall, kern, n_launch, hs_ = timed_route()
                B.free(*hs_)
                walls.append(wall)
                kerns.append(kern)
            B.free(w, *row_p)
            mv = {"wall_ms": statistics.median(walls), "kernel_ms": statistics.median(kerns), "launches": n_launch,
                  "kernel_ms_all": [round(v, 3) for v in kerns]}
            o["matvec"] = mv
            o["identical"] = same
            say("    matvec route (%d calls, lower-triangular 0/1 matrix, e_bits 1): kernel %.3f ms %s in %d launches, wall %.3f | "
                "fused is %.1f x faster (kernel), %.1f x (wall) | rows 0, %d, %d %s"
                % (rows, mv["kernel_ms"], mv["kernel_ms_all"], n_launch, mv["wall_ms"], mv["kernel_ms"] / t["kernel_ms"],
                   mv["wall_ms"] / t["wall_ms"], rows // 2, rows - 1, "identical" if same else "DIFFERENT"))
        if args.sweep and case != "c":
            o["sweep"] = []
            for c in SWEEP:
                so, st = run_fused(c)
                same = bool(np.array_equal(out, so))
                ok = ok and same
                o["sweep"].append(st)
                say("    chunk %3d: levels %d, products %d, kernel %.3f ms %s (up %s; scans %s), wall %.3f, %.3f of the ideal%s"
                    % (c, st["levels"], st["products"], st["kernel_ms"], st["kernel_ms_all"], st["up_ms"], st["scan_ms_deepest_first"],
                       st["wall_ms"], st["frac_of_ideal"], "" if same else "  DIFFERENT"))
        say("JSON " + json.dumps(o))
    pa.terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
