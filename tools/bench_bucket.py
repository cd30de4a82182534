"""Bucket-method encrypted matvec against the window-table matvec, on the same key and the same resident x, in the same
process (tools/, a measurement; bench.py is the headline).

  bucket     pgpu_batch_ct_matvec_bucket(x, w on the host)       the new call
  matvec     pgpu_batch_ct_matvec(x, w as an uploaded batch)     existing, unchanged code: the baseline

Shapes (2048-bit key), rows x cols x e_bits:
  (a) 1 x 2^20 x 32          an encrypted SUM(v * x) over a million-row column
  (b) 16 x 65536 x 32
  (c) 1 x 65536 x 32
  (d) 1 x 1024 x 32          where the matvec may well win: reported either way
  (e) 1 x 65536 x 2048       full-width weights (signed weights as w mod n)

The results of both calls are downloaded and compared bit for bit.  Per call: HIP-event kernel time (pgpu_set_timing:
the sum over the launches) and wall time (host clock around the call, ending in pgpu_synchronize), medians of --reps
runs after one warm-up; the product counts of both plan queries; for the bucket call its launches one by one and the
share of wall time that is not kernel time (the host's digit cut and sort, the plan image and its upload).  The bar:
at (a), (b) and (e) the kernel-time speed-up is at least half the ratio of the two product counts.
--sweep forces PGPU_BUCKET_WINDOW over 4..10 (and PGPU_BUCKET_BLOCK at the plan's window) on (a) and (b).

usage: python tools/bench_bucket.py [--reps 5] [--cases abcde] [--sweep] [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
KIND_BUCKET, KIND_MATVEC = 12, 5
BITS = 2048
CASES = {"a": (1, 1 << 20, 32), "b": (16, 65536, 32), "c": (1, 65536, 32), "d": (1, 1024, 32), "e": (1, 65536, 2048)}
QUICK = {"a": (1, 3000, 32), "b": (3, 500, 32), "c": (1, 700, 32), "d": (1, 64, 32), "e": (1, 200, 2048)}
BAR = "abe"
KNOBS = ("PGPU_BUCKET_WINDOW", "PGPU_BUCKET_BLOCK")


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Box:
    def __init__(self):
        pa.initialize(0)
        self.L = _capi.lib()

    def up(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        h = ctypes.c_void_p()
        _capi.check(self.L.pgpu_batch_upload(ptr(arr), arr.shape[0], arr.shape[1], arr.shape[1], ctypes.byref(h)))
        return h

    def op(self, fn, *a):
        h = ctypes.c_void_p()
        _capi.check(fn(*a, ctypes.byref(h)))
        return h

    def down(self, h):
        out = np.empty((self.L.pgpu_batch_count(h), self.L.pgpu_batch_words(h)), dtype=np.uint64)
        _capi.check(self.L.pgpu_batch_download(h, ptr(out)))
        return out

    def free(self, *hs):
        for h in hs:
            self.L.pgpu_batch_destroy(h)

    def sync(self):
        _capi.check(self.L.pgpu_synchronize())

    def timed(self, fn):
        """-> (wall ms, [(kind, ms)] of the launches, result handle)"""
        L = self.L
        self.sync()
        L.pgpu_set_timing(1)
        t0 = time.perf_counter()
        h = fn()
        self.sync()
        wall = (time.perf_counter() - t0) * 1e3
        cap = 1 << 12
        kinds, ms = (ctypes.c_int * cap)(), (ctypes.c_double * cap)()
        n = L.pgpu_timing_collect(kinds, ms, cap)
        L.pgpu_set_timing(0)
        return wall, [(kinds[i], ms[i]) for i in range(n)], h

    def measure(self, fn, reps):
        """one warm-up (code objects, arena blocks), whose result is the one compared; then reps timed runs"""
        _, _, h = self.timed(fn)
        out = self.down(h)
        self.free(h)
        walls, kerns, recs = [], [], None
        for _ in range(reps):
            wall, rec, h = self.timed(fn)
            self.free(h)
            walls.append(wall)
            kerns.append(sum(ms for _, ms in rec))
            recs = rec
        return out, {"kernel_ms": round(statistics.median(kerns), 3), "wall_ms": round(statistics.median(walls), 3),
                     "kernel_ms_all": [round(v, 3) for v in kerns], "wall_ms_all": [round(v, 3) for v in walls],
                     "launches": [(k, round(ms, 3)) for k, ms in recs]}


def key_of():
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    return int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)


def bucket_plan(L, rows, cols, e_bits):
    c, b = ctypes.c_int(), ctypes.c_int()
    by, pr, de = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    _capi.check(L.pgpu_ct_matvec_bucket_plan(BITS, rows, cols, e_bits, ctypes.byref(c), ctypes.byref(b), ctypes.byref(by),
                                             ctypes.byref(pr), ctypes.byref(de)))
    return {"window": c.value, "block": b.value, "bucket_bytes": by.value, "products": pr.value, "depth": de.value}


def matvec_plan(L, rows, cols, e_bits):
    w, s, tb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _capi.check(L.pgpu_ct_matvec_plan(BITS, rows, cols, e_bits, ctypes.byref(w), ctypes.byref(s), ctypes.byref(tb)))
    w, s = w.value, s.value
    nwin = -(-e_bits // w)
    products = cols * ((1 << w) - 2) + rows * s * e_bits + rows * cols * nwin + rows * (s - 1)      # policy.hpp: matvec_products
    return {"window": w, "slices": s, "table_bytes": tb.value, "products": products}


def run_case(B, pk, case, reps, quick, sweep):
    L = B.L
    nw = BITS // 64
    rng = np.random.default_rng(ord(case))
    rows, cols, e_bits = (QUICK if quick else CASES)[case]
    ew = (e_bits + 63) // 64
    # x: a resident DJN encrypt of random plaintexts (pair rows)
    bm = B.up(rng.integers(0, 1 << 62, size=(cols, nw), dtype=np.uint64))
    br = B.up(rng.integers(0, 1 << 62, size=(cols, nw // 2), dtype=np.uint64))
    x = B.op(L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2))
    B.free(bm, br)
    if e_bits >= 64:
        w = rng.integers(0, 1 << 63, size=(rows * cols, ew), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(rows * cols, ew), dtype=np.uint64)
        if e_bits % 64:
            w[:, -1] &= np.uint64((1 << (e_bits % 64)) - 1)
    else:
        w = rng.integers(0, 1 << e_bits, size=(rows * cols, 1), dtype=np.uint64)
    wb = B.up(w)

    def bucket():
        return B.op(L.pgpu_batch_ct_matvec_bucket, pk._h, x, ptr(w), ew, rows, e_bits)

    def matvec():
        return B.op(L.pgpu_batch_ct_matvec, pk._h, x, wb, rows, e_bits)

    out = {"case": case, "key_bits": BITS, "rows": rows, "cols": cols, "e_bits": e_bits,
           "bucket_plan": bucket_plan(L, rows, cols, e_bits), "matvec_plan": matvec_plan(L, rows, cols, e_bits)}
    got, out["bucket"] = B.measure(bucket, reps)
    assert all(k == KIND_BUCKET for k, _ in out["bucket"]["launches"])
    ref, out["matvec"] = B.measure(matvec, reps)
    assert all(k == KIND_MATVEC for k, _ in out["matvec"]["launches"])
    identical = bool(np.array_equal(ref, got))
    out["product_ratio"] = round(out["matvec_plan"]["products"] / max(1, out["bucket_plan"]["products"]), 2)
    out["kernel_speedup"] = round(out["matvec"]["kernel_ms"] / out["bucket"]["kernel_ms"], 2)
    out["wall_speedup"] = round(out["matvec"]["wall_ms"] / out["bucket"]["wall_ms"], 2)
    out["host_share_of_wall"] = round(1 - out["bucket"]["kernel_ms"] / out["bucket"]["wall_ms"], 3)
    out["bar"] = (out["kernel_speedup"] >= out["product_ratio"] / 2) if case in BAR else None
    if sweep and (case in "ab" or quick):
        out["sweep"] = []
        c0 = out["bucket_plan"]["window"]
        plans = [(c, None) for c in range(4, 11)] + [(c0, 1 << k) for k in range(0, c0 + 1, 2)]
        for c, b in plans:
            os.environ["PGPU_BUCKET_WINDOW"] = str(c)                            # (read at every call)
            if b is not None:
                os.environ["PGPU_BUCKET_BLOCK"] = str(b)
            try:
                p = bucket_plan(L, rows, cols, e_bits)
                res, r = B.measure(bucket, reps)
            finally:
                for name in KNOBS:
                    os.environ.pop(name, None)
            identical = identical and bool(np.array_equal(ref, res))
            out["sweep"].append({"window": p["window"], "block": p["block"], "products": p["products"], "depth": p["depth"],
                                 "kernel_ms": r["kernel_ms"], "wall_ms": r["wall_ms"], "launches": len(r["launches"]),
                                 "kernel_ms_all": r["kernel_ms_all"]})
    out["identical"] = identical
    B.free(x, wb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--sweep", action="store_true", help="force PGPU_BUCKET_WINDOW / PGPU_BUCKET_BLOCK over a range on cases (a) and (b)")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    for name in KNOBS + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_SEGSUM_CHUNK"):
        os.environ.pop(name, None)
    B = Box()
    p, q, hs = key_of()
    pk = pa.PublicKey(p * q, BITS, hs=hs)
    print("# box:", B.L.pgpu_device_name().decode(), "| key", BITS, "| reps:", args.reps, "| times: median, ms")
    print("# case rows x cols x e_bits | bucket plan c b depth | products matvec / bucket = ratio | kernel ms matvec / bucket = "
          "speed-up | wall ms matvec / bucket = speed-up | host share of the bucket call's wall | bar | identical")
    ok = True
    for case in args.cases:
        o = run_case(B, pk, case, args.reps, args.quick, args.sweep)
        ok = ok and o["identical"]
        bp, mp = o["bucket_plan"], o["matvec_plan"]
        print("(%s) %2d x %-7d x %-4d | c=%-2d b=%-3d depth=%-5d | %10d / %9d = %6.2f | %9.3f / %8.3f = %6.2f | %9.3f / %8.3f = %6.2f | %5.3f | %s | %s"
              % (case, o["rows"], o["cols"], o["e_bits"], bp["window"], bp["block"], bp["depth"], mp["products"], bp["products"],
                 o["product_ratio"], o["matvec"]["kernel_ms"], o["bucket"]["kernel_ms"], o["kernel_speedup"], o["matvec"]["wall_ms"],
                 o["bucket"]["wall_ms"], o["wall_speedup"], o["host_share_of_wall"],
                 {True: "met", False: "MISSED", None: "-"}[o["bar"]], "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("    matvec plan: w=%d S=%d table %d bytes; launches (kind, ms): %s" % (mp["window"], mp["slices"], mp["table_bytes"],
                                                                                    o["matvec"]["launches"]), flush=True)
        print("    bucket launches (kind, ms): %s   all runs: %s" % (o["bucket"]["launches"], o["bucket"]["kernel_ms_all"]), flush=True)
        for s in o.get("sweep", []):
            print("    PGPU_BUCKET_WINDOW=%-2d PGPU_BUCKET_BLOCK=%-4d %d launches %9d products depth %-5d | kernel %9.3f ms  wall %9.3f ms  %s"
                  % (s["window"], s["block"], s["launches"], s["products"], s["depth"], s["kernel_ms"], s["wall_ms"], s["kernel_ms_all"]),
                  flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
