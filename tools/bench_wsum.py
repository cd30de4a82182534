"""Encrypted weighted sum of K resident batches: the fused call against the route a caller can compose today, on the same
key and the same resident inputs, in the same process (tools/, a measurement; bench.py is the headline).

  fused      pgpu_batch_ct_weighted_sum(xs, K, weights)
  composed   K pgpu_batch_ct_mul calls with a one-element exponent (each with its own squaring chain and window table),
             then K - 1 pgpu_batch_ct_add calls; with weights == NULL the K - 1 pgpu_batch_ct_add calls alone

Cases (2048-bit key):
  (a) K = 16, 65536 elements, random 32-bit weights      the federated average
  (b) K = 16, 65536 elements, weights == NULL            the plain sum
  (c) K = 64, 16384 elements, random 32-bit weights      many clients
  (d) K = 16, 256 elements, random 32-bit weights        the latency end

The results of both routes are downloaded and compared bit for bit.  Per route: HIP-event kernel time (pgpu_set_timing:
the sum over the launches) and wall time (host clock around the calls, ending in pgpu_synchronize), medians of --reps runs
after one warm-up, with the spread; the plan (form, slices, steps) and the pair products of both schedules per element.
The roofline share weighs the fused schedule's squarings with 4788 and its products with 6696 32-bit multiplies (the
(4,18) form) against 39.32 T MAC32/s.  --sweep forces PGPU_WSUM_SLICES and PGPU_WSUM_WIDE over a
range on cases (c) and (d) and compares every result with the default plan's.

usage: python tools/bench_wsum.py [--reps 5] [--cases abcd] [--sweep] [--quick]
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
KIND_WSUM = 10
BITS, E_BITS = 2048, 32
PEAK_MAC32 = 39.32e12
MUL_SQR, MUL_GEN = 4788, 6696
CASES = {"a": (16, 65536, True), "b": (16, 65536, False), "c": (64, 16384, True), "d": (16, 256, True)}
QUICK = {"a": (4, 300, True), "b": (4, 300, False), "c": (9, 100, True), "d": (16, 20, True)}
SWEEP_SLICES = (1, 2, 4, 8, 16)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def fixed_window(exp_bits):
    """csrc/policy.cpp: pick_window -- the window of pgpu_batch_ct_mul"""
    return min(range(1, 6), key=lambda w: ((1 << w) - 2) + (exp_bits + w - 1) // w)


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


def key_of(bits):
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    return int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)


def plan_of(L, count, K, w):
    g, k, s, st, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    _capi.check(L.pgpu_ct_weighted_sum_plan(BITS, count, K, ptr(w) if w is not None else None, 1 if w is not None else 0,
                                            ctypes.byref(g), ctypes.byref(k), ctypes.byref(s), ctypes.byref(st), ctypes.byref(pr)))
    return {"lanes": g.value, "limbs": k.value, "slices": s.value, "steps": st.value, "products": pr.value // count}


def run_case(B, pk, case, reps, quick, sweep):
    L = B.L
    nw = BITS // 64
    rng = np.random.default_rng(ord(case))
    K, count, weighted = (QUICK if quick else CASES)[case]
    # K clients' encrypted vectors: resident DJN encrypts of random plaintexts
    xs = []
    for _ in range(K):
        bm = B.up(rng.integers(0, 1 << 62, size=(count, nw), dtype=np.uint64))
        br = B.up(rng.integers(0, 1 << 62, size=(count, nw // 2), dtype=np.uint64))
        xs.append(B.op(L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2)))
        B.free(bm, br)
    arr = (ctypes.c_void_p * K)(*[h.value for h in xs])
    w = rng.integers(0, 1 << E_BITS, size=(K, 1), dtype=np.uint64) if weighted else None

    def fused():
        return B.op(L.pgpu_batch_ct_weighted_sum, pk._h, arr, K, ptr(w) if weighted else None, 1 if weighted else 0)

    out = {"case": case, "key_bits": BITS, "terms": K, "count": count, "weighted": weighted, "plan": plan_of(L, count, K, w)}
    ref, out["fused"] = B.measure(fused, reps)
    assert all(k == KIND_WSUM for k, _ in out["fused"]["launches"])
    es = [B.up(w[k:k + 1]) for k in range(K)] if weighted else []

    def composed():
        acc = None
        for k in range(K):
            term = B.op(L.pgpu_batch_ct_mul, pk._h, xs[k], es[k], E_BITS) if weighted else xs[k]
            if acc is None:
                acc = term
                continue
            nxt = B.op(L.pgpu_batch_ct_add, pk._h, acc, term)
            if weighted:
                B.free(term)
            if weighted or k > 1:
                B.free(acc)
            acc = nxt
        return acc
    got, out["composed"] = B.measure(composed, reps)
    identical = bool(np.array_equal(ref, got))
    cw = fixed_window(E_BITS)
    cn = -(-E_BITS // cw)
    per_term = (cn - 1) * cw + (cn - 1) + (1 << cw) - 2
    out["composed_products"] = (K * per_term if weighted else 0) + K - 1
    out["fused_products"] = out["plan"]["products"]
    out["product_ratio"] = round(out["composed_products"] / max(1, out["fused_products"]), 2)
    out["kernel_speedup"] = round(out["composed"]["kernel_ms"] / out["fused"]["kernel_ms"], 2)
    out["wall_speedup"] = round(out["composed"]["wall_ms"] / out["fused"]["wall_ms"], 2)
    # the share of the multiply roofline: squarings and products of the fused schedule, from the weights
    if weighted:
        S = out["plan"]["slices"]
        cuts = [w[s * K // S:(s + 1) * K // S, 0] for s in range(S)]
        sq = sum(int(c.max()).bit_length() - 1 for c in cuts if c.any())
    else:
        sq = 0
    mul = out["fused_products"] - sq
    out["squarings"], out["general_products"] = sq, mul
    out["roofline_share"] = round(count * (sq * MUL_SQR + mul * MUL_GEN) / (out["fused"]["kernel_ms"] * 1e-3) / PEAK_MAC32, 4)
    if sweep and (case in "cd" or quick):
        out["sweep"] = []
        for wide in (0, 1):
            for slices in SWEEP_SLICES:
                if slices > K:
                    continue
                os.environ["PGPU_WSUM_SLICES"], os.environ["PGPU_WSUM_WIDE"] = str(slices), str(wide)    # (read at every call)
                try:
                    p = plan_of(L, count, K, w)
                    got, r = B.measure(fused, reps)
                finally:
                    del os.environ["PGPU_WSUM_SLICES"], os.environ["PGPU_WSUM_WIDE"]
                identical = identical and bool(np.array_equal(ref, got))
                out["sweep"].append({"slices": slices, "wide": wide, "form": (p["lanes"], p["limbs"]), "products": p["products"],
                                     "kernel_ms": r["kernel_ms"], "wall_ms": r["wall_ms"], "launches": len(r["launches"]),
                                     "kernel_ms_all": r["kernel_ms_all"]})
    out["identical"] = identical
    B.free(*xs, *es)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--sweep", action="store_true", help="force PGPU_WSUM_SLICES / PGPU_WSUM_WIDE over a range on cases (c) and (d)")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    for name in ("PGPU_WSUM_SLICES", "PGPU_WSUM_WIDE"):
        os.environ.pop(name, None)
    B = Box()
    p, q, hs = key_of(BITS)
    pk = pa.PublicKey(p * q, BITS, hs=hs)
    print("# box:", B.L.pgpu_device_name().decode(), "| key", BITS, "| e_bits", E_BITS, "| reps:", args.reps, "| times: median, ms")
    print("# case K x count | plan form slices steps | products per element composed / fused = ratio | kernel ms composed / fused = "
          "speed-up | wall ms composed / fused = speed-up | roofline share | identical")
    ok = True
    for case in args.cases:
        o = run_case(B, pk, case, args.reps, args.quick, args.sweep)
        ok = ok and o["identical"]
        pl = o["plan"]
        print("(%s) %3d x %-6d %s | (%d,%d) S=%-2d steps=%-4d | %5d / %4d = %5.2f | %9.3f / %8.3f = %5.2f | %9.3f / %8.3f = %5.2f | %6.4f | %s"
              % (case, o["terms"], o["count"], "w32 " if o["weighted"] else "NULL", pl["lanes"], pl["limbs"], pl["slices"], pl["steps"],
                 o["composed_products"], o["fused_products"], o["product_ratio"], o["composed"]["kernel_ms"], o["fused"]["kernel_ms"],
                 o["kernel_speedup"], o["composed"]["wall_ms"], o["fused"]["wall_ms"], o["wall_speedup"], o["roofline_share"],
                 "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("    fused launches (kind, ms): %s   all runs: %s" % (o["fused"]["launches"], o["fused"]["kernel_ms_all"]), flush=True)
        for s in o.get("sweep", []):
            print("    PGPU_WSUM_SLICES=%-3d PGPU_WSUM_WIDE=%d (%d,%d) %d launches %5d products | kernel %9.3f ms  wall %9.3f ms  %s"
                  % (s["slices"], s["wide"], s["form"][0], s["form"][1], s["launches"], s["products"], s["kernel_ms"], s["wall_ms"],
                     s["kernel_ms_all"]), flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
