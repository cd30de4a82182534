"""Encrypted matrix-vector product: the fused call against the route a caller composes from the element-wise operations,
on the same key and the same resident inputs, in the same process (tools/, a measurement; bench.py is the headline).

  (a) fused      pgpu_batch_ct_matvec(x, w, rows)
  (b) composed   per column j: pgpu_batch_ct_mul of x[j] (tiled over the rows) by column j of w -- rows*cols terms in all --
                 then a ceil(log2 cols)-deep tree of pgpu_batch_ct_add over the column batches.  (The C-ABI has no views
                 into a batch, so the tree runs across batches of `rows` elements; every operand is resident pair rows
                 before the clock starts, and the intermediates of a shape stay in HBM: rows*cols pair rows.)

Both results are downloaded and compared bit for bit.  Per shape: HIP-event kernel time (pgpu_set_timing: the sum over
the launches of the route) and wall time (host clock around the calls, ending in pgpu_synchronize), the executed pair
products of both schedules, the plan (window, slices, table bytes), and for the multi-exponentiation kernel alone the
executed share of the 39.32 T MAC32/s peak.  One warm-up of each route, then --reps timed runs; the median is reported and
the spread printed.

usage: python tools/bench_matvec.py [--reps 3] [--quick]
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

PEAK_TMAC32 = 39.32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
KIND_MATVEC = 5
GEOMETRY = {1024: (2, 19), 2048: (4, 18), 3072: (8, 14)}
SHAPES = [(2048, 1, 1024, 32), (2048, 64, 1024, 32), (2048, 1024, 1024, 32), (2048, 4096, 256, 32), (3072, 256, 512, 32),
          (2048, 256, 512, 64)]
QUICK = [(2048, 1, 64, 32), (2048, 40, 96, 32), (3072, 16, 48, 32), (2048, 8, 24, 64)]


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def fixed_window(exp_bits):
    """csrc/policy.cpp: pick_window -- the window of pgpu_batch_ct_mul"""
    return min(range(1, 6), key=lambda w: ((1 << w) - 2) + (exp_bits + w - 1) // w)


class Box:
    def __init__(self):
        pa.initialize(0)
        self.L = _capi.lib()
        self.live = []

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
        cap = 1 << 16
        kinds, ms = (ctypes.c_int * cap)(), (ctypes.c_double * cap)()
        n = L.pgpu_timing_collect(kinds, ms, cap)
        L.pgpu_set_timing(0)
        return wall, [(kinds[i], ms[i]) for i in range(n)], h


def key_of(bits):
    if bits == 2048:
        k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
        return int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
    c = [c for c in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"] if c["bits"] == bits and c["djn"]][0]
    return int(c["p"], 16), int(c["q"], 16), int(c["hs"], 16)


def run_shape(B, bits, rows, cols, e_bits, reps):
    L = B.L
    p, q, hs = key_of(bits)
    pk = pa.PublicKey(p * q, bits, hs=hs)
    nw, ew = bits // 64, (e_bits + 63) // 64
    rng = np.random.default_rng(bits + rows + cols)
    # the encrypted vector: a resident DJN encrypt of random plaintexts
    m = rng.integers(0, 1 << 62, size=(cols, nw), dtype=np.uint64)
    r = rng.integers(0, 1 << 62, size=(cols, nw // 2), dtype=np.uint64)
    bm, br = B.up(m), B.up(r)
    x = B.op(L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2))
    xw = B.down(x)
    w = rng.integers(0, 1 << 63, size=(rows * cols, ew), dtype=np.uint64)
    if e_bits % 64:
        w[:, -1] &= np.uint64((1 << (e_bits % 64)) - 1)
    wb = B.up(w)
    plan_w, plan_s, plan_tb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _capi.check(L.pgpu_ct_matvec_plan(bits, rows, cols, e_bits, ctypes.byref(plan_w), ctypes.byref(plan_s), ctypes.byref(plan_tb)))
    pw, ps = plan_w.value, plan_s.value
    # composed route's operands, resident as pair rows: x[j] tiled over the rows (CT + PT with the plaintext 0 turns the
    # uploaded words into pair rows), column j of w
    zero = B.up(np.zeros((1, 1), dtype=np.uint64))
    w3 = w.reshape(rows, cols, ew)
    xt, wc = [], []
    for j in range(cols):
        t = B.up(np.repeat(xw[j:j + 1], rows, axis=0))
        xt.append(B.op(L.pgpu_batch_ct_add_plain, pk._h, t, zero))
        B.free(t)
        wc.append(B.up(w3[:, j, :]))
    B.sync()

    def fused():
        return B.op(L.pgpu_batch_ct_matvec, pk._h, x, wb, rows, e_bits)

    def composed():
        cur = [B.op(L.pgpu_batch_ct_mul, pk._h, xt[j], wc[j], e_bits) for j in range(cols)]
        while len(cur) > 1:
            nxt = []
            for k in range(0, len(cur) - 1, 2):
                nxt.append(B.op(L.pgpu_batch_ct_add, pk._h, cur[k], cur[k + 1]))
                B.free(cur[k], cur[k + 1])
            if len(cur) % 2:
                nxt.append(cur[-1])
            cur = nxt
        return cur[0]

    res = {}
    for name, fn in (("fused", fused), ("composed", composed)):
        _, _, h = B.timed(fn)                      # warm-up (code objects, arena blocks); its result is the one compared
        res[name + "_out"] = B.down(h)
        B.free(h)
        walls, kerns, main = [], [], []
        for _ in range(reps):
            wall, rec, h = B.timed(fn)
            B.free(h)
            walls.append(wall)
            kerns.append(sum(ms for _, ms in rec))
            if name == "fused":
                assert all(k == KIND_MATVEC for k, _ in rec), rec
                main.append(rec[1][1])             # launches: table build, multi-exponentiation, folds
        res[name] = {"wall_ms": statistics.median(walls), "kernel_ms": statistics.median(kerns),
                     "kernel_ms_all": [round(v, 3) for v in kerns]}
        if main:
            res[name]["multiexp_ms"] = statistics.median(main)
    identical = bool(np.array_equal(res["fused_out"], res["composed_out"]))
    # executed pair products of the two schedules
    nwin = (e_bits + pw - 1) // pw
    f_sq, f_mul = rows * ps * (nwin - 1) * pw, rows * (cols * nwin - ps)
    f_prod = cols * ((1 << pw) - 2) + f_sq + f_mul + rows * (ps - 1)
    cw = fixed_window(e_bits)
    cn = (e_bits + cw - 1) // cw
    c_prod = rows * cols * ((cn - 1) * cw + (cn - 1) + (1 << cw) - 2) + rows * (cols - 1)
    g, k = GEOMETRY[bits]
    l2 = g * k
    macs = f_sq * (l2 * (l2 + g) // 2 + 3 * l2 * l2) + f_mul * 5 * l2 * l2       # the multi-exponentiation kernel alone
    out = {"key_bits": bits, "rows": rows, "cols": cols, "e_bits": e_bits, "window": pw, "slices": ps,
           "table_bytes": plan_tb.value, "identical": identical,
           "fused_kernel_ms": round(res["fused"]["kernel_ms"], 3), "fused_wall_ms": round(res["fused"]["wall_ms"], 3),
           "composed_kernel_ms": round(res["composed"]["kernel_ms"], 3), "composed_wall_ms": round(res["composed"]["wall_ms"], 3),
           "fused_products": f_prod, "composed_products": c_prod, "product_ratio": round(c_prod / f_prod, 2),
           "kernel_speedup": round(res["composed"]["kernel_ms"] / res["fused"]["kernel_ms"], 2),
           "wall_speedup": round(res["composed"]["wall_ms"] / res["fused"]["wall_ms"], 2),
           "multiexp_ms": round(res["fused"]["multiexp_ms"], 3),
           "multiexp_frac_of_peak": round(macs / (res["fused"]["multiexp_ms"] * 1e-3) / 1e12 / PEAK_TMAC32, 3),
           "fused_kernel_ms_all": res["fused"]["kernel_ms_all"], "composed_kernel_ms_all": res["composed"]["kernel_ms_all"]}
    B.free(bm, br, x, wb, zero, *xt, *wc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    B = Box()
    print("# box:", B.L.pgpu_device_name().decode(), "| reps:", args.reps, "| times: median, ms")
    print("# key rows x cols e_bits | plan w S table | products composed / fused = ratio | kernel ms composed / fused = speed-up "
          "| wall ms composed / fused = speed-up | multi-exp kernel ms, share of %.2f T MAC32/s | identical" % PEAK_TMAC32)
    ok = True
    for bits, rows, cols, e_bits in (QUICK if args.quick else SHAPES):
        o = run_shape(B, bits, rows, cols, e_bits, args.reps)
        ok = ok and o["identical"]
        print("%d %5d x %-5d %3d | w=%d S=%-3d %6.1f MB | %11d / %10d = %5.2f | %9.3f / %8.3f = %5.2f | %9.3f / %8.3f = %5.2f | %8.3f %.3f | %s"
              % (bits, rows, cols, e_bits, o["window"], o["slices"], o["table_bytes"] / 1e6, o["composed_products"],
                 o["fused_products"], o["product_ratio"], o["composed_kernel_ms"], o["fused_kernel_ms"], o["kernel_speedup"],
                 o["composed_wall_ms"], o["fused_wall_ms"], o["wall_speedup"], o["multiexp_ms"], o["multiexp_frac_of_peak"],
                 "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("fused and composed results differ")


if __name__ == "__main__":
    main()
