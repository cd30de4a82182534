"""Encrypted sparse matrix-vector product: the fused call against the routes a caller has today, on the same key and the
same resident inputs, in the same process (tools/, a measurement; bench.py is the headline).

  spmv       pgpu_batch_ct_spmv(x, row_ptr, col_idx, w, rows)
  composed   pgpu_batch_ct_mul of the GATHERED x[col_idx[t]] by w[t] -- one term per non-zero, each with its own squaring
             chain and window table -- then pgpu_batch_ct_segment_sum with the row of every term as its segment id.  The
             C-ABI has no gather: where a column is used by more than one row the gathered batch is uploaded before the
             clock starts (pre-gathered; a caller would pay a host gather on top), where every column is used exactly once
             in CSR order (the group-by case) x itself is the operand.
  dense      pgpu_batch_ct_matvec on the same matrix written out densely (case c only)

Cases (2048-bit key, 32-bit weights):
  (a) 65536 rows x 16 random non-zeros over 65536 columns        the graph / sparse-layer shape
  (b) 2^20 elements into 1024 segments, one non-zero per column   a weighted group-by
  (c) 1024 x 1024 at 10 % density                                 against the dense matvec
  (d) 256 rows x 8 over 256 columns                               the latency end

All results of a case are downloaded and compared bit for bit.  Per route: HIP-event kernel time (pgpu_set_timing: the sum
over the launches) and wall time (host clock around the calls, ending in pgpu_synchronize), medians of --reps runs after
one warm-up, with the spread; the plan (window, chunk, levels, table bytes) and the pair products of both schedules.
--sweep forces PGPU_SPMV_CHUNK over a range on cases (a) and (b) and compares every result with the default plan's.

usage: python tools/bench_spmv.py [--reps 5] [--cases abcd] [--sweep] [--quick]
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
KIND_SPMV = 9
BITS, E_BITS = 2048, 32
SWEEP = {"a": (4, 8, 16), "b": (4, 8, 16, 32, 64, 128, 256, 1024), "q": (1, 2, 4)}


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
    if bits == 2048:
        k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
        return int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
    c = [c for c in json.load(open(os.path.join(GOLD, "seeded_vectors.json")))["cases"] if c["bits"] == bits and c["djn"]][0]
    return int(c["p"], 16), int(c["q"], 16), int(c["hs"], 16)


def matrix(case, rng, quick):
    """-> rows, cols, row_ptr (uint64), col_idx (uint32), each column once in CSR order?"""
    if case == "a":
        rows, cols, per = (512, 512, 16) if quick else (65536, 65536, 16)
        return rows, cols, np.arange(rows + 1, dtype=np.uint64) * per, rng.integers(0, cols, size=rows * per, dtype=np.uint32), False
    if case == "b":
        n, segs = (4096, 16) if quick else (1 << 20, 1024)
        ids = rng.integers(0, segs, size=n)
        order = np.argsort(ids, kind="stable").astype(np.uint32)       # the group-by as CSR: indices = argsort(ids)
        row_ptr = np.concatenate(([0], np.cumsum(np.bincount(ids, minlength=segs)))).astype(np.uint64)
        return segs, n, row_ptr, order, True
    if case == "c":
        rows = cols = 64 if quick else 1024
        mask = rng.random((rows, cols)) < 0.10
        row_ptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1)))).astype(np.uint64)
        return rows, cols, row_ptr, np.nonzero(mask)[1].astype(np.uint32), False
    rows, cols, per = (16, 16, 8) if quick else (256, 256, 8)
    return rows, cols, np.arange(rows + 1, dtype=np.uint64) * per, rng.integers(0, cols, size=rows * per, dtype=np.uint32), False


def run_case(B, pk, case, reps, quick, sweep):
    L = B.L
    nw = BITS // 64
    rng = np.random.default_rng(ord(case))
    rows, cols, row_ptr, col_idx, once = matrix(case, rng, quick)
    nnz = int(row_ptr[-1])
    lens = np.diff(row_ptr.astype(np.int64))
    # the encrypted vector: a resident DJN encrypt of random plaintexts
    bm = B.up(rng.integers(0, 1 << 62, size=(cols, nw), dtype=np.uint64))
    br = B.up(rng.integers(0, 1 << 62, size=(cols, nw // 2), dtype=np.uint64))
    x = B.op(L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2))
    B.free(bm, br)
    w = rng.integers(0, 1 << E_BITS, size=(nnz, 1), dtype=np.uint64)
    wb = B.up(w)
    pw, pc, pl, ptb, ppr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    _capi.check(L.pgpu_ct_spmv_plan(BITS, rows, cols, nnz, int(lens.max()), E_BITS, ctypes.byref(pw), ctypes.byref(pc),
                                    ctypes.byref(pl), ctypes.byref(ptb), ctypes.byref(ppr)))

    def products(chunk, win):
        chains = int(np.maximum(1, -(-lens // chunk)).sum())
        return cols * ((1 << win) - 2) + chains * E_BITS + nnz * -(-E_BITS // win) + (chains - rows)

    def spmv():
        return B.op(L.pgpu_batch_ct_spmv, pk._h, x, ptr(row_ptr), ptr(col_idx), wb, rows, E_BITS)

    out = {"case": case, "key_bits": BITS, "rows": rows, "cols": cols, "nnz": nnz, "longest_row": int(lens.max()),
           "e_bits": E_BITS, "window": pw.value, "chunk": pc.value, "levels": pl.value, "table_bytes": ptb.value,
           "spmv_products": products(pc.value, pw.value)}
    ref, out["spmv"] = B.measure(spmv, reps)
    assert all(k == KIND_SPMV for k, _ in out["spmv"]["launches"])
    # the composed route: CT x PT per term, then the segmented sum over the rows
    ids = np.repeat(np.arange(rows, dtype=np.uint32), lens)
    if once:                                                           # x itself, weights and ids in element order
        xg, wv, ids_el = x, np.empty_like(w), np.empty_like(ids)
        wv[col_idx], ids_el[col_idx] = w, ids
        wc, ids = B.up(wv), ids_el
    else:
        wc = wb
        t = B.up(B.down(x)[col_idx])                                   # pre-gathered on the host, before the clock starts
        zero = B.up(np.zeros((1, 1), dtype=np.uint64))
        xg = B.op(L.pgpu_batch_ct_add_plain, pk._h, t, zero)           # (CT + 0 turns the uploaded words into pair rows)
        B.free(t, zero)

    def composed():
        terms = B.op(L.pgpu_batch_ct_mul, pk._h, xg, wc, E_BITS)
        h = B.op(L.pgpu_batch_ct_segment_sum, pk._h, terms, ptr(ids), 1, rows)
        B.free(terms)
        return h
    got, out["composed"] = B.measure(composed, reps)
    out["composed_pre_gathered"] = not once
    identical = bool(np.array_equal(ref, got))
    cw = fixed_window(E_BITS)
    cn = -(-E_BITS // cw)
    out["composed_products"] = nnz * ((cn - 1) * cw + (cn - 1) + (1 << cw) - 2) + int(np.maximum(0, lens - 1).sum())
    out["product_ratio"] = round(out["composed_products"] / out["spmv_products"], 2)
    out["kernel_speedup"] = round(out["composed"]["kernel_ms"] / out["spmv"]["kernel_ms"], 2)
    out["wall_speedup"] = round(out["composed"]["wall_ms"] / out["spmv"]["wall_ms"], 2)
    B.free(wc if once else xg)
    if case == "c":                                                    # the dense call on the same matrix
        dense = np.zeros((rows * cols, 1), dtype=np.uint64)
        dense[np.repeat(np.arange(rows), lens) * cols + col_idx, 0] = w[:, 0]
        db = B.up(dense)
        got, out["dense"] = B.measure(lambda: B.op(L.pgpu_batch_ct_matvec, pk._h, x, db, rows, E_BITS), reps)
        identical = identical and bool(np.array_equal(ref, got))
        out["dense_kernel_speedup"] = round(out["dense"]["kernel_ms"] / out["spmv"]["kernel_ms"], 2)
        B.free(db)
    if sweep and (case in SWEEP or quick):
        out["sweep"] = []
        for chunk in SWEEP["q" if quick else case]:
            os.environ["PGPU_SPMV_CHUNK"] = str(chunk)                 # (read at every call)
            try:
                got, r = B.measure(spmv, reps)
            finally:
                del os.environ["PGPU_SPMV_CHUNK"]
            identical = identical and bool(np.array_equal(ref, got))
            out["sweep"].append({"chunk": chunk, "kernel_ms": r["kernel_ms"], "wall_ms": r["wall_ms"],
                                 "launches": len(r["launches"]), "products": products(chunk, pw.value),
                                 "kernel_ms_all": r["kernel_ms_all"]})
    out["identical"] = identical
    B.free(x, wb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--sweep", action="store_true", help="force PGPU_SPMV_CHUNK over a range on cases (a) and (b)")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    for name in ("PGPU_SPMV_CHUNK", "PGPU_SPMV_WINDOW"):
        os.environ.pop(name, None)
    B = Box()
    p, q, hs = key_of(BITS)
    pk = pa.PublicKey(p * q, BITS, hs=hs)
    print("# box:", B.L.pgpu_device_name().decode(), "| key", BITS, "| e_bits", E_BITS, "| reps:", args.reps, "| times: median, ms")
    print("# case rows x cols nnz | plan w chunk levels table | products composed / spmv = ratio | kernel ms composed / spmv = speed-up "
          "| wall ms composed / spmv = speed-up | identical")
    ok = True
    for case in args.cases:
        o = run_case(B, pk, case, args.reps, args.quick, args.sweep)
        ok = ok and o["identical"]
        print("(%s) %6d x %-7d %8d | w=%d c=%-3d L=%d %7.1f MB | %10d / %9d = %5.2f | %9.3f / %8.3f = %5.2f | %9.3f / %8.3f = %5.2f | %s"
              % (case, o["rows"], o["cols"], o["nnz"], o["window"], o["chunk"], o["levels"], o["table_bytes"] / 1e6,
                 o["composed_products"], o["spmv_products"], o["product_ratio"], o["composed"]["kernel_ms"], o["spmv"]["kernel_ms"],
                 o["kernel_speedup"], o["composed"]["wall_ms"], o["spmv"]["wall_ms"], o["wall_speedup"],
                 "identical" if o["identical"] else "DIFFERENT"), flush=True)
        if "dense" in o:
            print("    dense matvec: kernel %.3f ms, wall %.3f ms; spmv is %.2f x by kernel time"
                  % (o["dense"]["kernel_ms"], o["dense"]["wall_ms"], o["dense_kernel_speedup"]), flush=True)
        for s in o.get("sweep", []):
            print("    PGPU_SPMV_CHUNK=%-5d %2d launches %10d products | kernel %9.3f ms  wall %9.3f ms  %s"
                  % (s["chunk"], s["launches"], s["products"], s["kernel_ms"], s["wall_ms"], s["kernel_ms_all"]), flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
