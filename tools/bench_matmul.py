"""Encrypted matrix product: pgpu_batch_ct_matmul against the one route a caller had before it, the pgpu_batch_ct_spmv
formulation, on the same key and the same resident x, alternated in the same process (tools/, a measurement; bench.py is
the headline).

  matmul   pgpu_batch_ct_matmul(x, w, n_vec, rows): the rows * cols weights uploaded once
  spmv     pgpu_batch_ct_spmv with the flat matrix as x: n_vec * rows CSR rows of cols entries, column numbers v * cols + j,
           the weight matrix replicated n_vec times -- the host builds and uploads n_vec * rows * cols column numbers and
           as many weights, and the window table covers every column of x

Shapes (2048-bit key, 32-bit weights), n_vec x cols -> rows:
  (a) 64 x 256 -> 256      (b) 1024 x 64 -> 16      (c) 4096 x 256 -> 64: the tiled case      (d) 8 x 24 -> 8: latency-bound

Per route: HIP-event kernel time (pgpu_set_timing: the sum over the launches of the call) and wall time -- host clock from
the caller's arrays (the weight matrix; for spmv also the CSR build) to pgpu_synchronize after the call, the weight upload
included --, medians of --reps runs after one warm-up, the two routes alternating run by run, with the spread; the plans
and the pair products of both plan queries.  The results are downloaded and compared bit for bit; --transposed adds the
transposed layout on x stored the other way round (compared with the default result transposed).
--matvec times pgpu_batch_ct_matvec at 1024 x 1024 alone; with --root DIR the package of another tree (the parent commit,
built) is loaded instead of this one, so the same script measures before and after.

--force W,T,S forces the plan of the matmul route (the spmv route is untouched): a sweep is one run per plan.

usage: python tools/bench_matmul.py [--reps 5] [--cases abcd] [--transposed] [--force W,T,S] [--quick] [--matvec] [--root DIR]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KIND_MATMUL, KIND_SPMV, KIND_MATVEC = 11, 9, 5
BITS, E_BITS = 2048, 32
SHAPES = {"a": (64, 256, 256), "b": (1024, 16, 64), "c": (4096, 64, 256), "d": (8, 8, 24)}      # n_vec, rows, cols
QUICK = {"a": (4, 8, 8), "b": (16, 2, 4), "c": (12, 3, 8), "d": (2, 2, 3)}


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Box:
    def __init__(self, pa, capi):
        pa.initialize(0)
        self.capi, self.L = capi, capi.lib()

    def up(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        h = ctypes.c_void_p()
        self.capi.check(self.L.pgpu_batch_upload(ptr(arr), arr.shape[0], arr.shape[1], arr.shape[1], ctypes.byref(h)))
        return h

    def op(self, fn, *a):
        h = ctypes.c_void_p()
        self.capi.check(fn(*a, ctypes.byref(h)))
        return h

    def down(self, h):
        out = np.empty((self.L.pgpu_batch_count(h), self.L.pgpu_batch_words(h)), dtype=np.uint64)
        self.capi.check(self.L.pgpu_batch_download(h, ptr(out)))
        return out

    def free(self, *hs):
        for h in hs:
            self.L.pgpu_batch_destroy(h)

    def sync(self):
        self.capi.check(self.L.pgpu_synchronize())

    def timed(self, fn):
        """-> (wall ms, [(kind, ms)] of the launches, result handle)"""
        L = self.L
        self.sync()
        L.pgpu_set_timing(1)
        t0 = time.perf_counter()
        h = fn()
        self.sync()
        wall = (time.perf_counter() - t0) * 1e3
        cap = 1 << 14
        kinds, ms = (ctypes.c_int * cap)(), (ctypes.c_double * cap)()
        n = L.pgpu_timing_collect(kinds, ms, cap)
        L.pgpu_set_timing(0)
        return wall, [(kinds[i], ms[i]) for i in range(n)], h


def summary(walls, kerns, launches):
    return {"kernel_ms": round(statistics.median(kerns), 3), "wall_ms": round(statistics.median(walls), 3),
            "kernel_ms_all": [round(v, 3) for v in kerns], "wall_ms_all": [round(v, 3) for v in walls], "launches": launches}


def key_of():
    k = json.load(open(os.path.join(HERE, "..", "tests", "golden", "iso_kat.json")))
    return int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)


def encrypt(B, pk, rng, count):
    nw = BITS // 64
    bm = B.up(rng.integers(0, 1 << 62, size=(count, nw), dtype=np.uint64))
    br = B.up(rng.integers(0, 1 << 62, size=(count, nw // 2), dtype=np.uint64))
    x = B.op(B.L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2))
    B.free(bm, br)
    return x


def run_case(B, pk, case, shape, reps, transposed):
    L = B.L
    n_vec, rows, cols = shape
    rng = np.random.default_rng(ord(case))
    x = encrypt(B, pk, rng, n_vec * cols)
    w = rng.integers(0, 1 << E_BITS, size=(rows * cols, 1), dtype=np.uint64)
    pw, ps, pt, ptb, ppr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    B.capi.check(L.pgpu_ct_matmul_plan(BITS, n_vec, rows, cols, E_BITS, ctypes.byref(pw), ctypes.byref(ps), ctypes.byref(pt),
                                       ctypes.byref(ptb), ctypes.byref(ppr)))
    sw, sc, sl, stb, spr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    B.capi.check(L.pgpu_ct_spmv_plan(BITS, n_vec * rows, n_vec * cols, n_vec * rows * cols, cols, E_BITS, ctypes.byref(sw),
                                     ctypes.byref(sc), ctypes.byref(sl), ctypes.byref(stb), ctypes.byref(spr)))

    def matmul(xb=x, flags=0):
        wb = B.up(w)
        h = B.op(L.pgpu_batch_ct_matmul, pk._h, xb, wb, n_vec, rows, E_BITS, flags)
        B.free(wb)
        return h

    def spmv():
        row_ptr = np.arange(n_vec * rows + 1, dtype=np.uint64) * cols
        col_idx = (np.repeat(np.arange(n_vec, dtype=np.uint32) * cols, rows)[:, None] + np.arange(cols, dtype=np.uint32)[None, :]).reshape(-1)
        wb = B.up(np.tile(w, (n_vec, 1)))
        h = B.op(L.pgpu_batch_ct_spmv, pk._h, x, ptr(row_ptr), ptr(col_idx), wb, n_vec * rows, E_BITS)
        B.free(wb)
        return h

    routes = {"matmul": (matmul, KIND_MATMUL), "spmv": (spmv, KIND_SPMV)}
    outs, walls, kerns, launches = {}, {k: [] for k in routes}, {k: [] for k in routes}, {}
    for name, (fn, _) in routes.items():                      # warm-up (code objects, arena blocks); its result is the one compared
        _, _, h = B.timed(fn)
        outs[name] = B.down(h)
        B.free(h)
    for _ in range(reps):                                     # the two routes alternate
        for name, (fn, kind) in routes.items():
            wall, rec, h = B.timed(fn)
            B.free(h)
            assert all(k == kind for k, _ in rec), (name, rec[:8])
            walls[name].append(wall)
            kerns[name].append(sum(ms for _, ms in rec))
            launches[name] = len(rec)
    out = {"case": case, "key_bits": BITS, "e_bits": E_BITS, "n_vec": n_vec, "rows": rows, "cols": cols,
           "matmul_plan": {"window": pw.value, "slices": ps.value, "tile": pt.value, "passes": -(-n_vec // pt.value),
                           "table_bytes": ptb.value, "products": ppr.value},
           "spmv_plan": {"window": sw.value, "chunk": sc.value, "levels": sl.value, "table_bytes": stb.value, "products": spr.value},
           "product_ratio": round(spr.value / ppr.value, 3),
           "matmul": summary(walls["matmul"], kerns["matmul"], launches["matmul"]),
           "spmv": summary(walls["spmv"], kerns["spmv"], launches["spmv"]),
           "identical": bool(np.array_equal(outs["matmul"], outs["spmv"]))}
    out["kernel_speedup"] = round(out["spmv"]["kernel_ms"] / out["matmul"]["kernel_ms"], 3)
    out["wall_speedup"] = round(out["spmv"]["wall_ms"] / out["matmul"]["wall_ms"], 3)
    if transposed:
        xw = B.down(x)
        t = B.up(xw.reshape(n_vec, cols, -1).transpose(1, 0, 2).reshape(n_vec * cols, -1))
        zero = B.up(np.zeros((1, 1), dtype=np.uint64))
        xt = B.op(L.pgpu_batch_ct_add_plain, pk._h, t, zero)      # (CT + 0 turns the uploaded words into pair rows)
        B.free(t, zero)
        _, _, h = B.timed(lambda: matmul(xt, 1))
        got = B.down(h)
        B.free(h)
        tw, tk, n = [], [], 0
        for _ in range(reps):
            wall, rec, h = B.timed(lambda: matmul(xt, 1))
            B.free(h)
            tw.append(wall)
            tk.append(sum(ms for _, ms in rec))
            n = len(rec)
        out["matmul_transposed"] = summary(tw, tk, n)
        want = outs["matmul"].reshape(n_vec, rows, -1).transpose(1, 0, 2).reshape(n_vec * rows, -1)
        out["identical"] = out["identical"] and bool(np.array_equal(got, want))
        B.free(xt)
    B.free(x)
    return out


def run_matvec(B, pk, reps, quick):
    """pgpu_batch_ct_matvec alone at 1024 x 1024: the call this tree must not have moved"""
    L = B.L
    rows = cols = 32 if quick else 1024
    rng = np.random.default_rng(1024)
    x = encrypt(B, pk, rng, cols)
    wb = B.up(rng.integers(0, 1 << E_BITS, size=(rows * cols, 1), dtype=np.uint64))
    fn = lambda: B.op(L.pgpu_batch_ct_matvec, pk._h, x, wb, rows, E_BITS)      # noqa: E731
    _, _, h = B.timed(fn)
    digest = int(np.bitwise_xor.reduce(B.down(h).reshape(-1)))
    B.free(h)
    walls, kerns, n = [], [], 0
    for _ in range(reps):
        wall, rec, h = B.timed(fn)
        B.free(h)
        assert all(k == KIND_MATVEC for k, _ in rec)
        walls.append(wall)
        kerns.append(sum(ms for _, ms in rec))
        n = len(rec)
    B.free(x, wb)
    return {"matvec": "%d x %d" % (rows, cols), "key_bits": BITS, "e_bits": E_BITS, "xor_of_result_words": "%016x" % digest,
            **summary(walls, kerns, n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--transposed", action="store_true", help="also time the transposed layout")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--matvec", action="store_true", help="time pgpu_batch_ct_matvec at 1024 x 1024 instead of the cases")
    ap.add_argument("--force", default="", help="W,T,S: force PGPU_MATMUL_WINDOW / _TILE / _SLICES for the run (0: leave to the policy)")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the tree whose built package is loaded (default: this one)")
    args = ap.parse_args()
    for name in ("PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES", "PGPU_SPMV_CHUNK", "PGPU_SPMV_WINDOW",
                 "PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES"):
        os.environ.pop(name, None)
    if args.force:                                                 # (the knobs are read at every call, the plan query included)
        for name, v in zip(("PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES"), args.force.split(",")):
            if int(v) > 0:
                os.environ[name] = str(int(v))
    sys.path.insert(0, os.path.abspath(args.root))
    import pailliercryptolib_amd as pa
    from pailliercryptolib_amd import _capi
    B = Box(pa, _capi)
    p, q, hs = key_of()
    pk = pa.PublicKey(p * q, BITS, hs=hs)
    print("# box:", B.L.pgpu_device_name().decode(), "| package:", os.path.dirname(os.path.abspath(pa.__file__)), "| key", BITS,
          "| e_bits", E_BITS, "| reps:", args.reps, "| times: median, ms")
    if args.matvec:
        o = run_matvec(B, pk, args.reps, args.quick)
        print("matvec %s | kernel %.3f ms %s | wall %.3f ms | %d launches | xor %s"
              % (o["matvec"], o["kernel_ms"], o["kernel_ms_all"], o["wall_ms"], o["launches"], o["xor_of_result_words"]), flush=True)
        print("JSON " + json.dumps(o), flush=True)
        pa.terminate()
        return
    print("# case n_vec x cols -> rows | matmul plan w tile passes S table | spmv plan w | products spmv / matmul = ratio | "
          "kernel ms spmv / matmul = speed-up | wall ms spmv / matmul = speed-up | identical")
    ok = True
    for case in args.cases:
        o = run_case(B, pk, case, (QUICK if args.quick else SHAPES)[case], args.reps, args.transposed)
        ok = ok and o["identical"]
        mp, sp = o["matmul_plan"], o["spmv_plan"]
        print("(%s) %5d x %-4d -> %-4d | w=%d t=%-4d p=%-4d S=%-3d %6.1f MB | w=%d %7.1f MB | %11d / %10d = %5.2f | %10.3f / %9.3f = %5.2f | "
              "%10.3f / %9.3f = %5.2f | %s"
              % (case, o["n_vec"], o["cols"], o["rows"], mp["window"], mp["tile"], mp["passes"], mp["slices"], mp["table_bytes"] / 1e6,
                 sp["window"], sp["table_bytes"] / 1e6, sp["products"], mp["products"], o["product_ratio"], o["spmv"]["kernel_ms"],
                 o["matmul"]["kernel_ms"], o["kernel_speedup"], o["spmv"]["wall_ms"], o["matmul"]["wall_ms"], o["wall_speedup"],
                 "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("    kernel ms, all runs: matmul %s spmv %s" % (o["matmul"]["kernel_ms_all"], o["spmv"]["kernel_ms_all"]), flush=True)
        if "matmul_transposed" in o:
            t = o["matmul_transposed"]
            print("    transposed: kernel %.3f ms %s, wall %.3f ms, %d launches" % (t["kernel_ms"], t["kernel_ms_all"], t["wall_ms"], t["launches"]),
                  flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
