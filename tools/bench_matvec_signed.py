"""Signed-weight encrypted matvec / matmul: the signed call against the two routes a caller has without it, on the same key
and the same resident x, in the same process (tools/, a measurement; bench.py is the headline).

  (a) signed     pgpu_batch_ct_matvec_signed(x, W)                      (matmul shapes: pgpu_batch_ct_matmul_signed)
  (b) composed   pgpu_batch_ct_sub(matvec(x, W+), matvec(x, W-))        two unsigned calls over the same x and an inversion of
                                                                        the results: what a caller can do without (a)
  (c) unsigned   pgpu_batch_ct_matvec(x, |W|)                           the same shape and e_bits: what the sign costs

(a) and (b) are downloaded and compared bit for bit.  Per shape: HIP-event kernel time (pgpu_set_timing: the sum over the
launches of the route; for (a) the inversion's share -- kind PGPU_KERNEL_INVERT and the conversions of its one host round
trip -- is broken out) and wall time (host clock around the calls, ending in pgpu_synchronize), and the pair products of
the three plans.  One warm-up of each route, then --reps timed runs; medians, the spread printed.
--unsigned-only times (c) alone (the existing calls, for a comparison between two builds of the library).

usage: python tools/bench_matvec_signed.py [--reps 5] [--quick] [--unsigned-only]
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
BITS, E_BITS = 2048, 32
KIND_MATVEC, KIND_MATMUL, KIND_INVERT = 5, 11, 14
# (n_vec, rows, cols): n_vec = 0 is the matvec call
SHAPES = [(0, 1024, 1024), (0, 4096, 256), (0, 1, 1024), (1024, 16, 64), (64, 256, 256)]
QUICK = [(0, 40, 96), (0, 1, 64), (24, 8, 16)]
UNSIGNED_ONLY = [(0, 1024, 1024), (1024, 16, 64)]


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


def unsigned_products(L, n_vec, rows, cols):
    if n_vec:
        pr = ctypes.c_size_t()
        _capi.check(L.pgpu_ct_matmul_plan(BITS, n_vec, rows, cols, E_BITS, None, None, None, None, ctypes.byref(pr)))
        return pr.value
    w, s = ctypes.c_int(), ctypes.c_int()
    _capi.check(L.pgpu_ct_matvec_plan(BITS, rows, cols, E_BITS, ctypes.byref(w), ctypes.byref(s), None))
    w, s = w.value, s.value
    return cols * ((1 << w) - 2) + rows * s * E_BITS + rows * cols * ((E_BITS + w - 1) // w) + rows * (s - 1)


def signed_plan(L, n_vec, rows, cols):
    w, s, t, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(1), ctypes.c_size_t()
    if n_vec:
        _capi.check(L.pgpu_ct_matmul_signed_plan(BITS, n_vec, rows, cols, E_BITS, ctypes.byref(w), ctypes.byref(s), ctypes.byref(t),
                                                 None, ctypes.byref(pr)))
    else:
        _capi.check(L.pgpu_ct_matvec_signed_plan(BITS, rows, cols, E_BITS, ctypes.byref(w), ctypes.byref(s), None, ctypes.byref(pr)))
    return w.value, s.value, t.value, pr.value


def run_shape(B, pk, n_vec, rows, cols, reps, unsigned_only):
    L = B.L
    nw = BITS // 64
    nv = max(n_vec, 1)
    rng = np.random.default_rng(rows + cols + n_vec)
    m = rng.integers(0, 1 << 62, size=(nv * cols, nw), dtype=np.uint64)
    r = rng.integers(0, 1 << 62, size=(nv * cols, nw // 2), dtype=np.uint64)
    bm, br = B.up(m), B.up(r)
    x = B.op(L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2))
    ws = rng.integers(-(1 << 31), 1 << 31, size=(rows * cols, 1), dtype=np.int64)        # uniformly random signed 32-bit weights
    w_signed = B.up(ws.view(np.uint64))
    w_pos, w_neg, w_abs = B.up(np.maximum(ws, 0).astype(np.uint64)), B.up(np.maximum(-ws, 0).astype(np.uint64)), \
        B.up((np.abs(ws) & 0xFFFFFFFF).astype(np.uint64))
    n_out = nv * rows

    def unsigned_call(w):
        if n_vec:
            return B.op(L.pgpu_batch_ct_matmul, pk._h, x, w, n_vec, rows, E_BITS, 0)
        return B.op(L.pgpu_batch_ct_matvec, pk._h, x, w, rows, E_BITS)

    def signed():
        if n_vec:
            return B.op(L.pgpu_batch_ct_matmul_signed, pk._h, x, w_signed, n_vec, rows, E_BITS, 0)
        return B.op(L.pgpu_batch_ct_matvec_signed, pk._h, x, w_signed, rows, E_BITS)

    def composed():
        yp, yn = unsigned_call(w_pos), unsigned_call(w_neg)
        y = B.op(L.pgpu_batch_ct_sub, pk._h, yp, yn)
        B.free(yp, yn)
        return y

    routes = [("unsigned", lambda: unsigned_call(w_abs))] if unsigned_only else \
        [("signed", signed), ("composed", composed), ("unsigned", lambda: unsigned_call(w_abs))]
    res, outs = {}, {}
    for name, fn in routes:
        _, _, h = B.timed(fn)                      # warm-up (code objects, arena blocks); its result is the one compared
        if name != "unsigned":
            outs[name] = B.down(h)
        B.free(h)
    for _ in range(reps):                          # the routes alternate
        for name, fn in routes:
            wall, rec, h = B.timed(fn)
            B.free(h)
            own = sum(ms for k, ms in rec if k in (KIND_MATVEC, KIND_MATMUL))
            d = res.setdefault(name, {"wall": [], "kernel": [], "own": [], "launches": len(rec)})
            d["wall"].append(wall)
            d["kernel"].append(sum(ms for _, ms in rec))
            d["own"].append(own)
    med = {name: {k: statistics.median(v) for k, v in d.items() if isinstance(v, list)} for name, d in res.items()}
    out = {"n_vec": n_vec, "rows": rows, "cols": cols, "e_bits": E_BITS, "key_bits": BITS,
           "unsigned_products": unsigned_products(L, n_vec, rows, cols),
           "unsigned_kernel_ms": round(med["unsigned"]["kernel"], 3), "unsigned_wall_ms": round(med["unsigned"]["wall"], 3),
           "unsigned_kernel_ms_all": [round(v, 3) for v in res["unsigned"]["kernel"]]}
    if not unsigned_only:
        pw, ps, pt, pr = signed_plan(L, n_vec, rows, cols)
        up = out["unsigned_products"]
        cp = 2 * up + 3 * (n_out - 1) + n_out     # two unsigned calls and the subtraction: 3 (c - 1) + c
        identical = bool(np.array_equal(outs["signed"], outs["composed"]))
        out.update({"window": pw, "slices": ps, "tile": pt, "identical": identical, "signed_products": pr, "composed_products": cp,
                    "product_ratio_composed": round(cp / pr, 3), "product_ratio_unsigned": round(pr / up, 4),
                    "signed_kernel_ms": round(med["signed"]["kernel"], 3), "signed_wall_ms": round(med["signed"]["wall"], 3),
                    "signed_inversion_ms": round(med["signed"]["kernel"] - med["signed"]["own"], 3),
                    "signed_launches": res["signed"]["launches"], "composed_launches": res["composed"]["launches"],
                    "composed_kernel_ms": round(med["composed"]["kernel"], 3), "composed_wall_ms": round(med["composed"]["wall"], 3),
                    "kernel_speedup_composed": round(med["composed"]["kernel"] / med["signed"]["kernel"], 3),
                    "wall_speedup_composed": round(med["composed"]["wall"] / med["signed"]["wall"], 3),
                    "kernel_ratio_unsigned": round(med["signed"]["kernel"] / med["unsigned"]["kernel"], 3),
                    "signed_kernel_ms_all": [round(v, 3) for v in res["signed"]["kernel"]],
                    "composed_kernel_ms_all": [round(v, 3) for v in res["composed"]["kernel"]]})
    B.free(bm, br, x, w_signed, w_pos, w_neg, w_abs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--unsigned-only", action="store_true", help="the existing unsigned calls alone, at two shapes")
    args = ap.parse_args()
    B = Box()
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    pk = pa.PublicKey(int(k["p"], 16) * int(k["q"], 16), BITS, hs=int(k["bench_hs"], 16))
    print("# box:", B.L.pgpu_device_name().decode(), "| key", BITS, "| e_bits", E_BITS, "| reps:", args.reps, "| times: median, ms")
    shapes = UNSIGNED_ONLY if args.unsigned_only else QUICK if args.quick else SHAPES
    ok = True
    for n_vec, rows, cols in shapes:
        o = run_shape(B, pk, n_vec, rows, cols, args.reps, args.unsigned_only)
        name = ("matmul %d x %d -> %d" % (n_vec, cols, rows)) if n_vec else "matvec %d x %d" % (rows, cols)
        if args.unsigned_only:
            print("%-26s | unsigned kernel %9.3f ms, wall %9.3f ms | runs %s" % (name, o["unsigned_kernel_ms"], o["unsigned_wall_ms"],
                                                                               o["unsigned_kernel_ms_all"]), flush=True)
        else:
            ok = ok and o["identical"]
            print("%-26s | w=%d S=%d tile=%d | products composed / signed = %.2f, signed / unsigned = %.4f | kernel ms composed %.3f / "
                  "signed %.3f = %.2f (inversion %.3f), unsigned %.3f: signed / unsigned = %.3f | wall ms composed %.3f / signed %.3f = %.2f | %s"
                  % (name, o["window"], o["slices"], o["tile"], o["product_ratio_composed"], o["product_ratio_unsigned"],
                     o["composed_kernel_ms"], o["signed_kernel_ms"], o["kernel_speedup_composed"], o["signed_inversion_ms"],
                     o["unsigned_kernel_ms"], o["kernel_ratio_unsigned"], o["composed_wall_ms"], o["signed_wall_ms"],
                     o["wall_speedup_composed"], "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("signed and composed results differ")


if __name__ == "__main__":
    main()
