"""Signed-weight encrypted conv2d / spmv: the signed call against the two routes a caller has without it, on the same key
and the same resident x, in the same process (tools/, a measurement; bench.py is the headline).

  (a) signed     pgpu_batch_ct_conv2d_signed(x, W)                      (spmv shapes: pgpu_batch_ct_spmv_signed)
  (b) composed   pgpu_batch_ct_sub(conv2d(x, W+), conv2d(x, W-))        two unsigned calls over the same x and an inversion of
                                                                        the results: what a caller can do without (a)
  (c) unsigned   pgpu_batch_ct_conv2d(x, |W|)                           the same shape and e_bits: what the sign costs

(a) and (b) are downloaded in full, one after the other, and compared through their SHA-256 digests before any time is taken
(one result in host memory at a time: the 1024-image shape's are 2.4 GB each).  Per shape: HIP-event kernel time
(pgpu_set_timing: the sum over the launches of the route; for (a) the inversion's share -- kind PGPU_KERNEL_INVERT and the
conversions of its one host round trip -- is broken out) and wall time (host clock around the calls, ending in
pgpu_synchronize), and the pair products the plan queries report (the composed route: twice pgpu_ct_conv2d_plan /
pgpu_ct_spmv_plan, plus pgpu_ct_negate_plan over the outputs and one product per output for the subtraction's last walk).
One warm-up of each route, then --reps timed runs, the routes alternating; medians, the runs printed.  The bar ("Signed-weight conv2d and spmv"): kernel-time speed-up
over (b) of at least half the product ratio, for the shapes whose ratio is 2 or more.
--unsigned-only times (c) alone (the existing calls, for a comparison between two builds of the library).
--max-outputs N leaves out the shapes with more outputs.

usage: python tools/bench_conv_signed.py [--reps 5] [--quick] [--unsigned-only] [--max-outputs N]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pailliercryptolib_amd as pa
from bench_matvec_signed import BITS, E_BITS, GOLD, Box, ptr
from pailliercryptolib_amd import _capi

KIND_SPMV, KIND_CONV = 9, 13
# ("conv", (n_img, C_in, H, W, C_out, kh, kw, sh, sw, ph, pw)) | ("spmv", (rows, cols, entries per row or None, density))
SHAPES = [("conv", (1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0)), ("conv", (64, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0)),
          ("conv", (64, 16, 14, 14, 16, 3, 3, 1, 1, 1, 1)), ("conv", (1, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0)),
          ("spmv", (65536, 65536, 16, None)), ("spmv", (1024, 1024, None, 0.10))]
QUICK = [("conv", (3, 2, 7, 6, 4, 3, 3, 1, 1, 1, 1)), ("spmv", (64, 48, 5, None)), ("spmv", (32, 32, None, 0.25))]
UNSIGNED_ONLY = [("conv", (64, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0)), ("spmv", (65536, 65536, 16, None))]


def conv_case(B, pk, shape, rng):
    L = B.L
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    n_x, n_w = n_img * c_in * h * w, c_out * c_in * kh * kw
    n_out = n_img * c_out * ((h + 2 * ph - kh) // sh + 1) * ((w + 2 * pw - kw) // sw + 1)
    cs = _capi.Conv2dShape(*shape)

    def plan(fn):
        pw_, ps, pt, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        _capi.check(fn(BITS, ctypes.byref(cs), E_BITS, ctypes.byref(pw_), ctypes.byref(ps), ctypes.byref(pt), None, ctypes.byref(pr)))
        return {"window": pw_.value, "slices": ps.value, "tile": pt.value, "products": pr.value}
    return {"name": "conv2d %d x %dx%dx%d, %d of %dx%d" % (n_img, c_in, h, w, c_out, kh, kw), "n_x": n_x, "n_w": n_w, "n_out": n_out,
            "signed": lambda x, wb: B.op(L.pgpu_batch_ct_conv2d_signed, pk._h, x, wb, ctypes.byref(cs), E_BITS),
            "unsigned": lambda x, wb: B.op(L.pgpu_batch_ct_conv2d, pk._h, x, wb, ctypes.byref(cs), E_BITS),
            "plan_signed": lambda: plan(L.pgpu_ct_conv2d_signed_plan), "plan_unsigned": lambda: plan(L.pgpu_ct_conv2d_plan), "kind": KIND_CONV}


def spmv_case(B, pk, shape, rng):
    L = B.L
    rows, cols, per_row, density = shape
    if per_row:
        lens = np.full(rows, per_row, dtype=np.int64)
    else:
        lens = rng.binomial(cols, density, size=rows).astype(np.int64)
        lens[0] = max(lens[0], 1)
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, size=nnz, dtype=np.uint32)
    longest = int(lens.max())

    def plan(fn):
        pw_, pc, pl, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        _capi.check(fn(BITS, rows, cols, nnz, longest, E_BITS, ctypes.byref(pw_), ctypes.byref(pc), ctypes.byref(pl), None, ctypes.byref(pr)))
        return {"window": pw_.value, "chunk": pc.value, "levels": pl.value, "products": pr.value}
    return {"name": "spmv %d x %d, nnz %d" % (rows, cols, nnz), "n_x": cols, "n_w": nnz, "n_out": rows,
            "signed": lambda x, wb: B.op(L.pgpu_batch_ct_spmv_signed, pk._h, x, ptr(rp), ptr(ci), wb, rows, E_BITS),
            "unsigned": lambda x, wb: B.op(L.pgpu_batch_ct_spmv, pk._h, x, ptr(rp), ptr(ci), wb, rows, E_BITS),
            "plan_signed": lambda: plan(L.pgpu_ct_spmv_signed_plan), "plan_unsigned": lambda: plan(L.pgpu_ct_spmv_plan), "kind": KIND_SPMV}


def run_shape(B, pk, what, shape, reps, unsigned_only):
    L = B.L
    nw = BITS // 64
    rng = np.random.default_rng(sum(int(v or 0) for v in shape[:4]))
    case = (conv_case if what == "conv" else spmv_case)(B, pk, shape, rng)
    m = rng.integers(0, 1 << 62, size=(case["n_x"], nw), dtype=np.uint64)
    r = rng.integers(0, 1 << 62, size=(case["n_x"], nw // 2), dtype=np.uint64)
    bm, br = B.up(m), B.up(r)
    x = B.op(L.pgpu_batch_encrypt, pk._h, bm, br, 64 * (nw // 2))
    ws = rng.integers(-(1 << 31), 1 << 31, size=(case["n_w"], 1), dtype=np.int64)        # uniformly random signed 32-bit weights
    w_signed = B.up(ws.view(np.uint64))
    w_pos, w_neg, w_abs = B.up(np.maximum(ws, 0).astype(np.uint64)), B.up(np.maximum(-ws, 0).astype(np.uint64)), \
        B.up((np.abs(ws) & 0xFFFFFFFF).astype(np.uint64))
    n_out = case["n_out"]

    def composed():
        yp, yn = case["unsigned"](x, w_pos), case["unsigned"](x, w_neg)
        y = B.op(L.pgpu_batch_ct_sub, pk._h, yp, yn)
        B.free(yp, yn)
        return y

    unsigned = ("unsigned", lambda: case["unsigned"](x, w_abs))
    routes = [unsigned] if unsigned_only else [("signed", lambda: case["signed"](x, w_signed)), ("composed", composed), unsigned]
    res, outs = {}, {}
    for name, fn in routes:
        _, _, h = B.timed(fn)                      # warm-up (code objects, arena blocks); its result is the one compared
        if name != "unsigned":
            full = B.down(h)                       # the whole result; only its digest is kept
            outs[name] = (full.shape, hashlib.sha256(full).digest())
            del full
        B.free(h)
    identical = unsigned_only or outs["signed"] == outs["composed"]
    for _ in range(reps):                          # the routes alternate
        for name, fn in routes:
            wall, rec, h = B.timed(fn)
            B.free(h)
            d = res.setdefault(name, {"wall": [], "kernel": [], "own": [], "launches": len(rec)})
            d["wall"].append(wall)
            d["kernel"].append(sum(ms for _, ms in rec))
            d["own"].append(sum(ms for k, ms in rec if k == case["kind"]))
    med = {name: {k: statistics.median(v) for k, v in d.items() if isinstance(v, list)} for name, d in res.items()}
    up = case["plan_unsigned"]()
    out = {"shape": case["name"], "e_bits": E_BITS, "key_bits": BITS, "unsigned_plan": up,
           "unsigned_kernel_ms": round(med["unsigned"]["kernel"], 3), "unsigned_wall_ms": round(med["unsigned"]["wall"], 3),
           "unsigned_kernel_ms_all": [round(v, 3) for v in res["unsigned"]["kernel"]]}
    if not unsigned_only:
        sp = case["plan_signed"]()
        inv = ctypes.c_size_t()
        _capi.check(L.pgpu_ct_negate_plan(BITS, n_out, None, None, None, ctypes.byref(inv)))
        cp = 2 * up["products"] + inv.value + n_out           # two unsigned calls, the inversion of the outputs, a[i] multiplied in
        out.update({"signed_plan": sp, "identical": identical, "composed_products": cp,
                    "product_ratio_composed": round(cp / sp["products"], 3), "product_ratio_unsigned": round(sp["products"] / up["products"], 4),
                    "signed_kernel_ms": round(med["signed"]["kernel"], 3), "signed_wall_ms": round(med["signed"]["wall"], 3),
                    "signed_inversion_ms": round(med["signed"]["kernel"] - med["signed"]["own"], 3),
                    "signed_launches": res["signed"]["launches"], "composed_launches": res["composed"]["launches"],
                    "composed_kernel_ms": round(med["composed"]["kernel"], 3), "composed_wall_ms": round(med["composed"]["wall"], 3),
                    "kernel_speedup_composed": round(med["composed"]["kernel"] / med["signed"]["kernel"], 3),
                    "wall_speedup_composed": round(med["composed"]["wall"] / med["signed"]["wall"], 3),
                    "kernel_ratio_unsigned": round(med["signed"]["kernel"] / med["unsigned"]["kernel"], 3),
                    "signed_kernel_ms_all": [round(v, 3) for v in res["signed"]["kernel"]],
                    "composed_kernel_ms_all": [round(v, 3) for v in res["composed"]["kernel"]]})
        ratio, speed = cp / sp["products"], med["composed"]["kernel"] / med["signed"]["kernel"]      # unrounded
        out["bar"] = ("met" if speed >= ratio / 2 else "MISSED") if ratio >= 2 else "reported only (ratio below 2)"
    B.free(bm, br, x, w_signed, w_pos, w_neg, w_abs)
    return out


def outputs_of(what, shape):
    if what == "spmv":
        return shape[0]
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    return n_img * c_out * ((h + 2 * ph - kh) // sh + 1) * ((w + 2 * pw - kw) // sw + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--unsigned-only", action="store_true", help="the existing unsigned calls alone, at two shapes")
    ap.add_argument("--max-outputs", type=int, default=0, help="leave out shapes with more outputs (0: none)")
    args = ap.parse_args()
    B = Box()
    k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
    pk = pa.PublicKey(int(k["p"], 16) * int(k["q"], 16), BITS, hs=int(k["bench_hs"], 16))
    print("# box:", B.L.pgpu_device_name().decode(), "| key", BITS, "| e_bits", E_BITS, "| reps:", args.reps, "| times: median, ms")
    shapes = UNSIGNED_ONLY if args.unsigned_only else QUICK if args.quick else SHAPES
    ok = True
    for what, shape in shapes:
        if args.max_outputs and outputs_of(what, shape) > args.max_outputs:
            print("# left out (more than %d outputs): %s %s" % (args.max_outputs, what, shape), flush=True)
            continue
        o = run_shape(B, pk, what, shape, args.reps, args.unsigned_only)
        if args.unsigned_only:
            print("%-40s | unsigned kernel %9.3f ms, wall %9.3f ms | runs %s" % (o["shape"], o["unsigned_kernel_ms"], o["unsigned_wall_ms"],
                                                                               o["unsigned_kernel_ms_all"]), flush=True)
        else:
            ok = ok and o["identical"]
            print("%-40s | plan %s | products composed / signed = %.2f, signed / unsigned = %.4f | kernel ms composed %.3f / "
                  "signed %.3f = %.2f (inversion %.3f), unsigned %.3f: signed / unsigned = %.3f | wall ms composed %.3f / signed %.3f = %.2f "
                  "| bar: %s | %s"
                  % (o["shape"], o["signed_plan"], o["product_ratio_composed"], o["product_ratio_unsigned"],
                     o["composed_kernel_ms"], o["signed_kernel_ms"], o["kernel_speedup_composed"], o["signed_inversion_ms"],
                     o["unsigned_kernel_ms"], o["kernel_ratio_unsigned"], o["composed_wall_ms"], o["signed_wall_ms"],
                     o["wall_speedup_composed"], o["bar"], "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("signed and composed results differ")


if __name__ == "__main__":
    main()
