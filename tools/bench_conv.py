"""Encrypted 2-D convolution: pgpu_batch_ct_conv2d against the one route a caller had before it, the pgpu_batch_ct_spmv
formulation ("a convolution as a banded matrix"), on the same key and the same resident x, alternated in the same process
(tools/, a measurement; bench.py is the headline).

  conv2d   pgpu_batch_ct_conv2d(x, w, shape): the C_out * C_in * kh * kw filter taps uploaded once
  spmv     pgpu_batch_ct_spmv over the same x: n_img * C_out * OH * OW CSR rows of the taps inside the image, column numbers
           ((n * C_in + ci) * H + iy) * W + ix, the weights replicated per output -- the host builds and uploads one column
           number and one weight per term, and the window table covers all of x

Shapes (2048-bit key, 32-bit weights), n_img x C_in x H x W -> C_out filters of kh x kw:
  (a) 1 x 1x28x28 -> 8 of 5x5: one pass      (b) 64 of those images      (c) 1024 of those images
  (d) 64 x 16x14x14 -> 16 of 3x3, padding 1: multi-channel

Per route: HIP-event kernel time (pgpu_set_timing: the sum over the launches of the call) and wall time -- host clock from
the caller's arrays (the filters; for spmv also the CSR build) to pgpu_synchronize after the call, the weight upload
included --, medians of --reps runs after one warm-up, the two routes alternating run by run, with the spread; the plans
and the pair products of both plan queries.  The results are downloaded and compared bit for bit.

--force W,T,S forces the plan of the conv2d route (the spmv route is untouched): a sweep is one run per plan.

usage: python tools/bench_conv.py [--reps 5] [--cases abcd] [--force W,T,S] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_matmul import BITS, E_BITS, Box, encrypt, key_of, ptr, summary  # noqa: E402

KIND_CONV, KIND_SPMV = 13, 9
KNOBS = ("PGPU_CONV_WINDOW", "PGPU_CONV_TILE", "PGPU_CONV_SLICES")
# n_img, C_in, H, W, C_out, kh, kw, stride_h, stride_w, pad_h, pad_w
SHAPES = {"a": (1, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0), "b": (64, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0),
          "c": (1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0), "d": (64, 16, 14, 14, 16, 3, 3, 1, 1, 1, 1)}
QUICK = {"a": (1, 1, 6, 6, 2, 3, 3, 1, 1, 0, 0), "b": (4, 1, 6, 6, 2, 3, 3, 1, 1, 0, 0), "c": (9, 1, 6, 6, 2, 3, 3, 1, 1, 0, 0),
         "d": (3, 2, 5, 4, 3, 3, 3, 2, 1, 1, 1)}


def csr_of(shape, w):
    """the spmv formulation: (row_ptr, col_idx, replicated weights) with the taps outside the image left out"""
    n_img, c_in, h, wd, c_out, kh, kw, sh, sw, ph, pw = shape
    oh, ow = (h + 2 * ph - kh) // sh + 1, (wd + 2 * pw - kw) // sw + 1
    elems, taps = c_in * h * wd, c_in * kh * kw
    ci, ky, kx = (g.reshape(-1) for g in np.meshgrid(np.arange(c_in), np.arange(kh), np.arange(kw), indexing="ij"))
    oy, ox = (g.reshape(-1) for g in np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij"))
    iy, ix = oy[:, None] * sh + ky[None, :] - ph, ox[:, None] * sw + kx[None, :] - pw          # [oh*ow][taps]
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < wd)
    elem = ((ci[None, :] * h + iy) * wd + ix)[inside]                                          # row-major: output by output, tap by tap
    tap = np.broadcast_to(np.arange(taps)[None, :], inside.shape)[inside]
    counts = np.tile(inside.sum(1), n_img * c_out)
    row_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    col_img = np.tile(elem, c_out)
    col_idx = (col_img[None, :] + (np.arange(n_img) * elems)[:, None]).reshape(-1).astype(np.uint32)
    w_img = np.concatenate([w[co * taps + tap] for co in range(c_out)])
    return row_ptr, col_idx, np.tile(w_img, (n_img, 1)), int(inside.sum(1).max())


def run_case(B, pk, case, shape, reps):
    L = B.L
    n_img, c_in, h, wd, c_out, kh, kw, sh, sw, ph, pw = shape
    oh, ow = (h + 2 * ph - kh) // sh + 1, (wd + 2 * pw - kw) // sw + 1
    n_out = n_img * c_out * oh * ow
    rng = np.random.default_rng(ord(case))
    x = encrypt(B, pk, rng, n_img * c_in * h * wd)
    w = rng.integers(0, 1 << E_BITS, size=(c_out * c_in * kh * kw, 1), dtype=np.uint64)
    cs = B.capi.Conv2dShape(*shape)
    pw_, ps, pt, ptb, ppr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    B.capi.check(L.pgpu_ct_conv2d_plan(BITS, ctypes.byref(cs), E_BITS, ctypes.byref(pw_), ctypes.byref(ps), ctypes.byref(pt),
                                       ctypes.byref(ptb), ctypes.byref(ppr)))
    row_ptr, col_idx, _, longest = csr_of(shape, w)
    nnz = int(row_ptr[-1])
    sw_, sc, sl, stb, spr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    B.capi.check(L.pgpu_ct_spmv_plan(BITS, n_out, n_img * c_in * h * wd, nnz, longest, E_BITS, ctypes.byref(sw_),
                                     ctypes.byref(sc), ctypes.byref(sl), ctypes.byref(stb), ctypes.byref(spr)))

    def conv():
        wb = B.up(w)
        hd = B.op(L.pgpu_batch_ct_conv2d, pk._h, x, wb, ctypes.byref(cs), E_BITS)
        B.free(wb)
        return hd

    def spmv():
        rp, ci, ws, _ = csr_of(shape, w)
        wb = B.up(ws)
        hd = B.op(L.pgpu_batch_ct_spmv, pk._h, x, ptr(rp), ptr(ci), wb, n_out, E_BITS)
        B.free(wb)
        return hd

    routes = {"conv2d": (conv, KIND_CONV), "spmv": (spmv, KIND_SPMV)}
    walls, kerns, launches = {k: [] for k in routes}, {k: [] for k in routes}, {}
    identical = None
    for name, (fn, _) in routes.items():                      # warm-up (code objects, arena blocks); its result is the one compared
        _, _, hd = B.timed(fn)
        got = B.down(hd)
        B.free(hd)
        if identical is None:
            first = got
            identical = True
        else:
            identical = bool(np.array_equal(first, got))
        del got
    del first
    for _ in range(reps):                                     # the two routes alternate
        for name, (fn, kind) in routes.items():
            wall, rec, hd = B.timed(fn)
            B.free(hd)
            assert all(k == kind for k, _ in rec), (name, rec[:8])
            walls[name].append(wall)
            kerns[name].append(sum(ms for _, ms in rec))
            launches[name] = len(rec)
    B.free(x)
    out = {"case": case, "key_bits": BITS, "e_bits": E_BITS, "shape": list(shape), "outputs": n_out, "nnz": nnz,
           "conv2d_plan": {"window": pw_.value, "slices": ps.value, "tile": pt.value, "passes": -(-n_img // pt.value),
                           "table_bytes": ptb.value, "products": ppr.value},
           "spmv_plan": {"window": sw_.value, "chunk": sc.value, "levels": sl.value, "table_bytes": stb.value, "products": spr.value},
           "product_ratio": round(spr.value / ppr.value, 3),
           "conv2d": summary(walls["conv2d"], kerns["conv2d"], launches["conv2d"]),
           "spmv": summary(walls["spmv"], kerns["spmv"], launches["spmv"]),
           "identical": identical}
    out["kernel_speedup"] = round(out["spmv"]["kernel_ms"] / out["conv2d"]["kernel_ms"], 3)
    out["wall_speedup"] = round(out["spmv"]["wall_ms"] / out["conv2d"]["wall_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--force", default="", help="W,T,S: force PGPU_CONV_WINDOW / _TILE / _SLICES for the run (0: leave to the policy)")
    args = ap.parse_args()
    for name in KNOBS + ("PGPU_SPMV_CHUNK", "PGPU_SPMV_WINDOW", "PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES"):
        os.environ.pop(name, None)
    if args.force:                                                 # (the knobs are read at every call, the plan query included)
        for name, v in zip(KNOBS, args.force.split(",")):
            if int(v) > 0:
                os.environ[name] = str(int(v))
    sys.path.insert(0, os.path.dirname(HERE))
    import pailliercryptolib_amd as pa
    from pailliercryptolib_amd import _capi
    B = Box(pa, _capi)
    p, q, hs = key_of()
    pk = pa.PublicKey(p * q, BITS, hs=hs)
    print("# box:", B.L.pgpu_device_name().decode(), "| key", BITS, "| e_bits", E_BITS, "| reps:", args.reps, "| times: median, ms")
    print("# case n_img x C_in x H x W -> C_out of kh x kw | conv2d plan w tile passes S table | spmv plan w table | products spmv / conv2d "
          "= ratio | kernel ms spmv / conv2d = speed-up | wall ms spmv / conv2d = speed-up | identical")
    ok = True
    for case in args.cases:
        o = run_case(B, pk, case, (QUICK if args.quick else SHAPES)[case], args.reps)
        ok = ok and o["identical"]
        cp, sp, s = o["conv2d_plan"], o["spmv_plan"], o["shape"]
        print("(%s) %4d x %dx%dx%d -> %d of %dx%d | w=%d t=%-4d p=%-4d S=%-3d %6.1f MB | w=%d %7.1f MB | %11d / %10d = %5.2f | "
              "%10.3f / %9.3f = %5.2f | %10.3f / %9.3f = %5.2f | %s"
              % (case, s[0], s[1], s[2], s[3], s[4], s[5], s[6], cp["window"], cp["tile"], cp["passes"], cp["slices"], cp["table_bytes"] / 1e6,
                 sp["window"], sp["table_bytes"] / 1e6, sp["products"], cp["products"], o["product_ratio"], o["spmv"]["kernel_ms"],
                 o["conv2d"]["kernel_ms"], o["kernel_speedup"], o["spmv"]["wall_ms"], o["conv2d"]["wall_ms"], o["wall_speedup"],
                 "identical" if o["identical"] else "DIFFERENT"), flush=True)
        print("    kernel ms, all runs: conv2d %s spmv %s | launches conv2d %d spmv %d"
              % (o["conv2d"]["kernel_ms_all"], o["spmv"]["kernel_ms_all"], o["conv2d"]["launches"], o["spmv"]["launches"]), flush=True)
        print("JSON " + json.dumps(o), flush=True)
    pa.terminate()
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
