"""Encrypted segmented sum: the fused call against its two yardsticks, on the same key and the same resident inputs, in
the same process (tools/, a measurement; bench.py is the headline).  2048-bit key.

  fused     pgpu_batch_ct_segment_sum(x, ids, groups, n_segments)
  matvec    pgpu_batch_ct_matvec with the 0/1 matrix of the grouping and e_bits = 1 (what a caller could do before):
            groups * n_segments * cols pair products, almost all of them by one -- on the cases where the matrix fits
  ideal     ONE pgpu_batch_ct_add launch over as many elements as the call has products (elements - non-empty segments):
            every product useful, rows read in order -- measured on 2^20 elements and scaled by the product count

Cases: (a) 65536 samples x 16 groups x 32 bins, roughly uniform; (b) the same shape with 90 % of every group in one bin;
(c) 2^20 elements, 1 group, 1024 segments; (d) 4096 samples x 1 group x 32 bins (small enough for everything).
Results of the fused call and of the matvec route are downloaded and compared bit for bit.  Per case: HIP-event kernel
time (pgpu_set_timing: the sum over the launches; one launch per level) and wall time (host clock around the call, which
includes the host's sort and plan, ending in pgpu_synchronize), the plan (chunk, levels), the share of the executed
products that are padding (a chain past its own end multiplies by one until the longest chain of its wavefront is done),
and the product rate as a fraction of the ideal.  One warm-up, then --reps timed runs; the median is reported and all runs
printed.  --sweep repeats every case with PGPU_SEGSUM_CHUNK forced to each of 2 .. 512.

usage: python tools/bench_segsum.py [--reps 5] [--sweep] [--cases a,b,c,d] [--quick] [--out profiles/segsum_bench.txt]
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
import numpy as np

import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi

GOLD = os.path.join(ROOT, "tests", "golden")
KIND_SEGSUM, KIND_MATVEC = 6, 5
BITS, G = 2048, 4
IPW = 64 // G
NONE = 0xFFFFFFFF
SWEEP = [2, 4, 8, 16, 32, 64, 128, 256, 512]


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

    def measure(self, fn, reps, kind):
        _, _, h = self.timed(fn)                       # warm-up (code objects, arena blocks); its result is the one compared
        out = self.down(h)
        self.free(h)
        walls, kerns, launches = [], [], []
        for _ in range(reps):
            wall, rec, h = self.timed(fn)
            self.free(h)
            assert kind is None or all(k == kind for k, _ in rec), rec
            walls.append(wall)
            kerns.append(sum(ms for _, ms in rec))
            launches.append([round(ms, 3) for _, ms in rec])
        return out, {"wall_ms": statistics.median(walls), "kernel_ms": statistics.median(kerns),
                     "kernel_ms_all": [round(v, 3) for v in kerns], "launch_ms": launches[len(launches) // 2]}


def schedule_stats(seg_lens, chunk):
    """the plan of csrc/policy.cpp: segsum_plan restated on segment lengths: per level the chains, the executed products
    (64/G chains per wavefront -- half as many in the wide form of small levels --, all running to the wavefront's longest) and the useful ones"""
    levels = []
    lens = np.asarray(seg_lens, dtype=np.int64)
    while True:
        small, large = lens[lens <= chunk], lens[lens > chunk]
        rem = large % chunk
        chains = np.concatenate([small, np.full(int((large // chunk).sum()), chunk, dtype=np.int64), rem[rem > 0]])
        chains = np.sort(chains)[::-1]
        ipw = IPW // 2 if len(chains) <= (IPW // 2) * 1024 else IPW      # (csrc/policy.cpp: segsum_wide_pays, 2048-bit keys)
        pad = (-len(chains)) % ipw
        waves = np.concatenate([chains, np.full(pad, chains[-1], dtype=np.int64)]).reshape(-1, ipw)
        executed = int(np.maximum(waves[:, 0] - 1, 0).sum()) * ipw
        useful = int(np.maximum(chains - 1, 0).sum())
        levels.append({"chains": int(len(chains)), "wavefronts": int(len(waves)), "executed": executed, "useful": useful})
        if len(large) == 0:
            return levels
        lens = -(-large // chunk)


def random_rows(rng, count, nw):
    """`count` values below n^2 as rows of 2*nw words (any residue serves as a ciphertext for a product)"""
    a = rng.integers(0, 1 << 63, size=(count, 2 * nw), dtype=np.uint64)
    a[:, -1] &= np.uint64((1 << 40) - 1)
    return a


def make_ids(rng, case, cols, n_segments, groups):
    ids = rng.integers(0, n_segments, size=groups * cols, dtype=np.uint32)
    if case == "b":                                    # 90 % of every group in one bin
        ids[rng.random(groups * cols) < 0.9] = 0
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="repeat every case with every forced chunk of %s" % SWEEP)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segsum_bench.txt"))
    args = ap.parse_args()
    os.environ.pop("PGPU_SEGSUM_CHUNK", None)
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
    say("# box: %s | key %d bits | reps %d | times: median, ms" % (L.pgpu_device_name().decode(), BITS, args.reps))
    # the ideal: one CT + CT launch, every product useful, rows read in order
    _, ideal = B.measure(lambda: B.op(L.pgpu_batch_ct_add, pk._h, big, big), args.reps, None)
    ideal_per_product = ideal["kernel_ms"] / big_n
    say("ideal: pgpu_batch_ct_add of %d elements: kernel %.3f ms %s = %.3f ns per product"
        % (big_n, ideal["kernel_ms"], ideal["kernel_ms_all"], ideal_per_product * 1e6))
    shapes = {"a": (65536, 32, 16), "b": (65536, 32, 16), "c": (big_n, 1024, 1), "d": (4096, 32, 1)}
    if args.quick:
        shapes = {"a": (2048, 32, 4), "b": (2048, 32, 4), "c": (big_n, 64, 1), "d": (512, 8, 1)}
    matvec_cases = ("a", "b", "d")
    xs = {}
    ok = True
    for case in args.cases.split(","):
        cols, n_segments, groups = shapes[case]
        if cols not in xs:
            xs[cols] = big if cols == big_n else resident(cols)
        x = xs[cols]
        ids = make_ids(rng, case, cols, n_segments, groups)
        seg_lens = np.bincount((ids.astype(np.int64) + np.repeat(np.arange(groups), cols) * n_segments),
                               minlength=groups * n_segments)
        products = int(np.maximum(seg_lens - 1, 0).sum())

        def fused():
            return B.op(L.pgpu_batch_ct_segment_sum, pk._h, x, ptr(ids), groups, n_segments)

        def run_fused(forced=None):
            if forced is None:
                os.environ.pop("PGPU_SEGSUM_CHUNK", None)
            else:
                os.environ["PGPU_SEGSUM_CHUNK"] = str(forced)
            chunk, levels = ctypes.c_int(), ctypes.c_int()
            _capi.check(L.pgpu_ct_segment_sum_plan(BITS, int(seg_lens.sum()), groups * n_segments, int(seg_lens.max()),
                                                   ctypes.byref(chunk), ctypes.byref(levels)))
            out, t = B.measure(fused, args.reps, KIND_SEGSUM)
            os.environ.pop("PGPU_SEGSUM_CHUNK", None)
            st = schedule_stats(seg_lens, chunk.value)
            assert len(st) == levels.value == len(t["launch_ms"]), (len(st), levels.value, t["launch_ms"])
            executed = sum(s["executed"] for s in st)
            t.update({"chunk": chunk.value, "levels": levels.value, "executed_products": executed,
                      "padding_share": round(1 - products / max(1, executed), 4),
                      "level0_wavefronts": st[0]["wavefronts"],
                      "fold_ms": round(sum(t["launch_ms"][1:]), 3),
                      "frac_of_ideal": round(products * ideal_per_product / t["kernel_ms"], 3)})
            return out, t

        out, t = run_fused()
        o = {"case": case, "cols": cols, "n_segments": n_segments, "groups": groups, "elements": int(seg_lens.sum()),
             "products": products, "longest_segment": int(seg_lens.max()), "fused": t}
        say("(%s) %d x %d groups x %d segments | products %d, longest segment %d | chunk %d, levels %d, level-0 wavefronts %d | "
            "fused kernel %.3f ms (launches %s; folds %.3f) wall %.3f | padding %.1f %% of executed | %.3f of the ideal"
            % (case, cols, groups, n_segments, products, o["longest_segment"], t["chunk"], t["levels"], t["level0_wavefronts"],
               t["kernel_ms"], t["launch_ms"], t["fold_ms"], t["wall_ms"], 100 * t["padding_share"], t["frac_of_ideal"]))
        if case in matvec_cases:
            w = np.zeros((groups * n_segments, cols), dtype=np.uint64)
            w[ids.astype(np.int64) + np.repeat(np.arange(groups), cols) * n_segments, np.tile(np.arange(cols), groups)] = 1
            wb = B.up(w.reshape(-1, 1))
            del w
            mv_out, mv = B.measure(lambda: B.op(L.pgpu_batch_ct_matvec, pk._h, x, wb, groups * n_segments, 1), args.reps, KIND_MATVEC)
            B.free(wb)
            same = bool(np.array_equal(out, mv_out))
            ok = ok and same
            o["matvec"] = mv
            o["identical"] = same
            say("    matvec route (0/1 matrix, e_bits 1): kernel %.3f ms %s wall %.3f | fused is %.1f x faster (kernel), %.1f x (wall) | %s"
                % (mv["kernel_ms"], mv["kernel_ms_all"], mv["wall_ms"], mv["kernel_ms"] / t["kernel_ms"], mv["wall_ms"] / t["wall_ms"],
                   "identical" if same else "DIFFERENT"))
        if args.sweep:
            o["sweep"] = []
            for c in SWEEP:
                so, st = run_fused(c)
                same = bool(np.array_equal(out, so))
                ok = ok and same
                o["sweep"].append(st)
                say("    chunk %3d: levels %d, level-0 wavefronts %5d, kernel %.3f ms %s (folds %.3f), wall %.3f, padding %.1f %%, %.3f of the ideal%s"
                    % (c, st["levels"], st["level0_wavefronts"], st["kernel_ms"], st["kernel_ms_all"], st["fold_ms"], st["wall_ms"],
                       100 * st["padding_share"], st["frac_of_ideal"], "" if same else "  DIFFERENT"))
        say("JSON " + json.dumps(o))
    pa.terminate()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit("results differ")


if __name__ == "__main__":
    main()
