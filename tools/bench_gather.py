"""Gather, concat and slice of resident batches: the device-side re-indexing against what it is bounded by and against the
route a caller had before, 2048-bit key, one process (tools/, a measurement; bench.py is the headline).

  (a) a random permutation of 2^20 resident ciphertexts (576-byte pair rows) by pgpu_batch_gather, against a stream-ordered
      device-to-device copy of the same bytes (the same bytes read and written), both timed by HIP events
  (b) the same gather with the identity index and with all-equal indices
  (c) the use case: 1024 of 65536 resident vectors of 64 ciphertexts gathered, then pgpu_batch_ct_matmul 64 -> 16; against
      uploading the 1024 x 64 ciphertexts from pinned host memory followed by the same matmul (wall and kernel time)
  (d) CipherText::rotate(1) of 65536 resident ciphertexts at the ipcl:: API, on the device against the host path it took
      before (wall time; the API is C++: tools/bench_rotate.cpp, built and run as a child after the cases above)

Per figure: the median of --reps runs after one warm-up, with the spread.  Kernel times are pgpu_set_timing's HIP events
around the launch; wall times the host clock around the calls, ending in pgpu_synchronize.

usage: python tools/bench_gather.py [--reps 5] [--cases abcd] [--quick]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
KIND_GATHER, KIND_MATMUL = 15, 11
BITS = 2048


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Box:
    def __init__(self):
        pa.initialize(0)
        self.L = _capi.lib()
        k = json.load(open(os.path.join(GOLD, "iso_kat.json")))
        p, q, hs = int(k["p"], 16), int(k["q"], 16), int(k["bench_hs"], 16)
        self.n = p * q
        self.pk = pa.PublicKey(self.n, BITS, hs=hs)

    def op(self, fn, *a):
        h = ctypes.c_void_p()
        _capi.check(fn(*a, ctypes.byref(h)))
        return h

    def up(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        return self.op(self.L.pgpu_batch_upload, ptr(arr), arr.shape[0], arr.shape[1], arr.shape[1])

    def down(self, h):
        out = np.empty((self.L.pgpu_batch_count(h), self.L.pgpu_batch_words(h)), dtype=np.uint64)
        _capi.check(self.L.pgpu_batch_download(h, ptr(out)))
        return out

    def free(self, *hs):
        for h in hs:
            self.L.pgpu_batch_destroy(h)

    def sync(self):
        _capi.check(self.L.pgpu_synchronize())

    def encrypt(self, count, seed):
        rng = np.random.default_rng(seed)
        m = rng.integers(0, 1 << 63, size=(count, 1), dtype=np.uint64)
        r = rng.integers(0, 1 << 63, size=(count, 16), dtype=np.uint64)
        hm, hr = self.up(m), self.up(r)
        c = self.op(self.L.pgpu_batch_encrypt, self.pk._h, hm, hr, 1024)
        self.free(hm, hr)
        return c

    def repeated(self, h, times):
        """h put end to end `times` times: a large resident batch without as many encryptions"""
        arr = (ctypes.c_void_p * times)(*[h.value] * times)
        return self.op(self.L.pgpu_batch_concat, arr, times)

    def gather(self, h, idx):
        arr = (ctypes.c_void_p * 1)(h.value)
        return self.op(self.L.pgpu_batch_gather, arr, 1, ptr(idx), len(idx))

    def timed(self, fn):
        """-> (wall ms, {kind: ms summed over the launches}, result handle)"""
        L = self.L
        kinds, ms = (ctypes.c_int * 4096)(), (ctypes.c_double * 4096)()
        self.sync()
        L.pgpu_set_timing(1)
        L.pgpu_timing_collect(kinds, ms, 4096)
        t0 = time.perf_counter()
        h = fn()
        self.sync()
        wall = (time.perf_counter() - t0) * 1e3
        n = L.pgpu_timing_collect(kinds, ms, 4096)
        L.pgpu_set_timing(0)
        by = {}
        for i in range(n):
            by[kinds[i]] = by.get(kinds[i], 0.0) + ms[i]
        return wall, by, h


def med(xs):
    return "%.3f (%.3f-%.3f)" % (statistics.median(xs), min(xs), max(xs))


def plan_of(L, row_bytes, n_out):
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _capi.check(L.pgpu_batch_gather_plan(row_bytes, n_out, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return "%d lanes per row, %d rows per wavefront, %d-byte accesses" % (a.value, b.value, c.value)


def d2d_copy_ms(nbytes, reps):
    """a stream-ordered device-to-device copy of nbytes, HIP events around it (torch's stream and events)"""
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.random_(0, 256)
    out = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return out[1:]


def cases_ab(box, reps, count, base, do_b):
    L = box.L
    small = box.encrypt(base, 1)
    x = box.repeated(small, count // base)
    row_bytes = 4 * L.pgpu_batch_row_limbs(x)
    nbytes = count * row_bytes
    print("(a) %d resident ciphertexts, rows of %d bytes (%.1f MB read + as many written); plan: %s"
          % (count, row_bytes, nbytes / 1e6, plan_of(L, row_bytes, count)))
    copy = d2d_copy_ms(nbytes, reps)
    rng = np.random.default_rng(7)
    lists = [("random permutation", rng.permutation(count).astype(np.uint64))]
    if do_b:
        lists += [("identity", np.arange(count, dtype=np.uint64)), ("all equal", np.full(count, count // 3, dtype=np.uint64))]
    ref = box.down(small)
    for name, idx in lists:
        kern, wall = [], []
        for rep in range(reps + 1):
            w, by, y = box.timed(lambda: box.gather(x, idx))
            if rep == 0:                                     # the result, once: a sample of rows against the source
                part = box.op(L.pgpu_batch_slice, y, 0, min(count, 4096), 1)
                got = box.down(part)
                assert (got == ref[(idx[:len(got)] % base).astype(np.int64)]).all(), name
                box.free(part)
            else:
                kern.append(by.get(KIND_GATHER, 0.0))
                wall.append(w)
            box.free(y)
        k, c = statistics.median(kern), statistics.median(copy)
        print("    %-18s kernel %s ms = %.2f TB/s read + written; wall %s ms" % (name, med(kern), 2 * nbytes / k / 1e9, med(wall)))
        if name == "random permutation":
            print("    device-to-device copy of the same bytes: %s ms = %.2f TB/s; gather / copy byte rate %.2f (bar: at least 0.50)"
                  % (med(copy), 2 * nbytes / c / 1e9, c / k))
    box.free(small, x)


def case_c(box, reps, n_all, n_pick, cols, rows):
    L = box.L
    vec = box.encrypt(n_all, 2)
    x = box.repeated(vec, cols)                              # n_all * cols ciphertexts, read as [n_all][cols]
    rng = random.Random(3)
    w = box.up(np.array([[rng.getrandbits(32)] for _ in range(rows * cols)], dtype=np.uint64))
    pick = rng.sample(range(n_all), n_pick)
    idx = np.array([v * cols + j for v in pick for j in range(cols)], dtype=np.uint64)
    # the same minibatch on the host, in pinned memory
    part = box.down(vec)                                     # (row r of x is row r % n_all of vec)
    host = ctypes.c_void_p()
    words = part.shape[1]
    _capi.check(L.pgpu_host_alloc(len(idx) * words * 8, ctypes.byref(host)))
    pinned = np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_uint64)), shape=(len(idx), words))
    pinned[:] = part[(idx % n_all).astype(np.int64)]
    del part

    def matmul(h):
        return box.op(L.pgpu_batch_ct_matmul, box.pk._h, h, w, n_pick, rows, 32, 0)

    def via_gather():
        g = box.gather(x, idx)
        y = matmul(g)
        box.free(g)
        return y

    def via_upload():
        u = box.op(L.pgpu_batch_upload, host, len(idx), words, words)
        y = matmul(u)
        box.free(u)
        return y
    print("(c) %d of %d resident vectors of %d ciphertexts, then matmul %d -> %d" % (n_pick, n_all, cols, cols, rows))
    outs = {}
    for name, fn in (("gather + matmul", via_gather), ("pinned upload + matmul", via_upload)):
        wall, kern, gk = [], [], []
        for rep in range(reps + 1):
            wl, by, y = box.timed(fn)
            if rep == 0:
                outs[name] = box.down(y)
            else:
                wall.append(wl)
                kern.append(sum(by.values()))
                gk.append(by.get(KIND_GATHER, 0.0))
            box.free(y)
        print("    %-24s wall %s ms; kernels %s ms (gather %s ms)" % (name, med(wall), med(kern), med(gk)))
    assert (outs["gather + matmul"] == outs["pinned upload + matmul"]).all()
    print("    both routes download the same bits")
    L.pgpu_host_free(host)
    box.free(vec, x, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--quick", action="store_true", help="small shapes: a functional run of the tool")
    a = ap.parse_args()
    box = Box()
    print("device:", box.L.pgpu_device_name().decode())
    if "a" in a.cases or "b" in a.cases:
        cases_ab(box, a.reps, 1 << (12 if a.quick else 20), 1 << (8 if a.quick else 16), "b" in a.cases)
    if "c" in a.cases:
        case_c(box, a.reps, 256 if a.quick else 65536, 16 if a.quick else 1024, 8 if a.quick else 64, 4 if a.quick else 16)
    pa.terminate()
    if "d" in a.cases:
        case_d(a.reps, 256 if a.quick else 65536)


def case_d(reps, count):
    """rotate(1) at the ipcl:: API, which is C++: tools/bench_rotate.cpp, compiled here and run as a child once this
    process has let go of the GPU.  `resident` is rotate as it is now, `host path` the steps it took before for the same
    text (download, conversion, host rotation; the next operator uploads again)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "pailliercryptolib_amd")
    os.makedirs(os.path.join(root, "build"), exist_ok=True)
    exe = os.path.join(root, "build", "bench_rotate")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tools", "bench_rotate.cpp"), "-L" + lib, "-lipcl_amd", "-lpgpu", "-Wl,-rpath," + lib,
                    "-o", exe], check=True)
    print("(d)", end=" ", flush=True)
    subprocess.run([exe, str(count), str(reps)], check=True, timeout=600)


if __name__ == "__main__":
    main()
