"""The schedule of the encrypted segmented prefix sum (csrc/hensel_segscan.hpp: segscan_kernel, and segsum_kernel for the
up-sweep, driven by the plan of csrc/policy.cpp: segscan_plan) restated in plain integers modulo a small n^2: one product
chain per descriptor, 64/G chains per wavefront with the most products of any chain of the wavefront as the trip count (a
chain past its own end multiplies by one and stores nothing), idle chains of the last wavefront that do not store, a
chain that starts from its carry row or -- without one -- as its first entry, stored unchanged, the step of +1 or -1,
the totals of every chunk but the last of a row scanned by the same procedure.  The plan is the real one -- printed by
the policy test binary, which is built from policy.cpp -- and the result is held against the direct prefix and suffix
products.  In the reference such a running sum is composed from CipherText::operator+ (ipcl/ciphertext.cpp:35-72)."""
import random
import shutil
import subprocess

import pytest

from test_segscan_policy import build_policy_binary, clean_env

NSQ = (1009 * 1013) ** 2
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = build_policy_binary(tmp_path_factory.mktemp("segscan_model"))

    def plan(rows, seg_len, chunk, reverse):
        r = subprocess.run([exe, "plan"], input=f"{rows} {seg_len} {chunk} {int(reverse)}\n", capture_output=True, text=True,
                           env=clean_env())
        assert r.returncode == 0, r.stdout
        lines = r.stdout.split("\n")
        head = lines[0].split()
        levels, at = [], 1
        for _ in range(int(head[1])):
            lrows, m, rev, n_up, totals, n_scan = (int(v) for v in lines[at].split()[1:])
            up = [tuple(int(v) for v in lines[at + 1 + i].split()) for i in range(n_up)]
            scan = [tuple(int(v) for v in lines[at + 1 + n_up + i].split()) for i in range(n_scan)]
            levels.append({"rows": lrows, "seg_len": m, "step": -1 if rev else 1, "up": up, "totals": totals, "scan": scan})
            at += 1 + n_up + n_scan
        return levels, int(head[3])
    return plan


def run_segsum(src, chunks, partial, ipw, stats):
    """segsum_kernel with perm == null: the chunk totals"""
    n = len(chunks)
    for w0 in range(0, n, ipw):
        lanes = [min(w0 + g, n - 1) for g in range(ipw)]
        longest = max(chunks[ci][1] for ci in lanes)
        for g, ci in enumerate(lanes):
            begin, length, dst = chunks[ci]
            acc = src[begin]
            for t in range(1, longest):
                acc = acc * (src[begin + t] if t < length else 1) % NSQ
                stats["products"] += 1
                stats["padding"] += t >= length or w0 + g >= n
            if w0 + g < n:
                assert partial[dst] is None
                partial[dst] = acc


def run_segscan(src, carry, chunks, out, step, ipw, stats):
    """segscan_kernel in integers"""
    n = len(chunks)
    assert n >= 1
    for w0 in range(0, n, ipw):
        lanes = [min(w0 + g, n - 1) for g in range(ipw)]             # idle chains clamp to the last descriptor
        longest = max(chunks[ci][1] - (chunks[ci][2] < 0) for ci in lanes)
        for g, ci in enumerate(lanes):
            begin, length, cr = chunks[ci]
            live = w0 + g < n
            first = 0 if cr >= 0 else 1
            acc = carry[cr] if cr >= 0 else src[begin]
            assert acc is not None
            if cr < 0 and live:
                assert out[begin] is None
                out[begin] = acc
            for i in range(longest):
                t = first + i
                acc = acc * (src[begin + step * t] if t < length else 1) % NSQ
                stats["products"] += 1
                stats["padding"] += t >= length or not live
                if t < length and live:
                    assert 0 <= begin + step * t < len(out) and out[begin + step * t] is None   # every row once
                    out[begin + step * t] = acc


def segment_scan_model(planner, xs, rows, seg_len, chunk, reverse, ipw=16):
    levels, products = planner(rows, seg_len, chunk, reverse)
    stats = {"products": 0, "padding": 0, "levels": len(levels), "plan_products": products, "launches": 0}
    ins = [xs]
    for lv in levels[:-1]:
        totals = [None] * lv["totals"]
        run_segsum(ins[-1], lv["up"], totals, ipw, stats)
        stats["launches"] += 1
        assert None not in totals
        ins.append(totals)
    res = None
    for lv, src in zip(reversed(levels), reversed(ins)):
        out = [None] * len(src)
        run_segscan(src, res, lv["scan"], out, lv["step"], ipw, stats)
        stats["launches"] += 1
        assert None not in out
        res = out
    return res, stats


def direct(xs, rows, seg_len, reverse):
    out = [None] * len(xs)
    for r in range(rows):
        acc = 1
        order = range(seg_len - 1, -1, -1) if reverse else range(seg_len)
        for t in order:
            acc = acc * xs[r * seg_len + t] % NSQ
            out[r * seg_len + t] = acc
    return out


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("chunk", [2, 3, 8])
def test_schedule_equals_direct_scan(planner, chunk, reverse):
    rng = random.Random(chunk * 10 + reverse)
    for rows in (1, 3, 17):
        for m in (1, 2, chunk - 1, chunk, chunk + 1, chunk * chunk, chunk * chunk + 1, chunk ** 3 + 1):
            xs = [rng.randrange(1, NSQ) for _ in range(rows * m)]
            want = direct(xs, rows, m, reverse)
            for ipw in (8, 16, 32):                                  # 3072-, 2048- and 1024-bit key classes
                got, stats = segment_scan_model(planner, xs, rows, m, chunk, reverse, ipw)
                assert got == want, (rows, m, ipw)
                assert stats["products"] - stats["padding"] == stats["plan_products"], (rows, m, ipw)
                assert stats["launches"] == 2 * stats["levels"] - 1
                if m <= chunk:
                    assert stats["levels"] == 1 and stats["plan_products"] == rows * (m - 1)


@pytest.mark.parametrize("rows,seg_len", [(1, 1), (1, 2), (3, 7), (5, 32), (17, 5), (1, 65), (2, 300)])
def test_shapes_of_the_gpu_tests(planner, rows, seg_len):
    rng = random.Random(rows * 1000 + seg_len)
    xs = [rng.randrange(1, NSQ) for _ in range(rows * seg_len)]
    for chunk in (8, 64, 300):
        for reverse in (False, True):
            got, stats = segment_scan_model(planner, xs, rows, seg_len, chunk, reverse)
            assert got == direct(xs, rows, seg_len, reverse)
            assert stats["products"] - stats["padding"] == stats["plan_products"]
            assert stats["levels"] == (1 if seg_len <= chunk else 2 if -(-seg_len // chunk) - 1 <= chunk else 3)
