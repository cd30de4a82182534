"""The schedule of the encrypted segmented sum (csrc/hensel_segsum.hpp: segsum_kernel, driven by the plan of
csrc/policy.cpp: segsum_plan) restated in plain integers modulo a small n^2: one product chain per chunk descriptor,
64/G chains per wavefront with the wavefront's longest chunk as the trip count (a chain past its own end multiplies by
one), idle chains of the last wavefront that do not store, partial rows folded level by level with the identity
permutation, the last level of every segment written to its output row.  The plan is the real one -- printed by the
policy test binary, which is built from policy.cpp -- and the result is held against the direct product
prod_{j: ids[g][j] == s} x[j] for random, skewed and degenerate groupings.  In the reference such a sum is composed from
CipherText::operator+ (ipcl/ciphertext.cpp:35-72)."""
import random
import shutil
import subprocess

import pytest

from test_segsum_policy import build_policy_binary, clean_env

NONE = 0xFFFFFFFF
NSQ = (1009 * 1013) ** 2
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = build_policy_binary(tmp_path_factory.mktemp("segsum_model"))

    def plan(ids, groups, cols, n_segments, chunk):
        text = f"{groups} {cols} {n_segments} {chunk}\n" + " ".join(str(v) for v in ids) + "\n"
        r = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, env=clean_env())
        assert r.returncode == 0, r.stdout
        lines = r.stdout.split("\n")
        perm = [int(v) for v in lines[0].split()[1:]]
        levels, at = [], 2
        for _ in range(int(lines[1].split()[1])):
            _, n_chunks, partial_rows = lines[at].split()
            chunks = [tuple(int(v) for v in lines[at + 1 + i].split()) for i in range(int(n_chunks))]
            levels.append((chunks, int(partial_rows)))
            at += 1 + int(n_chunks)
        return perm, levels
    return plan


def run_kernel(src, perm, chunks, out, partial, ipw, stats):
    """segsum_kernel in integers: groups of ipw chains, a common trip count, products by one past a chain's end"""
    n = len(chunks)
    assert n >= 1
    for w0 in range(0, n, ipw):
        lanes = [min(w0 + g, n - 1) for g in range(ipw)]             # idle chains clamp to the last chunk
        longest = max(chunks[ci][1] for ci in lanes)
        for g, ci in enumerate(lanes):
            begin, length, dst, is_partial = chunks[ci]

            def row(t):
                if t >= length:
                    return 1
                return src[perm[begin + t] if perm is not None else begin + t]
            acc = row(0)
            for t in range(1, longest):
                acc = acc * row(t) % NSQ
                stats["products"] += 1
                stats["padding"] += t >= length or w0 + g >= n
            if w0 + g < n:
                (partial if is_partial else out)[dst] = acc


def segment_sum_model(planner, xs, ids, groups, n_segments, chunk, ipw=16):
    cols = len(xs)
    perm, levels = planner(ids, groups, cols, n_segments, chunk)
    out = [None] * (groups * n_segments)
    stats = {"products": 0, "padding": 0, "levels": len(levels)}
    src, pm = xs, perm
    for chunks, partial_rows in levels:
        partial = [None] * partial_rows
        run_kernel(src, pm, chunks, out, partial, ipw, stats)
        assert None not in partial
        src, pm = partial, None
    return out, stats


def direct(xs, ids, groups, n_segments):
    cols = len(xs)
    out = [1] * (groups * n_segments)
    for g in range(groups):
        for j in range(cols):
            s = ids[g * cols + j]
            if s != NONE:
                out[g * n_segments + s] = out[g * n_segments + s] * xs[j] % NSQ
    return out


def groupings(rng, cols, n_segments, groups):
    uniform = [rng.randrange(n_segments) for _ in range(groups * cols)]
    skewed = [0 if rng.random() < 0.9 else rng.randrange(n_segments) for _ in range(groups * cols)]   # 90 % in one segment
    holes = [NONE if rng.random() < 0.2 else rng.randrange(n_segments) // 2 * 2 % n_segments for _ in range(groups * cols)]
    return {"uniform": uniform, "skewed": skewed, "holes": holes, "all in 0": [0] * (groups * cols),
            "all NONE": [NONE] * (groups * cols), "one each": [j % n_segments for _ in range(groups) for j in range(cols)]}


@pytest.mark.parametrize("chunk", [2, 3, 8, 64])
@pytest.mark.parametrize("cols,n_segments,groups", [(1, 1, 1), (7, 3, 1), (33, 5, 2), (64, 64, 1), (65, 1, 1), (300, 9, 3), (37, 2, 1)])
def test_schedule_equals_direct_product(planner, chunk, cols, n_segments, groups):
    rng = random.Random(chunk * 1000 + cols)
    xs = [rng.randrange(1, NSQ) for _ in range(cols)]
    for name, ids in groupings(rng, cols, n_segments, groups).items():
        for ipw in (8, 16, 32):                                      # 3072-, 2048- and 1024-bit key classes
            got, stats = segment_sum_model(planner, xs, ids, groups, n_segments, chunk, ipw)
            assert got == direct(xs, ids, groups, n_segments), (name, ipw)
            longest = max([0] + [sum(1 for j in range(cols) if ids[g * cols + j] == s)
                                 for g in range(groups) for s in range(n_segments)])
            want_levels = 1
            while longest > chunk:
                longest = -(-longest // chunk)
                want_levels += 1
            assert stats["levels"] == want_levels, name


def test_level_boundaries_and_padding(planner):
    """a segment of exactly chunk, chunk + 1 and chunk^2 + 1 elements; the useful products are elements - segments"""
    rng = random.Random(5)
    for chunk in (2, 3, 8):
        for m in (chunk, chunk + 1, chunk * chunk, chunk * chunk + 1):
            cols = m + 3
            xs = [rng.randrange(1, NSQ) for _ in range(cols)]
            ids = [0] * m + [1, NONE, 1]
            got, stats = segment_sum_model(planner, xs, ids, 1, 3, chunk)
            assert got == direct(xs, ids, 1, 3) and got[2] == 1
            assert stats["products"] - stats["padding"] == (m - 1) + 1      # segment 0 and the two elements of segment 1
            levels = 1 if m <= chunk else 2 if m <= chunk * chunk else 3
            assert stats["levels"] == levels, (chunk, m)


def test_length_order_keeps_padding_small(planner):
    """ordered by length, the chains of a wavefront differ by little: on a skewed grouping the padded products stay a small
    share, where the segment order would pad every wavefront to its longest segment"""
    rng = random.Random(6)
    cols, n_segments = 4000, 40
    xs = [rng.randrange(1, NSQ) for _ in range(cols)]
    ids = [0 if rng.random() < 0.9 else rng.randrange(n_segments) for _ in range(cols)]
    got, stats = segment_sum_model(planner, xs, ids, 1, n_segments, 8)
    assert got == direct(xs, ids, 1, n_segments)
    assert stats["padding"] <= 0.25 * stats["products"], stats
