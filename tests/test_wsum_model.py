"""The schedule of the encrypted weighted sum of K resident batches (csrc/hensel_wsum.hpp: wsum_kernel, driven by the plan
of csrc/policy.cpp: wsum_plan) restated in plain integers modulo a small n^2: one chain per element and slice, 64/G
elements per wavefront, the accumulator loaded from the slice's first operand, one squaring per SQR step and one product
per MUL step with the operand staged one MUL ahead (the row that `next` names, the row of one past the last MUL), idle
groups of the last wavefront that walk the last element and do not store, slice 0 writing the result batch and the
others a partial region each, the fold -- the same kernel over the regions with an all-MUL list -- in place.  The
schedule is the real one -- printed by the policy test binary, which is built from policy.cpp -- and the result is held
against pow.  In the reference such a sum is composed from CipherText::operator* (ipcl/ciphertext.cpp:83-106) and
operator+ (ciphertext.cpp:35-72)."""
import random
import shutil
import subprocess

import pytest

from test_wsum_policy import build_policy_binary, clean_env

N = 1009 * 1013
NSQ = N * N
SQR, NONE = 0xFFFFFFFF, 0xFFFFFFFE
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = build_policy_binary(tmp_path_factory.mktemp("wsum_model"))

    def plan(weights, n_terms, S):
        """-> None (refused), or (slices, totals): slices = [(term_begin, term_end, first, first_mul, [(op, next)])]"""
        if weights is None:
            text = f"{n_terms} 0 {S} 1\n"
        else:
            ww = max(1, (max(v.bit_length() for v in weights) + 63) // 64)
            words = [(v >> (64 * j)) & (2 ** 64 - 1) for v in weights for j in range(ww)]
            text = f"{n_terms} {ww} {S} 0\n" + " ".join(f"{v:x}" for v in words) + "\n"
        r = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, env=clean_env())
        assert r.returncode == 0, r.stdout
        lines = r.stdout.split("\n")
        if lines[0] == "refused":
            return None
        _, n_slices, longest, squarings, muls, products, all_zero = lines[0].split()
        at, slices = 1, []
        for _ in range(int(n_slices)):
            _, lo, hi, first, first_mul, n_steps = lines[at].split()
            steps = [tuple(int(v) for v in lines[at + 1 + t].split()) for t in range(int(n_steps))]
            slices.append((int(lo), int(hi), int(first), int(first_mul), steps))
            at += 1 + int(n_steps)
        return slices, dict(longest=int(longest), squarings=int(squarings), muls=int(muls), products=int(products),
                            all_zero=bool(int(all_zero)))
    return plan


def run_wsum_kernel(rows, slices, dst, count, ipw, stats):
    """wsum_kernel in integers: rows[term] a list of count values (the table of row bases), slices as the planner prints
    them, dst[j] the list slice j stores to"""
    for j, (_, _, first, first_mul, steps) in enumerate(slices):               # blockIdx.y
        for w0 in range(0, count, ipw):                                        # one wavefront
            for g in range(ipw):
                live = w0 + g < count
                i = w0 + g if live else count - 1                              # idle groups walk the last element
                row_of = lambda term: 1 if term == NONE else rows[term][i]     # noqa: E731 -- the row of one
                acc, staged = row_of(first), row_of(first_mul)
                for op, nxt in steps:
                    if op == SQR:
                        acc = acc * acc % NSQ
                        stats["squarings"] += live
                    else:
                        assert staged == row_of(op)                            # the staged row is the one this MUL names
                        coming = row_of(nxt)                                   # loaded before the product starts
                        acc = acc * staged % NSQ
                        staged = coming
                        stats["muls"] += live
                if live:
                    dst[j][i] = acc


def weighted_sum_model(planner, xs, weights, S, ipw):
    """the whole call as capi_aggregate.inc runs it: the slices' launch, then the fold over the regions, in place"""
    K, count = len(xs), len(xs[0])
    got = planner(weights, K, S)
    assert got is not None
    slices, totals = got
    stats = {"squarings": 0, "muls": 0, "launches": 1}
    out = [None] * count
    regions = [out] + [[None] * count for _ in slices[1:]]
    used = {t for _, _, first, _, steps in slices for t in [first] + [op for op, _ in steps if op != SQR]} - {NONE}
    rows = [x if k in used else None for k, x in enumerate(xs)]               # a batch of weight zero is never read
    run_wsum_kernel(rows, slices, regions, count, ipw, stats)
    if len(slices) > 1:
        fold, _ = planner(None, len(slices), 1)
        run_wsum_kernel(regions, fold, [out], count, ipw, stats)
        stats["launches"] = 2
    return out, stats, totals, slices


def expect(xs, weights):
    return [eval_row(xs, weights, i) for i in range(len(xs[0]))]


def eval_row(xs, weights, i):
    acc = 1
    for k, x in enumerate(xs):
        acc = acc * pow(x[i], 1 if weights is None else weights[k], NSQ) % NSQ
    return acc


def weight_sets(rng, K):
    e = 32
    sets = [
        [rng.getrandbits(e) for _ in range(K)],
        [0] * K,                                                               # all weights zero
        [1] * K,
        [(1 << e) - 1] * K,                                                    # 2^e - 1
        [1 << (e - 1)] * K,                                                    # a lone top bit
        [(0, 1, (1 << e) - 1, 1 << 63, rng.getrandbits(64) | (1 << 64), rng.getrandbits(99) | (1 << 99), N - 1)[k % 7] for k in range(K)],
        [N - 1] + [rng.getrandbits(20) for _ in range(K - 1)],
        [0] * (K // 2) + [rng.getrandbits(e) | 1 for _ in range(K - K // 2)],    # leading slices of zeros are dropped
        None,                                                                  # weights == NULL
    ]
    return sets


@pytest.mark.parametrize("K", [1, 2, 3, 5, 17])
def test_schedule_in_integers_matches_pow(planner, K):
    rng = random.Random(K)
    for count, ipw in ((1, 16), (5, 8), (37, 16), (70, 32)):
        xs = [[rng.randrange(1, NSQ) for _ in range(count)] for _ in range(K)]
        for weights in weight_sets(rng, K):
            want = expect(xs, weights)
            for S in sorted({1, 2, 3, K}):
                out, stats, totals, slices = weighted_sum_model(planner, xs, weights, S, ipw)
                assert out == want, (K, count, weights, S)
                # the counts of the formulas, per element, padding excluded
                w = [1] * K if weights is None else weights
                Sc = min(S, K)
                cuts = [w[s * K // Sc:(s + 1) * K // Sc] for s in range(Sc)]
                cuts = [c for c in cuts if any(c)]
                sq = sum(max(v.bit_length() for v in c) - 1 for c in cuts)
                mul = sum(sum(bin(v).count("1") for v in c) - 1 for c in cuts)
                fold = max(0, len(cuts) - 1)
                assert totals["squarings"] == sq and totals["muls"] == mul and totals["products"] == sq + mul + fold
                assert stats["squarings"] == count * sq and stats["muls"] == count * (mul + fold)
                assert len(slices) == max(1, len(cuts)) and stats["launches"] == (2 if len(cuts) > 1 else 1)
                assert totals["all_zero"] == (not cuts)


def test_the_issue_count(planner):
    """16 random 32-bit weights: (32 - 1) + (sum of popcounts - 1) pair products per element against 47 K - 1 composed"""
    rng = random.Random(16)
    w = [rng.getrandbits(32) | (1 << 31) for _ in range(16)]
    _, totals = planner(w, 16, 1)
    assert totals["products"] == 31 + sum(bin(v).count("1") for v in w) - 1
    assert 47 * 16 - 1 == 751 and 2.0 < 751 / totals["products"] < 3.4
