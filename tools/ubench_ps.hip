// Microbenchmark (tools/, diagnostics only; round 6): the pair squaring / pair product of csrc/hensel_ps.hpp exactly as
// hensel_decrypt_ps_kernel runs them -- 5 squarings + 1 general product per window, 205 windows = one 1024-bit exponentiation
// of the 2048-bit key class -- with the SHADER clock read inside the kernel: every wavefront brackets its loop with s_memtime
// (tick = one shader cycle, MI355X_MICROARCH.md), so that cycles per instruction and the clock the chip held are two separate
// numbers:   cycles/instr = s_memtime span / instructions of the loop;   clock = s_memtime span / wall time of the launch.
// Round 5's version printed "cycles at 2.4 GHz" computed from WALL time, which cannot tell cadence from clock.
// Instructions per window: counted by tools/count_loop_instr.py on this file's code object and passed as argv[1] / argv[2]
// (unsigned form, two- / one-wavefront build) and argv[3] / argv[4] (balanced form); defaults below.
// Third part (the 6-bit window and the doubled operand of the balanced pair squaring): exp_kernel_bal runs the operation sequence
// of ONE whole exponentiation -- table build, then nwin - 1 windows of w squarings + 1 product -- in four forms from this one
// binary: the parent's (30 chained products, 204 x (5 + 1)), the half-squared table at w = 5 (15 x (1 + 1), 204 x (5 + 1)) and at
// w = 6 (31 x (1 + 1), 170 x (6 + 1)), each with psb_pairsqr<K, LB, false> and <K, LB, true>; and 1020 squarings alone in both.
// Fourth part (the odd-power window table): exp_kernel_bal<..., ODD = true> runs the decrypt kernel's odd form next to the parent's
// in this binary -- one squaring and `build` products, then nwin windows (the top one of `half` squarings) of w squarings and one
// product that stands after w - ctz(digit) of them, the digits a fixed pseudo-random sequence in SGPRs, the loop shape that of
// hensel_decrypt_psb_kernel (one body of each operation, wave-uniform branches).
// Fifth part (the Karatsuba split of the single products): exp_kernel_bal<..., KARA = true> runs psb_pairsqr / psb_pairmul with the
// a2*b and a*c products split in the middle next to the schoolbook form, the odd-table loop shape, the parent's form first and last.
// Sixth part (the folded reductions, hensel_ps_bal.hpp KRED): exp_kernel_bal<..., KRED = true> folds the upper q*n columns of the
// reductions of a2*b and a*c, next to the parent's form (KARA alone) in the same binary; `ubench_ps r` runs this part alone.
// Reported in shader cycles per exponentiation (no instruction count needed).
// build: python tools/build_ubench.py ubench_ps -I<repo>/pailliercryptolib_amd/csrc [-DPGPU_PS_SPLIT=1]   (the library's compile step, alignment pass included)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "hensel_ps_bal.hpp"
using namespace pgpu;

template <int K, int LB, int MINW>
__global__ __launch_bounds__(256, MINW) void sq_kernel(const uint32_t* in, const uint32_t* nn, uint32_t* out, unsigned long long* cyc,
                                                       int iters, int side) {
  extern __shared__ uint32_t claim[];
  __shared__ uint4 park_[kWavesPerWG][(K + 3) / 4][kWave];
  uint32_t a[K], b[K], n[K], c[K], d[K];
  const int lane = threadIdx.x + blockIdx.x * 256;
  uint4* slot = &park_[threadIdx.x / kWave][0][threadIdx.x % kWave];
  const uint32_t* np = nn + __builtin_amdgcn_readfirstlane(side) * K;
  __builtin_amdgcn_s_setprio(3);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    a[j] = in[(size_t)lane * 2 * K + j];
    b[j] = in[(size_t)lane * 2 * K + K + j];
    n[j] = ps_uniform(np[j]);
  }
  const uint32_t n1p = n[1] + 1;
  const unsigned long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int w = 0; w < iters; ++w) {
#pragma unroll 1
    for (int i = 0; i < 5; ++i) ps_pairsqr<K, LB>(a, b, n, n1p);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      c[j] = in[(size_t)lane * 2 * K + j] ^ (w & 1);
      d[j] = in[(size_t)lane * 2 * K + K + j] ^ (w & 2);
    }
    ps_pairmul<K, LB, true>(a, b, c, d, n, n1p, 0, slot);
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  if (threadIdx.x % kWave == 0) cyc[lane / kWave] = t1 - t0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    out[(size_t)lane * 2 * K + j] = a[j];
    out[(size_t)lane * 2 * K + K + j] = b[j];
  }
}

// the same window on BALANCED limbs (csrc/hensel_ps_bal.hpp: K = 36 limbs of 29 bits carry the prime the unsigned form gives
// 38 limbs of 28): nn holds the balanced limbs of the modulus, n0inv = -n^-1 mod 2^LB
template <int K, int LB, int MINW>
__global__ __launch_bounds__(256, MINW) void sq_kernel_bal(const uint32_t* in, const uint32_t* nn, uint32_t* out,
                                                           unsigned long long* cyc, int iters, uint32_t n0inv_in) {
  extern __shared__ uint32_t claim[];
  __shared__ uint4 park_[kWavesPerWG][(K + 3) / 4][kWave];
  int32_t a[K], b[K], n[K], c[K], d[K];
  const int lane = threadIdx.x + blockIdx.x * 256;
  uint4* slot = &park_[threadIdx.x / kWave][0][threadIdx.x % kWave];
  __builtin_amdgcn_s_setprio(3);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    a[j] = (int32_t)in[(size_t)lane * 2 * K + j];
    b[j] = (int32_t)in[(size_t)lane * 2 * K + K + j];
    n[j] = (int32_t)ps_uniform(nn[j]);
  }
  const uint32_t n0inv = ps_uniform(n0inv_in);
  int32_t dn[K / 2];
#pragma unroll
  for (int j = 0; j < K / 2; ++j) dn[j] = (int32_t)ps_uniform((uint32_t)(n[K / 2 + j] - n[j]));
  const unsigned long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int w = 0; w < iters; ++w) {
#pragma unroll 1
    for (int i = 0; i < 5; ++i) psb_pairsqr<K, LB>(a, b, n, dn, n0inv);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      c[j] = (int32_t)(in[(size_t)lane * 2 * K + j] ^ (w & 1));
      d[j] = (int32_t)(in[(size_t)lane * 2 * K + K + j] ^ (w & 2));
    }
    psb_pairmul<K, LB>(a, b, c, d, n, dn, n0inv, slot);
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  if (threadIdx.x % kWave == 0) cyc[lane / kWave] = t1 - t0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    out[(size_t)lane * 2 * K + j] = (uint32_t)a[j];
    out[(size_t)lane * 2 * K + K + j] = (uint32_t)b[j];
  }
}

// one exponentiation's operations on balanced limbs: `build` times ([a squaring if half] + a product), then `nwin` times
// (w squarings + [a product if do_mul]); DBL: the pair squaring on the doubled operand; KRED: the reductions of a2*b and a*c folded
template <int K, int LB, int MINW, bool DBL, bool ODD = false, bool KARA = false, bool KRED = false>
__global__ __launch_bounds__(256, MINW) void exp_kernel_bal(const uint32_t* in, const uint32_t* nn, uint32_t* out,
                                                            unsigned long long* cyc, uint32_t n0inv_in, int build, int half,
                                                            int nwin, int w, int do_mul) {
  extern __shared__ uint32_t claim[];
  __shared__ uint4 park_[kWavesPerWG][(K + 3) / 4][kWave];
  int32_t a[K], b[K], n[K], c[K], d[K];
  const int lane = threadIdx.x + blockIdx.x * 256;
  uint4* slot = &park_[threadIdx.x / kWave][0][threadIdx.x % kWave];
  __builtin_amdgcn_s_setprio(3);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    a[j] = (int32_t)in[(size_t)lane * 2 * K + j];
    b[j] = (int32_t)in[(size_t)lane * 2 * K + K + j];
    n[j] = (int32_t)ps_uniform(nn[j]);
  }
  const uint32_t n0inv = ps_uniform(n0inv_in);
  int32_t dn[K / 2];
#pragma unroll
  for (int j = 0; j < K / 2; ++j) dn[j] = KRED ? (int32_t)ps_uniform((uint32_t)(n[K / 2 + j] - n[j])) : 0;
  const unsigned long long t0 = __builtin_readcyclecounter();
  if constexpr (ODD) {
    // `half` holds the squarings of the top window here.  Table: trip 0 squares, trips 1 .. build multiply
#pragma unroll 1
    for (int e = 0; e <= build; ++e) {
      if (e == 0) psb_pairsqr<K, LB, DBL, KARA, KRED>(a, b, n, dn, n0inv);
      __builtin_amdgcn_sched_barrier(0);
      if (e > 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          c[j] = (int32_t)(in[(size_t)lane * 2 * K + j] ^ (e & 1));
          d[j] = (int32_t)(in[(size_t)lane * 2 * K + K + j] ^ (e & 2));
        }
        psb_pairmul<K, LB, KARA, KRED>(a, b, c, d, n, dn, n0inv, slot);
      }
    }
#pragma unroll 1
    for (int wi = 0; wi < nwin; ++wi) {
      const int wl = wi == 0 ? half : w;
      const int dg = (int)(((unsigned)wi * 2654435761u) >> 7) & ((1 << wl) - 1);     // digits 0 .. 2^wl - 1, every ctz
      int pos, idx;
      ps_window_place(dg, wl, true, pos, idx);
#pragma unroll 1
      for (int i = 0; i <= wl; ++i) {
        if (i == pos) {
#pragma unroll
          for (int j = 0; j < K; ++j) {
            c[j] = (int32_t)(in[(size_t)lane * 2 * K + j] ^ (idx & 1));
            d[j] = (int32_t)(in[(size_t)lane * 2 * K + K + j] ^ (idx & 2));
          }
          psb_pairmul<K, LB, KARA, KRED>(a, b, c, d, n, dn, n0inv, slot);
        }
        if (i < wl) psb_pairsqr<K, LB, DBL, KARA, KRED>(a, b, n, dn, n0inv);
      }
    }
  } else {
#pragma unroll 1
  for (int e = 0; e < build; ++e) {
    if (half) psb_pairsqr<K, LB, DBL, KARA, KRED>(a, b, n, dn, n0inv);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      c[j] = (int32_t)(in[(size_t)lane * 2 * K + j] ^ (e & 1));
      d[j] = (int32_t)(in[(size_t)lane * 2 * K + K + j] ^ (e & 2));
    }
    psb_pairmul<K, LB, KARA, KRED>(a, b, c, d, n, dn, n0inv, slot);
  }
#pragma unroll 1
  for (int wi = 0; wi < nwin; ++wi) {
#pragma unroll 1
    for (int i = 0; i < w; ++i) psb_pairsqr<K, LB, DBL, KARA, KRED>(a, b, n, dn, n0inv);
    if (do_mul) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        c[j] = (int32_t)(in[(size_t)lane * 2 * K + j] ^ (wi & 1));
        d[j] = (int32_t)(in[(size_t)lane * 2 * K + K + j] ^ (wi & 2));
      }
      psb_pairmul<K, LB, KARA, KRED>(a, b, c, d, n, dn, n0inv, slot);
    }
  }
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  if (threadIdx.x % kWave == 0) cyc[lane / kWave] = t1 - t0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    out[(size_t)lane * 2 * K + j] = (uint32_t)a[j];
    out[(size_t)lane * 2 * K + K + j] = (uint32_t)b[j];
  }
}

template <int K, int LB, bool DBL, bool ODD = false, bool KARA = false, bool KRED = false>
void run_exp(const char* name, int blocks, unsigned lds, int build, int half, int nwin, int w, int do_mul) {
  const size_t lanes = (size_t)blocks * 256, waves = lanes / 64;
  std::vector<uint32_t> h(lanes * 2 * K), hn(K);
  srand(1);
  for (auto& v : h) v = (uint32_t)((int32_t)((((uint32_t)rand() * 2654435761u) & ((1u << LB) - 1)) >> 1) - (1 << (LB - 2)));
  for (auto& v : hn) v = (uint32_t)((int32_t)((((uint32_t)rand() * 2654435761u) & ((1u << LB) - 1)) >> 1) - (1 << (LB - 2)));
  hn[0] |= 1u;
  hn[K - 1] = 1u << (LB - 10);
  uint32_t inv = 1;
  for (int i = 0; i < 5; ++i) inv *= 2u - hn[0] * inv;
  const uint32_t n0inv = (0u - inv) & ((1u << LB) - 1);
  uint32_t *din, *dn, *dout;
  unsigned long long* dcyc;
  hipMalloc(&din, h.size() * 4); hipMalloc(&dn, hn.size() * 4); hipMalloc(&dout, h.size() * 4); hipMalloc(&dcyc, waves * 8);
  hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(dn, hn.data(), hn.size() * 4, hipMemcpyHostToDevice);
  if (lds) hipFuncSetAttribute((const void*)exp_kernel_bal<K, LB, 1, DBL, ODD, KARA, KRED>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  std::vector<unsigned long long> cyc(waves);
  for (int rep = 0; rep < 4; ++rep) {
    hipEventRecord(e0);
    hipLaunchKernelGGL((exp_kernel_bal<K, LB, 1, DBL, ODD, KARA, KRED>), dim3(blocks), dim3(256), lds, 0, din, dn, dout, dcyc, n0inv, build, half, nwin, w, do_mul);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipMemcpy(cyc.data(), dcyc, waves * 8, hipMemcpyDeviceToHost);
    std::sort(cyc.begin(), cyc.end());
    double mean = 0;
    for (auto v : cyc) mean += (double)v;
    mean /= waves;
    const int sq = ODD ? 1 + (nwin - 1) * w + half : (half ? build : 0) + nwin * w, mul = build + (do_mul ? nwin : 0);
    if (rep) printf("%-52s doubled=%d karatsuba=%d folded=%d  %4d squarings + %3d products  wall %7.3f ms | cycles per exponentiation: mean %.5g (min %.5g max %.5g)"
                    " | clock held %.3f GHz\n", name, (int)DBL, (int)KARA, (int)KRED, sq, mul, ms, mean, (double)cyc.front(), (double)cyc.back(),
                    (double)cyc.back() / (ms * 1e6));
  }
  hipFree(din); hipFree(dn); hipFree(dout); hipFree(dcyc);
}

template <int K, int LB, int MINW, bool BAL = false>
void run(const char* name, int blocks, unsigned lds, int iters, double instr_per_iter) {
  const size_t lanes = (size_t)blocks * 256, waves = lanes / 64;
  std::vector<uint32_t> h(lanes * 2 * K), hn(2 * K);
  srand(1);
  for (auto& v : h) v = ((uint32_t)rand() * 2654435761u) & ((1u << LB) - 1);
  for (auto& v : hn) v = ((uint32_t)rand() * 2654435761u) & ((1u << LB) - 1);
  hn[0] = hn[K] = (1u << LB) - 1;
  uint32_t n0inv = 0;
  if (BAL) {   // limbs in [-2^(LB-2), 2^(LB-2)) (the products keep them balanced), an odd modulus and its true n0inv
    for (auto& v : h) v = (uint32_t)((int32_t)(v >> 1) - (1 << (LB - 2)));
    for (auto& v : hn) v = (uint32_t)((int32_t)(v >> 1) - (1 << (LB - 2)));
    hn[0] |= 1u;
    hn[K - 1] = 1u << (LB - 10);      // (a positive modulus near 2^(LB*K - 9): the 1040-bit case of the class)
    uint32_t inv = 1;
    for (int i = 0; i < 5; ++i) inv *= 2u - hn[0] * inv;
    n0inv = (0u - inv) & ((1u << LB) - 1);
  }
  uint32_t *din, *dn, *dout;
  unsigned long long* dcyc;
  hipMalloc(&din, h.size() * 4); hipMalloc(&dn, hn.size() * 4); hipMalloc(&dout, h.size() * 4); hipMalloc(&dcyc, waves * 8);
  hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(dn, hn.data(), hn.size() * 4, hipMemcpyHostToDevice);
  const void* kfn;
  if constexpr (BAL) kfn = (const void*)sq_kernel_bal<K, LB, MINW>;
  else kfn = (const void*)sq_kernel<K, LB, MINW>;
  if (lds) hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  std::vector<unsigned long long> cyc(waves);
  for (int rep = 0; rep < 4; ++rep) {
    hipEventRecord(e0);
    if constexpr (BAL) hipLaunchKernelGGL((sq_kernel_bal<K, LB, MINW>), dim3(blocks), dim3(256), lds, 0, din, dn, dout, dcyc, iters, n0inv);
    else hipLaunchKernelGGL((sq_kernel<K, LB, MINW>), dim3(blocks), dim3(256), lds, 0, din, dn, dout, dcyc, iters, 0);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipMemcpy(cyc.data(), dcyc, waves * 8, hipMemcpyDeviceToHost);
    std::sort(cyc.begin(), cyc.end());
    double mean = 0;
    for (auto v : cyc) mean += (double)v;
    mean /= waves;
    const double instr = iters * instr_per_iter;
    if (rep) printf("%-56s K=%d blocks=%4d  wall %7.3f ms | s_memtime span per wave: mean %.4g (min %.4g max %.4g) cycles "
                    "= %.3f cycles/instr | clock held %.3f GHz | wall-time figure %.2f ns/instr\n",
                    name, K, blocks, ms, mean, (double)cyc.front(), (double)cyc.back(), mean / instr, (double)cyc.back() / (ms * 1e6),
                    ms * 1e6 / instr);
  }
  hipFree(din); hipFree(dn); hipFree(dout); hipFree(dcyc);
}

int main(int argc, char** argv) {
  if (argc > 1 && argv[1][0] == 'r') {   // `ubench_ps r`: the sixth part alone, the parent's form first, between and last
    printf("# folded reductions: w=6, odd-power table, lone quarter chip (64 WGs, CU claim, MINW=1)\n");
    run_exp<36, 29, true, true, true, false>("schoolbook reductions (parent)", 64, 84000, 31, 4, 171, 6, 1);
    run_exp<36, 29, true, true, true, true>("folded reductions of a2*b and a*c", 64, 84000, 31, 4, 171, 6, 1);
    run_exp<36, 29, true, true, true, false>("schoolbook reductions (parent)", 64, 84000, 31, 4, 171, 6, 1);
    run_exp<36, 29, true, true, true, true>("folded reductions of a2*b and a*c", 64, 84000, 31, 4, 171, 6, 1);
    run_exp<36, 29, true, true, true, false>("schoolbook reductions (parent again)", 64, 84000, 31, 4, 171, 6, 1);
    return 0;
  }
  // instructions per window (5 squarings + 1 product + the loop's own) of sq_kernel<38,28,*>: tools/asm_stats.py
  const double ipi38 = argc > 1 ? atof(argv[1]) : 5 * 5560.0 + 7700.0;
  const double ipi38w1 = argc > 2 ? atof(argv[2]) : ipi38;
  printf("# PGPU_PS_SPLIT=%d  instructions per window: %.0f (two wavefronts per SIMD build) / %.0f (one wavefront per SIMD build)\n",
         PGPU_PS_SPLIT, ipi38, ipi38w1);
  run<38, 28, 1>("lone quarter chip (64 WGs, CU claim, MINW=1)", 64, 84000, 205, ipi38w1);
  run<38, 28, 1>("full chip, one wavefront per SIMD (MINW=1)", 256, 84000, 205, ipi38w1);
  run<38, 28, 2>("full chip, one wavefront per SIMD (MINW=2)", 256, 84000, 205, ipi38);
  run<38, 28, 2>("full chip, two wavefronts per SIMD (MINW=2)", 512, 0, 205, ipi38);
  run<38, 28, 1>("one WG only (4 waves on one CU, MINW=1)", 1, 84000, 205, ipi38w1);
  // the balanced K = 36, LB = 29 window: instructions per window of sq_kernel_bal<36,29,2> / <36,29,1> as argv[3] / argv[4]
  const double ipi36 = argc > 3 ? atof(argv[3]) : 5 * 5250.0 + 7400.0;
  const double ipi36w1 = argc > 4 ? atof(argv[4]) : ipi36;
  printf("# balanced K=36 LB=29  instructions per window: %.0f (two wavefronts per SIMD build) / %.0f (one wavefront per SIMD build)\n",
         ipi36, ipi36w1);
  run<36, 29, 1, true>("balanced: lone quarter chip (64 WGs, CU claim, MINW=1)", 64, 84000, 205, ipi36w1);
  run<36, 29, 1, true>("balanced: full chip, one wavefront per SIMD (MINW=1)", 256, 84000, 205, ipi36w1);
  run<36, 29, 2, true>("balanced: full chip, one wavefront per SIMD (MINW=2)", 256, 84000, 205, ipi36);
  run<36, 29, 2, true>("balanced: full chip, two wavefronts per SIMD (MINW=2)", 512, 0, 205, ipi36);
  run<38, 28, 1>("unsigned again: lone quarter chip (MINW=1)", 64, 84000, 205, ipi38w1);
  // whole exponentiations of a 1024-bit exponent on balanced limbs, lone quarter chip with the CU claim, MINW = 1:
  // the parent's form first and last
  printf("# one exponentiation (1024-bit exponent), balanced K=36 LB=29, lone quarter chip (64 WGs, CU claim, MINW=1)\n");
  run_exp<36, 29, false>("parent: w=5, chained table (30 products)", 64, 84000, 30, 0, 204, 5, 1);
  run_exp<36, 29, false>("w=5, half-squared table", 64, 84000, 15, 1, 204, 5, 1);
  run_exp<36, 29, false>("w=6, half-squared table", 64, 84000, 31, 1, 170, 6, 1);
  run_exp<36, 29, true>("w=5, chained table (30 products)", 64, 84000, 30, 0, 204, 5, 1);
  run_exp<36, 29, true>("w=5, half-squared table", 64, 84000, 15, 1, 204, 5, 1);
  run_exp<36, 29, true>("w=6, half-squared table", 64, 84000, 31, 1, 170, 6, 1);
  // the odd-power table: 1 squaring + 31 products, 171 windows (the top one of 4 bits) with the product inside; its parent beside it
  run_exp<36, 29, true, true>("w=6, odd-power table, product inside the window", 64, 84000, 31, 4, 171, 6, 1);
  run_exp<36, 29, true>("w=6, half-squared table (parent of the odd form)", 64, 84000, 31, 1, 170, 6, 1);
  run_exp<36, 29, true, true>("w=6, odd-power table, product inside the window", 64, 84000, 31, 4, 171, 6, 1);
  run_exp<36, 29, true>("w=6, half-squared table (parent of the odd form)", 64, 84000, 31, 1, 170, 6, 1);
  run_exp<36, 29, false>("squarings alone", 64, 84000, 0, 0, 170, 6, 0);
  run_exp<36, 29, true>("squarings alone", 64, 84000, 0, 0, 170, 6, 0);
  run_exp<36, 29, false>("parent again: w=5, chained table (30 products)", 64, 84000, 30, 0, 204, 5, 1);
  // the Karatsuba split of a2*b (pair squaring) and a*c (pair product), hensel_ps_bal.hpp KARA: the schoolbook form first and last
  printf("# Karatsuba split of the single products: w=6, odd-power table, lone quarter chip (64 WGs, CU claim, MINW=1)\n");
  run_exp<36, 29, true, true, false>("schoolbook single products (parent)", 64, 84000, 31, 4, 171, 6, 1);
  run_exp<36, 29, true, true, true>("Karatsuba a2*b and a*c", 64, 84000, 31, 4, 171, 6, 1);
  run_exp<36, 29, true, true, false>("schoolbook single products (parent)", 64, 84000, 31, 4, 171, 6, 1);
  run_exp<36, 29, true, true, true>("Karatsuba a2*b and a*c", 64, 84000, 31, 4, 171, 6, 1);
  run_exp<36, 29, true, true, false>("schoolbook single products (parent again)", 64, 84000, 31, 4, 171, 6, 1);
  return 0;
}
