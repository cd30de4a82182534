// CPU unit test of the plan of the encrypted matrix-vector product (pailliercryptolib_amd/csrc/policy.cpp: matvec_*):
// key class -> geometry, (rows, cols) -> column slices, (rows, cols, e_bits, slices) -> window.  Pure host logic -- built
// with g++ from policy.cpp alone, no device, no HIP call.  The shapes are those tools/bench_matvec.py measures, plus the
// edges.  In the reference such a map is composed from CipherText::operator* (ipcl/ciphertext.cpp:83-106) and operator+
// (ciphertext.cpp:35-72) term by term; the rule is documented in DESIGN.md ("Encrypted matrix-vector product").
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "policy.hpp"

namespace pol = pgpu::policy;
static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failed;                                                          \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static int best_window(size_t rows, size_t cols, int e_bits, size_t S, size_t row_bytes) {
  int best = 1;
  for (int w = 2; w <= 6; ++w)
    if (cols * ((size_t)1 << w) * row_bytes <= pol::kMatvecTableCap &&
        pol::matvec_products(rows, cols, e_bits, w, S) < pol::matvec_products(rows, cols, e_bits, best, S))
      best = w;
  return best;
}

int main() {
  int G = 0, K = 0;
  // ---- geometry: the sequential-halves forms of the three key classes with pair rows ----
  CHECK(pol::matvec_geometry(1024, &G, &K) && G == 2 && K == 19);
  CHECK(pol::matvec_geometry(2048, &G, &K) && G == 4 && K == 18);
  CHECK(pol::matvec_geometry(3072, &G, &K) && G == 8 && K == 14);
  CHECK(pol::matvec_geometry(1536, &G, &K) && G == 4 && K == 18);     // between the classes: the next wider rows
  CHECK(pol::matvec_geometry(1065, &G, &K) && G == 2);
  CHECK(pol::matvec_geometry(1066, &G, &K) && G == 4);
  CHECK(!pol::matvec_geometry(4096, &G, &K) && !pol::matvec_geometry(0, &G, &K));
  // ---- slices, 2048-bit keys: 16 rows of one slice per wavefront ----
  CHECK(pol::matvec_slices(4, 1024, 1024) == 16);     // 64 wavefronts per slice: 16 slices cover the 1024 SIMDs
  CHECK(pol::matvec_slices(4, 64, 1024) == 256);      // 4 wavefronts per slice; 256 slices of 4 columns
  CHECK(pol::matvec_slices(4, 1, 1024) == 256);       // a lone dot product: the cap, 4 columns per slice
  CHECK(pol::matvec_slices(4, 4096, 256) == 4);
  CHECK(pol::matvec_slices(4, 16384, 256) == 1);      // the rows alone fill the chip
  CHECK(pol::matvec_slices(4, 100000, 16) == 1);
  CHECK(pol::matvec_slices(8, 256, 512) == 32);       // 3072-bit keys: 8 rows per wavefront
  CHECK(pol::matvec_slices(2, 1024, 1024) == 32);     // 1024-bit keys: 32 rows per wavefront
  // edges: one row, one column, fewer columns than slices wanted
  CHECK(pol::matvec_slices(4, 1, 1) == 1 && pol::matvec_slices(4, 3, 1) == 1);
  CHECK(pol::matvec_slices(4, 1, 3) == 1);            // fewer than 4 columns: one slice
  CHECK(pol::matvec_slices(4, 1, 7) == 1 && pol::matvec_slices(4, 1, 8) == 2);
  CHECK(pol::matvec_slices(4, 5, 33) == 8);           // wanted 1024, the columns allow 8
  for (size_t rows : {1, 5, 64, 1000, 5000})
    for (size_t cols : {1, 2, 9, 300, 4096}) {
      const size_t S = pol::matvec_slices(4, rows, cols);
      CHECK(S >= 1 && S <= cols);
      CHECK(S == 1 || cols / S >= pol::kMatvecMinSliceCols);
    }
  // ---- window: the fewest products of the documented count, under the table cap ----
  struct { size_t rows, cols; int e_bits, G, K; } shapes[] = {
      {1, 1024, 32, 4, 18}, {64, 1024, 32, 4, 18}, {1024, 1024, 32, 4, 18}, {4096, 256, 32, 4, 18},
      {256, 512, 32, 8, 14}, {256, 512, 64, 4, 18}, {1, 1, 32, 4, 18}, {3, 1, 32, 4, 18}, {1, 7, 127, 4, 18}};
  for (const auto& s : shapes) {
    const size_t rb = (size_t)2 * s.G * s.K * 4, S = pol::matvec_slices(s.G, s.rows, s.cols);
    CHECK(pol::matvec_window(s.rows, s.cols, s.e_bits, S, rb) == best_window(s.rows, s.cols, s.e_bits, S, rb));
  }
  CHECK(pol::matvec_window(1024, 1024, 32, 16, 576) == 6);    // many rows amortise a large table
  CHECK(pol::matvec_window(1, 1024, 32, 256, 576) == 3);      // a lone dot product: the table is most of the work
  CHECK(pol::matvec_window(1, 1, 32, 1, 576) == 3);           // one term: 6 + 32 + 11 products (w = 4: 14 + 32 + 8)
  CHECK(pol::matvec_window(64, 300, 1, 1, 576) == 1);         // e_bits = 1: a homomorphic sum, no table products at all
  CHECK(pol::matvec_window(1000, 1000, 1, 4, 576) == 1);
  CHECK(pol::matvec_window(4096, 100000, 32, 1, 576) == 2);   // the cap: 100000 columns x 8 entries x 576 B = 461 MB > 256 MiB
  CHECK(pol::matvec_window(4096, (size_t)1 << 20, 32, 1, 576) == 1);   // ... and w = 1 (two entries) is always allowed
  // products of the schedule: table + squarings + multiplications + fold
  CHECK(pol::matvec_products(1024, 1024, 32, 4, 16) == 1024.0 * 14 + 1024.0 * 16 * 32 + 1024.0 * 1024 * 8 + 1024.0 * 15);
  // ---- forced knobs (read at every call) ----
  setenv("PGPU_MATVEC_WINDOW", "5", 1);
  setenv("PGPU_MATVEC_SLICES", "7", 1);
  CHECK(pol::matvec_window(1, 1, 1, 1, 576) == 5 && pol::matvec_slices(4, 100000, 300) == 7);
  CHECK(pol::matvec_slices(4, 2, 3) == 3);                    // clamped to the columns
  setenv("PGPU_MATVEC_WINDOW", "9", 1);
  CHECK(pol::matvec_window(1, 1, 1, 1, 576) == 6);
  unsetenv("PGPU_MATVEC_WINDOW");
  unsetenv("PGPU_MATVEC_SLICES");
  CHECK(pol::matvec_slices(4, 1024, 1024) == 16);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
