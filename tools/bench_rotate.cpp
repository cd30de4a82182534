// CipherText::rotate(1) of a device-resident text at the ipcl:: API, wall time (tools/, a measurement):
//   resident   the text's current copy is the device's: one pgpu_batch_gather, the result stays resident
//   host       what rotate did before for the same text, and still does for a text whose host copy is current: download
//              and conversion to BigNumbers (a fresh copy of the text each time, so that every run pays it), rotation of
//              the host vector; the next operator then uploads the result again (timed here as rotate + operator+)
// build: g++ -O2 -std=c++17 -fopenmp -Iinclude tools/bench_rotate.cpp -Lpailliercryptolib_amd -lipcl_amd -lpgpu
//        -Wl,-rpath,$PWD/pailliercryptolib_amd -o build/bench_rotate
// usage: bench_rotate [count = 65536] [reps = 5]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ipcl/ipcl.hpp"
#include "pgpu.h"

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  const size_t count = argc > 1 ? (size_t)std::atol(argv[1]) : 65536;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
  ipcl::initializeContext("default");
  {
    ipcl::KeyPair key = ipcl::generateKeypair(2048, true);
    std::mt19937 rng(1);
    std::vector<uint32_t> m(count);
    for (auto& v : m) v = rng();
    ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(m));
    std::vector<double> res, res_add, host, host_add;
    for (int r = 0; r <= reps; ++r) {
      pgpu_synchronize();
      double t0 = now_ms();
      ipcl::CipherText a = ct.rotate(1);
      pgpu_synchronize();
      double t1 = now_ms();
      ipcl::CipherText s = a + ct;
      pgpu_synchronize();
      double t2 = now_ms();
      ipcl::CipherText copy(ct);                        // shares the device batch, downloads on its own
      double t3 = now_ms();
      (void)copy.getElement(0);                         // the download and conversion the host path begins with
      ipcl::CipherText b = copy.rotate(1);
      double t4 = now_ms();
      ipcl::CipherText u = b + ct;
      pgpu_synchronize();
      double t5 = now_ms();
      if (r == 0) {                                     // warm-up, and the values once
        bool same = a.getSize() == b.getSize();
        for (size_t i = 0; same && i < count; i += 997) same = a.getElement(i) == b.getElement(i) && s.getElement(i) == u.getElement(i);
        std::printf("resident and host rotate agree: %s\n", same ? "yes" : "NO");
        if (!same) return 1;
        continue;
      }
      res.push_back(t1 - t0);
      res_add.push_back(t2 - t0);
      host.push_back(t4 - t3);
      host_add.push_back(t5 - t3);
    }
    std::printf("rotate(1) of %zu resident ciphertexts, 2048-bit key, wall ms, median of %d\n", count, reps);
    std::printf("  resident (gather on the device):        rotate %.3f   rotate + operator+ %.3f\n", median(res), median(res_add));
    std::printf("  host path (download, rotate, upload):   rotate %.3f   rotate + operator+ %.3f\n", median(host), median(host_add));
  }
  ipcl::terminateContext();
  return 0;
}
