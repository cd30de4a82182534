// C++ tests of ipcl::ext::packSlots / unpackSlots (include/ipcl/ext/aggregate.hpp), run on a real MI355X by
// tests/test_gpu_pack_cpp.py: the encrypted slot packing against host BigNumber arithmetic
// (prod_t x[r][t]^(2^(slot_bits t)) mod n^2), with device-resident and host-constructed CipherTexts, through
// PrivateKey::decrypt and unpackSlots back to the values that went in, on the result of segmentScan without leaving
// the device, and the exceptions of the error paths.  In the reference such a packed sum could only be composed from
// CipherText::operator* by powers of two and CipherText::operator+ (ipcl/ciphertext.cpp), element by element.
#include <cstdio>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ipcl/ext/aggregate.hpp"
#include "ipcl/ipcl.hpp"

static int g_failed = 0, g_checks = 0;
#define EXPECT_TRUE(c)                                                                 \
  do {                                                                                 \
    ++g_checks;                                                                        \
    if (!(c)) { ++g_failed; std::printf("  FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } \
  } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))
#define EXPECT_THROW(stmt)                                        \
  do {                                                            \
    bool thrown_ = false;                                         \
    try { stmt; } catch (const std::runtime_error&) { thrown_ = true; } \
    EXPECT_TRUE(thrown_);                                         \
  } while (0)

struct Case { const char* name; std::function<void()> fn; };
static std::vector<Case>& cases() { static std::vector<Case> c; return c; }
struct Reg { Reg(const char* n, std::function<void()> f) { cases().push_back({n, f}); } };
#define TEST(name) static void name(); static Reg reg_##name(#name, name); static void name()

static std::vector<uint32_t> random_u32(size_t n, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<uint32_t> v(n);
  for (auto& x : v) x = rng();
  return v;
}

static ipcl::KeyPair& shared_key() {
  static ipcl::KeyPair key = ipcl::generateKeypair(2048, true);
  return key;
}

// Horner on the host: start as the last entry, slot_bits squarings and one product per entry, downwards
static std::vector<BigNumber> host_pack(const std::vector<BigNumber>& x, size_t seg_len, size_t slot_bits, const BigNumber& nsq) {
  std::vector<BigNumber> out;
  for (size_t r = 0; r < x.size() / seg_len; ++r) {
    BigNumber acc = x[r * seg_len + seg_len - 1];
    for (size_t t = seg_len - 1; t-- > 0;) {
      for (size_t i = 0; i < slot_bits; ++i) acc = (acc * acc) % nsq;
      acc = (acc * x[r * seg_len + t]) % nsq;
    }
    out.push_back(acc);
  }
  return out;
}

TEST(pack_against_host_bignumber_resident_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 3, seg_len = 5, slot_bits = 12;
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(rows * seg_len, 11)));
  EXPECT_TRUE(ct.isDeviceResident());
  ipcl::CipherText y = ipcl::ext::packSlots(ct, seg_len, slot_bits);       // the resident batch is used in place
  EXPECT_TRUE(ct.isDeviceResident());
  EXPECT_TRUE(y.isDeviceResident());                                       // (before getTexts() materialises host copies)
  EXPECT_EQ(y.getSize(), rows);
  ipcl::CipherText copy = ipcl::ext::packSlots(ct, 1, 9);                  // one slot per row: a copy
  EXPECT_TRUE(copy.isDeviceResident());
  EXPECT_EQ(copy.getSize(), rows * seg_len);
  const std::vector<BigNumber> texts = ct.getTexts();                      // an accessor: ct holds host values from here on
  std::vector<BigNumber> want = host_pack(texts, seg_len, slot_bits, *key.pub_key.getNSQ());
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), want[i]);
  for (size_t i = 0; i < texts.size(); ++i) EXPECT_EQ(copy.getElement(i), texts[i]);
}

TEST(pack_host_constructed_input) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 4, seg_len = 3, slot_bits = 7;
  std::vector<BigNumber> texts = key.pub_key.encrypt(ipcl::PlainText(random_u32(rows * seg_len, 21))).getTexts();
  ipcl::CipherText host_ct(key.pub_key, texts);                            // built around host BigNumbers
  ipcl::CipherText y = ipcl::ext::packSlots(host_ct, seg_len, slot_bits);
  EXPECT_TRUE(y.isDeviceResident());
  EXPECT_EQ(y.getSize(), rows);
  std::vector<BigNumber> want = host_pack(texts, seg_len, slot_bits, *key.pub_key.getNSQ());
  for (size_t i = 0; i < want.size(); ++i) EXPECT_EQ(y.getElement(i), want[i]);
}

TEST(round_trip_through_decrypt_and_unpack) {
  ipcl::KeyPair& key = shared_key();
  {
    const size_t rows = 5, seg_len = 31, slot_bits = 32;                   // 32-bit values, slot boundaries inside 64-bit words
    std::vector<uint32_t> m = random_u32(rows * seg_len, 31);
    m[0] = 0xFFFFFFFFu;                                                    // a slot at its largest value next to an empty one
    m[1] = 0;
    ipcl::CipherText packed = ipcl::ext::packSlots(key.pub_key.encrypt(ipcl::PlainText(m)), seg_len, slot_bits);
    EXPECT_EQ(packed.getSize(), rows);
    ipcl::PlainText back = ipcl::ext::unpackSlots(key.priv_key.decrypt(packed), seg_len, slot_bits);
    EXPECT_EQ(back.getSize(), m.size());
    for (size_t i = 0; i < m.size(); ++i) EXPECT_EQ(back.getElement(i), BigNumber(m[i]));
  }
  {
    const size_t rows = 2, seg_len = 24, slot_bits = 83;                   // slots that straddle words, values of 83 bits
    std::mt19937_64 rng(41);
    std::vector<BigNumber> m;
    for (size_t i = 0; i < rows * seg_len; ++i) {
      uint64_t limbs[2] = {rng(), rng() & (((uint64_t)1 << 19) - 1)};
      if (i == 3) { limbs[0] = ~(uint64_t)0; limbs[1] = ((uint64_t)1 << 19) - 1; }
      if (i == 4) limbs[0] = limbs[1] = 0;
      m.push_back(BigNumber::fromLimbs64(limbs, 2));
    }
    ipcl::CipherText packed = ipcl::ext::packSlots(key.pub_key.encrypt(ipcl::PlainText(m)), seg_len, slot_bits);
    ipcl::PlainText back = ipcl::ext::unpackSlots(key.priv_key.decrypt(packed), seg_len, slot_bits);
    EXPECT_EQ(back.getSize(), m.size());
    for (size_t i = 0; i < m.size(); ++i) EXPECT_EQ(back.getElement(i), m[i]);
  }
}

TEST(scan_then_pack_without_leaving_the_device) {
  ipcl::KeyPair& key = shared_key();
  const size_t rows = 3, seg_len = 8;
  std::vector<uint32_t> m = random_u32(rows * seg_len, 51);
  ipcl::CipherText sums = ipcl::ext::segmentScan(key.pub_key.encrypt(ipcl::PlainText(m)), seg_len);
  EXPECT_TRUE(sums.isDeviceResident());
  ipcl::CipherText packed = ipcl::ext::packSlots(sums, seg_len, 40);       // 8 sums of 32-bit values: 35 bits, 40-bit slots
  EXPECT_TRUE(sums.isDeviceResident());
  EXPECT_TRUE(packed.isDeviceResident());
  ipcl::PlainText back = ipcl::ext::unpackSlots(key.priv_key.decrypt(packed), seg_len, 40);
  for (size_t r = 0; r < rows; ++r) {
    BigNumber acc(0u);
    for (size_t t = 0; t < seg_len; ++t) {
      acc = acc + BigNumber(m[r * seg_len + t]);
      EXPECT_EQ(back.getElement(r * seg_len + t), acc);
    }
  }
  // the result is an ordinary CipherText: it feeds the operators (packed rows add slot-wise)
  ipcl::PlainText twice = ipcl::ext::unpackSlots(key.priv_key.decrypt(packed + packed), seg_len, 40);
  EXPECT_EQ(twice.getElement(0), BigNumber(m[0]) + BigNumber(m[0]));
}

TEST(error_paths_throw) {
  ipcl::KeyPair& key = shared_key();
  ipcl::CipherText ct = key.pub_key.encrypt(ipcl::PlainText(random_u32(6, 61)));
  EXPECT_THROW(ipcl::ext::packSlots(ct, 0, 8));                            // no segment length
  EXPECT_THROW(ipcl::ext::packSlots(ct, 4, 8));                            // 6 % 4 != 0
  EXPECT_THROW(ipcl::ext::packSlots(ct, 7, 8));                            // longer than the vector
  EXPECT_THROW(ipcl::ext::packSlots(ct, 3, 0));                            // no slot width
  EXPECT_THROW(ipcl::ext::packSlots(ct, 2, 1024));                         // 2048 bits: wraps modulo a 2048-bit n
  EXPECT_THROW(ipcl::ext::packSlots(ct, 2, (size_t)1 << 40));              // beyond an int
  EXPECT_THROW(ipcl::ext::packSlots(ipcl::CipherText(), 1, 8));            // empty CipherText
  EXPECT_EQ(ipcl::ext::packSlots(ct, 2, 1023).getSize(), (size_t)3);       // at the bound
  EXPECT_EQ(ipcl::ext::packSlots(ct, 6, 16).getSize(), (size_t)1);
  ipcl::PlainText pt(std::vector<uint32_t>{0x12345678u, 7u});
  EXPECT_THROW(ipcl::ext::unpackSlots(pt, 0, 8));
  EXPECT_THROW(ipcl::ext::unpackSlots(pt, 4, 0));
  EXPECT_THROW(ipcl::ext::unpackSlots(pt, 3, 8));                          // 0x12345678 has bits beyond 3 slots of 8
  EXPECT_THROW(ipcl::ext::unpackSlots(pt, (size_t)1 << 62, 4));            // the span overflows
  EXPECT_THROW(ipcl::ext::unpackSlots(ipcl::PlainText(), 1, 8));           // empty PlainText
  ipcl::PlainText bytes = ipcl::ext::unpackSlots(pt, 4, 8);
  EXPECT_EQ(bytes.getSize(), (size_t)8);
  EXPECT_EQ(bytes.getElement(0), BigNumber(0x78u));
  EXPECT_EQ(bytes.getElement(3), BigNumber(0x12u));
  EXPECT_EQ(bytes.getElement(4), BigNumber(7u));
  EXPECT_EQ(bytes.getElement(7), BigNumber(0u));
}

int main(int argc, char** argv) {
  ipcl::initializeContext("default");
  std::string filter = argc > 1 ? argv[1] : "";
  int ran = 0;
  for (auto& c : cases()) {
    if (!filter.empty() && std::string(c.name).find(filter) == std::string::npos) continue;
    int before = g_failed;
    std::printf("[ RUN  ] %s\n", c.name);
    try {
      c.fn();
    } catch (const std::exception& e) {
      ++g_failed;
      std::printf("  EXCEPTION: %s\n", e.what());
    }
    std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", c.name);
    ++ran;
  }
  ipcl::terminateContext();
  std::printf("%d tests, %d checks, %d failed\n", ran, g_checks, g_failed);
  return g_failed ? 1 : 0;
}
