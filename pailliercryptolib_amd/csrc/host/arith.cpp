// ipcl::ext::negate / subtract -- ciphertext negation and subtraction (include/ipcl/ext/arith.hpp): one
// pgpu_batch_ct_negate / pgpu_batch_ct_sub call on resident batches.  The reference has no such operation; its route to
// Enc(-m) is CipherText::operator*(PlainText) with n - 1 (ciphertext.cpp:83-107), an exponentiation per element.
#include "ipcl/ext/arith.hpp"

#include "detail.hpp"

namespace ipcl {

CipherText CipherText::inverseMap(const CipherText* b) const {
  const char* what = b ? "CT - CT" : "negate";
  if (b) {
    ERROR_CHECK(m_size == b->getSize() || b->getSize() == 1, "CT - CT error: Size mismatch!");
    ERROR_CHECK(*(m_pk->getN()) == *(b->m_pk->getN()), "CT - CT error: 2 different public keys detected!");
  }
  ERROR_CHECK(m_size > 0, b ? "CT - CT error: empty CipherText" : "negate error: empty CipherText");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  auto da = deviceBatch(W, &nsq);
  pgpu_batch* o = nullptr;
  if (b) {
    auto db = b->deviceBatch(W, &nsq);
    IPCL_GPU_CHECK(pgpu_batch_ct_sub(m_pk->device()->h, da->h, db->h, &o), what);
  } else {
    IPCL_GPU_CHECK(pgpu_batch_ct_negate(m_pk->device()->h, da->h, &o), what);
  }
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText negate(const CipherText& x) { return x.inverseMap(nullptr); }

CipherText subtract(const CipherText& a, const CipherText& b) { return a.inverseMap(&b); }

}  // namespace ext
}  // namespace ipcl
