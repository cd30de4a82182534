// ipcl::ext::matVec / dot / sparseMatVec -- linear maps on encrypted vectors (include/ipcl/ext/linear.hpp): one
// pgpu_batch_ct_matvec / pgpu_batch_ct_spmv call on resident batches.  The reference composes such a map from CipherText::operator*
// (ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72) term by term.
#include "ipcl/ext/linear.hpp"

#include <algorithm>

#include "detail.hpp"

namespace ipcl {

CipherText CipherText::linearMap(const PlainText& w, std::size_t rows) const {
  ERROR_CHECK(m_size > 0, "matVec error: empty CipherText");
  ERROR_CHECK(rows > 0 && w.getSize() / rows == m_size && w.getSize() % rows == 0, "matVec error: Size mismatch!");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  if (!w.isDeviceResident())
    for (const auto& e : w.m_texts) ERROR_CHECK(!e.isNegative(), "matVec error: negative plaintext");
  const int ebits = std::max(1, w.maxBitsHint());
  const int ew = w.isDeviceResident() ? w.m_dev->words : detail::words_for_bits(ebits);
  auto dx = deviceBatch(W, &nsq), dw = w.deviceBatch(ew);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_matvec(m_pk->device()->h, dx->h, dw->h, rows, ebits, &o), "matVec");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

CipherText CipherText::sparseLinearMap(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                                       const PlainText& w) const {
  ERROR_CHECK(m_size > 0, "sparseMatVec error: empty CipherText");
  ERROR_CHECK(row_ptr.size() >= 2 && w.getSize() > 0, "sparseMatVec error: empty matrix");
  ERROR_CHECK(row_ptr.back() == col_idx.size() && w.getSize() == col_idx.size(), "sparseMatVec error: Size mismatch!");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  if (!w.isDeviceResident())
    for (const auto& e : w.m_texts) ERROR_CHECK(!e.isNegative(), "sparseMatVec error: negative plaintext");
  const int ebits = std::max(1, w.maxBitsHint());
  const int ew = w.isDeviceResident() ? w.m_dev->words : detail::words_for_bits(ebits);
  auto dx = deviceBatch(W, &nsq), dw = w.deviceBatch(ew);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_spmv(m_pk->device()->h, dx->h, row_ptr.data(), col_idx.data(), dw->h, row_ptr.size() - 1,
                                    ebits, &o),
                 "sparseMatVec");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText matVec(const PlainText& w, std::size_t rows, const CipherText& x) { return x.linearMap(w, rows); }
CipherText dot(const PlainText& w, const CipherText& x) { return matVec(w, 1, x); }
CipherText sparseMatVec(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx, const PlainText& w,
                        const CipherText& x) {
  return x.sparseLinearMap(row_ptr, col_idx, w);
}

}  // namespace ext
}  // namespace ipcl
