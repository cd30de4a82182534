// ipcl::ext::matVec / dot / matVecBucket / matMul / matVecSigned / dotSigned / matMulSigned / sparseMatVec / sparseMatVecSigned / weightedSum / sum -- linear maps on encrypted vectors (include/ipcl/ext/linear.hpp): one
// pgpu_batch_ct_matvec / pgpu_batch_ct_matvec_bucket / pgpu_batch_ct_matmul / pgpu_batch_ct_matvec_signed / pgpu_batch_ct_matmul_signed / pgpu_batch_ct_spmv / pgpu_batch_ct_spmv_signed / pgpu_batch_ct_weighted_sum call on resident batches.  The reference composes such a map from CipherText::operator*
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

CipherText CipherText::linearMapBucket(const PlainText& w, std::size_t rows) const {
  ERROR_CHECK(m_size > 0, "matVec error: empty CipherText");
  ERROR_CHECK(rows > 0 && w.getSize() / rows == m_size && w.getSize() % rows == 0, "matVec error: Size mismatch!");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  // the weights as host words: the digits are cut from them, the device never reads them
  const std::vector<BigNumber> a = w.getTexts();
  int ebits = 1;
  for (const auto& e : a) {
    ERROR_CHECK(!e.isNegative(), "matVec error: negative plaintext");
    ebits = std::max(ebits, e.BitSize());
  }
  const int ww = detail::words_for_bits(ebits);
  std::vector<uint64_t> words(a.size() * (size_t)ww, 0);
  std::vector<Ipp32u> v;
  for (size_t k = 0; k < a.size(); ++k) {
    v.clear();
    a[k].num2vec(v);
    for (size_t j = 0; j < v.size() && j < (size_t)2 * ww; ++j) words[k * (size_t)ww + j / 2] |= (uint64_t)v[j] << (32 * (j & 1));
  }
  auto dx = deviceBatch(W, &nsq);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_matvec_bucket(m_pk->device()->h, dx->h, words.data(), ww, rows, ebits, &o), "matVecBucket");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

CipherText CipherText::linearMapBatch(const PlainText& w, std::size_t rows, std::size_t n_vec, bool transposed) const {
  ERROR_CHECK(m_size > 0, "matMul error: empty CipherText");
  ERROR_CHECK(n_vec > 0 && m_size % n_vec == 0, "matMul error: Size mismatch! (n_vec must divide the CipherText)");
  const std::size_t cols = m_size / n_vec;
  ERROR_CHECK(rows > 0 && w.getSize() / rows == cols && w.getSize() % rows == 0, "matMul error: Size mismatch!");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  if (!w.isDeviceResident())
    for (const auto& e : w.m_texts) ERROR_CHECK(!e.isNegative(), "matMul error: negative plaintext");
  const int ebits = std::max(1, w.maxBitsHint());
  const int ew = w.isDeviceResident() ? w.m_dev->words : detail::words_for_bits(ebits);
  auto dx = deviceBatch(W, &nsq), dw = w.deviceBatch(ew);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_matmul(m_pk->device()->h, dx->h, dw->h, n_vec, rows, ebits,
                                      transposed ? PGPU_MATMUL_TRANSPOSED : 0u, &o),
                 "matMul");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

CipherText CipherText::signedLinearMap(const std::vector<int64_t>& w, std::size_t rows, std::size_t n_vec, bool transposed) const {
  const bool batch = n_vec != 0;
  const char* what = batch ? "matMulSigned" : "matVecSigned";
  ERROR_CHECK(m_size > 0, batch ? "matMulSigned error: empty CipherText" : "matVecSigned error: empty CipherText");
  ERROR_CHECK(!batch || m_size % n_vec == 0, "matMulSigned error: Size mismatch! (n_vec must divide the CipherText)");
  const std::size_t cols = batch ? m_size / n_vec : m_size;
  ERROR_CHECK(rows > 0 && w.size() / rows == cols && w.size() % rows == 0,
              batch ? "matMulSigned error: Size mismatch!" : "matVecSigned error: Size mismatch!");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  std::vector<uint64_t> words;
  const int ebits = detail::signed_weight_words(w, &words);
  auto dx = deviceBatch(W, &nsq), dw = detail::DeviceBatch::upload(words, words.size(), 1);
  pgpu_batch* o = nullptr;
  if (batch)
    IPCL_GPU_CHECK(pgpu_batch_ct_matmul_signed(m_pk->device()->h, dx->h, dw->h, n_vec, rows, ebits,
                                               transposed ? PGPU_MATMUL_TRANSPOSED : 0u, &o),
                   what);
  else
    IPCL_GPU_CHECK(pgpu_batch_ct_matvec_signed(m_pk->device()->h, dx->h, dw->h, rows, ebits, &o), what);
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

CipherText CipherText::signedSparseLinearMap(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                                             const std::vector<int64_t>& w) const {
  ERROR_CHECK(m_size > 0, "sparseMatVecSigned error: empty CipherText");
  ERROR_CHECK(row_ptr.size() >= 2 && !w.empty(), "sparseMatVecSigned error: empty matrix");
  ERROR_CHECK(row_ptr.back() == col_idx.size() && w.size() == col_idx.size(), "sparseMatVecSigned error: Size mismatch!");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  std::vector<uint64_t> words;
  const int ebits = detail::signed_weight_words(w, &words);
  auto dx = deviceBatch(W, &nsq), dw = detail::DeviceBatch::upload(words, words.size(), 1);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_spmv_signed(m_pk->device()->h, dx->h, row_ptr.data(), col_idx.data(), dw->h, row_ptr.size() - 1,
                                           ebits, &o),
                 "sparseMatVecSigned");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

CipherText CipherText::weightedSumMap(const std::vector<CipherText>& xs, const PlainText* w) {
  ERROR_CHECK(!xs.empty(), "weightedSum error: no CipherText");
  ERROR_CHECK(xs[0].m_size > 0, "weightedSum error: empty CipherText");
  ERROR_CHECK(!w || w->getSize() == xs.size(), "weightedSum error: Size mismatch! (one weight per CipherText)");
  const std::shared_ptr<PublicKey>& pk = xs[0].m_pk;
  for (const CipherText& x : xs) {
    ERROR_CHECK(x.m_size == xs[0].m_size, "weightedSum error: Size mismatch!");
    ERROR_CHECK(*(x.m_pk->getN()) == *(pk->getN()), "weightedSum error: 2 different public keys detected!");
  }
  const BigNumber& nsq = *(pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  // the weights as host words: the schedule is built from them, the device never reads them
  std::vector<uint64_t> words;
  int ww = 0;
  if (w) {
    const std::vector<BigNumber> a = w->getTexts();
    int bits = 1;
    for (const auto& e : a) {
      ERROR_CHECK(!e.isNegative(), "weightedSum error: negative plaintext");
      bits = std::max(bits, e.BitSize());
    }
    ww = detail::words_for_bits(bits);
    words.assign(a.size() * (size_t)ww, 0);
    std::vector<Ipp32u> v;
    for (size_t k = 0; k < a.size(); ++k) {
      v.clear();
      a[k].num2vec(v);
      for (size_t j = 0; j < v.size() && j < (size_t)2 * ww; ++j) words[k * (size_t)ww + j / 2] |= (uint64_t)v[j] << (32 * (j & 1));
    }
  }
  std::vector<std::shared_ptr<detail::DeviceBatch>> keep;      // device-resident operands are used in place
  std::vector<const pgpu_batch*> hs;
  for (const CipherText& x : xs) {
    keep.push_back(x.deviceBatch(W, &nsq));
    hs.push_back(keep.back()->h);
  }
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_weighted_sum(pk->device()->h, hs.data(), hs.size(), w ? words.data() : nullptr, ww, &o),
                 "weightedSum");
  return CipherText(pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText weightedSum(const std::vector<CipherText>& xs, const PlainText& w) { return CipherText::weightedSumMap(xs, &w); }
CipherText sum(const std::vector<CipherText>& xs) { return CipherText::weightedSumMap(xs, nullptr); }
CipherText matVec(const PlainText& w, std::size_t rows, const CipherText& x) { return x.linearMap(w, rows); }
CipherText dot(const PlainText& w, const CipherText& x) { return matVec(w, 1, x); }
CipherText matVecBucket(const PlainText& w, std::size_t rows, const CipherText& x) { return x.linearMapBucket(w, rows); }
CipherText matMul(const PlainText& w, std::size_t rows, const CipherText& x, std::size_t n_vec, bool transposed) {
  return x.linearMapBatch(w, rows, n_vec, transposed);
}
CipherText matVecSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x) {
  return x.signedLinearMap(w, rows, 0, false);
}
CipherText dotSigned(const std::vector<int64_t>& w, const CipherText& x) { return matVecSigned(w, 1, x); }
CipherText matMulSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x, std::size_t n_vec, bool transposed) {
  ERROR_CHECK(n_vec > 0, "matMulSigned error: Size mismatch! (n_vec must divide the CipherText)");
  return x.signedLinearMap(w, rows, n_vec, transposed);
}
CipherText sparseMatVec(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx, const PlainText& w,
                        const CipherText& x) {
  return x.sparseLinearMap(row_ptr, col_idx, w);
}
CipherText sparseMatVecSigned(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                              const std::vector<int64_t>& w, const CipherText& x) {
  return x.signedSparseLinearMap(row_ptr, col_idx, w);
}

}  // namespace ext
}  // namespace ipcl
