// ipcl::ext::gather / concat / slice -- re-indexing of ciphertexts on the device (include/ipcl/ext/index.hpp): one
// pgpu_batch_gather / _concat / _slice call on resident batches.  The reference re-orders host vectors
// (CipherText::rotate, ciphertext.cpp:117-133; BaseText::getChunk, base_text.cpp:88-95).
#include "ipcl/ext/index.hpp"

#include "detail.hpp"

namespace ipcl {

CipherText CipherText::indexMap(const char* what, const std::vector<const CipherText*>& xs, const std::vector<uint64_t>* idx,
                                std::size_t start, std::size_t count, std::size_t step) {
  const std::string op(what);
  ERROR_CHECK(!xs.empty(), op + " error: no CipherText");
  std::size_t total = 0;
  for (const CipherText* x : xs) {
    ERROR_CHECK(x != nullptr, op + " error: null CipherText");
    ERROR_CHECK(x->m_size > 0, op + " error: empty CipherText");
    ERROR_CHECK(*(x->m_pk->getN()) == *(xs[0]->m_pk->getN()), op + " error: 2 different public keys detected!");
    total += x->m_size;
  }
  if (idx) {
    ERROR_CHECK(!idx->empty(), op + " error: empty index list");
    for (uint64_t v : *idx) ERROR_CHECK(v < total || v == ext::kGatherOne, op + " error: index is out of range");
  } else if (step) {
    ERROR_CHECK(count > 0, op + " error: count must be positive");
    ERROR_CHECK(start < total && count - 1 <= (total - 1 - start) / step, op + " error: parameter is incorrect");
  }
  const std::shared_ptr<PublicKey>& pk = xs[0]->m_pk;
  const BigNumber& nsq = *(pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  std::vector<std::shared_ptr<detail::DeviceBatch>> keep;      // device-resident operands are used in place
  std::vector<const pgpu_batch*> hs;
  for (const CipherText* x : xs) {
    keep.push_back(x->deviceBatch(W, &nsq));
    hs.push_back(keep.back()->h);
  }
  pgpu_batch* o = nullptr;
  if (idx) IPCL_GPU_CHECK(pgpu_batch_gather(hs.data(), hs.size(), idx->data(), idx->size(), &o), what);
  else if (step) IPCL_GPU_CHECK(pgpu_batch_slice(hs[0], start, count, step, &o), what);
  else IPCL_GPU_CHECK(pgpu_batch_concat(hs.data(), hs.size(), &o), what);
  return CipherText(pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText gather(const CipherText& x, const std::vector<uint64_t>& idx) { return gather(std::vector<const CipherText*>{&x}, idx); }

CipherText gather(const std::vector<const CipherText*>& xs, const std::vector<uint64_t>& idx) {
  return CipherText::indexMap("gather", xs, &idx, 0, 0, 0);
}

CipherText concat(const std::vector<const CipherText*>& xs) { return CipherText::indexMap("concat", xs, nullptr, 0, 0, 0); }

CipherText slice(const CipherText& x, std::size_t start, std::size_t count, std::size_t step) {
  ERROR_CHECK(step > 0, "slice error: step must be positive");
  return CipherText::indexMap("slice", {&x}, nullptr, start, count, step);
}

}  // namespace ext
}  // namespace ipcl
