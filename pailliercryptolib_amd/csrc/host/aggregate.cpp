// ipcl::ext::segmentSum -- grouped aggregation on encrypted vectors (include/ipcl/ext/aggregate.hpp): one
// pgpu_batch_ct_segment_sum call on resident batches.  The reference composes such a sum from CipherText::operator+
// (ciphertext.cpp:35-72) element by element, after gathering the elements of every group on the host.
#include "ipcl/ext/aggregate.hpp"

#include "detail.hpp"

namespace ipcl {

CipherText CipherText::segmentMap(const std::vector<uint32_t>& ids, std::size_t n_segments, std::size_t groups) const {
  ERROR_CHECK(m_size > 0, "segmentSum error: empty CipherText");
  ERROR_CHECK(groups > 0 && n_segments > 0, "segmentSum error: groups and n_segments must be positive");
  ERROR_CHECK(ids.size() / groups == m_size && ids.size() % groups == 0, "segmentSum error: Size mismatch!");
  for (uint32_t id : ids) ERROR_CHECK(id < n_segments || id == ext::kSegmentNone, "segmentSum error: segment id out of range");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  auto dx = deviceBatch(W, &nsq);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_segment_sum(m_pk->device()->h, dx->h, ids.data(), groups, n_segments, &o), "segmentSum");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText segmentSum(const CipherText& x, const std::vector<uint32_t>& ids, std::size_t n_segments, std::size_t groups) {
  return x.segmentMap(ids, n_segments, groups);
}

}  // namespace ext
}  // namespace ipcl
