// ipcl::ext::segmentSum / segmentScan -- grouped aggregation on encrypted vectors (include/ipcl/ext/aggregate.hpp): one
// pgpu_batch_ct_segment_sum / pgpu_batch_ct_segment_scan call on resident batches.  The reference composes such a sum from CipherText::operator+
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

CipherText CipherText::segmentScanMap(std::size_t seg_len, bool reverse) const {
  ERROR_CHECK(m_size > 0, "segmentScan error: empty CipherText");
  ERROR_CHECK(seg_len > 0 && m_size % seg_len == 0, "segmentScan error: seg_len must be positive and divide the size");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  auto dx = deviceBatch(W, &nsq);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_segment_scan(m_pk->device()->h, dx->h, seg_len, reverse ? PGPU_SCAN_REVERSE : 0u, &o), "segmentScan");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText segmentSum(const CipherText& x, const std::vector<uint32_t>& ids, std::size_t n_segments, std::size_t groups) {
  return x.segmentMap(ids, n_segments, groups);
}

CipherText segmentScan(const CipherText& x, std::size_t seg_len, bool reverse) { return x.segmentScanMap(seg_len, reverse); }

}  // namespace ext
}  // namespace ipcl
