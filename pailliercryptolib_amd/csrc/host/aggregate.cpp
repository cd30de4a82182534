// ipcl::ext::segmentSum / segmentScan / packSlots -- grouped aggregation on encrypted vectors (include/ipcl/ext/aggregate.hpp): one
// pgpu_batch_ct_segment_sum / pgpu_batch_ct_segment_scan / pgpu_batch_ct_pack call on resident batches.  The reference composes such a sum from CipherText::operator+
// (ciphertext.cpp:35-72) element by element, after gathering the elements of every group on the host.
#include "ipcl/ext/aggregate.hpp"

#include <climits>

#include "detail.hpp"
#include "ipcl/ext/slots.hpp"

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

CipherText CipherText::packMap(std::size_t seg_len, std::size_t slot_bits) const {
  ERROR_CHECK(m_size > 0, "packSlots error: empty CipherText");
  ERROR_CHECK(seg_len > 0 && m_size % seg_len == 0, "packSlots error: seg_len must be positive and divide the size");
  ERROR_CHECK(slot_bits > 0 && slot_bits <= (std::size_t)INT_MAX, "packSlots error: slot_bits must be positive");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  auto dx = deviceBatch(W, &nsq);
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_pack(m_pk->device()->h, dx->h, seg_len, (int)slot_bits, &o), "packSlots");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

CipherText segmentSum(const CipherText& x, const std::vector<uint32_t>& ids, std::size_t n_segments, std::size_t groups) {
  return x.segmentMap(ids, n_segments, groups);
}

CipherText segmentScan(const CipherText& x, std::size_t seg_len, bool reverse) { return x.segmentScanMap(seg_len, reverse); }

CipherText packSlots(const CipherText& x, std::size_t seg_len, std::size_t slot_bits) { return x.packMap(seg_len, slot_bits); }

PlainText unpackSlots(const PlainText& m, std::size_t seg_len, std::size_t slot_bits) {
  std::size_t span = 0;
  ERROR_CHECK(detail::slots_span(seg_len, slot_bits, &span), "unpackSlots error: seg_len and slot_bits must be positive (and their product a bit count)");
  ERROR_CHECK(m.getSize() > 0, "unpackSlots error: empty PlainText");
  const std::vector<BigNumber> texts = m.getTexts();
  std::vector<BigNumber> out;
  out.reserve(texts.size() * seg_len);
  std::vector<uint64_t> slot(detail::slot_limbs(slot_bits));
  for (const BigNumber& v : texts) {
    const BigNumber::Limbs& limbs = v.limbs64();
    ERROR_CHECK(!v.isNegative() && detail::slots_fit(limbs.data(), limbs.size(), span),
                "unpackSlots error: a plaintext does not fit seg_len slots of slot_bits bits");
    for (std::size_t t = 0; t < seg_len; ++t) {
      detail::slice_slot(limbs.data(), limbs.size(), t * slot_bits, slot_bits, slot.data());
      out.push_back(BigNumber::fromLimbs64(slot.data(), slot.size()));
    }
  }
  return PlainText(out);
}

}  // namespace ext
}  // namespace ipcl
