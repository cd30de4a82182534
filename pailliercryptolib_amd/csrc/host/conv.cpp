// ipcl::ext::conv2d / conv1d / conv2dSigned / conv1dSigned -- 2-D convolution on encrypted images
// (include/ipcl/ext/conv.hpp): one pgpu_batch_ct_conv2d / pgpu_batch_ct_conv2d_signed call on resident batches.  The reference composes such a map from CipherText::operator* (ciphertext.cpp:83-106) and
// operator+ (ciphertext.cpp:35-72) term by term.
#include "ipcl/ext/conv.hpp"

#include <algorithm>

#include "detail.hpp"

namespace ipcl {

CipherText CipherText::convMap(const PlainText& w, const ext::Conv2dShape& s) const {
  ERROR_CHECK(m_size > 0, "conv2d error: empty CipherText");
  ERROR_CHECK(s.n_img > 0 && s.c_in > 0 && s.h > 0 && s.w > 0 && s.c_out > 0 && s.kh > 0 && s.kw > 0 && s.stride_h > 0 && s.stride_w > 0,
              "conv2d error: every dimension and stride must be positive");
  ERROR_CHECK(s.pad_h < s.kh && s.pad_w < s.kw, "conv2d error: the padding must be smaller than the kernel");
  ERROR_CHECK(s.kh - s.pad_h <= s.h + s.pad_h && s.kw - s.pad_w <= s.w + s.pad_w, "conv2d error: the kernel exceeds the padded image");
  // (sizes by division: no product is formed before the GPU layer has checked it)
  ERROR_CHECK(m_size % s.n_img == 0 && m_size / s.n_img % s.c_in == 0 && m_size / s.n_img / s.c_in % s.h == 0 &&
                  m_size / s.n_img / s.c_in / s.h == s.w,
              "conv2d error: Size mismatch! (the CipherText must hold n_img * c_in * h * w elements)");
  const std::size_t ws = w.getSize();
  ERROR_CHECK(ws > 0 && ws % s.c_out == 0 && ws / s.c_out % s.c_in == 0 && ws / s.c_out / s.c_in % s.kh == 0 &&
                  ws / s.c_out / s.c_in / s.kh == s.kw,
              "conv2d error: Size mismatch! (the filters must hold c_out * c_in * kh * kw elements)");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  if (!w.isDeviceResident())
    for (const auto& e : w.m_texts) ERROR_CHECK(!e.isNegative(), "conv2d error: negative plaintext");
  const int ebits = std::max(1, w.maxBitsHint());
  const int ew = w.isDeviceResident() ? w.m_dev->words : detail::words_for_bits(ebits);
  auto dx = deviceBatch(W, &nsq), dw = w.deviceBatch(ew);
  const pgpu_conv2d_shape shape{s.n_img, s.c_in, s.h, s.w, s.c_out, s.kh, s.kw, s.stride_h, s.stride_w, s.pad_h, s.pad_w};
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_conv2d(m_pk->device()->h, dx->h, dw->h, &shape, ebits, &o), "conv2d");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

CipherText CipherText::signedConvMap(const std::vector<int64_t>& w, const ext::Conv2dShape& s) const {
  ERROR_CHECK(m_size > 0, "conv2dSigned error: empty CipherText");
  ERROR_CHECK(s.n_img > 0 && s.c_in > 0 && s.h > 0 && s.w > 0 && s.c_out > 0 && s.kh > 0 && s.kw > 0 && s.stride_h > 0 && s.stride_w > 0,
              "conv2dSigned error: every dimension and stride must be positive");
  ERROR_CHECK(s.pad_h < s.kh && s.pad_w < s.kw, "conv2dSigned error: the padding must be smaller than the kernel");
  ERROR_CHECK(s.kh - s.pad_h <= s.h + s.pad_h && s.kw - s.pad_w <= s.w + s.pad_w, "conv2dSigned error: the kernel exceeds the padded image");
  // (sizes by division: no product is formed before the GPU layer has checked it)
  ERROR_CHECK(m_size % s.n_img == 0 && m_size / s.n_img % s.c_in == 0 && m_size / s.n_img / s.c_in % s.h == 0 &&
                  m_size / s.n_img / s.c_in / s.h == s.w,
              "conv2dSigned error: Size mismatch! (the CipherText must hold n_img * c_in * h * w elements)");
  const std::size_t ws = w.size();
  ERROR_CHECK(ws > 0 && ws % s.c_out == 0 && ws / s.c_out % s.c_in == 0 && ws / s.c_out / s.c_in % s.kh == 0 &&
                  ws / s.c_out / s.c_in / s.kh == s.kw,
              "conv2dSigned error: Size mismatch! (the filters must hold c_out * c_in * kh * kw elements)");
  const BigNumber& nsq = *(m_pk->getNSQ());
  const int W = detail::words_for_bits(nsq.BitSize());
  std::vector<uint64_t> words;
  const int ebits = detail::signed_weight_words(w, &words);
  auto dx = deviceBatch(W, &nsq), dw = detail::DeviceBatch::upload(words, words.size(), 1);
  const pgpu_conv2d_shape shape{s.n_img, s.c_in, s.h, s.w, s.c_out, s.kh, s.kw, s.stride_h, s.stride_w, s.pad_h, s.pad_w};
  pgpu_batch* o = nullptr;
  IPCL_GPU_CHECK(pgpu_batch_ct_conv2d_signed(m_pk->device()->h, dx->h, dw->h, &shape, ebits, &o), "conv2dSigned");
  return CipherText(m_pk, detail::DeviceBatch::adopt(o));
}

namespace ext {

static Conv2dShape conv1d_shape(std::size_t n_seq, std::size_t c_in, std::size_t len, std::size_t c_out, std::size_t k,
                                std::size_t stride, std::size_t pad) {
  Conv2dShape s;
  s.n_img = n_seq;
  s.c_in = c_in;
  s.w = len;
  s.c_out = c_out;
  s.kw = k;
  s.stride_w = stride;
  s.pad_w = pad;
  return s;
}

CipherText conv2d(const PlainText& w, const CipherText& x, const Conv2dShape& shape) { return x.convMap(w, shape); }
CipherText conv1d(const PlainText& w, const CipherText& x, std::size_t n_seq, std::size_t c_in, std::size_t len,
                  std::size_t c_out, std::size_t k, std::size_t stride, std::size_t pad) {
  return conv2d(w, x, conv1d_shape(n_seq, c_in, len, c_out, k, stride, pad));
}
CipherText conv2dSigned(const std::vector<int64_t>& w, const CipherText& x, const Conv2dShape& shape) { return x.signedConvMap(w, shape); }
CipherText conv1dSigned(const std::vector<int64_t>& w, const CipherText& x, std::size_t n_seq, std::size_t c_in, std::size_t len,
                        std::size_t c_out, std::size_t k, std::size_t stride, std::size_t pad) {
  return conv2dSigned(w, x, conv1d_shape(n_seq, c_in, len, c_out, k, stride, pad));
}

}  // namespace ext
}  // namespace ipcl
