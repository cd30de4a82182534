// ipcl::ext -- 2-D convolution on encrypted images (an extension: the reference has CT + CT, CT + PT and CT * PT only; this
// header is not part of ipcl.hpp).
//
//   conv2d(w, x, shape)  x read as [n_img][c_in][h][w], the plaintext filters w as [c_out][c_in][kh][kw]; with
//                        oh = (h + 2*pad_h - kh) / stride_h + 1 (floor), ow likewise, the result holds
//                        n_img*c_out*oh*ow ciphertexts laid out [n_img][c_out][oh][ow],
//                        Y[n][co][oy][ox] = prod_{ci,ky,kx} X[n][ci][oy*stride_h + ky - pad_h][ox*stride_w + kx - pad_w]^w[co][ci][ky][kx] mod n^2
//                        -- a tap outside the image contributes nothing (zero padding): the decryption is the
//                        cross-correlation a convolutional layer computes, mod n.  An all-zero filter yields encryptions of
//                        0 (the ciphertext 1).  A second layer takes the result as it is.  One pgpu_batch_ct_conv2d call:
//                        the window tables of a tile of whole images built once and shared by every output that reads a
//                        pixel, table rows addressed by arithmetic on the output position -- no column numbers, no
//                        replicated weights (what sparseMatVec of linear.hpp needs for the same map).
//   conv1d(w, x, n_seq, c_in, len, c_out, k, stride = 1, pad = 0)
//                        the h = kh = 1 case: x read as [n_seq][c_in][len], w as [c_out][c_in][k]
//   conv2dSigned(w, x, shape) / conv1dSigned(w, x, n_seq, c_in, len, c_out, k, stride = 1, pad = 0)
//                        conv2d and conv1d for SIGNED filters, given as int64_t in the same [c_out][c_in][kh][kw] order:
//                        X^-1 for the negative taps, i.e. the cross-correlation with a real CNN filter, mod n.  One
//                        pgpu_batch_ct_conv2d_signed call: the inverses of x from ONE modular inversion, window tables
//                        over [x ; x^-1], Booth digits of the filters -- the cost of conv2d plus three products per
//                        pixel, where w mod n costs a key-width exponent and subtract(conv2d(w+, x), conv2d(w-, x)) two
//                        calls.  The filters travel in the smallest two's-complement width that holds every tap.  Errors
//                        like conv2d's (no "negative plaintext" one); an x that holds a non-unit modulo n^2 -- no
//                        ciphertext -- is a std::runtime_error.
//
// Sum pooling is a reshape by the caller: n_img' = n_img*c, c_in = c_out = 1, all-ones taps, stride equal to the kernel.
// Not offered: dilation, groups, a bias (add it with CipherText::operator+(PlainText)), tiling inside one image.
// w: non-negative plaintext weights (negative numbers have no encoding in the reference either; pass w mod n).  A
// CipherText that is already device-resident is used in place; the result stays resident like the results of the operators.
// Errors are reported like the operators': a std::runtime_error from ERROR_CHECK (size mismatch, empty operands, a shape
// without output, negative weights) or from the GPU layer (keys beyond 3072 bits have no such kernel: no fall-back).
#ifndef PAILLIERCRYPTOLIB_AMD_IPCL_EXT_CONV_HPP_
#define PAILLIERCRYPTOLIB_AMD_IPCL_EXT_CONV_HPP_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ipcl/ciphertext.hpp"
#include "ipcl/plaintext.hpp"

namespace ipcl {
namespace ext {

struct Conv2dShape {
  std::size_t n_img = 1, c_in = 1, h = 1, w = 1, c_out = 1, kh = 1, kw = 1;
  std::size_t stride_h = 1, stride_w = 1, pad_h = 0, pad_w = 0;
  std::size_t outHeight() const { return (h + 2 * pad_h - kh) / stride_h + 1; }
  std::size_t outWidth() const { return (w + 2 * pad_w - kw) / stride_w + 1; }
};

CipherText conv2d(const PlainText& w, const CipherText& x, const Conv2dShape& shape);
CipherText conv1d(const PlainText& w, const CipherText& x, std::size_t n_seq, std::size_t c_in, std::size_t len,
                  std::size_t c_out, std::size_t k, std::size_t stride = 1, std::size_t pad = 0);
CipherText conv2dSigned(const std::vector<int64_t>& w, const CipherText& x, const Conv2dShape& shape);
CipherText conv1dSigned(const std::vector<int64_t>& w, const CipherText& x, std::size_t n_seq, std::size_t c_in, std::size_t len,
                        std::size_t c_out, std::size_t k, std::size_t stride = 1, std::size_t pad = 0);

}  // namespace ext
}  // namespace ipcl
#endif  // PAILLIERCRYPTOLIB_AMD_IPCL_EXT_CONV_HPP_
