// ipcl::ext -- linear maps on encrypted vectors (an extension: the reference has CT + CT, CT + PT and CT * PT only; this
// header is not part of ipcl.hpp).
//
//   matVec(w, rows, x)   y[i] = sum_j w[i*cols + j] * x[j]   under the encryption, cols = x.getSize():
//                        Y[i] = prod_j X[j]^w[i][j] mod n^2 -- an encrypted linear layer, a weighted aggregate
//   dot(w, x)            the rows = 1 case
//
// w: rows*cols non-negative plaintext weights, row-major (negative numbers have no encoding in the reference either; pass
// w mod n).  One fused launch sequence on the GPU (pgpu_batch_ct_matvec: window tables of the x[j] shared by all rows, the
// squarings shared by all terms of a row) instead of rows*cols CT * PT terms and a tree of CT + CT.  A CipherText that is
// already device-resident is used in place; the result stays resident like the results of the operators.
// Errors are reported like the operators': a std::runtime_error from ERROR_CHECK (size mismatch, empty operands,
// negative weights) or from the GPU layer (keys beyond 3072 bits have no such kernel: no fall-back).
#ifndef PAILLIERCRYPTOLIB_AMD_IPCL_EXT_LINEAR_HPP_
#define PAILLIERCRYPTOLIB_AMD_IPCL_EXT_LINEAR_HPP_

#include <cstddef>

#include "ipcl/ciphertext.hpp"
#include "ipcl/plaintext.hpp"

namespace ipcl {
namespace ext {

CipherText matVec(const PlainText& w, std::size_t rows, const CipherText& x);
CipherText dot(const PlainText& w, const CipherText& x);

}  // namespace ext
}  // namespace ipcl
#endif  // PAILLIERCRYPTOLIB_AMD_IPCL_EXT_LINEAR_HPP_
