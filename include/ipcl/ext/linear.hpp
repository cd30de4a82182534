// ipcl::ext -- linear maps on encrypted vectors (an extension: the reference has CT + CT, CT + PT and CT * PT only; this
// header is not part of ipcl.hpp).
//
//   matVec(w, rows, x)   y[i] = sum_j w[i*cols + j] * x[j]   under the encryption, cols = x.getSize():
//                        Y[i] = prod_j X[j]^w[i][j] mod n^2 -- an encrypted linear layer, a weighted aggregate
//   dot(w, x)            the rows = 1 case
//   matVecBucket(w, rows, x)
//                        matVec by the bucket method, the same arguments, errors and result bit for bit: for few rows over
//                        very many columns, or weights of any width (a signed weight passed as w mod n).  One
//                        pgpu_batch_ct_matvec_bucket call: no window tables -- per window of c bits the columns that
//                        share a digit are multiplied into a bucket, the buckets reduced by running products, the
//                        windows combined by Horner; the weights are read on the host.  matVec and dot never route here.
//   matMul(w, rows, x, n_vec, transposed = false)
//                        the same map for n_vec vectors at once, cols = x.getSize() / n_vec: x read as [n_vec][cols] and
//                        the result as [n_vec][rows], Y[v][i] = prod_j X[v][j]^w[i][j] mod n^2 (Y = X * W^T: a linear layer
//                        applied to a minibatch); transposed: x read as [cols][n_vec], the result as [rows][n_vec]
//                        (Y = W * X: a per-class gradient X^T * D).  One pgpu_batch_ct_matmul call: the matVec schedule
//                        per output, the vectors walked in tiles whose window tables share one block.  n_vec = 1 is matVec.
//   matVecSigned(w, rows, x) / dotSigned(w, x) / matMulSigned(w, rows, x, n_vec, transposed = false)
//                        matVec, dot and matMul for SIGNED weights, given as int64_t: Y[i] = prod_j X[j]^w[i][j] mod n^2 with
//                        X[j]^-1 for the negative ones, i.e. y = w * x mod n for a real linear layer, regression or filter.
//                        One pgpu_batch_ct_matvec_signed / pgpu_batch_ct_matmul_signed call: the inverses of x from ONE
//                        modular inversion, window tables over [x ; x^-1], Booth digits of the weights -- the cost of the
//                        unsigned call plus three products per element, where w mod n costs a key-width exponent and
//                        subtract(matVec(w+, x), matVec(w-, x)) two calls.  The weights travel in the smallest
//                        two's-complement width that holds every one.  Errors like matVec's (no "negative plaintext"
//                        one); an x that holds a non-unit modulo n^2 -- no ciphertext -- is a std::runtime_error.
//   sparseMatVec(row_ptr, col_idx, w, x)
//                        the same map with the plaintext matrix in CSR form, rows = row_ptr.size() - 1:
//                        Y[i] = prod_{ row_ptr[i] <= t < row_ptr[i+1] } X[col_idx[t]]^w[t] mod n^2 -- a neighbourhood
//                        aggregation over a graph, a sparse or pruned layer, a convolution as a banded matrix, a weighted
//                        group-by (a convolution proper has its own call: ipcl/ext/conv.hpp, conv2d -- no index list, no
//                        replicated weights, the images walked in tiles).  w holds the row_ptr.back() weights in CSR order.  Entries of a row need not be sorted, a
//                        column named twice contributes twice, an empty row yields an encryption of 0 (the ciphertext 1).
//                        One pgpu_batch_ct_spmv call: the window tables of the x[j] shared by all rows, the squarings
//                        shared by the terms of a chain of a row.
//   sparseMatVecSigned(row_ptr, col_idx, w, x)
//                        sparseMatVec for SIGNED weights, given as int64_t in CSR order (a graph Laplacian, a pruned layer):
//                        X[col_idx[t]]^-1 for the negative ones; a column named twice with weights a and -a contributes
//                        nothing.  One pgpu_batch_ct_spmv_signed call: the inverses of ALL of x from one modular
//                        inversion -- an element of x that is no unit is a std::runtime_error also where no entry names
//                        its column --, window tables over [x ; x^-1], Booth digits of the weights.  Widths and errors
//                        as matVecSigned's.
//   weightedSum(xs, w)   y[i] = sum_k w[k] * xs[k][i] under the encryption, ACROSS K CipherTexts of one size with one
//                        plaintext weight per CipherText: Y[i] = prod_k X_k[i]^w[k] mod n^2 -- a federated average over K
//                        clients' encrypted vectors.  A zero weight contributes nothing; all weights zero yield
//                        encryptions of 0 (the ciphertext 1).  One pgpu_batch_ct_weighted_sum call: one bit-serial
//                        schedule for all elements, the squarings shared by the K terms, no intermediate CipherText.
//   sum(xs)              the case of every weight 1
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
#include <cstdint>
#include <vector>

#include "ipcl/ciphertext.hpp"
#include "ipcl/plaintext.hpp"

namespace ipcl {
namespace ext {

CipherText matVec(const PlainText& w, std::size_t rows, const CipherText& x);
CipherText dot(const PlainText& w, const CipherText& x);
CipherText matVecBucket(const PlainText& w, std::size_t rows, const CipherText& x);
CipherText matMul(const PlainText& w, std::size_t rows, const CipherText& x, std::size_t n_vec, bool transposed = false);
CipherText matVecSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x);
CipherText dotSigned(const std::vector<int64_t>& w, const CipherText& x);
CipherText matMulSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x, std::size_t n_vec,
                        bool transposed = false);
CipherText sparseMatVec(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx, const PlainText& w,
                        const CipherText& x);
CipherText sparseMatVecSigned(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                              const std::vector<int64_t>& w, const CipherText& x);
CipherText weightedSum(const std::vector<CipherText>& xs, const PlainText& w);
CipherText sum(const std::vector<CipherText>& xs);

}  // namespace ext
}  // namespace ipcl
#endif  // PAILLIERCRYPTOLIB_AMD_IPCL_EXT_LINEAR_HPP_
