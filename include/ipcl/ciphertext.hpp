// pailliercryptolib_amd -- CipherText (reference ipcl/include/ipcl/ciphertext.hpp:16-75).
#ifndef PAILLIERCRYPTOLIB_AMD_IPCL_CIPHERTEXT_HPP_
#define PAILLIERCRYPTOLIB_AMD_IPCL_CIPHERTEXT_HPP_

#include <memory>
#include <vector>

#include "ipcl/plaintext.hpp"
#include "ipcl/pub_key.hpp"
#include "ipcl/utils/util.hpp"

namespace ipcl {

class CipherText;
namespace ext {   // include/ipcl/ext/linear.hpp
CipherText matVec(const PlainText& w, std::size_t rows, const CipherText& x);
CipherText matVecBucket(const PlainText& w, std::size_t rows, const CipherText& x);
CipherText matMul(const PlainText& w, std::size_t rows, const CipherText& x, std::size_t n_vec, bool transposed);
CipherText sparseMatVec(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx, const PlainText& w,
                        const CipherText& x);
CipherText weightedSum(const std::vector<CipherText>& xs, const PlainText& w);
CipherText sum(const std::vector<CipherText>& xs);
CipherText matVecSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x);
CipherText matMulSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x, std::size_t n_vec, bool transposed);
CipherText sparseMatVecSigned(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                              const std::vector<int64_t>& w, const CipherText& x);
struct Conv2dShape;   // include/ipcl/ext/conv.hpp
CipherText conv2d(const PlainText& w, const CipherText& x, const Conv2dShape& shape);
CipherText conv2dSigned(const std::vector<int64_t>& w, const CipherText& x, const Conv2dShape& shape);
// include/ipcl/ext/aggregate.hpp
CipherText segmentSum(const CipherText& x, const std::vector<uint32_t>& ids, std::size_t n_segments, std::size_t groups);
CipherText segmentScan(const CipherText& x, std::size_t seg_len, bool reverse);
CipherText packSlots(const CipherText& x, std::size_t seg_len, std::size_t slot_bits);
// include/ipcl/ext/arith.hpp
CipherText negate(const CipherText& x);
CipherText subtract(const CipherText& a, const CipherText& b);
// include/ipcl/ext/index.hpp
CipherText gather(const std::vector<const CipherText*>& xs, const std::vector<uint64_t>& idx);
CipherText concat(const std::vector<const CipherText*>& xs);
CipherText slice(const CipherText& x, std::size_t start, std::size_t count, std::size_t step);
}

class CipherText : public BaseText {
 public:
  CipherText() = default;
  ~CipherText() = default;
  CipherText(const PublicKey& pk, const uint32_t& n);
  CipherText(const PublicKey& pk, const std::vector<uint32_t>& n_v);
  CipherText(const PublicKey& pk, const BigNumber& bn);
  CipherText(const PublicKey& pk, const std::vector<BigNumber>& bn_vec);
  CipherText(const CipherText& ct) = default;
  CipherText& operator=(const CipherText& other) = default;

  CipherText operator+(const CipherText& other) const;  // CT+CT: batched modmul mod n^2 on the GPU
  CipherText operator+(const PlainText& other) const;   // CT+PT
  CipherText operator*(const PlainText& other) const;   // CT*PT: batched modexp on the GPU

  CipherText getCipherText(const size_t& idx) const;
  std::shared_ptr<PublicKey> getPubKey() const;
  // (a text whose current copy is the device's is rotated there -- one pgpu_batch_gather -- and the result stays resident;
  // same checks, messages and values as the host path, which a text with a current host copy still takes, and every text
  // on a pool of more than one GPU, where the gather is not available)
  CipherText rotate(int shift) const;

  void save(serializer::OutputArchive& ar) const;   // reference ciphertext.hpp:69-74: base, "pk"
  void load(serializer::InputArchive& ar);

 private:
  friend class PublicKey;
  friend CipherText ext::matVec(const PlainText& w, std::size_t rows, const CipherText& x);
  CipherText linearMap(const PlainText& w, std::size_t rows) const;   // prod_j this[j]^w[i][j]: csrc/host/linear.cpp
  friend CipherText ext::matVecBucket(const PlainText& w, std::size_t rows, const CipherText& x);
  CipherText linearMapBucket(const PlainText& w, std::size_t rows) const;   // the same by the bucket method: csrc/host/linear.cpp
  friend CipherText ext::matMul(const PlainText& w, std::size_t rows, const CipherText& x, std::size_t n_vec, bool transposed);
  // prod_j this(v, j)^w[i][j] for the n_vec vectors this holds: csrc/host/linear.cpp
  CipherText linearMapBatch(const PlainText& w, std::size_t rows, std::size_t n_vec, bool transposed) const;
  friend CipherText ext::sparseMatVec(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                                      const PlainText& w, const CipherText& x);
  // prod_t this[col_idx[t]]^w[t] over the CSR entries t of every row: csrc/host/linear.cpp
  CipherText sparseLinearMap(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                             const PlainText& w) const;
  friend CipherText ext::weightedSum(const std::vector<CipherText>& xs, const PlainText& w);
  friend CipherText ext::sum(const std::vector<CipherText>& xs);
  // prod_k xs[k][i]^w[k] (w == null: every weight 1), one weight per CipherText: csrc/host/linear.cpp
  static CipherText weightedSumMap(const std::vector<CipherText>& xs, const PlainText* w);
  friend CipherText ext::matVecSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x);
  friend CipherText ext::matMulSigned(const std::vector<int64_t>& w, std::size_t rows, const CipherText& x, std::size_t n_vec,
                                      bool transposed);
  // prod_j this(v, j)^w[i][j] for signed w (n_vec == 0: the matvec call, this one vector): csrc/host/linear.cpp
  CipherText signedLinearMap(const std::vector<int64_t>& w, std::size_t rows, std::size_t n_vec, bool transposed) const;
  friend CipherText ext::sparseMatVecSigned(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                                            const std::vector<int64_t>& w, const CipherText& x);
  // prod_t this[col_idx[t]]^w[t] over the CSR entries t of every row, for signed w: csrc/host/linear.cpp
  CipherText signedSparseLinearMap(const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
                                   const std::vector<int64_t>& w) const;
  friend CipherText ext::conv2d(const PlainText& w, const CipherText& x, const ext::Conv2dShape& shape);
  friend CipherText ext::conv2dSigned(const std::vector<int64_t>& w, const CipherText& x, const ext::Conv2dShape& shape);
  // the same for signed w: csrc/host/conv.cpp
  CipherText signedConvMap(const std::vector<int64_t>& w, const ext::Conv2dShape& shape) const;
  // prod_{ci,ky,kx} this(n, ci, oy*sh + ky - ph, ox*sw + kx - pw)^w[co][ci][ky][kx]: csrc/host/conv.cpp
  CipherText convMap(const PlainText& w, const ext::Conv2dShape& shape) const;
  friend CipherText ext::segmentSum(const CipherText& x, const std::vector<uint32_t>& ids, std::size_t n_segments,
                                    std::size_t groups);
  // prod_{j: ids[g][j] == s} this[j]: csrc/host/aggregate.cpp
  CipherText segmentMap(const std::vector<uint32_t>& ids, std::size_t n_segments, std::size_t groups) const;
  friend CipherText ext::segmentScan(const CipherText& x, std::size_t seg_len, bool reverse);
  // prod_{u <= t} this[r][u] (reverse: u >= t), this read as [m_size / seg_len][seg_len]: csrc/host/aggregate.cpp
  CipherText segmentScanMap(std::size_t seg_len, bool reverse) const;
  friend CipherText ext::packSlots(const CipherText& x, std::size_t seg_len, std::size_t slot_bits);
  // prod_t this[r][t]^(2^(slot_bits t)), this read as [m_size / seg_len][seg_len]: csrc/host/aggregate.cpp
  CipherText packMap(std::size_t seg_len, std::size_t slot_bits) const;
  friend CipherText ext::negate(const CipherText& x);
  friend CipherText ext::subtract(const CipherText& a, const CipherText& b);
  // this[i] * b[i]^-1 mod n^2 (b == null: this[i]^-1), all inverses from one modular inversion: csrc/host/arith.cpp
  CipherText inverseMap(const CipherText* b) const;
  friend CipherText ext::gather(const std::vector<const CipherText*>& xs, const std::vector<uint64_t>& idx);
  friend CipherText ext::concat(const std::vector<const CipherText*>& xs);
  friend CipherText ext::slice(const CipherText& x, std::size_t start, std::size_t count, std::size_t step);
  // rows of the texts xs put end to end, re-indexed on the device: idx != null: row (*idx)[i]; step == 0: all of them
  // (concat); else rows start, start + step, ..., count of them: csrc/host/index.cpp
  static CipherText indexMap(const char* what, const std::vector<const CipherText*>& xs, const std::vector<uint64_t>* idx,
                             std::size_t start, std::size_t count, std::size_t step);
  CipherText(const PublicKey& pk, std::shared_ptr<detail::DeviceBatch> dev);
  CipherText(std::shared_ptr<PublicKey> pk, std::shared_ptr<detail::DeviceBatch> dev);
  std::shared_ptr<PublicKey> m_pk;
};

}  // namespace ipcl
#endif  // PAILLIERCRYPTOLIB_AMD_IPCL_CIPHERTEXT_HPP_
