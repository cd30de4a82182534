// ipcl::ext -- re-indexing of ciphertexts on the device (an extension: the reference's own re-ordering calls,
// CipherText::rotate / getChunk / getCipherText, index host vectors; this header is not part of ipcl.hpp).
//
//   gather(x, idx)        y[i] = x[idx[i]]; indices in any order, repeats allowed; kGatherOne yields the ciphertext 1, an
//                         encryption of 0 (zero padding, a missing value)
//   gather(xs, idx)       the same over the texts xs put end to end (the same text may be named twice)
//   concat(xs)            the texts xs put end to end
//   slice(x, start, count, step)   y[i] = x[start + i * step], count elements (step = 1: a contiguous part; the column of
//                         an [n_vec][cols] text: start = column, step = cols, count = n_vec)
//
// -- a minibatch drawn from a resident encrypted data set, K clients' vectors stacked before ext::segmentSum, a layer's
// output split or permuted before the next layer.  One pgpu_batch_gather / _concat / _slice call: rows move as bytes, at
// memory speed.  A CipherText that is already device-resident is used in place; a host-only one is uploaded, as the other
// ext calls do; the result stays resident like the results of the operators.  There is no conversion inside these calls:
// texts that are resident results (of encrypt, of the operators) and texts built from host values do not mix in one call
// -- pass the host-built text through any operator first, or gather before mixing.
// Errors are reported like the operators': a std::runtime_error from ERROR_CHECK (no or empty texts, an index out of
// range, a slice past the end, two different keys) or from the GPU layer (texts of different layouts, pools of more than
// one GPU).
#ifndef PAILLIERCRYPTOLIB_AMD_IPCL_EXT_INDEX_HPP_
#define PAILLIERCRYPTOLIB_AMD_IPCL_EXT_INDEX_HPP_

#include <cstdint>
#include <vector>

#include "ipcl/ciphertext.hpp"

namespace ipcl {
namespace ext {

constexpr uint64_t kGatherOne = ~0ull;
CipherText gather(const CipherText& x, const std::vector<uint64_t>& idx);
CipherText gather(const std::vector<const CipherText*>& xs, const std::vector<uint64_t>& idx);
CipherText concat(const std::vector<const CipherText*>& xs);
CipherText slice(const CipherText& x, std::size_t start, std::size_t count, std::size_t step = 1);

}  // namespace ext
}  // namespace ipcl
#endif  // PAILLIERCRYPTOLIB_AMD_IPCL_EXT_INDEX_HPP_
