"""Host-side Python mirror of the hot-path seam: batched modExp / modMul on the GPU.

Mirrors ipcl::modExp(vector, vector, vector) (reference ipcl/mod_exp.cpp:680-737) and
CipherText::raw_add (ciphertext.cpp:135-141) over numpy / torch buffers.  Every function calls
the C-ABI (include/pgpu.h); nothing here computes on the CPU.
"""
import ctypes

import numpy as np

from . import _capi
from .limbs import ints_to_limbs, limbs_to_ints

_initialized = False


def initialize(device=None):
    """ipcl::initializeContext counterpart (utils/context.cpp:40-55): bind this process to one GPU."""
    global _initialized
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; if torch is going to
    # share this process it must bring the runtime up first (the library then binds to the same one).
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    L = _capi.lib()
    _capi.check(L.pgpu_init(-1 if device is None else int(device)))
    _initialized = True


def terminate():
    global _initialized
    if _capi._lib is not None:
        _capi.lib().pgpu_shutdown()
    _initialized = False


def _ensure():
    if not _initialized:
        initialize()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def mod_exp_limbs(base, exp, mod, exp_bits=None):
    """base: [n, W] or [1, W] (shared); exp: [n, E] or [1, E] (shared); mod: [W] -> out [n, W]."""
    _ensure()
    base = np.ascontiguousarray(base, dtype=np.uint64)
    exp = np.ascontiguousarray(exp, dtype=np.uint64)
    mod = np.ascontiguousarray(mod, dtype=np.uint64).reshape(-1)
    W = mod.shape[0]
    if base.ndim != 2 or exp.ndim != 2 or base.shape[1] != W:
        raise RuntimeError("modExp: input vector size error")
    n = max(base.shape[0], exp.shape[0])
    if base.shape[0] not in (1, n) or exp.shape[0] not in (1, n):
        raise RuntimeError("modExp: input vector size error")   # mod_exp.cpp:452-454
    if exp_bits is None:
        exp_bits = max((int(v).bit_length() for v in limbs_to_ints(exp)), default=0)
    out = np.empty((n, W), dtype=np.uint64)
    bs = W if base.shape[0] == n else 0            # stride 0 == one shared value
    es = exp.shape[1] if exp.shape[0] == n else 0
    _capi.check(_capi.lib().pgpu_modexp(_ptr(base), bs, _ptr(exp), es, exp.shape[1], int(exp_bits),
                                        _ptr(mod), W, _ptr(out), n))
    return out


def mod_exp(base, exp, mod):
    """ipcl::modExp over Python ints.  base/exp: lists (len n or 1); mod: one int (shared)."""
    W = (int(mod).bit_length() + 63) // 64
    E = max(1, (max((int(e).bit_length() for e in exp), default=1) + 63) // 64)
    out = mod_exp_limbs(ints_to_limbs([b % (1 << (64 * W)) for b in base], W), ints_to_limbs(exp, E),
                        ints_to_limbs([mod], W)[0])
    return limbs_to_ints(out)


def mod_mul_limbs(a, b, mod):
    """a: [n, W]; b: [n, W] or [1, W] (scalar broadcast); mod: [W]."""
    _ensure()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    mod = np.ascontiguousarray(mod, dtype=np.uint64).reshape(-1)
    W = mod.shape[0]
    n = a.shape[0]
    if a.shape[1] != W or b.shape[1] != W or b.shape[0] not in (1, n):
        raise RuntimeError("CT + CT error: Size mismatch!")
    out = np.empty((n, W), dtype=np.uint64)
    bstride = W if b.shape[0] == n else 0
    _capi.check(_capi.lib().pgpu_modmul(_ptr(a), _ptr(b), bstride, _ptr(mod), W, _ptr(out), n))
    return out


def mod_mul(a, b, mod):
    W = (int(mod).bit_length() + 63) // 64
    out = mod_mul_limbs(ints_to_limbs(a, W), ints_to_limbs(b, W), ints_to_limbs([mod], W)[0])
    return limbs_to_ints(out)


class PublicKey:
    """Host-side mirror of ipcl::PublicKey's encrypt path (reference ipcl/pub_key.cpp:82-129).

    ``hs`` set -> DJN scheme (obfuscator hs^r); otherwise r^n.  Randomness is supplied by the
    caller (like ``setRandom``, pub_key.cpp:92-95) so results are reproducible.
    """

    def __init__(self, n, bits=None, hs=None):
        _ensure()
        self.n = int(n)
        self.bits = int(bits) if bits is not None else self.n.bit_length()
        self.n_words = (self.n.bit_length() + 63) // 64
        self.hs = None if hs is None else int(hs)
        self.nsq = self.n * self.n
        self._h = ctypes.c_void_p()
        n_l = ints_to_limbs([self.n], self.n_words)
        hs_l = None if hs is None else ints_to_limbs([self.hs], 2 * self.n_words)
        _capi.check(_capi.lib().pgpu_pubkey_create(_ptr(n_l), self.n_words,
                                                   None if hs_l is None else _ptr(hs_l),
                                                   ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _capi._lib is not None:
            _capi._lib.pgpu_pubkey_destroy(self._h)
            self._h = None

    def encrypt_limbs(self, m, r, r_bits=None):
        """m: [n, Wm] uint64, r: [n, Wr] uint64 -> ciphertexts [n, 2*n_words]."""
        m = np.ascontiguousarray(m, dtype=np.uint64)
        r = np.ascontiguousarray(r, dtype=np.uint64)
        if m.shape[0] == 0:
            raise RuntimeError("encrypt: Cannot encrypt empty PlainText")     # pub_key.cpp:116
        if r.shape[0] != m.shape[0]:
            raise RuntimeError("modExp: input vector size error")             # mod_exp.cpp:452-454
        if r_bits is None:
            r_bits = max(int(v).bit_length() for v in limbs_to_ints(r))
        out = np.empty((m.shape[0], 2 * self.n_words), dtype=np.uint64)
        _capi.check(_capi.lib().pgpu_paillier_encrypt(self._h, _ptr(m), m.shape[1], m.shape[1], _ptr(r),
                                                      r.shape[1], r.shape[1], int(r_bits), _ptr(out),
                                                      m.shape[0]))
        return out

    def encrypt(self, m, r):
        mw = max(1, (max(int(v).bit_length() for v in m) + 63) // 64) if len(m) else 1
        rw = max(1, (max(int(v).bit_length() for v in r) + 63) // 64) if len(r) else 1
        if len(m) == 0:
            raise RuntimeError("encrypt: Cannot encrypt empty PlainText")
        return limbs_to_ints(self.encrypt_limbs(ints_to_limbs(m, mw), ints_to_limbs(r, rw)))

    def _resident_call(self, operands, rows, call):
        """One aggregation call on resident batches: uploads every (ints, words per row) of ``operands``, runs
        ``call(L, handles, byref(out))`` -- the pgpu_batch_ct_* call, which returns its status -- downloads the
        rows x 2*n_words result and destroys every handle, whatever happened on the way."""
        L = _capi.lib()
        hs, ho = [], ctypes.c_void_p()
        try:
            arrays = [ints_to_limbs(vals, words) for vals, words in operands]
            for a in arrays:
                h = ctypes.c_void_p()
                _capi.check(L.pgpu_batch_upload(_ptr(a), a.shape[0], a.shape[1], a.shape[1], ctypes.byref(h)))
                hs.append(h)
            _capi.check(call(L, hs, ctypes.byref(ho)))
            out = np.empty((rows, 2 * self.n_words), dtype=np.uint64)
            _capi.check(L.pgpu_batch_download(ho, _ptr(out)))
        finally:
            for h in hs + [ho]:
                if h:
                    L.pgpu_batch_destroy(h)
        return limbs_to_ints(out)

    def _ct(self, x):
        return [int(v) for v in x], 2 * self.n_words

    @staticmethod
    def _signed_weights(flat, e_bits):
        """(e_bits, words, two's-complement values) of signed weights; e_bits None: the smallest width holding every one"""
        if e_bits is None:
            e_bits = max((v if v >= 0 else ~v).bit_length() + 1 for v in flat)
        ew = (int(e_bits) + 63) // 64
        return int(e_bits), ew, [v & ((1 << (64 * ew)) - 1) for v in flat]

    def matvec(self, x, w, e_bits=None, signed=False):
        """Encrypted matrix-vector product: x a list of ciphertexts (ints modulo n^2), w a plaintext matrix (a list of
        rows, or one flat row for a dot product) of non-negative ints -> the list of ciphertexts
        prod_j x[j]^w[i][j] mod n^2, i.e. encryptions of (w @ m) mod n.  One pgpu_batch_ct_matvec call on resident batches
        (a shared-table multi-exponentiation); there is no element-wise fall-back.
        signed=True: the weights may be negative; they are packed as two's complement in e_bits bits (default: the smallest
        width that holds every weight) and the one call is pgpu_batch_ct_matvec_signed (x^-1 by one batched inversion, a
        table over [x ; x^-1], Booth digits)."""
        rows = [list(r) for r in w] if len(w) and isinstance(w[0], (list, tuple)) else [list(w)]
        cols = len(x)
        if cols == 0 or not rows or any(len(r) != cols for r in rows):
            raise RuntimeError("matvec error: Size mismatch!")
        flat = [int(v) for r in rows for v in r]
        if signed:
            e_bits, ew, packed = self._signed_weights(flat, e_bits)
            return self._resident_call([self._ct(x), (packed, ew)], len(rows), lambda L, h, out:
                                       L.pgpu_batch_ct_matvec_signed(self._h, h[0], h[1], len(rows), e_bits, out))
        if min(flat) < 0:
            raise RuntimeError("matvec error: negative weights have no encoding (pass w mod n)")
        if e_bits is None:
            e_bits = max(1, max(v.bit_length() for v in flat))
        ew = (int(e_bits) + 63) // 64
        return self._resident_call([self._ct(x), (flat, ew)], len(rows), lambda L, h, out:
                                   L.pgpu_batch_ct_matvec(self._h, h[0], h[1], len(rows), int(e_bits), out))

    def matvec_bucket(self, x, w, e_bits=None):
        """The encrypted matrix-vector product of ``matvec`` by the bucket method: the same arguments, the same result
        bit for bit, for few rows over very many columns or weights of any width (a signed weight as w mod n).  One
        pgpu_batch_ct_matvec_bucket call on a resident batch -- the weights stay on the host, which cuts their digits;
        no window tables; there is no fall-back to ``matvec`` or to the element-wise route."""
        rows = [list(r) for r in w] if len(w) and isinstance(w[0], (list, tuple)) else [list(w)]
        cols = len(x)
        if cols == 0 or not rows or any(len(r) != cols for r in rows):
            raise RuntimeError("matvec error: Size mismatch!")
        flat = [int(v) for r in rows for v in r]
        if min(flat) < 0:
            raise RuntimeError("matvec error: negative weights have no encoding (pass w mod n)")
        if e_bits is None:
            e_bits = max(1, max(v.bit_length() for v in flat))
        ew = (int(e_bits) + 63) // 64
        wa = ints_to_limbs([v & ((1 << (64 * ew)) - 1) for v in flat], ew)
        return self._resident_call([self._ct(x)], len(rows), lambda L, h, out:
                                   L.pgpu_batch_ct_matvec_bucket(self._h, h[0], _ptr(wa), ew, len(rows), int(e_bits), out))

    def matmul(self, x, w, transposed=False, e_bits=None, signed=False):
        """Encrypted matrix product: x a list of n_vec lists of cols ciphertexts (ints modulo n^2), w a plaintext matrix
        (a list of rows of cols non-negative ints) -> a list of n_vec lists of rows ciphertexts, out[v][i] =
        prod_j x[v][j]^w[i][j] mod n^2, i.e. encryptions of (m @ w.T) mod n -- a linear layer applied to a minibatch.
        transposed: x a list of cols lists of n_vec ciphertexts, the result a list of rows lists of n_vec, out[i][v] =
        prod_j x[j][v]^w[i][j] mod n^2, i.e. encryptions of (w @ m) mod n.  One pgpu_batch_ct_matmul call on resident
        batches (the matvec's multi-exponentiation per output, the vectors walked in tiles); there is no element-wise
        fall-back.  signed=True: the weights may be negative, packed as for ``matvec``; one pgpu_batch_ct_matmul_signed
        call."""
        xs, rows = [list(r) for r in x], [list(r) for r in w]
        if not xs or not xs[0] or not rows or any(len(r) != len(xs[0]) for r in xs):
            raise RuntimeError("matmul error: Size mismatch!")
        n_vec, cols = (len(xs[0]), len(xs)) if transposed else (len(xs), len(xs[0]))
        if any(len(r) != cols for r in rows):
            raise RuntimeError("matmul error: Size mismatch!")
        flat = [int(v) for r in rows for v in r]
        call = _capi.lib().pgpu_batch_ct_matmul
        if signed:
            e_bits, ew, flat = self._signed_weights(flat, e_bits)
            call = _capi.lib().pgpu_batch_ct_matmul_signed
        else:
            if min(flat) < 0:
                raise RuntimeError("matmul error: negative weights have no encoding (pass w mod n)")
            if e_bits is None:
                e_bits = max(1, max(v.bit_length() for v in flat))
            ew = (int(e_bits) + 63) // 64
        out = self._resident_call([self._ct([c for r in xs for c in r]), (flat, ew)], n_vec * len(rows), lambda L, h, out:
                                  call(self._h, h[0], h[1], n_vec, len(rows), int(e_bits), 1 if transposed else 0, out))
        inner = n_vec if transposed else len(rows)
        return [out[k:k + inner] for k in range(0, len(out), inner)]

    def conv2d(self, x, w, stride=1, padding=0, e_bits=None, signed=False):
        """Encrypted 2-D convolution: x nested lists [n_img][C_in][H][W] of ciphertexts (ints modulo n^2), w nested lists
        [C_out][C_in][kh][kw] of ints (non-negative, or of either sign with signed=True), stride and padding an int or a (vertical, horizontal) pair -> nested
        lists [n_img][C_out][OH][OW] of ciphertexts, OH = (H + 2 pad_h - kh) // stride_h + 1, OW likewise,
        out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*stride_h + ky - pad_h][ox*stride_w + kx - pad_w]^w[co][ci][ky][kx]
        mod n^2 with taps outside the image left out (zero padding), i.e. encryptions of what
        torch.nn.functional.conv2d(m, w, stride=stride, padding=padding) computes, mod n.  One pgpu_batch_ct_conv2d call on
        resident batches (window tables per tile of images, addressed by the output position: no index list); there is
        no element-wise fall-back and none through ``spmv``.
        signed=False: a negative weight is an error (it has no encoding; pass w mod n), e_bits defaults to the widest weight.
        signed=True: a CNN filter as it is -- the weights are packed as two's complement in e_bits bits (default: the smallest
        width that holds every one) and the one call is pgpu_batch_ct_conv2d_signed (x^-1 by one batched inversion, a table
        over [x ; x^-1] per tile, Booth digits)."""
        def pair(v, what):
            p = (v, v) if isinstance(v, int) else tuple(v)
            if len(p) != 2 or any(int(q) != q or q < 0 for q in p):
                raise RuntimeError(f"conv2d error: {what} must be a non-negative int or a pair of them")
            return int(p[0]), int(p[1])
        (sh, sw), (ph, pw) = pair(stride, "stride"), pair(padding, "padding")
        try:
            xs = [[[list(row) for row in ch] for ch in img] for img in x]
            ws = [[[list(row) for row in ch] for ch in f] for f in w]
            n_img, c_in, h, wd = len(xs), len(xs[0]), len(xs[0][0]), len(xs[0][0][0])
            c_out, kh, kw = len(ws), len(ws[0][0]), len(ws[0][0][0])
        except (TypeError, IndexError):
            raise RuntimeError("conv2d error: Size mismatch! (x must be [n_img][C_in][H][W], w [C_out][C_in][kh][kw])") from None
        if not (n_img and c_in and h and wd and c_out and kh and kw) or \
                any(len(img) != c_in or any(len(ch) != h or any(len(row) != wd for row in ch) for ch in img) for img in xs) or \
                any(len(f) != c_in or any(len(ch) != kh or any(len(row) != kw for row in ch) for ch in f) for f in ws):
            raise RuntimeError("conv2d error: Size mismatch! (x must be [n_img][C_in][H][W], w [C_out][C_in][kh][kw])")
        if sh < 1 or sw < 1:
            raise RuntimeError("conv2d error: the stride must be positive")
        if ph >= kh or pw >= kw:
            raise RuntimeError("conv2d error: the padding must be smaller than the kernel")
        if kh > h + 2 * ph or kw > wd + 2 * pw:
            raise RuntimeError("conv2d error: the kernel exceeds the padded image")
        flat = [int(v) for f in ws for ch in f for row in ch for v in row]
        call = _capi.lib().pgpu_batch_ct_conv2d
        if signed:
            e_bits, ew, flat = self._signed_weights(flat, e_bits)
            call = _capi.lib().pgpu_batch_ct_conv2d_signed
        else:
            if min(flat) < 0:
                raise RuntimeError("conv2d error: negative weights have no encoding (pass w mod n)")
            if e_bits is None:
                e_bits = max(1, max(v.bit_length() for v in flat))
            ew = (int(e_bits) + 63) // 64
        oh, ow = (h + 2 * ph - kh) // sh + 1, (wd + 2 * pw - kw) // sw + 1
        shape = _capi.Conv2dShape(n_img, c_in, h, wd, c_out, kh, kw, sh, sw, ph, pw)
        cts = [c for img in xs for ch in img for row in ch for c in row]
        out = self._resident_call([self._ct(cts), (flat, ew)], n_img * c_out * oh * ow, lambda L, hd, o:
                                  call(self._h, hd[0], hd[1], ctypes.byref(shape), int(e_bits), o))
        it = iter(out)
        return [[[[next(it) for _ in range(ow)] for _ in range(oh)] for _ in range(c_out)] for _ in range(n_img)]

    def spmv(self, x, indptr, indices, w, e_bits=None, signed=False):
        """Encrypted sparse matrix-vector product: x a list of ciphertexts (ints modulo n^2), the plaintext matrix in CSR
        form -- indptr (rows + 1 offsets, starting at 0), indices (a column of x per entry), w (an int per
        entry: non-negative, or of either sign with signed=True) -> the list of ciphertexts prod_t x[indices[t]]^w[t] mod n^2 over the entries t of every row, i.e.
        encryptions of (A @ m) mod n; an empty row gives 1.  A weighted group-by SUM(v * x) GROUP BY id is the CSR with
        indices = argsort(ids, stable), w = v[indices], indptr = the running count of every id.  One pgpu_batch_ct_spmv
        call on resident batches (a shared-table multi-exponentiation per chain of a row); there is no element-wise
        fall-back.
        signed=False: a negative weight is an error (it has no encoding; pass w mod n), e_bits defaults to the widest weight.
        signed=True: a graph Laplacian as it is -- the weights are packed as two's complement in e_bits bits (default: the
        smallest width that holds every one) and the one call is pgpu_batch_ct_spmv_signed, which inverts EVERY element of x:
        a non-unit refuses the call also where no entry names its column."""
        indptr, indices, flat = [int(v) for v in indptr], [int(v) for v in indices], [int(v) for v in w]
        cols, rows = len(x), len(indptr) - 1
        if cols == 0 or rows < 1 or not flat or len(indices) != len(flat) or indptr[0] != 0 or indptr[-1] != len(flat):
            raise RuntimeError("spmv error: Size mismatch!")
        if any(b < a for a, b in zip(indptr, indptr[1:])):
            raise RuntimeError("spmv error: indptr must be non-decreasing")
        if min(indices) < 0 or max(indices) >= cols:
            raise RuntimeError("spmv error: a column index is not below len(x)")
        call = _capi.lib().pgpu_batch_ct_spmv
        if signed:
            e_bits, ew, flat = self._signed_weights(flat, e_bits)
            call = _capi.lib().pgpu_batch_ct_spmv_signed
        else:
            if min(flat) < 0:
                raise RuntimeError("spmv error: negative weights have no encoding (pass w mod n)")
            if e_bits is None:
                e_bits = max(1, max(v.bit_length() for v in flat))
            ew = (int(e_bits) + 63) // 64
        rp, ci = np.array(indptr, dtype=np.uint64), np.array(indices, dtype=np.uint32)
        return self._resident_call([self._ct(x), (flat, ew)], rows, lambda L, h, out:
                                   call(self._h, h[0], _ptr(rp), _ptr(ci), h[1], rows, int(e_bits), out))

    def weighted_sum(self, xs, w=None):
        """Encrypted weighted sum across K batches: xs a list of K lists of ciphertexts (ints modulo n^2), all of one
        length, w one non-negative int per LIST (None: all ones, the plain sum) -> the list of ciphertexts
        prod_k xs[k][i]^w[k] mod n^2, i.e. encryptions of sum_k w[k] * m_k[i] mod n -- a federated average over K
        clients' vectors.  A zero weight contributes 1; all weights zero give 1 everywhere.  One
        pgpu_batch_ct_weighted_sum call on resident batches (one bit-serial schedule shared by all elements); there is
        no element-wise fall-back."""
        K = len(xs)
        if K == 0 or len(xs[0]) == 0 or any(len(x) != len(xs[0]) for x in xs):
            raise RuntimeError("weighted sum error: Size mismatch!")
        wa = None
        if w is not None:
            flat = [int(v) for v in w]
            if len(flat) != K:
                raise RuntimeError("weighted sum error: Size mismatch! (one weight per batch)")
            if min(flat) < 0:
                raise RuntimeError("weighted sum error: negative weights have no encoding (pass w mod n)")
            ew = max(1, (max(v.bit_length() for v in flat) + 63) // 64)
            wa = ints_to_limbs(flat, ew)
        return self._resident_call([self._ct(x) for x in xs], len(xs[0]), lambda L, h, out:
                                   L.pgpu_batch_ct_weighted_sum(self._h, (ctypes.c_void_p * K)(*[v.value for v in h]), K,
                                                                _ptr(wa) if wa is not None else None,
                                                                wa.shape[1] if wa is not None else 0, out))

    @staticmethod
    def _sources(h):
        """the uploaded handles of a _resident_call as the `const pgpu_batch* const*` array of a several-source call"""
        return (ctypes.c_void_p * len(h))(*[v.value for v in h])

    def gather(self, x, idx):
        """Re-indexing on the device: x a list of ciphertexts (ints modulo n^2), or a list of such lists (the sources, put
        end to end), idx a list of positions in any order, repeats allowed; None is the ciphertext 1 (an encryption of 0:
        padding, a missing value) -> the list [x[i] for i in idx].  One pgpu_batch_gather call on resident batches (rows
        move as bytes, one launch); there is no host indexing behind it."""
        xs = [list(r) for r in x] if len(x) and isinstance(x[0], (list, tuple)) else [list(x)]
        total = sum(len(r) for r in xs)
        if total == 0 or any(len(r) == 0 for r in xs) or len(idx) == 0:
            raise RuntimeError("gather error: empty batch or empty index list")
        flat = [_capi.GATHER_ONE if v is None else int(v) for v in idx]
        if any(v < 0 or (v >= total and v != _capi.GATHER_ONE) for v in flat):
            raise RuntimeError("gather error: an index is not below the number of rows")
        ia = np.array(flat, dtype=np.uint64)
        return self._resident_call([self._ct(r) for r in xs], len(flat), lambda L, h, out:
                                   L.pgpu_batch_gather(self._sources(h), len(h), _ptr(ia), len(flat), out))

    def concat(self, xs):
        """xs a list of lists of ciphertexts (ints modulo n^2) -> the one list that holds them end to end, put together
        on the device: one pgpu_batch_concat call on resident batches (one device-to-device copy per source)."""
        xs = [list(r) for r in xs]
        if len(xs) == 0 or any(len(r) == 0 for r in xs):
            raise RuntimeError("concat error: empty batch")
        return self._resident_call([self._ct(r) for r in xs], sum(len(r) for r in xs), lambda L, h, out:
                                   L.pgpu_batch_concat(self._sources(h), len(h), out))

    def segment_sum(self, x, ids, n_segments):
        """Encrypted segmented sum: x a list of ciphertexts (ints modulo n^2), ids one flat list of segment numbers (one
        group) or a list of such lists (several groupings of the same x); None leaves an element out of that group ->
        for one group the list of n_segments ciphertexts prod_{j: ids[j] == s} x[j] mod n^2, i.e. encryptions of the
        per-segment sums mod n, for several groups all of them, group after group (an empty segment: 1).  One
        pgpu_batch_ct_segment_sum call on resident batches; there is no element-wise fall-back."""
        groups = [list(r) for r in ids] if len(ids) and isinstance(ids[0], (list, tuple)) else [list(ids)]
        cols, n_segments = len(x), int(n_segments)
        if cols == 0 or n_segments <= 0 or any(len(r) != cols for r in groups):
            raise RuntimeError("segment sum error: Size mismatch!")
        flat = np.array([_capi.SEGMENT_NONE if v is None else int(v) for r in groups for v in r], dtype=np.int64)
        if flat.min() < 0 or ((flat >= n_segments) & (flat != _capi.SEGMENT_NONE)).any():
            raise RuntimeError("segment sum error: a segment id is not below n_segments")
        flat = flat.astype(np.uint32)
        return self._resident_call([self._ct(x)], len(groups) * n_segments, lambda L, h, out:
                                   L.pgpu_batch_ct_segment_sum(self._h, h[0], _ptr(flat), len(groups), n_segments, out))

    def segment_scan(self, x, seg_len, reverse=False):
        """Encrypted segmented prefix sum: x a list of ciphertexts (ints modulo n^2) read as [len(x) // seg_len][seg_len]
        -> the list of as many ciphertexts prod_{u <= t} x[r][u] mod n^2 (reverse: u >= t), i.e. encryptions of the
        inclusive cumulative sums mod n along every row.  One pgpu_batch_ct_segment_scan call on resident batches; there
        is no element-wise fall-back."""
        count, seg_len = len(x), int(seg_len)
        if count == 0 or seg_len <= 0 or count % seg_len:
            raise RuntimeError("segment scan error: seg_len must be positive and divide len(x)")
        return self._resident_call([self._ct(x)], count, lambda L, h, out:
                                   L.pgpu_batch_ct_segment_scan(self._h, h[0], seg_len, _capi.SCAN_REVERSE if reverse else 0, out))

    def negate(self, x):
        """Ciphertext negation: x a list of ciphertexts (ints modulo n^2) -> the list of their inverses modulo n^2, i.e.
        encryptions of (-m) mod n, each the canonical value pow(c, -1, n^2).  One pgpu_batch_ct_negate call on resident
        batches (all inverses from one modular inversion); there is no element-wise fall-back."""
        if len(x) == 0:
            raise RuntimeError("negate error: empty batch")
        return self._resident_call([self._ct(x)], len(x), lambda L, h, out: L.pgpu_batch_ct_negate(self._h, h[0], out))

    def sub(self, a, b):
        """Ciphertext subtraction: a, b lists of ciphertexts (ints modulo n^2), b as long as a or of one element (taken
        from every a[i]) -> the list a[i] * b[i]^-1 mod n^2, i.e. encryptions of (ma - mb) mod n.  One
        pgpu_batch_ct_sub call on resident batches; there is no element-wise fall-back."""
        if len(a) == 0 or len(b) not in (len(a), 1):
            raise RuntimeError("CT - CT error: Size mismatch!")
        return self._resident_call([self._ct(a), self._ct(b)], len(a), lambda L, h, out:
                                   L.pgpu_batch_ct_sub(self._h, h[0], h[1], out))

    def pack(self, x, seg_len, slot_bits):
        """Encrypted slot packing: x a list of ciphertexts (ints modulo n^2) read as [len(x) // seg_len][seg_len] -> the
        list of len(x) // seg_len ciphertexts prod_t x[r][t]^(2^(slot_bits * t)) mod n^2, i.e. encryptions of
        sum_t m[r][t] * 2^(slot_bits * t) mod n: seg_len slots of slot_bits bits per plaintext, slot 0 the least
        significant (unpack_slots takes the decrypted values apart).  One pgpu_batch_ct_pack call on resident batches;
        there is no element-wise fall-back."""
        count, seg_len, slot_bits = len(x), int(seg_len), int(slot_bits)
        if count == 0 or seg_len <= 0 or count % seg_len:
            raise RuntimeError("pack error: seg_len must be positive and divide len(x)")
        if not 1 <= slot_bits <= 1 << 30:
            raise RuntimeError("pack error: slot_bits must be positive")
        return self._resident_call([self._ct(x)], count // seg_len, lambda L, h, out:
                                   L.pgpu_batch_ct_pack(self._h, h[0], seg_len, slot_bits, out))


def unpack_slots(ms, seg_len, slot_bits, width_bits=None):
    """The way back from PublicKey.pack, after decrypt: every plaintext of ms holds seg_len slots of slot_bits bits, slot 0
    the least significant -> the len(ms) * seg_len slot values in input order (ms[0]'s slots first).  Pure host bit
    slicing; a slot that overflowed before the decrypt has carried into its neighbour and cannot be told apart here.
    width_bits: the width of the plaintexts (the bits of n, less one) when the caller wants the capacity checked too.
    ValueError: non-positive seg_len or slot_bits, seg_len * slot_bits above width_bits, a negative plaintext or one with
    bits beyond the last slot."""
    seg_len, slot_bits = int(seg_len), int(slot_bits)
    if seg_len <= 0 or slot_bits <= 0:
        raise ValueError("unpack_slots: seg_len and slot_bits must be positive")
    if width_bits is not None and seg_len * slot_bits > int(width_bits):
        raise ValueError("unpack_slots: seg_len * slot_bits exceeds the plaintext width")
    mask = (1 << slot_bits) - 1
    out = []
    for m in ms:
        m = int(m)
        if m < 0 or m >> (seg_len * slot_bits):
            raise ValueError("unpack_slots: a plaintext does not fit seg_len slots of slot_bits bits")
        out.extend((m >> (slot_bits * t)) & mask for t in range(seg_len))
    return out


class PrivateKey:
    """Host-side mirror of ipcl::PrivateKey::decrypt (CRT path, pri_key.cpp:65-90,114-157)."""

    def __init__(self, p, q):
        _ensure()
        self.p, self.q = (int(p), int(q)) if int(p) < int(q) else (int(q), int(p))
        self.n = self.p * self.q
        self.n_words = (self.n.bit_length() + 63) // 64
        pw = (max(self.p.bit_length(), self.q.bit_length()) + 63) // 64
        self._h = ctypes.c_void_p()
        _capi.check(_capi.lib().pgpu_privkey_create(_ptr(ints_to_limbs([self.p], pw)),
                                                    _ptr(ints_to_limbs([self.q], pw)), pw,
                                                    ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _capi._lib is not None:
            _capi._lib.pgpu_privkey_destroy(self._h)
            self._h = None

    def decrypt_limbs(self, c):
        c = np.ascontiguousarray(c, dtype=np.uint64)
        if c.shape[0] == 0:
            raise RuntimeError("decrypt: Cannot decrypt empty CipherText")     # pri_key.cpp:71
        if c.shape[1] != 2 * self.n_words:
            raise RuntimeError("decrypt: ciphertext width mismatch")
        out = np.empty((c.shape[0], self.n_words), dtype=np.uint64)
        _capi.check(_capi.lib().pgpu_paillier_decrypt_crt(self._h, _ptr(c), _ptr(out), c.shape[0]))
        return out

    def decrypt(self, c):
        if len(c) == 0:
            raise RuntimeError("decrypt: Cannot decrypt empty CipherText")
        return limbs_to_ints(self.decrypt_limbs(ints_to_limbs(c, 2 * self.n_words)))
