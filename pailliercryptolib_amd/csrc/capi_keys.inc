// pailliercryptolib_amd -- Paillier key objects: pgpu_pubkey_create / pgpu_privkey_create and the constants of their split forms (hensel.hpp, hensel_ps.hpp).
// Part of the translation unit of capi.cpp (included there, in place): the helpers of its anonymous namespaces --
// Montgomery contexts, geometry selection, launch wrappers -- are shared by every part.  Round 5 cut the file by topic;
// the kernel-form policy is a translation unit of its own (policy.cpp).

// ===================== Paillier public key / encrypt =====================
namespace {
// Constants of the split forms of n^2 (hensel.hpp) for DJN encrypt, r^n and CT x PT: per lane count the smallest
// compiled form (fixed-base or generic kernel) with enough limbs for n*k and a full-width twin Geo<2H,K> wide enough
// for n^2.  The way back to a full-width residue has constants of its own, so the forms need not match the geometry
// of the key's n^2 context; Montgomery-form results carry that context's radix Rs (they mix with the full-width
// kernels of resident batches).
// (n, n_words, the radix exponent of the n^2 context): all a form needs -- a PRIVATE key builds the same constants for its
// n = p*q, to bring word ciphertexts into pair rows ahead of the kernels that take only those (make_conv_form)
int make_pub_form(const BigNumber& n, int n_words, int nsq_rbits, int H, int K, std::shared_ptr<pgpu_pubkey::PubForm>* out) {
  const int L2 = H * K;
  const BigNumber N = n * n;
  const int cw = std::min(n_words, n.BitSize() / 64);
  if (cw <= 0) return PGPU_OK;
  const int nch = (2 * n_words + cw - 1) / cw;
  std::shared_ptr<pgpu_pubkey::PubForm> f(new pgpu_pubkey::PubForm);
  f->H = H;
  f->K = K;
  f->chunk_words = cw;
  f->nchunks = nch;
  f->n_words = n_words;
  f->n = n;
  auto n0inv_of = [](const BigNumber& v) {
    uint32_t n0 = (uint32_t)(v.limbs64()[0] & pgpu::kLimbMask), inv = n0;
    for (int i = 0; i < 5; ++i) inv *= 2u - n0 * inv;
    return (0u - inv) & pgpu::kLimbMask;
  };
  f->n0inv = n0inv_of(n);
  f->n0inv_full = n0inv_of(N);
  const BigNumber P = n * BigNumber((Ipp32u)f->n0inv), P2 = P * P;
  const BigNumber R = pow2(L2 * pgpu::kLimbBits);
  std::vector<uint32_t> h((size_t)L2 * (6 + 4 * (size_t)nch), 0);
  auto put_pair = [&](uint32_t* dst, const BigNumber& z) {
    const BigNumber zr = z % P2;
    const BigNumber q = zr / P;
    to_limbs29(zr % P, L2, dst);
    to_limbs29(q.isZero() ? q : P - q, L2, dst + L2);
  };
  to_limbs29(P, L2, h.data());
  to_limbs29(n, L2, h.data() + L2);
  {
    // gm = (-k^-1 mod n) * R^2 mod n  (kargs.hpp HenselPubDev::gm; hensel.hpp pair_times_gm)
    const BigNumber kinv = n.InverseMul(BigNumber((Ipp32u)f->n0inv) % n);
    const BigNumber Rn = R % n;
    to_limbs29((((n - kinv) % n) * ((Rn * Rn) % n)) % n, L2, h.data() + (size_t)L2 * (5 + 4 * (size_t)nch));
  }
  to_limbs29((R % n) * BigNumber((Ipp32u)f->n0inv) % n, L2, h.data() + 2 * L2);
  const BigNumber Rm = R % P2, R2 = (Rm * Rm) % P2;
  put_pair(h.data() + 3 * L2, Rm);
  f->one_host.assign(h.begin() + 3 * L2, h.begin() + 5 * L2);
  // (second set: bases that arrive as c*Rs mod n^2 -- resident ciphertexts)
  const BigNumber Rs = pow2(nsq_rbits);
  const BigNumber R2m = (R2 * P2.InverseMul(Rs % P2)) % P2;
  for (int i = 0; i < nch; ++i) {
    const BigNumber sh = pow2(64 * cw * i) % P2;
    put_pair(h.data() + 5 * L2 + (size_t)i * 2 * L2, (R2 * sh) % P2);
    put_pair(h.data() + 5 * L2 + (size_t)(nch + i) * 2 * L2, (R2m * sh) % P2);
  }
  RC_TRY(f->pub.upload(h.data(), h.size() * sizeof(uint32_t), false));
  const int LF = 2 * L2;
  const BigNumber Rf = pow2(LF * pgpu::kLimbBits) % N, Rsn = Rs % N;
  std::vector<uint32_t> g((size_t)4 * LF, 0);
  to_limbs29(N, LF, g.data());
  to_limbs29((n * Rf) % N, LF, g.data() + LF);
  to_limbs29((((n * Rf) % N) * Rsn) % N, LF, g.data() + 2 * LF);
  to_limbs29((Rf * Rsn) % N, LF, g.data() + 3 * LF);
  RC_TRY(f->full.upload(g.data(), g.size() * sizeof(uint32_t), false));
  *out = std::move(f);
  return PGPU_OK;
}
int build_hensel_pub_form(pgpu_pubkey* k, int H, int K) {
  std::shared_ptr<pgpu_pubkey::PubForm> f;
  RC_TRY(make_pub_form(k->n, k->n_words, k->nsq->geo.rbits(), H, K, &f));
  if (f) k->hforms.push_back(std::move(f));
  return PGPU_OK;
}
int build_hensel_pub(pgpu_pubkey* k) {
  // which forms, and in which order (the pair form of the key last: pair_form, use_split_encrypt): policy.hpp
  std::vector<std::pair<int, int>> forms;
  policy::pub_forms_for_bits(k->n.BitSize(), &forms);
  for (const auto& f : forms) RC_TRY(build_hensel_pub_form(k, f.first, f.second));
  return PGPU_OK;
}
}  // namespace

int pgpu_pubkey_create(const uint64_t* n, int n_words, const uint64_t* hs_or_null,
                       pgpu_pubkey** out) {
  RC_TRY(rt::check_ready());
  if (!n || n_words <= 0 || !out) return fail(PGPU_ERR_INVALID_PARAM, "null key material");
  std::unique_ptr<pgpu_pubkey> k(new pgpu_pubkey);
  k->gen = rt::pool_generation();
  k->n_words = n_words;
  k->n = BigNumber::fromLimbs64(n, (size_t)n_words);
  if (!k->n.IsOdd()) return fail(PGPU_ERR_EVEN_MODULUS, "n must be odd");
  BigNumber nsq = k->n * k->n;
  const GeoInfo* geo = pick_geo(2 * n_words, nsq.BitSize(), true);
  if (!geo) return fail(PGPU_ERR_UNSUPPORTED, "key wider than the compiled kernel geometries");
  CtxExtras ex;
  ex.nr_n = &k->n;
  ex.unit_q = true;
  RC_TRY(build_modctx(nsq, 2 * n_words, *geo, ex, &k->nsq));
  if (hs_or_null) {
    k->djn = true;
    RC_TRY(k->d_hs.upload(hs_or_null, (size_t)2 * n_words * 8, false));
  }
  RC_TRY(k->d_n.upload(n, (size_t)n_words * 8, false));
  if (sliding_enabled()) RC_TRY(make_schedule(k->n, pick_sliding_window(k->n.BitSize()), &k->sched_n, false));
  k->fb.resize((size_t)rt::pool_size());
  k->fbh.resize((size_t)rt::pool_size());
  RC_TRY(build_hensel_pub(k.get()));
  *out = k.release();
  return PGPU_OK;
}

void pgpu_pubkey_destroy(pgpu_pubkey* key) { delete key; }

// ===================== Paillier private key / CRT decrypt =====================
namespace {
// Constants of the split-form exponentiation (hensel.hpp) for both sides of the key.  A residue z modulo P^2 is
// the pair (a, b) with z == a - P*b: a = z mod P, b = (P - z div P) mod P.
// limbs per half of the pair rows a PUBLIC key over n uses (policy.hpp: pair_form_for_bits, as build_hensel_pub), 0: none
int pair_l2_for_modulus(const BigNumber& n, int* H_out = nullptr, int* K_out = nullptr) {
  int H = 0, K = 0;
  if (!policy::pair_form_for_bits(n.BitSize(), &H, &K)) return 0;
  if (H_out) *H_out = H;
  if (K_out) *K_out = K;
  return H * K;
}

int build_hensel_set(pgpu_privkey* k, pgpu_privkey::HenselSet* hs, int H, int K, const BigNumber& p,
                     const BigNumber& q, const BigNumber& hp, const BigNumber& hq, int lb = pgpu::kLimbBits,
                     bool balanced = false) {
  // lb: bits per limb of the constants (R = 2^(lb*L2), P = prime * (-prime^-1 mod 2^lb)); the pair rows this set reads are
  // rows of 29-bit limbs in any case
  // balanced (hensel_ps_bal.hpp): k = 1 -- P is the prime itself, n0inv its true -p^-1 mod 2^lb -- and every constant, the
  // same value in [0, prime) and the same sign convention z = a - P*b of the pairs, is written in BALANCED limbs
  // (two's complement words in [-2^(lb-1), 2^(lb-1)))
  const int L2 = H * K;
  const uint32_t lmask = (1u << lb) - 1;
  auto to_limbs29 = [lb, balanced](const BigNumber& v, int L, uint32_t* out) {   // (shadows the 29-bit one)
    to_limbs(v, L, out, lb);
    if (!balanced) return;
    uint32_t c = 0;
    for (int j = 0; j < L; ++j) {       // (values are below 2^(lb*L - 4): the carry dies below the top limb)
      const uint32_t u = out[j] + c;
      c = u >= (1u << (lb - 1)) ? 1u : 0u;
      out[j] = c ? u - (1u << lb) : u;
    }
  };
  hs->lb = lb;
  const int bits_lo = std::min(p.BitSize(), q.BitSize());
  // a ciphertext enters in chunks z < 2^(64*cw) <= 2P (P >= prime > 2^(bits-1))
  const int cw = std::min(k->pq_words, bits_lo / 64);
  if (cw <= 0) return PGPU_OK;   // (leaves hs->H == 0: no split form for this key)
  const int ct_words = 2 * k->n_words;
  const int nch = (ct_words + cw - 1) / cw;
  const BigNumber R = pow2(L2 * lb);
  hs->H = H;
  hs->K = K;
  hs->chunk_words = cw;
  hs->nchunks = nch;
  // entry from pair rows of the n^2 domain: the a part in chunks of at most L2 limbs (so that a chunk fits the lanes of
  // one half), evenly sized; with narrower limbs: as many 29-bit row limbs as fit a half with two bits to spare
  const BigNumber nmod = p * q;
  hs->pair_l2 = pair_l2_for_modulus(nmod);
  if (hs->pair_l2) {
    // (the one-lane product-scanning form, H == 1, re-limbs a chunk into K canonical limbs whatever its limb width)
    const int fit = (lb == pgpu::kLimbBits && H != 1) ? L2 : (L2 * lb - 2) / pgpu::kLimbBits;
    hs->pchunks = (hs->pair_l2 + fit - 1) / fit;
    hs->pchunk_limbs = (hs->pair_l2 + hs->pchunks - 1) / hs->pchunks;
  }
  uint32_t kn = 0;   // Pn = n * kn == -1 mod 2^29
  {
    uint32_t n0 = (uint32_t)(nmod.limbs64()[0] & pgpu::kLimbMask), inv = n0;
    for (int i = 0; i < 5; ++i) inv *= 2u - n0 * inv;
    kn = (0u - inv) & pgpu::kLimbMask;
  }
  const size_t side_words = hs->side_words();
  std::vector<uint32_t> h(2 * side_words, 0);
  for (int sd = 0; sd < 2; ++sd) {
    const BigNumber& pr = sd ? q : p;
    uint32_t n0 = (uint32_t)(pr.limbs64()[0] & lmask), inv = n0;
    for (int i = 0; i < 5; ++i) inv *= 2u - n0 * inv;
    const uint32_t n0inv = (0u - inv) & lmask;
    const BigNumber kfac((Ipp32u)(balanced ? 1u : n0inv));     // P = prime * k
    const BigNumber P = pr * kfac;
    const BigNumber P2 = P * P;
    uint32_t* b = h.data() + sd * side_words;
    auto put_pair = [&](uint32_t* dst, const BigNumber& z) {
      const BigNumber zr = z % P2;
      const BigNumber f = zr / P;
      to_limbs29(zr % P, L2, dst);
      to_limbs29(f.isZero() ? f : P - f, L2, dst + L2);
    };
    to_limbs29(P, L2, b);
    to_limbs29(pr, L2, b + L2);
    to_limbs29(sd ? hq : hp, L2, b + 2 * L2);
    to_limbs29((R % pr) * kfac % pr, L2, b + 3 * L2);   // P = prime * (-prime^-1 mod 2^29)
    const BigNumber Rm = R % P2, R2 = (Rm * Rm) % P2;
    put_pair(b + 4 * L2, Rm);
    const BigNumber R2m = (R2 * P2.InverseMul(pow2(k->nsq_rbits) % P2)) % P2;   // cancels the R of the n^2 context
    for (int i = 0; i < nch; ++i) {
      const BigNumber sh = pow2(64 * cw * i) % P2;
      put_pair(b + 6 * L2 + (size_t)i * 2 * L2, (R2 * sh) % P2);
      put_pair(b + 6 * L2 + (size_t)(nch + i) * 2 * L2, (R2m * sh) % P2);
    }
    if (hs->pair_l2) {
      // c*Rn == a - Pn*b (mod n^2), Pn = n*kn = pr * (n/pr) * kn.  Modulo pr^2:  c*Rn == a - P*(kappa*b) with
      // kappa = (n/pr) * kn * k^-1 mod pr  (P = pr*k; P*y only depends on y mod pr).  The pair of c*R is that times R/Rn.
      const BigNumber Rn = pow2(hs->pair_l2 * pgpu::kLimbBits);
      const BigNumber R2n = (R2 * P2.InverseMul(Rn % P2)) % P2;            // R^2 * Rn^-1 mod P^2
      const BigNumber other = sd ? p : q;
      const BigNumber kinv = pr.InverseMul(kfac % pr);   // k^-1 mod pr
      const BigNumber kappa = (((other % pr) * (BigNumber((Ipp32u)kn) % pr)) % pr * kinv) % pr;
      const BigNumber Rp = R % pr;
      const BigNumber r2n_p = (((Rp * Rp) % pr) * pr.InverseMul(Rn % pr)) % pr;   // R^2 * Rn^-1 mod pr
      uint32_t* pc = b + (size_t)L2 * (6 + 4 * (size_t)nch);
      uint32_t* pb = pc + (size_t)hs->pchunks * 2 * L2;
      for (int i = 0; i < hs->pchunks; ++i) {
        const BigNumber sh = pow2(pgpu::kLimbBits * hs->pchunk_limbs * i);
        put_pair(pc + (size_t)i * 2 * L2, (R2n * (sh % P2)) % P2);
        to_limbs29((((kappa * (sh % pr)) % pr) * r2n_p) % pr, L2, pb + (size_t)i * L2);
      }
    }
    hs->n0inv[sd] = n0inv;
  }
  const int rc = hs->blob.upload(h.data(), h.size() * sizeof(uint32_t), true);
  secure_wipe(h.data(), h.size() * sizeof(h[0]));
  return rc;
}
int build_hensel(pgpu_privkey* k, const BigNumber& p, const BigNumber& q, const BigNumber& hp, const BigNumber& hq) {
  // R = 2^(29*H*K) >= 256 * P, P = prime * k < 2^(bits + 29): per lane count the smallest compiled form with
  // enough limbs
  const int need = std::max(p.BitSize(), q.BitSize()) + 29 + 8;
  for (int H : {8, 4, 2})
    for (int K = 1; K <= 19; ++K)
      if (pgpu::hensel_has(H, K) && pgpu::kLimbBits * H * K >= need) {
        std::unique_ptr<pgpu_privkey::HenselSet> set(new pgpu_privkey::HenselSet);
        RC_TRY(build_hensel_set(k, set.get(), H, K, p, q, hp, hq));
        if (set->H) k->hs.push_back(std::move(set));
        break;
      }
  if (!k->hs.empty() && k->hs.front()->pair_l2) {
    int H = 0, K = 0;
    const BigNumber n = p * q;
    if (pair_l2_for_modulus(n, &H, &K)) RC_TRY(make_pub_form(n, k->n_words, k->nsq_rbits, H, K, &k->conv_form));
  }
  // one lane per exponentiation, product scanning (hensel_ps.hpp): K limbs of lb bits per half, R = 2^(lb*K) >= 16 * P,
  // P = prime * k < 2^(bits + lb).  Reads pair rows only.  (16 is enough for this kernel: a lazy product of values below
  // c1*P and c2*P comes out below (c1*c2/16 + 1)*P, a pair product's second half below ((c1*d2 + d1*c2)/16 + 1)*P; the
  // entry sums at most 4 chunk products (a below 5 P, b below 10 P), the table recurrence then settles below (1.5 P, 2.5 P)
  // and the main loop below 2 P -- the multi-lane forms keep 256 for their relaxed limbs.  For 3072-bit keys that is the
  // difference between 56 and 57 limbs: 3.5 % of the products.)
  if (!k->hs.empty() && k->hs.front()->pair_l2) {
    const int bits = std::max(p.BitSize(), q.BitSize());
    for (int lb : {28, 29})
      for (int K = 1; K <= 64 && !k->hs_ps; ++K)
        if (pgpu::hensel_ps_has(K, lb) && lb * K >= bits + lb + 4 && lb * (K - 1) < bits + lb + 4) {
          std::unique_ptr<pgpu_privkey::HenselSet> set(new pgpu_privkey::HenselSet);
          RC_TRY(build_hensel_set(k, set.get(), 1, K, p, q, hp, hq, lb));
          if (set->H && set->pair_l2) k->hs_ps = std::move(set);
        }
    // ... on balanced limbs (hensel_ps_bal.hpp): K limbs of lb bits hold the prime itself with four bits to spare (the entry
    // sums up to four chunk products: below 5 p).  A third set beside hs / hs_ps, which the wavefront-wide forms keep reading
    if (k->hs_ps)
      for (int K = 1; K <= 64 && !k->hs_psb; ++K)
        if (pgpu::hensel_psb_has(K, pgpu::kLimbBits) && bits <= pgpu::kLimbBits * K - 4 && pgpu::hensel_ps_has(k->hs_ps->K, k->hs_ps->lb) &&
            k->hs_ps->K > K) {
          std::unique_ptr<pgpu_privkey::HenselSet> set(new pgpu_privkey::HenselSet);
          RC_TRY(build_hensel_set(k, set.get(), 1, K, p, q, hp, hq, pgpu::kLimbBits, true));
          if (set->H && set->pair_l2 == k->hs_ps->pair_l2) k->hs_psb = std::move(set);
        }
  }
  return PGPU_OK;
}
}  // namespace

int pgpu_privkey_create(const uint64_t* p_in, const uint64_t* q_in, int pq_words,
                        pgpu_privkey** out) {
  RC_TRY(rt::check_ready());
  if (!p_in || !q_in || pq_words <= 0 || !out) return fail(PGPU_ERR_INVALID_PARAM, "null key material");
  BigNumber p = BigNumber::fromLimbs64(p_in, (size_t)pq_words);
  BigNumber q = BigNumber::fromLimbs64(q_in, (size_t)pq_words);
  if (q < p) std::swap(p, q);  // pri_key.cpp:19-22
  if (p == q) return fail(PGPU_ERR_NOT_INVERTIBLE, "PrivateKey: p and q are same");
  if (!p.IsOdd() || !q.IsOdd() || p <= BigNumber::Two())
    return fail(PGPU_ERR_EVEN_MODULUS, "p and q must be odd primes");
  std::unique_ptr<pgpu_privkey> k(new pgpu_privkey);
  k->gen = rt::pool_generation();
  const BigNumber n = p * q;
  const int nw = (n.BitSize() + 63) / 64;  // words of n; p^2, q^2 rows use the same width
  k->n_words = nw;
  k->pq_words = pq_words;
  const BigNumber psq = p * p, qsq = q * q;
  const BigNumber pm1 = p - 1, qm1 = q - 1;
  if (psq.BitSize() > 64 * nw || qsq.BitSize() > 64 * nw)
    return fail(PGPU_ERR_INVALID_PARAM, "p and q differ too much in size");
  // hp = L_p(g^(p-1) mod p^2)^-1 mod p   (computeHfun, pri_key.cpp:159-167).  The reference's g is always
  // n + 1 (pub_key.cpp:17, pri_key.cpp:47) and n^2 == 0 mod p^2, so the binomial series stops after two terms:
  //   g^(p-1) = 1 + (p-1)*n  (mod p^2)   =>   L_p(.) = ((p-1)*n mod p^2) / p = (p-1)*q mod p
  // -- the same value without an exponentiation.
  BigNumber hp, hq;
  try {
    hp = p.InverseMul((pm1 * q) % p);
    hq = q.InverseMul((qm1 * p) % q);
  } catch (const std::exception& e) {
    return fail(PGPU_ERR_NOT_INVERTIBLE, std::string("PrivateKey precompute: ") + e.what());
  }
  // half-width exponentiation contexts: inputs are 2*nw-word ciphertexts reduced on load
  const int sq_bits = std::max(psq.BitSize(), qsq.BitSize());
  const GeoInfo* ge = pick_geo(nw, sq_bits, true);
  if (!ge) return fail(PGPU_ERR_UNSUPPORTED, "key wider than the compiled kernel geometries");
  k->geo_exp = *ge;
  // Montgomery-form ciphertexts carry the R of the n^2 context (pgpu_pubkey_create picks it the same way)
  const BigNumber nsq = n * n;
  const GeoInfo* gn = pick_geo(2 * nw, nsq.BitSize(), true);
  if (!gn) return fail(PGPU_ERR_UNSUPPORTED, "key wider than the compiled kernel geometries");
  k->nsq_rbits = gn->rbits();
  CtxExtras exp_p, exp_q;
  exp_p.want_r2s = exp_q.want_r2s = true;
  exp_p.unit_q = exp_q.unit_q = true;
  exp_p.secret = exp_q.secret = true;
  exp_p.mont_src_rbits = exp_q.mont_src_rbits = k->nsq_rbits;
  exp_p.fc = &hp;
  exp_q.fc = &hq;
  // both sides of a launch share one instruction stream: unit quotient digits only if BOTH moduli leave room
  // (p^2 can be a bit shorter than q^2 and straddle the threshold on its own)
  exp_p.force_unit = exp_q.force_unit = unit_fits(*ge, sq_bits) ? 1 : 0;
  RC_TRY(build_modctx(psq, nw, *ge, exp_p, &k->p2));
  RC_TRY(build_modctx(qsq, nw, *ge, exp_q, &k->q2));
  k->geo_lat = latency_geo(*ge);
  if (k->geo_lat.L() == ge->L()) {
    k->p2l = k->p2;
    k->q2l = k->q2;
  } else {
    exp_p.force_unit = exp_q.force_unit = unit_fits(k->geo_lat, sq_bits) ? 1 : 0;
    RC_TRY(build_modctx(psq, nw, k->geo_lat, exp_p, &k->p2l));
    RC_TRY(build_modctx(qsq, nw, k->geo_lat, exp_q, &k->q2l));
  }
  std::vector<uint64_t> exps((size_t)2 * pq_words, 0);
  pm1.toLimbs64(exps.data(), pq_words);
  qm1.toLimbs64(exps.data() + pq_words, pq_words);
  RC_TRY(k->d_exps.upload(exps.data(), exps.size() * 8, true));
  secure_wipe(exps.data(), exps.size() * sizeof(exps[0]));
  k->exp_bits = std::max(pm1.BitSize(), qm1.BitSize());
  {
    const int sw = pick_sliding_window(k->exp_bits);
    RC_TRY(make_schedule(pm1, sw, &k->sched[0], true));
    RC_TRY(make_schedule(qm1, sw, &k->sched[1], true));
  }

  RC_TRY(build_hensel(k.get(), p, q, hp, hq));

  // recombination: auxiliary modulus M = 2^(29*(L-1)) - 1 must exceed n (exact u*p product)
  const GeoInfo* gc = nullptr;
  for (const GeoInfo& gg : kGeos)
    if (!(gg.G == 4 && gg.K == 10) && pgpu::kLimbBits * (gg.L() - 1) >= n.BitSize() + 2 && gg.rbits() >= 64 * nw) {
      gc = &gg;
      break;
    }
  if (!gc) return fail(PGPU_ERR_UNSUPPORTED, "key wider than the compiled kernel geometries");
  k->geo_crt = *gc;
  const int Lc = gc->L();
  const BigNumber M = pow2(pgpu::kLimbBits * (Lc - 1)) - 1;
  if (M.gcd(p) != BigNumber::One() || M.gcd(q) != BigNumber::One())
    return fail(PGPU_ERR_NOT_INVERTIBLE, "auxiliary modulus shares a factor with the key");
  const int mwM = (M.BitSize() + 63) / 64;
  CtxExtras sec;
  sec.secret = true;
  RC_TRY(build_modctx(M, mwM, *gc, CtxExtras(), &k->cM));
  RC_TRY(build_modctx(q, nw, *gc, sec, &k->cQ));
  const BigNumber Rc = pow2(gc->rbits());
  const BigNumber pinv_q = q.InverseMul(p);  // p^-1 mod q (pri_key.cpp:27)
  std::vector<uint32_t> c32((size_t)4 * Lc);
  to_limbs29((M.InverseMul(p) * Rc) % M, Lc, c32.data());
  to_limbs29((M.InverseMul(q) * Rc) % M, Lc, c32.data() + Lc);
  to_limbs29((pinv_q * Rc) % q, Lc, c32.data() + 2 * Lc);
  to_limbs29((p * Rc) % M, Lc, c32.data() + 3 * Lc);
  RC_TRY(k->d_crt32.upload(c32.data(), c32.size() * 4, true));
  secure_wipe(c32.data(), c32.size() * sizeof(c32[0]));
  const int pad = gc->w64() + 1;  // rows padded so word helpers can run over W64 words
  std::vector<uint64_t> c64((size_t)5 * pad, 0);
  hp.toLimbs64(c64.data(), pad);
  hq.toLimbs64(c64.data() + pad, pad);
  psq.toLimbs64(c64.data() + 2 * pad, pad);
  qsq.toLimbs64(c64.data() + 3 * pad, pad);
  q.toLimbs64(c64.data() + 4 * pad, pad);
  RC_TRY(k->d_crt64.upload(c64.data(), c64.size() * 8, true));
  secure_wipe(c64.data(), c64.size() * sizeof(c64[0]));
  *out = k.release();
  return PGPU_OK;
}

void pgpu_privkey_destroy(pgpu_privkey* key) { delete key; }
