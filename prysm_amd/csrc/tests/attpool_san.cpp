// The pending-attestation pool's selection rules on the CPU, under ASan+UBSan (plain g++; no GPU
// code): attpool_dev.h -- the text the kernels of attpool.hip compile -- driven through a sequential
// form of the four phases (size, scan, commit, write) over column sets held in vectors of exactly
// their capacities, against a std::vector-of-records model: random batches, appends at a non-zero
// base, prunes between the two buffer sets, each of the seven capacities hit alone with the
// rollback, and the inverted-range rule.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../attpool_dev.h"

using namespace pz;

namespace {

struct Rec {
  uint64_t slot = 0, shard = 0, jslot = 0;
  std::vector<uint8_t> jbh, sbh, bits;
  std::vector<std::vector<uint8_t>> obl;
  std::vector<uint64_t> sig;
  uint32_t committee = 0;
  bool operator==(const Rec& o) const {
    return slot == o.slot && shard == o.shard && jslot == o.jslot && jbh == o.jbh && sbh == o.sbh && bits == o.bits &&
           obl == o.obl && sig == o.sig && committee == o.committee;
  }
};

// A column set in vectors of exactly the sizes given: one byte past any of them is ASan's.
struct Cols {
  std::vector<uint64_t> slot, shard, jslot, jbh_offs, sbh_offs, bits_offs, obl_offs, obl_first, sig, sig_first;
  std::vector<uint8_t> jbh, sbh, bits, obl;
  std::vector<uint32_t> committee, shard32;
  explicit Cols(const uint64_t cap[kApCols])
      : slot(cap[0]), shard(cap[0]), jslot(cap[0]), jbh_offs(cap[0] + 1), sbh_offs(cap[0] + 1), bits_offs(cap[0] + 1),
        obl_offs(cap[kApElems] + 1), obl_first(cap[0] + 1), sig(cap[kApSigs]), sig_first(cap[0] + 1), jbh(cap[kApJbh]),
        sbh(cap[kApSbh]), bits(cap[kApBits]), obl(cap[kApElemBytes]), committee(cap[0]), shard32(cap[0]) {}
  pz_attestation_cols view() const {
    pz_attestation_cols c{};
    c.slot = slot.data(), c.shard_id = shard.data(), c.justified_slot = jslot.data();
    c.justified_block_hash = jbh.data(), c.justified_block_hash_offs = jbh_offs.data();
    c.shard_block_hash = sbh.data(), c.shard_block_hash_offs = sbh_offs.data();
    c.attester_bitfield = bits.data(), c.attester_bitfield_offs = bits_offs.data();
    c.oblique_parent_hashes = obl.data(), c.oblique_offs = obl_offs.data(), c.oblique_first = obl_first.data();
    c.aggregate_sig = sig.data(), c.aggregate_sig_first = sig_first.data();
    return c;
  }
};

void sizes_of(const std::vector<Rec>& v, uint64_t n[kApCols]) {
  for (int c = 0; c < kApCols; ++c) n[c] = 0;
  for (const Rec& r : v) {
    n[kApRows] += 1, n[kApJbh] += r.jbh.size(), n[kApSbh] += r.sbh.size(), n[kApBits] += r.bits.size();
    n[kApElems] += r.obl.size(), n[kApSigs] += r.sig.size();
    for (const auto& e : r.obl) n[kApElemBytes] += e.size();
  }
}

// The records as a column set sized to hold exactly them (ranges start at 0).
Cols to_cols(const std::vector<Rec>& v) {
  uint64_t n[kApCols];
  sizes_of(v, n);
  Cols c(n);
  uint64_t at[kApCols] = {};
  for (const Rec& r : v) {
    const uint64_t i = at[0]++;
    c.slot[i] = r.slot, c.shard[i] = r.shard, c.jslot[i] = r.jslot, c.committee[i] = r.committee;
    c.shard32[i] = ap_shard32(r.shard);
    c.jbh_offs[i] = at[kApJbh], c.sbh_offs[i] = at[kApSbh], c.bits_offs[i] = at[kApBits];
    c.obl_first[i] = at[kApElems], c.sig_first[i] = at[kApSigs];
    if (!r.jbh.empty()) std::memcpy(&c.jbh[at[kApJbh]], r.jbh.data(), r.jbh.size());
    if (!r.sbh.empty()) std::memcpy(&c.sbh[at[kApSbh]], r.sbh.data(), r.sbh.size());
    if (!r.bits.empty()) std::memcpy(&c.bits[at[kApBits]], r.bits.data(), r.bits.size());
    at[kApJbh] += r.jbh.size(), at[kApSbh] += r.sbh.size(), at[kApBits] += r.bits.size();
    for (const auto& e : r.obl) {
      c.obl_offs[at[kApElems]++] = at[kApElemBytes];
      if (!e.empty()) std::memcpy(&c.obl[at[kApElemBytes]], e.data(), e.size());
      at[kApElemBytes] += e.size();
    }
    for (uint64_t x : r.sig) c.sig[at[kApSigs]++] = x;
  }
  c.jbh_offs[at[0]] = at[kApJbh], c.sbh_offs[at[0]] = at[kApSbh], c.bits_offs[at[0]] = at[kApBits];
  c.obl_first[at[0]] = at[kApElems], c.sig_first[at[0]] = at[kApSigs], c.obl_offs[at[kApElems]] = at[kApElemBytes];
  return c;
}

std::vector<Rec> from_cols(const Cols& c, const uint64_t n[kApCols]) {
  std::vector<Rec> v(n[0]);
  for (uint64_t i = 0; i < n[0]; ++i) {
    Rec& r = v[i];
    r.slot = c.slot[i], r.shard = c.shard[i], r.jslot = c.jslot[i], r.committee = c.committee[i];
    if (c.shard32[i] != ap_shard32(r.shard)) std::abort();
    r.jbh.assign(c.jbh.begin() + c.jbh_offs[i], c.jbh.begin() + c.jbh_offs[i + 1]);
    r.sbh.assign(c.sbh.begin() + c.sbh_offs[i], c.sbh.begin() + c.sbh_offs[i + 1]);
    r.bits.assign(c.bits.begin() + c.bits_offs[i], c.bits.begin() + c.bits_offs[i + 1]);
    for (uint64_t e = c.obl_first[i]; e < c.obl_first[i + 1]; ++e)
      r.obl.emplace_back(c.obl.begin() + c.obl_offs[e], c.obl.begin() + c.obl_offs[e + 1]);
    r.sig.assign(c.sig.begin() + c.sig_first[i], c.sig.begin() + c.sig_first[i + 1]);
  }
  return v;
}

// The pool: two column sets, the counts, the sticky error word.
struct Pool {
  uint64_t cap[kApCols];
  Cols set[2];
  int live = 0;
  uint64_t counts[kApCols] = {};
  uint64_t err = 0;
  explicit Pool(const uint64_t c[kApCols]) : set{Cols(c), Cols(c)} { std::memcpy(cap, c, sizeof cap); }
};

constexpr uint64_t kSanTile = 4;  // (small tiles: many tile bases; the rules do not depend on the width)

// One selection, phase by phase as the launches run.  Returns whether it landed.
bool select(Pool& p, const pz_attestation_cols& src, const uint32_t* src_comm, uint64_t n, const int32_t* status,
            const uint8_t* take, bool prune, uint64_t lsr, Cols& dst) {
  const uint64_t ntiles = (n + kSanTile - 1) / kSanTile;
  auto keep = [&](uint64_t i) { return prune ? ap_keep_prune(src.slot[i], lsr) : ap_keep_append(status, take, i); };
  // 1 size
  std::vector<uint64_t> tiles(kApCols * (ntiles ? ntiles : 1), 0);
  for (uint64_t i = 0; i < n; ++i)
    if (keep(i)) {
      const ApRow r = ap_row(src, i);
      if (r.inverted) p.err |= kApErrInverted;
      for (int c = 0; c < kApCols; ++c) tiles[c * ntiles + i / kSanTile] += r.sz[c];
    }
  // 2 scan
  uint64_t total[kApCols];
  for (int c = 0; c < kApCols; ++c) {
    uint64_t run = 0;
    for (uint64_t t = 0; t < ntiles; ++t) {
      const uint64_t x = tiles[c * ntiles + t];
      tiles[c * ntiles + t] = run;
      run += x;
    }
    total[c] = run;
  }
  // 3 commit
  uint64_t base[kApCols];
  for (int c = 0; c < kApCols; ++c) base[c] = prune ? 0 : p.counts[c];
  if (!ap_fits(base, total, p.cap)) {
    p.err |= kApErrCapacity;
    return false;
  }
  for (int c = 0; c < kApCols; ++c) p.counts[c] = base[c] + total[c];
  // 4 write
  for (uint64_t t = 0; t < ntiles; ++t) {
    uint64_t at[kApCols];
    for (int c = 0; c < kApCols; ++c) at[c] = base[c] + tiles[c * ntiles + t];
    for (uint64_t i = t * kSanTile; i < n && i < (t + 1) * kSanTile; ++i) {
      if (!keep(i)) continue;
      const ApRow r = ap_row(src, i);
      const uint64_t row = at[0];
      const bool z = r.inverted;
      dst.slot[row] = (!z && src.slot) ? src.slot[i] : 0;
      dst.shard[row] = (!z && src.shard_id) ? src.shard_id[i] : 0;
      dst.jslot[row] = (!z && src.justified_slot) ? src.justified_slot[i] : 0;
      dst.committee[row] = z ? 0xFFFFFFFFu : src_comm[i];
      dst.shard32[row] = ap_shard32(dst.shard[row]);
      dst.jbh_offs[row] = at[kApJbh], dst.sbh_offs[row] = at[kApSbh], dst.bits_offs[row] = at[kApBits];
      dst.obl_first[row] = at[kApElems], dst.sig_first[row] = at[kApSigs];
      if (r.sz[kApJbh]) std::memcpy(&dst.jbh[at[kApJbh]], src.justified_block_hash + r.lo[kApJbh], r.sz[kApJbh]);
      if (r.sz[kApSbh]) std::memcpy(&dst.sbh[at[kApSbh]], src.shard_block_hash + r.lo[kApSbh], r.sz[kApSbh]);
      if (r.sz[kApBits]) std::memcpy(&dst.bits[at[kApBits]], src.attester_bitfield + r.lo[kApBits], r.sz[kApBits]);
      for (uint64_t k = 0; k < r.sz[kApElems]; ++k)
        dst.obl_offs[at[kApElems] + k] = at[kApElemBytes] + (src.oblique_offs[r.lo[kApElems] + k] - r.lo[kApElemBytes]);
      if (r.sz[kApElemBytes])
        std::memcpy(&dst.obl[at[kApElemBytes]], src.oblique_parent_hashes + r.lo[kApElemBytes], r.sz[kApElemBytes]);
      if (r.sz[kApSigs]) std::memcpy(&dst.sig[at[kApSigs]], src.aggregate_sig + r.lo[kApSigs], r.sz[kApSigs] * 8);
      for (int c = 0; c < kApCols; ++c) at[c] += r.sz[c];
    }
  }
  const uint64_t* e = p.counts;
  dst.jbh_offs[e[0]] = e[kApJbh], dst.sbh_offs[e[0]] = e[kApSbh], dst.bits_offs[e[0]] = e[kApBits];
  dst.obl_first[e[0]] = e[kApElems], dst.sig_first[e[0]] = e[kApSigs], dst.obl_offs[e[kApElems]] = e[kApElemBytes];
  return true;
}

bool append(Pool& p, const Cols& batch, uint64_t n, const std::vector<int32_t>& status, const std::vector<uint8_t>* take) {
  return select(p, batch.view(), batch.committee.data(), n, status.data(), take ? take->data() : nullptr, false, 0,
                p.set[p.live]);
}

void prune(Pool& p, uint64_t lsr) {
  const Cols& from = p.set[p.live];
  if (!select(p, from.view(), from.committee.data(), p.counts[0], nullptr, nullptr, true, lsr, p.set[p.live ^ 1])) std::abort();
  p.live ^= 1;
}

std::mt19937_64 rng(20181);
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }
std::vector<uint8_t> blob(uint64_t len) {
  std::vector<uint8_t> b(len);
  for (auto& x : b) x = (uint8_t)rng();
  return b;
}

Rec random_rec() {
  Rec r;
  r.slot = rnd(200), r.jslot = rnd(100), r.committee = (uint32_t)rnd(64);
  const uint64_t shards[] = {rnd(1024), 0xFFFFFFFFull, 0x100000000ull, 1ull << 63};
  r.shard = shards[rnd(8) < 5 ? 0 : 1 + rnd(3)];
  r.jbh = blob(rnd(3) ? 32 : rnd(40)), r.sbh = blob(rnd(3) ? 32 : rnd(70)), r.bits = blob(rnd(66));
  const uint64_t ne = rnd(4) ? 0 : rnd(15);
  for (uint64_t e = 0; e < ne; ++e) r.obl.push_back(blob(rnd(5) ? rnd(41) : 0));
  const uint64_t ns = rnd(3) ? 0 : rnd(18);
  for (uint64_t s = 0; s < ns; ++s) r.sig.push_back(rng());
  return r;
}

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

void check_equal(const Pool& p, const std::vector<Rec>& model) {
  uint64_t n[kApCols];
  sizes_of(model, n);
  for (int c = 0; c < kApCols; ++c) CHECK(p.counts[c] == n[c]);
  CHECK(from_cols(p.set[p.live], p.counts) == model);
}

}  // namespace

int main() {
  uint64_t landed = 0, rolled = 0, pruned = 0;
  static const int32_t kStatuses[] = {PZ_ATT_PROCESSED, PZ_ATT_NOT_PROCESSED, PZ_ATT_SLOT_HIGH, PZ_ATT_SLOT_LOW,
                                      PZ_ATT_JUSTIFIED, PZ_ATT_NO_COMMITTEE, PZ_ATT_BITFIELD_LEN, PZ_ATT_TRAILING_BITS,
                                      PZ_EINVAL, PZ_ERANGE, PZ_EINDEX};
  // ---- random batches, appends at a non-zero base, prunes -----------------------------------
  for (int round = 0; round < 60; ++round) {
    const uint64_t big[kApCols] = {400, 16000, 24000, 24000, 3000, 60000, 4000};
    Pool p(big);
    std::vector<Rec> model;
    for (int call = 0; call < 8; ++call) {
      if (call && rnd(3) == 0) {
        const uint64_t lsr = rnd(220);
        prune(p, lsr);
        std::vector<Rec> kept;
        for (const Rec& r : model)
          if (r.slot > lsr) kept.push_back(r);
        model.swap(kept);
        ++pruned;
        check_equal(p, model);
        continue;
      }
      const uint64_t n = rnd(5) ? rnd(40) : 0;
      std::vector<Rec> batch(n);
      for (Rec& r : batch) r = random_rec();
      std::vector<int32_t> status(n);
      std::vector<uint8_t> take(n);
      const int pattern = (int)rnd(5);  // all, none, alternating, first only, last only; else by status
      for (uint64_t i = 0; i < n; ++i) {
        status[i] = rnd(2) ? PZ_ATT_PROCESSED : kStatuses[rnd(sizeof kStatuses / sizeof *kStatuses)];
        take[i] = pattern == 0 ? 1 : pattern == 1 ? 0 : pattern == 2 ? (uint8_t)(i & 1) : pattern == 3 ? i == 0 : i + 1 == n;
      }
      const bool with_take = rnd(2);
      const Cols cols = to_cols(batch);
      const std::vector<Rec> before = model;
      std::vector<Rec> want = model;
      for (uint64_t i = 0; i < n; ++i)
        if (status[i] == PZ_ATT_PROCESSED && (!with_take || take[i])) want.push_back(batch[i]);
      uint64_t need[kApCols];
      sizes_of(want, need);
      bool fits = true;
      for (int c = 0; c < kApCols; ++c) fits = fits && need[c] <= p.cap[c];
      const bool ok = append(p, cols, n, status, with_take ? &take : nullptr);
      CHECK(ok == fits);
      if (ok) model.swap(want), ++landed;
      else ++rolled;
      check_equal(p, model);
    }
    CHECK(!(p.err & kApErrInverted));
  }
  // ---- each of the seven capacities hit alone, with the rollback --------------------------------
  for (int c = 0; c < kApCols; ++c)
    for (int round = 0; round < 20; ++round) {
      std::vector<Rec> first(1 + rnd(6)), second(1 + rnd(6));
      for (Rec& r : first) r = random_rec();
      for (Rec& r : second) r = random_rec();
      Rec& last = second.back();  // every size of the second batch is non-zero
      last.jbh = blob(32), last.sbh = blob(32), last.bits = blob(5), last.obl = {blob(3), blob(0)}, last.sig = {1, 2};
      std::vector<Rec> both = first;
      both.insert(both.end(), second.begin(), second.end());
      uint64_t cap[kApCols];
      sizes_of(both, cap);
      for (int k = 0; k < kApCols; ++k) cap[k] += k == c ? 0 : 7;
      cap[c] -= 1;  // one short in capacity c alone
      Pool p(cap);
      const std::vector<int32_t> s1(first.size(), PZ_ATT_PROCESSED), s2(second.size(), PZ_ATT_PROCESSED);
      CHECK(append(p, to_cols(first), first.size(), s1, nullptr));
      const Cols snapshot = p.set[p.live];
      uint64_t counts[kApCols];
      std::memcpy(counts, p.counts, sizeof counts);
      CHECK(!append(p, to_cols(second), second.size(), s2, nullptr));
      ++rolled;
      CHECK(p.err == kApErrCapacity);
      CHECK(!std::memcmp(counts, p.counts, sizeof counts));
      CHECK(from_cols(p.set[p.live], p.counts) == from_cols(snapshot, counts));
      check_equal(p, first);
      // a later call that fits still lands
      second.pop_back();
      const std::vector<int32_t> s3(second.size(), PZ_ATT_PROCESSED);
      CHECK(append(p, to_cols(second), second.size(), s3, nullptr));
      ++landed;
      first.insert(first.end(), second.begin(), second.end());
      check_equal(p, first);
    }
  // ---- the inverted-range rule --------------------------------------------------------------
  {
    std::vector<Rec> batch(5);
    for (Rec& r : batch) r = random_rec(), r.bits = blob(9), r.obl = {blob(4)};
    Cols cols = to_cols(batch);
    std::swap(cols.bits_offs[2], cols.bits_offs[3]);  // row 2 inverted; rows 1 and 3 change length
    const uint64_t big[kApCols] = {16, 4000, 4000, 4000, 400, 4000, 400};
    Pool p(big);
    const std::vector<int32_t> st = {PZ_ATT_PROCESSED, PZ_ATT_SLOT_LOW, PZ_ATT_PROCESSED, PZ_ATT_SLOT_LOW, PZ_ATT_PROCESSED};
    CHECK(append(p, cols, 5, st, nullptr));
    CHECK(p.err == kApErrInverted);
    Rec empty;
    empty.committee = 0xFFFFFFFFu;
    check_equal(p, {batch[0], empty, batch[4]});
  }
  // ---- the predicates and the saturation at their edges ---------------------------------------
  CHECK(ap_shard32(0xFFFFFFFEull) == 0xFFFFFFFEu && ap_shard32(0xFFFFFFFFull) == 0xFFFFFFFFu);
  CHECK(ap_shard32(0x100000000ull) == 0xFFFFFFFFu && ap_shard32(1ull << 63) == 0xFFFFFFFFu);
  CHECK(!ap_keep_prune(64, 64) && ap_keep_prune(65, 64) && !ap_keep_prune(0, 0));
  {
    const uint64_t cap[kApCols] = {1, 1, 1, 1, 1, 1, ~0ull}, base[kApCols] = {1, 0, 0, 0, 0, 0, ~0ull};
    const uint64_t none[kApCols] = {}, wrap[kApCols] = {0, 0, 0, 0, 0, 0, 1}, one[kApCols] = {0, 1, 1, 1, 1, 1, 0};
    CHECK(ap_fits(base, none, cap) && !ap_fits(base, wrap, cap) && ap_fits(base, one, cap));
  }
  std::printf("ok: %llu calls landed, %llu rolled back, %llu prunes\n", (unsigned long long)landed, (unsigned long long)rolled,
              (unsigned long long)pruned);
  return 0;
}
