// The pending-attestation pool's growth rules on the CPU, under ASan+UBSan (plain g++; no GPU code):
// attpool_dev.h -- the text pz_att_pool_move_kernel and pz_att_pool_need_kernel compile -- driven
// through a sequential form of the move (every lane of a small grid in turn, column by column) over
// buffer sets held in vectors of EXACTLY the old and the new sizes plus the bytes columns' 4 bytes of
// slack, so that one element read or written too far is ASan's; against a vector-of-records model:
// every bytes column at live lengths 0, 1, 15, 16, 17 and 33, each capacity grown alone and all
// together, random pools, reserve -> append -> prune -> reserve, and the need sums against the
// model's append at 0, 1, 255, 256, 257 and 513 rows with inverted rows among them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../attpool_dev.h"

using namespace pz;

namespace {

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

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

// The buffers in att_cols.h's order, then committee, shard32.
enum { B_SLOT, B_SHARD, B_JSLOT, B_JBH, B_JBH_OFFS, B_SBH, B_SBH_OFFS, B_BITS, B_BITS_OFFS, B_OBL, B_OBL_OFFS, B_OBL_FIRST,
       B_SIG, B_SIG_FIRST, B_COMM, B_S32 };
static_assert(B_S32 + 1 == kApSetBufs, "the pool's buffers");

constexpr uint64_t kSlack = 4;  // behind a bytes column's capacity: readable, never part of the live bytes

// A buffer set of exactly the capacities' sizes: one byte past any buffer is ASan's.
struct Set {
  std::vector<uint8_t> buf[kApSetBufs];
  uint64_t cap[kApCols];
  explicit Set(const uint64_t c[kApCols]) {
    std::memcpy(cap, c, sizeof cap);
    for (int k = 0; k < kApSetBufs; ++k) {
      const ApColRule r = ap_col_rule(k);
      buf[k].assign(ap_col_live_bytes(r, c) + (r.width == 1 ? kSlack : 0), 0xEE);
    }
  }
  uint64_t* u64(int k) { return reinterpret_cast<uint64_t*>(buf[k].data()); }
  const uint64_t* u64(int k) const { return reinterpret_cast<const uint64_t*>(buf[k].data()); }
  uint32_t* u32(int k) { return reinterpret_cast<uint32_t*>(buf[k].data()); }
  const uint32_t* u32(int k) const { return reinterpret_cast<const uint32_t*>(buf[k].data()); }
  pz_attestation_cols view() const {
    pz_attestation_cols c{};
    for (int k = 0; k < kAttNCols; ++k) att_set_in(&c, k, buf[k].data());
    return c;
  }
  bool holds(const uint64_t c[kApCols]) const {
    for (int k = 0; k < kApCols; ++k)
      if (cap[k] < c[k]) return false;
    return true;
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

void put(std::vector<uint8_t>& dst, uint64_t at, const std::vector<uint8_t>& src) {
  if (!src.empty()) std::memcpy(dst.data() + at, src.data(), src.size());
}

// The records as a buffer set sized to hold exactly them (ranges start at 0).
Set to_set(const std::vector<Rec>& v) {
  uint64_t n[kApCols];
  sizes_of(v, n);
  Set s(n);
  uint64_t at[kApCols] = {};
  for (const Rec& r : v) {
    const uint64_t i = at[0]++;
    s.u64(B_SLOT)[i] = r.slot, s.u64(B_SHARD)[i] = r.shard, s.u64(B_JSLOT)[i] = r.jslot;
    s.u32(B_COMM)[i] = r.committee, s.u32(B_S32)[i] = ap_shard32(r.shard);
    s.u64(B_JBH_OFFS)[i] = at[kApJbh], s.u64(B_SBH_OFFS)[i] = at[kApSbh], s.u64(B_BITS_OFFS)[i] = at[kApBits];
    s.u64(B_OBL_FIRST)[i] = at[kApElems], s.u64(B_SIG_FIRST)[i] = at[kApSigs];
    put(s.buf[B_JBH], at[kApJbh], r.jbh), put(s.buf[B_SBH], at[kApSbh], r.sbh), put(s.buf[B_BITS], at[kApBits], r.bits);
    at[kApJbh] += r.jbh.size(), at[kApSbh] += r.sbh.size(), at[kApBits] += r.bits.size();
    for (const auto& e : r.obl) {
      s.u64(B_OBL_OFFS)[at[kApElems]++] = at[kApElemBytes];
      put(s.buf[B_OBL], at[kApElemBytes], e);
      at[kApElemBytes] += e.size();
    }
    for (uint64_t x : r.sig) s.u64(B_SIG)[at[kApSigs]++] = x;
  }
  s.u64(B_JBH_OFFS)[at[0]] = at[kApJbh], s.u64(B_SBH_OFFS)[at[0]] = at[kApSbh], s.u64(B_BITS_OFFS)[at[0]] = at[kApBits];
  s.u64(B_OBL_FIRST)[at[0]] = at[kApElems], s.u64(B_SIG_FIRST)[at[0]] = at[kApSigs];
  s.u64(B_OBL_OFFS)[at[kApElems]] = at[kApElemBytes];
  return s;
}

std::vector<uint8_t> cut(const std::vector<uint8_t>& b, uint64_t lo, uint64_t hi) {
  return std::vector<uint8_t>(b.begin() + lo, b.begin() + hi);
}

std::vector<Rec> from_set(const Set& s, const uint64_t n[kApCols]) {
  std::vector<Rec> v(n[0]);
  for (uint64_t i = 0; i < n[0]; ++i) {
    Rec& r = v[i];
    r.slot = s.u64(B_SLOT)[i], r.shard = s.u64(B_SHARD)[i], r.jslot = s.u64(B_JSLOT)[i], r.committee = s.u32(B_COMM)[i];
    CHECK(s.u32(B_S32)[i] == ap_shard32(r.shard));
    r.jbh = cut(s.buf[B_JBH], s.u64(B_JBH_OFFS)[i], s.u64(B_JBH_OFFS)[i + 1]);
    r.sbh = cut(s.buf[B_SBH], s.u64(B_SBH_OFFS)[i], s.u64(B_SBH_OFFS)[i + 1]);
    r.bits = cut(s.buf[B_BITS], s.u64(B_BITS_OFFS)[i], s.u64(B_BITS_OFFS)[i + 1]);
    for (uint64_t e = s.u64(B_OBL_FIRST)[i]; e < s.u64(B_OBL_FIRST)[i + 1]; ++e)
      r.obl.push_back(cut(s.buf[B_OBL], s.u64(B_OBL_OFFS)[e], s.u64(B_OBL_OFFS)[e + 1]));
    r.sig.assign(s.u64(B_SIG) + s.u64(B_SIG_FIRST)[i], s.u64(B_SIG) + s.u64(B_SIG_FIRST)[i + 1]);
  }
  return v;
}

// The pool: two buffer sets (each of the capacities it was last grown to), the counts, the error word.
struct Pool {
  uint64_t cap[kApCols];
  Set set[2];
  int live = 0;
  uint64_t counts[kApCols] = {};
  uint64_t err = 0;
  explicit Pool(const uint64_t c[kApCols]) : set{Set(c), Set(c)} {
    std::memcpy(cap, c, sizeof cap);
    for (Set& s : set)  // (pz_att_pool_new's zero fill: the offsets' entry 0)
      for (int k : {B_JBH_OFFS, B_SBH_OFFS, B_BITS_OFFS, B_OBL_OFFS, B_OBL_FIRST, B_SIG_FIRST}) s.u64(k)[0] = 0;
  }
};

uint64_t g_moved_cols = 0, g_moved_bytes = 0;

// What an append of these rows would add, through 256-row tiles and their scan as the launches form it.
void need_of(const pz_attestation_cols& src, uint64_t n, const int32_t* status, const uint8_t* take, uint64_t total[kApCols],
             bool* inverted = nullptr) {
  constexpr uint64_t kTile = 256;
  const uint64_t ntiles = (n + kTile - 1) / kTile;
  std::vector<uint64_t> tiles(kApCols * (ntiles ? ntiles : 1), 0);
  for (uint64_t i = 0; i < ntiles * kTile; ++i) {  // (a lane per row of every tile: past n nothing is read)
    uint64_t sz[kApCols];
    const bool inv = ap_kept_sizes(i < n && ap_keep_append(status, take, i), src, i, sz);
    if (inv && inverted) *inverted = true;
    for (int c = 0; c < kApCols; ++c) tiles[c * ntiles + i / kTile] += sz[c];
  }
  for (int c = 0; c < kApCols; ++c) {
    total[c] = 0;
    for (uint64_t t = 0; t < ntiles; ++t) total[c] += tiles[c * ntiles + t];
  }
}

// One selection of rows of src into dst at a base, as append (status / take) or prune (lsr) make it.
bool select(Pool& p, const Set& from, uint64_t n, const int32_t* status, const uint8_t* take, bool prune, uint64_t lsr, Set& dst) {
  const pz_attestation_cols src = from.view();
  auto keep = [&](uint64_t i) { return prune ? ap_keep_prune(src.slot[i], lsr) : ap_keep_append(status, take, i); };
  uint64_t total[kApCols] = {}, base[kApCols];
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t sz[kApCols];
    if (ap_kept_sizes(keep(i), src, i, sz)) p.err |= kApErrInverted;
    for (int c = 0; c < kApCols; ++c) total[c] += sz[c];
  }
  for (int c = 0; c < kApCols; ++c) base[c] = prune ? 0 : p.counts[c];
  if (!ap_fits(base, total, p.cap)) {
    p.err |= kApErrCapacity;
    return false;
  }
  uint64_t at[kApCols];
  for (int c = 0; c < kApCols; ++c) at[c] = base[c], p.counts[c] = base[c] + total[c];
  for (uint64_t i = 0; i < n; ++i) {
    if (!keep(i)) continue;
    const ApRow r = ap_row(src, i);
    const uint64_t row = at[0];
    const bool z = r.inverted;
    dst.u64(B_SLOT)[row] = z ? 0 : src.slot[i], dst.u64(B_SHARD)[row] = z ? 0 : src.shard_id[i];
    dst.u64(B_JSLOT)[row] = z ? 0 : src.justified_slot[i];
    dst.u32(B_COMM)[row] = z ? 0xFFFFFFFFu : from.u32(B_COMM)[i];
    dst.u32(B_S32)[row] = ap_shard32(dst.u64(B_SHARD)[row]);
    dst.u64(B_JBH_OFFS)[row] = at[kApJbh], dst.u64(B_SBH_OFFS)[row] = at[kApSbh], dst.u64(B_BITS_OFFS)[row] = at[kApBits];
    dst.u64(B_OBL_FIRST)[row] = at[kApElems], dst.u64(B_SIG_FIRST)[row] = at[kApSigs];
    if (r.sz[kApJbh]) std::memcpy(dst.buf[B_JBH].data() + at[kApJbh], src.justified_block_hash + r.lo[kApJbh], r.sz[kApJbh]);
    if (r.sz[kApSbh]) std::memcpy(dst.buf[B_SBH].data() + at[kApSbh], src.shard_block_hash + r.lo[kApSbh], r.sz[kApSbh]);
    if (r.sz[kApBits]) std::memcpy(dst.buf[B_BITS].data() + at[kApBits], src.attester_bitfield + r.lo[kApBits], r.sz[kApBits]);
    for (uint64_t k = 0; k < r.sz[kApElems]; ++k)
      dst.u64(B_OBL_OFFS)[at[kApElems] + k] = at[kApElemBytes] + (src.oblique_offs[r.lo[kApElems] + k] - r.lo[kApElemBytes]);
    if (r.sz[kApElemBytes])
      std::memcpy(dst.buf[B_OBL].data() + at[kApElemBytes], src.oblique_parent_hashes + r.lo[kApElemBytes], r.sz[kApElemBytes]);
    if (r.sz[kApSigs]) std::memcpy(dst.u64(B_SIG) + at[kApSigs], src.aggregate_sig + r.lo[kApSigs], r.sz[kApSigs] * 8);
    for (int c = 0; c < kApCols; ++c) at[c] += r.sz[c];
  }
  const uint64_t* e = p.counts;
  dst.u64(B_JBH_OFFS)[e[0]] = e[kApJbh], dst.u64(B_SBH_OFFS)[e[0]] = e[kApSbh], dst.u64(B_BITS_OFFS)[e[0]] = e[kApBits];
  dst.u64(B_OBL_FIRST)[e[0]] = e[kApElems], dst.u64(B_SIG_FIRST)[e[0]] = e[kApSigs], dst.u64(B_OBL_OFFS)[e[kApElems]] = e[kApElemBytes];
  return true;
}

bool append(Pool& p, const std::vector<Rec>& batch, const std::vector<int32_t>& status, const uint8_t* take = nullptr) {
  const Set b = to_set(batch);
  return select(p, b, batch.size(), status.data(), take, false, 0, p.set[p.live]);
}

// The other set holds the pool's capacities before a prune writes into it (attpool.hip's grow_set).
void grow_other(Pool& p) {
  if (!p.set[p.live ^ 1].holds(p.cap)) p.set[p.live ^ 1] = Set(p.cap);
}

void prune(Pool& p, uint64_t lsr) {
  grow_other(p);
  CHECK(select(p, p.set[p.live], p.counts[0], nullptr, nullptr, true, lsr, p.set[p.live ^ 1]));
  p.live ^= 1;
}

// pz_[dev_]att_pool_reserve, the move lane by lane over a grid of T lanes.  Returns whether it grew.
bool reserve(Pool& p, const uint64_t min_caps[kApCols], uint64_t T) {
  uint64_t new_cap[kApCols];
  if (!ap_reserve_caps(p.cap, min_caps, new_cap)) return false;
  const int other = p.live ^ 1;
  p.set[other] = Set(new_cap);  // exactly the new sizes
  const Set& from = p.set[p.live];
  Set& to = p.set[other];
  uint64_t counts[kApCols];
  for (int c = 0; c < kApCols; ++c) counts[c] = p.counts[c] < p.cap[c] ? p.counts[c] : p.cap[c];
  for (int k = 0; k < kApSetBufs; ++k) {
    const uint64_t live = ap_col_live_bytes(ap_col_rule(k), counts);
    for (uint64_t t = 0; t < T; ++t) ap_move_lane(to.buf[k].data(), from.buf[k].data(), live, t, T);
    CHECK(live == 0 || !std::memcmp(to.buf[k].data(), from.buf[k].data(), live));
    for (uint64_t b = live; b < to.buf[k].size(); ++b) CHECK(to.buf[k][b] == 0xEE);  // nothing behind the live bytes is written
    ++g_moved_cols, g_moved_bytes += live;
  }
  p.live = other;
  std::memcpy(p.cap, new_cap, sizeof p.cap);
  return true;
}

std::mt19937_64 rng(20183);
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

void check_equal(const Pool& p, const std::vector<Rec>& model) {
  uint64_t n[kApCols];
  sizes_of(model, n);
  for (int c = 0; c < kApCols; ++c) CHECK(p.counts[c] == n[c] && p.counts[c] <= p.cap[c]);
  CHECK(from_set(p.set[p.live], p.counts) == model);
}

std::vector<int32_t> processed(uint64_t n) { return std::vector<int32_t>(n, PZ_ATT_PROCESSED); }

const uint64_t kGrids[] = {6, 64, 256};

}  // namespace

int main() {
  uint64_t reserves = 0, noops = 0, appends = 0, prunes = 0, needs = 0;
  // ---- every column's rule: what the table says, restated by hand once as the check ---------------
  {
    const uint64_t n[kApCols] = {10, 20, 30, 40, 50, 60, 70};
    const uint64_t want[kApSetBufs] = {80, 80, 80, 20, 88, 30, 88, 40, 88, 60, 408, 88, 560, 88, 40, 40};
    for (int k = 0; k < kApSetBufs; ++k) CHECK(ap_col_live_bytes(ap_col_rule(k), n) == want[k]);
  }
  // ---- a reserve's capacities ---------------------------------------------------------------------
  {
    const uint64_t cap[kApCols] = {4, 5, 6, 7, 8, 9, 10}, below[kApCols] = {0, 5, 1, 7, 0, 9, 10}, one[kApCols] = {0, 0, 0, 8, 0, 0, 0};
    uint64_t out[kApCols];
    CHECK(!ap_reserve_caps(cap, cap, out) && !std::memcmp(out, cap, sizeof out));
    CHECK(!ap_reserve_caps(cap, below, out) && !std::memcmp(out, cap, sizeof out));
    CHECK(ap_reserve_caps(cap, one, out) && out[kApBits] == 8 && out[0] == 4 && out[kApSigs] == 10);
  }
  // ---- every bytes column at live lengths 0, 1, 15, 16, 17, 33; each capacity alone, then all --------
  for (uint64_t len : {0, 1, 15, 16, 17, 33})
    for (uint64_t rows : {1, 2, 3, 5})  // (the u32 columns' tails: 4, 8, 12 and 16 + 4 bytes)
      for (int grow = 0; grow <= kApCols; ++grow)
        for (uint64_t T : kGrids) {
          std::vector<Rec> model(rows);
          for (Rec& r : model) r = random_rec(), r.jbh.clear(), r.sbh.clear(), r.bits.clear(), r.obl.clear(), r.sig.clear();
          Rec& r0 = model[0];  // the whole column's live bytes are row 0's
          r0.jbh = blob(len), r0.sbh = blob(len), r0.bits = blob(len), r0.obl = {blob(len)};
          if (len & 1) r0.sig = {rng(), rng()};
          uint64_t cap[kApCols];
          sizes_of(model, cap);  // full in every capacity
          Pool p(cap);
          CHECK(append(p, model, processed(rows)));
          ++appends;
          uint64_t min_caps[kApCols] = {};
          for (int c = 0; c < kApCols; ++c)
            if (grow == kApCols || grow == c) min_caps[c] = cap[c] + 1 + rnd(40);
          CHECK(reserve(p, min_caps, T));
          ++reserves;
          for (int c = 0; c < kApCols; ++c) CHECK(p.cap[c] == (min_caps[c] > cap[c] ? min_caps[c] : cap[c]));
          check_equal(p, model);
          CHECK(!reserve(p, min_caps, T) && !reserve(p, cap, T));  // equal and below: nothing to do
          noops += 2;
        }
  // ---- the empty pool -----------------------------------------------------------------------------
  for (uint64_t T : kGrids) {
    const uint64_t cap[kApCols] = {1, 0, 0, 0, 0, 0, 0}, more[kApCols] = {3, 1, 1, 1, 1, 1, 1};
    Pool p(cap);
    CHECK(reserve(p, more, T));
    ++reserves;
    check_equal(p, {});
    std::vector<Rec> one = {random_rec()};
    one[0].jbh = blob(1), one[0].sbh = blob(1), one[0].bits = blob(1), one[0].obl = {blob(1)}, one[0].sig = {7};
    CHECK(append(p, one, processed(1)));
    ++appends;
    check_equal(p, one);
  }
  // ---- random pools: reserve, the append that did not fit, prune, reserve again -------------------------
  for (int round = 0; round < 120; ++round) {
    const uint64_t T = kGrids[rnd(3)];
    std::vector<Rec> model(rnd(4) ? 1 + rnd(60) : 0), more(1 + rnd(20));
    for (Rec& r : model) r = random_rec();
    for (Rec& r : more) r = random_rec();
    Rec& last = more.back();  // every size of the second batch is non-zero
    last.jbh = blob(32), last.sbh = blob(32), last.bits = blob(5), last.obl = {blob(3), blob(0)}, last.sig = {1, 2};
    uint64_t cap[kApCols], add[kApCols];
    sizes_of(model, cap);
    sizes_of(more, add);
    const int c = (int)rnd(kApCols);  // room for `more` everywhere but in capacity c
    for (int k = 0; k < kApCols; ++k) cap[k] += k == c ? add[k] - 1 : add[k] + rnd(9);
    if (cap[0] == 0) cap[0] = 1;
    Pool p(cap);
    CHECK(append(p, model, processed(model.size())));
    const bool fits0 = c == 0 && model.empty() && add[0] == 1;  // (the row capacity's floor of 1 made room)
    if (!fits0) {
      CHECK(!append(p, more, processed(more.size())));
      CHECK(p.err == kApErrCapacity);
      check_equal(p, model);
    }
    const uint64_t err = p.err;
    uint64_t min_caps[kApCols] = {};
    min_caps[c] = cap[c] + 1;  // exactly what is short
    if (reserve(p, min_caps, T)) ++reserves;
    CHECK(p.err == err);  // the sticky word is carried over
    check_equal(p, model);
    if (!fits0) {
      CHECK(append(p, more, processed(more.size())));
      model.insert(model.end(), more.begin(), more.end());
    }
    ++appends;
    check_equal(p, model);
    const uint64_t lsr = rnd(220);
    prune(p, lsr);  // into the set the reserve left behind: it grows first
    ++prunes;
    std::vector<Rec> kept;
    for (const Rec& r : model)
      if (r.slot > lsr) kept.push_back(r);
    model.swap(kept);
    check_equal(p, model);
    uint64_t twice[kApCols];
    for (int k = 0; k < kApCols; ++k) twice[k] = rnd(2) ? 2 * p.cap[k] + 1 : 0;
    if (reserve(p, twice, T)) ++reserves;
    check_equal(p, model);
    std::vector<Rec> tail(rnd(6));
    for (Rec& r : tail) r = random_rec(), r.obl.clear(), r.sig.clear(), r.jbh = blob(1), r.sbh = blob(1), r.bits = blob(1);
    if (append(p, tail, processed(tail.size()))) model.insert(model.end(), tail.begin(), tail.end()), ++appends;
    check_equal(p, model);
  }
  // ---- the need sums against the model's append -----------------------------------------------------
  static const int32_t kStatuses[] = {PZ_ATT_PROCESSED, PZ_ATT_NOT_PROCESSED, PZ_ATT_SLOT_HIGH, PZ_ATT_SLOT_LOW, PZ_EINVAL};
  for (uint64_t n : {0, 1, 255, 256, 257, 513})
    for (int form = 0; form < 4; ++form) {  // no take, a take, a take of zeros, inverted rows among them
      std::vector<Rec> batch(n);
      for (Rec& r : batch) r = random_rec(), r.bits = blob(1 + rnd(9)), r.obl = {blob(4)};
      std::vector<int32_t> status(n);
      std::vector<uint8_t> take(n);
      for (uint64_t i = 0; i < n; ++i) status[i] = rnd(3) ? PZ_ATT_PROCESSED : kStatuses[rnd(5)], take[i] = form == 2 ? 0 : rnd(2);
      Set cols = to_set(batch);
      uint64_t ninv = 0;
      if (form == 3)
        for (uint64_t i = 0; i + 2 < n; i += 1 + rnd(40)) {  // row i inverted; its neighbours change length
          std::swap(cols.u64(B_BITS_OFFS)[i + 1], cols.u64(B_BITS_OFFS)[i + 2]);
          i += 2, ++ninv;
        }
      const uint8_t* tk = form == 0 ? nullptr : take.data();
      uint64_t need[kApCols];
      bool inverted = false;
      need_of(cols.view(), n, status.data(), tk, need, &inverted);
      ++needs;
      // the model's append: into a pool with room for every row of the batch, from a non-zero base
      uint64_t cap[kApCols];
      sizes_of(batch, cap);
      std::vector<Rec> base = {random_rec(), random_rec()};
      uint64_t nb[kApCols];
      sizes_of(base, nb);
      for (int c = 0; c < kApCols; ++c) cap[c] += nb[c];
      Pool p(cap);
      CHECK(append(p, base, processed(2)));
      uint64_t before[kApCols];
      std::memcpy(before, p.counts, sizeof before);
      CHECK(select(p, cols, n, status.data(), tk, false, 0, p.set[p.live]));
      ++appends;
      for (int c = 0; c < kApCols; ++c) CHECK(need[c] == p.counts[c] - before[c]);
      CHECK(inverted == ((p.err & kApErrInverted) != 0));
      if (form == 2) CHECK(need[0] == 0);
      if (form == 3 && n >= 255) CHECK(ninv > 0);
      // and exactly the need is what a pool must have left: one less in any column that adds refuses it
      for (int c = 0; c < kApCols; ++c) {
        if (need[c] == 0) continue;
        uint64_t tight[kApCols];
        for (int k = 0; k < kApCols; ++k) tight[k] = nb[k] + need[k] - (k == c);
        Pool q(tight);
        CHECK(append(q, base, processed(2)));
        CHECK(!select(q, cols, n, status.data(), tk, false, 0, q.set[q.live]));
        uint64_t exact[kApCols] = {};
        exact[c] = tight[c] + 1;
        CHECK(reserve(q, exact, kGrids[c % 3]));
        ++reserves;
        CHECK(select(q, cols, n, status.data(), tk, false, 0, q.set[q.live]));
        ++appends;
        for (int k = 0; k < kApCols; ++k) CHECK(q.counts[k] == q.cap[k]);  // full, to the element
      }
    }
  std::printf("ok: %llu reserves, %llu no-ops, %llu columns moved, %llu bytes moved, %llu appends, %llu prunes, %llu need batches\n",
              (unsigned long long)reserves, (unsigned long long)noops, (unsigned long long)g_moved_cols,
              (unsigned long long)g_moved_bytes, (unsigned long long)appends, (unsigned long long)prunes, (unsigned long long)needs);
  return 0;
}
