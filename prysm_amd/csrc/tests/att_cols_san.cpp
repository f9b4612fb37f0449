// The attestation column table and the one staging rule (att_cols.h) on the CPU, under ASan+UBSan
// (plain g++; no GPU code): stage_att_cols -- the text the host-pointer entry points compile --
// driven by an uploader that copies into heap blocks of exactly the bytes asked for, over column
// sets held in vectors of exactly their sizes.  For every row, the bytes seen through the staged
// (data, offsets) must be the bytes seen through the caller's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../att_cols.h"

using namespace pz;

namespace {

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// ---- the table against the structs -------------------------------------------------------------
#define MEMBERS(X)                                                                                              \
  X(0, slot) X(1, shard_id) X(2, justified_slot) X(3, justified_block_hash) X(4, justified_block_hash_offs)     \
  X(5, shard_block_hash) X(6, shard_block_hash_offs) X(7, attester_bitfield) X(8, attester_bitfield_offs)       \
  X(9, oblique_parent_hashes) X(10, oblique_offs) X(11, oblique_first) X(12, aggregate_sig) X(13, aggregate_sig_first)
#define CHECK_MEMBER(k, m)                                                                                 \
  static_assert(kAttTable[k].in_off == offsetof(pz_attestation_cols, m), #m);                              \
  static_assert(kAttTable[k].out_off == offsetof(pz_attestation_cols_out, m), #m);                         \
  static_assert(kAttTable[k].in_off == k * sizeof(void*) && kAttTable[k].out_off == k * sizeof(void*), #m); \
  static_assert(kAttTable[k].width == sizeof(*pz_attestation_cols{}.m), #m);                               \
  static_assert(kAttTable[k].width == sizeof(*pz_attestation_cols_out{}.m), #m);
MEMBERS(CHECK_MEMBER)
static_assert(sizeof(pz_attestation_cols) == kAttNCols * sizeof(void*), "the table names every member");
static_assert(offsetof(pz_attestation_cols_out, n_oblique) == kAttNCols * sizeof(void*), "out's columns come first");

// the named groups: each ranges pair is a data column and its per-row offsets, by member
#define COL(m) int(offsetof(pz_attestation_cols, m) / sizeof(void*))
static_assert(kAttRanges[0][0] == COL(justified_block_hash) && kAttRanges[0][1] == COL(justified_block_hash_offs), "");
static_assert(kAttRanges[1][0] == COL(shard_block_hash) && kAttRanges[1][1] == COL(shard_block_hash_offs), "");
static_assert(kAttRanges[2][0] == COL(attester_bitfield) && kAttRanges[2][1] == COL(attester_bitfield_offs), "");
static_assert(kAttRanges[3][0] == COL(aggregate_sig) && kAttRanges[3][1] == COL(aggregate_sig_first), "");
static_assert(kColObl == COL(oblique_parent_hashes) && kColOblOffs == COL(oblique_offs) && kColOblFirst == COL(oblique_first), "");
static_assert(kAttKeyCols == (1u << COL(slot) | 1u << COL(shard_id) | 1u << COL(shard_block_hash_offs) | 1u << COL(oblique_first)), "");
static_assert(kAttBitsCols == 1u << COL(attester_bitfield_offs) && kAttObliqueCols == 1u << COL(oblique_first), "");
static_assert(kAttAllCols == (1u << 14) - 1 && kAttNCols == 14, "");

void check_table() {
  for (const auto& r : kAttRanges)  // a data column governed by a total, an offsets column by the rows + 1
    REQUIRE(kAttTable[r[0]].total >= 0 && !kAttTable[r[0]].plus && kAttTable[r[1]].total < 0 && kAttTable[r[1]].plus == 1);
  const uint64_t totals[kAttTotals] = {11, 12, 13, 4, 15, 6};  // jbh, sbh, bits, elements, element bytes, sigs
  const uint64_t want[kAttNCols] = {5, 5, 5, 11, 6, 12, 6, 13, 6, 15, 5, 6, 6, 6};
  for (int k = 0; k < kAttNCols; ++k) REQUIRE(att_col_len(kAttTable[k], 5, totals) == want[k]);
  const char* const names[kAttTotals] = {"justified_block_hash", "shard_block_hash", "attester_bitfield",
                                         "oblique elements",     "oblique bytes",    "aggregate_sig"};
  for (int t = 0; t < kAttTotals; ++t) REQUIRE(std::string(att_total_name(t)) == names[t]);
  pz_attestation_cols c{};
  pz_attestation_cols_out o{};
  static uint64_t mark[kAttNCols];
  for (int k = 0; k < kAttNCols; ++k) {
    att_set_in(&c, k, mark + k), att_set_out(&o, k, mark + k);
    REQUIRE(att_in(c, k) == mark + k && att_out(o, k) == mark + k);
  }
  REQUIRE(c.slot == mark && c.aggregate_sig_first == mark + 13 && o.oblique_offs == mark + 10);
}

// ---- the uploader --------------------------------------------------------------------------------
struct MemUp {
  int rc = 0;
  std::deque<std::unique_ptr<uint8_t[]>> blocks;
  std::deque<std::vector<uint64_t>> kept;
  uint64_t bytes_up = 0;
  void* put(const void* host, size_t bytes) {
    blocks.emplace_back(new uint8_t[bytes]);
    if (host && bytes) std::memcpy(blocks.back().get(), host, bytes);
    bytes_up += bytes;
    return blocks.back().get();
  }
  std::vector<uint64_t>& keep() { return kept.emplace_back(); }
};

// ---- a column set in vectors of exactly its sizes ---------------------------------------------------
struct Rec {
  uint64_t slot, shard, jslot;
  std::vector<uint8_t> jbh, sbh, bits;
  std::vector<std::vector<uint8_t>> obl;
  std::vector<uint64_t> sig;
};

struct Cols {
  uint64_t n = 0;
  std::vector<uint64_t> slot, shard, jslot, offs[4], obl_offs, obl_first, sig;
  std::vector<uint8_t> dat[3], obl;
  pz_attestation_cols view() const {
    pz_attestation_cols c{};
    c.slot = slot.data(), c.shard_id = shard.data(), c.justified_slot = jslot.data();
    c.justified_block_hash = dat[0].data(), c.justified_block_hash_offs = offs[0].data();
    c.shard_block_hash = dat[1].data(), c.shard_block_hash_offs = offs[1].data();
    c.attester_bitfield = dat[2].data(), c.attester_bitfield_offs = offs[2].data();
    c.oblique_parent_hashes = obl.data(), c.oblique_offs = obl_offs.data(), c.oblique_first = obl_first.data();
    c.aggregate_sig = sig.data(), c.aggregate_sig_first = offs[3].data();
    return c;
  }
};

// base[0..2]: bytes before the first range of a bytes column; base[3]: sig values, base[4]: elements
// and base[5]: element bytes before the first ones the rows name.
Cols build(const std::vector<Rec>& recs, const uint64_t base[6]) {
  Cols c;
  c.n = recs.size();
  for (int k = 0; k < 3; ++k) c.dat[k].assign(base[k], 0xEE), c.offs[k].push_back(base[k]);
  c.sig.assign(base[3], 0xEEEE), c.offs[3].push_back(base[3]);
  c.obl.assign(base[5], 0xEE);
  for (uint64_t e = 0; e < base[4]; ++e) c.obl_offs.push_back(0);  // elements no row names
  c.obl_offs.push_back(base[5]);
  c.obl_first.push_back(base[4]);
  for (const Rec& r : recs) {
    c.slot.push_back(r.slot), c.shard.push_back(r.shard), c.jslot.push_back(r.jslot);
    const std::vector<uint8_t>* b[3] = {&r.jbh, &r.sbh, &r.bits};
    for (int k = 0; k < 3; ++k) c.dat[k].insert(c.dat[k].end(), b[k]->begin(), b[k]->end()), c.offs[k].push_back(c.dat[k].size());
    c.sig.insert(c.sig.end(), r.sig.begin(), r.sig.end()), c.offs[3].push_back(c.sig.size());
    for (const auto& e : r.obl) c.obl.insert(c.obl.end(), e.begin(), e.end()), c.obl_offs.push_back(c.obl.size());
    c.obl_first.push_back(c.obl_offs.size() - 1);
  }
  return c;
}

// What row i shows through a column set: one string a column ("-": a NULL column, "!": an inverted range).
std::string bytes_of(const void* data, uint64_t lo, uint64_t hi, uint64_t w) {
  if (hi < lo) return "!";
  return "[" + std::string(static_cast<const char*>(data) + lo * w, (hi - lo) * w) + "]";
}
std::vector<std::string> row_view(const pz_attestation_cols& c, uint64_t i) {
  std::vector<std::string> v;
  for (int k = 0; k < 3; ++k) {
    const uint64_t* s = static_cast<const uint64_t*>(att_in(c, k));
    v.push_back(s ? std::to_string(s[i]) : "-");
  }
  for (const auto& r : kAttRanges) {
    const uint64_t* o = static_cast<const uint64_t*>(att_in(c, r[1]));
    v.push_back(o ? bytes_of(att_in(c, r[0]), o[i], o[i + 1], kAttTable[r[0]].width) : "-");
  }
  if (!c.oblique_first) {
    v.push_back("-");
  } else if (c.oblique_first[i + 1] < c.oblique_first[i]) {
    v.push_back("!");
  } else {
    std::string s = "{";
    for (uint64_t e = c.oblique_first[i]; e < c.oblique_first[i + 1]; ++e)
      s += bytes_of(c.oblique_parent_hashes, c.oblique_offs[e], c.oblique_offs[e + 1], 1);
    v.push_back(s + "}");
  }
  return v;
}

uint64_t g_cases = 0;

// Stages `which` of host and checks every row, the NULL rules and (monotone sets) what was uploaded.
void check_staged(const pz_attestation_cols& host, uint64_t n, uint32_t which, const uint64_t* want_staged = nullptr) {
  MemUp up;
  pz_attestation_cols dev;
  uint64_t staged[kAttTotals];
  REQUIRE(stage_att_cols(up, host, n, which, &dev, staged) == 0);
  pz_attestation_cols expect = host;  // the columns the call reads: the others must come back NULL
  for (int k = 0; k < 3; ++k)
    if (!(which & (1u << k))) att_set_in(&expect, k, nullptr);
  for (const auto& r : kAttRanges)
    if (!(which & (1u << r[1])) || !att_in(host, r[1])) att_set_in(&expect, r[0], nullptr), att_set_in(&expect, r[1], nullptr);
  if (!(which & kAttObliqueCols) || !host.oblique_first)
    expect.oblique_parent_hashes = nullptr, expect.oblique_offs = nullptr, expect.oblique_first = nullptr;
  for (int k = 0; k < kAttNCols; ++k) {  // (a data column is staged with its offsets, also when it holds no byte)
    int governs = k >= kColObl && k <= kColOblFirst ? kColOblFirst : k;
    for (const auto& r : kAttRanges)
      if (k == r[0]) governs = r[1];
    REQUIRE((att_in(dev, k) != nullptr) == (att_in(expect, governs) != nullptr));
  }
  for (uint64_t i = 0; i < n; ++i) REQUIRE(row_view(dev, i) == row_view(expect, i));
  if (want_staged)
    for (int t = 0; t < kAttTotals; ++t) REQUIRE(staged[t] == want_staged[t]);
  ++g_cases;
}

Rec random_rec(std::mt19937_64& g) {
  auto bytes = [&](uint64_t max) {
    std::vector<uint8_t> b(g() % (max + 1));
    for (auto& x : b) x = (uint8_t)g();
    return b;
  };
  Rec r{g(), g() % 1024, g(), bytes(5), bytes(5), bytes(5), {}, {}};
  for (uint64_t e = g() % 4; e > 0; --e) r.obl.push_back(bytes(4));
  for (uint64_t s = g() % 4; s > 0; --s) r.sig.push_back(g());
  return r;
}

// What a monotone set uploads: the rows' own bytes, elements and values, whatever lies before them.
void totals_of(const std::vector<Rec>& recs, uint64_t t[kAttTotals]) {
  std::memset(t, 0, kAttTotals * 8);
  for (const Rec& r : recs) {
    t[kTotJbh] += r.jbh.size(), t[kTotSbh] += r.sbh.size(), t[kTotBits] += r.bits.size();
    t[kTotElems] += r.obl.size(), t[kTotSigs] += r.sig.size();
    for (const auto& e : r.obl) t[kTotElemBytes] += e.size();
  }
}

// Every NULL combination an entry point allows: any scalar, any offsets column (its data NULL or not).
void check_null_combinations(const Cols& c, uint32_t which) {
  for (uint32_t m = 0; m < (1u << 8); ++m) {
    pz_attestation_cols h = c.view();
    for (int k = 0; k < 3; ++k)
      if (m & (1u << k)) att_set_in(&h, k, nullptr);
    for (int q = 0; q < 4; ++q)
      if (m & (8u << q)) {
        att_set_in(&h, kAttRanges[q][1], nullptr);
        if (m & 1) att_set_in(&h, kAttRanges[q][0], nullptr);
      }
    if (m & 128u) {
      h.oblique_first = nullptr;
      if (m & 2) h.oblique_offs = nullptr, h.oblique_parent_hashes = nullptr;
    }
    check_staged(h, c.n, which);
  }
}

}  // namespace

int main() {
  check_table();
  std::mt19937_64 g(20181101);
  const uint64_t zero[6] = {0, 0, 0, 0, 0, 0}, off[6] = {7, 3, 9, 2, 3, 5};
  const uint32_t subsets[4] = {kAttAllCols, kAttKeyCols, kAttObliqueCols | kAttBitsCols, kAttBitsCols};

  // five records: two oblique elements, an empty bitfield, a signature; zero, one and several elements
  std::vector<Rec> five;
  for (int i = 0; i < 5; ++i) five.push_back(random_rec(g));
  five[0].jbh = {1}, five[0].sbh = {2, 3}, five[0].bits = {0x80}, five[0].sig = {7, 8};
  five[0].obl = {{1, 2, 3}, {4}};
  five[1].bits.clear(), five[1].obl.clear();
  five[2].sig = {42}, five[2].obl = {{9, 9}};
  five[3].obl = {{}, {5, 6}, {}, {7}};
  five[4].jbh = {9}, five[4].sbh = {8}, five[4].bits = {7}, five[4].sig = {5}, five[4].obl = {{6}};
  uint64_t want[kAttTotals];
  totals_of(five, want);
  for (const uint64_t* base : {zero, off}) {  // monotone offsets from 0 and from a non-zero base
    const Cols c = build(five, base);
    for (uint32_t w : subsets) check_staged(c.view(), c.n, w, w == kAttAllCols ? want : nullptr);
    check_null_combinations(c, kAttAllCols);
  }
  // an inverted range among valid ones: the first and the last row of each ranges column (the
  // largest offset is then not the last one), then the first and the last element
  for (int q = 0; q < 6; ++q)
    for (const uint64_t row : {uint64_t(0), uint64_t(4)}) {
      Cols c = build(five, off);
      std::vector<uint64_t>& o = q < 4 ? c.offs[q] : q == 4 ? c.obl_first : c.obl_offs;
      const size_t at = q < 5 ? row : row ? o.size() - 2 : c.obl_first[0];
      REQUIRE(o[at] < o[at + 1]);
      std::swap(o[at], o[at + 1]);  // (both ends stay inside the span the rows name)
      REQUIRE(row_view(c.view(), row)[q < 4 ? 3 + q : 7].find('!') != std::string::npos);
      check_staged(c.view(), c.n, kAttAllCols);
    }
  {  // empty columns: every range empty, the data vectors empty; then n = 0
    std::vector<Rec> e(3, Rec{1, 2, 3, {}, {}, {}, {}, {}});
    const Cols c = build(e, zero);
    uint64_t none[kAttTotals] = {};
    check_staged(c.view(), c.n, kAttAllCols, none);
    check_null_combinations(c, kAttAllCols);
    for (const uint64_t* base : {zero, off}) {
      const Cols z = build({}, base);
      for (uint32_t w : subsets) check_staged(z.view(), 0, w, none);
    }
  }
  for (int t = 0; t < 240; ++t) {  // random column sets of up to 8 rows
    std::vector<Rec> recs(g() % 9);
    for (Rec& r : recs) r = random_rec(g);
    uint64_t base[6];
    for (uint64_t& b : base) b = g() % 8;
    Cols c = build(recs, base);
    totals_of(recs, want);
    pz_attestation_cols h = c.view();
    check_staged(h, c.n, kAttAllCols, want);
    for (int k = 0; k < kAttNCols; ++k)  // random NULLs (a data column only with its offsets)
      if (g() % 4 == 0 && kAttTable[k].total < 0) att_set_in(&h, k, nullptr);
    check_staged(h, c.n, subsets[g() % 4]);
    if (c.n >= 2) {  // and an inverted row among them (the last one too), as the pool receives it
      std::vector<uint64_t>& o = c.offs[g() % 4];
      const size_t at = 1 + g() % c.n;
      std::swap(o[at - 1], o[at]);
      check_staged(c.view(), c.n, kAttAllCols);
    }
  }
  std::printf("ok: %llu cases\n", (unsigned long long)g_cases);
  return 0;
}
